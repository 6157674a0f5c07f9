"""Shared helpers of the parity tests: the same numpy cell arrays feed the oracle (CPU) and the
HIP path (uploaded to HBM), and results are compared bit for bit."""
from __future__ import annotations

import struct
import zlib

import numpy as np

from amrvolumerenderer_amd import runtime, scenes
from amrvolumerenderer_amd.types import (AmrBox, CameraParameters, ScalarTransform, VolumeBounds,
                                         make_params)


def bits(a: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_bit_equal(got: np.ndarray, want: np.ndarray, what: str = "") -> None:
    got = np.ascontiguousarray(got, dtype=np.float32).reshape(-1)
    want = np.ascontiguousarray(want, dtype=np.float32).reshape(-1)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.nonzero(got.view(np.uint32) != want.view(np.uint32))[0]
    if bad.size:
        i = int(bad[0])
        raise AssertionError(
            f"{what}: {bad.size} of {got.size} floats differ; first at {i} "
            f"(pixel {i // 5}, comp {i % 5}): got {got[i]!r} want {want[i]!r}")


def oracle_camera(O, cam: CameraParameters):
    return O.make_camera(cam.eye, cam.look_at, cam.up, cam.fov_y_degrees, cam.near_plane,
                         cam.far_plane)


def oracle_transform(O, tr: ScalarTransform):
    return O.make_transform(tr.log_scale_input, tr.normalize_to_unit_range, tr.positive_floor,
                            tr.normalization_min, tr.inverse_normalization_span)


def oracle_params(O, width, height, scalar_range, box_transparency, ref_dist,
                  bounds: VolumeBounds, color_map=None):
    return O.make_params(width, height, scalar_range, box_transparency, ref_dist,
                         bounds.min_corner, bounds.max_corner, color_map)


def device_box(ctx, cells: np.ndarray, min_corner, max_corner, level=0, owner=0) -> AmrBox:
    import torch
    t = torch.from_numpy(np.ascontiguousarray(cells)).to(ctx.device)
    return AmrBox(tuple(min_corner), tuple(max_corner), t, level=level, owner=owner)


def scene_cells(spec):
    return [scenes.box_cells_numpy(spec, i) for i in range(len(spec.boxes))]


def free_port() -> int:
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def spawn_ranks(worker, nprocs: int, args_for_port) -> None:
    """torch.multiprocessing.spawn with a rendezvous port probed here.  Between the probe and rank
    0's bind the kernel may hand the port to somebody else (EADDRINUSE: seen once in some thirty
    runs of the suite); that attempt has queued nothing yet and is made again on another port."""
    import torch.multiprocessing as mp
    for attempt in range(4):
        try:
            mp.spawn(worker, args=args_for_port(free_port()), nprocs=nprocs, join=True)
            return
        except Exception as error:   # (mp.ProcessRaisedException carries the rank's traceback as text)
            if "EADDRINUSE" not in str(error) or attempt == 3:
                raise


# ---- reading sample counts out of the oracle's volume march ------------------------------------

SAMPLING_BOUNDS = VolumeBounds((-0.05,) * 3, (1.05,) * 3)
INDICATOR_MAP = [(0.0, 0.5, 0.5, 0.5, 0.0), (1.0, 0.5, 0.5, 0.5, 0.002)]
_RECURRENCES = {}


def count_samples(O, indicator, minc, maxc, cam, width, height, ref_dist, box):
    """m(p): the number of samples per pixel on cells of value 1 (tests/test_projection_gpu.py, module docstring), and the
    oracle's fetch count."""
    params = make_params(width, height, (0.0, 1.0), 0.0, ref_dist, SAMPLING_BOUNDS, INDICATOR_MAP)
    _, factor, alpha_scale = runtime.box_sampling(box, params)
    table = O.build_color_table(alpha_scale, factor, (0.0, 1.0), INDICATOR_MAP).reshape(256, 4)
    assert table[0, 3] == 0.0
    w = np.float32(table[255, 3])
    assert 0.0 < w < 0.01
    ob = O.make_box(np.ascontiguousarray(indicator, dtype=np.float64), minc, maxc)
    op = oracle_params(O, width, height, (0.0, 1.0), 0.0, ref_dist, SAMPLING_BOUNDS, INDICATOR_MAP)
    img, fetches = O.paint_box(ob, oracle_transform(O, ScalarTransform(normalize_to_unit_range=True)), op, oracle_camera(O, cam), threads=16)
    alpha = img[..., 3].astype(np.float32)
    # the recurrence's values, as far as the image needs them (strictly increasing: checked)
    a, top = np.float32(0.0), alpha.max()
    alphas = _RECURRENCES.setdefault(w.tobytes(), ([a], {a.tobytes(): 0}))
    values, index = alphas
    while values[-1] < top:
        a = values[-1]
        b = np.float32(a + np.float32(w * np.float32(np.float32(1.0) - a)))
        assert b > a and b < 1.0
        index[b.tobytes()] = len(values)
        values.append(b)
    m = np.array([index[v.tobytes()] for v in alpha.reshape(-1)], dtype=np.int64)
    return m.reshape(height, width), fetches


# ---- step maps: reading maximum indices out of the oracle's volume march -----------------------

def step_map(t, scalar_range=(0.0, 1.0)):
    """Colour map (value, r, g, b, alpha) whose table alpha is 0 for entries < t, > 0 from t on."""
    lo, hi = float(scalar_range[0]), float(scalar_range[1])
    at = lambda i: lo + (hi - lo) * i / 255.0  # noqa: E731
    if t <= 0:
        return [(lo, 0.5, 0.5, 0.5, 1.0), (hi, 0.5, 0.5, 0.5, 1.0)]
    points = [(lo, 0.5, 0.5, 0.5, 0.0), (at(t - 0.5), 0.5, 0.5, 0.5, 0.0)]
    if t < 255:
        points.append((at(t), 0.5, 0.5, 0.5, 1.0))
    points.append((hi, 0.5, 0.5, 0.5, 1.0))
    return points


_checked_tables = set()


def check_step_table(O, t, scalar_range):
    """Opacity nodes interpolate: the alpha > 0 set of the step map's table must be {i >= t}."""
    key = (t, tuple(scalar_range))
    if key in _checked_tables:
        return
    for factor in (1.0, 0.5, 0.25, 2.0):
        table = O.build_color_table(1.0, factor, scalar_range, step_map(t, scalar_range))
        lit = np.nonzero(table.reshape(256, 4)[:, 3] > 0.0)[0]
        assert np.array_equal(lit, np.arange(t, 256)), (t, factor, lit[:4])
    _checked_tables.add(key)


# ---- pictures ----------------------------------------------------------------------------------

def read_png(path):
    raw = open(path, "rb").read()
    assert raw[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, width, height = 8, b"", 0, 0
    while pos < len(raw):
        size, tag = struct.unpack(">I4s", raw[pos:pos + 8])
        body = raw[pos + 8:pos + 8 + size]
        if tag == b"IHDR":
            width, height = struct.unpack(">II", body[:8])
        elif tag == b"IDAT":
            idat += body
        pos += 12 + size
    rows = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(height, 1 + 3 * width)
    assert not rows[:, 0].any()   # filter type 0
    return rows[:, 1:].reshape(height, width, 3)


def colorize(q, lo, hi, table, eligible=None):
    """numpy restatement of avr_projection_colorize (every sampled pixel here has q > 0)."""
    if eligible is None:
        eligible = q > 0.0
    t = np.floor((q - lo) / (hi - lo) * 255.0)
    entry = np.clip(np.where(eligible, t, 0), 0, 255).astype(np.int64)
    rgb = table[entry]
    rgb[~eligible] = 0
    return rgb[::-1]
