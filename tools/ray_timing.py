"""Ray timing on config-4 (176 boxes of 128^3, three levels, 2.95 GB of cells), one rank: 2^16 rays,
the pixels of a 256 x 256 orthographic view along (1, 0.7, 0.4) across the whole domain, through
the field f = 1 + x y + z evaluated at the cell centres.  A call pair is what api.ray_scene makes:
the count pass, torch.cumsum and the read of the total, the emit pass.  --warmup pairs first, then
--frames, each call timed with events on the context's stream and waited for under its own time
limit (--limit seconds; a call that is not done by then ends the tool with status 3 and nothing
more is launched).  Segments per second counts the segments of one pair over the pair's time.  The
kernel does not report its trips, so trips per ray come from the reference
(tests/ray_reference.py) on 64 of the same rays over the same hierarchy described by rules instead
of arrays, whose segments must be the device's by bits: that is reported too.  One JSON line is
printed.

Needs a HIP device: fails loudly without one."""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N0, LEVELS, BOX = 512, 3, 128
IMAGE = 256
VIEW = (1.0, 0.7, 0.4)
REFERENCE_RAYS = 64
FIELD = lambda x, y, z: 1.0 + x * y + z


def rays():
    """(start, end) [IMAGE^2, 3]: parallel segments of length 2 along VIEW through the pixel
    centres of a square of side sqrt(3), the domain's diagonal, around its centre."""
    import numpy as np
    w = np.array(VIEW) / math.sqrt(sum(v * v for v in VIEW))
    u = np.cross(w, [0.0, 0.0, 1.0])
    u /= np.sqrt((u * u).sum())
    v = np.cross(u, w)
    side = math.sqrt(3.0)
    f = ((np.arange(IMAGE) + 0.5) / IMAGE - 0.5) * side
    py, px = np.meshgrid(f, f, indexing="ij")
    centre = 0.5 + px.reshape(-1, 1) * u[None, :] + py.reshape(-1, 1) * v[None, :]
    return np.ascontiguousarray(centre - w[None, :]), np.ascontiguousarray(centre + w[None, :])


class _Rule:
    """What the reference indexes like a level's array, answered from the cell's indices."""

    def __init__(self, shape, answer):
        self.shape, self.answer = shape, answer

    def __getitem__(self, at):
        return self.answer(*at)


def rule_hierarchy():
    """tests/ray_reference.Hierarchy over config-4 without its 2048^3 arrays: the leaves of
    scenes.make_amr_scene (every level a cube of N0 cells, its centred half covered by the next)
    and the field at the cell centres."""
    import ray_reference as rr
    h = rr.Hierarchy.__new__(rr.Hierarchy)
    h.max_level, h.n_levels, h.ratio = LEVELS - 1, LEVELS, [2] * (LEVELS - 1)
    h.prob_lo = [0.0, 0.0, 0.0]
    h.blo, h.bhi = [0, 0, 0], [N0 - 1] * 3
    h.origin, h.mask, h.values, h.dx = [], [], [], []
    first = 0
    for level in range(LEVELS):
        if level > 0:
            first = (first + N0 // 4) * 2
        n = N0 << level

        def leaf(k, j, i, first=first, level=level):
            rel = [v - first for v in (i, j, k)]
            held = all(0 <= v < N0 for v in rel)
            covered = all(N0 // 4 <= v < N0 - N0 // 4 for v in rel)
            return held and not (covered and level + 1 < LEVELS)

        def cells(k, j, i, n=n):
            x, y, z = ((index + 0.5) / n for index in (i, j, k))
            return FIELD(x, y, z)

        h.origin.append([0, 0, 0])
        h.mask.append(_Rule((n, n, n), leaf))
        h.values.append(_Rule((n, n, n), cells))
        h.dx.append([1.0 / n] * 3)
    return h


def wait(event, limit: float, what: str) -> None:
    """Returns when the event is done.  When it is not after `limit` seconds the tool reports it and
    ends with status 3 without launching anything more; it does not close the scene or the
    context, which would wait for the very call that is not coming back."""
    deadline = time.monotonic() + limit
    while not event.query():
        if time.monotonic() > deadline:
            print(json.dumps({"error": f"{what} was not done after {limit} s"}))
            sys.stdout.flush()
            os._exit(3)
        time.sleep(0.0005)


def run(frames: int, warmup: int, limit: float, reference: bool = True) -> dict:
    import numpy as np
    import torch
    from amrvolumerenderer_amd import rays as ray_rules
    from amrvolumerenderer_amd import runtime, scenes
    from amrvolumerenderer_amd.types import AmrBox, ScalarTransform
    if not torch.cuda.is_available():
        raise SystemExit("tools/ray_timing.py needs a HIP device")
    ctx = runtime.Context(0)
    spec = scenes.make_amr_scene(N0, LEVELS, BOX, "smooth", "config4_amr3_512")
    boxes = []
    for m in spec.boxes:
        x, y, z = scenes._cell_centres(m, spec, torch, device=ctx.device)
        cells = FIELD(x[None, None, :], y[None, :, None], z[:, None, None]).contiguous()
        boxes.append(AmrBox(m.min_corner, m.max_corner, cells, m.level))
    field = ctx.create_scene(boxes, ScalarTransform())
    torch.cuda.synchronize()
    index = np.array([m.lo for m in spec.boxes], dtype=np.int32)
    sizes = np.array([[1.0 / (N0 << l)] * 3 for l in range(LEVELS)])
    ratios = [2] * (LEVELS - 1)
    bounds = ray_rules.level0_bounds(index, [m.dims for m in spec.boxes],
                                     [m.level for m in spec.boxes], ratios)
    max_trips = ray_rules.default_max_trips(bounds, ratios, LEVELS)
    start, end = rays()
    a, b = torch.from_numpy(start).to(ctx.device), torch.from_numpy(end).to(ctx.device)
    arguments = (a, b, max_trips, index, ratios, sizes, [0.0, 0.0, 0.0])
    n = start.shape[0]

    def timed(call, what):
        begin, done = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        begin.record(ctx.stream)
        out = call()
        done.record(ctx.stream)
        wait(done, limit, what)
        return out, begin.elapsed_time(done)

    pairs = []
    for _ in range(warmup + frames):
        t0 = time.perf_counter()
        (counts, status, span), count_ms = timed(lambda: field.rays(*arguments), "the count pass")
        offsets = torch.zeros(n + 1, dtype=torch.int64, device=ctx.device)
        torch.cumsum(counts.to(torch.int64), 0, out=offsets[1:])
        ctx.synchronize()
        total = int(offsets[-1].item())
        emitted, emit_ms = timed(lambda: field.rays(*arguments, offsets=offsets, n_segments=total),
                                 "the emit pass")
        pairs.append((count_ms, emit_ms, (time.perf_counter() - t0) * 1e3))
    pairs = pairs[warmup:]
    mean = lambda k: sum(p[k] for p in pairs) / len(pairs)
    pair_ms = mean(2)
    t0_dev, t1_dev, level, value, integral, covered = (t.cpu().numpy() for t in emitted)
    status, offsets = status.cpu().numpy(), offsets.cpu().numpy()
    result = {"config": "config-4", "boxes": len(spec.boxes), "rays": n, "max_trips": max_trips,
              "frames": frames, "warmup": warmup, "count_ms": round(mean(0), 4),
              "emit_ms": round(mean(1), 4), "pair_ms": round(pair_ms, 4),
              "pair_ms_min": round(min(p[2] for p in pairs), 4), "segments": total,
              "segments_per_ray": round(total / n, 2),
              "rays_crossing": int(np.count_nonzero(np.diff(offsets) > 0)),
              "segments_per_crossing_ray": round(
                  total / max(int(np.count_nonzero(np.diff(offsets) > 0)), 1), 2),
              "segments_per_s": round(total / (pair_ms * 1e-3)),
              "status": np.bincount(status, minlength=4).tolist(),
              "by_level": np.bincount(level.astype(np.int64) + 1, minlength=LEVELS + 1).tolist()}
    field.close()
    ctx.close()
    if not reference:
        return result
    # the reference on 64 of the same rays, spread over the middle half of the image
    i = np.arange(REFERENCE_RAYS)
    pick = (IMAGE // 4 + 2 * i) * IMAGE + IMAGE // 4 + (i * 37) % (IMAGE // 2)
    hierarchy = rule_hierarchy()
    begin = time.perf_counter()
    want = hierarchy.rays(start[pick], end[pick], max_trips)
    seconds = time.perf_counter() - begin
    cut = np.concatenate([np.arange(offsets[s], offsets[s + 1]) for s in pick]).astype(np.int64)
    same = (np.array_equal(np.diff(want["offsets"]), np.diff(offsets)[pick]) and
            np.array_equal(want["status"], status[pick]) and
            want["t0"].tobytes() == t0_dev[cut].tobytes() and
            want["t1"].tobytes() == t1_dev[cut].tobytes() and
            np.array_equal(want["level"], level[cut]) and
            want["value"].tobytes() == value[cut].tobytes() and
            want["integral"].tobytes() == integral[pick].tobytes() and
            want["covered"].tobytes() == covered[pick].tobytes())
    segments = int(want["offsets"][-1])
    result["reference"] = {"rays": REFERENCE_RAYS, "seconds": round(seconds, 3),
                           "segments": segments,
                           "segments_per_s": round(segments / seconds),
                           "trips_per_ray": round(float(want["trips"].mean()), 2),
                           "trips_per_segment": round(float(want["trips"].sum()) / max(segments, 1), 3),
                           "equal_bits": bool(same)}
    return result


if __name__ == "__main__":
    parser = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    parser.add_argument("--frames", type=int, default=10)
    parser.add_argument("--warmup", type=int, default=3)
    parser.add_argument("--limit", type=float, default=60.0,
                        help="seconds one call may take before the tool gives up")
    parser.add_argument("--no-reference", action="store_true", help="leave the reference out")
    args = parser.parse_args()
    print(json.dumps(run(args.frames, args.warmup, args.limit, not args.no_reference)))
