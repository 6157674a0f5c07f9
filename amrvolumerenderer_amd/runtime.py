"""Context (one per rank = per GPU) and thin tensor-level wrappers over the C ABI.

PyTorch is plumbing here: it owns device memory (HBM tensors) and the HIP stream; every
computation goes through libavr_hip.so.  Host-only helpers (colour table, sampling constants,
depth hints, layer order, piece ranges) work without a GPU.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _capi
from .types import AmrBox, CameraParameters, ScalarTransform

INF = float("inf")
# what a column-projection picture shows (avr_projection_colorize: AVR_PROJECTION_COLUMN, _MEAN)
PROJECTION_QUANTITIES = ("column", "mean")


# ---------------------------------------------------------------------------------------------
# host-only helpers
# ---------------------------------------------------------------------------------------------

def build_color_table(alpha_scale: float, normalization_factor: float,
                      scalar_range=(0.0, 1.0), color_map=None) -> np.ndarray:
    """buildColorTable (Common/VolumePainter.cpp:442-516) -> [256, 4] float32."""
    from .types import colormap_to_c
    out = np.empty(1024, dtype=np.float32)
    rng = (C.c_float * 2)(float(scalar_range[0]), float(scalar_range[1]))
    arr, n = colormap_to_c(color_map)
    _capi.check(_capi.lib().avr_build_color_table(
        float(alpha_scale), float(normalization_factor), rng,
        C.cast(arr, C.POINTER(_capi.ColormapPoint)) if n else None, n,
        out.ctypes.data_as(C.POINTER(C.c_float))))
    return out.reshape(256, 4)


def box_sampling(box: AmrBox, params: _capi.PaintParams) -> Tuple[float, float, float]:
    """(sampleDistance, normalizationFactor, alphaScale), VolumePainter.cpp:571-613."""
    sd, nf, als = C.c_float(), C.c_float(), C.c_float()
    cbox = box.to_c()
    _capi.check(_capi.lib().avr_box_sampling(C.byref(cbox), C.byref(params), C.byref(sd),
                                             C.byref(nf), C.byref(als)))
    return sd.value, nf.value, als.value


def box_depth_hint(box: AmrBox, camera: CameraParameters) -> float:
    """computeBoxDepthHint (VolumeRenderer/VolumeRenderer.cpp:541-553)."""
    out = C.c_float()
    cbox, ccam = box.to_c(), camera.to_c()
    _capi.check(_capi.lib().avr_box_depth_hint(C.byref(cbox), C.byref(ccam), C.byref(out)))
    return out.value


def reference_sample_distance(boxes: Sequence[AmrBox], bounds_min, bounds_max) -> float:
    """VolumeRenderer/VolumeRenderer.cpp:1138-1190 over the given boxes."""
    arr = (_capi.Box * max(len(boxes), 1))(*[b.to_c() for b in boxes])
    bmin = (C.c_double * 3)(*map(float, bounds_min))
    bmax = (C.c_double * 3)(*map(float, bounds_max))
    out = C.c_float()
    _capi.check(_capi.lib().avr_reference_sample_distance(arr, len(boxes), bmin, bmax,
                                                          C.byref(out)))
    return out.value


class VisibilityGraph:
    """avr_visibility_graph: the rank order of the compositing group for a camera
    (BuildVisibilityOrderedGroup, Common/VisibilityOrdering.cpp:63-632) over the replicated box
    metadata.  Host only."""

    def __init__(self, all_boxes: Sequence[AmrBox], n_ranks: int):
        self.n_ranks = int(n_ranks)
        arr = (_capi.Box * max(len(all_boxes), 1))(*[b.to_c() for b in all_boxes])
        owners = (C.c_int32 * max(len(all_boxes), 1))(*[int(b.owner) for b in all_boxes])
        handle = C.c_void_p()
        _capi.check(_capi.lib().avr_visibility_graph_create(arr, owners, len(all_boxes),
                                                            self.n_ranks, C.byref(handle)))
        self._handle = handle
        self.last_succeeded = True
        self.last_splits = 0

    def close(self) -> None:
        if getattr(self, "_handle", None):
            _capi.lib().avr_visibility_graph_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def order(self, camera: CameraParameters, aspect: float, use_visibility_graph: bool = True,
              dot_prefix: Optional[str] = None) -> List[int]:
        """The ranks in group order.  A failed ordering returns the default order and clears
        last_succeeded (the reference warns once and continues)."""
        out = (C.c_int32 * self.n_ranks)()
        ok, splits = C.c_int(1), C.c_int(0)
        ccam = camera.to_c()
        _capi.check(_capi.lib().avr_visibility_order(
            self._handle, C.byref(ccam), C.c_float(aspect), int(bool(use_visibility_graph)),
            dot_prefix.encode() if dot_prefix else None, out, C.byref(ok), C.byref(splits)))
        self.last_succeeded = bool(ok.value)
        self.last_splits = int(splits.value)
        return list(out)


def tight_bounds(boxes: Sequence[AmrBox], fallback_min, fallback_max):
    """computeTightBounds (VolumeRenderer/VolumeRenderer.cpp:791-848) over replicated metadata."""
    arr = (_capi.Box * max(len(boxes), 1))(*[b.to_c() for b in boxes])
    fmin = (C.c_double * 3)(*map(float, fallback_min))
    fmax = (C.c_double * 3)(*map(float, fallback_max))
    omin, omax = (C.c_double * 3)(), (C.c_double * 3)()
    _capi.check(_capi.lib().avr_tight_bounds(arr, len(boxes), fmin, fmax, omin, omax))
    return tuple(omin), tuple(omax)


def layer_order(hints, owner, local_index) -> Tuple[np.ndarray, np.ndarray]:
    """Global layer order and run ends (DirectSend/Base/DirectSendBase.cpp:363-410)."""
    hints = np.ascontiguousarray(hints, dtype=np.float32)
    owner = np.ascontiguousarray(owner, dtype=np.int32)
    local_index = np.ascontiguousarray(local_index, dtype=np.int32)
    n = int(hints.size)
    order = np.empty(max(n, 1), dtype=np.int32)
    run_end = np.empty(max(n, 1), dtype=np.int32)
    n_runs = C.c_int()
    ip = C.POINTER(C.c_int32)
    _capi.check(_capi.lib().avr_layer_order(
        hints.ctypes.data_as(C.POINTER(C.c_float)), owner.ctypes.data_as(ip),
        local_index.ctypes.data_as(ip), n, order.ctypes.data_as(ip), run_end.ctypes.data_as(ip),
        C.byref(n_runs)))
    return order[:n].copy(), run_end[:n_runs.value].copy()


def scene_transform_from_stats(stats: Sequence[float], finite_count: int, log_scale: bool = False,
                               normalize_to_data_range: bool = True):
    """The scalar-transform part of BuildSceneGeometry (SceneBuilder.cpp:315-443) from reduced
    statistics (min, max, min positive).  Returns (ScalarTransform, processed_range,
    scalar_range); raises RuntimeError where the reference throws std::runtime_error."""
    st = (C.c_double * 3)(*[float(v) for v in stats])
    ctr = _capi.ScalarTransform()
    processed = (C.c_double * 2)()
    pr, sr = (C.c_float * 2)(), (C.c_float * 2)()
    _capi.check(_capi.lib().avr_scene_transform_from_stats(
        st, int(finite_count), int(bool(log_scale)), int(bool(normalize_to_data_range)),
        C.byref(ctr), processed, pr, sr))
    span = processed[1] - processed[0]
    transform = ScalarTransform(
        log_scale_input=bool(ctr.log_scale_input),
        normalize_to_unit_range=bool(ctr.normalize_to_unit_range),
        positive_floor=ctr.positive_floor, processed_min=processed[0], processed_max=processed[1],
        inverse_processed_span=1.0 / span, normalization_min=ctr.normalization_min,
        normalization_max=processed[1],
        inverse_normalization_span=ctr.inverse_normalization_span)
    return transform, (pr[0], pr[1]), (sr[0], sr[1])


def piece_range(image_size: int, piece_index: int, num_pieces: int) -> Tuple[int, int]:
    """getPieceRange (DirectSend/Base/DirectSendBase.cpp:59-74)."""
    b, e = C.c_int64(), C.c_int64()
    _capi.check(_capi.lib().avr_piece_range(int(image_size), int(piece_index), int(num_pieces),
                                            C.byref(b), C.byref(e)))
    return b.value, e.value


# ---------------------------------------------------------------------------------------------
# device context
# ---------------------------------------------------------------------------------------------

class Context:
    """One rendering context per rank (= per GPU).  Owns a HIP stream (a torch stream, so
    torch allocations / collectives can be ordered against the kernels)."""

    def __init__(self, device: Optional[int] = None, priority: int = 0):
        """priority: 0 = default, -1 = high (torch.cuda.Stream's convention): work queued on a
        high-priority stream is dispatched before work of default streams."""
        if not torch.cuda.is_available():
            raise _capi.AvrNoDevice("no HIP device visible to PyTorch; the renderer has no CPU "
                                    "fallback")
        self.device_index = torch.cuda.current_device() if device is None else int(device)
        self.device = torch.device("cuda", self.device_index)
        handle = C.c_void_p()
        _capi.check(_capi.lib().avr_context_create(self.device_index, C.byref(handle)))
        self._handle = handle
        self.stream = torch.cuda.Stream(device=self.device, priority=priority)
        _capi.check(_capi.lib().avr_context_set_stream(self._handle,
                                                       C.c_void_p(self.stream.cuda_stream)))

    def close(self) -> None:
        if getattr(self, "_handle", None):
            _capi.lib().avr_context_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- stream ordering -----------------------------------------------------------------------
    def join(self) -> None:
        """Make the context stream wait for work already queued on torch's current stream."""
        self.stream.wait_stream(torch.cuda.current_stream(self.device))

    def publish(self) -> None:
        """Make torch's current stream wait for the context stream."""
        torch.cuda.current_stream(self.device).wait_stream(self.stream)

    def synchronize(self) -> None:
        _capi.check(_capi.lib().avr_context_synchronize(self._handle))

    def set_velocity_cube_scratch_entries(self, entries: int = 0) -> None:
        """avr_context_set_velocity_cube_scratch_entries: the bound on channels of a batch x
        entries of a partial plane of Scene.velocity_cube (0: the default of 2^27)."""
        _capi.check(_capi.lib().avr_context_set_velocity_cube_scratch_entries(self._handle,
                                                                              int(entries)))

    def set_ray_transfer_chunk(self, channels: int = 0) -> None:
        """avr_context_set_ray_transfer_chunk: the channels a workgroup of Scene.ray_transfer keeps
        in LDS at a time, 1 .. 32 (0: the default of 16).  The results do not depend on it."""
        _capi.check(_capi.lib().avr_context_set_ray_transfer_chunk(self._handle, int(channels)))

    def set_march_occupancy(self, workgroups_per_cu: int) -> None:
        """avr_context_set_march_occupancy: resident march workgroups per CU (0 = uncapped)."""
        _capi.check(_capi.lib().avr_context_set_march_occupancy(self._handle,
                                                                int(workgroups_per_cu)))

    def set_march_counters(self, counters: Optional[torch.Tensor]) -> None:
        """avr_context_set_march_counters: diagnostics for the parity tests (5 x int64 on the
        device, or None to switch them off)."""
        if counters is not None:
            self._check_tensor(counters, torch.int64, "counters")
            if counters.numel() < 5:
                raise ValueError("counters needs 5 entries")
        self._march_counters = counters  # keep alive while set
        _capi.check(_capi.lib().avr_context_set_march_counters(
            self._handle, C.c_void_p(counters.data_ptr()) if counters is not None else None))

    def last_march_mode(self) -> int:
        """avr_context_last_march_mode: the index mode the latest march of this context was
        specialised on (0 power-of-two product, 1 reciprocal, 2 exact divide, 3 power-of-two product
        with the four-instruction bricklet offset), -1 if its boxes differed, -2 before any march."""
        mode = C.c_int(-2)
        _capi.check(_capi.lib().avr_context_last_march_mode(self._handle, C.byref(mode)))
        return int(mode.value)

    # -- helpers ----------------------------------------------------------------------------
    def _check_tensor(self, t: torch.Tensor, dtype, what: str) -> None:
        if not isinstance(t, torch.Tensor) or t.device != self.device:
            raise ValueError(f"{what} must be a tensor on {self.device}")
        if t.dtype != dtype or not t.is_contiguous():
            raise ValueError(f"{what} must be a contiguous {dtype} tensor")

    def empty(self, *shape, dtype=torch.float32) -> torch.Tensor:
        return torch.empty(*shape, dtype=dtype, device=self.device)

    # -- power spectra ------------------------------------------------------------------------
    def fft3d(self, values: torch.Tensor) -> torch.Tensor:
        """avr_field_fft: the forward, unnormalised 3-D transform of a real grid (DESIGN.md 7,
        "Power spectrum").  values: contiguous float64 [nz, ny, nx] on the device, every
        dimension a power of two in [1, 1024].  Returns the spectrum, float64 [nz, ny, nx, 2]
        with (re, im) interleaved, on the device.  Asynchronous on the context's stream."""
        self._check_tensor(values, torch.float64, "values")
        if values.ndim != 3 or values.numel() == 0:
            raise ValueError("values must be [nz, ny, nx] with at least one cell")
        nz, ny, nx = (int(v) for v in values.shape)
        dims = np.array([nx, ny, nz], dtype=np.int32)
        spectrum = torch.empty((nz, ny, nx, 2), dtype=torch.float64, device=self.device)
        _native(self, "avr_field_fft", self._handle, _pointer(values), _ints(dims),
                _pointer(spectrum))
        return spectrum

    def spectrum_bins(self, spectrum: torch.Tensor, inverse_length_sq, edges_sq, out=None):
        """avr_spectrum_bins: ADDS the shell sums of a spectrum (float64 [nz, ny, nx, 2] on the
        device, as fft3d returns it) to (modes int64 [n], power float64 [n], totals int64 [2] =
        (outside, nonfinite)) on the device: `out`, or new zeroed tensors.  inverse_length_sq:
        1 / L_d^2 for d = x, y, z; edges_sq: the n + 1 squared edges (e / (2 pi))^2, strictly
        increasing from a value >= 0 ("Power spectrum").  Returns (modes, power,
        totals).  Asynchronous on the context's stream."""
        dims = self._spectrum_dims(spectrum)
        g = np.ascontiguousarray(inverse_length_sq, dtype=np.float64)
        edges = np.ascontiguousarray(edges_sq, dtype=np.float64)
        _require_triple(g, "inverse_length_sq")
        if edges.ndim != 1 or edges.size < 2:
            raise ValueError("edges_sq must hold at least two values")
        n = int(edges.size) - 1
        modes, power, totals = out if out is not None else (None, None, None)
        wrong = "out must be (modes int64 [n], power float64 [n], totals int64 [2])"
        modes = _output(self, modes, torch.int64, (n,), "modes", torch.zeros, wrong)
        power = _output(self, power, torch.float64, (n,), "power", torch.zeros, wrong)
        totals = _output(self, totals, torch.int64, (2,), "totals", torch.zeros, wrong)
        _native(self, "avr_spectrum_bins", self._handle, _pointer(spectrum), _ints(dims),
                _doubles(g), _doubles(edges), n, _pointer(modes), _pointer(power),
                _pointer(totals))
        return modes, power, totals

    # -- inverse transform, Helmholtz split, potential -----------------------------------------
    def _spectrum_dims(self, spectrum: torch.Tensor, what: str = "spectrum") -> np.ndarray:
        self._check_tensor(spectrum, torch.float64, what)
        if spectrum.ndim != 4 or spectrum.shape[3] != 2 or spectrum.numel() == 0:
            raise ValueError(f"{what} must be [nz, ny, nx, 2] with at least one mode")
        nz, ny, nx = (int(v) for v in spectrum.shape[:3])
        return np.array([nx, ny, nz], dtype=np.int32)

    def ifft3d(self, spectrum: torch.Tensor, with_imag: bool = False):
        """avr_field_ifft: the normalised inverse 3-D transform of a spectrum (float64
        [nz, ny, nx, 2] on the device, as fft3d returns it; DESIGN.md 7, "Inverse transform,
        Helmholtz split, potential").  The strided passes run in place: what `spectrum` holds
        afterwards is unspecified.  Returns the real part, float64 [nz, ny, nx] on the device --
        with with_imag (real, imag), the imaginary part a grid of the same shape.  Asynchronous on
        the context's stream."""
        dims = self._spectrum_dims(spectrum)
        shape = tuple(int(v) for v in spectrum.shape[:3])
        values = torch.empty(shape, dtype=torch.float64, device=self.device)
        imag = torch.empty(shape, dtype=torch.float64, device=self.device) if with_imag else None
        _native(self, "avr_field_ifft", self._handle, _pointer(spectrum), _ints(dims),
                _pointer(values), _pointer(imag))
        return (values, imag) if with_imag else values

    def helmholtz_split(self, fx: torch.Tensor, fy: torch.Tensor, fz: torch.Tensor,
                        inverse_length):
        """avr_spectrum_helmholtz: splits the spectra of (vx, vy, vz) (float64 [nz, ny, nx, 2] on
        the device, of one shape) into their solenoidal and compressive parts (DESIGN.md 7,
        "Inverse transform, Helmholtz split, potential").  inverse_length: 1 / L_d for d = x, y,
        z.  Returns (solenoidal, compressive), three spectra each: the solenoidal ones are fx, fy
        and fz themselves, overwritten; the compressive ones are new.  Asynchronous on the
        context's stream."""
        dims = self._spectrum_dims(fx, "fx")
        for other, what in ((fy, "fy"), (fz, "fz")):
            if not np.array_equal(self._spectrum_dims(other, what), dims):
                raise ValueError("fx, fy and fz must have one shape")
        h = np.ascontiguousarray(inverse_length, dtype=np.float64)
        _require_triple(h, "inverse_length")
        compressive = tuple(torch.empty_like(fx) for _ in range(3))
        inputs = (C.c_void_p * 3)(*(f.data_ptr() for f in (fx, fy, fz)))
        outputs = (C.c_void_p * 3)(*(c.data_ptr() for c in compressive))
        _native(self, "avr_spectrum_helmholtz", self._handle, inputs, _ints(dims), _doubles(h),
                outputs)
        return (fx, fy, fz), compressive

    def inverse_laplacian(self, spectrum: torch.Tensor, inverse_length_sq,
                          scale: float) -> torch.Tensor:
        """avr_spectrum_inverse_laplacian: every mode of a spectrum (float64 [nz, ny, nx, 2] on the
        device) times scale / q in place, q = sum_d m_d^2 / L_d^2 as the shell sums have it, and
        (0, 0) where q == 0 ("Inverse transform, Helmholtz split, potential").
        inverse_length_sq: 1 / L_d^2 for d = x, y, z.  Returns `spectrum`.  Asynchronous on the
        context's stream."""
        dims = self._spectrum_dims(spectrum)
        g = np.ascontiguousarray(inverse_length_sq, dtype=np.float64)
        _require_triple(g, "inverse_length_sq")
        _native(self, "avr_spectrum_inverse_laplacian", self._handle, _pointer(spectrum),
                _ints(dims), _doubles(g), float(scale))
        return spectrum

    # -- isolated potential -------------------------------------------------------------------
    def isolated_green(self, padded_dims, cell_size, scale: float,
                       self_value: float = 0.0) -> torch.Tensor:
        """avr_isolated_green: the open-boundary Green's function scale / r on the zero-padded
        grid of padded_dims = (Px, Py, Pz), powers of two in [1, 1024], with cells of cell_size =
        (dx, dy, dz); r is measured to the nearer image of the origin along every axis, and the
        cell (0, 0, 0) holds self_value ("Isolated potential").  Returns float64
        [Pz, Py, Px] on the device.  Asynchronous on the context's stream."""
        dims = np.ascontiguousarray(padded_dims, dtype=np.int64)
        size = np.ascontiguousarray(cell_size, dtype=np.float64)
        if dims.shape != (3,):
            raise ValueError("padded_dims must hold three values")
        _require_triple(size, "cell_size")
        if not ((dims >= 1) & (dims <= 1024)).all():
            raise ValueError("padded_dims must be powers of two in [1, 1024]")
        px, py, pz = (int(v) for v in dims)
        dims = dims.astype(np.int32)
        green = torch.empty((pz, py, px), dtype=torch.float64, device=self.device)
        _native(self, "avr_isolated_green", self._handle, _ints(dims),
                _doubles(size), float(scale), float(self_value), _pointer(green))
        return green

    def spectrum_multiply(self, a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
        """avr_spectrum_multiply: a <- a b, the complex product mode by mode of two spectra
        (float64 [nz, ny, nx, 2] on the device, of one shape, sharing no memory; DESIGN.md 7,
        "Isolated potential").  b is only read.  Returns `a`.  Asynchronous on the context's
        stream."""
        dims = self._spectrum_dims(a, "a")
        if not np.array_equal(self._spectrum_dims(b, "b"), dims):
            raise ValueError("a and b must have one shape")
        _native(self, "avr_spectrum_multiply", self._handle, _pointer(a), _pointer(b),
                _ints(dims))
        return a

    # -- structure functions ------------------------------------------------------------------
    def structure_functions(self, components, lags, directions=None, max_order: int = 6,
                            periodic: bool = False, out=None):
        """avr_grid_structure_functions: ADDS the moments of the increments of one grid or of
        three (contiguous float64 [nz, ny, nx] on the device, of one shape, any dims >= 1) over the
        lags (integers [M, 3], rows (lx, ly, lz), M in [1, 4096], every |l_d| < N_d) to (pairs
        int64 [M], sums float64 [M, K, max_order], totals int64 [2] = (outside, nonfinite)) on the
        device: `out`, or new zeroed tensors.  K = 1 for one grid (|dv|), 3 for three
        (longitudinal, transverse, magnitude), which need directions float64 [M, 3], the unit
        vector of every lag (structure.unit_directions).  periodic wraps the partner once along
        every axis; without it a pair that leaves the grid counts as outside (DESIGN.md 7,
        "Structure functions").  Returns (pairs, sums, totals).  Asynchronous on the context's
        stream."""
        if isinstance(components, torch.Tensor):
            components = (components,)
        components = tuple(components)
        if len(components) not in (1, 3):
            raise ValueError("components must be one grid or three")
        for c, grid in enumerate(components):
            self._check_tensor(grid, torch.float64, f"components[{c}]")
            if grid.ndim != 3 or grid.numel() == 0:
                raise ValueError("a component must be [nz, ny, nx] with at least one cell")
            if grid.shape != components[0].shape:
                raise ValueError("the components must have one shape")
        nz, ny, nx = (int(v) for v in components[0].shape)
        dims = np.array([nx, ny, nz], dtype=np.int32)
        table = np.asarray(lags)
        if table.ndim != 2 or table.shape[1] != 3 or table.shape[0] < 1:
            raise ValueError("lags must be [M, 3] with at least one lag")
        if not np.array_equal(table, table.astype(np.int32)):
            raise ValueError("lags must be 32-bit integers")
        table = np.ascontiguousarray(table, dtype=np.int32)
        n_lags, kinds = int(table.shape[0]), len(components)
        if (directions is not None) != (kinds == 3):
            raise ValueError("directions are given exactly with three components")
        if directions is not None:
            directions = np.ascontiguousarray(directions, dtype=np.float64)
            if directions.shape != (n_lags, 3):
                raise ValueError("directions must hold three values per lag")
        order = int(max_order)
        if order < 1:
            raise ValueError("max_order must lie in [1, 8]")
        pairs, sums, totals = out if out is not None else (None, None, None)
        wrong = "out must be (pairs int64 [M], sums float64 [M, K, max_order], totals int64 [2])"
        pairs = _output(self, pairs, torch.int64, (n_lags,), "pairs", torch.zeros, wrong)
        sums = _output(self, sums, torch.float64, (n_lags, kinds, order), "sums", torch.zeros,
                       wrong)
        totals = _output(self, totals, torch.int64, (2,), "totals", torch.zeros, wrong)
        grids = (C.c_void_p * 3)(*(grid.data_ptr() for grid in components))
        _native(self, "avr_grid_structure_functions", self._handle, grids, kinds, _ints(dims),
                _ints(table), _doubles(directions) if directions is not None else None, n_lags,
                order, int(bool(periodic)), _pointer(pairs), _pointer(sums), _pointer(totals))
        return pairs, sums, totals

    # -- clump binding ------------------------------------------------------------------------
    def clump_pair_energy(self, offsets, x: torch.Tensor, y: torch.Tensor, z: torch.Tensor,
                          m: torch.Tensor, w: Optional[torch.Tensor] = None):
        """avr_clump_pair_energy: per segment s of the members offsets[s] .. offsets[s + 1] - 1
        (offsets: n_segments + 1 ascending int64 on the host, from 0) the self-energy
        sum_{i<j} m_i m_j / |x_i - x_j| by direct summation in float64 ("Clump
        binding").  x, y, z, m: float64 [offsets[-1]] on the device.  Returns (W float64
        [n_segments] on the device, depth int64 [n_segments] numpy: the longest chain of rounded
        additions a term of the segment passes through).  Asynchronous on the context's stream."""
        offsets = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
        if offsets.size < 1:
            raise ValueError("offsets must hold n_segments + 1 values")
        n_segments = int(offsets.size) - 1
        for name, t in (("x", x), ("y", y), ("z", z), ("m", m)):
            self._check_tensor(t, torch.float64, name)
            if t.numel() != int(offsets[-1]):
                raise ValueError("x, y, z and m must hold offsets[-1] values")
        w = _output(self, w, torch.float64, (n_segments,), "w", wrong_size="w must hold one value "
                    "per segment")
        depth = np.zeros(n_segments, dtype=np.int64)
        _native(self, "avr_clump_pair_energy", self._handle,
                offsets.ctypes.data_as(C.POINTER(C.c_int64)), n_segments, _pointer(x), _pointer(y),
                _pointer(z), _pointer(m), _pointer(w),
                depth.ctypes.data_as(C.POINTER(C.c_int64)))
        return w, depth

    # -- particle groups ----------------------------------------------------------------------
    def particle_group_cells(self, points, lo, hi, dims, periodic,
                             totals: Optional[torch.Tensor] = None):
        """avr_particle_group_cells: the cell of every particle of points (float64 [n, 3]; a tensor
        on the device, or anything numpy takes) in the uniform grid of dims cells over the box lo,
        hi with the flags periodic ("Particle groups").  Returns (points as they lie
        on the device, cells int32 [n] -- the cell's bits as uint32, all ones for a particle
        outside --, parent int32 [n] likewise, totals int64 [1]: the outside particles; a tensor
        handed in is added to).  Asynchronous on the context's stream."""
        lo, hi, dims, periodic = _group_box(lo, hi, dims, periodic)
        points = _device_points(self, points, "points must hold three values per particle")
        n = int(points.shape[0])
        cells = torch.empty(n, dtype=torch.int32, device=self.device)
        parent = torch.empty(n, dtype=torch.int32, device=self.device)
        totals = _output(self, totals, torch.int64, (1,), "totals", torch.zeros,
                         "totals must hold one value")
        _native(self, "avr_particle_group_cells", self._handle, _pointer(points), n, _doubles(lo),
                _doubles(hi), _ints(dims), _ints(periodic), _pointer(cells), _pointer(parent),
                _pointer(totals))
        return points, cells, parent, totals

    def particle_groups(self, points: torch.Tensor, cells: torch.Tensor, parent: torch.Tensor,
                        linking_length: float, lo, hi, dims, periodic, min_members: int = 1,
                        max_pair_tests: Optional[int] = None):
        """avr_particle_groups behind the sort it needs: points, cells and parent as
        particle_group_cells returned them, for the same box and dims.  The particles are sorted by
        cell with a stable torch sort, the first slot of every cell is found with
        torch.searchsorted and the points are gathered into that order (plumbing).  The number of
        pair tests the link kernel will make is counted exactly from the cells' occupancies first;
        above max_pair_tests (None: no cap) ValueError is raised and nothing more is launched.
        Returns (labels int32 [n], parent int32 [n] -- each inside particle's root, in place --,
        sizes int32 [n] -- the members at a root's index --, n_groups int64 [1]) on the device
        and pair_tests, an int.  Synchronises once, for the counts; the native call itself is
        asynchronous on the context's stream."""
        lo, hi, dims, periodic = _group_box(lo, hi, dims, periodic)
        self._check_tensor(points, torch.float64, "points")
        self._check_tensor(cells, torch.int32, "cells")
        self._check_tensor(parent, torch.int32, "parent")
        n = int(cells.numel())
        if tuple(points.shape) != (n, 3) or int(parent.numel()) != n:
            raise ValueError("points, cells and parent must describe the same particles")
        n_cells = int(dims[0]) * int(dims[1]) * int(dims[2])
        labels = torch.empty(n, dtype=torch.int32, device=self.device)
        sizes = torch.empty(n, dtype=torch.int32, device=self.device)
        n_groups = torch.zeros(1, dtype=torch.int64, device=self.device)
        ordered = order = cell_begin = None
        n_inside = pair_tests = 0
        if n:
            # the cell as an unsigned number: an outside particle's sorts behind every cell;
            # stable, so that the slots of a cell ascend in particle index
            keys, order = torch.sort(cells.to(torch.int64) & 0xFFFFFFFF, stable=True)
            edges = torch.arange(n_cells + 1, dtype=torch.int64, device=self.device)
            cell_begin = torch.searchsorted(keys, edges).contiguous()
            ordered = points[order].contiguous()
            counts = (cell_begin[1:] - cell_begin[:-1]).reshape(int(dims[2]), int(dims[1]),
                                                                int(dims[0]))
            pair_tests = group_pair_tests(counts, periodic)
            n_inside = int(cell_begin[-1].item())
        if max_pair_tests is not None and pair_tests > int(max_pair_tests):
            raise ValueError(
                f"the link kernel would test {pair_tests} pairs of particles, more than "
                f"max_pair_tests = {int(max_pair_tests)}: the cells around the densest particles "
                "hold too many; use a smaller linking length, or raise max_pair_tests")
        _native(self, "avr_particle_groups", self._handle, _pointer(ordered), _pointer(order),
                _pointer(cell_begin), n, n_inside, float(linking_length), _doubles(lo),
                _doubles(hi), _ints(dims), _ints(periodic), int(min_members), _pointer(parent),
                _pointer(labels), _pointer(sizes), _pointer(n_groups))
        return labels, parent, sizes, n_groups, pair_tests

    # -- painter ----------------------------------------------------------------------------
    def paint_box(self, box: AmrBox, transform: ScalarTransform, params: _capi.PaintParams,
                  camera: CameraParameters, out: Optional[torch.Tensor] = None,
                  samples: Optional[torch.Tensor] = None) -> torch.Tensor:
        """avr_paint_box: one box -> [H, W, 5] depth-sort layer."""
        if out is None:
            out = self.empty(params.height, params.width, 5)
        self._check_tensor(out, torch.float32, "out")
        if out.numel() != params.width * params.height * 5:
            raise ValueError("out has the wrong size")
        if samples is not None:
            self._check_tensor(samples, torch.int64, "samples")
        cbox, ctr, ccam = box.to_c(), transform.to_c(), camera.to_c()
        self.join()
        _capi.check(_capi.lib().avr_paint_box(
            self._handle, C.byref(cbox), C.byref(ctr), C.byref(params), C.byref(ccam),
            C.c_void_p(out.data_ptr()),
            C.c_void_p(samples.data_ptr()) if samples is not None else None))
        self.publish()
        return out

    def paint_box_max(self, box: AmrBox, transform: ScalarTransform, params: _capi.PaintParams,
                      camera: CameraParameters, out: Optional[torch.Tensor] = None,
                      samples: Optional[torch.Tensor] = None) -> torch.Tensor:
        """avr_paint_box_max: one box -> [H, W] int16 maximum-intensity indices (-1: no sample),
        rows in paint_box's order (row 0 at the bottom)."""
        if out is None:
            out = torch.empty((params.height, params.width), dtype=torch.int16, device=self.device)
        self._check_tensor(out, torch.int16, "out")
        if out.numel() != params.width * params.height:
            raise ValueError("out has the wrong size")
        if samples is not None:
            self._check_tensor(samples, torch.int64, "samples")
        cbox, ctr, ccam = box.to_c(), transform.to_c(), camera.to_c()
        self.join()
        _capi.check(_capi.lib().avr_paint_box_max(
            self._handle, C.byref(cbox), C.byref(ctr), C.byref(params), C.byref(ccam),
            C.c_void_p(out.data_ptr()),
            C.c_void_p(samples.data_ptr()) if samples is not None else None))
        self.publish()
        return out

    def paint_box_projection(self, box: AmrBox, params: _capi.PaintParams, camera: CameraParameters,
                             column: Optional[torch.Tensor] = None,
                             length: Optional[torch.Tensor] = None,
                             samples: Optional[torch.Tensor] = None):
        """avr_paint_box_projection: one box -> (column, length), [H, W] float64 each: per pixel
        f64(step) times the sum, and times the number, of the finite raw cell values the box's
        march samples; rows in paint_box's order (row 0 at the bottom).  samples (int64) gains
        every sample taken."""
        outs = []
        for name, t in (("column", column), ("length", length)):
            if t is None:
                t = torch.empty((params.height, params.width), dtype=torch.float64, device=self.device)
            self._check_tensor(t, torch.float64, name)
            if t.numel() != params.width * params.height:
                raise ValueError(f"{name} has the wrong size")
            outs.append(t)
        if samples is not None:
            self._check_tensor(samples, torch.int64, "samples")
        cbox, ccam = box.to_c(), camera.to_c()
        self.join()
        _capi.check(_capi.lib().avr_paint_box_projection(
            self._handle, C.byref(cbox), C.byref(params), C.byref(ccam),
            C.c_void_p(outs[0].data_ptr()), C.c_void_p(outs[1].data_ptr()),
            C.c_void_p(samples.data_ptr()) if samples is not None else None))
        self.publish()
        return outs[0], outs[1]

    def projection_colorize(self, column: torch.Tensor, length: torch.Tensor, rgb_table: torch.Tensor,
                            quantity: str = "column", log_scale: bool = False,
                            value_range: Optional[Sequence[float]] = None):
        """avr_projection_colorize: (column, length) [H, W] float64 (row 0 at the bottom) ->
        (rgb8 [H, W, 3] uint8, rows top-down; range float64 [2], the [lo, hi] used -- the min and
        max of the displayed quantity when value_range is None).  rgb_table: [256, 3] uint8."""
        if quantity not in PROJECTION_QUANTITIES:
            raise ValueError(f"quantity must be one of {', '.join(PROJECTION_QUANTITIES)}, not {quantity!r}")
        self._check_tensor(column, torch.float64, "column")
        self._check_tensor(length, torch.float64, "length")
        self._check_tensor(rgb_table, torch.uint8, "rgb_table")
        if column.dim() != 2 or column.shape != length.shape or rgb_table.numel() != 256 * 3:
            raise ValueError("column and length must be [H, W] alike; rgb_table [256, 3]")
        height, width = column.shape
        rgb8 = torch.empty((height, width, 3), dtype=torch.uint8, device=self.device)
        if value_range is None:
            rng = torch.empty(2, dtype=torch.float64, device=self.device)
        else:
            rng = torch.tensor([float(value_range[0]), float(value_range[1])], dtype=torch.float64,
                               device=self.device)
        self.join()
        _capi.check(_capi.lib().avr_projection_colorize(
            self._handle, C.c_void_p(column.data_ptr()), C.c_void_p(length.data_ptr()), int(width),
            int(height), PROJECTION_QUANTITIES.index(quantity), int(bool(log_scale)),
            C.c_void_p(rng.data_ptr()), int(value_range is None), C.c_void_p(rgb_table.data_ptr()),
            C.c_void_p(rgb8.data_ptr())))
        self.publish()
        return rgb8, rng

    def slice_outline(self, box: torch.Tensor, rgb8: torch.Tensor,
                      color: Sequence[int] = (255, 255, 255)) -> torch.Tensor:
        """avr_slice_outline: box [H, W] int32 (Scene.slice's, row 0 at the bottom), rgb8 [H, W, 3]
        uint8 (rows top-down, written in place): every pixel whose box differs from that of its
        right or upper neighbour gets `color`."""
        self._check_tensor(box, torch.int32, "box")
        self._check_tensor(rgb8, torch.uint8, "rgb8")
        if box.dim() != 2 or tuple(rgb8.shape) != (box.shape[0], box.shape[1], 3):
            raise ValueError("box must be [H, W] and rgb8 [H, W, 3]")
        rgb = tuple(int(c) for c in color)
        if len(rgb) != 3 or not all(0 <= c <= 255 for c in rgb):
            raise ValueError("color must hold three values in [0, 255]")
        height, width = box.shape
        self.join()
        _capi.check(_capi.lib().avr_slice_outline(
            self._handle, C.c_void_p(box.data_ptr()), int(width), int(height), rgb[0], rgb[1],
            rgb[2], C.c_void_p(rgb8.data_ptr())))
        self.publish()
        return rgb8

    def create_scene(self, boxes: Sequence[AmrBox], transform: ScalarTransform) -> "Scene":
        return Scene(self, boxes, transform)

    # -- image algebra -------------------------------------------------------------------------
    _BLEND = {"depthsort": ("avr_blend_depthsort_f32x5", torch.float32, 5),
              "rgba_f32": ("avr_blend_rgba_f32x4", torch.float32, 4),
              "rgba_u8": ("avr_blend_rgba_u8x4", torch.int32, 1)}
    _KIND = {"depthsort": 0, "rgba_f32": 1, "rgba_u8": 2}

    def blend(self, kind: str, top: torch.Tensor, bottom: torch.Tensor,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
        name, dtype, vec = self._BLEND[kind]
        self._check_tensor(top, dtype, "top")
        self._check_tensor(bottom, dtype, "bottom")
        if top.numel() != bottom.numel():
            raise ValueError("top and bottom differ in size")
        if out is None:
            out = torch.empty_like(top)
        self._check_tensor(out, dtype, "out")
        self.join()
        _capi.check(getattr(_capi.lib(), name)(
            self._handle, C.c_void_p(top.data_ptr()), C.c_void_p(bottom.data_ptr()),
            C.c_void_p(out.data_ptr()), top.numel() // vec))
        self.publish()
        return out

    def blend_regions(self, kind: str, top: torch.Tensor, tb: int, te: int, bottom: torch.Tensor,
                      bb: int, be: int) -> Tuple[torch.Tensor, int, int]:
        _, dtype, vec = self._BLEND[kind]
        self._check_tensor(top, dtype, "top")
        self._check_tensor(bottom, dtype, "bottom")
        if top.numel() != (te - tb) * vec or bottom.numel() != (be - bb) * vec:
            raise ValueError("buffer sizes do not match the regions")
        ob, oe = min(tb, bb), max(te, be)
        out = self.empty((oe - ob) * vec, dtype=dtype)
        self.join()
        _capi.check(_capi.lib().avr_blend_regions(
            self._handle, self._KIND[kind], C.c_void_p(top.data_ptr()), tb, te,
            C.c_void_p(bottom.data_ptr()), bb, be, C.c_void_p(out.data_ptr())))
        self.publish()
        return out, ob, oe

    def encode_rgba_u8(self, rgba: torch.Tensor) -> torch.Tensor:
        self._check_tensor(rgba, torch.float32, "rgba")
        out = self.empty(rgba.numel() // 4, dtype=torch.int32)
        self.join()
        _capi.check(_capi.lib().avr_encode_rgba_u8(self._handle, C.c_void_p(rgba.data_ptr()),
                                                   C.c_void_p(out.data_ptr()), out.numel()))
        self.publish()
        return out

    def decode_rgba_u8(self, encoded: torch.Tensor) -> torch.Tensor:
        self._check_tensor(encoded, torch.int32, "encoded")
        out = self.empty(encoded.numel(), 4)
        self.join()
        _capi.check(_capi.lib().avr_decode_rgba_u8(self._handle, C.c_void_p(encoded.data_ptr()),
                                                   C.c_void_p(out.data_ptr()), encoded.numel()))
        self.publish()
        return out

    def fold_runs(self, slices: Sequence[torch.Tensor], n_pixels: int,
                  out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """avr_fold_runs_depthsort: left fold of run slices (each n_pixels x 5) in order."""
        for s in slices:
            self._check_tensor(s, torch.float32, "slice")
            if s.numel() != n_pixels * 5:
                raise ValueError("slice has the wrong size")
        if out is None:
            out = self.empty(n_pixels, 5)
        self._check_tensor(out, torch.float32, "out")
        ptrs = (C.c_void_p * max(len(slices), 1))(*[s.data_ptr() for s in slices])
        self.join()
        _capi.check(_capi.lib().avr_fold_runs_depthsort(self._handle, ptrs, len(slices),
                                                        C.c_void_p(out.data_ptr()), n_pixels))
        self.publish()
        return out

    def fold_plan(self, plan, recv: torch.Tensor, want_rgb8: bool = False,
                  sync_streams: bool = True, want_piece: bool = True,
                  own_send: Optional[torch.Tensor] = None):
        """avr_fold_plan: receiver-side fold of this rank's piece.  Returns
        (piece [piece_len, 5] or None, rgb8 [piece_len, 3] or None).  sync_streams=False: the
        caller already runs on this context's stream.  own_send (avr_fold_plan_own): the rank's
        send buffer, from which the blocks of its own runs are read instead of from recv."""
        if not (want_piece or want_rgb8):
            raise ValueError("nothing to produce")
        self._check_tensor(recv, torch.float32, "recv")
        if own_send is not None:
            self._check_tensor(own_send, torch.float32, "own_send")
            if own_send.numel() < plan.send_floats:
                raise ValueError("send buffer is too small")
        if recv.numel() < plan.recv_floats:
            raise ValueError("receive buffer is too small")
        n = plan.piece_end - plan.piece_begin
        piece = self.empty(max(n, 0), 5) if want_piece else None
        rgb8 = self.empty(max(n, 0), 3, dtype=torch.uint8) if want_rgb8 else None
        if sync_streams:
            self.join()
        _capi.check(_capi.lib().avr_fold_plan_own(
            self._handle, plan._handle, C.c_void_p(recv.data_ptr()),
            C.c_void_p(own_send.data_ptr()) if own_send is not None else None,
            C.c_void_p(piece.data_ptr()) if piece is not None else None,
            C.c_void_p(rgb8.data_ptr()) if rgb8 is not None else None))
        if sync_streams:
            self.publish()
        return piece, rgb8

    def fold_plan_image(self, plan, recv: torch.Tensor) -> torch.Tensor:
        """avr_fold_plan_image (one rank): the fold with its bytes written as the output file's
        rows, top-down.  Returns rgb8 [height, width, 3]."""
        self._check_tensor(recv, torch.float32, "recv")
        if recv.numel() < plan.recv_floats:
            raise ValueError("receive buffer is too small")
        rgb8 = self.empty(plan.height, plan.width, 3, dtype=torch.uint8)
        self.join()
        _capi.check(_capi.lib().avr_fold_plan_image(self._handle, plan._handle,
                                                    C.c_void_p(recv.data_ptr()), None,
                                                    C.c_void_p(rgb8.data_ptr())))
        self.publish()
        return rgb8

    def downsample(self, src: torch.Tensor, target_w: int, target_h: int, block: int
                   ) -> torch.Tensor:
        self._check_tensor(src, torch.float32, "src")
        if src.numel() != target_w * block * target_h * block * 5:
            raise ValueError("src has the wrong size")
        out = self.empty(target_h, target_w, 5)
        self.join()
        _capi.check(_capi.lib().avr_downsample_depthsort(
            self._handle, C.c_void_p(src.data_ptr()), target_w, target_h, block,
            C.c_void_p(out.data_ptr())))
        self.publish()
        return out

    def bbox_overlay(self, image: torch.Tensor, bounds_min, bounds_max,
                     camera: CameraParameters, sqrt_antialiasing: int, width: int, height: int,
                     pixel_begin: int = 0, pixel_end: Optional[int] = None,
                     want_rgb8: bool = False, sync_streams: bool = True) -> Optional[torch.Tensor]:
        """avr_bbox_overlay: the wireframe of the bounds blended in place over the pixels
        [pixel_begin, pixel_end) held by `image` (renderBoundingBoxLayer,
        VolumeRenderer.cpp:139-335); optionally also returns those pixels as RGB8."""
        self._check_tensor(image, torch.float32, "image")
        pixel_end = width * height if pixel_end is None else pixel_end
        if image.numel() != (pixel_end - pixel_begin) * 5:
            raise ValueError("image does not hold the pixel range")
        bmin = (C.c_double * 3)(*map(float, bounds_min))
        bmax = (C.c_double * 3)(*map(float, bounds_max))
        ccam = camera.to_c()
        rgb8 = self.empty(pixel_end - pixel_begin, 3, dtype=torch.uint8) if want_rgb8 else None
        if sync_streams:
            self.join()
        _capi.check(_capi.lib().avr_bbox_overlay(
            self._handle, bmin, bmax, C.byref(ccam), int(sqrt_antialiasing), width, height,
            pixel_begin, pixel_end, C.c_void_p(image.data_ptr()),
            C.c_void_p(rgb8.data_ptr()) if rgb8 is not None else None))
        if sync_streams:
            self.publish()
        return rgb8

    def quantize_rgb8(self, src: torch.Tensor, w: int, h: int) -> torch.Tensor:
        self._check_tensor(src, torch.float32, "src")
        stride = src.numel() // (w * h)
        out = self.empty(h, w, 3, dtype=torch.uint8)
        self.join()
        _capi.check(_capi.lib().avr_quantize_rgb8(self._handle, C.c_void_p(src.data_ptr()), w, h,
                                                  stride, C.c_void_p(out.data_ptr())))
        self.publish()
        return out


# ---------------------------------------------------------------------------------------------
# what Scene's field products share: pointers, level arguments, outputs, points, the native call
# ---------------------------------------------------------------------------------------------

_ABSENT = object()


def _doubles(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _ints(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def _require_triple(a: np.ndarray, name: str) -> None:
    """ValueError, naming the argument, unless the float64 array holds (x, y, z)."""
    if a.shape != (3,):
        raise ValueError(f"{name} must hold three values")


def _pointer(t: Optional[torch.Tensor]):
    """A tensor's address; null for None and for an empty tensor, which has none."""
    return C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None


def _level_arguments(n_boxes: int, box_index_lo, level_ratio, level_cell_size=_ABSENT,
                     prob_lo=_ABSENT, per_axis: bool = True):
    """(index int32 [n_boxes, 3], ratios int32, sizes float64 or None, origin float64 [3] or
    None) as the native calls that cross levels take them.  level_cell_size is [n_levels, 3], or
    [n_levels] (the sizes along one axis) without per_axis; with it there is one ratio per level
    transition, without it the ratios alone say how many levels there are."""
    index = np.ascontiguousarray(box_index_lo, dtype=np.int32)
    ratios = np.ascontiguousarray(level_ratio, dtype=np.int32)
    sizes = origin = None
    if level_cell_size is not _ABSENT:
        sizes = np.ascontiguousarray(level_cell_size, dtype=np.float64)
    if prob_lo is not _ABSENT:
        origin = np.ascontiguousarray(prob_lo, dtype=np.float64)
    if index.shape != (n_boxes, 3):
        raise ValueError("box_index_lo must hold three values per box")
    if sizes is not None and per_axis:
        if sizes.ndim != 2 or sizes.shape[1] != 3 or sizes.shape[0] < 1:
            raise ValueError("level_cell_size must hold three values per level")
    elif sizes is not None and (sizes.ndim != 1 or sizes.size < 1):
        raise ValueError("level_cell_size must hold one value per level")
    if ratios.ndim != 1 or (sizes is not None and ratios.size != sizes.shape[0] - 1):
        raise ValueError("level_ratio must hold one value per level transition")
    if origin is not None and origin.shape != (3,):
        raise ValueError("prob_lo must hold three values")
    return index, ratios, sizes, origin


def _output(ctx: "Context", given: Optional[torch.Tensor], dtype, shape, name: str,
            fill=torch.empty, wrong_size: Optional[str] = None,
            exact: bool = False) -> torch.Tensor:
    """The caller's output tensor, or a new one made by fill (torch.empty or torch.zeros):
    `dtype` on the context's device, contiguous, with as many elements as `shape` -- of that
    very shape with exact."""
    if given is None:
        given = fill(shape, dtype=dtype, device=ctx.device)
    ctx._check_tensor(given, dtype, name)
    fits = tuple(given.shape) == tuple(shape) if exact else given.numel() == math.prod(shape)
    if not fits:
        raise ValueError(wrong_size or f"{name} has the wrong size")
    return given


def _device_points(ctx: "Context", points, wrong_shape: str) -> torch.Tensor:
    """Points [n, 3] (a tensor, or anything numpy takes) as contiguous float64 on the device."""
    if not isinstance(points, torch.Tensor):
        points = torch.from_numpy(np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3))
    points = points.to(device=ctx.device, dtype=torch.float64).contiguous()
    if points.ndim != 2 or points.shape[1] != 3:
        raise ValueError(wrong_shape)
    return points


def _group_box(lo, hi, dims, periodic):
    """(lo float64 [3], hi float64 [3], dims int32 [3], periodic int32 [3]) of the particle
    groups' calls; periodic is a flag or three."""
    lo = np.ascontiguousarray(lo, dtype=np.float64)
    hi = np.ascontiguousarray(hi, dtype=np.float64)
    _require_triple(lo, "lo")
    _require_triple(hi, "hi")
    dims = np.ascontiguousarray(dims, dtype=np.int32)
    if dims.shape != (3,):
        raise ValueError("dims must hold three values")
    flags = np.ascontiguousarray(np.broadcast_to(np.asarray(periodic, dtype=bool), (3,)),
                                 dtype=np.int32)
    return lo, hi, dims, flags


def group_pair_tests(counts: torch.Tensor, periodic) -> int:
    """The pair tests group_link_kernel makes on a grid whose cells hold counts (int64 [nz, ny,
    nx]) particles: m (m - 1) / 2 inside a cell plus m times the occupancy of each of its 13
    forward neighbours, wrapped on a periodic axis and absent past another face -- as shifted
    products of the dense grid.  Exact; ValueError where it would not fit 63 bits."""
    counts = counts.to(torch.int64)
    flags = [bool(v) for v in np.broadcast_to(np.asarray(periodic, dtype=bool), (3,))]
    terms = [(counts, counts - 1, 2)]
    for e in range(14, 27):
        offset = (e % 3 - 1, (e // 3) % 3 - 1, e // 9 - 1)   # (dx, dy, dz)
        a = b = counts
        for axis, d in zip((2, 1, 0), offset):               # the grid is [nz, ny, nx]
            if d == 0:
                continue
            if flags[2 - axis]:
                b = torch.roll(b, -d, dims=axis)
            else:
                size = a.shape[axis]
                a = a.narrow(axis, 0 if d > 0 else 1, size - 1)
                b = b.narrow(axis, 1 if d > 0 else 0, size - 1)
        terms.append((a, b, 1))
    total = 0
    for a, b, divisor in terms:
        if float((a.double() * b.double()).sum().item()) >= 2.0 ** 62:
            raise ValueError("the link kernel would test more than 2^62 pairs of particles; use "
                             "a smaller linking length")
        total += int((a * b).sum().item()) // divisor
    return total


def _native(ctx: "Context", entry: str, *arguments) -> None:
    """One call of the library on the context's stream, ordered behind torch's current stream
    and ahead of what torch queues next."""
    ctx.join()
    _capi.check(getattr(_capi.lib(), entry)(*arguments))
    ctx.publish()


class Scene:
    """The rank's local boxes + scalar transform (avr_scene).  Keeps the cell tensors alive."""

    def scalar_stats(self) -> Tuple[float, float, float, int]:
        """avr_scene_scalar_stats: (min, max, min positive, finite count) of this rank's cells
        (reduceLocalScalarStats, SceneBuilder.cpp:53-97).  Synchronises."""
        stats = (C.c_double * 3)()
        count = C.c_int64()
        self.ctx.join()
        _capi.check(_capi.lib().avr_scene_scalar_stats(self.ctx._handle, self._handle, stats,
                                                       C.byref(count)))
        return stats[0], stats[1], stats[2], int(count.value)

    def histogram(self, transform: ScalarTransform, range_min: float, range_max: float,
                  bin_count: int, counts: Optional[torch.Tensor] = None) -> torch.Tensor:
        """avr_scene_histogram: adds this rank's cells to counts[bin_count] (int64 on device)."""
        if bin_count <= 0:
            raise ValueError("binCount must be positive")
        counts = _output(self.ctx, counts, torch.int64, (bin_count,), "counts", torch.zeros)
        ctr = transform.to_c()
        _native(self.ctx, "avr_scene_histogram", self.ctx._handle, self._handle, C.byref(ctr),
                float(range_min), float(range_max), int(bin_count), _pointer(counts))
        return counts

    def joint_histogram(self, x_edges, y: Optional["Scene"] = None, y_edges=None,
                        s: Optional["Scene"] = None, n_levels: Optional[int] = None,
                        cells: Optional[torch.Tensor] = None, sums: Optional[torch.Tensor] = None,
                        totals: Optional[torch.Tensor] = None):
        """avr_scene_joint_histogram with this scene as the x field: adds this rank's cells to
        (cells int64 [L, ny, nx], sums float64 [L, ny, nx] or None without s, totals int64 [2] =
        (outside, nonfinite)) on the device.  y and s are scenes of the same context with the same
        box list (other fields of the same cells); without y there is one y bin.  x_edges /
        y_edges: float64, strictly increasing, n + 1 each.  L = n_levels, by default 1 + the
        largest level among this scene's boxes."""
        ctx = self.ctx
        ex = np.ascontiguousarray(x_edges, dtype=np.float64)
        if ex.ndim != 1 or ex.size < 2:
            raise ValueError("x_edges must hold at least two values")
        nx, ny, ey = ex.size - 1, 1, None
        if y is not None:
            if y_edges is None:
                raise ValueError("y_edges must be given with y")
            ey = np.ascontiguousarray(y_edges, dtype=np.float64)
            if ey.ndim != 1 or ey.size < 2:
                raise ValueError("y_edges must hold at least two values")
            ny = ey.size - 1
        elif y_edges is not None:
            raise ValueError("y_edges must be given with y")
        if n_levels is None:
            n_levels = 1 + max((int(b.level) for b in self.boxes), default=0)
        n_levels = int(n_levels)
        if n_levels < 1:
            raise ValueError("n_levels must be positive")
        shape = (n_levels, ny, nx)
        wrong = "cells must be [n_levels, ny, nx] and totals [2]"
        cells = _output(ctx, cells, torch.int64, shape, "cells", torch.zeros, wrong, exact=True)
        totals = _output(ctx, totals, torch.int64, (2,), "totals", torch.zeros, wrong)
        sums = None if s is None else _output(ctx, sums, torch.float64, shape, "sums", torch.zeros,
                                              "sums must be [n_levels, ny, nx]", exact=True)
        _native(ctx, "avr_scene_joint_histogram", ctx._handle, self._handle,
                y._handle if y is not None else None, s._handle if s is not None else None,
                _doubles(ex), int(nx), _doubles(ey) if ey is not None else None, int(ny), n_levels,
                _pointer(cells), _pointer(sums), _pointer(totals))
        return cells, sums, totals

    def slice(self, origin: Sequence[float], du: Sequence[float], dv: Sequence[float], width: int,
              height: int, global_index: Optional[Sequence[int]] = None,
              value: Optional[torch.Tensor] = None, level: Optional[torch.Tensor] = None,
              box: Optional[torch.Tensor] = None):
        """avr_slice_scene: the plane origin + (x + 0.5) du + (y + 0.5) dv (scene coordinates)
        through this scene's boxes -> (value float64, level int8, box int32), [height, width]
        each, row 0 at the bottom: the raw value of the cell that contains the pixel's point, its
        box's level and global_index[its box] (the box's position in this scene if None);
        (0.0, -1, -1) where no box contains the point."""
        width, height = int(width), int(height)
        if width <= 0 or height <= 0:
            raise ValueError("image width and height must be positive")
        vectors = []
        for name, vec in (("origin", origin), ("du", du), ("dv", dv)):
            values = tuple(float(c) for c in vec)
            if len(values) != 3:
                raise ValueError(f"{name} must hold three values")
            vectors.append((C.c_double * 3)(*values))
        index = None
        if global_index is not None:
            index = np.ascontiguousarray(global_index, dtype=np.int32)
            if index.shape != (len(self.boxes),):
                raise ValueError("global_index must hold one entry per box of the scene")
        ctx = self.ctx
        value = _output(ctx, value, torch.float64, (height, width), "value")
        level = _output(ctx, level, torch.int8, (height, width), "level")
        box = _output(ctx, box, torch.int32, (height, width), "box")
        _native(ctx, "avr_slice_scene", ctx._handle, self._handle, *vectors, width, height,
                _ints(index) if index is not None else None, _pointer(value), _pointer(level),
                _pointer(box))
        return value, level, box

    def axis_projection(self, axis: int, origin_uv: Sequence[float], du: float, dv: float,
                        width: int, height: int, level_dl: Sequence[float],
                        weight_scene: Optional["Scene"] = None,
                        integral: Optional[torch.Tensor] = None,
                        weight: Optional[torch.Tensor] = None,
                        length: Optional[torch.Tensor] = None):
        """avr_scene_axis_projection with this scene as the field: the line integral along axis
        (0 = x, 1 = y, 2 = z) through every box that contains the pixel's line u = origin_uv[0] +
        (x + 0.5) du, v = origin_uv[1] + (y + 0.5) dv (scene coordinates; (U, V) = (y, z), (z, x),
        (x, y)), a cell's path length being level_dl[its box's level].  weight_scene: a scene of
        the same context with the same box list, whose cells weight the field's.  Returns
        (integral, weight or None without weight_scene, length), float64 [height, width] on the
        device, row 0 at the bottom; all 0 where no box contains the line."""
        axis, width, height = int(axis), int(width), int(height)
        if axis not in (0, 1, 2):
            raise ValueError("axis must be 0 (x), 1 (y) or 2 (z)")
        if width <= 0 or height <= 0:
            raise ValueError("image width and height must be positive")
        origin = tuple(float(c) for c in origin_uv)
        if len(origin) != 2:
            raise ValueError("origin_uv must hold two values")
        dl = np.ascontiguousarray(level_dl, dtype=np.float64)
        if dl.ndim != 1 or dl.size < 1:
            raise ValueError("level_dl must hold one value per level")
        ctx = self.ctx
        integral = _output(ctx, integral, torch.float64, (height, width), "integral")
        if weight_scene is not None:
            weight = _output(ctx, weight, torch.float64, (height, width), "weight")
        elif weight is not None:
            raise ValueError("weight is given exactly when weight_scene is")
        length = _output(ctx, length, torch.float64, (height, width), "length")
        _native(ctx, "avr_scene_axis_projection", ctx._handle, self._handle,
                weight_scene._handle if weight_scene is not None else None, axis,
                (C.c_double * 2)(*origin), float(du), float(dv), width, height, _doubles(dl),
                int(dl.size), _pointer(integral), _pointer(weight), _pointer(length))
        return integral, weight, length

    def velocity_cube(self, velocity: "Scene", edges, axis: int, origin_uv: Sequence[float],
                      du: float, dv: float, width: int, height: int, level_dl: Sequence[float],
                      width_scene: Optional["Scene"] = None,
                      cube: Optional[torch.Tensor] = None, under: Optional[torch.Tensor] = None,
                      over: Optional[torch.Tensor] = None, length: Optional[torch.Tensor] = None):
        """avr_scene_velocity_cube with this scene as the emission: the on-axis projection of
        Scene.axis_projection (same axis, window, level_dl and row order) split into the channels
        edges[c] <= g < edges[c + 1] (the last closed at the top) of the cells g of `velocity`, a
        scene of the same context with the same box list; width_scene, another such scene, gives a
        cell's 1-sigma width in the units of g, which spreads its share over the channels as a
        Gaussian.  edges: float64, finite, strictly increasing, n + 1 <= 1025 values.  Returns
        (cube [n, height, width], under, over, length [height, width]), float64 on the device;
        all 0 where no box contains the line."""
        axis, width, height = int(axis), int(width), int(height)
        if axis not in (0, 1, 2):
            raise ValueError("axis must be 0 (x), 1 (y) or 2 (z)")
        if width <= 0 or height <= 0:
            raise ValueError("image width and height must be positive")
        origin = tuple(float(c) for c in origin_uv)
        if len(origin) != 2:
            raise ValueError("origin_uv must hold two values")
        dl = np.ascontiguousarray(level_dl, dtype=np.float64)
        if dl.ndim != 1 or dl.size < 1:
            raise ValueError("level_dl must hold one value per level")
        e = np.ascontiguousarray(edges, dtype=np.float64)
        if e.ndim != 1 or e.size < 2:
            raise ValueError("edges must hold at least two values")
        n = int(e.size) - 1
        ctx = self.ctx
        cube = _output(ctx, cube, torch.float64, (n, height, width), "cube")
        under = _output(ctx, under, torch.float64, (height, width), "under")
        over = _output(ctx, over, torch.float64, (height, width), "over")
        length = _output(ctx, length, torch.float64, (height, width), "length")
        _native(ctx, "avr_scene_velocity_cube", ctx._handle, self._handle, velocity._handle,
                width_scene._handle if width_scene is not None else None, axis,
                (C.c_double * 2)(*origin), float(du), float(dv), width, height, _doubles(dl),
                int(dl.size), _doubles(e), n, _pointer(cube), _pointer(under), _pointer(over),
                _pointer(length))
        return cube, under, over, length

    def derive(self, inputs: Sequence["Scene"], instructions, constants, box_origin,
               level_cell_size) -> None:
        """avr_scene_derive with this scene as the output: overwrites the cells of this scene's
        boxes with the program's value per cell.  inputs: up to six scenes of the same context with
        the same box list (the program's fields, in order); instructions: uint32 words; constants:
        float64; box_origin: [n_boxes, 3] float64, the physical position of every box's low
        corner; level_cell_size: [n_levels, 3] float64.  This scene's cells must not overlap any
        input's.  Asynchronous on the context's stream."""
        ctx = self.ctx
        inputs = list(inputs)
        code = np.ascontiguousarray(instructions, dtype=np.uint32)
        consts = np.ascontiguousarray(constants, dtype=np.float64)
        origin = np.ascontiguousarray(box_origin, dtype=np.float64)
        sizes = np.ascontiguousarray(level_cell_size, dtype=np.float64)
        if code.ndim != 1 or consts.ndim != 1:
            raise ValueError("instructions and constants must be one-dimensional")
        if origin.shape != (len(self.boxes), 3):
            raise ValueError("box_origin must hold three values per box")
        if sizes.ndim != 2 or sizes.shape[1] != 3 or sizes.shape[0] < 1:
            raise ValueError("level_cell_size must hold three values per level")
        handles = (C.c_void_p * max(len(inputs), 1))(*[s._handle.value for s in inputs])
        _native(ctx, "avr_scene_derive", ctx._handle, handles, len(inputs), self._handle,
                code.ctypes.data_as(C.POINTER(C.c_uint32)), int(code.size), _doubles(consts),
                int(consts.size), _doubles(origin), _doubles(sizes), int(sizes.shape[0]))

    def gradient(self, field: "Scene", axis: int, box_index_lo, level_ratio,
                 level_cell_size) -> None:
        """avr_scene_gradient with this scene as the output: overwrites the cells of this scene's
        boxes with the difference of `field` (a scene of the same context with the same box list)
        along axis (0 = x, 1 = y, 2 = z).  box_index_lo: [n_boxes, 3] int32, the index of every
        box's first cell in its level's index space; level_ratio: n_levels - 1 ints; level_cell_size:
        n_levels float64, the cell size along the axis.  This scene's cells must not overlap the
        field's.  Asynchronous on the context's stream."""
        ctx = self.ctx
        index, ratios, sizes, _ = _level_arguments(len(self.boxes), box_index_lo, level_ratio,
                                                   level_cell_size, per_axis=False)
        _native(ctx, "avr_scene_gradient", ctx._handle, field._handle, self._handle, int(axis),
                _ints(index), _ints(ratios), _doubles(sizes), int(sizes.size))

    def clumps(self, field: "Scene", lower: float, upper: float, box_index_lo, level_ratio,
               count: Optional[torch.Tensor] = None) -> torch.Tensor:
        """avr_scene_clumps with this scene as the output: overwrites the cells of this scene's
        boxes with the clump labels of `field` (a scene of the same context with the same box
        list) over lower <= v <= upper: f64(label) in 1..N for a selected cell, +0.0 otherwise.
        box_index_lo: [n_boxes, 3] int32; level_ratio: n_levels - 1 ints.  Returns the number of
        clumps N as a one-element int64 tensor on the device (count, if given).  This scene's
        cells must not overlap the field's.  Asynchronous on the context's stream."""
        ctx = self.ctx
        index, ratios, _, _ = _level_arguments(len(self.boxes), box_index_lo, level_ratio)
        count = _output(ctx, count, torch.int64, (1,), "count", torch.zeros,
                        "count must hold one value")
        _native(ctx, "avr_scene_clumps", ctx._handle, field._handle, self._handle, float(lower),
                float(upper), _ints(index), _ints(ratios), int(ratios.size) + 1, _pointer(count))
        return count

    def clump_table(self, n_clumps: int, n_levels: int, field: Optional["Scene"] = None,
                    cells: Optional[torch.Tensor] = None, sums: Optional[torch.Tensor] = None,
                    totals: Optional[torch.Tensor] = None):
        """avr_scene_clump_table with this scene as the labels: per level and label the number of
        cells and, with `field` (a scene of the same context with the same box list), the sum of
        its values.  Returns (cells int64 [n_levels, n_clumps], sums float64 of the same shape or
        None without field, totals int64 [2]: labels that are no integer in [1, n_clumps], field
        values that are not finite) on the device; tensors handed in are added to."""
        ctx = self.ctx
        n_clumps, n_levels = int(n_clumps), int(n_levels)
        if n_clumps < 1 or n_levels < 1:
            raise ValueError("n_clumps and n_levels must be at least 1")
        shape = (n_levels, n_clumps)
        wrong = "cells must be [n_levels, n_clumps] and totals hold two values"
        cells = _output(ctx, cells, torch.int64, shape, "cells", torch.zeros, wrong, exact=True)
        totals = _output(ctx, totals, torch.int64, (2,), "totals", torch.zeros, wrong)
        if field is not None:
            sums = _output(ctx, sums, torch.float64, shape, "sums", torch.zeros,
                           "sums must be [n_levels, n_clumps]", exact=True)
        elif sums is not None:
            raise ValueError("sums is given exactly when field is")
        _native(ctx, "avr_scene_clump_table", ctx._handle, self._handle,
                field._handle if field is not None else None, n_clumps, n_levels, _pointer(cells),
                _pointer(sums), _pointer(totals))
        return cells, sums, totals

    def clump_links(self, n_clumps: int, box_index_lo, level_ratio,
                    parents: Optional["Scene"] = None, n_parents: int = 0,
                    extent: Optional[torch.Tensor] = None,
                    parent_lo: Optional[torch.Tensor] = None,
                    parent_hi: Optional[torch.Tensor] = None,
                    totals: Optional[torch.Tensor] = None):
        """avr_scene_clump_links with this scene as the labels: per label the index bounding box
        in the finest level's index space and, with `parents` (the label scene of a selection that
        contains this one, same context and box list, labels 1..n_parents), the smallest and the
        largest parent label its cells carry.  box_index_lo: [n_boxes, 3] int32; level_ratio:
        n_levels - 1 ints.  Returns (extent int32 [6, n_clumps]: lows of x, y, z, then highs,
        inclusive; parent_lo, parent_hi uint32 [n_clumps] or None without parents; totals int64
        [2]: labels that are no integer in [1, n_clumps], parent labels that are none in [1,
        n_parents]) on the device.  Tensors handed in are combined into (min / max, totals added
        to); new ones start at INT32_MAX / INT32_MIN, UINT32_MAX / 0 and 0.  Asynchronous on the
        context's stream."""
        ctx = self.ctx
        n_clumps, n_parents = int(n_clumps), int(n_parents)
        if n_clumps < 1:
            raise ValueError("n_clumps must be at least 1")
        if (parents is None) != (n_parents == 0) or n_parents < 0:
            raise ValueError("n_parents is at least 1 with parents and 0 without")
        index, ratios, _, _ = _level_arguments(len(self.boxes), box_index_lo, level_ratio)

        def ends(shape, dtype, low, high):
            made = torch.empty(shape, dtype=dtype, device=ctx.device)
            made[:shape[0] // 2] = low
            made[shape[0] // 2:] = high
            return made

        wrong = "extent must be [6, n_clumps] and totals hold two values"
        if extent is None:
            extent = ends((6, n_clumps), torch.int32, 2 ** 31 - 1, -2 ** 31)
        extent = _output(ctx, extent, torch.int32, (6, n_clumps), "extent", wrong_size=wrong,
                         exact=True)
        totals = _output(ctx, totals, torch.int64, (2,), "totals", torch.zeros, wrong)
        if parents is not None:
            wrong = "parent_lo and parent_hi must hold n_clumps values"
            if parent_lo is None:       # all bits set: UINT32_MAX
                parent_lo = torch.full((n_clumps,), -1, dtype=torch.int32,
                                       device=ctx.device).view(torch.uint32)
            if parent_hi is None:
                parent_hi = torch.zeros((n_clumps,), dtype=torch.int32,
                                        device=ctx.device).view(torch.uint32)
            parent_lo = _output(ctx, parent_lo, torch.uint32, (n_clumps,), "parent_lo",
                                wrong_size=wrong)
            parent_hi = _output(ctx, parent_hi, torch.uint32, (n_clumps,), "parent_hi",
                                wrong_size=wrong)
        elif parent_lo is not None or parent_hi is not None:
            raise ValueError("parent_lo and parent_hi are given exactly when parents is")
        _native(ctx, "avr_scene_clump_links", ctx._handle, self._handle,
                parents._handle if parents is not None else None, n_clumps, n_parents,
                _ints(index), _ints(ratios), int(ratios.size) + 1, _pointer(extent),
                _pointer(parent_lo), _pointer(parent_hi), _pointer(totals))
        return extent, parent_lo, parent_hi, totals

    def clump_members(self, n_clumps: int, wanted, capacity: int,
                      totals: Optional[torch.Tensor] = None):
        """avr_scene_clump_members with this scene as the labels: the keys (label - 1) << 32 |
        cell ordinal of the cells whose label c has wanted[c - 1] != 0 (wanted: n_clumps bytes, a
        tensor on the device or anything numpy takes), sorted ascending -- by label, then by
        ordinal: the canonical member list ("Clump binding").  capacity: the number
        of members, which the caller knows from the clump table; ValueError if the kernel counts
        another number.  Returns (keys int64 [capacity], totals int64 [1]: labels that are no
        integer in [1, n_clumps], added to a tensor handed in) on the device.  Synchronises, to
        read the count."""
        ctx = self.ctx
        n_clumps, capacity = int(n_clumps), int(capacity)
        if n_clumps < 1:
            raise ValueError("n_clumps must be at least 1")
        if not isinstance(wanted, torch.Tensor):
            wanted = torch.from_numpy(np.ascontiguousarray(wanted).astype(np.uint8).reshape(-1))
        wanted = wanted.to(device=ctx.device, dtype=torch.uint8).contiguous()
        if wanted.numel() != n_clumps:
            raise ValueError("wanted must hold one byte per label")
        totals = _output(ctx, totals, torch.int64, (1,), "totals", torch.zeros,
                         "totals must hold one value")
        if capacity == 0 and not bool(wanted.any().item()):
            return torch.zeros(0, dtype=torch.int64, device=ctx.device), totals
        keys = torch.empty(max(capacity, 1), dtype=torch.int64, device=ctx.device)
        count = torch.zeros(1, dtype=torch.int64, device=ctx.device)
        _native(ctx, "avr_scene_clump_members", ctx._handle, self._handle, n_clumps,
                _pointer(wanted), max(capacity, 1), _pointer(keys), _pointer(count),
                _pointer(totals))
        found = int(count.item())
        if found != capacity:
            raise ValueError(f"the label scene holds {found} member cells, not the {capacity} "
                             "its table counted")
        # keys are below 2^60: the signed order is the unsigned one
        return torch.sort(keys[:capacity]).values, totals

    def clump_member_data(self, keys: torch.Tensor, box_index_lo, level_ratio, level_cell_size,
                          prob_lo, field: Optional["Scene"] = None, centres: bool = True):
        """avr_scene_clump_member_data with this scene's boxes: per key of clump_members (int64
        [n] on the device) the level and centre of its cell (centres=True) and/or the raw value
        of `field` (a scene of the same context with the same box list) there.  box_index_lo,
        level_ratio, level_cell_size and prob_lo as isosurface takes them.  Returns (levels uint8
        [n] or None, centres float64 [3, n] or None, values float64 [n] or None) on the device.
        Asynchronous on the context's stream."""
        ctx = self.ctx
        ctx._check_tensor(keys, torch.int64, "keys")
        if keys.ndim != 1:
            raise ValueError("keys must be one-dimensional")
        if field is None and not centres:
            raise ValueError("no output is asked for")
        n = int(keys.numel())
        index, ratios, sizes, origin = _level_arguments(len(self.boxes), box_index_lo, level_ratio,
                                                        level_cell_size, prob_lo)
        levels = torch.empty(n, dtype=torch.uint8, device=ctx.device) if centres else None
        where = torch.empty((3, n), dtype=torch.float64, device=ctx.device) if centres else None
        values = torch.empty(n, dtype=torch.float64, device=ctx.device) \
            if field is not None else None
        if n == 0:      # nothing to look up, and a tensor without elements has no address
            return levels, where, values
        _native(ctx, "avr_scene_clump_member_data", ctx._handle, self._handle, _pointer(keys), n,
                field._handle if field is not None else None, _pointer(values), _ints(index),
                _ints(ratios), _doubles(sizes), _doubles(origin), int(sizes.shape[0]),
                _pointer(where), _pointer(levels))
        return levels, where, values

    def isosurface(self, value: float, box_index_lo, level_ratio, level_cell_size, prob_lo,
                   sample: Optional["Scene"] = None, capacity: int = 0,
                   counts: Optional[torch.Tensor] = None):
        """avr_scene_isosurface with this scene as the field: the isosurface field == value by
        marching tetrahedra.  box_index_lo: [n_boxes, 3] int32; level_ratio: n_levels - 1 ints;
        level_cell_size: [n_levels, 3] float64; prob_lo: three values; sample: a scene of the
        same context with the same box list, interpolated at every vertex.  capacity == 0 only
        counts.  Returns (counts int64 [2] on the device: triangles T and skipped cubes,
        vertices float64 [capacity, 3, 3], levels uint8 [capacity], samples float64 [capacity, 3]
        or None without sample); the three arrays are None with capacity == 0 and written iff
        T <= capacity.  Asynchronous on the context's stream."""
        ctx = self.ctx
        index, ratios, sizes, origin = _level_arguments(len(self.boxes), box_index_lo,
                                                        level_ratio, level_cell_size, prob_lo)
        capacity = int(capacity)
        if capacity < 0:
            raise ValueError("capacity must not be negative")
        counts = _output(ctx, counts, torch.int64, (2,), "counts", torch.zeros,
                         "counts must hold two values")
        vertices = levels = samples = None
        if capacity > 0:
            vertices = torch.empty((capacity, 3, 3), dtype=torch.float64, device=ctx.device)
            levels = torch.empty(capacity, dtype=torch.uint8, device=ctx.device)
            if sample is not None:
                samples = torch.empty((capacity, 3), dtype=torch.float64, device=ctx.device)
        _native(ctx, "avr_scene_isosurface", ctx._handle, self._handle,
                sample._handle if sample is not None else None, float(value), _ints(index),
                _ints(ratios), _doubles(sizes), _doubles(origin), int(sizes.shape[0]), capacity,
                _pointer(vertices), _pointer(levels), _pointer(samples), _pointer(counts))
        return counts, vertices, levels, samples

    def streamlines(self, vy: "Scene", vz: "Scene", seeds, step: float, direction: int,
                    max_steps: int, box_index_lo, level_ratio, level_cell_size, prob_lo,
                    sample: Optional["Scene"] = None):
        """avr_scene_streamlines with this scene as the x component: RK4 field lines of (this
        scene, vy, vz) -- scenes of the same context with the same box list -- from seeds
        (float64 [n, 3] in physical units; a tensor on the device, or anything numpy takes).
        step in (0, 1] cell sizes of the leaf; direction +1 or -1; box_index_lo: [n_boxes, 3]
        int32; level_ratio: n_levels - 1 ints; level_cell_size: [n_levels, 3] float64; prob_lo:
        three values; sample: a scene with the same box list, interpolated at every point.
        Returns (points float64 [n, max_steps + 1, 3], samples float64 [n, max_steps + 1] or None
        without sample, counts int32 [n], status uint8 [n]: 0 max_steps reached, 1 outside, 2
        stagnant, 3 not finite) on the device; points and samples past a line's count are NaN.
        Asynchronous on the context's stream."""
        ctx = self.ctx
        index, ratios, sizes, origin = _level_arguments(len(self.boxes), box_index_lo,
                                                        level_ratio, level_cell_size, prob_lo)
        max_steps = int(max_steps)
        if max_steps < 0:
            raise ValueError("max_steps must not be negative")
        seeds = _device_points(ctx, seeds, "seeds must hold three values per seed")
        n = int(seeds.shape[0])
        points = torch.full((n, max_steps + 1, 3), math.nan, dtype=torch.float64,
                            device=ctx.device)
        samples = None
        if sample is not None:
            samples = torch.full((n, max_steps + 1), math.nan, dtype=torch.float64,
                                 device=ctx.device)
        counts = torch.zeros(n, dtype=torch.int32, device=ctx.device)
        status = torch.zeros(n, dtype=torch.uint8, device=ctx.device)
        if n == 0:                     # nothing to launch, and empty tensors have no address
            return points, samples, counts, status
        _native(ctx, "avr_scene_streamlines", ctx._handle, self._handle, vy._handle, vz._handle,
                sample._handle if sample is not None else None, _pointer(seeds), n, float(step),
                int(direction), max_steps, _ints(index), _ints(ratios), _doubles(sizes),
                _doubles(origin), int(sizes.shape[0]), _pointer(points), _pointer(samples),
                _pointer(counts), _pointer(status))
        return points, samples, counts, status

    def rays(self, start, end, max_trips: int, box_index_lo, level_ratio, level_cell_size,
             prob_lo, offsets: Optional[torch.Tensor] = None, n_segments: int = 0):
        """avr_scene_rays with this scene as the field: the leaf cells that the segments start[s]
        -> end[s] cross (float64 [n, 3] in physical units; tensors on the device, or anything
        numpy takes).  max_trips in [1, 2^30]; box_index_lo: [n_boxes, 3] int32; level_ratio:
        n_levels - 1 ints; level_cell_size: [n_levels, 3] float64; prob_lo: three values.
        Without offsets it is the count pass and returns (counts int32 [n], status uint8 [n]: 0
        complete, 1 miss, 2 max_trips reached, 3 invalid, span float64 [n, 2]: t_enter and
        t_leave, NaN for status 1 and 3).  With offsets (int64 [n + 1] on the device: the
        exclusive scan of the counts and their total) and n_segments (that total) it is the emit
        pass and returns (t0, t1 float64 [n_segments], level int8 [n_segments], value float64
        [n_segments], integral, covered float64 [n]).  Everything is on the device;
        asynchronous on the context's stream."""
        ctx = self.ctx
        index, ratios, sizes, origin = _level_arguments(len(self.boxes), box_index_lo,
                                                        level_ratio, level_cell_size, prob_lo)
        max_trips, n_segments = int(max_trips), int(n_segments)
        if not 1 <= max_trips <= 2 ** 30:
            raise ValueError("max_trips must lie in [1, 2^30]")
        if n_segments < 0:
            raise ValueError("n_segments must not be negative")
        start = _device_points(ctx, start, "start and end must hold three values per ray")
        end = _device_points(ctx, end, "start and end must hold three values per ray")
        if start.shape != end.shape:
            raise ValueError("start and end must hold the same number of rays")
        n = int(start.shape[0])
        emit = offsets is not None
        if emit:
            ctx._check_tensor(offsets, torch.int64, "offsets")
            if offsets.numel() != n + 1:
                raise ValueError("offsets must hold n + 1 values")
            t0 = torch.empty(n_segments, dtype=torch.float64, device=ctx.device)
            t1 = torch.empty(n_segments, dtype=torch.float64, device=ctx.device)
            level = torch.empty(n_segments, dtype=torch.int8, device=ctx.device)
            value = torch.empty(n_segments, dtype=torch.float64, device=ctx.device)
            integral = torch.zeros(n, dtype=torch.float64, device=ctx.device)
            covered = torch.zeros(n, dtype=torch.float64, device=ctx.device)
            counts = status = span = None
            result = (t0, t1, level, value, integral, covered)
        else:
            counts = torch.zeros(n, dtype=torch.int32, device=ctx.device)
            status = torch.full((n,), 3, dtype=torch.uint8, device=ctx.device)
            span = torch.full((n, 2), math.nan, dtype=torch.float64, device=ctx.device)
            t0 = t1 = level = value = integral = covered = None
            result = (counts, status, span)
        if n == 0:                     # nothing to launch, and empty tensors have no address
            return result
        _native(ctx, "avr_scene_rays", ctx._handle, self._handle, _pointer(start), _pointer(end),
                n, max_trips, _ints(index), _ints(ratios), _doubles(sizes), _doubles(origin),
                int(sizes.shape[0]), _pointer(offsets), n_segments, _pointer(counts),
                _pointer(status), _pointer(span), _pointer(t0), _pointer(t1), _pointer(level),
                _pointer(value), _pointer(integral), _pointer(covered))
        return result

    def ray_sums(self, start, end, max_trips: int, box_index_lo, level_ratio, level_cell_size,
                 prob_lo, weight: Optional["Scene"] = None):
        """avr_scene_ray_sums with this scene as the field: Scene.rays' walk once, with nothing
        stored per segment ("Off-axis projection").  The arguments are Scene.rays';
        weight: a scene of the same context with the same boxes, or None.  Returns (counts int32
        [n], status uint8 [n], span float64 [n, 2]) as Scene.rays' count pass gives them and
        (integral, weight sum or None without weight, counted, covered), float64 [n]: over the
        leaf segments in walk order, w being a segment's length, covered = sum w; without weight
        integral = sum v w and counted = sum w where the value v is finite; with it integral =
        sum (v q) w, weight sum = sum q w and counted = sum w where v and the weight's value q
        are both finite.  Everything is on the device; asynchronous on the context's stream."""
        ctx = self.ctx
        index, ratios, sizes, origin = _level_arguments(len(self.boxes), box_index_lo,
                                                        level_ratio, level_cell_size, prob_lo)
        max_trips = int(max_trips)
        if not 1 <= max_trips <= 2 ** 30:
            raise ValueError("max_trips must lie in [1, 2^30]")
        if weight is not None and weight.ctx is not ctx:
            raise ValueError("the weight scene belongs to another context")
        start = _device_points(ctx, start, "start and end must hold three values per ray")
        end = _device_points(ctx, end, "start and end must hold three values per ray")
        if start.shape != end.shape:
            raise ValueError("start and end must hold the same number of rays")
        n = int(start.shape[0])
        counts = torch.zeros(n, dtype=torch.int32, device=ctx.device)
        status = torch.full((n,), 3, dtype=torch.uint8, device=ctx.device)
        span = torch.full((n, 2), math.nan, dtype=torch.float64, device=ctx.device)
        integral = torch.zeros(n, dtype=torch.float64, device=ctx.device)
        weight_sum = None
        if weight is not None:
            weight_sum = torch.zeros(n, dtype=torch.float64, device=ctx.device)
        counted = torch.zeros(n, dtype=torch.float64, device=ctx.device)
        covered = torch.zeros(n, dtype=torch.float64, device=ctx.device)
        result = (counts, status, span, integral, weight_sum, counted, covered)
        if n == 0:                     # nothing to launch, and empty tensors have no address
            return result
        _native(ctx, "avr_scene_ray_sums", ctx._handle, self._handle,
                weight._handle if weight is not None else None, _pointer(start), _pointer(end), n,
                max_trips, _ints(index), _ints(ratios), _doubles(sizes), _doubles(origin),
                int(sizes.shape[0]), _pointer(counts), _pointer(status), _pointer(span),
                _pointer(integral), _pointer(weight_sum), _pointer(counted), _pointer(covered))
        return result

    def ray_transfer(self, opacity: "Scene", start, end, max_trips: int, box_index_lo, level_ratio,
                     level_cell_size, prob_lo, bin_scene: Optional["Scene"] = None,
                     width_scene: Optional["Scene"] = None, edges=None):
        """avr_scene_ray_transfer with this scene as the source function: emission and absorption
        along Scene.ray_sums' walk, nearest cell first ("Ray transfer").  opacity,
        bin_scene (the field the channels bin, or None: grey) and width_scene (a 1-sigma width in
        the bin field's units, or None; only with bin_scene): scenes of the same context with the
        same boxes.  edges: the nc + 1 channel edges, given exactly with bin_scene; grey has one
        channel.  The other arguments are Scene.rays'.  Returns (counts int32 [n], status uint8
        [n], span float64 [n, 2]) as Scene.rays' count pass gives them, (intensity, tau) float64
        [nc, n], outside float64 [2, n] (the optical depth below edges[0] and above edges[nc]; None
        for grey) and (counted, covered) float64 [n].  Everything is on the device; asynchronous
        on the context's stream."""
        ctx = self.ctx
        index, ratios, sizes, origin = _level_arguments(len(self.boxes), box_index_lo,
                                                        level_ratio, level_cell_size, prob_lo)
        max_trips = int(max_trips)
        if not 1 <= max_trips <= 2 ** 30:
            raise ValueError("max_trips must lie in [1, 2^30]")
        if opacity is None:
            raise ValueError("ray_transfer needs an opacity scene")
        if width_scene is not None and bin_scene is None:
            raise ValueError("a width scene needs a bin scene")
        if (bin_scene is None) != (edges is None):
            raise ValueError("edges are given exactly with a bin scene")
        for other in (opacity, bin_scene, width_scene):
            if other is not None and other.ctx is not ctx:
                raise ValueError("the scenes belong to different contexts")
        e, nc = None, 1
        if edges is not None:
            e = np.ascontiguousarray(edges, dtype=np.float64)
            if e.ndim != 1 or e.size < 2:
                raise ValueError("edges must hold at least two values")
            nc = int(e.size) - 1
        start = _device_points(ctx, start, "start and end must hold three values per ray")
        end = _device_points(ctx, end, "start and end must hold three values per ray")
        if start.shape != end.shape:
            raise ValueError("start and end must hold the same number of rays")
        n = int(start.shape[0])
        if nc * n >= 2 ** 31:
            raise ValueError("the channels of all rays are 2^31 entries or more")
        counts = torch.zeros(n, dtype=torch.int32, device=ctx.device)
        status = torch.full((n,), 3, dtype=torch.uint8, device=ctx.device)
        span = torch.full((n, 2), math.nan, dtype=torch.float64, device=ctx.device)
        intensity = torch.zeros((nc, n), dtype=torch.float64, device=ctx.device)
        tau = torch.zeros((nc, n), dtype=torch.float64, device=ctx.device)
        outside = None
        if bin_scene is not None:
            outside = torch.zeros((2, n), dtype=torch.float64, device=ctx.device)
        counted = torch.zeros(n, dtype=torch.float64, device=ctx.device)
        covered = torch.zeros(n, dtype=torch.float64, device=ctx.device)
        result = (counts, status, span, intensity, tau, outside, counted, covered)
        if n == 0:                     # nothing to launch, and empty tensors have no address
            return result
        _native(ctx, "avr_scene_ray_transfer", ctx._handle, self._handle, opacity._handle,
                bin_scene._handle if bin_scene is not None else None,
                width_scene._handle if width_scene is not None else None, _pointer(start),
                _pointer(end), n, max_trips, _ints(index), _ints(ratios), _doubles(sizes),
                _doubles(origin), int(sizes.shape[0]), _doubles(e) if e is not None else None, nc,
                _pointer(counts), _pointer(status), _pointer(span), _pointer(intensity),
                _pointer(tau), _pointer(outside), _pointer(counted), _pointer(covered))
        return result

    def covering_grid(self, level: int, lo, dims, box_index_lo, level_ratio,
                      fill: float = math.nan, with_coverage: bool = True):
        """avr_scene_covering_grid with this scene as the field: the field resampled to the cells
        [lo, lo + dims) of level `level` -- a leaf of the same or a coarser level gives its value,
        finer leaves their volume-weighted mean, and a cell no leaf touches gives fill.  lo, dims:
        three ints each, dims as (nx, ny, nz); box_index_lo: [n_boxes, 3] int32; level_ratio:
        n_levels - 1 ints, n_levels counting the levels up to the finer of `level` and the finest
        box level.  Returns (values float64 [nz, ny, nx], coverage float64 [nz, ny, nx], cell
        level int8 [nz, ny, nx]) on the device; the last two are None without with_coverage.
        Asynchronous on the context's stream."""
        ctx = self.ctx
        index, ratios, _, _ = _level_arguments(len(self.boxes), box_index_lo, level_ratio)
        first = np.ascontiguousarray(lo, dtype=np.int64)
        extent = np.ascontiguousarray(dims, dtype=np.int64)
        if first.shape != (3,) or extent.shape != (3,):
            raise ValueError("lo and dims must hold three values")
        if (extent < 1).any() or (extent > 2 ** 31 - 1).any() or (abs(first) > 2 ** 31 - 1).any():
            raise ValueError("dims must be at least 1 (and lo and dims fit 32 bits)")
        nx, ny, nz = (int(v) for v in extent)
        if nx * ny * nz >= 2 ** 31:
            raise ValueError("the region has 2^31 cells or more")
        first, extent = first.astype(np.int32), extent.astype(np.int32)
        values = torch.empty((nz, ny, nx), dtype=torch.float64, device=ctx.device)
        coverage = cell_level = None
        if with_coverage:
            coverage = torch.empty((nz, ny, nx), dtype=torch.float64, device=ctx.device)
            cell_level = torch.empty((nz, ny, nx), dtype=torch.int8, device=ctx.device)
        _native(ctx, "avr_scene_covering_grid", ctx._handle, self._handle, int(level),
                _ints(first), _ints(extent), _ints(index), _ints(ratios), int(ratios.size) + 1,
                float(fill), _pointer(values), _pointer(coverage), _pointer(cell_level))
        return values, coverage, cell_level

    def grid_field(self, grid: torch.Tensor, level: int, lo, box_index_lo, level_ratio,
                   interpolation: int = 0, periodic: bool = False, fill: float = math.nan,
                   totals: Optional[torch.Tensor] = None) -> torch.Tensor:
        """avr_scene_grid_field with this scene as the output: overwrites the cells of this scene's
        boxes with the uniform grid `grid` (float64 [nz, ny, nx], contiguous, on the device) of the
        level-`level` cells from the index lo on -- the grid's own value where a box is of that
        level, the value of the grid cell that holds it (interpolation 0) or the trilinear
        interpolation between the grid's cell centres (1; past the region's faces wrapped with
        periodic, clamped without) where it is finer, the mean of the grid cells inside it where it
        is coarser, and fill where the grid does not reach.  box_index_lo: [n_boxes, 3] int32;
        level_ratio: n_levels - 1 ints, n_levels counting the levels up to the finer of `level`
        and the finest box level.  Returns totals, int64 [2] on the device (a tensor handed in is
        added to): the cells that got fill, and the coarser cells only part of which the grid
        covers.  The grid must not overlap this scene's cells.  Asynchronous on the context's
        stream."""
        ctx = self.ctx
        index, ratios, _, _ = _level_arguments(len(self.boxes), box_index_lo, level_ratio)
        first = np.ascontiguousarray(lo, dtype=np.int64)
        if first.shape != (3,) or (abs(first) > 2 ** 31 - 1).any():
            raise ValueError("lo must hold three values that fit 32 bits")
        ctx._check_tensor(grid, torch.float64, "grid")
        if grid.ndim != 3 or grid.numel() == 0:
            raise ValueError("grid must be [nz, ny, nx] with at least one cell")
        if grid.numel() >= 2 ** 31:
            raise ValueError("the region has 2^31 cells or more")
        interpolation = int(interpolation)
        if interpolation not in (0, 1):
            raise ValueError("interpolation must be 0 (constant) or 1 (linear)")
        nz, ny, nx = (int(v) for v in grid.shape)
        extent = np.array([nx, ny, nz], dtype=np.int32)
        totals = _output(ctx, totals, torch.int64, (2,), "totals", torch.zeros,
                         "totals must hold two values")
        _native(ctx, "avr_scene_grid_field", ctx._handle, self._handle, _pointer(grid), int(level),
                _ints(first.astype(np.int32)), _ints(extent), _ints(index), _ints(ratios),
                int(ratios.size) + 1, interpolation, int(bool(periodic)), float(fill),
                _pointer(totals))
        return totals

    def particle_cells(self, points, values, method: int, box_index_lo, level_ratio,
                       level_cell_size, prob_lo, levels: bool = False,
                       totals: Optional[torch.Tensor] = None):
        """avr_scene_particle_cells with this scene's boxes: the contributions of the particles at
        points (float64 [n, 3] in physical units; a tensor on the device, or anything numpy takes)
        with values (float64 [n] likewise, or None: 1.0 each) to the cells of this scene's boxes,
        method 0 (nearest grid point, one entry per particle) or 1 (cloud in cell, eight).
        box_index_lo, level_ratio, level_cell_size and prob_lo as streamlines takes them.  Returns
        (cells int64 [n, C] -- cell ordinals, 0xFFFFFFFF for a particle outside --, shares float64
        [n, C], levels uint8 [n] (255 outside) or None without levels, totals int64 [2]: outside
        particles and rerouted corner shares; a tensor handed in is added to) on the device.
        Asynchronous on the context's stream."""
        ctx = self.ctx
        index, ratios, sizes, origin = _level_arguments(len(self.boxes), box_index_lo,
                                                        level_ratio, level_cell_size, prob_lo)
        method = int(method)
        if method not in (0, 1):
            raise ValueError("method must be 0 (nearest grid point) or 1 (cloud in cell)")
        points = _device_points(ctx, points, "points must hold three values per particle")
        n = int(points.shape[0])
        if values is not None:
            if not isinstance(values, torch.Tensor):
                values = torch.from_numpy(np.ascontiguousarray(values, dtype=np.float64))
            values = values.to(device=ctx.device, dtype=torch.float64).contiguous()
            if tuple(values.shape) != (n,):
                raise ValueError("values must hold one value per particle")
        entries = 8 if method == 1 else 1
        cells = torch.empty((n, entries), dtype=torch.int64, device=ctx.device)
        shares = torch.empty((n, entries), dtype=torch.float64, device=ctx.device)
        level_of = torch.empty(n, dtype=torch.uint8, device=ctx.device) if levels else None
        totals = _output(ctx, totals, torch.int64, (2,), "totals", torch.zeros,
                         "totals must hold two values")
        _native(ctx, "avr_scene_particle_cells", ctx._handle, self._handle, _pointer(points), n,
                _pointer(values), method, _ints(index), _ints(ratios), _doubles(sizes),
                _doubles(origin), int(sizes.shape[0]), _pointer(cells), _pointer(shares),
                _pointer(level_of), _pointer(totals))
        return cells, shares, level_of, totals

    def particle_deposit(self, cells: torch.Tensor, shares: torch.Tensor, quantity: int,
                         level_cell_size) -> None:
        """avr_scene_particle_deposit with this scene as the output: overwrites every cell of
        this scene's boxes with the sum of the shares that name it -- particle_cells' entries
        (int64 and float64 tensors of one shape on the device), sorted here by cell with a stable
        sort, so that a cell's shares are added in list order -- or, with quantity 1, that sum
        over the volume of a cell of the box's level (level_cell_size: [n_levels, 3] float64).  A
        cell nothing names gets +0.0.  Asynchronous on the context's stream."""
        ctx = self.ctx
        ctx._check_tensor(cells, torch.int64, "cells")
        ctx._check_tensor(shares, torch.float64, "shares")
        if tuple(cells.shape) != tuple(shares.shape):
            raise ValueError("cells and shares must have one shape")
        quantity = int(quantity)
        if quantity not in (0, 1):
            raise ValueError("quantity must be 0 (sum) or 1 (density)")
        sizes = np.ascontiguousarray(level_cell_size, dtype=np.float64)
        if sizes.ndim != 2 or sizes.shape[1] != 3 or sizes.shape[0] < 1:
            raise ValueError("level_cell_size must hold three values per level")
        n = int(cells.numel())
        ordered = picked = None
        if n:
            # stable: equal cells stay in list order, the order the definition adds them in
            ordered, order = torch.sort(cells.reshape(-1), stable=True)
            picked = shares.reshape(-1)[order]
        _native(ctx, "avr_scene_particle_deposit", ctx._handle, self._handle, _pointer(ordered),
                _pointer(picked), n, quantity, _doubles(sizes), int(sizes.shape[0]))

    def set_classification_cache(self, enabled: bool) -> None:
        """avr_scene_set_classification_cache: keep classified volumes across frames while the
        boxes, the scalar transform and the scalar range are unchanged (off by default)."""
        _capi.check(_capi.lib().avr_scene_set_classification_cache(self._handle, int(bool(enabled))))

    def invalidate(self) -> None:
        """avr_scene_invalidate: the cells were changed in place."""
        _capi.check(_capi.lib().avr_scene_invalidate(self._handle))

    def classify_plan(self, ctx: "Context", plan, slot: int) -> None:
        """avr_classify_plan on `ctx`'s stream: cells -> table indices into classified volume
        `slot`.  No stream ordering is added here; the caller orders it against the march."""
        _capi.check(_capi.lib().avr_classify_plan(ctx._handle, self._handle, plan._handle,
                                                  int(slot)))

    def march_plan(self, ctx: "Context", plan, slot: int, out: torch.Tensor,
                   samples: Optional[torch.Tensor] = None) -> torch.Tensor:
        """avr_march_plan on `ctx`'s stream: ray march of classified volume `slot` into the
        sparse send buffer."""
        ctx._check_tensor(out, torch.float32, "out")
        if out.numel() < plan.send_floats:
            raise ValueError("send buffer is too small")
        if samples is not None:
            ctx._check_tensor(samples, torch.int64, "samples")
        _capi.check(_capi.lib().avr_march_plan(
            ctx._handle, self._handle, plan._handle, int(slot), C.c_void_p(out.data_ptr()),
            C.c_void_p(samples.data_ptr()) if samples is not None else None))
        return out

    def classify_plan_chunked(self, ctx: "Context", plan, slot: int, n_chunks: int,
                              events=None, first_alone: bool = False) -> None:
        """avr_classify_plan_chunked: the frame's boxes in n_chunks depth-ordered chunks, one
        classify launch each; events (torch.cuda.Event list or None) are recorded behind them."""
        handles = None
        if events is not None:
            handles = (C.c_void_p * n_chunks)(*[C.c_void_p(e.cuda_event) for e in events])
        _capi.check(_capi.lib().avr_classify_plan_chunked(
            ctx._handle, self._handle, plan._handle, int(slot), int(n_chunks), handles,
            int(bool(first_alone))))

    def march_plan_chunked(self, ctx: "Context", plan, slot: int, out: torch.Tensor, n_chunks: int,
                           samples: Optional[torch.Tensor] = None, events=None) -> torch.Tensor:
        """avr_march_plan_chunked: one march launch per chunk, each resuming the run accumulators
        the launch before stored (waits for events[k] before launch k when given)."""
        ctx._check_tensor(out, torch.float32, "out")
        if out.numel() < plan.send_floats:
            raise ValueError("send buffer is too small")
        if samples is not None:
            ctx._check_tensor(samples, torch.int64, "samples")
        handles = None
        if events is not None:
            handles = (C.c_void_p * n_chunks)(*[C.c_void_p(e.cuda_event) for e in events])
        _capi.check(_capi.lib().avr_march_plan_chunked(
            ctx._handle, self._handle, plan._handle, int(slot), C.c_void_p(out.data_ptr()),
            C.c_void_p(samples.data_ptr()) if samples is not None else None, int(n_chunks),
            handles))
        return out

    def render_plan_culled(self, ctx: "Context", plan, slot: int, out: torch.Tensor, n_chunks: int,
                           samples: Optional[torch.Tensor] = None,
                           visibility: Optional[torch.Tensor] = None) -> torch.Tensor:
        """avr_render_plan_culled: the frame in n_chunks depth-ordered chunks, boxes no ray can
        still sample left out of the classify pass.  Returns the visibility flags (uint8,
        [n_chunks, n_local_boxes]: row k = what march k found visible behind chunk k)."""
        ctx._check_tensor(out, torch.float32, "out")
        if out.numel() < plan.send_floats:
            raise ValueError("send buffer is too small")
        if samples is not None:
            ctx._check_tensor(samples, torch.int64, "samples")
        n = max(len(self.boxes), 1)
        if visibility is None:
            visibility = torch.empty((n_chunks, n), dtype=torch.uint8, device=ctx.device)
        _capi.check(_capi.lib().avr_render_plan_culled(
            ctx._handle, self._handle, plan._handle, int(slot), C.c_void_p(out.data_ptr()),
            C.c_void_p(samples.data_ptr()) if samples is not None else None, int(n_chunks),
            C.c_void_p(visibility.data_ptr())))
        return visibility

    def classify_plan_flagged(self, ctx: "Context", plan, slot: int, flags: torch.Tensor,
                              gate: Optional[torch.Tensor] = None) -> None:
        """avr_classify_plan_flagged: the classify pass of the boxes whose flag (uint8, by position
        in the rank's layer order) is set; with a gate (int32[1]) nothing at all unless it is != 0."""
        ctx._check_tensor(flags, torch.uint8, "flags")
        if flags.numel() < len(self.boxes):
            raise ValueError("flags needs one entry per local box")
        if gate is not None:
            ctx._check_tensor(gate, torch.int32, "gate")
        _capi.check(_capi.lib().avr_classify_plan_flagged(
            ctx._handle, self._handle, plan._handle, int(slot), C.c_void_p(flags.data_ptr()),
            C.c_void_p(gate.data_ptr()) if gate is not None else None))

    @staticmethod
    def march_plan_workgroups(plan) -> int:
        """avr_march_plan_workgroups: an upper bound of the march launch's workgroups."""
        count = C.c_int64(0)
        _capi.check(_capi.lib().avr_march_plan_workgroups(plan._handle, C.byref(count)))
        return int(count.value)

    def classify_plan_positions(self, ctx: "Context", plan, slot: int, positions) -> None:
        """avr_classify_plan_positions: the classify pass of the boxes at these (ascending)
        positions of the rank's layer order -- a launch of exactly their tiles."""
        values = [int(v) for v in positions]
        array = (C.c_int32 * max(len(values), 1))(*values)
        _capi.check(_capi.lib().avr_classify_plan_positions(
            ctx._handle, self._handle, plan._handle, int(slot), array, len(values)))

    def march_plan_speculative(self, ctx: "Context", plan, slot: int, out: torch.Tensor,
                               classified: Optional[torch.Tensor] = None,
                               visited: Optional[torch.Tensor] = None,
                               missed: Optional[torch.Tensor] = None,
                               miss_count: Optional[torch.Tensor] = None,
                               gate: Optional[torch.Tensor] = None,
                               dirty_workgroups: Optional[torch.Tensor] = None) -> torch.Tensor:
        """avr_march_plan_speculative: the march that checks `classified` (the flags this frame's
        classify pass was given), records the boxes it samples in `visited` and the ones it needs
        but finds unclassified in `missed` / `miss_count` (uint8 per local box / int32[1])."""
        ctx._check_tensor(out, torch.float32, "out")
        if out.numel() < plan.send_floats:
            raise ValueError("send buffer is too small")
        n = len(self.boxes)
        for name, tensor, dtype in (("classified", classified, torch.uint8), ("visited", visited, torch.uint8),
                                    ("missed", missed, torch.uint8)):
            if tensor is not None:
                if name == "classified" and not tensor.is_cuda:   # (host flags are allowed here)
                    if tensor.dtype != dtype:
                        raise ValueError("classified must be uint8")
                else:
                    ctx._check_tensor(tensor, dtype, name)
                if tensor.numel() < n:
                    raise ValueError(f"{name} needs one entry per local box")
        for name, tensor in (("miss_count", miss_count), ("gate", gate)):
            if tensor is not None:
                ctx._check_tensor(tensor, torch.int32, name)
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        host = None
        if classified is not None and not classified.is_cuda:   # (host flags: staged with the launch)
            host, classified = classified.contiguous(), None
        if dirty_workgroups is not None:
            ctx._check_tensor(dirty_workgroups, torch.uint8, "dirty_workgroups")
            if dirty_workgroups.numel() < self.march_plan_workgroups(plan):
                raise ValueError("dirty_workgroups is smaller than avr_march_plan_workgroups says")
        spec = _capi.Speculation(ptr(classified), ptr(visited), ptr(missed), ptr(miss_count), None,
                                 ptr(gate), ptr(host), ptr(dirty_workgroups))
        _capi.check(_capi.lib().avr_march_plan_speculative(
            ctx._handle, self._handle, plan._handle, int(slot), C.c_void_p(out.data_ptr()),
            C.byref(spec)))
        return out

    def render_plan(self, plan, out: Optional[torch.Tensor] = None,
                    samples: Optional[torch.Tensor] = None,
                    sync_streams: bool = True) -> torch.Tensor:
        """avr_render_plan: classify + march of this rank's runs into the sparse send buffer."""
        ctx = self.ctx
        if out is None:
            out = ctx.empty(max(plan.send_floats, 1))
        ctx._check_tensor(out, torch.float32, "out")
        if out.numel() < plan.send_floats:
            raise ValueError("send buffer is too small")
        if samples is not None:
            ctx._check_tensor(samples, torch.int64, "samples")
        if sync_streams:
            ctx.join()
        _capi.check(_capi.lib().avr_render_plan(
            ctx._handle, self._handle, plan._handle, C.c_void_p(out.data_ptr()),
            C.c_void_p(samples.data_ptr()) if samples is not None else None))
        if sync_streams:
            ctx.publish()
        return out

    def __init__(self, ctx: Context, boxes: Sequence[AmrBox], transform: ScalarTransform):
        self.ctx = ctx
        self.boxes = list(boxes)
        self.transform = transform
        for b in self.boxes:
            if b.values is None or b.values.device != ctx.device:
                raise ValueError("scene boxes need cell data on the context's device")
        arr = (_capi.Box * max(len(self.boxes), 1))(*[b.to_c() for b in self.boxes])
        ctr = transform.to_c()
        handle = C.c_void_p()
        _capi.check(_capi.lib().avr_scene_create(ctx._handle, arr, len(self.boxes), C.byref(ctr),
                                                 C.byref(handle)))
        self._handle = handle

    def close(self) -> None:
        if getattr(self, "_handle", None):
            _capi.lib().avr_scene_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def render_runs(self, params: _capi.PaintParams, camera: CameraParameters,
                    box_order: Sequence[int], run_end: Sequence[int], n_pieces: int = 1,
                    out: Optional[torch.Tensor] = None,
                    samples: Optional[torch.Tensor] = None, sync_streams: bool = True
                    ) -> torch.Tensor:
        """avr_render_runs: fused paint + owner-side run fold; returns the send-layout buffer
        (n_runs * H * W * 5 floats)."""
        ctx = self.ctx
        order = np.ascontiguousarray(box_order, dtype=np.int32)
        ends = np.ascontiguousarray(run_end, dtype=np.int32)
        n_runs = int(ends.size)
        n_px = int(params.width) * int(params.height)
        if out is None:
            out = ctx.empty(max(n_runs, 1) * n_px * 5)
        ctx._check_tensor(out, torch.float32, "out")
        if out.numel() < n_runs * n_px * 5:
            raise ValueError("out is too small")
        if samples is not None:
            ctx._check_tensor(samples, torch.int64, "samples")
        ccam = camera.to_c()
        ip = C.POINTER(C.c_int32)
        if sync_streams:
            ctx.join()
        _capi.check(_capi.lib().avr_render_runs(
            ctx._handle, self._handle, C.byref(params), C.byref(ccam),
            order.ctypes.data_as(ip), int(order.size), ends.ctypes.data_as(ip), n_runs,
            int(n_pieces), C.c_void_p(out.data_ptr()),
            C.c_void_p(samples.data_ptr()) if samples is not None else None))
        if sync_streams:
            ctx.publish()
        return out


class Comm:
    """avr_comm: this rank's communicator over RCCL / xGMI (one process per GPU).  The 128-byte
    unique id is created on rank 0 and handed to the other ranks through `broadcast_bytes`, a
    callable (bytes or None) -> bytes of the caller's own control plane: torch.distributed's
    store / object broadcast in this package, MPI_Bcast in the reference's host."""

    def __init__(self, device_index: int, rank: int, n_ranks: int, broadcast_bytes):
        self.rank, self.n_ranks = int(rank), int(n_ranks)
        ident, failure = None, None
        if self.rank == 0:
            # Whatever happens here, the broadcast below still takes place: the other ranks are
            # waiting in it, and a rank 0 that raised first would leave them there (an empty id
            # tells them that rank 0 failed).
            try:
                buf = C.create_string_buffer(_capi.COMM_ID_BYTES)
                _capi.check(_capi.lib().avr_comm_unique_id(buf))
                ident = buf.raw
            except Exception as error:
                ident, failure = b"", error
        ident = broadcast_bytes(ident)
        if failure is not None:
            raise failure
        if not ident:
            raise RuntimeError("rank 0 could not create the communicator id (RCCL not loadable?)")
        if len(ident) != _capi.COMM_ID_BYTES:
            raise ValueError("the communicator id did not survive the broadcast")
        handle = C.c_void_p()
        _capi.check(_capi.lib().avr_comm_create(int(device_index), ident, self.rank, self.n_ranks,
                                                C.byref(handle)))
        self._handle = handle

    @classmethod
    def solo(cls, rank: int, n_ranks: int) -> "Comm":
        """avr_comm_create_solo: one rank of an N-rank frame played alone (timing studies)."""
        self = cls.__new__(cls)
        self.rank, self.n_ranks = int(rank), int(n_ranks)
        handle = C.c_void_p()
        _capi.check(_capi.lib().avr_comm_create_solo(self.rank, self.n_ranks, C.byref(handle)))
        self._handle = handle
        return self

    @classmethod
    def solo_rccl(cls, device_index: int, rank: int, n_ranks: int, percent: int = 100) -> "Comm":
        """avr_comm_create_solo_rccl: as solo(), the rank's collectives played through a one-rank
        RCCL communicator to itself (timing studies: RCCL's kernels beside the paint kernels)."""
        self = cls.__new__(cls)
        self.rank, self.n_ranks = int(rank), int(n_ranks)
        handle = C.c_void_p()
        _capi.check(_capi.lib().avr_comm_create_solo_rccl(int(device_index), self.rank,
                                                          self.n_ranks, int(percent),
                                                          C.byref(handle)))
        self._handle = handle
        return self

    @classmethod
    def shared(cls, name: str, rank: int, n_ranks: int, capacity_bytes: int = 256 << 20) -> "Comm":
        """avr_comm_create_shared: rank processes sharing ONE GPU meet in a POSIX shared-memory
        segment (collective).  Rehearsal of the multi-process flow, not a performance path."""
        self = cls.__new__(cls)
        self.rank, self.n_ranks = int(rank), int(n_ranks)
        handle = C.c_void_p()
        _capi.check(_capi.lib().avr_comm_create_shared(name.encode(), self.rank, self.n_ranks,
                                                       int(capacity_bytes), C.byref(handle)))
        self._handle = handle
        return self

    @classmethod
    def from_process_group(cls, device_index: int, group=None) -> "Comm":
        """Bootstraps over an initialised torch.distributed group (any backend)."""
        import torch.distributed as dist
        rank, world = dist.get_rank(group), dist.get_world_size(group)

        def broadcast(ident):
            box = [ident]
            dist.broadcast_object_list(box, src=dist.get_global_rank(group, 0) if group else 0,
                                       group=group)
            return box[0]

        return cls(device_index, rank, world, broadcast)

    def set_control(self, allgather_bytes) -> None:
        """avr_comm_set_control: the caller's control plane for the small host-side agreements of
        an N-rank frame (a new plan's agreement check, the co-run search's window decisions) --
        `allgather_bytes(mine: bytes) -> list of n_ranks bytes objects`, e.g. over gloo
        (control_over_process_group), MPI_Allgather in the reference's host.  None: back to the
        communicator's own (RCCL flavour: a tiny grouped round in band)."""
        if allgather_bytes is None:
            _capi.check(_capi.lib().avr_comm_set_control(self._handle, None, None))
            self._control = None
            return
        n = self.n_ranks

        def trampoline(_user, mine, out, size):
            try:
                parts = allgather_bytes(C.string_at(mine, size))
                if len(parts) != n or any(len(part) != size for part in parts):
                    return 1
                C.memmove(out, b"".join(parts), n * size)
                return 0
            except Exception:  # noqa: BLE001 -- no exception may cross the C ABI
                import traceback
                traceback.print_exc()
                return 1

        callback = _capi.CONTROL_ALLGATHER_FN(trampoline)
        _capi.check(_capi.lib().avr_comm_set_control(self._handle, callback, None))
        self._control = callback   # kept alive for as long as the communicator may call it

    def control_allgather(self, mine: bytes, ctx: Optional["Context"] = None):
        """avr_comm_control_allgather (collective, host-blocking): every rank's bytes."""
        size = len(mine)
        out = C.create_string_buffer(size * self.n_ranks)
        _capi.check(_capi.lib().avr_comm_control_allgather(
            self._handle, ctx._handle if ctx is not None else None, mine, out, size))
        return [out.raw[i * size:(i + 1) * size] for i in range(self.n_ranks)]

    def control_rounds(self) -> int:
        return int(_capi.lib().avr_comm_control_rounds(self._handle))

    def close(self) -> None:
        if getattr(self, "_handle", None):
            _capi.lib().avr_comm_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def control_over_process_group(group=None):
    """A control plane for Comm.set_control over an initialised torch.distributed group (gloo in
    bench.py): all_gather of a byte tensor on the CPU."""
    import torch.distributed as dist

    def allgather(mine: bytes):
        world = dist.get_world_size(group)
        local = torch.frombuffer(bytearray(mine), dtype=torch.uint8)
        parts = [torch.empty_like(local) for _ in range(world)]
        dist.all_gather(parts, local, group=group)
        return [bytes(part.numpy().tobytes()) for part in parts]

    return allgather


def set_frame_timeout_ms(milliseconds: int) -> None:
    """avr_set_frame_timeout_ms: deadline of every host wait on device work (0: none, < 0: default
    = AVR_FRAME_TIMEOUT_MS or 30 s)."""
    _capi.check(_capi.lib().avr_set_frame_timeout_ms(int(milliseconds)))


class NativeRenderer:
    """avr_renderer: the C++ frame driver of one rank (three HIP streams, rotating
    classified volumes and send layouts, RCCL exchange and gather).  Python only hands over the
    scene once and, per frame, the camera, the parameters and the output tensors."""

    def __init__(self, device_index: int, all_boxes: Sequence[AmrBox], transform: ScalarTransform,
                 bounds, scalar_range=(0.0, 1.0), rank: int = 0, n_ranks: int = 1,
                 comm: Optional[Comm] = None, color_map=None):
        from .types import make_params
        self.device_index = int(device_index)
        self.device = torch.device("cuda", self.device_index)
        self.rank, self.n_ranks = int(rank), int(n_ranks)
        self._comm = comm
        self._boxes = list(all_boxes)   # keeps the cell tensors alive
        n = len(self._boxes)
        arr = (_capi.Box * max(n, 1))(*[b.to_c() for b in self._boxes])
        owners = (C.c_int32 * max(n, 1))(*[int(b.owner) for b in self._boxes])
        ctr = transform.to_c()
        bmin = (C.c_double * 3)(*map(float, bounds.min_corner))
        bmax = (C.c_double * 3)(*map(float, bounds.max_corner))
        rng = (C.c_float * 2)(float(scalar_range[0]), float(scalar_range[1]))
        # make_params owns the conversion of a colour map to C points
        params = make_params(1, 1, scalar_range, 0.0, 0.0, bounds, color_map)
        handle = C.c_void_p()
        _capi.check(_capi.lib().avr_renderer_create(
            self.device_index, self.rank, self.n_ranks, comm._handle if comm is not None else None,
            arr, owners, n, C.byref(ctr), bmin, bmax, rng, params.colormap, params.colormap_count,
            C.byref(handle)))
        self._handle = handle
        self._keep = (arr, owners, params)
        out = C.c_float()
        _capi.check(_capi.lib().avr_renderer_reference_sample_distance(self._handle, C.byref(out)))
        self.reference_sample_distance = out.value
        # torch views of the driver's streams: outputs are allocated and consumed on stream X
        self.streams = [torch.cuda.ExternalStream(int(_capi.lib().avr_renderer_stream(self._handle, w)),
                                                  device=self.device) for w in range(3)]

    def close(self) -> None:
        helper = getattr(self, "_plan_ahead", None)
        if helper is not None:   # no plan may be in the making when the renderer goes
            self._plan_ahead = None
            try:
                helper.close()
            except Exception:  # noqa: BLE001 -- its error belongs to whoever submitted the job
                pass
        if getattr(self, "_handle", None):
            _capi.lib().avr_renderer_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_options(self, march_workgroups_per_cu: int = -1, cache_classification: bool = False):
        _capi.check(_capi.lib().avr_renderer_set_options(self._handle, int(march_workgroups_per_cu),
                                                         int(bool(cache_classification))))

    def synchronize(self) -> None:
        """avr_renderer_synchronize: everything queued so far has finished.  For ranks of several
        also sends the last frame's RGB8 pieces to rank 0 (collective: every rank calls it after
        the same frame)."""
        _capi.check(_capi.lib().avr_renderer_synchronize(self._handle))
        self._held_outputs = None

    def set_frame_chunks(self, chunks: int = -1) -> None:
        """avr_renderer_set_frame_chunks: -1 / 1 one launch per kernel (default), k > 1 every
        frame classified and marched in k depth-ordered chunks (measured not to pay:
        profiles/r5_latency/)."""
        _capi.check(_capi.lib().avr_renderer_set_frame_chunks(self._handle, int(chunks)))

    def set_occlusion_culling(self, chunks: int = -1) -> None:
        """avr_renderer_set_occlusion_culling: k >= 2 every frame in k depth-ordered chunks whose
        classify launches leave out the boxes no ray can still sample; -1 / 0 never (default:
        exact but not faster, profiles/r5_opaque/)."""
        _capi.check(_capi.lib().avr_renderer_set_occlusion_culling(self._handle, int(chunks)))

    def set_corun_balance(self, mode: int = -1) -> None:
        """avr_renderer_set_corun_balance: -1 / 1 one rank balances its two kernels by their
        durations (a bisection of ~70 frames), 0 always the full search of every candidate."""
        _capi.check(_capi.lib().avr_renderer_set_corun_balance(self._handle, int(mode)))

    def set_visibility_speculation(self, mode: int = -1) -> None:
        """avr_renderer_set_visibility_speculation: -1 / 1 (default) a frame whose plan repeats
        classifies only the boxes the frame two before sampled, checks and, if need be, repairs
        (exact); 0 never."""
        _capi.check(_capi.lib().avr_renderer_set_visibility_speculation(self._handle, int(mode)))

    def debug_set_speculation_threshold(self, sampled_fraction: float) -> None:
        """avr_renderer_debug_set_speculation_threshold (include/avr_hip_debug.h): tests only."""
        _capi.check(_capi.lib().avr_renderer_debug_set_speculation_threshold(
            self._handle, float(sampled_fraction)))

    _SPECULATION_STATES = {-1: "off", 0: "observing", 1: "waiting for an observation",
                           2: "speculating", 3: "not worth it", 4: "suspended after repairs"}

    def speculation_state(self) -> dict:
        """avr_renderer_speculation_state."""
        state = C.c_int(0)
        frames, repaired = C.c_int64(0), C.c_int64(0)
        fraction = C.c_float(0.0)
        _capi.check(_capi.lib().avr_renderer_speculation_state(
            self._handle, C.byref(state), C.byref(frames), C.byref(repaired), C.byref(fraction)))
        return {"state": self._SPECULATION_STATES.get(state.value, str(state.value)),
                "speculative_frames": int(frames.value), "repaired_frames": int(repaired.value),
                "sampled_fraction": None if fraction.value < 0 else round(float(fraction.value), 4)}

    def last_frame_chunks(self) -> int:
        return int(_capi.lib().avr_renderer_last_frame_chunks(self._handle))

    def outputs_complete(self):
        """avr_renderer_outputs_complete: (frames whose outputs are written once stream X has
        passed what is queued now, frames rendered so far)."""
        done, frames = C.c_uint64(), C.c_uint64()
        _capi.check(_capi.lib().avr_renderer_outputs_complete(self._handle, C.byref(done),
                                                              C.byref(frames)))
        return done.value, frames.value

    def set_overlap(self, overlap_classify: int) -> None:
        """avr_renderer_set_overlap (-1 default: measured, 0 back to back, 1 classify beside the
        march, 2 paired: frames alternate between two streams)."""
        _capi.check(_capi.lib().avr_renderer_set_overlap(self._handle, int(overlap_classify)))

    def set_host_backpressure(self, mode: int = -1) -> None:
        """avr_renderer_set_host_backpressure: -1 default (host-side for a rank of several), 0 the
        streams wait for the frame three back, 1 the host does."""
        _capi.check(_capi.lib().avr_renderer_set_host_backpressure(self._handle, int(mode)))

    def set_tighten(self, enabled: bool = True) -> None:
        """avr_renderer_set_tighten: per-row exchange layout of every plan the driver makes."""
        _capi.check(_capi.lib().avr_renderer_set_tighten(self._handle, int(bool(enabled))))

    def set_piece_layout(self, layout: int = _capi.PIECES_ROW_BANDS, band_rows: int = 8) -> None:
        """avr_renderer_set_piece_layout: how the image is dealt to the ranks' pieces (bands of
        rows dealt round-robin by default; _capi.PIECES_CONTIGUOUS = the reference's ranges)."""
        _capi.check(_capi.lib().avr_renderer_set_piece_layout(self._handle, int(layout),
                                                              int(band_rows)))

    def set_classify_share(self, lds_reserve_bytes: int = -1) -> None:
        """avr_renderer_set_classify_share: -1 = measured by the driver (default), >= 0 = fixed
        LDS reserve per classify workgroup while the pass runs beside the march."""
        _capi.check(_capi.lib().avr_renderer_set_classify_share(self._handle,
                                                                int(lds_reserve_bytes)))

    def corun_state(self) -> dict:
        """avr_renderer_corun_state: how the last frame placed the classify pass and the march."""
        overlap, reserve, settled, windows = C.c_int(0), C.c_int(0), C.c_int(0), C.c_long(0)
        _capi.check(_capi.lib().avr_renderer_corun_state(self._handle, C.byref(overlap),
                                                         C.byref(reserve), C.byref(settled),
                                                         C.byref(windows)))
        layout = {0: "before the march", 1: "beside the march",
                  2: "before its march, the frames alternating between two streams"}
        return {"classify": layout.get(overlap.value, str(overlap.value)),
                "lds_reserve_bytes": reserve.value, "settled": bool(settled.value),
                "timed_windows": windows.value}

    def set_deferred_gather(self, mode: int = -1) -> None:
        """avr_renderer_set_deferred_gather: -1 default (ranks of several: a frame's RGB8 pieces
        travel to rank 0 with the NEXT frame's grouped round; synchronize() sends the last
        frame's), 0 every frame gathers at once, 1 on."""
        _capi.check(_capi.lib().avr_renderer_set_deferred_gather(self._handle, int(mode)))

    def set_plan_check(self, enabled: bool = True) -> None:
        """avr_renderer_set_plan_check: whether a new plan of a rank of several is agreed on over
        the control plane before its first frame is queued (default on)."""
        _capi.check(_capi.lib().avr_renderer_set_plan_check(self._handle, int(bool(enabled))))

    def set_corun_coordination(self, mode: int = -1) -> None:
        """avr_renderer_set_corun_coordination: -1 default (ranks of several search as one
        system), 0 every rank on its own (round 3's behaviour), 1 on."""
        _capi.check(_capi.lib().avr_renderer_set_corun_coordination(self._handle, int(mode)))

    def set_corun_history(self, frames: int) -> None:
        """Record the co-run candidate of each of the next `frames` frames (diagnostics)."""
        _capi.check(_capi.lib().avr_renderer_set_corun_history(self._handle, int(frames)))

    def corun_history(self):
        """The recorded candidates: -1 back to back, k side by side with reserve k * 2 KiB,
        29 + k paired."""
        n = C.c_int(0)
        _capi.check(_capi.lib().avr_renderer_corun_history(self._handle, None, 0, C.byref(n)))
        out = (C.c_int16 * max(n.value, 1))()
        _capi.check(_capi.lib().avr_renderer_corun_history(self._handle, out, n.value, C.byref(n)))
        return list(out[:n.value])

    def last_march_mode(self) -> int:
        """avr_renderer_last_march_mode: Context.last_march_mode of the latest frame's march."""
        mode = C.c_int(-2)
        _capi.check(_capi.lib().avr_renderer_last_march_mode(self._handle, C.byref(mode)))
        return int(mode.value)

    def failure(self) -> Optional[str]:
        """avr_renderer_failure: what did not finish within the deadline, or None."""
        text = _capi.lib().avr_renderer_failure(self._handle)
        return text.decode("utf-8", "replace") if text else None

    def set_scalar_range(self, scalar_range) -> None:
        rng = (C.c_float * 2)(float(scalar_range[0]), float(scalar_range[1]))
        _capi.check(_capi.lib().avr_renderer_set_scalar_range(self._handle, rng))

    def invalidate(self) -> None:
        _capi.check(_capi.lib().avr_renderer_invalidate(self._handle))

    def plan_info(self) -> "_capi.FramePlanInfo":
        info = _capi.FramePlanInfo()
        _capi.check(_capi.lib().avr_renderer_plan_info(self._handle, C.byref(info)))
        return info

    def host_profile(self, reset: bool = True):
        """({section: microseconds per frame}, frames) spent inside avr_renderer_render."""
        sec = (C.c_double * 6)()
        n = C.c_long()
        _capi.check(_capi.lib().avr_renderer_host_profile(self._handle, sec, C.byref(n), int(reset)))
        names = ("plan", "classify", "march", "exchange", "fold", "gather+tail")
        frames = max(n.value, 1)
        return {k: 1e6 * v / frames for k, v in zip(names, sec)}, n.value

    def set_timing(self, enabled: bool) -> None:
        _capi.check(_capi.lib().avr_renderer_set_timing(self._handle, int(bool(enabled))))

    def timings(self):
        """(classify_ms, march_ms, busy_ms, frames) averaged per frame since set_timing(True)."""
        c, m, b, n = C.c_double(), C.c_double(), C.c_double(), C.c_int()
        _capi.check(_capi.lib().avr_renderer_timings(self._handle, C.byref(c), C.byref(m),
                                                     C.byref(b), C.byref(n)))
        return c.value, m.value, b.value, n.value

    def prepare(self, width: int, height: int, box_transparency: float, antialiasing: int,
                camera: CameraParameters, use_visibility_graph: bool = True,
                draw_bounds: bool = True, write_visibility_graph: bool = False,
                group_order: Optional[Sequence[int]] = None) -> None:
        """avr_renderer_prepare: makes and keeps the frame plan render() will want for these
        arguments -- host geometry only.  May run on another thread while render() queues a frame
        (ctypes releases the GIL for the call): see PlanAhead."""
        rp = _capi.RenderParams(int(width), int(height), float(box_transparency),
                                int(antialiasing), int(bool(use_visibility_graph)),
                                int(bool(draw_bounds)), int(bool(write_visibility_graph)))
        ccam = camera.to_c()
        group = None
        if group_order is not None:
            group = (C.c_int32 * self.n_ranks)(*[int(g) for g in group_order])
        _capi.check(_capi.lib().avr_renderer_prepare(self._handle, C.byref(rp), C.byref(ccam),
                                                     group))

    def render(self, width: int, height: int, box_transparency: float, antialiasing: int,
               camera: CameraParameters, use_visibility_graph: bool = True,
               draw_bounds: bool = True, write_visibility_graph: bool = False,
               group_order: Optional[Sequence[int]] = None,
               samples: Optional[torch.Tensor] = None, want_image: bool = False):
        """One frame (asynchronous).  Rank 0 returns (image [H, W, 5] or None, rgb8 [H, W, 3] with
        rows top-down); other ranks (None, None).  One rank: the tensors are complete on stream X
        (self.streams[2]) -- synchronize(), or order your stream after it.  Ranks of several: the
        RGB8 bytes of a frame without want_image travel to rank 0 inside the NEXT frame's round
        (avr_renderer_set_deferred_gather, the default), so after ordering a stream behind stream X
        only the frames outputs_complete() counts are written -- the last frame's tensor is still
        uninitialised memory until the next render() has passed stream X or synchronize() (a
        collective then: every rank calls it after the same frame) has returned."""
        # (a camera and parameters that repeat are converted once: per frame the Python layer costs
        # the host what matters beside a rank's 0.17 ms frame)
        key = (width, height, box_transparency, antialiasing, use_visibility_graph, draw_bounds,
               write_visibility_graph, tuple(map(float, camera.eye)),
               tuple(map(float, camera.look_at)), tuple(map(float, camera.up)),
               float(camera.fov_y_degrees), float(camera.near_plane), float(camera.far_plane))
        if getattr(self, "_converted_key", None) != key:
            self._converted = (
                _capi.RenderParams(int(width), int(height), float(box_transparency),
                                   int(antialiasing), int(bool(use_visibility_graph)),
                                   int(bool(draw_bounds)), int(bool(write_visibility_graph))),
                camera.to_c())
            self._converted_key = key
        rp, ccam = self._converted
        group = None
        if group_order is not None:
            group = (C.c_int32 * self.n_ranks)(*[int(g) for g in group_order])
        rgb8 = image = None
        caller = torch.cuda.current_stream(self.device)
        with torch.cuda.stream(self.streams[2]):
            if self.rank == 0:
                rgb8 = torch.empty((height, width, 3), dtype=torch.uint8, device=self.device)
                if want_image:
                    image = torch.empty((height, width, 5), dtype=torch.float32, device=self.device)
        if samples is not None and (samples.dtype != torch.int64 or samples.device != self.device):
            raise ValueError("samples must be an int64 tensor on the renderer's device")
        # Cell data / the samples counter may have been written on the caller's stream: the driver
        # orders this frame's classify pass (and with it the march) after that stream.  torch's
        # default stream has handle 0, which the C ABI reads as "nothing to wait for": it is named
        # by AVR_DEFAULT_STREAM (-1) instead -- the driver's streams are non-blocking and never
        # order themselves after the null stream implicitly.
        wait = None if caller.query() else C.c_void_p(caller.cuda_stream or _capi.DEFAULT_STREAM)
        _capi.check(_capi.lib().avr_renderer_render(
            self._handle, C.byref(rp), C.byref(ccam), group, wait,
            C.c_void_p(samples.data_ptr()) if samples is not None else None, int(bool(want_image)),
            C.c_void_p(rgb8.data_ptr()) if rgb8 is not None else None,
            C.c_void_p(image.data_ptr()) if image is not None else None))
        # (ranks of several: this frame's bytes are written while the NEXT frame is queued, or by
        # synchronize(): the tensor must outlive the caller's interest in it until then)
        self._held_outputs = (image, rgb8)
        return image, rgb8

    def render_max(self, width: int, height: int, camera: CameraParameters,
                   use_visibility_graph: bool = True, group_order: Optional[Sequence[int]] = None,
                   samples: Optional[torch.Tensor] = None):
        """One maximum-intensity frame (avr_renderer_render_max, asynchronous like render()).
        Rank 0 returns (rgb8 [H, W, 3] uint8, rows top-down; index [H, W] int16, the largest
        transfer-function table index per pixel, -1 where no box takes a sample, row 0 at the
        bottom like render()'s image); other ranks (None, None).  Both are complete on stream X."""
        rp = _capi.RenderParams(int(width), int(height), 0.0, 1, int(bool(use_visibility_graph)), 0, 0)
        ccam = camera.to_c()
        group = None
        if group_order is not None:
            group = (C.c_int32 * self.n_ranks)(*[int(g) for g in group_order])
        rgb8 = index = None
        caller = torch.cuda.current_stream(self.device)
        with torch.cuda.stream(self.streams[2]):
            if self.rank == 0:
                rgb8 = torch.empty((height, width, 3), dtype=torch.uint8, device=self.device)
                index = torch.empty((height, width), dtype=torch.int16, device=self.device)
        if samples is not None and (samples.dtype != torch.int64 or samples.device != self.device):
            raise ValueError("samples must be an int64 tensor on the renderer's device")
        wait = None if caller.query() else C.c_void_p(caller.cuda_stream or _capi.DEFAULT_STREAM)
        _capi.check(_capi.lib().avr_renderer_render_max(
            self._handle, C.byref(rp), C.byref(ccam), group, wait,
            C.c_void_p(samples.data_ptr()) if samples is not None else None,
            C.c_void_p(rgb8.data_ptr()) if rgb8 is not None else None,
            C.c_void_p(index.data_ptr()) if index is not None else None))
        self._held_outputs = (index, rgb8)
        return rgb8, index

    def render_projection(self, width: int, height: int, camera: CameraParameters,
                          use_visibility_graph: bool = True,
                          group_order: Optional[Sequence[int]] = None,
                          samples: Optional[torch.Tensor] = None):
        """One column-projection frame (avr_renderer_render_projection, asynchronous like
        render()).  Rank 0 returns (column, length) as float64 [H, W], row 0 at the bottom like
        render_max()'s index: per pixel the sums over the boxes of f64(step) times the sum, and
        times the number, of the finite raw cell values sampled ("Column projection");
        other ranks (None, None).  Both are complete on stream X.  samples (int64) gains every
        sample taken, finite or not.  The cells must stay unchanged until then."""
        rp = _capi.RenderParams(int(width), int(height), 0.0, 1, int(bool(use_visibility_graph)), 0, 0)
        ccam = camera.to_c()
        group = None
        if group_order is not None:
            group = (C.c_int32 * self.n_ranks)(*[int(g) for g in group_order])
        column = length = None
        caller = torch.cuda.current_stream(self.device)
        with torch.cuda.stream(self.streams[2]):
            if self.rank == 0:
                column = torch.empty((height, width), dtype=torch.float64, device=self.device)
                length = torch.empty((height, width), dtype=torch.float64, device=self.device)
        if samples is not None and (samples.dtype != torch.int64 or samples.device != self.device):
            raise ValueError("samples must be an int64 tensor on the renderer's device")
        wait = None if caller.query() else C.c_void_p(caller.cuda_stream or _capi.DEFAULT_STREAM)
        _capi.check(_capi.lib().avr_renderer_render_projection(
            self._handle, C.byref(rp), C.byref(ccam), group, wait,
            C.c_void_p(samples.data_ptr()) if samples is not None else None,
            C.c_void_p(column.data_ptr()) if column is not None else None,
            C.c_void_p(length.data_ptr()) if length is not None else None))
        self._held_outputs = (column, length)
        return column, length


class PlanAhead:
    """Plans the NEXT frame on a helper thread while the caller queues this one: for a camera
    that never repeats the host's geometry of a new camera (visibility order, frame plan, tightened
    exchange layout: ~0.1 ms for 176 boxes at N = 8) otherwise adds to every frame's queueing, and
    a rank of eight has 0.15 ms per frame.  submit() the arguments of the render() call that will
    follow the next one; render() finds the plan (or, if the helper is not through, waits for it
    and goes on).  Results never depend on it."""

    def __init__(self, native: "NativeRenderer"):
        import queue
        import threading
        self._native = native
        native._plan_ahead = self   # NativeRenderer.close() closes the helper first
        self._jobs = queue.SimpleQueue()
        self._error = None
        self._thread = threading.Thread(target=self._run, name="avr-plan-ahead", daemon=True)
        self._thread.start()

    def _run(self) -> None:
        while True:
            job = self._jobs.get()
            if job is None:
                return
            try:
                self._native.prepare(*job[0], **job[1])
            except Exception as error:  # noqa: BLE001 -- handed to the submitting thread
                self._error = error

    def submit(self, *args, **kwargs) -> None:
        if self._error is not None:
            error, self._error = self._error, None
            raise error
        self._jobs.put((args, kwargs))

    def close(self) -> None:
        if self._thread is not None:
            self._jobs.put(None)
            self._thread.join()
            self._thread = None
            if getattr(self._native, "_plan_ahead", None) is self:
                self._native._plan_ahead = None
        if self._error is not None:
            error, self._error = self._error, None
            raise error
