"""Streamline timing on config-4 (176 boxes of 128^3, three levels, 2.95 GB per component), one
rank: 2^16 seeds on a 64 x 32 x 32 lattice over the middle half of the domain, 256 steps at step =
0.5, through the swirl V = (-(y - 0.5), x - 0.5, 0.25) evaluated at the cell centres, with V's x
component as the sample.  Scene.streamlines is timed with events on the context's stream, --warmup
calls first, then --frames; steps per second counts the steps the lines really took.  The field is
exact in binary64 on the host and on the device alike, so the numpy reference
(tests/streamline_reference.py), run on 64 of the same lines for scale over the same hierarchy
described by rules instead of arrays, must give the device's bits: that is reported too.  One JSON
line is printed.  The kernel's own time comes from a kernel trace of the same run, which this tool
then reads back:

  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- \
      python tools/streamline_timing.py --no-reference
  python tools/streamline_timing.py --trace OUT

Needs a HIP device: fails loudly without one."""
import argparse
import csv
import glob
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N0, LEVELS, BOX = 512, 3, 128
LATTICE = (64, 32, 32)
STEPS, STEP = 256, 0.5
REFERENCE_LINES = 64
COMPONENTS = (lambda x, y, z: -(y - 0.5) + 0.0 * (x + z), lambda x, y, z: (x - 0.5) + 0.0 * (y + z),
              lambda x, y, z: 0.25 + 0.0 * (x + y + z))


def seeds():
    import numpy as np
    axes = [0.25 + (np.arange(n) + 0.5) * (0.5 / n) for n in LATTICE]
    x, y, z = np.meshgrid(*axes, indexing="ij")
    return np.ascontiguousarray(np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1))


def reference_lines(n):
    """Which of the n seeds the reference follows: one per x plane, y and z moving along."""
    import numpy as np
    per_plane = n // REFERENCE_LINES
    return np.arange(REFERENCE_LINES) * per_plane + (np.arange(REFERENCE_LINES) * 33) % per_plane


class _Rule:
    """What the reference indexes like a level's array, answered from the cell's indices."""

    def __init__(self, shape, answer):
        self.shape, self.answer = shape, answer

    def __getitem__(self, at):
        return self.answer(*(at[1:] if isinstance(at[0], slice) else at))


def rule_hierarchy():
    """tests/streamline_reference.Hierarchy over config-4 without its 2048^3 arrays: the leaves of
    scenes.make_amr_scene (every level a cube of N0 cells, its centred half covered by the next)
    and the swirl at the cell centres."""
    import numpy as np
    import streamline_reference as sl
    h = sl.Hierarchy.__new__(sl.Hierarchy)
    h.max_level, h.ratio, h.has_sample = LEVELS - 1, [2] * (LEVELS - 1), True
    h.prob_lo = np.zeros(3)
    h.origin, h.mask, h.values, h.dx = [], [], [], []
    first = 0
    for level in range(LEVELS):
        if level > 0:
            first = (first + N0 // 4) * 2
        n = N0 << level

        def leaf(k, j, i, first=first, level=level):
            rel = np.stack([i, j, k]) - first
            held = ((rel >= 0) & (rel < N0)).all(axis=0)
            covered = ((rel >= N0 // 4) & (rel < N0 - N0 // 4)).all(axis=0)
            return held & ~(covered & (level + 1 < LEVELS))

        def cells(k, j, i, n=n):
            x, y, z = ((index + 0.5) / n for index in (i, j, k))
            v = [f(x, y, z) for f in COMPONENTS]
            return np.stack(v + [v[0]])

        h.origin.append(np.zeros(3, dtype=np.int64))
        h.mask.append(_Rule((n, n, n), leaf))
        h.values.append(_Rule((4, n, n, n), cells))
        h.dx.append(np.full(3, 1.0 / n))
    return h


def run(frames: int, warmup: int, reference: bool = True) -> dict:
    import numpy as np
    import torch
    from amrvolumerenderer_amd import runtime, scenes
    from amrvolumerenderer_amd.types import AmrBox, ScalarTransform
    if not torch.cuda.is_available():
        raise SystemExit("tools/streamline_timing.py needs a HIP device")
    ctx = runtime.Context(0)
    spec = scenes.make_amr_scene(N0, LEVELS, BOX, "smooth", "config4_amr3_512")
    fields = []
    for f in COMPONENTS:
        boxes = []
        for m in spec.boxes:
            x, y, z = scenes._cell_centres(m, spec, torch, device=ctx.device)
            cells = f(x[None, None, :], y[None, :, None], z[:, None, None]).contiguous()
            boxes.append(AmrBox(m.min_corner, m.max_corner, cells, m.level))
        fields.append(ctx.create_scene(boxes, ScalarTransform()))
    torch.cuda.synchronize()
    index = np.array([m.lo for m in spec.boxes], dtype=np.int32)
    sizes = np.array([[1.0 / (N0 << l)] * 3 for l in range(LEVELS)])
    start = seeds()
    on_device = torch.from_numpy(start).to(ctx.device)
    call = lambda: fields[0].streamlines(fields[1], fields[2], on_device, STEP, 1, STEPS, index,
                                         [2] * (LEVELS - 1), sizes, [0.0, 0.0, 0.0], fields[0])
    for _ in range(warmup):
        out = call()
    ctx.synchronize()
    begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    begin.record(ctx.stream)
    for _ in range(frames):
        out = call()
    end.record(ctx.stream)
    end.synchronize()
    call_ms = begin.elapsed_time(end) / frames
    points, samples, counts, status = (t.cpu().numpy() for t in out)
    steps = int(np.maximum(counts.astype(np.int64) - 1, 0).sum())
    result = {"config": "config-4", "boxes": len(spec.boxes), "seeds": int(start.shape[0]),
              "max_steps": STEPS, "step": STEP, "frames": frames, "warmup": warmup,
              "call_ms": round(call_ms, 4), "steps_taken": steps,
              "steps_per_s": round(steps / (call_ms * 1e-3)),
              "status": np.bincount(status, minlength=4).tolist()}
    if not reference:
        return result
    # the numpy reference on 64 of the same lines, spread over the lattice
    pick = reference_lines(start.shape[0])
    hierarchy = rule_hierarchy()
    t0 = time.perf_counter()
    want = hierarchy.trace(start[pick], STEP, 1, STEPS)
    seconds = time.perf_counter() - t0
    taken = int(np.maximum(want["counts"] - 1, 0).sum())
    same = (np.array_equal(want["counts"], counts[pick]) and
            np.array_equal(want["status"], status[pick]) and
            np.array_equal(np.nan_to_num(want["points"], nan=-1.0),
                           np.nan_to_num(points[pick], nan=-1.0)) and
            np.array_equal(np.nan_to_num(want["samples"], nan=-1.0),
                           np.nan_to_num(samples[pick], nan=-1.0)))
    result["reference"] = {"lines": REFERENCE_LINES, "seconds": round(seconds, 3),
                           "steps_taken": taken, "steps_per_s": round(taken / seconds),
                           "equal_bits": bool(same)}
    return result


def read_trace(directory: str, frames: int, warmup: int) -> dict:
    """The mean and the smallest time of streamlines_kernel over the timed dispatches."""
    files = glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True)
    if len(files) != 1:
        raise SystemExit(f"expected one kernel trace under {directory}, found {len(files)}")
    rows = []
    with open(files[0], newline="") as fh:
        for row in csv.DictReader(fh):
            if "streamlines_kernel" in row["Kernel_Name"]:
                rows.append((int(row["Start_Timestamp"]), int(row["End_Timestamp"])))
    rows.sort()
    times = [(e - b) * 1e-6 for b, e in rows[warmup:warmup + frames]]
    if len(times) != frames:
        raise SystemExit(f"expected {warmup + frames} dispatches of streamlines_kernel, "
                         f"found {len(rows)}")
    return {"streamlines_kernel": {"mean_ms": round(sum(times) / frames, 4),
                                   "min_ms": round(min(times), 4)}}


if __name__ == "__main__":
    parser = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    parser.add_argument("--frames", type=int, default=10)
    parser.add_argument("--warmup", type=int, default=3)
    parser.add_argument("--trace", help="directory of a rocprofv3 --kernel-trace run of this tool")
    parser.add_argument("--no-reference", action="store_true",
                        help="leave the numpy reference out (a traced run)")
    args = parser.parse_args()
    if args.trace:
        print(json.dumps(read_trace(args.trace, args.frames, args.warmup), indent=1))
    else:
        print(json.dumps(run(args.frames, args.warmup, not args.no_reference)))
