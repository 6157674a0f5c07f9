"""On-axis projection timing on config-4 (176 boxes of 128^3, 2.95 GB per field), one rank, at
2048 x 2048 pixels over the whole data.  The weight field is derived from the field on the device
(its square), so both share one box list.  Per axis, without and with the weight, events on the
context's stream time the whole call (reduce + gather) and the same call into a 1 x 1 image (the
reduce stage with a gather of one wave); their difference is the gather stage.  In the same run
the yardstick, Scene.scalar_stats (scalar_stats_kernel) on the same scene, is timed as a call: it
synchronises and allocates, so its event time is an upper bound of the kernel's.  One JSON line is
printed.  The kernels' own times come from a kernel trace of the same run, which this tool then
reads back:

  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/axis_projection_timing.py
  python tools/axis_projection_timing.py --trace OUT

--trace tells the cases apart by the order of the dispatches, which is the order of CASES below
with 2 x (--warmup + --frames) dispatches of a reduce kernel each.  Needs a HIP device: fails
loudly without one."""
import argparse
import csv
import glob
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZE = 2048
# (label, axis, weighted, reduce kernel, bytes read per cell)
CASES = [(f"{'xyz'[axis]}{'_weighted' if w else ''}", axis, w,
          "axis_reduce_rows_kernel" if axis == 0 else "axis_reduce_columns_kernel", 16 if w else 8)
         for axis in range(3) for w in (False, True)]


def run(frames: int, warmup: int) -> dict:
    import torch
    from amrvolumerenderer_amd import runtime, scenes
    from amrvolumerenderer_amd.types import AmrBox, ScalarTransform
    if not torch.cuda.is_available():
        raise SystemExit("tools/axis_projection_timing.py needs a HIP device")
    ctx = runtime.Context(0)
    spec = scenes.config4("smooth")
    f_cells = [scenes.box_cells_torch(spec, i, ctx.device) for i in range(len(spec.boxes))]
    w_cells = [c * c for c in f_cells]
    torch.cuda.synchronize()

    def scene_of(cells):
        boxes = [AmrBox(m.min_corner, m.max_corner, c, m.level) for c, m in zip(cells, spec.boxes)]
        return ctx.create_scene(boxes, ScalarTransform())

    sf, sw = scene_of(f_cells), scene_of(w_cells)
    n_cells = spec.total_cells
    n_levels = 1 + max(int(m.level) for m in spec.boxes)
    lo = [min(m.min_corner[a] for m in spec.boxes) for a in range(3)]
    hi = [max(m.max_corner[a] for m in spec.boxes) for a in range(3)]
    result = {"config": "config-4", "boxes": len(spec.boxes), "cells": n_cells, "frames": frames,
              "warmup": warmup, "size": SIZE}

    def timed(call):
        for _ in range(warmup):
            call()
        ctx.synchronize()
        begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        begin.record(ctx.stream)
        for _ in range(frames):
            call()
        end.record(ctx.stream)
        end.synchronize()
        return begin.elapsed_time(end) / frames

    stats_ms = timed(sf.scalar_stats)
    result["scalar_stats_call_ms"] = round(stats_ms, 4)
    result["scalar_stats_call_TBps"] = round(n_cells * 8 / stats_ms / 1e9, 3)
    for label, axis, weighted, _, bytes_per_cell in CASES:
        au, av = (axis + 1) % 3, (axis + 2) % 3
        dl = [1.0 / (1 << level) for level in range(n_levels)]

        def images(size):
            return [torch.empty((size, size), dtype=torch.float64, device=ctx.device)
                    if (weighted or i != 1) else None for i in range(3)]

        def call(size, outs):
            return sf.axis_projection(axis, (lo[au], lo[av]), (hi[au] - lo[au]) / size,
                                      (hi[av] - lo[av]) / size, size, size, dl,
                                      sw if weighted else None, *outs)

        full, one = images(SIZE), images(1)
        total = timed(lambda: call(SIZE, full))
        reduce = timed(lambda: call(1, one))
        ctx.synchronize()
        result[label + "_total_ms"] = round(total, 4)
        result[label + "_reduce_ms"] = round(reduce, 4)
        result[label + "_gather_ms"] = round(total - reduce, 4)
        result[label + "_reduce_TBps"] = round(n_cells * bytes_per_cell / reduce / 1e9, 3)
        result[label + "_covered"] = float((full[2] > 0).double().mean().item())
    return result


def read_trace(directory: str, frames: int, warmup: int) -> dict:
    """Per case the mean and the smallest kernel time of the timed dispatches of its reduce kernel
    and of the 2048^2 gather, and of scalar_stats_kernel, from the kernel trace of one run."""
    files = glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True)
    if len(files) != 1:
        raise SystemExit(f"expected one kernel trace under {directory}, found {len(files)}")
    kernels = ("scalar_stats_kernel", "axis_reduce_rows_kernel", "axis_reduce_columns_kernel",
               "axis_gather_kernel")
    rows = {kernel: [] for kernel in kernels}
    with open(files[0], newline="") as fh:
        for row in csv.DictReader(fh):
            name = row["Kernel_Name"]
            for kernel in kernels:
                if f"::{kernel}" in name or f"{len(kernel)}{kernel}" in name:
                    rows[kernel].append((int(row["Start_Timestamp"]), int(row["End_Timestamp"])))
    for kernel in rows:
        rows[kernel].sort()
    cells = 176 * 128 ** 3

    def summary(times, bytes_per_cell=None):
        times = [(end - start) * 1e-6 for start, end in times]
        if len(times) != frames:
            raise SystemExit("the trace holds too few dispatches")
        mean = sum(times) / len(times)
        out = {"mean_ms": round(mean, 4), "min_ms": round(min(times), 4)}
        if bytes_per_cell is not None:
            out["TBps"] = round(cells * bytes_per_cell / mean / 1e9, 3)
        return out

    out = {"scalar_stats": summary(rows["scalar_stats_kernel"][warmup:warmup + frames], 8)}
    per_case = warmup + frames
    taken = {kernel: 0 for kernel in kernels}
    for label, _, _, kernel, bytes_per_cell in CASES:
        # per case: the 2048^2 calls, then the 1 x 1 calls
        first = taken[kernel] + warmup
        out[label + "_reduce"] = summary(rows[kernel][first:first + frames], bytes_per_cell)
        out[label + "_reduce"]["vs_scalar_stats_per_field"] = round(
            out[label + "_reduce"]["mean_ms"] / (bytes_per_cell // 8) / out["scalar_stats"]["mean_ms"], 3)
        first = taken["axis_gather_kernel"] + warmup
        out[label + "_gather"] = summary(rows["axis_gather_kernel"][first:first + frames])
        taken[kernel] += 2 * per_case
        taken["axis_gather_kernel"] += 2 * per_case
    return out


if __name__ == "__main__":
    parser = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    parser.add_argument("--frames", type=int, default=10)
    parser.add_argument("--warmup", type=int, default=3)
    parser.add_argument("--trace", help="directory of a rocprofv3 --kernel-trace run of this tool")
    args = parser.parse_args()
    if args.trace:
        print(json.dumps(read_trace(args.trace, args.frames, args.warmup), indent=1))
    else:
        print(json.dumps(run(args.frames, args.warmup)))
