"""Gradient-field timing on config-4 (176 boxes of 128^3, 2.95 GB per field), one rank: the three
axes, timed with events on the context's stream around Scene.gradient (both kernels: the halo and
the difference; the difference kernel moves 16 bytes per cell plus the faces).  In the same run the
yardstick, Scene.scalar_stats (scalar_stats_kernel) on the same scene, is timed as a call: it
synchronises and allocates, so its event time is an upper bound of the kernel's.  One JSON line is
printed.  The kernels' own times come from a kernel trace of the same run, which this tool then
reads back:

  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/gradient_timing.py
  python tools/gradient_timing.py --trace OUT

Hardware counters come from runs of their own, never together with a trace, one run per group of
counters that the hardware can hold at once, all below one directory, and are read back likewise
(per kernel and axis the mean over the dispatches; a counter's rows of one dispatch are summed):

  rocprofv3 --kernel-include-regex "gradient_kernel|scalar_stats_kernel" --pmc SQ_WAVES ... \
      --output-format csv -d OUT/pass0 -- python tools/gradient_timing.py
  python tools/gradient_timing.py --counters OUT

--trace and --counters tell the axes apart by the order of the dispatches, which is x, y, z with
--warmup + --frames dispatches each.  Needs a HIP device: fails loudly without one."""
import argparse
import collections
import csv
import glob
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

AXES = ("x", "y", "z")
CELLS = 176 * 128 ** 3
KERNELS = ("scalar_stats_kernel", "gradient_halo_kernel", "gradient_kernel")


def run(frames: int, warmup: int) -> dict:
    import numpy as np
    import torch
    from amrvolumerenderer_amd import runtime, scenes
    from amrvolumerenderer_amd.types import AmrBox, ScalarTransform
    if not torch.cuda.is_available():
        raise SystemExit("tools/gradient_timing.py needs a HIP device")
    ctx = runtime.Context(0)
    spec = scenes.config4("smooth")
    first = [scenes.box_cells_torch(spec, i, ctx.device) for i in range(len(spec.boxes))]
    target = [torch.empty_like(c) for c in first]
    torch.cuda.synchronize()

    def scene_of(tensors):
        boxes = [AmrBox(m.min_corner, m.max_corner, c, m.level) for c, m in zip(tensors, spec.boxes)]
        return ctx.create_scene(boxes, ScalarTransform())

    field, out = scene_of(first), scene_of(target)
    n_cells = spec.total_cells
    n_levels = 1 + max(int(m.level) for m in spec.boxes)
    index = np.array([m.lo for m in spec.boxes], dtype=np.int32)
    sizes = [[(m.max_corner[a] - m.min_corner[a]) / m.dims[a] for a in range(3)]
             for level in range(n_levels)
             for m in [next(b for b in spec.boxes if int(b.level) == level)]]
    result = {"config": "config-4", "boxes": len(spec.boxes), "cells": n_cells, "frames": frames,
              "warmup": warmup}

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

    stats_ms = timed(field.scalar_stats)
    result["scalar_stats_call_ms"] = round(stats_ms, 4)
    result["scalar_stats_call_TBps"] = round(n_cells * 8 / stats_ms / 1e9, 3)
    for axis, label in enumerate(AXES):
        ms = timed(lambda: out.gradient(field, axis, index, [2] * (n_levels - 1),
                                        [s[axis] for s in sizes]))
        result[label + "_call_ms"] = round(ms, 4)
        result[label + "_call_TBps"] = round(n_cells * 16 / ms / 1e9, 3)
        result[label + "_call_per_byte_vs_scalar_stats_call"] = round((ms / 16) / (stats_ms / 8), 3)
    return result


def _kernel_of(name: str):
    for kernel in KERNELS:
        if f"::{kernel}" in name or f"{len(kernel)}{kernel}" in name:
            return kernel
    return None


def read_trace(directory: str, frames: int, warmup: int) -> dict:
    """Per axis the mean and the smallest kernel time of the timed dispatches of gradient_kernel
    and of gradient_halo_kernel, and of scalar_stats_kernel, from the kernel trace of one run."""
    files = glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True)
    if len(files) != 1:
        raise SystemExit(f"expected one kernel trace under {directory}, found {len(files)}")
    rows = {kernel: [] for kernel in KERNELS}
    with open(files[0], newline="") as fh:
        for row in csv.DictReader(fh):
            kernel = _kernel_of(row["Kernel_Name"])
            if kernel is not None:
                rows[kernel].append((int(row["Start_Timestamp"]), int(row["End_Timestamp"])))
    for kernel in rows:
        rows[kernel].sort()

    def summary(times, bytes_per_cell=None):
        times = [(end - start) * 1e-6 for start, end in times]
        if len(times) != frames:
            raise SystemExit("the trace holds too few dispatches")
        mean = sum(times) / len(times)
        out = {"mean_ms": round(mean, 4), "min_ms": round(min(times), 4)}
        if bytes_per_cell is not None:
            out["bytes_per_cell"] = bytes_per_cell
            out["TBps"] = round(CELLS * bytes_per_cell / mean / 1e9, 3)
        return out

    out = {"scalar_stats": summary(rows["scalar_stats_kernel"][warmup:warmup + frames], 8)}
    per_byte = out["scalar_stats"]["mean_ms"] / 8
    for index, label in enumerate(AXES):
        first = index * (warmup + frames) + warmup
        out[label] = summary(rows["gradient_kernel"][first:first + frames], 16)
        out[label]["per_byte_vs_scalar_stats"] = round(out[label]["mean_ms"] / 16 / per_byte, 3)
        out[label + "_halo"] = summary(rows["gradient_halo_kernel"][first:first + frames])
    return out


def read_counters(directory: str, frames: int, warmup: int) -> dict:
    """Per kernel and axis, every counter's mean over the dispatches (warm-up ones included: a
    counter run is not about time) of the counter runs below `directory`."""
    files = glob.glob(os.path.join(directory, "**", "*counter_collection.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no counter collection under {directory}")
    out = collections.defaultdict(dict)
    for path in sorted(files):
        # (kernel, dispatch) -> counter -> the sum of its rows
        values = collections.defaultdict(lambda: collections.defaultdict(float))
        with open(path, newline="") as fh:
            for row in csv.DictReader(fh):
                kernel = _kernel_of(row["Kernel_Name"])
                if kernel is not None:
                    values[kernel, int(row["Dispatch_Id"])][row["Counter_Name"]] += float(
                        row["Counter_Value"])
        ordered = lambda kernel: [v for (k, _), v in sorted(values.items(), key=lambda e: e[0][1])
                                  if k == kernel]
        groups = {"scalar_stats": ordered("scalar_stats_kernel")}
        for kernel, suffix in (("gradient_kernel", ""), ("gradient_halo_kernel", "_halo")):
            dispatches = ordered(kernel)
            if not dispatches:
                continue
            if len(dispatches) != len(AXES) * (warmup + frames):
                raise SystemExit(f"{path}: {len(dispatches)} dispatches of {kernel}, expected "
                                 f"{len(AXES) * (warmup + frames)}")
            for index, label in enumerate(AXES):
                groups[label + suffix] = dispatches[index * (warmup + frames):
                                                    (index + 1) * (warmup + frames)]
        for label, dispatches in groups.items():
            for counter in sorted({c for d in dispatches for c in d}):
                out[label][counter] = sum(d[counter] for d in dispatches) / len(dispatches)
    return out


if __name__ == "__main__":
    parser = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    parser.add_argument("--frames", type=int, default=10)
    parser.add_argument("--warmup", type=int, default=3)
    parser.add_argument("--trace", help="directory of a rocprofv3 --kernel-trace run of this tool")
    parser.add_argument("--counters", help="directory above the rocprofv3 --pmc runs of this tool")
    args = parser.parse_args()
    if args.trace:
        print(json.dumps(read_trace(args.trace, args.frames, args.warmup), indent=1))
    elif args.counters:
        print(json.dumps(read_counters(args.counters, args.frames, args.warmup), indent=1))
    else:
        print(json.dumps(run(args.frames, args.warmup)))
