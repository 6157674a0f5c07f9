"""Velocity cube timing on config-4 (176 boxes of 128^3, 2.95 GB per field), one rank, at 512 x 512
pixels over the whole data.  The velocity g and the width s are made from the emission e on the
device (g = e, so the channels span e's range; s = 2 channel widths everywhere), so all three
share one box list.  Per axis, for 1, 64 and 256 channels, sharp and broadened, events on the
context's stream time the whole call (every batch's reduce and gather).  In the same run the
yardstick, the parent's unchanged weighted on-axis projection of the same two fields
(Scene.axis_projection of e weighted by g: axis_reduce_columns_kernel<AXIS, true>, or the rows
kernel on x), is timed the same way.  One JSON line is printed.  The kernels' own times come from a
kernel trace of the same run, which this tool then reads back:

  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/velocity_cube_timing.py
  python tools/velocity_cube_timing.py --trace OUT

--trace tells the cases apart by the order of the dispatches, which is the order of the cases
below; a call dispatches one reduce kernel per batch of channels, and their times are added per
call.  --axes, --channels and --modes cut the run down (the same options go to --trace).  Needs a
HIP device: fails loudly without one."""
import argparse
import csv
import glob
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZE = 512
BOXES, SIDE = 176, 128
ENTRIES = BOXES * SIDE * SIDE            # of one partial plane: columns of 128 cells, one segment
BOUND = 1 << 27


def batches(nc: int) -> int:
    batch = min(nc, BOUND // ENTRIES)
    return -(-nc // batch)


def cases(args):
    """(label, axis, nc, broadened) in the order they run; per axis the yardstick comes first."""
    return [(f"{'xyz'[axis]}_{nc}_{mode}", axis, nc, mode == "broadened")
            for axis in args.axes for nc in args.channels for mode in args.modes]


def run(args) -> dict:
    import numpy as np
    import torch
    from amrvolumerenderer_amd import runtime, scenes
    from amrvolumerenderer_amd.types import AmrBox, ScalarTransform
    if not torch.cuda.is_available():
        raise SystemExit("tools/velocity_cube_timing.py needs a HIP device")
    ctx = runtime.Context(0)
    spec = scenes.config4("smooth")
    assert len(spec.boxes) == BOXES
    e_cells = [scenes.box_cells_torch(spec, i, ctx.device) for i in range(len(spec.boxes))]
    g_cells = [c.clone() for c in e_cells]
    s_cells = [torch.zeros_like(c) for c in e_cells]
    torch.cuda.synchronize()

    def scene_of(cells):
        boxes = [AmrBox(m.min_corner, m.max_corner, c, m.level) for c, m in zip(cells, spec.boxes)]
        return ctx.create_scene(boxes, ScalarTransform())

    se, sg, ss = scene_of(e_cells), scene_of(g_cells), scene_of(s_cells)
    g_lo, g_hi = se.scalar_stats()[:2]
    n_levels = 1 + max(int(m.level) for m in spec.boxes)
    dl = [1.0 / (1 << level) for level in range(n_levels)]
    lo = [min(m.min_corner[a] for m in spec.boxes) for a in range(3)]
    hi = [max(m.max_corner[a] for m in spec.boxes) for a in range(3)]
    result = {"config": "config-4", "boxes": len(spec.boxes), "cells": spec.total_cells,
              "frames": args.frames, "warmup": args.warmup, "size": SIZE}

    def timed(call):
        for _ in range(args.warmup):
            call()
        ctx.synchronize()
        begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        begin.record(ctx.stream)
        for _ in range(args.frames):
            call()
        end.record(ctx.stream)
        end.synchronize()
        return begin.elapsed_time(end) / args.frames

    images = [torch.empty((SIZE, SIZE), dtype=torch.float64, device=ctx.device) for _ in range(3)]
    done = set()
    for label, axis, nc, broadened in cases(args):
        au, av = (axis + 1) % 3, (axis + 2) % 3
        window = ((lo[au], lo[av]), (hi[au] - lo[au]) / SIZE, (hi[av] - lo[av]) / SIZE, SIZE, SIZE)
        if axis not in done:
            done.add(axis)
            ms = timed(lambda: se.axis_projection(axis, *window, dl, sg, *images))
            result[f"{'xyz'[axis]}_weighted_projection_ms"] = round(ms, 4)
        edges = np.linspace(g_lo, g_hi, nc + 1)
        if broadened:
            for c in s_cells:
                c.fill_(2.0 * (g_hi - g_lo) / nc)
            torch.cuda.synchronize()
        cube = torch.empty((nc, SIZE, SIZE), dtype=torch.float64, device=ctx.device)
        ms = timed(lambda: se.velocity_cube(sg, edges, axis, *window, dl, ss if broadened else None,
                                            cube, *images))
        ctx.synchronize()
        result[label + "_ms"] = round(ms, 4)
        result[label + "_vs_projection"] = round(
            ms / result[f"{'xyz'[axis]}_weighted_projection_ms"], 2)
        del cube
    return result


def read_trace(directory: str, args) -> dict:
    """Per case the mean and the smallest per-call sum of the kernel times of its reduce and gather
    dispatches, and per axis those of the weighted projection's reduce kernel, from the kernel
    trace of one run; `vs_projection` is the ratio of the reduce means."""
    files = glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True)
    if len(files) != 1:
        raise SystemExit(f"expected one kernel trace under {directory}, found {len(files)}")
    kernels = ("axis_reduce_rows_kernel", "axis_reduce_columns_kernel", "cube_reduce_rows_kernel",
               "cube_reduce_columns_kernel", "cube_gather_kernel")
    rows = {kernel: [] for kernel in kernels}
    with open(files[0], newline="") as fh:
        for row in csv.DictReader(fh):
            name = row["Kernel_Name"]
            for kernel in kernels:
                if f"::{kernel}" in name or f"{len(kernel)}{kernel}" in name:
                    rows[kernel].append((int(row["Start_Timestamp"]), int(row["End_Timestamp"])))
    for kernel in rows:
        rows[kernel].sort()
    taken = {kernel: 0 for kernel in kernels}

    def calls(kernel, per_call):
        """The timed calls' summed times of the next warmup + frames calls of `kernel`."""
        first = taken[kernel] + args.warmup * per_call
        taken[kernel] += (args.warmup + args.frames) * per_call
        times = rows[kernel][first:first + args.frames * per_call]
        if len(times) != args.frames * per_call:
            raise SystemExit("the trace holds too few dispatches")
        sums = [sum((end - start) * 1e-6 for start, end in times[i * per_call:(i + 1) * per_call])
                for i in range(args.frames)]
        return {"mean_ms": round(sum(sums) / len(sums), 4), "min_ms": round(min(sums), 4)}

    out, yardstick = {}, {}
    for label, axis, nc, _ in cases(args):
        if axis not in yardstick:
            yardstick[axis] = calls("axis_reduce_rows_kernel" if axis == 0 else
                                    "axis_reduce_columns_kernel", 1)
            out[f"{'xyz'[axis]}_weighted_projection_reduce"] = yardstick[axis]
        reduce = calls("cube_reduce_rows_kernel" if axis == 0 else "cube_reduce_columns_kernel",
                       batches(nc))
        reduce["vs_projection"] = round(reduce["mean_ms"] / yardstick[axis]["mean_ms"], 2)
        out[label + "_reduce"] = reduce
        out[label + "_gather"] = calls("cube_gather_kernel", batches(nc))
    return out


if __name__ == "__main__":
    parser = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    parser.add_argument("--frames", type=int, default=10)
    parser.add_argument("--warmup", type=int, default=3)
    parser.add_argument("--axes", type=int, nargs="+", default=[0, 1, 2])
    parser.add_argument("--channels", type=int, nargs="+", default=[1, 64, 256])
    parser.add_argument("--modes", nargs="+", default=["sharp", "broadened"],
                        choices=["sharp", "broadened"])
    parser.add_argument("--trace", help="directory of a rocprofv3 --kernel-trace run of this tool")
    args = parser.parse_args()
    if args.trace:
        print(json.dumps(read_trace(args.trace, args), indent=1))
    else:
        print(json.dumps(run(args)))
