"""Joint-histogram timing on config-4 (176 boxes of 128^3, 2.95 GB per field), one rank.  The second
and third field are derived from the first on the device (its square; a copy rolled by one cell
along x), so all three share one box list.  Timed: the joint histogram at 64 x 64, 256 x 256 and
1024 x 1024 linear bins, each without and with a summed field, one 64 x 64 histogram whose cells all
fall into one bin, and -- the yardstick -- Scene.histogram (histogram_kernel, 256 bins) on the same
scene.  Event times on the context's stream are printed as one JSON line; the kernels' own times
come from a kernel trace of the same run, which this tool then reads back:

  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/joint_histogram_timing.py
  python tools/joint_histogram_timing.py --trace OUT

The dispatches of one kernel differ only in their arguments, so --trace tells the cases apart by
their order, which is the order of CASES below with --warmup + --frames dispatches each.  Needs a HIP
device: fails loudly without one."""
import argparse
import csv
import glob
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

BINS = (64, 256, 1024)
# (label, kernel, bytes read per cell)
CASES = [("histogram_256", "histogram_kernel", 8)] + \
        [(f"joint_{n}x{n}{'_s' if s else ''}", "joint_histogram_kernel", 24 if s else 16)
         for n in BINS for s in (False, True)] + \
        [("joint_64x64_one_bin", "joint_histogram_kernel", 16),
         ("joint_64x64_one_bin_s", "joint_histogram_kernel", 24)]


def run(frames: int, warmup: int) -> dict:
    import torch
    from amrvolumerenderer_amd import api, runtime, scenes
    from amrvolumerenderer_amd.types import AmrBox, ScalarTransform
    if not torch.cuda.is_available():
        raise SystemExit("tools/joint_histogram_timing.py needs a HIP device")
    ctx = runtime.Context(0)
    spec = scenes.config4("smooth")
    x_cells = [scenes.box_cells_torch(spec, i, ctx.device) for i in range(len(spec.boxes))]
    y_cells = [c * c for c in x_cells]
    s_cells = [torch.roll(c, 1, dims=2) for c in x_cells]
    torch.cuda.synchronize()

    def scene_of(cells):
        boxes = [AmrBox(m.min_corner, m.max_corner, c, m.level) for c, m in zip(cells, spec.boxes)]
        return ctx.create_scene(boxes, ScalarTransform())

    sx, sy, ss = scene_of(x_cells), scene_of(y_cells), scene_of(s_cells)
    n_cells = spec.total_cells
    x_lo, x_hi, x_lo_positive, finite = sx.scalar_stats()
    y_lo, y_hi, _, _ = sy.scalar_stats()
    n_levels = 1 + max(int(m.level) for m in spec.boxes)
    result = {"config": "config-4", "boxes": len(spec.boxes), "cells": n_cells, "frames": frames,
              "warmup": warmup, "x_range": [x_lo, x_hi], "y_range": [y_lo, y_hi]}

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

    def report(label, ms, bytes_per_cell):
        result[label + "_ms"] = round(ms, 4)
        result[label + "_TBps"] = round(n_cells * bytes_per_cell / ms / 1e9, 3)

    transform, _, rng = runtime.scene_transform_from_stats((x_lo, x_hi, x_lo_positive), finite, False, True)
    counts = torch.zeros(256, dtype=torch.int64, device=ctx.device)
    report("histogram_256", timed(lambda: sx.histogram(transform, rng[0], rng[1], 256, counts)), 8)
    assert int(counts.sum().item()) == n_cells * (warmup + frames)

    def joint(label, xe, ye, with_s):
        outs = sx.joint_histogram(xe, sy, ye, ss if with_s else None, n_levels)
        for t in outs:
            if t is not None:
                t.zero_()
        report(label, timed(lambda: sx.joint_histogram(xe, sy, ye, ss if with_s else None,
                                                       n_levels, *outs)),
               24 if with_s else 16)
        ctx.synchronize()
        binned = int(outs[0].sum().item()) + int(outs[2].sum().item())
        assert binned == n_cells * (warmup + frames), (label, binned)
        result[label + "_filled_bins"] = int((outs[0].sum(dim=0) > 0).sum().item())

    for n in BINS:
        xe, ye = api.bin_edges(x_lo, x_hi, n), api.bin_edges(y_lo, y_hi, n)
        for with_s in (False, True):
            joint(f"joint_{n}x{n}{'_s' if with_s else ''}", xe, ye, with_s)
    # every cell in bin (0, 0): the first bin spans the data, the other 63 lie above it
    span_x, span_y = x_hi - x_lo + 1.0, y_hi - y_lo + 1.0
    xe = [x_lo] + [x_hi + span_x * (i + 1) / 64.0 for i in range(64)]
    ye = [y_lo] + [y_hi + span_y * (i + 1) / 64.0 for i in range(64)]
    joint("joint_64x64_one_bin", xe, ye, False)
    joint("joint_64x64_one_bin_s", xe, ye, True)
    return result


def read_trace(directory: str, frames: int, warmup: int) -> dict:
    """Per case the mean and the smallest kernel time of its timed dispatches, from the kernel
    trace of one run of this tool."""
    files = glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True)
    if len(files) != 1:
        raise SystemExit(f"expected one kernel trace under {directory}, found {len(files)}")
    rows = {"histogram_kernel": [], "joint_histogram_kernel": []}
    with open(files[0], newline="") as fh:
        for row in csv.DictReader(fh):
            name = row["Kernel_Name"]
            for kernel in rows:
                # demangled (avr::(anonymous namespace)::NAME<...>) or mangled (<length>NAME I ...)
                if f"::{kernel}<" in name or f"{len(kernel)}{kernel}I" in name:
                    rows[kernel].append((int(row["Start_Timestamp"]), int(row["End_Timestamp"]),
                                         row["Kernel_Name"]))
    out, cells = {}, 176 * 128 ** 3
    per_case = frames + warmup
    taken = {kernel: 0 for kernel in rows}
    for kernel in rows:
        rows[kernel].sort()
    for label, kernel, bytes_per_cell in CASES:
        extra = 1 if kernel == "joint_histogram_kernel" else 0    # the call that made the arrays
        first = taken[kernel] + extra + warmup
        mine = rows[kernel][first:first + frames]
        taken[kernel] += extra + per_case
        if len(mine) != frames:
            raise SystemExit(f"the trace holds too few dispatches of {kernel} for {label}")
        times = [(end - start) * 1e-6 for start, end, _ in mine]
        mean = sum(times) / len(times)
        out[label] = {"mean_ms": round(mean, 4), "min_ms": round(min(times), 4),
                      "TBps": round(cells * bytes_per_cell / mean / 1e9, 3),
                      "kernel": mine[0][2][:96]}
    base = out["histogram_256"]["TBps"]
    for label in out:
        out[label]["per_byte_vs_histogram"] = round(out[label]["TBps"] / base, 3)
    return out


if __name__ == "__main__":
    parser = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    parser.add_argument("--frames", type=int, default=5)
    parser.add_argument("--warmup", type=int, default=2)
    parser.add_argument("--trace", help="directory of a rocprofv3 --kernel-trace run of this tool")
    args = parser.parse_args()
    if args.trace:
        print(json.dumps(read_trace(args.trace, args.frames, args.warmup), indent=1))
    else:
        print(json.dumps(run(args.frames, args.warmup)))
