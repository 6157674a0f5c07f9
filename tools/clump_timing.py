"""Clump timing on config-4 (176 boxes of 128^3, 2.95 GB per field), one rank, two workloads:
"large" -- the smooth field above 0.2, a few large clumps -- and "small" -- the noise field above
0.75, a quarter of the cells in small clumps (uniform noise percolates into one clump well before
half the cells are selected).  Scene.clumps (six kernels) and Scene.clump_table with the field
summed are timed with events on the context's stream; in the same run the yardstick,
Scene.scalar_stats (scalar_stats_kernel) on the same scene, is timed as a call.  One JSON line is
printed.  The kernels' own times come from a kernel trace of the same run, which this tool then
reads back:

  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/clump_timing.py
  python tools/clump_timing.py --trace OUT

--trace tells the workloads apart by the order of the dispatches, which is large, small with
--warmup + --frames dispatches each, and gives every kernel's mean time and its ratio to
scalar_stats_kernel per byte moved (init 8 B read + 4 B written per cell, flatten 8 B, labels 4 B
read + 8 B written, table 16 B read; merge, scan and rank have no such count and are given as
times).  Needs a HIP device: fails loudly without one."""
import argparse
import csv
import glob
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WORKLOADS = (("large", "smooth", 0.2), ("small", "noise", 0.75))
CELLS = 176 * 128 ** 3
BYTES = {"clump_init_kernel": 12, "clump_flatten_kernel": 8, "clump_label_kernel": 12,
         "clump_table_kernel": 16, "clump_merge_kernel": None, "clump_scan_kernel": None,
         "clump_rank_kernel": None}
KERNELS = ("scalar_stats_kernel",) + tuple(BYTES)


def run(frames: int, warmup: int) -> dict:
    import numpy as np
    import torch
    from amrvolumerenderer_amd import runtime, scenes
    from amrvolumerenderer_amd.types import AmrBox, ScalarTransform
    if not torch.cuda.is_available():
        raise SystemExit("tools/clump_timing.py needs a HIP device")
    ctx = runtime.Context(0)
    result = {"config": "config-4", "cells": CELLS, "frames": frames, "warmup": warmup}

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

    for label, field_name, lower in WORKLOADS:
        spec = scenes.config4(field_name)
        first = [scenes.box_cells_torch(spec, i, ctx.device) for i in range(len(spec.boxes))]
        target = [torch.empty_like(c) for c in first]
        torch.cuda.synchronize()

        def scene_of(tensors):
            boxes = [AmrBox(m.min_corner, m.max_corner, c, m.level)
                     for c, m in zip(tensors, spec.boxes)]
            return ctx.create_scene(boxes, ScalarTransform())

        field, out = scene_of(first), scene_of(target)
        n_levels = 1 + max(int(m.level) for m in spec.boxes)
        index = np.array([m.lo for m in spec.boxes], dtype=np.int32)
        ratios = [2] * (n_levels - 1)
        stats_ms = timed(field.scalar_stats)
        count = torch.zeros(1, dtype=torch.int64, device=ctx.device)
        ms = timed(lambda: out.clumps(field, lower, float("inf"), index, ratios, count))
        ctx.synchronize()
        n = int(count.item())
        result[label] = {"field": field_name, "lower": lower, "n_clumps": n,
                         "scalar_stats_call_ms": round(stats_ms, 4), "clumps_call_ms": round(ms, 4)}
        if 0 < n and n * n_levels < (1 << 28):
            cells = torch.zeros((n_levels, n), dtype=torch.int64, device=ctx.device)
            sums = torch.zeros((n_levels, n), dtype=torch.float64, device=ctx.device)
            totals = torch.zeros(2, dtype=torch.int64, device=ctx.device)
            ms = timed(lambda: out.clump_table(n, n_levels, field, cells, sums, totals))
            result[label]["table_call_ms"] = round(ms, 4)
        field.close()
        out.close()
        del first, target
        torch.cuda.empty_cache()
    return result


def _kernel_of(name: str):
    for kernel in KERNELS:
        if f"::{kernel}" in name or f"{len(kernel)}{kernel}" in name:
            return kernel
    return None


def read_trace(directory: str, frames: int, warmup: int) -> dict:
    """Per workload every kernel's mean and smallest time over the timed dispatches and, where the
    bytes moved are counted, its ratio to scalar_stats_kernel per byte."""
    files = glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True)
    if len(files) != 1:
        raise SystemExit(f"expected one kernel trace under {directory}, found {len(files)}")
    rows = {kernel: [] for kernel in KERNELS}
    with open(files[0], newline="") as fh:
        for row in csv.DictReader(fh):
            kernel = _kernel_of(row["Kernel_Name"])
            if kernel is not None:
                rows[kernel].append((int(row["Start_Timestamp"]), int(row["End_Timestamp"])))
    out = {}
    for index, (label, _, _) in enumerate(WORKLOADS):
        first = index * (warmup + frames) + warmup
        entry = {}
        for kernel in KERNELS:
            times = [(end - start) * 1e-6 for start, end in sorted(rows[kernel])[first:first + frames]]
            if len(times) != frames:
                continue              # the table does not run for a workload without clumps
            entry[kernel] = {"mean_ms": round(sum(times) / frames, 4), "min_ms": round(min(times), 4)}
        per_byte = entry["scalar_stats_kernel"]["mean_ms"] / 8
        for kernel, moved in BYTES.items():
            if moved is not None and kernel in entry:
                entry[kernel]["bytes_per_cell"] = moved
                entry[kernel]["per_byte_vs_scalar_stats"] = round(
                    entry[kernel]["mean_ms"] / moved / per_byte, 3)
        out[label] = entry
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
