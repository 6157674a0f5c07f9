"""Clump-tree timing on config-4 (176 boxes of 128^3, 2.95 GB per field), one rank, the two
workloads of tools/clump_timing.py: "large" -- the smooth field above 0.2, a few large clumps --
and "small" -- the noise field above 0.75, a quarter of the cells in small clumps.  Per workload
two label scenes are made, of the workload's threshold (the parents) and of the ladder's next one
(the labels), and on the labels these are timed with events on the context's stream, in this
order: Scene.scalar_stats (the yardstick, as a call), Scene.clump_table without a field,
Scene.clump_links without and with the parent scene, and Scene.clump_table once more, so that the
trace shows what two runs of one kernel differ by.  After both workloads the whole six-threshold
api.clump_tree_scene call is timed on each, --tree-warmup + --tree-frames calls.  One JSON line is
printed.  The kernels' own times come from a kernel trace of the same run, which this tool then
reads back:

  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/clump_tree_timing.py
  python tools/clump_tree_timing.py --trace OUT

--trace tells the workloads apart by the order of the dispatches (large, then small, --warmup +
--frames dispatches per timed loop; the tree calls' dispatches come after all of them) and gives
every kernel's mean and smallest time and its ratio to scalar_stats_kernel per byte moved
(scalar_stats 8 B per cell, the table without a field 8 B, the links 8 B, or 16 B with a parent
scene).  Needs a HIP device: fails loudly without one."""
import argparse
import csv
import glob
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# (label, field, the six thresholds: the first is the workload's, the second the labels')
WORKLOADS = (("large", "smooth", (0.2, 0.3, 0.4, 0.5, 0.6, 0.7)),
             ("small", "noise", (0.75, 0.8, 0.85, 0.9, 0.95, 0.99)))
CELLS = 176 * 128 ** 3
# kernel as the trace names it -> (bytes per cell, timed loops per workload)
KERNELS = {"scalar_stats_kernel": (8, 1), "clump_table_kernel<false>": (8, 2),
           "clump_link_kernel<false>": (8, 1), "clump_link_kernel<true>": (16, 1)}


def run(frames: int, warmup: int, tree_frames: int, tree_warmup: int) -> dict:
    import time

    import numpy as np
    import torch
    from amrvolumerenderer_amd import api, runtime, scenes
    from amrvolumerenderer_amd.types import AmrBox, ScalarTransform
    if not torch.cuda.is_available():
        raise SystemExit("tools/clump_tree_timing.py needs a HIP device")
    ctx = runtime.Context(0)
    result = {"config": "config-4", "cells": CELLS, "frames": frames, "warmup": warmup,
              "tree_frames": tree_frames, "tree_warmup": tree_warmup}

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
        return round(begin.elapsed_time(end) / frames, 4)

    geometries = {}
    for label, field_name, thresholds in WORKLOADS:
        spec = scenes.config4(field_name)
        first = [scenes.box_cells_torch(spec, i, ctx.device) for i in range(len(spec.boxes))]
        torch.cuda.synchronize()

        def boxes_of(tensors):
            return [AmrBox(m.min_corner, m.max_corner, c, m.level)
                    for c, m in zip(tensors, spec.boxes)]

        n_levels = 1 + max(int(m.level) for m in spec.boxes)
        index = np.array([m.lo for m in spec.boxes], dtype=np.int32)
        ratios = [2] * (n_levels - 1)
        field = ctx.create_scene(boxes_of(first), ScalarTransform())
        made, counts = [], []
        for threshold in thresholds[:2]:
            out = ctx.create_scene(boxes_of([torch.empty_like(c) for c in first]), ScalarTransform())
            count = out.clumps(field, threshold, float("inf"), index, ratios)
            ctx.synchronize()
            made.append(out)
            counts.append(int(count.item()))
        parents, labels = made
        n_parents, n = counts
        entry = {"field": field_name, "thresholds": list(thresholds), "n_parents": n_parents,
                 "n_clumps": n}
        if 0 < n and n * n_levels < (1 << 28):
            cells = torch.zeros((n_levels, n), dtype=torch.int64, device=ctx.device)
            totals = torch.zeros(2, dtype=torch.int64, device=ctx.device)
            entry["scalar_stats_call_ms"] = timed(labels.scalar_stats)
            entry["table_call_ms"] = timed(lambda: labels.clump_table(n, n_levels, None, cells,
                                                                       None, totals))
            extent, _, _, link_totals = labels.clump_links(n, index, ratios)
            entry["links_call_ms"] = timed(lambda: labels.clump_links(
                n, index, ratios, extent=extent, totals=link_totals))
            _, low, high, _ = labels.clump_links(n, index, ratios, parents, n_parents,
                                                 extent=extent, totals=link_totals)
            entry["links_with_parents_call_ms"] = timed(lambda: labels.clump_links(
                n, index, ratios, parents, n_parents, extent, low, high, link_totals))
            entry["table_again_call_ms"] = timed(lambda: labels.clump_table(n, n_levels, None,
                                                                             cells, None, totals))
            ctx.synchronize()
            entry["split_parents"] = int((low != high).sum().item())
        for scene in (field, parents, labels):
            scene.close()
        del made, parents, labels
        torch.cuda.empty_cache()
        result[label] = entry
        boxes = boxes_of(first)
        geometries[label] = (api.SceneGeometry(boxes, boxes, ScalarTransform(), spec.bounds),
                             [(spec.extent / (spec.n0 << l),) * 3 for l in range(n_levels)],
                             ratios, thresholds)
        del first

    # the lone warm-up + timed link calls above (made to allocate the outputs) are two dispatches
    # more per link kernel and workload: read_trace counts them
    for label, (geometry, sizes, ratios, thresholds) in geometries.items():
        times = []
        for call in range(tree_warmup + tree_frames):
            ctx.synchronize()
            begin = time.perf_counter()
            tree = api.clump_tree_scene(ctx, geometry, thresholds, float("inf"), sizes,
                                        (0.0, 0.0, 0.0), ratios)
            ctx.synchronize()
            if call >= tree_warmup:
                times.append((time.perf_counter() - begin) * 1e3)
        result[label]["tree_call_ms"] = round(sum(times) / max(len(times), 1), 3)
        result[label]["tree_counts"] = tree["counts"]
    return result


def read_trace(directory: str, frames: int, warmup: int) -> dict:
    """Per workload every kernel's mean and smallest time over the timed dispatches of each of its
    loops and its ratio to scalar_stats_kernel per byte."""
    files = glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True)
    if len(files) != 1:
        raise SystemExit(f"expected one kernel trace under {directory}, found {len(files)}")
    rows = {kernel: [] for kernel in KERNELS}
    with open(files[0], newline="") as fh:
        for row in csv.DictReader(fh):
            for kernel in KERNELS:
                if kernel in row["Kernel_Name"]:
                    rows[kernel].append((int(row["Start_Timestamp"]), int(row["End_Timestamp"])))
    out = {}
    for index, (label, _, _) in enumerate(WORKLOADS):
        entry = {}
        for kernel, (moved, loops) in KERNELS.items():
            # a link kernel's loop is preceded by the one call that allocated its outputs
            lone = 1 if "link" in kernel else 0
            per_workload = loops * (warmup + frames) + lone
            for loop in range(loops):
                first = index * per_workload + lone + loop * (warmup + frames) + warmup
                times = [(end - start) * 1e-6
                         for start, end in sorted(rows[kernel])[first:first + frames]]
                if len(times) != frames:
                    continue
                entry[kernel if loop == 0 else kernel + " again"] = {
                    "mean_ms": round(sum(times) / frames, 4), "min_ms": round(min(times), 4),
                    "max_ms": round(max(times), 4), "bytes_per_cell": moved}
        per_byte = entry["scalar_stats_kernel"]["mean_ms"] / 8
        for name, figures in entry.items():
            figures["per_byte_vs_scalar_stats"] = round(
                figures["mean_ms"] / figures["bytes_per_cell"] / per_byte, 3)
        out[label] = entry
    return out


if __name__ == "__main__":
    parser = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    parser.add_argument("--frames", type=int, default=10)
    parser.add_argument("--warmup", type=int, default=3)
    parser.add_argument("--tree-frames", type=int, default=3)
    parser.add_argument("--tree-warmup", type=int, default=1)
    parser.add_argument("--trace", help="directory of a rocprofv3 --kernel-trace run of this tool")
    args = parser.parse_args()
    if args.trace:
        print(json.dumps(read_trace(args.trace, args.frames, args.warmup), indent=1))
    else:
        print(json.dumps(run(args.frames, args.warmup, args.tree_frames, args.tree_warmup)))
