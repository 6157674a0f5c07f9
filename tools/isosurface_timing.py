"""Isosurface timing on config-4 (176 boxes of 128^3, 2.95 GB per field), one rank, two workloads:
"few" -- the smooth field at 0.2, a surface that cuts few cubes -- and "many" -- the noise field
(uniform in [0, 1)) at 0.98, which cuts about one cube in seven (at 0.5 nearly every cube is cut
and the triangles no longer fit the device).  Scene.isosurface is timed with events on the
context's stream as the count-only call and as the emitting call at the counted capacity; in the
same run the yardstick, Scene.scalar_stats (scalar_stats_kernel) on the same scene, is timed as a call.  One
JSON line is printed.  The kernels' own times come from a kernel trace of the same run, which this
tool then reads back:

  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/isosurface_timing.py
  python tools/isosurface_timing.py --trace OUT

--trace tells the passes apart by the order of the dispatches -- per workload --warmup + --frames
count-only calls, then as many emitting calls, each of which counts first -- and gives every
kernel's mean time and, for the count pass (8 B read per cell), its ratio to scalar_stats_kernel
per byte.  Needs a HIP device: fails loudly without one."""
import argparse
import csv
import glob
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WORKLOADS = (("few", "smooth", 0.2), ("many", "noise", 0.98))
CELLS = 176 * 128 ** 3
KERNELS = ("scalar_stats_kernel", "iso_shell_kernel", "iso_cubes_kernel", "iso_scan_kernel")
MAX_TRIANGLES = 1 << 28          # 72 B each: the emitting call is left out above it


def run(frames: int, warmup: int) -> dict:
    import numpy as np
    import torch
    from amrvolumerenderer_amd import runtime, scenes
    from amrvolumerenderer_amd.types import AmrBox, ScalarTransform
    if not torch.cuda.is_available():
        raise SystemExit("tools/isosurface_timing.py needs a HIP device")
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

    for label, field_name, value in WORKLOADS:
        spec = scenes.config4(field_name)
        cells = [scenes.box_cells_torch(spec, i, ctx.device) for i in range(len(spec.boxes))]
        torch.cuda.synchronize()
        boxes = [AmrBox(m.min_corner, m.max_corner, c, m.level) for c, m in zip(cells, spec.boxes)]
        field = ctx.create_scene(boxes, ScalarTransform())
        n_levels = 1 + max(int(m.level) for m in spec.boxes)
        index = np.array([m.lo for m in spec.boxes], dtype=np.int32)
        ratios = [2] * (n_levels - 1)
        sizes = np.zeros((n_levels, 3))
        for m in spec.boxes:
            sizes[m.level] = [(m.max_corner[a] - m.min_corner[a]) / m.dims[a] for a in range(3)]
        origin = [0.0, 0.0, 0.0]
        stats_ms = timed(field.scalar_stats)
        counts = torch.zeros(2, dtype=torch.int64, device=ctx.device)
        count_ms = timed(lambda: field.isosurface(value, index, ratios, sizes, origin,
                                                  counts=counts))
        ctx.synchronize()
        n, skipped = (int(v) for v in counts.cpu().tolist())
        entry = {"field": field_name, "value": value, "triangles": n, "skipped": skipped,
                 "scalar_stats_call_ms": round(stats_ms, 4), "count_call_ms": round(count_ms, 4)}
        if 0 < n <= MAX_TRIANGLES:
            ms = timed(lambda: field.isosurface(value, index, ratios, sizes, origin, capacity=n,
                                                counts=counts))
            entry["emit_call_ms"] = round(ms, 4)
        result[label] = entry
        field.close()
        del cells, boxes
        torch.cuda.empty_cache()
    return result


def _kernel_of(name: str):
    for kernel in KERNELS:
        if f"::{kernel}" in name or f"{len(kernel)}{kernel}" in name:
            return kernel
    return None


def read_trace(directory: str, frames: int, warmup: int) -> dict:
    """Per workload the mean and smallest time of the shell kernel, the count pass, the scan and
    the emit pass over the timed dispatches, and the count pass's ratio to scalar_stats_kernel per
    byte read."""
    files = glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True)
    if len(files) != 1:
        raise SystemExit(f"expected one kernel trace under {directory}, found {len(files)}")
    rows = {kernel: [] for kernel in KERNELS}
    with open(files[0], newline="") as fh:
        for row in csv.DictReader(fh):
            kernel = _kernel_of(row["Kernel_Name"])
            if kernel is not None:
                rows[kernel].append((int(row["Start_Timestamp"]), int(row["End_Timestamp"])))
    for kernel in KERNELS:
        rows[kernel].sort()
    calls = warmup + frames

    def stats(kernel, positions):
        times = [(rows[kernel][p][1] - rows[kernel][p][0]) * 1e-6 for p in positions
                 if p < len(rows[kernel])]
        if len(times) != frames:
            return None
        return {"mean_ms": round(sum(times) / frames, 4), "min_ms": round(min(times), 4)}

    out = {}
    cubes_before = 0          # dispatches of iso_cubes_kernel by the workloads before this one
    for index, (label, _, _) in enumerate(WORKLOADS):
        emitted = len(rows["iso_cubes_kernel"]) - cubes_before >= 3 * calls
        entry = {"scalar_stats_kernel": stats("scalar_stats_kernel",
                                              range(index * calls + warmup, (index + 1) * calls))}
        # a count-only call dispatches the cubes kernel once, an emitting call twice
        entry["count_pass"] = stats("iso_cubes_kernel",
                                    range(cubes_before + warmup, cubes_before + calls))
        if emitted:
            first = cubes_before + calls + 2 * warmup
            entry["emit_pass"] = stats("iso_cubes_kernel", range(first + 1, first + 2 * frames, 2))
        out[label] = entry
        cubes_before += 3 * calls if emitted else calls
    # the shell kernel and the scan run once per call of either kind
    before = 0
    for index, (label, _, _) in enumerate(WORKLOADS):
        emitted = "emit_pass" in out[label]
        out[label]["iso_shell_kernel"] = stats("iso_shell_kernel", range(before + warmup, before + calls))
        out[label]["iso_scan_kernel"] = stats("iso_scan_kernel", range(before + warmup, before + calls))
        before += 2 * calls if emitted else calls
        yardstick, count = out[label]["scalar_stats_kernel"], out[label]["count_pass"]
        if yardstick and count:
            count["bytes_per_cell"] = 8
            count["per_byte_vs_scalar_stats"] = round(count["mean_ms"] / yardstick["mean_ms"], 3)
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
