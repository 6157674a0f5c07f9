"""Derived-field timing on config-4 (176 boxes of 128^3, 2.95 GB per field), one rank.  The extra
fields are made from the first on the device, so all share one box list.  Five programs -- copy (1
field), product (2), velocity magnitude (3), kinetic energy (4) and radius (no field) -- are timed
with events on the context's stream around Scene.derive; a program moves 8 * (fields + 1) bytes
per cell.  In the same run the yardstick, Scene.scalar_stats (scalar_stats_kernel) on the same
scene, is timed as a call: it synchronises and allocates, so its event time is an upper bound of
the kernel's.  One JSON line is printed.  The kernels' own times come from a kernel trace of the
same run, which this tool then reads back:

  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/derive_timing.py
  python tools/derive_timing.py --trace OUT

Hardware counters come from runs of their own, never together with a trace, one run per group of
counters that the hardware can hold at once, all below one directory, and are read back likewise
(per kernel and program the mean over the dispatches; a counter's rows of one dispatch are summed):

  rocprofv3 --kernel-include-regex "derive_kernel|scalar_stats_kernel" --pmc SQ_WAVES ... \
      --output-format csv -d OUT/pass0 -- python tools/derive_timing.py --programs copy,radius
  python tools/derive_timing.py --programs copy,radius --counters OUT

--trace and --counters tell the programs apart by the order of the dispatches of derive_kernel,
which is the order of --programs (all of PROGRAMS below unless given) with --warmup + --frames
dispatches each.  Needs a HIP device: fails loudly without one."""
import argparse
import collections
import csv
import glob
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# (label, expression)
PROGRAMS = [("copy", "a"), ("product", "a * b"), ("velocity_magnitude", "sqrt(a**2 + b**2 + c**2)"),
            ("kinetic_energy", "0.5 * d * (a**2 + b**2 + c**2)"),
            ("radius", "sqrt((x - 0.5)**2 + (y - 0.5)**2 + (z - 0.5)**2)")]
CELLS = 176 * 128 ** 3


def run(frames: int, warmup: int, programs) -> dict:
    import numpy as np
    import torch
    from amrvolumerenderer_amd import api, runtime, scenes
    from amrvolumerenderer_amd.types import AmrBox, ScalarTransform
    if not torch.cuda.is_available():
        raise SystemExit("tools/derive_timing.py needs a HIP device")
    ctx = runtime.Context(0)
    spec = scenes.config4("smooth")
    first = [scenes.box_cells_torch(spec, i, ctx.device) for i in range(len(spec.boxes))]
    compiled = [(label, api.compile_expression(text)) for label, text in programs]
    used = {name for _, program in compiled for name in program.fields}
    make = {"b": lambda c: c * c, "c": lambda c: c + 1.0, "d": lambda c: c * 0.5}
    cells = {"a": first, "out": [torch.empty_like(c) for c in first]}
    cells.update({name: [make[name](c) for c in first] for name in sorted(used - {"a"})})
    torch.cuda.synchronize()

    def scene_of(tensors):
        boxes = [AmrBox(m.min_corner, m.max_corner, c, m.level) for c, m in zip(tensors, spec.boxes)]
        return ctx.create_scene(boxes, ScalarTransform())

    fields = {name: scene_of(tensors) for name, tensors in cells.items()}
    n_cells = spec.total_cells
    n_levels = 1 + max(int(m.level) for m in spec.boxes)
    origin = np.array([m.min_corner for m in spec.boxes], dtype=np.float64)
    sizes = np.array([[(m.max_corner[a] - m.min_corner[a]) / m.dims[a] for a in range(3)]
                      for level in range(n_levels)
                      for m in [next(b for b in spec.boxes if int(b.level) == level)]])
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

    stats_ms = timed(fields["a"].scalar_stats)
    result["scalar_stats_call_ms"] = round(stats_ms, 4)
    result["scalar_stats_call_TBps"] = round(n_cells * 8 / stats_ms / 1e9, 3)
    # what the device's own copy of one field takes (Tensor.copy_ of the 2.95 GB at once): as many
    # bytes read and written as the copy program moves, no interpreter
    whole = torch.cat([c.reshape(-1) for c in first])
    target = torch.empty_like(whole)
    for _ in range(warmup):
        target.copy_(whole)
    begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    begin.record()
    for _ in range(frames):
        target.copy_(whole)
    end.record()
    end.synchronize()
    copy_ms = begin.elapsed_time(end) / frames
    del whole, target
    result["device_copy_ms"] = round(copy_ms, 4)
    result["device_copy_TBps"] = round(n_cells * 16 / copy_ms / 1e9, 3)
    result["device_copy_per_byte_vs_scalar_stats_call"] = round((copy_ms / 16) / (stats_ms / 8), 3)
    for label, program in compiled:
        inputs = [fields[name] for name in program.fields]
        ms = timed(lambda: fields["out"].derive(inputs, program.instructions, program.constants,
                                                origin, sizes))
        moved = 8 * (len(program.fields) + 1)
        result[label + "_ms"] = round(ms, 4)
        result[label + "_bytes_per_cell"] = moved
        result[label + "_TBps"] = round(n_cells * moved / ms / 1e9, 3)
        result[label + "_per_byte_vs_scalar_stats_call"] = round((ms / moved) / (stats_ms / 8), 3)
    return result


def read_trace(directory: str, frames: int, warmup: int, programs) -> dict:
    """Per program the mean and the smallest kernel time of the timed dispatches of derive_kernel,
    and of scalar_stats_kernel, from the kernel trace of one run."""
    files = glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True)
    if len(files) != 1:
        raise SystemExit(f"expected one kernel trace under {directory}, found {len(files)}")
    kernels = ("scalar_stats_kernel", "derive_kernel")
    rows = {kernel: [] for kernel in kernels}
    with open(files[0], newline="") as fh:
        for row in csv.DictReader(fh):
            name = row["Kernel_Name"]
            for kernel in kernels:
                if f"::{kernel}" in name or f"{len(kernel)}{kernel}" in name:
                    rows[kernel].append((int(row["Start_Timestamp"]), int(row["End_Timestamp"])))
    for kernel in rows:
        rows[kernel].sort()

    def summary(times, bytes_per_cell):
        times = [(end - start) * 1e-6 for start, end in times]
        if len(times) != frames:
            raise SystemExit("the trace holds too few dispatches")
        mean = sum(times) / len(times)
        return {"mean_ms": round(mean, 4), "min_ms": round(min(times), 4),
                "bytes_per_cell": bytes_per_cell,
                "TBps": round(CELLS * bytes_per_cell / mean / 1e9, 3)}

    out = {"scalar_stats": summary(rows["scalar_stats_kernel"][warmup:warmup + frames], 8)}
    per_byte = out["scalar_stats"]["mean_ms"] / 8
    fields = {"copy": 1, "product": 2, "velocity_magnitude": 3, "kinetic_energy": 4, "radius": 0}
    for index, (label, _) in enumerate(programs):
        first = index * (warmup + frames) + warmup
        moved = 8 * (fields[label] + 1)
        out[label] = summary(rows["derive_kernel"][first:first + frames], moved)
        out[label]["per_byte_vs_scalar_stats"] = round(out[label]["mean_ms"] / moved / per_byte, 3)
    return out


def read_counters(directory: str, frames: int, warmup: int, programs) -> dict:
    """Per kernel and program, every counter's mean over the dispatches (warm-up ones included:
    a counter run is not about time) of the counter runs below `directory`."""
    files = glob.glob(os.path.join(directory, "**", "*counter_collection.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no counter collection under {directory}")
    out = collections.defaultdict(dict)
    for path in sorted(files):
        # (kernel, dispatch) -> counter -> the sum of its rows
        values = collections.defaultdict(lambda: collections.defaultdict(float))
        with open(path, newline="") as fh:
            for row in csv.DictReader(fh):
                name = row["Kernel_Name"]
                for kernel in ("scalar_stats_kernel", "derive_kernel"):
                    if f"::{kernel}" in name or f"{len(kernel)}{kernel}" in name:
                        values[kernel, int(row["Dispatch_Id"])][row["Counter_Name"]] += float(
                            row["Counter_Value"])
        groups = {"scalar_stats": [v for (k, _), v in sorted(values.items(), key=lambda e: e[0][1])
                                   if k == "scalar_stats_kernel"]}
        derive = [v for (k, _), v in sorted(values.items(), key=lambda e: e[0][1])
                  if k == "derive_kernel"]
        if len(derive) != len(programs) * (warmup + frames):
            raise SystemExit(f"{path}: {len(derive)} dispatches of derive_kernel, expected "
                             f"{len(programs) * (warmup + frames)}")
        for index, (label, _) in enumerate(programs):
            groups[label] = derive[index * (warmup + frames):(index + 1) * (warmup + frames)]
        for label, dispatches in groups.items():
            for counter in sorted({c for d in dispatches for c in d}):
                out[label][counter] = sum(d[counter] for d in dispatches) / len(dispatches)
    return out


if __name__ == "__main__":
    parser = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    parser.add_argument("--frames", type=int, default=10)
    parser.add_argument("--warmup", type=int, default=3)
    parser.add_argument("--programs", help="comma-separated labels out of PROGRAMS (default: all)")
    parser.add_argument("--trace", help="directory of a rocprofv3 --kernel-trace run of this tool")
    parser.add_argument("--counters", help="directory above the rocprofv3 --pmc runs of this tool")
    args = parser.parse_args()
    chosen = PROGRAMS
    if args.programs:
        labels = args.programs.split(",")
        unknown = [label for label in labels if label not in dict(PROGRAMS)]
        if unknown:
            parser.error(f"unknown programs {unknown}")
        chosen = [(label, dict(PROGRAMS)[label]) for label in labels]
    if args.trace:
        print(json.dumps(read_trace(args.trace, args.frames, args.warmup, chosen), indent=1))
    elif args.counters:
        print(json.dumps(read_counters(args.counters, args.frames, args.warmup, chosen), indent=1))
    else:
        print(json.dumps(run(args.frames, args.warmup, chosen)))
