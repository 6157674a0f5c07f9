"""Clump-binding timing, one rank.  Two parts, one JSON line.

Pairs: synthetic segments of distinct cell centres -- one segment of 2^10, of 2^14 and of 2^18
members, and 2^16 segments of 8 to 64 members -- through Context.clump_pair_energy, --warmup +
--frames calls each, timed with events on the context's stream; pairs per second from the call
times.

Members: the "large" workload of tools/clump_timing.py on config-4 (176 boxes of 128^3, 2.95 GB
per field; the smooth field above 0.2, a few large clumps).  On its label scene these are timed in
this order: Scene.scalar_stats (the yardstick), Scene.clump_table without a field,
avr_scene_clump_members with every clump wanted, avr_scene_clump_member_data (levels and centres
and the field's value, on the sorted keys), and Scene.clump_table once more, so that the trace
shows what two runs of one kernel differ by -- the margin the members kernel is held to.

The kernels' own times come from a kernel trace of the same run, which this tool then reads back:

  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/clump_binding_timing.py
  python tools/clump_binding_timing.py --trace OUT

--trace tells the timed loops apart by the order of the dispatches and gives, per kernel, the mean
and smallest time; for the pair kernels pairs per second; for the cell scans the ratio to
scalar_stats_kernel per byte moved (8 B per cell for scalar_stats, the table and the members; per
member 8 B of key and 25 B of level and centre, or 16 B of value read and written, for the data
kernel).  Needs a
HIP device: fails loudly without one."""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CELLS = 176 * 128 ** 3
THRESHOLD = 0.2
# (label, members per segment or None for 2^16 segments of 8 to 64)
PAIR_WORKLOADS = (("one_2^10", 1 << 10), ("one_2^14", 1 << 14), ("one_2^18", 1 << 18),
                  ("2^16_of_8_to_64", None))


def pair_offsets(members):
    import numpy as np
    if members is not None:
        return np.array([0, members], dtype=np.int64)
    counts = np.random.default_rng(7).integers(8, 65, 1 << 16)
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


def pair_count(offsets) -> int:
    return int(sum(int(n) * (int(n) - 1) // 2 for n in (offsets[1:] - offsets[:-1])))


def run(frames: int, warmup: int) -> dict:
    import numpy as np
    import torch
    from amrvolumerenderer_amd import _capi, runtime, scenes
    from amrvolumerenderer_amd.types import AmrBox, ScalarTransform
    if not torch.cuda.is_available():
        raise SystemExit("tools/clump_binding_timing.py needs a HIP device")
    ctx = runtime.Context(0)
    result = {"frames": frames, "warmup": warmup, "pairs": {}, "members": {}}

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

    # ---- pairs: distinct centres of a lattice of 256^3 cells, masses in [0.5, 1.5)
    rng = np.random.default_rng(11)
    lattice = rng.permutation(1 << 24)
    for label, members in PAIR_WORKLOADS:
        offsets = pair_offsets(members)
        sites = lattice[:int(offsets[-1])]
        x, y, z = (torch.from_numpy(((sites >> (8 * a) & 255) + 0.5) / 256.0).to(ctx.device)
                   for a in range(3))
        m = torch.from_numpy(rng.random(sites.size) + 0.5).to(ctx.device)
        w = torch.empty(offsets.size - 1, dtype=torch.float64, device=ctx.device)
        call_ms = timed(lambda: ctx.clump_pair_energy(offsets, x, y, z, m, w))
        pairs = pair_count(offsets)
        result["pairs"][label] = {"segments": int(offsets.size - 1), "members": int(offsets[-1]),
                                  "pairs": pairs, "call_ms": call_ms,
                                  "pairs_per_second": round(pairs / (call_ms * 1e-3), 1)}
        del x, y, z, m, w
    torch.cuda.empty_cache()

    # ---- members: the label scene of config-4's smooth field above 0.2
    spec = scenes.config4("smooth")
    first = [scenes.box_cells_torch(spec, i, ctx.device) for i in range(len(spec.boxes))]
    torch.cuda.synchronize()

    def boxes_of(tensors):
        return [AmrBox(m.min_corner, m.max_corner, c, m.level) for c, m in zip(tensors, spec.boxes)]

    n_levels = 1 + max(int(m.level) for m in spec.boxes)
    index = np.array([m.lo for m in spec.boxes], dtype=np.int32)
    ratios = np.array([2] * (n_levels - 1), dtype=np.int32)
    sizes = np.array([(spec.extent / (spec.n0 << l),) * 3 for l in range(n_levels)])
    origin = np.zeros(3)
    field = ctx.create_scene(boxes_of(first), ScalarTransform())
    labels = ctx.create_scene(boxes_of([torch.empty_like(c) for c in first]), ScalarTransform())
    n = int(labels.clumps(field, THRESHOLD, float("inf"), index, ratios).item())
    entry = {"config": "config-4", "cells": CELLS, "field": "smooth", "threshold": THRESHOLD,
             "n_clumps": n}
    if 0 < n and n * n_levels < (1 << 28):
        cells = torch.zeros((n_levels, n), dtype=torch.int64, device=ctx.device)
        totals = torch.zeros(2, dtype=torch.int64, device=ctx.device)
        labels.clump_table(n, n_levels, None, cells, None, totals)
        ctx.synchronize()
        members = int(cells.sum().item())
        entry["members"] = members
        cells.zero_()
        wanted = torch.ones(n, dtype=torch.uint8, device=ctx.device)
        keys = torch.empty(members, dtype=torch.int64, device=ctx.device)
        count = torch.zeros(1, dtype=torch.int64, device=ctx.device)
        outside = torch.zeros(1, dtype=torch.int64, device=ctx.device)
        lib = _capi.lib()
        pointer = lambda t: C.c_void_p(t.data_ptr())
        doubles = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        ints = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))

        def list_members():
            ctx.join()
            _capi.check(lib.avr_scene_clump_members(
                ctx._handle, labels._handle, n, pointer(wanted), members, pointer(keys),
                pointer(count), pointer(outside)))
            ctx.publish()

        entry["scalar_stats_call_ms"] = timed(labels.scalar_stats)
        entry["table_call_ms"] = timed(lambda: labels.clump_table(n, n_levels, None, cells, None,
                                                                   totals))
        entry["members_call_ms"] = timed(list_members)
        ctx.synchronize()
        entry["members_counted"] = int(count.item())
        keys = torch.sort(keys).values
        levels = torch.empty(members, dtype=torch.uint8, device=ctx.device)
        centres = torch.empty((3, members), dtype=torch.float64, device=ctx.device)
        values = torch.empty(members, dtype=torch.float64, device=ctx.device)

        def look_up(with_centres, with_values):
            ctx.join()
            _capi.check(lib.avr_scene_clump_member_data(
                ctx._handle, labels._handle, pointer(keys), members,
                field._handle if with_values else None, pointer(values) if with_values else None,
                ints(index), ints(ratios), doubles(sizes), doubles(origin), n_levels,
                pointer(centres) if with_centres else None,
                pointer(levels) if with_centres else None))
            ctx.publish()

        entry["data_centres_call_ms"] = timed(lambda: look_up(True, False))
        entry["data_values_call_ms"] = timed(lambda: look_up(False, True))
        entry["table_again_call_ms"] = timed(lambda: labels.clump_table(n, n_levels, None, cells,
                                                                         None, totals))
        ctx.synchronize()
    result["members"] = entry
    for scene in (field, labels):
        scene.close()
    return result


def read_trace(directory: str, frames: int, warmup: int) -> dict:
    """Per timed loop every kernel's mean, smallest and largest time over the timed dispatches."""
    files = glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True)
    if len(files) != 1:
        raise SystemExit(f"expected one kernel trace under {directory}, found {len(files)}")
    names = ("clump_pair_kernel", "clump_pair_reduce_kernel", "scalar_stats_kernel",
             "clump_table_kernel<false>", "clump_members_kernel", "clump_member_data_kernel")
    rows = {name: [] for name in names}
    with open(files[0], newline="") as fh:
        for row in csv.DictReader(fh):
            for name in names:
                if name in row["Kernel_Name"]:
                    rows[name].append((int(row["Start_Timestamp"]), int(row["End_Timestamp"])))

    def loop(name, number, lone=0):
        """The timed dispatches of the kernel's loop `number`, `lone` dispatches before the loops."""
        first = lone + number * (warmup + frames) + warmup
        times = [(end - start) * 1e-6 for start, end in sorted(rows[name])[first:first + frames]]
        if len(times) != frames:
            return None
        return {"mean_ms": round(sum(times) / frames, 4), "min_ms": round(min(times), 4),
                "max_ms": round(max(times), 4)}

    out = {"pairs": {}, "members": {}}
    for number, (label, members) in enumerate(PAIR_WORKLOADS):
        pairs = pair_count(pair_offsets(members))
        entry = {"pairs": pairs}
        for name in names[:2]:
            figures = loop(name, number)
            if figures is not None:
                entry[name] = figures
        if "clump_pair_kernel" in entry:
            entry["pairs_per_second"] = round(pairs / (entry["clump_pair_kernel"]["mean_ms"] * 1e-3), 1)
        out["pairs"][label] = entry
    # the table's first dispatch is the lone call that counted the members
    scans = {"scalar_stats_kernel": loop("scalar_stats_kernel", 0),
             "clump_table_kernel<false>": loop("clump_table_kernel<false>", 0, 1),
             "clump_table_kernel<false> again": loop("clump_table_kernel<false>", 1, 1),
             "clump_members_kernel": loop("clump_members_kernel", 0),
             "clump_member_data_kernel centres": loop("clump_member_data_kernel", 0),
             "clump_member_data_kernel values": loop("clump_member_data_kernel", 1)}
    out["members"] = {name: figures for name, figures in scans.items() if figures is not None}
    if "scalar_stats_kernel" in out["members"]:
        per_byte = out["members"]["scalar_stats_kernel"]["mean_ms"] / (8 * CELLS)
        for name, figures in out["members"].items():
            if "data" not in name:
                figures["per_byte_vs_scalar_stats"] = round(
                    figures["mean_ms"] / (8 * CELLS) / per_byte, 3)
        out["members"]["scalar_stats_ms_per_gigabyte"] = round(per_byte * 1e9, 4)
    return out


if __name__ == "__main__":
    parser = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    parser.add_argument("--frames", type=int, default=10)
    parser.add_argument("--warmup", type=int, default=3)
    parser.add_argument("--trace", help="directory of a rocprofv3 --kernel-trace run of this tool")
    parser.add_argument("--members", type=int, default=None,
                        help="with --trace: the members the run reported, for the data kernel's "
                             "rate per byte")
    args = parser.parse_args()
    if args.trace:
        found = read_trace(args.trace, args.frames, args.warmup)
        if args.members and "scalar_stats_ms_per_gigabyte" in found["members"]:
            per_byte = found["members"]["scalar_stats_ms_per_gigabyte"] * 1e-9
            for name, moved in (("clump_member_data_kernel centres", 33),
                                ("clump_member_data_kernel values", 24)):
                if name in found["members"]:
                    figures = found["members"][name]
                    figures["per_byte_vs_scalar_stats"] = round(
                        figures["mean_ms"] / (moved * args.members) / per_byte, 3)
        print(json.dumps(found, indent=1))
    else:
        print(json.dumps(run(args.frames, args.warmup)))
