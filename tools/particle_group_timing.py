"""Particle-group timing, one rank: 2^20 and 2^24 particles in the unit box, once uniform and once
clustered (half of them in n / 4096 Gaussian blobs of 2048 particles with sigma = 4 linking lengths
around uniform centres, the rest uniform), with a linking length of 0.2 mean separations, on the
grid api.particle_groups chooses, min_members 20.  Every step is timed on its own with events, 3
warm-up + 10 timed calls, one run:

  cells    group_cells_kernel (avr_particle_group_cells), on the context's stream
  sort     the stable sort by cell, the cell ranges (searchsorted) and the gather of the points
           (torch), on torch's stream
  groups   avr_particle_groups from a fresh forest: the sizes' clear, link, flatten, count, scan,
           rank, label -- and the copy that refreshes the forest, which is timed alone (copy) too
  labels   avr_particle_groups with n_inside = 0 on the flattened forest: everything but the link
  link     groups - labels - copy: group_link_kernel (a difference of measured times)

With them pair_tests (counted from the cell occupancies), pair tests per second of link time, the
number of groups and the largest group.  With --scipy and scipy importable, the host time of
cKDTree.query_pairs plus connected_components at 2^20 uniform is added, for scale only.  One JSON
line is printed.  Needs a HIP device: fails loudly without one."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def run(frames: int, warmup: int, counts, with_scipy: bool) -> dict:
    import numpy as np
    import torch
    from amrvolumerenderer_amd import groups, runtime
    if not torch.cuda.is_available():
        raise SystemExit("tools/particle_group_timing.py needs a HIP device")
    ctx = runtime.Context(0)
    device = ctx.device
    lo, hi, flags = np.zeros(3), np.ones(3), (False, False, False)
    result = {"frames": frames, "warmup": warmup, "min_members": 20}

    def timed(call, stream):
        for _ in range(warmup):
            call()
        torch.cuda.synchronize()
        begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        begin.record(stream)
        for _ in range(frames):
            call()
        end.record(stream)
        end.synchronize()
        return begin.elapsed_time(end) / frames

    generator = torch.Generator(device=device).manual_seed(11)
    for n in counts:
        b = groups.linking_length(n, 1.0)
        dims = groups.choose_dims(n, b, lo, hi, flags)
        box = runtime._group_box(lo, hi, dims, flags)
        n_cells = dims[0] * dims[1] * dims[2]
        for spread in ("uniform", "clustered"):
            points = torch.rand((n, 3), dtype=torch.float64, device=device, generator=generator)
            if spread == "clustered":
                blobs = max(1, n // 4096)
                centres = torch.rand((blobs, 3), dtype=torch.float64, device=device,
                                     generator=generator)
                members = blobs * 2048
                points[:members] = centres.repeat_interleave(2048, dim=0) + 4.0 * b * torch.randn(
                    (members, 3), dtype=torch.float64, device=device, generator=generator)
            torch.cuda.synchronize()
            label = f"n{n}_{spread}"
            result[label + "_b"] = b
            result[label + "_dims"] = list(dims)
            totals = torch.zeros(1, dtype=torch.int64, device=device)
            locate = lambda: ctx.particle_group_cells(points, lo, hi, dims, flags, totals=totals)
            result[label + "_cells_ms"] = round(timed(locate, ctx.stream), 4)
            _, cells, fresh, _ = locate()
            ctx.synchronize()
            edges = torch.arange(n_cells + 1, dtype=torch.int64, device=device)

            def sort():
                keys, order = torch.sort(cells.to(torch.int64) & 0xFFFFFFFF, stable=True)
                return order, torch.searchsorted(keys, edges).contiguous(), \
                    points[order].contiguous()

            result[label + "_sort_ms"] = round(timed(sort, torch.cuda.current_stream()), 4)
            order, cell_begin, ordered = sort()
            counts_grid = (cell_begin[1:] - cell_begin[:-1]).reshape(dims[2], dims[1], dims[0])
            pair_tests = runtime.group_pair_tests(counts_grid, flags)
            n_inside = int(cell_begin[-1].item())
            parent = fresh.clone()
            labels = torch.empty(n, dtype=torch.int32, device=device)
            sizes = torch.empty(n, dtype=torch.int32, device=device)
            n_groups = torch.zeros(1, dtype=torch.int64, device=device)

            def native(inside):
                runtime._native(ctx, "avr_particle_groups", ctx._handle, runtime._pointer(ordered),
                                runtime._pointer(order), runtime._pointer(cell_begin), n, inside, b,
                                runtime._doubles(box[0]), runtime._doubles(box[1]),
                                runtime._ints(box[2]), runtime._ints(box[3]), 20,
                                runtime._pointer(parent), runtime._pointer(labels),
                                runtime._pointer(sizes), runtime._pointer(n_groups))

            def whole():
                parent.copy_(fresh)
                native(n_inside)

            copy_ms = timed(lambda: parent.copy_(fresh), torch.cuda.current_stream())
            groups_ms = timed(whole, ctx.stream)
            found, largest = int(n_groups.item()), int(sizes.max().item())
            labels_ms = timed(lambda: native(0), ctx.stream)     # the forest is flattened by now
            assert int(n_groups.item()) == found
            link_ms = groups_ms - labels_ms - copy_ms
            result[label + "_copy_ms"] = round(copy_ms, 4)
            result[label + "_groups_ms"] = round(groups_ms, 4)
            result[label + "_labels_ms"] = round(labels_ms, 4)
            result[label + "_link_ms"] = round(link_ms, 4)
            result[label + "_pair_tests"] = pair_tests
            result[label + "_pair_tests_per_s"] = float(f"{pair_tests / (link_ms * 1e-3):.4g}")
            result[label + "_groups"] = found
            result[label + "_largest"] = largest
            if with_scipy and n == 2 ** 20 and spread == "uniform":
                try:
                    from scipy.sparse import coo_matrix
                    from scipy.sparse.csgraph import connected_components
                    from scipy.spatial import cKDTree
                except ImportError:
                    pass
                else:
                    host = points.cpu().numpy()
                    begin = time.perf_counter()
                    pairs = cKDTree(host).query_pairs(b, output_type="ndarray")
                    graph = coo_matrix((np.ones(len(pairs), dtype=np.int8),
                                        (pairs[:, 0], pairs[:, 1])), shape=(n, n))
                    connected_components(graph, directed=False)
                    result[label + "_scipy_host_s"] = round(time.perf_counter() - begin, 3)
            del points, cells, fresh, parent, labels, sizes, order, cell_begin, ordered
    return result


if __name__ == "__main__":
    parser = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    parser.add_argument("--frames", type=int, default=10)
    parser.add_argument("--warmup", type=int, default=3)
    parser.add_argument("--particles", type=int, nargs="+", default=[2 ** 20, 2 ** 24])
    parser.add_argument("--scipy", action="store_true")
    args = parser.parse_args()
    print(json.dumps(run(args.frames, args.warmup, args.particles, args.scipy)))
