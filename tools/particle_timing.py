"""Particle-field timing on a synthetic three-level scene, one rank: a 128^3 level-0 domain whose
central 64^3 cells are refined by 2, and the central half of that refined by 2 again (20 leaf boxes,
5.8 M leaf cells, f64; tools/covering_grid_timing.py's scene).  2^20 and 2^24 particles, once
uniform over the domain and once Gaussian-clustered inside the finest region (many particles per
cell: long runs), are deposited with both methods, and every step is timed on its own with events,
3 warm-up + 10 timed calls:

  cells   particle_cells_kernel (avr_scene_particle_cells), on the context's stream
  sort    the stable sort by cell and the gather of the shares (torch), on torch's stream
  clear   particle_clear_kernel alone (a deposit of no contributions)
  sum     particle_sum_kernel: a deposit of the sorted contributions, less the clear

Next to them, in the same process, a torch fill of the output's bytes (8 per leaf cell) is timed the
same way.  One JSON line is printed.  Needs a HIP device: fails loudly without one."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from covering_grid_timing import DOMAIN, leaf_boxes  # noqa: E402  (the scene is that tool's)


def run(frames: int, warmup: int, counts) -> dict:
    import numpy as np
    import torch
    from amrvolumerenderer_amd import runtime
    from amrvolumerenderer_amd.types import AmrBox, ScalarTransform
    if not torch.cuda.is_available():
        raise SystemExit("tools/particle_timing.py needs a HIP device")
    ctx = runtime.Context(0)
    described = leaf_boxes()
    boxes = []
    for level, lo, dims in described:
        size = 1.0 / (DOMAIN << level)
        cells = torch.empty((dims[2], dims[1], dims[0]), dtype=torch.float64, device=ctx.device)
        boxes.append(AmrBox(tuple(v * size for v in lo),
                            tuple((v + n) * size for v, n in zip(lo, dims)), cells, level))
    scene = ctx.create_scene(boxes, ScalarTransform())
    index = np.array([lo for _, lo, _ in described], dtype=np.int32)
    sizes = np.array([[1.0 / (DOMAIN << level)] * 3 for level in range(3)])
    leaves = sum(d[0] * d[1] * d[2] for _, _, d in described)
    result = {"scene": "three levels, 128^3 refined twice", "boxes": len(boxes),
              "leaf_cells": leaves, "frames": frames, "warmup": warmup}

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

    def deposit(cells, shares):
        n = 0 if cells is None else int(cells.numel())
        runtime._native(ctx, "avr_scene_particle_deposit", ctx._handle, scene._handle,
                        runtime._pointer(cells), runtime._pointer(shares), n, 1,
                        runtime._doubles(sizes), 3)

    generator = torch.Generator(device=ctx.device).manual_seed(7)
    target = torch.empty(leaves * 8, dtype=torch.uint8, device=ctx.device)
    fill_ms = timed(lambda: target.fill_(1), torch.cuda.current_stream())
    del target
    result["fill_ms"] = round(fill_ms, 4)
    clear_ms = timed(lambda: deposit(None, None), ctx.stream)
    result["clear_ms"] = round(clear_ms, 4)
    result["clear_vs_fill"] = round(clear_ms / fill_ms, 2)
    for n in counts:
        for spread in ("uniform", "clustered"):
            if spread == "uniform":
                points = torch.rand((n, 3), dtype=torch.float64, device=ctx.device,
                                    generator=generator)
            else:           # inside the finest region, the central quarter of the domain
                points = 0.5 + 0.02 * torch.randn((n, 3), dtype=torch.float64, device=ctx.device,
                                                  generator=generator)
            values = torch.rand(n, dtype=torch.float64, device=ctx.device, generator=generator)
            torch.cuda.synchronize()
            for method, name in enumerate(("ngp", "cic")):
                label = f"n{n}_{spread}_{name}"
                totals = torch.zeros(2, dtype=torch.int64, device=ctx.device)
                locate = lambda: scene.particle_cells(points, values, method, index, [2, 2],
                                                      sizes, (0.0, 0.0, 0.0), totals=totals)
                result[label + "_cells_ms"] = round(timed(locate, ctx.stream), 4)
                cells, shares, _, _ = locate()
                ctx.synchronize()

                def sort():
                    ordered, order = torch.sort(cells.reshape(-1), stable=True)
                    return ordered, shares.reshape(-1)[order]

                result[label + "_sort_ms"] = round(timed(sort, torch.cuda.current_stream()), 4)
                ordered, picked = sort()
                torch.cuda.synchronize()
                both_ms = timed(lambda: deposit(ordered, picked), ctx.stream)
                result[label + "_sum_ms"] = round(both_ms - clear_ms, 4)
                runs = torch.unique_consecutive(ordered, return_counts=True)[1]
                result[label + "_longest_run"] = int(runs.max().item())
                del cells, shares, ordered, picked, runs
            del points, values
    scene.close()
    return result


if __name__ == "__main__":
    parser = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    parser.add_argument("--frames", type=int, default=10)
    parser.add_argument("--warmup", type=int, default=3)
    parser.add_argument("--particles", type=int, nargs="+", default=[2 ** 20, 2 ** 24])
    args = parser.parse_args()
    print(json.dumps(run(args.frames, args.warmup, args.particles)))
