"""Covering-grid timing on a synthetic three-level scene, one rank: a 128^3 level-0 domain whose
central 64^3 cells are refined by 2, and the central half of that refined by 2 again (20 leaf boxes,
5.8 M leaf cells, f64).  Scene.covering_grid over the whole domain is timed with events on the
context's stream at two levels:

  L = 2 (the finest)   512^3 output cells, every one a copy of a leaf of the same or a coarser
                       level: the kernel is bound by its stores, 17 bytes per cell
  L = 0                128^3 output cells, one in eight the mean of 8 to 64 finer leaves: the
                       kernel is bound by its gathers

Next to each, in the same process, a torch fill of the same number of output bytes (17 per cell:
value, coverage, cell level) is timed the same way: the floor that any kernel writing that much can
reach.  One JSON line is printed.  Needs a HIP device: fails loudly without one."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DOMAIN = 128          # level-0 cells along an axis


def shell(lo, n):
    """The cells [lo, lo + n)^3 without their central (n / 2)^3, as six boxes (lo, dims)."""
    q, h = n // 4, n // 2
    boxes = [((lo, lo, lo), (q, n, n)), ((lo + q + h, lo, lo), (q, n, n)),
             ((lo + q, lo, lo), (h, q, n)), ((lo + q, lo + q + h, lo), (h, q, n)),
             ((lo + q, lo + q, lo), (h, h, q)), ((lo + q, lo + q, lo + q + h), (h, h, q))]
    return boxes


def leaf_boxes():
    """(level, lo, dims) of the leaf boxes: two shells and the finest cube as eight boxes."""
    out = [(0, lo, dims) for lo, dims in shell(0, DOMAIN)]
    first = DOMAIN // 4 * 2                      # the refined region at level 1
    out += [(1, lo, dims) for lo, dims in shell(first, DOMAIN)]
    finest, half = (first + DOMAIN // 4) * 2, DOMAIN // 2
    out += [(2, (finest + a * half, finest + b * half, finest + c * half), (half,) * 3)
            for c in range(2) for b in range(2) for a in range(2)]
    return out


def run(frames: int, warmup: int) -> dict:
    import numpy as np
    import torch
    from amrvolumerenderer_amd import runtime
    from amrvolumerenderer_amd.types import AmrBox, ScalarTransform
    if not torch.cuda.is_available():
        raise SystemExit("tools/covering_grid_timing.py needs a HIP device")
    ctx = runtime.Context(0)
    described = leaf_boxes()
    generator = torch.Generator(device=ctx.device).manual_seed(7)
    boxes = []
    for level, lo, dims in described:
        size = 1.0 / (DOMAIN << level)
        cells = torch.randn((dims[2], dims[1], dims[0]), dtype=torch.float64, device=ctx.device,
                            generator=generator)
        boxes.append(AmrBox(tuple(v * size for v in lo),
                            tuple((v + n) * size for v, n in zip(lo, dims)), cells, level))
    torch.cuda.synchronize()
    scene = ctx.create_scene(boxes, ScalarTransform())
    index = np.array([lo for _, lo, _ in described], dtype=np.int32)
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

    for level in (2, 0):
        n = DOMAIN << level
        cells = n ** 3
        ms = timed(lambda: scene.covering_grid(level, (0, 0, 0), (n, n, n), index, [2, 2]),
                   ctx.stream)
        target = torch.empty(cells * 17, dtype=torch.uint8, device=ctx.device)
        fill_ms = timed(lambda: target.fill_(1), torch.cuda.current_stream())
        del target
        label = f"L{level}"
        result[label + "_cells"] = cells
        result[label + "_call_ms"] = round(ms, 4)
        result[label + "_output_TBps"] = round(cells * 17 / ms / 1e9, 3)
        result[label + "_fill_ms"] = round(fill_ms, 4)
        result[label + "_fill_TBps"] = round(cells * 17 / fill_ms / 1e9, 3)
        result[label + "_call_vs_fill"] = round(ms / fill_ms, 2)
    scene.close()
    return result


if __name__ == "__main__":
    parser = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    parser.add_argument("--frames", type=int, default=10)
    parser.add_argument("--warmup", type=int, default=3)
    args = parser.parse_args()
    print(json.dumps(run(args.frames, args.warmup)))
