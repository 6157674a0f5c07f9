"""Grid-field timing on a synthetic three-level scene, one rank: a 128^3 level-0 domain whose
central 64^3 cells are refined by 2, and the central half of that refined by 2 again (20 leaf boxes,
5.8 M leaf cells, f64; tools/covering_grid_timing.py's scene).  Scene.grid_field writes a grid of
the whole domain onto every leaf and is timed with events on the context's stream, 3 warm-up + 10
timed calls, for source grids at two levels, each with constant and with linear interpolation:

  L = 0   128^3 grid cells: the level-0 leaves copy, the finer ones repeat (constant) or
          interpolate eight values (linear)
  L = 2   512^3 grid cells: the finest leaves copy, the coarser ones average 8 or 64 grid cells
          (both modes are the same there)

Next to each, in the same process, a torch fill of the same number of output bytes (8 per leaf
cell) is timed the same way: the floor that any kernel writing that much can reach.  One JSON line
is printed.  Needs a HIP device: fails loudly without one."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from covering_grid_timing import DOMAIN, leaf_boxes  # noqa: E402  (the scene is that tool's)


def run(frames: int, warmup: int) -> dict:
    import numpy as np
    import torch
    from amrvolumerenderer_amd import runtime
    from amrvolumerenderer_amd.types import AmrBox, ScalarTransform
    if not torch.cuda.is_available():
        raise SystemExit("tools/grid_field_timing.py needs a HIP device")
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

    generator = torch.Generator(device=ctx.device).manual_seed(7)
    totals = torch.zeros(2, dtype=torch.int64, device=ctx.device)
    target = torch.empty(leaves * 8, dtype=torch.uint8, device=ctx.device)
    fill_ms = timed(lambda: target.fill_(1), torch.cuda.current_stream())
    del target
    result["fill_ms"] = round(fill_ms, 4)
    result["fill_TBps"] = round(leaves * 8 / fill_ms / 1e9, 3)
    for level in (0, 2):
        n = DOMAIN << level
        grid = torch.randn((n, n, n), dtype=torch.float64, device=ctx.device, generator=generator)
        torch.cuda.synchronize()
        for mode, name in enumerate(("constant", "linear")):
            ms = timed(lambda: scene.grid_field(grid, level, (0, 0, 0), index, [2, 2], mode, True,
                                                totals=totals), ctx.stream)
            label = f"L{level}_{name}"
            result[label + "_call_ms"] = round(ms, 4)
            result[label + "_output_TBps"] = round(leaves * 8 / ms / 1e9, 3)
            result[label + "_call_vs_fill"] = round(ms / fill_ms, 2)
        del grid
    scene.close()
    return result


if __name__ == "__main__":
    parser = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    parser.add_argument("--frames", type=int, default=10)
    parser.add_argument("--warmup", type=int, default=3)
    args = parser.parse_args()
    print(json.dumps(run(args.frames, args.warmup)))
