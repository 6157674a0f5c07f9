"""Column-projection timing on config-4 at 2048^2 (BASELINE.json's headline scene): projection
frames pipelined and one synchronised frame, next to MIP and volume frames pipelined, one rank.
Prints one JSON line.  The projection march alone (render_runs_sum_kernel, against
render_runs_max_kernel) comes from a kernel trace of this script, its memory traffic from a
counter-only run ("Column projection"):
  rocprofv3 --kernel-trace --stats -d OUT -- python tools/projection_timing.py
  rocprofv3 --pmc FETCH_SIZE -d OUT -- python tools/projection_timing.py --frames 3 --warmup 1
Needs a HIP device: fails loudly without one."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from amrvolumerenderer_amd import runtime, scenes  # noqa: E402
from amrvolumerenderer_amd.renderer import FrameRenderer, RenderParameters  # noqa: E402
from amrvolumerenderer_amd.types import AmrBox  # noqa: E402

W = H = 2048
TRANSPARENCY = 0.97   # the volume frame bench.py times


def main(frames: int = 50, warmup: int = 10) -> int:
    if not torch.cuda.is_available():
        raise SystemExit("tools/projection_timing.py needs a HIP device")
    ctx = runtime.Context(0)
    spec = scenes.config4("smooth")
    cells = [scenes.box_cells_torch(spec, i, ctx.device) for i in range(len(spec.boxes))]
    torch.cuda.synchronize()
    meta = [scenes.metadata_box(spec, i) for i in range(len(cells))]
    local = [AmrBox(m.min_corner, m.max_corner, c, m.level) for c, m in zip(cells, spec.boxes)]
    renderer = FrameRenderer(ctx, meta, local, spec.transform, spec.bounds, spec.scalar_range)
    native = renderer.native
    if native is None:
        raise SystemExit("the native frame driver is not available")
    cam = scenes.default_camera()
    flat = RenderParameters(W, H, 0.0, 1, draw_bounds=False)
    vol = RenderParameters(W, H, TRANSPARENCY, 1, draw_bounds=False)
    result = {"config": "config-4", "width": W, "height": H, "frames": frames,
              "cell_bytes": int(sum(c.numel() for c in cells) * 8)}

    counter = torch.zeros(1, dtype=torch.int64, device=ctx.device)
    renderer.render_projection(flat, cam, samples=counter)
    renderer.synchronize()
    result["projection_samples"] = int(counter.item())

    def pipelined(render):
        for _ in range(warmup):
            render()
        renderer.synchronize()
        t0 = time.perf_counter()
        for _ in range(frames):
            render()
        renderer.synchronize()
        return (time.perf_counter() - t0) * 1e3 / frames

    result["projection_pipelined_ms"] = round(
        pipelined(lambda: renderer.render_projection(flat, cam)), 4)
    result["mip_pipelined_ms"] = round(pipelined(lambda: renderer.render_max_intensity(flat, cam)), 4)
    result["volume_pipelined_ms"] = round(pipelined(lambda: renderer.render(vol, cam)), 4)
    synced = []
    for _ in range(5):
        renderer.synchronize()
        t0 = time.perf_counter()
        renderer.render_projection(flat, cam)
        renderer.synchronize()
        synced.append((time.perf_counter() - t0) * 1e3)
    result["projection_synchronised_ms"] = round(min(synced), 4)
    print(json.dumps(result))
    native.close()
    return 0


if __name__ == "__main__":
    parser = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    parser.add_argument("--frames", type=int, default=50)
    parser.add_argument("--warmup", type=int, default=10)
    args = parser.parse_args()
    raise SystemExit(main(args.frames, args.warmup))
