"""Maximum-intensity projection timing on config-4 at 2048^2 (BASELINE.json's headline scene):
MIP frames pipelined and one synchronised frame, and the MIP march alone next to the volume march
alone (avr_renderer_set_timing / avr_renderer_timings), one rank.  Prints one JSON line.
Needs a HIP device: fails loudly without one."""
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
        raise SystemExit("tools/mip_timing.py needs a HIP device")
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
    mip = RenderParameters(W, H, 0.0, 1, draw_bounds=False)
    vol = RenderParameters(W, H, TRANSPARENCY, 1, draw_bounds=False)
    result = {"config": "config-4", "width": W, "height": H, "frames": frames}

    counter = torch.zeros(1, dtype=torch.int64, device=ctx.device)
    renderer.render_max_intensity(mip, cam, samples=counter)
    renderer.synchronize()
    result["mip_samples"] = int(counter.item())

    def pipelined(render):
        for _ in range(warmup):
            render()
        renderer.synchronize()
        t0 = time.perf_counter()
        for _ in range(frames):
            render()
        renderer.synchronize()
        return (time.perf_counter() - t0) * 1e3 / frames

    result["mip_pipelined_ms"] = round(pipelined(lambda: renderer.render_max_intensity(mip, cam)), 4)
    result["volume_pipelined_ms"] = round(pipelined(lambda: renderer.render(vol, cam)), 4)
    synced = []
    for _ in range(5):
        renderer.synchronize()
        t0 = time.perf_counter()
        renderer.render_max_intensity(mip, cam)
        renderer.synchronize()
        synced.append((time.perf_counter() - t0) * 1e3)
    result["mip_synchronised_ms"] = round(min(synced), 4)

    # the kernels alone, back to back on one stream (no co-run beside the next classify pass)
    native.set_overlap(0)
    for name, render in (("mip", lambda: renderer.render_max_intensity(mip, cam)),
                         ("volume", lambda: renderer.render(vol, cam))):
        for _ in range(warmup):
            render()
        renderer.synchronize()
        native.set_timing(True)
        for _ in range(frames):
            render()
        classify_ms, march_ms, _, n = native.timings()
        native.set_timing(False)
        result[f"{name}_march_alone_ms"] = round(march_ms, 4)
        result[f"{name}_classify_alone_ms"] = round(classify_ms, 4)
    print(json.dumps(result))
    native.close()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
