"""Slice timing on config-4 at 2048^2 (BASELINE.json's headline scene), one rank: an axis-aligned
and an oblique slice through the middle of the scene (Scene.slice: point location + one gather per
pixel), timed with events on the context's stream after a warm-up, next to the pipelined MIP frame
of the same scene and size.  Every step runs in a child process of its own under a time limit and
the first failure ends the run; prints one JSON line.  The kernel's own time comes from a kernel
trace of one step ("Slice"):
  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/slice_timing.py --step axis
Needs a HIP device: fails loudly without one."""
import argparse
import json
import os
import subprocess
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from amrvolumerenderer_amd import api, runtime, scenes  # noqa: E402
from amrvolumerenderer_amd.renderer import FrameRenderer, RenderParameters  # noqa: E402
from amrvolumerenderer_amd.types import AmrBox  # noqa: E402

W = H = 2048
STEPS = ("axis", "oblique", "mip")
PLANES = {"axis": ((0.0, 0.0, 1.0), (0.0, 1.0, 0.0)),
          "oblique": ((0.3, -0.4, 1.0), (0.0, 1.0, 0.0))}


def load(ctx):
    spec = scenes.config4("smooth")
    cells = [scenes.box_cells_torch(spec, i, ctx.device) for i in range(len(spec.boxes))]
    torch.cuda.synchronize()
    local = [AmrBox(m.min_corner, m.max_corner, c, m.level) for c, m in zip(cells, spec.boxes)]
    return spec, cells, local


def slice_step(name: str, frames: int, warmup: int) -> dict:
    ctx = runtime.Context(0)
    spec, cells, local = load(ctx)
    lo = [min(b.min_corner[a] for b in local) for a in range(3)]
    hi = [max(b.max_corner[a] for b in local) for a in range(3)]
    _, u, v = api.slice_basis(*PLANES[name])
    # a little off the middle, so that the plane does not run along the faces of a cell layer
    center = [0.5 * (lo[a] + hi[a]) + 0.0137 * (hi[a] - lo[a]) for a in range(3)]
    wu, wv = (sum(abs(e[a]) * (hi[a] - lo[a]) for a in range(3)) for e in (u, v))
    origin = [center[a] - 0.5 * wu * u[a] - 0.5 * wv * v[a] for a in range(3)]
    du = [u[a] * wu / W for a in range(3)]
    dv = [v[a] * wv / H for a in range(3)]
    scene = ctx.create_scene(local, spec.transform)
    outs = scene.slice(origin, du, dv, W, H)
    for _ in range(warmup):
        scene.slice(origin, du, dv, W, H, None, *outs)
    ctx.synchronize()
    begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    begin.record(ctx.stream)
    for _ in range(frames):
        scene.slice(origin, du, dv, W, H, None, *outs)
    end.record(ctx.stream)
    end.synchronize()
    level = outs[1]
    return {f"{name}_slice_ms": round(begin.elapsed_time(end) / frames, 4),
            f"{name}_hit_fraction": round(float((level >= 0).float().mean().item()), 4),
            "boxes": len(local)}


def mip_step(frames: int, warmup: int) -> dict:
    ctx = runtime.Context(0)
    spec, cells, local = load(ctx)
    meta = [scenes.metadata_box(spec, i) for i in range(len(cells))]
    renderer = FrameRenderer(ctx, meta, local, spec.transform, spec.bounds, spec.scalar_range)
    if renderer.native is None:
        raise SystemExit("the native frame driver is not available")
    cam = scenes.default_camera()
    flat = RenderParameters(W, H, 0.0, 1, draw_bounds=False)
    for _ in range(warmup):
        renderer.render_max_intensity(flat, cam)
    renderer.synchronize()
    t0 = time.perf_counter()
    for _ in range(frames):
        renderer.render_max_intensity(flat, cam)
    renderer.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / frames
    renderer.native.close()
    return {"mip_pipelined_ms": round(ms, 4)}


def main(step: str, frames: int, warmup: int, limit: int) -> int:
    if not torch.cuda.is_available():
        raise SystemExit("tools/slice_timing.py needs a HIP device")
    if step != "all":
        result = mip_step(frames, warmup) if step == "mip" else slice_step(step, frames, warmup)
        print(json.dumps(result))
        return 0
    result = {"config": "config-4", "width": W, "height": H, "frames": frames}
    for name in STEPS:
        child = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name,
                                "--frames", str(frames), "--warmup", str(warmup)],
                               capture_output=True, text=True, timeout=limit)
        if child.returncode != 0:
            sys.stderr.write(child.stdout + child.stderr)
            print(json.dumps({**result, "failed_step": name, "status": child.returncode}))
            return 1    # nothing more is started on the device
        result.update(json.loads(child.stdout.strip().splitlines()[-1]))
    print(json.dumps(result))
    return 0


if __name__ == "__main__":
    parser = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    parser.add_argument("--step", choices=STEPS + ("all",), default="all")
    parser.add_argument("--frames", type=int, default=50)
    parser.add_argument("--warmup", type=int, default=10)
    parser.add_argument("--limit", type=int, default=240, help="seconds per step")
    args = parser.parse_args()
    raise SystemExit(main(args.step, args.frames, args.warmup, args.limit))
