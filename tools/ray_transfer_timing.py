"""Ray transfer timing on config-4 (176 boxes of 128^3, three levels, 2.95 GB of cells per field),
one rank: avr_scene_ray_transfer in its grey, sharp and broadened forms beside the yardstick, the
weighted per-ray sums of avr_scene_ray_sums on the same rays in the same run.  The rays are the
pixels of tools/off_axis_projection_timing.py's orthographic view along (1, 0.7, 0.4) across the
whole domain, at 256 x 256 and at 512 x 512, in row-major order.  Four fields at the cell centres,
each its own allocation: the source function S = 1 + x y + z, the opacity a = 2 + x (optical depths
of a few), the bin field g = x + y + z - 1.5 in [-1.5, 1.5] and the width s = 2 channel widths.  The
channels cover [-1.5, 1.5].  Per view: the yardstick; the grey form; the sharp and the broadened
form at every --channels and every --chunks (the channels a workgroup keeps in LDS; a chunk above
the channel count is the channel count, and is measured once).  --warmup calls first, then
--frames, each call timed with events on the context's stream and waited for under its own time
limit (--limit seconds; a call that is not done by then ends the tool with status 3 and nothing more
is launched).  The event times hold what Scene.ray_transfer does around the kernel: the staging of
the plan's tables and the allocation of the outputs.  Every chunk size must give the bits of the
first: that is reported.  There is no pass or fail threshold on time.  One JSON line is printed.

Needs a HIP device: fails loudly without one."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from off_axis_projection_timing import BOX, IMAGES, LEVELS, N0, view_rays, wait  # noqa: E402

CHANNELS = (1, 16, 64)
CHUNKS = (4, 8, 16, 32)
RANGE = (-1.5, 1.5)
SOURCE = lambda x, y, z: 1.0 + x * y + z
OPACITY = lambda x, y, z: 2.0 + x + 0.0 * (y + z)
BIN = lambda x, y, z: (x + y) + (z - 1.5)


def run(frames: int, warmup: int, limit: float, images=IMAGES, channels=CHANNELS,
        chunks=CHUNKS) -> dict:
    import numpy as np
    import torch
    from amrvolumerenderer_amd import rays as ray_rules
    from amrvolumerenderer_amd import runtime, scenes
    from amrvolumerenderer_amd.types import AmrBox, ScalarTransform
    if not torch.cuda.is_available():
        raise SystemExit("tools/ray_transfer_timing.py needs a HIP device")
    ctx = runtime.Context(0)
    spec = scenes.make_amr_scene(N0, LEVELS, BOX, "smooth", "config4_amr3_512")

    def scene_of(rule):
        boxes = []
        for m in spec.boxes:
            x, y, z = scenes._cell_centres(m, spec, torch, device=ctx.device)
            cells = rule(x[None, None, :], y[None, :, None], z[:, None, None]).contiguous()
            boxes.append(AmrBox(m.min_corner, m.max_corner, cells, m.level))
        return ctx.create_scene(boxes, ScalarTransform())

    source, opacity, bin_scene = scene_of(SOURCE), scene_of(OPACITY), scene_of(BIN)
    torch.cuda.synchronize()
    index = np.array([m.lo for m in spec.boxes], dtype=np.int32)
    sizes = np.array([[1.0 / (N0 << l)] * 3 for l in range(LEVELS)])
    ratios = [2] * (LEVELS - 1)
    bounds = ray_rules.level0_bounds(index, [m.dims for m in spec.boxes],
                                     [m.level for m in spec.boxes], ratios)
    max_trips = ray_rules.default_max_trips(bounds, ratios, LEVELS)

    def timed(call, what):
        begin, done = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        begin.record(ctx.stream)
        out = call()
        done.record(ctx.stream)
        wait(done, limit, what)
        return out, begin.elapsed_time(done)

    def measure(call, what):
        print(what, file=sys.stderr, flush=True)
        samples = []
        for _ in range(warmup + frames):
            t0 = time.perf_counter()
            out, ms = timed(call, what)
            ctx.synchronize()
            samples.append((ms, (time.perf_counter() - t0) * 1e3))
        samples = samples[warmup:]
        return out, {"event_ms": round(sum(s[0] for s in samples) / len(samples), 4),
                     "wall_ms": round(sum(s[1] for s in samples) / len(samples), 4),
                     "wall_ms_min": round(min(s[1] for s in samples), 4)}

    def bits(out):
        return [None if t is None else t.cpu().numpy().tobytes() for t in out]

    result = {"config": "config-4", "boxes": len(spec.boxes), "max_trips": max_trips,
              "frames": frames, "warmup": warmup, "views": {}}
    for image in images:
        start, end = view_rays(image)
        rays_of = lambda points: torch.from_numpy(np.ascontiguousarray(points)).to(ctx.device)
        walk = (rays_of(start), rays_of(end), max_trips, index, ratios, sizes, [0.0, 0.0, 0.0])
        view = {"rays": int(start.shape[0])}
        sums, view["weighted_sums"] = measure(lambda: source.ray_sums(*walk, opacity),
                                              "the weighted sums call")
        yardstick = view["weighted_sums"]["wall_ms"]
        ctx.set_ray_transfer_chunk(0)
        grey, view["grey"] = measure(lambda: source.ray_transfer(opacity, *walk), "the grey call")
        view["grey"]["over_yardstick"] = round(view["grey"]["wall_ms"] / yardstick, 3)
        view["grey_walk_equals_the_sums"] = bool(
            bits(sums[:3]) == bits(grey[:3]) and bits([sums[6]]) == bits([grey[7]]))
        view["tau_max"] = float(grey[4].max().item())
        del sums, grey
        for nc in channels:
            edges = np.linspace(RANGE[0], RANGE[1], nc + 1)
            width = 2.0 * (RANGE[1] - RANGE[0]) / nc
            width_scene = scene_of(lambda x, y, z: width + 0.0 * ((x + y) + z))
            for form, s in (("sharp", None), ("broadened", width_scene)):
                first, same = None, True
                for chunk in sorted({min(c, nc) for c in chunks}):
                    ctx.set_ray_transfer_chunk(chunk)
                    out, times = measure(
                        lambda: source.ray_transfer(opacity, *walk, bin_scene, s, edges),
                        f"the {form} call, {nc} channels in chunks of {chunk}")
                    times["over_yardstick"] = round(times["wall_ms"] / yardstick, 3)
                    view[f"{form}_nc{nc}_chunk{chunk}"] = times
                    if first is None:
                        first = bits(out)
                    else:
                        same = same and bits(out) == first
                    del out
                view[f"{form}_nc{nc}_chunks_agree_by_bits"] = bool(same)
            width_scene.close()
        result["views"][f"{image}x{image}"] = view
    ctx.set_ray_transfer_chunk(0)
    for scene in (source, opacity, bin_scene):
        scene.close()
    ctx.close()
    return result


if __name__ == "__main__":
    parser = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    parser.add_argument("--frames", type=int, default=10)
    parser.add_argument("--warmup", type=int, default=3)
    parser.add_argument("--limit", type=float, default=60.0,
                        help="seconds one call may take before the tool gives up")
    parser.add_argument("--images", type=int, nargs="+", default=list(IMAGES),
                        help="the views' sizes in pixels a side")
    parser.add_argument("--channels", type=int, nargs="+", default=list(CHANNELS))
    parser.add_argument("--chunks", type=int, nargs="+", default=list(CHUNKS),
                        help="channels a workgroup keeps in LDS (1 .. 32)")
    args = parser.parse_args()
    print(json.dumps(run(args.frames, args.warmup, args.limit, tuple(args.images),
                         tuple(args.channels), tuple(args.chunks))))
