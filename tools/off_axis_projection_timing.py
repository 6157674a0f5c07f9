"""Off-axis projection timing on config-4 (176 boxes of 128^3, three levels, 2.95 GB of cells per
field), one rank: the per-ray sums of avr_scene_ray_sums beside the count + emit pair of
avr_scene_rays on the same rays.  The rays are the pixels of tools/ray_timing.py's orthographic view
along (1, 0.7, 0.4) across the whole domain, at 256 x 256 and at 512 x 512, through f = 1 + x y + z
at the cell centres; the weight is w = 2 + x, a second allocation.  Per view: the sums call with
the rays in tile order (rays.pixel_order) and in row-major order, the weighted sums call in tile
order, and the call pair (count pass, torch.cumsum and the read of the total, emit pass) in both
orders.  --warmup calls first, then --frames, each call timed with events on the context's stream
and waited for under its own time limit (--limit seconds; a call that is not done by then ends the
tool with status 3 and nothing more is launched).  The event times hold what Scene.ray_sums and
Scene.rays do around the kernel: the staging of the plan's tables and the allocation of the
outputs.  The sums must be the pair's by bits (count, status, span, integral, covered), and the
tile order's those of the row-major order un-permuted: both are reported.  One JSON line is
printed.

Needs a HIP device: fails loudly without one."""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N0, LEVELS, BOX = 512, 3, 128
IMAGES = (256, 512)
VIEW = (1.0, 0.7, 0.4)
FIELD = lambda x, y, z: 1.0 + x * y + z
WEIGHT = lambda x, y, z: 2.0 + x + 0.0 * (y + z)


def view_rays(image: int):
    """(start, end) [image^2, 3], row-major: parallel segments of length 2 along VIEW through the
    pixel centres of a square of side sqrt(3), the domain's diagonal, around its centre -- the
    rays of tools/ray_timing.py."""
    import numpy as np
    w = np.array(VIEW) / math.sqrt(sum(v * v for v in VIEW))
    u = np.cross(w, [0.0, 0.0, 1.0])
    u /= np.sqrt((u * u).sum())
    v = np.cross(u, w)
    side = math.sqrt(3.0)
    f = ((np.arange(image) + 0.5) / image - 0.5) * side
    py, px = np.meshgrid(f, f, indexing="ij")
    centre = 0.5 + px.reshape(-1, 1) * u[None, :] + py.reshape(-1, 1) * v[None, :]
    return np.ascontiguousarray(centre - w[None, :]), np.ascontiguousarray(centre + w[None, :])


def wait(event, limit: float, what: str) -> None:
    """Returns when the event is done.  When it is not after `limit` seconds the tool reports it and
    ends with status 3 without launching anything more; it does not close the scenes or the
    context, which would wait for the very call that is not coming back."""
    deadline = time.monotonic() + limit
    while not event.query():
        if time.monotonic() > deadline:
            print(json.dumps({"error": f"{what} was not done after {limit} s"}))
            sys.stdout.flush()
            os._exit(3)
        time.sleep(0.0005)


def run(frames: int, warmup: int, limit: float, images=IMAGES) -> dict:
    import numpy as np
    import torch
    from amrvolumerenderer_amd import rays as ray_rules
    from amrvolumerenderer_amd import runtime, scenes
    from amrvolumerenderer_amd.types import AmrBox, ScalarTransform
    if not torch.cuda.is_available():
        raise SystemExit("tools/off_axis_projection_timing.py needs a HIP device")
    ctx = runtime.Context(0)
    spec = scenes.make_amr_scene(N0, LEVELS, BOX, "smooth", "config4_amr3_512")

    def scene_of(rule):
        boxes = []
        for m in spec.boxes:
            x, y, z = scenes._cell_centres(m, spec, torch, device=ctx.device)
            cells = rule(x[None, None, :], y[None, :, None], z[:, None, None]).contiguous()
            boxes.append(AmrBox(m.min_corner, m.max_corner, cells, m.level))
        return ctx.create_scene(boxes, ScalarTransform())

    field, weight = scene_of(FIELD), scene_of(WEIGHT)
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

    def measure(call):
        """call() -> (outputs, event ms); the means of the event and the wall time and the least
        wall time of the timed calls, and the last outputs."""
        samples = []
        for _ in range(warmup + frames):
            t0 = time.perf_counter()
            out, ms = call()
            ctx.synchronize()
            samples.append((ms, (time.perf_counter() - t0) * 1e3))
        samples = samples[warmup:]
        return out, {"event_ms": round(sum(s[0] for s in samples) / len(samples), 4),
                     "wall_ms": round(sum(s[1] for s in samples) / len(samples), 4),
                     "wall_ms_min": round(min(s[1] for s in samples), 4)}

    host = lambda t: None if t is None else t.cpu().numpy()
    result = {"config": "config-4", "boxes": len(spec.boxes), "max_trips": max_trips,
              "frames": frames, "warmup": warmup, "views": {}}
    for image in images:
        start, end = view_rays(image)
        n = start.shape[0]
        order = ray_rules.pixel_order(image, image)
        rays_of = lambda points: torch.from_numpy(np.ascontiguousarray(points)).to(ctx.device)
        row = (rays_of(start), rays_of(end), max_trips, index, ratios, sizes, [0.0, 0.0, 0.0])
        tile = (rays_of(start[order]), rays_of(end[order])) + row[2:]

        def pair(arguments):
            (counts, status, span), count_ms = timed(lambda: field.rays(*arguments), "the count pass")
            offsets = torch.zeros(n + 1, dtype=torch.int64, device=ctx.device)
            torch.cumsum(counts.to(torch.int64), 0, out=offsets[1:])
            ctx.synchronize()
            total = int(offsets[-1].item())
            emitted, emit_ms = timed(
                lambda: field.rays(*arguments, offsets=offsets, n_segments=total), "the emit pass")
            return (counts, status, span, emitted[4], emitted[5], total), count_ms + emit_ms

        view = {"rays": n}
        sums_tile, view["sums_tile_order"] = measure(
            lambda: timed(lambda: field.ray_sums(*tile), "the sums call, tile order"))
        sums_row, view["sums_row_major"] = measure(
            lambda: timed(lambda: field.ray_sums(*row), "the sums call, row-major"))
        weighted, view["weighted_sums_tile_order"] = measure(
            lambda: timed(lambda: field.ray_sums(*tile, weight), "the weighted sums call"))
        pair_tile, view["pair_tile_order"] = measure(lambda: pair(tile))
        pair_row, view["pair_row_major"] = measure(lambda: pair(row))
        view["segments"] = pair_row[5]
        counts, status, span, integral, _, counted, covered = (host(t) for t in sums_tile)
        view["status"] = np.bincount(status, minlength=4).tolist()
        same = lambda a, b: a.tobytes() == b.tobytes()
        view["sums_equal_the_pair_by_bits"] = bool(
            all(same(host(a), host(b)) for a, b in
                ((sums_tile[0], pair_tile[0]), (sums_tile[1], pair_tile[1]),
                 (sums_tile[2], pair_tile[2]), (sums_tile[3], pair_tile[3]),
                 (sums_tile[6], pair_tile[4]), (sums_row[3], pair_row[3]),
                 (sums_row[6], pair_row[4]))))
        view["tile_order_equals_row_major_by_bits"] = bool(
            all(same(host(a), host(b)[order]) for a, b in zip(sums_tile, sums_row) if a is not None))
        view["weighted_counted_equals_covered"] = bool(same(host(weighted[5]), host(weighted[6])))
        view["sums_over_pair"] = round(view["sums_tile_order"]["wall_ms"] /
                                       view["pair_tile_order"]["wall_ms"], 4)
        view["tile_over_row"] = round(view["sums_tile_order"]["wall_ms"] /
                                      view["sums_row_major"]["wall_ms"], 4)
        result["views"][f"{image}x{image}"] = view
        del sums_tile, sums_row, weighted, pair_tile, pair_row
    field.close()
    weight.close()
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
    args = parser.parse_args()
    print(json.dumps(run(args.frames, args.warmup, args.limit, tuple(args.images))))
