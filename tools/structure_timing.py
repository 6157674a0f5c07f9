"""Timing of the structure functions, one rank: Context.structure_functions on random float64
vector grids of 128^3 and 256^3 cells with structure.default_lags (156 and 182 lags), three
components, orders 1 to 6, periodic, timed with events on the context's stream (3 warm-up and 10
timed calls by default).  Next to each, in the same process and timed the same way on torch's
stream, a torch restatement of the same sums -- per lag torch.roll of the three grids, the
differences, the longitudinal, transverse and whole increments, their powers and torch.sum -- which
is the only comparison; the largest relative difference between the two sets of sums is printed
with the times, with the pairs per second and the bytes per pair the kernel loads (48: the centre
and the partner of three grids, before any reuse in the caches).

One JSON line is printed.  Needs a HIP device: fails loudly without one."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = (128, 256)
ORDER = 6


def run(frames: int, warmup: int, sizes=SIZES) -> dict:
    import torch
    from amrvolumerenderer_amd import runtime, structure
    if not torch.cuda.is_available():
        raise SystemExit("tools/structure_timing.py needs a HIP device")
    ctx = runtime.Context(0)
    generator = torch.Generator(device=ctx.device).manual_seed(17)
    result = {"frames": frames, "warmup": warmup, "max_order": ORDER}

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

    for n in sizes:
        dims, size = (n, n, n), (1.0 / n,) * 3
        lags = structure.default_lags(dims)
        units = structure.unit_directions(lags, size)
        grids = [torch.randn((n, n, n), dtype=torch.float64, device=ctx.device,
                             generator=generator) for _ in range(3)]
        out = tuple(torch.zeros(shape, dtype=dtype, device=ctx.device) for shape, dtype in
                    (((len(lags),), torch.int64), ((len(lags), 3, ORDER), torch.float64),
                     ((2,), torch.int64)))
        torch.cuda.synchronize()
        here = torch.cuda.current_stream()
        restated = torch.zeros((len(lags), 3, ORDER), dtype=torch.float64, device=ctx.device)

        def restatement():
            for m, (lag, u) in enumerate(zip(lags.tolist(), units.tolist())):
                shift = (-lag[2], -lag[1], -lag[0])         # v(x + l) at x
                dx, dy, dz = (torch.roll(g, shift, (0, 1, 2)) - g for g in grids)
                along = dx * u[0] + dy * u[1] + dz * u[2]
                across = ((dx - along * u[0]) ** 2 + (dy - along * u[1]) ** 2 +
                          (dz - along * u[2]) ** 2).sqrt()
                whole = (dx * dx + dy * dy + dz * dz).sqrt()
                for kind, amount in enumerate((along.abs(), across, whole)):
                    power = amount
                    for p in range(ORDER):
                        if p > 0:
                            power = power * amount
                        restated[m, kind, p] = power.sum()

        kernel_ms = timed(lambda: ctx.structure_functions(grids, lags, units, ORDER, True, out),
                          ctx.stream)
        torch_ms = timed(restatement, here)
        calls = warmup + frames
        ctx.synchronize()
        difference = ((out[1] / calls - restated).abs() / restated).max().item()
        pairs = len(lags) * n ** 3
        label = f"n{n}"
        result[label + "_lags"] = len(lags)
        result[label + "_pairs"] = pairs
        result[label + "_kernel_ms"] = round(kernel_ms, 4)
        result[label + "_Gpairs_per_s"] = round(pairs / kernel_ms / 1e6, 2)
        result[label + "_loaded_TBps"] = round(pairs * 48 / kernel_ms / 1e9, 3)
        result[label + "_torch_ms"] = round(torch_ms, 3)
        result[label + "_torch_over_kernel"] = round(torch_ms / kernel_ms, 1)
        result[label + "_largest_relative_difference"] = difference
        assert int(out[0].min()) == int(out[0].max()) == calls * n ** 3 and not out[2].any()
        del grids, restated
    ctx.close()
    return result


if __name__ == "__main__":
    parser = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    parser.add_argument("--frames", type=int, default=10)
    parser.add_argument("--warmup", type=int, default=3)
    args = parser.parse_args()
    print(json.dumps(run(args.frames, args.warmup)))
