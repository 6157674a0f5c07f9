"""Timing of the isolated potential, one rank: Context.isolated_green and
Context.spectrum_multiply on the padded grids of regions of 64^3, 128^3 and 256^3 cells (128^3,
256^3 and 512^3 padded cells), and the whole chain of api.isolated_potential_scene's device work --
pad, transform, Green's grid, transform, product, inverse transform with its imaginary part, crop
-- on a random float64 region, timed with events on the context's stream (3 warm-up and 10 timed
calls by default).  Next to each kernel, in the same process and timed the same way on torch's
stream, a torch call that moves the bytes the kernel must move:

  green      one fill of a real grid (8 bytes per cell written)
  multiply   one copy of a spectrum and one read of another (32 bytes per mode read, 16 written):
             torch.add of two spectra into the first

One JSON line is printed.  Needs a HIP device: fails loudly without one."""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = (64, 128, 256)


def run(frames: int, warmup: int, sizes=SIZES) -> dict:
    import torch
    from amrvolumerenderer_amd import runtime, spectra
    if not torch.cuda.is_available():
        raise SystemExit("tools/isolated_potential_timing.py needs a HIP device")
    ctx = runtime.Context(0)
    generator = torch.Generator(device=ctx.device).manual_seed(13)
    result = {"frames": frames, "warmup": warmup}

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
        padded = spectra.padded_dims((n, n, n))
        cells = math.prod(padded)
        size = (1.0 / n,) * 3
        scale = -(size[0] * size[1] * size[2] / (4.0 * math.pi))
        region = torch.randn((n, n, n), dtype=torch.float64, device=ctx.device,
                             generator=generator)
        a = torch.randn(padded[::-1] + (2,), dtype=torch.float64, device=ctx.device,
                        generator=generator)
        b = torch.randn(padded[::-1] + (2,), dtype=torch.float64, device=ctx.device,
                        generator=generator) * 0.5       # |b| stays near 1: no overflow in 13 calls
        real = torch.empty(padded[::-1], dtype=torch.float64, device=ctx.device)
        torch.cuda.synchronize()
        here = torch.cuda.current_stream()
        label = f"n{n}"
        result[label + "_padded_cells"] = cells

        green_ms = timed(lambda: ctx.isolated_green(padded, size, scale), ctx.stream)
        fill_ms = timed(lambda: real.fill_(0.5), here)
        multiply_ms = timed(lambda: ctx.spectrum_multiply(a, b), ctx.stream)
        add_ms = timed(lambda: a.add_(b), here)
        del a, b, real

        def chain():
            grid = torch.zeros(padded[::-1], dtype=torch.float64, device=ctx.device)
            grid[:n, :n, :n] = region
            spectrum = ctx.fft3d(grid)
            del grid
            green = ctx.isolated_green(padded, size, scale)
            kernel = ctx.fft3d(green)
            del green
            ctx.spectrum_multiply(spectrum, kernel)
            del kernel
            values, imag = ctx.ifft3d(spectrum, with_imag=True)
            del spectrum
            worst = imag[:n, :n, :n].abs().max()
            potential = values[:n, :n, :n].contiguous()
            ctx.join()                  # the context's stream, and its end event, behind the crop
            return potential, worst
        chain_ms = timed(chain, ctx.stream)

        for name, ms, bytes_per_cell, other, other_ms in (
                ("green", green_ms, 8, "fill", fill_ms),
                ("multiply", multiply_ms, 48, "add", add_ms)):
            result[f"{label}_{name}_ms"] = round(ms, 4)
            result[f"{label}_{name}_TBps"] = round(cells * bytes_per_cell / ms / 1e9, 3)
            result[f"{label}_{name}_{other}_ms"] = round(other_ms, 4)
            result[f"{label}_{name}_vs_{other}"] = round(ms / other_ms, 2)
        result[label + "_chain_ms"] = round(chain_ms, 4)
        del region
    ctx.close()
    return result


if __name__ == "__main__":
    parser = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    parser.add_argument("--frames", type=int, default=10)
    parser.add_argument("--warmup", type=int, default=3)
    args = parser.parse_args()
    print(json.dumps(run(args.frames, args.warmup)))
