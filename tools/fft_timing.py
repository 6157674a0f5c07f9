"""Power-spectrum timing, one rank: Context.fft3d of a random float64 grid of 128^3, 256^3 and 512^3
cells, and Context.spectrum_bins of its spectrum with the default edges, timed with events on the
context's stream (3 warm-up and 10 timed calls by default).  Next to each transform, in the same
process and timed the same way on torch's stream:

  copy   three torch copies of a tensor as large as the spectrum (16 bytes per cell read and 16
         written, three times): the bytes that three read-and-write passes over the spectrum
         move, the floor of any transform that makes one pass per axis
  fftn   torch.fft.fftn of the same array: the vendor library

One JSON line is printed.  Needs a HIP device: fails loudly without one."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = (128, 256, 512)


def run(frames: int, warmup: int, sizes=SIZES) -> dict:
    import torch
    from amrvolumerenderer_amd import runtime, spectra
    if not torch.cuda.is_available():
        raise SystemExit("tools/fft_timing.py needs a HIP device")
    ctx = runtime.Context(0)
    generator = torch.Generator(device=ctx.device).manual_seed(11)
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
        cells = n ** 3
        values = torch.randn((n, n, n), dtype=torch.float64, device=ctx.device,
                             generator=generator)
        torch.cuda.synchronize()
        fft_ms = timed(lambda: ctx.fft3d(values), ctx.stream)
        spectrum = ctx.fft3d(values)
        size = (1.0 / n,) * 3
        g = spectra.inverse_length_sq((n, n, n), size)
        edges_sq = spectra.squared_edges(spectra.default_edges((n, n, n), size))
        out = ctx.spectrum_bins(spectrum, g, edges_sq)
        bins_ms = timed(lambda: ctx.spectrum_bins(spectrum, g, edges_sq, out), ctx.stream)
        target = torch.empty_like(spectrum)

        def three_copies():
            for _ in range(3):
                target.copy_(spectrum)
        copy_ms = timed(three_copies, torch.cuda.current_stream())
        del target
        fftn_ms = timed(lambda: torch.fft.fftn(values), torch.cuda.current_stream())
        label = f"n{n}"
        result[label + "_cells"] = cells
        result[label + "_fft_ms"] = round(fft_ms, 4)
        result[label + "_fft_TBps"] = round(cells * 88 / fft_ms / 1e9, 3)   # 8 + 16 + 4 x 16 bytes
        result[label + "_bins_ms"] = round(bins_ms, 4)
        result[label + "_bins_TBps"] = round(cells * 16 / bins_ms / 1e9, 3)
        result[label + "_copy_ms"] = round(copy_ms, 4)
        result[label + "_fftn_ms"] = round(fftn_ms, 4)
        result[label + "_fft_vs_copy"] = round(fft_ms / copy_ms, 2)
        result[label + "_fft_vs_fftn"] = round(fft_ms / fftn_ms, 2)
        del values, spectrum, out
    ctx.close()
    return result


if __name__ == "__main__":
    parser = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    parser.add_argument("--frames", type=int, default=10)
    parser.add_argument("--warmup", type=int, default=3)
    args = parser.parse_args()
    print(json.dumps(run(args.frames, args.warmup)))
