"""Timing of the inverse transform and the per-mode operators, one rank: Context.ifft3d (with and
without the imaginary part), Context.helmholtz_split and Context.inverse_laplacian on random
float64 spectra of 128^3, 256^3 and 512^3 modes, timed with events on the context's stream (3
warm-up and 10 timed calls by default).  Next to each call, in the same process and timed the same
way on torch's stream, torch copies of the bytes the call must move:

  ifft3d       two copies of a tensor as large as the spectrum (16 bytes per mode read and 16
               written per strided pass) and one copy of its real parts into a real grid (16 read,
               8 written: the x pass)
  helmholtz    three copies of a spectrum and three fills of one (48 bytes per mode read, 96 written)
  laplacian    one copy of a spectrum (16 read, 16 written)

and, for the inverse, torch.fft.ifftn of the same complex array: the vendor library.  One JSON
line is printed.  Needs a HIP device: fails loudly without one."""
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
        raise SystemExit("tools/spectral_timing.py needs a HIP device")
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
        modes = n ** 3
        size = (1.0 / n,) * 3
        g = spectra.inverse_length_sq((n, n, n), size)
        h = spectra.inverse_length((n, n, n), size)
        three = [torch.randn((n, n, n, 2), dtype=torch.float64, device=ctx.device,
                             generator=generator) for _ in range(3)]
        spectrum = three[0]
        target = torch.empty_like(spectrum)
        real = torch.empty((n, n, n), dtype=torch.float64, device=ctx.device)
        torch.cuda.synchronize()
        here = torch.cuda.current_stream()
        label = f"n{n}"
        result[label + "_modes"] = modes

        # the per-mode operators first: the inverse overwrites its spectrum
        split_ms = timed(lambda: ctx.helmholtz_split(*three, h), ctx.stream)

        def split_bytes():
            for source in three:
                target.copy_(source)
            for _ in range(3):
                target.zero_()
        split_copy_ms = timed(split_bytes, here)
        laplacian_ms = timed(lambda: ctx.inverse_laplacian(three[1], g, -1.0), ctx.stream)
        laplacian_copy_ms = timed(lambda: target.copy_(spectrum), here)

        ifftn_ms = timed(lambda: torch.fft.ifftn(torch.view_as_complex(three[2])), here)
        ifft_ms = timed(lambda: ctx.ifft3d(spectrum), ctx.stream)
        ifft_imag_ms = timed(lambda: ctx.ifft3d(spectrum, with_imag=True), ctx.stream)

        def ifft_bytes():
            for _ in range(2):
                target.copy_(spectrum)
            real.copy_(spectrum[..., 0])
        ifft_copy_ms = timed(ifft_bytes, here)

        for name, ms, bytes_per_mode, copy_ms in (
                ("ifft", ifft_ms, 88, ifft_copy_ms),             # 2 x (16 + 16) + 16 + 8
                ("ifft_imag", ifft_imag_ms, 96, ifft_copy_ms),   # ... + 8: no copy times those
                ("helmholtz", split_ms, 144, split_copy_ms),
                ("laplacian", laplacian_ms, 32, laplacian_copy_ms)):
            result[f"{label}_{name}_ms"] = round(ms, 4)
            result[f"{label}_{name}_TBps"] = round(modes * bytes_per_mode / ms / 1e9, 3)
            result[f"{label}_{name}_copy_ms"] = round(copy_ms, 4)
            result[f"{label}_{name}_vs_copy"] = round(ms / copy_ms, 2)
        result[label + "_ifftn_ms"] = round(ifftn_ms, 4)
        result[label + "_ifft_vs_ifftn"] = round(ifft_ms / ifftn_ms, 2)
        del three, spectrum, target, real
    ctx.close()
    return result


if __name__ == "__main__":
    parser = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    parser.add_argument("--frames", type=int, default=10)
    parser.add_argument("--warmup", type=int, default=3)
    args = parser.parse_args()
    print(json.dumps(run(args.frames, args.warmup)))
