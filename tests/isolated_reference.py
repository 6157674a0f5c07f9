"""The definitions of DESIGN.md 7, "Isolated potential", in numpy: the padding rule, the
open-boundary Green's grid -- vectorised, and with every loop written out in Python floats --, the
product of two spectra and the whole zero-padded convolution with the transforms of
fft_reference and spectral_reference, every operation in the stated order.  numpy's elementwise
float64 arithmetic rounds every product, sum, quotient and square root on its own, which is what the
kernels do.  direct_sum is the independent answer: the potential cell by cell with math.fsum."""
import math

import numpy as np

import fft_reference as fr
import spectral_reference as sr

U = 2.0 ** -53


def padded_dims(dims):
    """(Px, Py, Pz): per axis the smallest power of two >= 2 N - 1, by a loop."""
    out = []
    for n in dims:
        n = int(n)
        if not 1 <= n <= 512:
            raise ValueError("every N must lie in [1, 512]")
        p = 1
        while p < 2 * n - 1:
            p *= 2
        out.append(p)
    return tuple(out)


def host_values(constant, size, self_term=0.0):
    """(scale, self_value) as the host forms them: volume = (dx dy) dz, scale = -((constant
    volume) / (4.0 pi)), self_value = scale self_term."""
    volume = (float(size[0]) * float(size[1])) * float(size[2])
    scale = -((float(constant) * volume) / (4.0 * math.pi))
    return scale, scale * float(self_term)


def image_offsets(p):
    """s = min(i, P - i) for every index of an axis of P cells, as float64 [P]."""
    i = np.arange(p, dtype=np.int64)
    return np.minimum(i, p - i).astype(np.float64)


def green(padded, size, scale, self_value=0.0):
    """G float64 [Pz, Py, Px]: x_d = f64(s_d) size_d, r2 = x x + y y, then + z z, G = scale /
    sqrt(r2), and self_value where r2 == 0."""
    px, py, pz = padded
    x = (image_offsets(px) * size[0])[None, None, :]
    y = (image_offsets(py) * size[1])[None, :, None]
    z = (image_offsets(pz) * size[2])[:, None, None]
    r2 = x * x + y * y
    r2 = r2 + z * z
    with np.errstate(all="ignore"):
        g = np.float64(scale) / np.sqrt(r2)
    return np.ascontiguousarray(np.where(r2 == 0.0, np.float64(self_value), g))


def green_loops(padded, size, scale, self_value=0.0):
    """The same grid, every loop written out in Python floats (IEEE binary64, math.sqrt correctly
    rounded, nothing fused)."""
    px, py, pz = padded
    out = np.zeros((pz, py, px), dtype=np.float64)
    for k in range(pz):
        for j in range(py):
            for i in range(px):
                x = float(min(i, px - i)) * float(size[0])
                y = float(min(j, py - j)) * float(size[1])
                z = float(min(k, pz - k)) * float(size[2])
                r2 = x * x + y * y
                r2 = r2 + z * z
                out[k, j, i] = float(self_value) if r2 == 0.0 else float(scale) / math.sqrt(r2)
    return out


def multiply(a, b):
    """The product of two spectra [nz, ny, nx, 2]: re = a.re b.re - a.im b.im, im = a.re b.im +
    a.im b.re, each from two products and one addition."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    with np.errstate(all="ignore"):
        re = a[..., 0] * b[..., 0] - a[..., 1] * b[..., 1]
        im = a[..., 0] * b[..., 1] + a[..., 1] * b[..., 0]
    return np.ascontiguousarray(np.stack([re, im], axis=-1))


def pad(rho, padded):
    """rho [nz, ny, nx] at the low corner of a grid [Pz, Py, Px] of +0.0."""
    rho = np.asarray(rho, dtype=np.float64)
    nz, ny, nx = rho.shape
    grid = np.zeros(tuple(padded)[::-1], dtype=np.float64)
    grid[:nz, :ny, :nx] = rho
    return grid


def isolated_potential(rho, size, scale, self_value=0.0):
    """rho float64 [nz, ny, nx] with cells of size (dx, dy, dz) -> a dict: potential and imag
    [nz, ny, nx], imag_max, padded_dims, and the norms of the bound: rho_norm = ||rho_pad||_2,
    green_norm = ||G||_2."""
    rho = np.asarray(rho, dtype=np.float64)
    nz, ny, nx = rho.shape
    padded = padded_dims((nx, ny, nz))
    grid = pad(rho, padded)
    g = green(padded, size, scale, self_value)
    with np.errstate(all="ignore"):
        real, imag = sr.ifft3d(multiply(fr.fft3d(grid), fr.fft3d(g)))
        real = np.ascontiguousarray(real[:nz, :ny, :nx])
        imag = np.ascontiguousarray(imag[:nz, :ny, :nx])
        worst = np.abs(imag).max()
    return {"potential": real, "imag": imag, "imag_max": float(worst),   # max lets a NaN through
            "padded_dims": padded, "rho_norm": float(np.linalg.norm(grid.ravel())),
            "green_norm": float(np.linalg.norm(g.ravel()))}


def unit(result):
    """One unit of the a-priori bound: 2^-53 log2(Ptot) ||rho_pad||_2 ||G||_2 (0 for Ptot = 1)."""
    cells = math.prod(result["padded_dims"])
    return U * math.log2(cells) * result["rho_norm"] * result["green_norm"]


def direct_sum(rho, size, scale, self_value=0.0):
    """phi_i = sum_j G(x_i - x_j) rho_j cell by cell: the terms rho_j * (scale / r_ij) in Python
    floats -- r_ij from the integer offsets as the Green's grid forms it -- and rho_i * self_value,
    added exactly by math.fsum and rounded once.  float64 [nz, ny, nx]."""
    rho = np.asarray(rho, dtype=np.float64)
    nz, ny, nx = rho.shape
    cells = [(k, j, i) for k in range(nz) for j in range(ny) for i in range(nx)]
    values = [float(rho[c]) for c in cells]
    out = np.zeros(rho.shape, dtype=np.float64)
    # G of every offset once: it depends on |di|, |dj|, |dk| alone
    table = green_loops((2 * nx, 2 * ny, 2 * nz), size, scale, self_value)[:nz, :ny, :nx]
    for k, j, i in cells:
        terms = [v * float(table[abs(k - c), abs(j - b), abs(i - a)])
                 for (c, b, a), v in zip(cells, values)]
        out[k, j, i] = math.fsum(terms)
    return out
