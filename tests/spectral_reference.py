"""The definitions of DESIGN.md 7, "Inverse transform, Helmholtz split, potential", in numpy: the
inverse table, the radix-2 transform of one line with a given table -- its loops written out, and
the same butterflies on many lines at once -- the 3-D inverse (z, then y, then x, then the scale),
the Helmholtz split and the inverse Laplacian with their operations in the stated order.  numpy's
elementwise float64 arithmetic rounds every product, sum and quotient on its own, which is what the
kernels do."""
import numpy as np

import fft_reference as fr


def inverse_twiddles(n):
    """V[m] = (W[m].re, -W[m].im) of the forward table: [n / 2, 2]."""
    table = fr.twiddles(n)
    table[:, 1] = -table[:, 1]
    return table


def line_loops(re, im, table):
    """One line with the table `table` ([n / 2, 2]), every loop written out: (re, im) float64 [n]
    -> the unscaled transform, new arrays."""
    n = len(re)
    p = n.bit_length() - 1
    assert 1 << p == n
    vr = np.array([re[fr.bit_reverse(i, p)] for i in range(n)], dtype=np.float64)
    vi = np.array([im[fr.bit_reverse(i, p)] for i in range(n)], dtype=np.float64)
    for s in range(1, p + 1):
        half, step = 1 << (s - 1), n >> s
        for block in range(0, n, 2 * half):
            for j in range(half):
                ar, ai = vr[block + j], vi[block + j]
                br, bi = vr[block + j + half], vi[block + j + half]
                wr, wi = table[j * step]
                tr = np.float64(wr * br) - np.float64(wi * bi)
                ti = np.float64(wr * bi) + np.float64(wi * br)
                vr[block + j], vi[block + j] = ar + tr, ai + ti
                vr[block + j + half], vi[block + j + half] = ar - tr, ai - ti
    return vr, vi


def lines(re, im, table):
    """The same butterflies on the last axis of (re, im) float64 [..., n], all lines at once."""
    n = re.shape[-1]
    p = n.bit_length() - 1
    assert 1 << p == n
    order = np.array([fr.bit_reverse(i, p) for i in range(n)], dtype=np.int64)
    vr, vi = np.array(re[..., order]), np.array(im[..., order])
    lead = vr.shape[:-1]
    for s in range(1, p + 1):
        half, step = 1 << (s - 1), n >> s
        wr, wi = table[np.arange(half) * step, 0], table[np.arange(half) * step, 1]
        vr = vr.reshape(lead + (n // (2 * half), 2, half))
        vi = vi.reshape(lead + (n // (2 * half), 2, half))
        ar, ai = vr[..., 0, :], vi[..., 0, :]
        br, bi = vr[..., 1, :], vi[..., 1, :]
        tr = wr * br - wi * bi
        ti = wr * bi + wi * br
        vr = np.stack([ar + tr, ar - tr], axis=-2).reshape(lead + (n,))
        vi = np.stack([ai + ti, ai - ti], axis=-2).reshape(lead + (n,))
    return vr, vi


def ifft3d(spectrum):
    """float64 [nz, ny, nx, 2] -> (values, imag), float64 [nz, ny, nx] each: along z, then y, then
    x with the inverse tables, then both times s = 1.0 / f64(nx ny nz)."""
    spectrum = np.asarray(spectrum, dtype=np.float64)
    re, im = np.array(spectrum[..., 0]), np.array(spectrum[..., 1])
    for axis in (0, 1, 2):
        table = inverse_twiddles(re.shape[axis])
        re, im = np.moveaxis(re, axis, -1), np.moveaxis(im, axis, -1)
        re, im = lines(re, im, table)
        re, im = np.moveaxis(re, -1, axis), np.moveaxis(im, -1, axis)
    s = 1.0 / float(re.size)
    return np.ascontiguousarray(re * s), np.ascontiguousarray(im * s)


def projector_modes(n):
    """The signed wave numbers with the Nyquist rule: k == n / 2 of an axis of n >= 2 counts 0."""
    m = fr.signed_modes(n)
    if n >= 2:
        m[n // 2] = 0.0
    return m


def kappas(shape, h):
    """(kx, ky, kz) broadcastable over [nz, ny, nx]: kappa_d = f64(m_d) h[d]."""
    nz, ny, nx = shape
    return ((projector_modes(nx) * h[0])[None, None, :], (projector_modes(ny) * h[1])[None, :, None],
            (projector_modes(nz) * h[2])[:, None, None])


def helmholtz(fx, fy, fz, h):
    """(solenoidal, compressive), three spectra [nz, ny, nx, 2] each, of the spectra of (vx, vy,
    vz): q = kx kx + ky ky, then + kz kz; q == 0: C = +0 and S = F with its bits kept; else per
    component d = kx Fx + ky Fy, then + kz Fz, s = d / q, C_d = kappa_d s, S_d = F_d - C_d."""
    f = [np.asarray(v, dtype=np.float64) for v in (fx, fy, fz)]
    k = [kappa[..., None] for kappa in kappas(f[0].shape[:3], h)]
    q = k[0] * k[0] + k[1] * k[1]
    q = q + k[2] * k[2]
    mean = np.broadcast_to(q == 0.0, f[0].shape)
    with np.errstate(all="ignore"):
        d = k[0] * f[0] + k[1] * f[1]
        d = d + k[2] * f[2]
        s = d / q
        compressive = [np.where(mean, 0.0, k[a] * s) for a in range(3)]
        solenoidal = [np.where(mean, f[a], f[a] - k[a] * s) for a in range(3)]
    return solenoidal, compressive


def inverse_laplacian(spectrum, g, scale):
    """The spectrum times r = scale / q (fft_reference.mode_q), (+0, +0) where q == 0."""
    spectrum = np.asarray(spectrum, dtype=np.float64)
    q = fr.mode_q(spectrum.shape[:3], g)[..., None]
    with np.errstate(all="ignore"):
        r = np.float64(scale) / q
        return np.where(q == 0.0, 0.0, spectrum * r)
