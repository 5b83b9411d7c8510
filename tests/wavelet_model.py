"""numpy model of the wavelet shrinkage of include/thzgpu.h ("Denoising every trace", K23): the undecimated transform with
periodic extension, the threshold from the lower median of |d_1|, soft or hard shrinkage and the inverse — in f64, and in
f32 with numpy's own summation order (products rounded one by one, no fused multiply-add).  With check_exact the f64 form
asserts that every intermediate, the partial sums of every chain included, is an f32 number: then no order of summation
and no fusing matters, and the library must return the same values.

The Daubechies filters are derived here, by spectral factorisation, independently of the library's literals."""
import functools
from math import comb

import numpy as np

BAR_FACTOR, BAR_FLOOR = 8.0, 16 * 2.0 ** -24
MAD = 0.6744897501960817


@functools.lru_cache(maxsize=None)
def daubechies(p):
    """the orthonormal Daubechies scaling filter with p vanishing moments, 2 p taps in minimum-phase order, sum = sqrt 2:
    |H(w)|^2 = 2 cos^2p(w/2) P(sin^2(w/2)) with P(y) = sum_k C(p-1+k, k) y^k; y = (2 - z - 1/z) / 4 maps every root of P
    to a pair (z, 1/z), of which the one inside the unit circle is kept"""
    h = np.array([1.0])
    if p > 1:
        for y in np.roots([comb(p - 1 + k, k) for k in range(p - 1, -1, -1)]):
            z = np.roots([1.0, 4.0 * y - 2.0, 1.0])     # z^2 - (2 - 4 y) z + 1 = 0
            h = np.convolve(h, [1.0, -z[np.argmin(np.abs(z))]])
    for _ in range(p):
        h = np.convolve(h, [1.0, 1.0])
    h = np.real(h)
    h = h * (np.sqrt(2.0) / h.sum())
    for m in range(p):                                   # sum_k h[k] h[k + 2 m] = delta_m
        assert abs(np.dot(h[:h.size - 2 * m], h[2 * m:]) - (m == 0)) < 1e-14, (p, m)
    h.setflags(write=False)
    return h


def analysis_pair(order):
    """(hn, gn) f32 rounded as thz_host_wavelet_filter rounds them: hn = h / sqrt 2, gn[k] = (-1)^k h[Lf-1-k] / sqrt 2"""
    h = daubechies(order)
    sign = np.where(np.arange(h.size) % 2, -1.0, 1.0)
    return (h / np.sqrt(2.0)).astype(np.float32), (sign * h[::-1] / np.sqrt(2.0)).astype(np.float32)


def universal(nt, n_levels):
    """the universal thresholds under the MAD noise estimate, f64"""
    j = np.arange(1, n_levels + 1)
    return (np.sqrt(2.0) / MAD) * 2.0 ** (-j / 2.0) * np.sqrt(2.0 * np.log(nt))


def _is_f32(v):
    return np.array_equal(v, v.astype(np.float32).astype(np.float64))


def _chain(taps, a, s, sign, dtype, check_exact):
    """out[:, i] = sum over k ascending of taps[k] a[:, (i + sign s k) mod N]"""
    acc = np.zeros(a.shape, dtype)
    for k in range(taps.size):
        acc = acc + dtype(taps[k]) * np.roll(a, -sign * s * k, axis=1)
        if check_exact:
            assert _is_f32(acc), "a partial sum is no f32 number"
    return acc


def shrink(d, th, hard):
    """th: one threshold per trace (column vector)"""
    if hard:
        return np.where(np.abs(d) > th, d, 0.0).astype(d.dtype)
    t = np.abs(d) - th
    return np.where(t > 0, np.copysign(t, d), 0.0).astype(d.dtype)


def denoise(y, hn, gn, scale, n_levels, shrink_mode=0, noise_mode=0, dtype=np.float64, check_exact=False):
    """-> dict(x (npix, nt), sigma (npix), kept (npix)) in `dtype`; hn, gn and scale are taken as the f32 numbers the
    library sees"""
    y = np.atleast_2d(np.asarray(y, np.float32)).astype(dtype)
    hn, gn, scale = (np.asarray(v, np.float32).astype(dtype) for v in (hn, gn, scale))
    assert not check_exact or dtype is np.float64
    nt = y.shape[1]
    a, details, m, kept = y, [], None, np.zeros(y.shape[0], np.int64)
    for j in range(1, n_levels + 1):
        s = 2 ** (j - 1)
        d = _chain(gn, a, s, +1, dtype, check_exact)
        a = _chain(hn, a, s, +1, dtype, check_exact)
        if j == 1:
            k = (nt - 1) // 2
            m = np.partition(np.abs(d), k, axis=1)[:, k]
        th = (scale[j - 1] * m if noise_mode == 0 else np.full_like(m, scale[j - 1])).astype(dtype)
        d = shrink(d, th[:, None], shrink_mode)
        if check_exact:
            assert _is_f32(th) and _is_f32(d)
        kept += (d != 0).sum(axis=1)
        details.append(d)
    for j in range(n_levels, 0, -1):
        s = 2 ** (j - 1)
        a = _chain(hn, a, s, -1, dtype, check_exact) + _chain(gn, details[j - 1], s, -1, dtype, check_exact)
        if check_exact:
            assert _is_f32(a)
    return dict(x=a, sigma=m, kept=kept)


def exact_solution(y, hn, gn, scale, n_levels, shrink_mode, noise_mode):
    """the exact-arithmetic result as the f32 numbers it consists of -> (x f32, sigma f32, kept int32)"""
    r = denoise(y, hn, gn, scale, n_levels, shrink_mode, noise_mode, np.float64, check_exact=True)
    return r["x"].astype(np.float32), r["sigma"].astype(np.float32), r["kept"].astype(np.int32)


HAAR = (np.array([0.5, 0.5], np.float32), np.array([0.5, -0.5], np.float32))


def haar_case(nt, npix=5, seed=0):
    """integer samples in [-256, 256]: every Haar level halves, so J <= 6 leaves multiples of 2^-12 below 2^10"""
    rng = np.random.default_rng(1000 * nt + seed)
    return rng.integers(-256, 257, (npix, nt)).astype(np.float32)


def integer_taps(n_taps, seed):
    """two taps of +-1 or +-2 at either end of each filter (one when n_taps == 1), zeros between: the wrap is exercised by
    the last tap, and a level multiplies magnitudes by at most 4 forward and 8 backward"""
    rng = np.random.default_rng(seed)
    hn, gn = np.zeros(n_taps, np.float32), np.zeros(n_taps, np.float32)
    for v in (hn, gn):
        v[0] = rng.choice((-2, -1, 1, 2))
        v[n_taps - 1] = rng.choice((-2, -1, 1, 2))
    return hn, gn


def integer_case(n_taps, nt, npix=5, seed=0):
    """-> (hn, gn, y, J): integer taps and samples, with the most levels (at most 6) whose values stay below 2^24:
    |a_j| <= 4^j |y|, |d_j| likewise, |r_{j-1}| <= 4 |r_j| + 4 |d_j|, so |x| <= 2 * 16^J max |y| with max |y| = 4"""
    hn, gn = integer_taps(n_taps, 31 * n_taps + nt + seed)
    rng = np.random.default_rng(77 * n_taps + nt + seed)
    y = rng.integers(-4, 5, (npix, nt)).astype(np.float32)
    J = max(j for j in range(1, 7) if 2 * 16 ** j * 4 < 2 ** 24)
    return hn, gn, y, J


def deviation(x, x64, y):
    """per trace: the largest |x - x64| against that trace's own largest |y|"""
    scale = np.abs(np.asarray(y, np.float64)).max(axis=1)
    return np.abs(np.asarray(x, np.float64) - np.asarray(x64, np.float64)).max(axis=1) / np.where(scale > 0, scale, 1.0)


def reference_and_bar(y, hn, gn, scale, n_levels, shrink_mode, noise_mode):
    """-> (f64 result dict, bar): the bar is BAR_FACTOR times the largest per-trace deviation of the numpy f32 form from
    the f64 form over the batch, at least BAR_FLOOR — taken from the two models alone"""
    ref = denoise(y, hn, gn, scale, n_levels, shrink_mode, noise_mode, np.float64)
    f32 = denoise(y, hn, gn, scale, n_levels, shrink_mode, noise_mode, np.float32)
    return ref, max(BAR_FACTOR * float(deviation(f32["x"], ref["x"], y).max()), BAR_FLOOR)


def pulse(t, tau=0.35):
    """the pulse of tests/synth.py"""
    z = np.asarray(t, np.float64) / tau
    return -z * np.exp(-z * z)


def noisy_pulses(npix=32, nt=1001, dt=0.05, sigma=0.03, seed=5):
    """traces shaped as tests/synth.py shapes them — amplitude 1 .. 1.5, the pulse 10 .. 12 ps in, an echo of 0.3 times
    the amplitude 3 .. 20 ps behind it, tau = 0.35 ps — plus white noise of deviation sigma -> (clean f64, noisy f32)"""
    rng = np.random.default_rng(seed)
    t = dt * np.arange(nt)[None, :]
    A = 1.0 + 0.5 * rng.random((npix, 1))
    tc = 10.0 + 2.0 * rng.random((npix, 1))
    delta = 3.0 + 17.0 * rng.random((npix, 1))
    clean = A * pulse(t - tc) + 0.3 * A * pulse(t - tc - delta)
    return clean, (clean + sigma * rng.standard_normal((npix, nt))).astype(np.float32)


def tolerance_case(nt, npix=8, seed=0):
    """noisy pulses of length nt for the tolerance configurations"""
    return noisy_pulses(npix, nt, seed=100 + nt + seed)[1]


TOLERANCE_CONFIGS = [(order, J, nt) for order in (2, 4) for J in (3, 5) for nt in (257, 1001)]
