"""numpy model of the sparse deconvolution (include/thzgpu.h, "Sparse deconvolution"): ISTA / FISTA on a batch of traces
in f64, and in f32 with every product a numpy matrix product (numpy's own summation order, not the library's).  Also the
cases the tests of the feature share: the exact-arithmetic inputs, the tolerance configurations with their bars, and the
thin-coating traces.  Not a test module."""
import functools

import numpy as np

EPS24 = 2.0 ** -24
BAR_FACTOR, BAR_FLOOR = 8.0, 16 * EPS24

# (P, c, nt): every intermediate of two iterations is an f32 number for these (the model asserts it)
EXACT_SHAPES = ((1, 0, 17), (5, 2, 33), (65, 64, 97), (64, 0, 130), (33, 16, 257), (256, 128, 300))
EXACT_STEP, EXACT_REL = 2.0 ** -10, 2.0 ** -3
# (P, c, nt, n_iter, accelerate)
TOLERANCE_CONFIGS = ((64, 32, 257, 100, 0), (64, 32, 257, 100, 1), (128, 40, 300, 60, 1), (31, 15, 130, 200, 1))


def pulse(t, tau=0.35):
    """the pulse of tests/synth.py"""
    z = np.asarray(t, np.float64) / tau
    return -z * np.exp(-z * z)


def pulse_taps(n_taps, center, dt=0.05):
    """-> (taps f32, step f32 = 1 / (sum |taps|)^2 in double)"""
    h = pulse((np.arange(n_taps) - center) * dt).astype(np.float32)
    return h, np.float32(1.0 / np.abs(h.astype(np.float64)).sum() ** 2)


@functools.lru_cache(maxsize=2)
def _toeplitz(taps, c, nt):
    h = np.frombuffer(taps, np.float64)
    k = np.arange(nt, dtype=np.int32)[:, None] + np.int32(c) - np.arange(nt, dtype=np.int32)[None, :]
    M = np.where((k >= 0) & (k < h.size), h[np.clip(k, 0, h.size - 1)], 0.0)
    M.setflags(write=False)
    return M


def toeplitz(h, c, nt):
    """T[i, m] = h[i + c - m], zero outside the taps (f64, read-only: the last two are kept)"""
    return _toeplitz(np.ascontiguousarray(h, np.float64).tobytes(), int(c), int(nt))


def apply_h(x, h, c):
    """H x per trace in f64"""
    x, h = np.atleast_2d(np.asarray(x, np.float64)), np.asarray(h, np.float64)
    nt = x.shape[1]
    return np.array([np.convolve(row, h)[c:c + nt] for row in x])


def momentum(n_iter):
    """beta[n] = (float)((t_n - 1) / t_{n+1}) in double"""
    beta, t = np.zeros(n_iter, np.float32), 1.0
    for n in range(n_iter):
        tn = (1.0 + np.sqrt(1.0 + 4.0 * t * t)) / 2.0
        beta[n] = np.float32((t - 1.0) / tn)
        t = tn
    return beta


def _is_f32(a):
    return np.array_equal(a, a.astype(np.float32).astype(np.float64))


def solve(y, h, c, n_iter, accelerate, step, rel_lambda, min_lambda=0.0, dtype=np.float64, check_exact=False):
    """y (npix, nt) -> dict(x (npix, nt), resid (npix) f64 of the returned x, nnz (npix)) in `dtype` arithmetic;
    check_exact: assert that every intermediate is an f32 number (the exact-arithmetic cases, dtype f64)"""
    y = np.ascontiguousarray(y, dtype)
    M = toeplitz(h, c, y.shape[1]).astype(dtype)
    step, beta = dtype(step), momentum(n_iter).astype(dtype)
    g0 = (y @ M).astype(dtype)                                    # row p: H^T y_p
    gmax = np.abs(g0).max(axis=1, keepdims=True)
    lam = np.maximum((dtype(rel_lambda) * gmax).astype(dtype), dtype(min_lambda))
    th = (step * lam).astype(dtype)
    if check_exact:
        assert _is_f32(g0) and _is_f32(lam) and _is_f32(th)
    x = np.zeros_like(y)
    z = x.copy()
    for n in range(n_iter):
        r = (y - (z @ M.T).astype(dtype)).astype(dtype)
        g = (r @ M).astype(dtype)
        v = (z + (step * g).astype(dtype)).astype(dtype)
        a = (np.abs(v) - th).astype(dtype)
        xn = np.where(a > 0, np.copysign(a, v), 0).astype(dtype)
        if check_exact:
            assert all(_is_f32(q) for q in (r, g, (step * g).astype(dtype), v, a, xn)), n
        z = (xn + (beta[n] * (xn - x)).astype(dtype)).astype(dtype) if accelerate else xn
        x = xn
    x64 = x.astype(np.float64)
    d = y.astype(np.float64) - x64 @ toeplitz(h, c, y.shape[1]).T
    return dict(x=x, resid=(d * d).sum(axis=1), nnz=(x != 0).sum(axis=1).astype(np.int32))


def resid_of(y, h, c, x):
    """sum of (y - H x)^2 per trace in f64, of a given x"""
    d = np.atleast_2d(np.asarray(y, np.float64)) - apply_h(x, h, c)
    return (d * d).sum(axis=1)


def exact_case(P, c, nt, npix=6, seed=7, taps=None):
    """integer taps in [-3, 3] with h[c] = 3, integer samples in [-8, 8] -> (h f32, y f32 (npix, nt))"""
    rng = np.random.default_rng(seed + 1000 * P + nt)
    h = rng.integers(-3, 4, P).astype(np.float32)
    h[c] = 3
    if taps is not None:
        h = np.asarray(taps, np.float32)
    return h, rng.integers(-8, 9, (npix, nt)).astype(np.float32)


def exact_solution(h, c, y, n_iter, accelerate):
    """the exact x of the exact-arithmetic inputs, f32 (the model asserts that every intermediate is representable)"""
    out = solve(y, h, c, n_iter, accelerate, EXACT_STEP, EXACT_REL, 0.0, np.float64, check_exact=True)
    return out["x"].astype(np.float32), out["nnz"]


def planted_traces(h, c, nt, npix, seed, spikes=None, noise=0.01):
    """two planted spikes 4 .. 29 samples apart (or the given list of (sample, amplitude) per trace), convolved with the
    taps, `noise` added -> y f32 (npix, nt)"""
    rng = np.random.default_rng(seed)
    M = toeplitz(h, c, nt)
    y = np.zeros((npix, nt))
    for p in range(npix):
        xt = np.zeros(nt)
        if spikes is None:
            a = int(rng.integers(20, nt - 60))
            xt[a] = 1 + rng.random()
            xt[a + int(rng.integers(4, 30))] = 0.6 * (1 if p % 2 else -1)
        else:
            for at, amp in spikes[p % len(spikes)]:
                xt[at] += amp
        y[p] = M @ xt + noise * rng.standard_normal(nt)
    return y.astype(np.float32)


def tolerance_case(P, c, nt, npix=24, seed=11):
    """-> (h f32, step f32, y f32 (npix, nt)) of one tolerance configuration"""
    h, step = pulse_taps(P, c)
    return h, step, planted_traces(h, c, nt, npix, seed + P + nt)


def deviation(x, x64):
    """per trace: the largest |x - x64| against that trace's own largest |x64|"""
    x64 = np.asarray(x64, np.float64)
    scale = np.abs(x64).max(axis=1)
    return np.abs(np.asarray(x, np.float64) - x64).max(axis=1) / np.where(scale > 0, scale, 1.0)


def reference_and_bar(y, h, c, n_iter, accelerate, step, rel_lambda=0.05, min_lambda=0.0):
    """-> (f64 solution dict, bar): the bar is BAR_FACTOR times the largest per-trace deviation of the numpy f32 form from
    the f64 form over the batch, at least BAR_FLOOR — taken from the two models alone"""
    ref = solve(y, h, c, n_iter, accelerate, step, rel_lambda, min_lambda, np.float64)
    f32 = solve(y, h, c, n_iter, accelerate, step, rel_lambda, min_lambda, np.float32)
    return ref, max(BAR_FACTOR * float(deviation(f32["x"], ref["x"]).max()), BAR_FLOOR)


def thin_wedge_scan(nx=16, ny=12, nt=384, n_taps=64, center=32, gap0=8, gap1=39, noise=0.01, seed=9, dt=0.05):
    """a reflection scan of a thin wedge: per pixel a unit front-surface pulse (at sample 150 .. 152) and a back-surface
    pulse 0.6 times as large, of alternating sign, gap0 .. gap1 samples later — the gap rises over the grid in whole
    samples -> (time f32, cube (nx, ny, nt) f32, gap (nx, ny) in samples, h f32, step f32)"""
    h, step = pulse_taps(n_taps, center, dt)
    npix = nx * ny
    gap = gap0 + (np.arange(npix) * (gap1 - gap0 + 1)) // npix
    spikes = [((150 + p % 3, 1.0), (150 + p % 3 + int(gap[p]), 0.6 if p % 2 else -0.6)) for p in range(npix)]
    y = planted_traces(h, center, nt, npix, seed, spikes, noise)
    t = (1000.0 + dt * np.arange(nt)).astype(np.float32)
    return t, y.reshape(nx, ny, nt), gap.reshape(nx, ny), h, step


def thin_coating_traces(nt=384, n_taps=64, center=32, gaps=range(8, 40), signs=(1, -1), at=150, noise=0.01, seed=3):
    """a unit pulse at `at` and a +-0.6 echo `gap` samples later, one trace per gap and sign
    -> (h f32, step f32, y f32 (len(gaps) * len(signs), nt), gap per trace)"""
    h, step = pulse_taps(n_taps, center)
    spikes = [((at, 1.0), (at + g, 0.6 * s)) for s in signs for g in gaps]
    y = planted_traces(h, center, nt, len(spikes), seed, spikes, noise)
    return h, step, y, np.array([g for s in signs for g in gaps])
