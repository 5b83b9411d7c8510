"""numpy model of the principal-component calls (include/thzgpu.h, "Principal components of a scan"):
f64 sums, the f64 Gram matrix of the f32-subtracted values, numpy.linalg.eigh and the sign rule — what
tests/test_pca_host.py and tests/test_gpu_pca.py compare the library with.  Also the planted two-material scan."""
import numpy as np

import synth

EPS = 2.0 ** -24          # unit round-off of f32
MAX_LEN, MAX_COMPONENTS = 512, 8


def view(flat, npix, n, row_stride, col_step=1, off=0):
    """X[p, j] = flat[off + p * row_stride + j * col_step] as a (npix, n) array (a copy)"""
    idx = off + np.arange(npix, dtype=np.int64)[:, None] * row_stride + np.arange(n, dtype=np.int64)[None, :] * col_step
    return np.asarray(flat, np.float32).ravel()[idx]


def keep(npix, mask):
    return np.ones(npix, bool) if mask is None else np.asarray(mask).ravel() != 0


def sums(x, mask=None):
    """-> (sum f64 (n), sum of |x| f64 (n), count) over the unmasked pixels"""
    k = keep(x.shape[0], mask)
    x64 = x[k].astype(np.float64)
    return x64.sum(axis=0), np.abs(x64).sum(axis=0), int(k.sum())


def mean_of(total, count):
    """mu = (float)(sum / count) in f64"""
    return (np.asarray(total, np.float64) / float(count)).astype(np.float32)


def centred(x, mu=None, mask=None):
    """a = X - mu: ONE f32 subtraction; a masked pixel enters as zeros"""
    a = np.asarray(x, np.float32) if mu is None else (np.asarray(x, np.float32) - np.asarray(mu, np.float32)[None, :]).astype(np.float32)
    if mask is not None:
        a = np.where(keep(a.shape[0], mask)[:, None], a, np.float32(0.0))
    return a


def gram(a):
    """-> (G f64 (n, n), sum_p |a_pi a_pj| f64 (n, n)) of f32 values a"""
    a64 = a.astype(np.float64)
    with np.errstate(all="ignore"):
        return a64.T @ a64, np.abs(a64).T @ np.abs(a64)


def sign_rule(v):
    """the entry of largest magnitude positive, the lowest index winning a tie; magnitudes compared as they round to
    f32, so that a tie in exact arithmetic is a tie whatever the last bits of the f64 vector"""
    v = np.asarray(v, np.float64)
    v = v / np.sqrt((v * v).sum())
    top = int(np.argmax(np.abs(v.astype(np.float32))))      # argmax: the first of equal maxima
    return -v if v[top] < 0 else v


def components(g, count, k):
    """-> dict(components f32 (k, n), vectors f64 (k, n), eigenvalues f64 (k), all_eigenvalues f64 (n) descending,
    total_variance, cov f64 (n, n))"""
    c = np.asarray(g, np.float64) / float(count - 1)
    w, v = np.linalg.eigh(c)
    order = np.argsort(-w, kind="stable")
    w, v = w[order], v[:, order]
    vec = np.stack([sign_rule(v[:, i]) for i in range(k)])
    return dict(components=vec.astype(np.float32), vectors=vec, eigenvalues=w[:k].copy(), all_eigenvalues=w,
                total_variance=float(np.trace(c)), cov=c)


def scores(a, comps):
    """-> (S f64 (k, npix), sum_j |a_j v_j| f64 (k, npix)) of f32 a and f32 components"""
    a64, v64 = a.astype(np.float64), np.asarray(comps, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        return v64 @ a64.T, np.abs(v64) @ np.abs(a64).T


def residual(c, lam, vecs):
    """max |C v - lambda v| over the given pairs (vectors as rows)"""
    v = np.asarray(vecs, np.float64)
    return float(np.abs(c @ v.T - v.T * np.asarray(lam, np.float64)[None, :]).max())


def residual_floor(c):
    """L 2^-52 ||C||_F: the rounding of one L-term product row"""
    return c.shape[0] * 2.0 ** -52 * float(np.sqrt((c * c).sum()))


def orthogonality(vecs):
    v = np.asarray(vecs, np.float64)
    return float(np.abs(v @ v.T - np.eye(v.shape[0])).max())


def pca(x, k, centre=True, mask=None):
    """the four calls on one matrix -> dict(sum, count, mu, gram, scores, + components()'s entries)"""
    total, _, count = sums(x, mask)
    mu = mean_of(total, count) if centre else None
    g, _ = gram(centred(x, mu, mask))
    out = components(g, count, k)
    s, _ = scores(centred(x, mu), out["components"])
    out.update(sum=total, count=count, mu=np.zeros(x.shape[1], np.float32) if mu is None else mu, gram=g, scores=s)
    return out


# ---- the planted scan -------------------------------------------------------------------------------------------
def planted_scan(nx=16, ny=12, nt=1001, seed=5, noise=0.01):
    """A scan of a background material with two further materials planted in it: every trace is the mix
    (1 - a1 - a2) s0 + a1 s1 + a2 s2 of three pulses of one arrival time and different widths (different spectra), plus noise of
    `noise` times the background pulse's peak.
    -> (time, cube (nx, ny, nt) f32, a1 (nx, ny), a2 (nx, ny))"""
    rng = np.random.default_rng(seed)
    time = synth.make_time(nt)
    t = time.astype(np.float64) - float(time[0]) - 10.0

    def pulse(tau, amp):
        z = t / tau
        return amp * (-z * np.exp(-z * z))

    s0, s1, s2 = pulse(0.35, 1.0), pulse(0.55, 0.9), pulse(0.22, 0.8)
    xx, yy = np.meshgrid(np.arange(nx) / max(nx - 1, 1), np.arange(ny) / max(ny - 1, 1), indexing="ij")
    a1 = 0.8 * np.exp(-(((xx - 0.3) / 0.18) ** 2 + ((yy - 0.35) / 0.25) ** 2))          # an inclusion
    a2 = 0.6 * np.clip((xx - 0.55) / 0.3, 0.0, 1.0) * (yy > 0.5)                          # a wet patch with a ramp
    mix = ((1.0 - a1 - a2)[..., None] * s0 + a1[..., None] * s1 + a2[..., None] * s2)
    cube = mix + noise * np.abs(s0).max() * rng.standard_normal(mix.shape)
    return time, np.ascontiguousarray(cube, np.float32), a1, a2


def band_bins(time, lo=0.2, hi=5.0):
    """-> (first, count) of the bins with lo <= f <= hi on the frequency axis of `time`"""
    f = np.arange(len(time) // 2 + 1, dtype=np.float64) / (float(time[-1]) - float(time[0]))
    k = np.flatnonzero((f >= lo) & (f <= hi))
    return int(k[0]), int(k.size)


def explained(target, score_images):
    """R^2 of the least-squares fit of a map by a constant and the score images"""
    a = np.stack([np.ones(target.size)] + [s.ravel().astype(np.float64) for s in score_images], axis=1)
    coef, *_ = np.linalg.lstsq(a, target.ravel(), rcond=None)
    r = target.ravel() - a @ coef
    return 1.0 - float((r * r).sum() / ((target - target.mean()) ** 2).sum())
