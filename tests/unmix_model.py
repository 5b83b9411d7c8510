"""numpy model of the unmixing calls (include/thzgpu.h, "Unmixing every pixel into its materials"): the
element, the projection in the device's lane order, the normal matrix in f64, the coordinate descent in f32 in the
written order with a correctly rounded fmaf, and the residual — what tests/test_unmix_host.py and
tests/test_gpu_unmix.py compare the library with.  Also the planted Gaussian-line mixtures."""
import math

import numpy as np

from pca_model import view  # noqa: F401  (the strided view is the PCA calls')

EPS = 2.0 ** -24          # unit round-off of f32
UNMIX_MAX, MAX_SWEEPS, MAX_LEN = 16, 4096, 512
WAVE = 64


def fma32(x, y, z):
    """fmaf on f32 arrays, correctly rounded: the product of two f32 is exact in f64; its sum with z is rounded to odd
    in f64 (TwoSum gives the error of the f64 addition), and 53 >= 2 * 24 + 2 bits make the final rounding to f32 the
    rounding of the exact value"""
    p = np.asarray(x, np.float32).astype(np.float64) * np.asarray(y, np.float32).astype(np.float64)
    zz = np.asarray(z, np.float32).astype(np.float64)
    p, zz = np.broadcast_arrays(p, zz)
    with np.errstate(all="ignore"):
        s = p + zz
        bb = s - p
        err = (p - (s - bb)) + (zz - bb)
        inexact = np.isfinite(s) & (err != 0)
        back = inexact & (((s > 0) & (err < 0)) | ((s < 0) & (err > 0)))          # the exact sum lies towards zero of s
        t = np.where(back, np.nextafter(s, 0.0), s)
        bits = np.ascontiguousarray(t).view(np.int64) | inexact.astype(np.int64)
        return bits.view(np.float64).astype(np.float32)


def log_ref(ref):
    """lref[j] = (float)log((double)ref[j])"""
    return np.log(np.asarray(ref, np.float32).astype(np.float64)).astype(np.float32)


def element(x, ref=None):
    """-> (u f32 as the device forms it up to the 1 ulp of its logf, u f64 exact) of the f32 matrix x; ref: the
    reference spectrum of the absorbance mode, or None"""
    x = np.asarray(x, np.float32)
    if ref is None:
        return x, x.astype(np.float64)
    with np.errstate(all="ignore"):
        lx = np.log(x.astype(np.float64))
        u = (log_ref(ref)[None, :] - lx.astype(np.float32)).astype(np.float32)
        return u, np.log(np.asarray(ref, np.float32).astype(np.float64))[None, :] - lx


def element_bound(x, ref):
    """|u - exact| allowed per element in the absorbance mode: 2 ulp of |log X|, one rounding of the subtraction, and
    the rounding of lref itself"""
    with np.errstate(all="ignore"):
        lx = np.abs(np.log(np.asarray(x, np.float32).astype(np.float64)))
        lr = np.abs(np.log(np.asarray(ref, np.float32).astype(np.float64)))[None, :]
    return 2.0 * 2.0 ** -23 * lx + EPS * (lx + lr) + EPS * lr


def proj_bound(n):
    """relative to sum_j |u E|: a lane's fmaf chain of ceil(n / 64) terms, six tree adds, two units of slack"""
    return (math.ceil(n / WAVE) + 8) * EPS


def _tree(v):
    """the fixed tree of thz_pca_scores over the 64 lane sums (f32, (..., 64)): four row_shr steps inside each row of
    16 lanes, then the last lane of row 0 / 2 into rows 1 / 3, then lane 31 into rows 2 and 3; the sum is lane 63's"""
    v = np.array(v, np.float32)
    lane = np.arange(WAVE)
    for sh in (1, 2, 4, 8):
        src = np.where(lane % 16 >= sh, lane - sh, lane)
        v = (v + np.where(lane % 16 >= sh, v[..., src], np.float32(0))).astype(np.float32)
    odd = (lane // 16) % 2 == 1
    v = (v + np.where(odd, v[..., (lane // 16) * 16 - 1], np.float32(0))).astype(np.float32)
    high = lane >= 32
    v = (v + np.where(high, v[..., np.full(WAVE, 31)], np.float32(0))).astype(np.float32)
    return v[..., WAVE - 1]


def project(u, e):
    """-> b f32 (npix, K) in the device's order: lane l adds j = l, l + 64, ... with fmaf, then the tree"""
    u, e = np.asarray(u, np.float32), np.asarray(e, np.float32)
    npix, n = u.shape
    k = e.shape[0]
    acc = np.zeros((npix, k, WAVE), np.float32)
    for j0 in range(0, n, WAVE):
        w = min(WAVE, n - j0)
        acc[:, :, :w] = fma32(u[:, None, j0:j0 + w], e[None, :, j0:j0 + w], acc[:, :, :w])
    return _tree(acc)


def project_exact(u64, e):
    """-> (b f64 (npix, K), sum_j |u E| f64 (npix, K))"""
    e64 = np.asarray(e, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        return u64 @ e64.T, np.abs(u64) @ np.abs(e64).T


def prepare(e):
    """thz_host_unmix_prepare -> (G f32 (K, K), rd f32 (K), G64): the products of two f32 are exact in f64, and a
    cumulative sum adds them with j ascending"""
    e64 = np.asarray(e, np.float32).astype(np.float64)
    k = e64.shape[0]
    g64 = np.empty((k, k))
    for i in range(k):
        for c in range(k):
            g64[i, c] = np.cumsum(e64[i] * e64[c])[-1]
    with np.errstate(all="ignore"):
        return g64.astype(np.float32), (1.0 / np.diag(g64)).astype(np.float32), g64


def solve(b, g, rd, n_sweeps):
    """the coordinate descent in f32 in the written order, every pixel for n_sweeps sweeps (a pixel whose sweep changed
    nothing repeats it: the values are those of stopping) -> (a f32 (npix, K), kkt f32 (npix), the running gradient)"""
    b = np.atleast_2d(np.asarray(b, np.float32))
    g_mat, rd = np.asarray(g, np.float32), np.asarray(rd, np.float32)
    npix, k = b.shape
    a = np.zeros((npix, k), np.float32)
    grad = (-b).astype(np.float32)
    zero = np.float32(0.0)
    with np.errstate(all="ignore"):
        for _ in range(n_sweeps):
            moved = False
            for c in range(k):
                an = np.fmax(fma32(-grad[:, c], rd[c], a[:, c]), zero)
                d = (an - a[:, c]).astype(np.float32)
                moved = moved or bool(np.any(d != 0))
                grad = fma32(g_mat[:, c][None, :], d[:, None], grad)
                a[:, c] = an
            if not moved:
                break
        kkt = np.where(a > 0, np.abs(grad), np.fmax(-grad, zero)).max(axis=1).astype(np.float32)
    return a, kkt, grad


def model_of(a, e):
    """m_j: the fmaf(a[c], E[c, j], m) chain from +0 over ascending c -> f32 (npix, n)"""
    a, e = np.asarray(a, np.float32), np.asarray(e, np.float32)
    m = np.zeros((a.shape[0], e.shape[1]), np.float32)
    for c in range(e.shape[0]):
        m = fma32(a[:, c][:, None], e[c][None, :], m)
    return m


def residual(u64, a, e):
    """-> (resid f64 (npix): sum_j (u - m)^2 with m exact in f64, sum_j |u - m| f64, sum_j sum_c |a E| f64)"""
    a64, e64 = np.asarray(a, np.float32).astype(np.float64), np.asarray(e, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        r = u64 - a64 @ e64
        return (r * r).sum(axis=1), np.abs(r).sum(axis=1), (np.abs(a64) @ np.abs(e64))


def unmix(x, e, n_sweeps, ref=None):
    """the whole call on one matrix -> dict(u, b, G, rd, a, kkt, resid)"""
    u, u64 = element(x, ref)
    b = project(u, e)
    g, rd, _ = prepare(e)
    a, kkt, _ = solve(b, g, rd, n_sweeps)
    return dict(u=u, b=b, G=g, rd=rd, a=a, kkt=kkt, resid=residual(u64, a, e)[0])


# ---- the planted cases ------------------------------------------------------------------------------------------
def block_case(k=4, npix=9, seed=0):
    """Endmembers that are indicators of disjoint blocks of 4 columns: G = 4 I and rd = 0.25 exactly.  The rows are
    small non-negative integer mixtures, with block (p mod k) of pixel p set to -3: after one sweep the abundances are
    the planted integers exactly, the negative block gives exactly 0, residual 4 * 9 = 36 and kkt 12 there.
    -> (x f32 (npix, 4 k), E f32 (k, 4 k), planted f32 (npix, k))"""
    rng = np.random.default_rng(seed)
    e = np.zeros((k, 4 * k), np.float32)
    for c in range(k):
        e[c, 4 * c:4 * c + 4] = 1.0
    planted = rng.integers(0, 6, (npix, k)).astype(np.float32)
    planted[np.arange(npix), np.arange(npix) % k] = -3.0
    return (planted @ e).astype(np.float32), e, planted


def line_endmembers(n, k, w):
    """E[c, j] = exp(-1/2 ((j - cen_c) / w)^2) + 0.05, the centres spread evenly over 0.1 n .. 0.9 n"""
    cen = np.linspace(0.1 * n, 0.9 * n, k) if k > 1 else np.array([0.5 * n])
    j = np.arange(n, dtype=np.float64)
    return (np.exp(-0.5 * ((j[None, :] - cen[:, None]) / w) ** 2) + 0.05).astype(np.float32)


def line_mixtures(n, k, w, npix, seed, noise=0.02):
    """random sparse non-negative mixtures of the Gaussian-line endmembers plus `noise` (relative to the largest value
    of the clean rows) -> (x f32 (npix, n), E f32 (k, n), planted f64 (npix, k))"""
    rng = np.random.default_rng(seed)
    e = line_endmembers(n, k, w)
    planted = rng.uniform(0.2, 2.0, (npix, k)) * (rng.random((npix, k)) < 0.4)
    planted[np.arange(npix), rng.integers(0, k, npix)] += 0.5           # no empty row
    clean = planted @ e.astype(np.float64)
    x = clean + noise * np.abs(clean).max() * rng.standard_normal(clean.shape)
    return x.astype(np.float32), e, planted


def nnls_rows(u64, e):
    """scipy.optimize.nnls of every row, f64 -> (npix, K)"""
    from scipy.optimize import nnls
    a = np.asarray(e, np.float32).astype(np.float64).T.copy()
    return np.stack([nnls(a, row, maxiter=30 * a.shape[1])[0] for row in np.asarray(u64, np.float64)])
