"""numpy model of the k-means calls (include/thzgpu.h, "Segmenting a scan into materials"): the step
with f64 distances of the f32-subtracted values, the update, farthest-first seeding and the loop — what
tests/test_cluster_host.py and tests/test_gpu_cluster.py compare the library with.  Also the planted three-material scan."""
import math

import numpy as np

import synth
from pca_model import band_bins, keep, view  # noqa: F401  (the strided view and the mask rule are the PCA calls')

EPS = 2.0 ** -24          # unit round-off of f32
CLUSTER_MAX, MAX_LEN = 16, 512


def dist_bound(n):
    """relative bound of the device's f32 dist2 against the f64 sum over the f32 inputs: one subtraction (its error
    enters the square twice), a lane's fmaf chain of ceil(n / 64) terms, six tree adds, one unit of slack"""
    return (math.ceil(n / 64) + 9) * EPS


def distances(x, cent):
    """-> f64 (npix, K): sum_j (x_j - m_j)^2 with d = x - m ONE f32 subtraction, the squares and their sum exact in f64
    (for small integers) or to f64 rounding"""
    x = np.asarray(x, np.float32)
    cent = np.asarray(cent, np.float32).reshape(-1, x.shape[1])
    out = np.empty((x.shape[0], cent.shape[0]), np.float64)
    with np.errstate(all="ignore"):
        for c in range(cent.shape[0]):
            d = (x - cent[c][None, :]).astype(np.float32).astype(np.float64)
            out[:, c] = (d * d).sum(axis=1)
    return out


def assign(d2):
    """-> (label int32 (npix), dist2 f64 (npix)): the lowest c with the smallest distance, a NaN never wins; all NaN:
    label -1 and dist2 NaN"""
    nan = np.isnan(d2)
    filled = np.where(nan, np.inf, d2)
    label = np.argmin(filled, axis=1).astype(np.int32)          # argmin: the first of equal minima
    # a row whose finite entries are all +Inf: argmin gives the first Inf or NaN column; the rule wants the first non-NaN
    first_ok = np.argmax(~nan, axis=1).astype(np.int32)
    label = np.where(np.isinf(filled[np.arange(len(label)), label]), first_ok, label).astype(np.int32)
    none = nan.all(axis=1)
    best = d2[np.arange(len(label)), label]
    label[none] = -1
    return label, np.where(none, np.nan, best)


def margin_is_within(d2, bound):
    """pixels whose best and second-best distances lie within `bound` (relative) of each other: where an f32 label may
    differ from the f64 one"""
    if d2.shape[1] < 2:
        return np.zeros(d2.shape[0], bool)
    s = np.sort(np.where(np.isnan(d2), np.inf, d2), axis=1)
    with np.errstate(all="ignore"):
        return s[:, 1] - s[:, 0] <= bound * (s[:, 1] + s[:, 0])


def step(x, cent, prev_label=None, mask=None):
    """one thz_cluster_step -> dict(label, dist2 (f64), sums f64 (K, n), abs_sums, counts uint64 (K), inertia, changed,
    farthest, d2 (npix, K))"""
    x = np.asarray(x, np.float32)
    npix, n = x.shape
    cent = np.asarray(cent, np.float32).reshape(-1, n)
    k = cent.shape[0]
    d2 = distances(x, cent)
    label, best = assign(d2)
    prev = np.full(npix, -1, np.int32) if prev_label is None else np.asarray(prev_label, np.int32)
    on = keep(npix, mask) & (label >= 0)
    sums, abs_sums, counts = np.zeros((k, n)), np.zeros((k, n)), np.zeros(k, np.uint64)
    x64 = x.astype(np.float64)
    for c in range(k):
        sel = on & (label == c)
        counts[c] = int(sel.sum())
        sums[c] = x64[sel].sum(axis=0)
        abs_sums[c] = np.abs(x64[sel]).sum(axis=0)
    # dist2 as the device keeps it is f32; for small integers the two are the same number
    with np.errstate(all="ignore"):
        kept = best[on]
        inertia = float(kept.sum()) if kept.size else 0.0
    finite = on & np.isfinite(best)
    farthest = npix
    if finite.any():
        top = best[finite].max()
        farthest = int(np.flatnonzero(finite & (best == top))[0])
    return dict(label=label, dist2=best, sums=sums, abs_sums=abs_sums, counts=counts, inertia=inertia,
                changed=int((label != prev).sum()), farthest=farthest, d2=d2)


def update(sums, counts, previous):
    """thz_host_cluster_update: (float)(sum / count) in f64; an empty cluster keeps its previous centroid"""
    prev = np.asarray(previous, np.float32)
    out = prev.copy()
    for c in range(prev.shape[0]):
        if counts[c]:
            out[c] = (np.asarray(sums[c], np.float64) / float(counts[c])).astype(np.float32)
    return out


def seeds(x, k, mask=None):
    """farthest-first: the pixel farthest from the mean, then the one farthest from its nearest seed; with no finite
    farthest pixel the remaining seeds repeat the last one"""
    x = np.asarray(x, np.float32)
    on = keep(x.shape[0], mask)
    mu = (x[on].astype(np.float64).sum(axis=0) / float(on.sum())).astype(np.float32)
    cent = np.zeros((k, x.shape[1]), np.float32)
    for i in range(k):
        far = step(x, cent[:i] if i else mu[None, :], mask=mask)["farthest"]
        if far >= x.shape[0]:
            assert i > 0, "no pixel at a finite distance from the mean"
            cent[i] = cent[i - 1]
        else:
            cent[i] = x[far]
    return cent


def kmeans(x, k, max_iter=100, mask=None, centroids=None):
    """thz_session_cluster -> dict(label, dist2, centroids (the ones the last step used), counts, inertia, iterations,
    converged)"""
    cent = seeds(x, k, mask) if centroids is None else np.asarray(centroids, np.float32).reshape(k, -1).copy()
    label, out = None, None
    for it in range(1, max_iter + 1):
        out = step(x, cent, label, mask)
        label = out["label"]
        done = out["changed"] == 0
        if done or it == max_iter:
            break
        cent = update(out["sums"], out["counts"], cent)
    return dict(label=label, dist2=out["dist2"], centroids=cent, counts=out["counts"], inertia=out["inertia"], iterations=it,
                converged=int(done), last=out)


def same_partition(a, b):
    """do two label arrays name the same partition, up to a renaming of the labels?"""
    a, b = np.asarray(a).ravel(), np.asarray(b).ravel()
    pairs = set(zip(a.tolist(), b.tolist()))
    return len(pairs) == len({p[0] for p in pairs}) == len({p[1] for p in pairs})


# ---- the planted scan -------------------------------------------------------------------------------------------
LINES = ((0.55, 1.30), (0.80, 1.70), (1.05, 2.00))   # THz: each material's own absorption lines


def planted_materials(nx=16, ny=12):
    """three disjoint regions -> int (nx, ny): 0 the left block, 1 the upper right, 2 the lower right"""
    xx, yy = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    return np.where(xx < nx * 3 // 8, 0, np.where(yy < ny // 2, 1, 2)).astype(np.int32)


def planted_scan(nx=16, ny=12, nt=1001, seed=11, noise=0.01):
    """One pulse through three materials in disjoint regions: material m takes exp(-1.2) of the spectrum's amplitude out
    at each of its own two lines (Gaussian, 0.08 THz wide), plus noise of `noise` times the pulse's peak.
    -> (time, cube (nx, ny, nt) f32, material (nx, ny) int32)"""
    rng = np.random.default_rng(seed)
    time = synth.make_time(nt)
    t = time.astype(np.float64) - float(time[0]) - 10.0
    z = t / 0.35
    pulse = -z * np.exp(-z * z)
    spec = np.fft.rfft(pulse)
    f = np.arange(nt // 2 + 1, dtype=np.float64) / (float(time[-1]) - float(time[0]))
    traces = []
    for lines in LINES:
        a = sum(1.2 * np.exp(-0.5 * ((f - f0) / 0.08) ** 2) for f0 in lines)
        traces.append(np.fft.irfft(spec * np.exp(-a), nt))
    material = planted_materials(nx, ny)
    cube = np.stack(traces)[material] + noise * np.abs(pulse).max() * rng.standard_normal((nx, ny, nt))
    return time, np.ascontiguousarray(cube, np.float32), material
