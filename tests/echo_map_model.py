"""numpy model of the echo maps and the layer maps (include/thzgpu.h, "Echoes and layer thickness"): the selection of
the K strongest separated pulses per trace, their offsets through peak_tilt_model.peak_model's fp64 parabola, and
thz_layer_map in f32 in the operation order the header writes.  Also the planted scans the tests of the feature share.
Not a test module."""
import numpy as np

import peak_tilt_model as peak

C_MM_PER_PS = peak.C_MM_PER_PS
INT_MAX = np.iinfo(np.int32).max


def keys(x, mode):
    x = np.asarray(x, np.float32)
    return {0: np.abs(x), 1: x, 2: -x}[mode]


def vertex_model(x, k):
    """peak_model's value, fp64 parabola offset, rounding bar and `ok` around the given indices k (npix) of x (npix, nt);
    rows with k < 0 (absent ranks) give value 0, offset 0, ok False"""
    x = np.asarray(x, np.float32)
    nt = x.shape[-1]
    have = k >= 0
    kk = np.where(have, k, 0)
    x64 = x.astype(np.float64)
    take = lambda idx: np.take_along_axis(x64, idx[..., None], -1)[..., 0]
    y0, ym, yp = take(kk), take(np.clip(kk - 1, 0, nt - 1)), take(np.clip(kk + 1, 0, nt - 1))
    with np.errstate(all="ignore"):
        den = ym - 2 * y0 + yp
        ok = have & (kk > 0) & (kk < nt - 1) & (den != 0) & np.isfinite(ym) & np.isfinite(y0) & np.isfinite(yp)
        off = np.where(ok, 0.5 * (ym - yp) / np.where(ok, den, 1.0), 0.0)
        bar = np.where(ok, 8 * np.finfo(np.float32).eps * (np.abs(ym) + 2 * np.abs(y0) + np.abs(yp)) / np.abs(np.where(ok, den, 1.0)), 0.0)
    value = np.where(have, np.take_along_axis(x, kk[..., None], -1)[..., 0], np.float32(0))
    return value.astype(np.float32), np.clip(off, -0.5, 0.5), bar, ok


def echo_model(x, mode, n_echoes, guard, rel_threshold):
    """x (npix, nt) f32 -> dict(index (K, npix) int64 with -1 for absent ranks, count (npix), value (K, npix) f32,
    offset (K, npix) fp64, bar, ok (K, npix))"""
    x = np.ascontiguousarray(x, np.float32)
    npix, nt = x.shape
    rows, pos = np.arange(npix), np.arange(nt)
    k0 = peak.peak_model(x, mode)[0]
    with np.errstate(all="ignore"):
        key = keys(x, mode)
        low = np.where(np.isnan(key), np.float32(-np.inf), key)          # a NaN key is ordered as -Inf
        rise = np.ones((npix, nt), bool)
        rise[:, 1:] = key[:, 1:] > low[:, :-1]
        hold = np.ones((npix, nt), bool)
        hold[:, :-1] = key[:, :-1] >= low[:, 1:]
        thr = np.float32(rel_threshold) * key[rows, k0]                  # one f32 product
        avail = ~np.isnan(key) & rise & hold & (key >= thr[:, None])     # false throughout for a NaN threshold
    index = np.full((n_echoes, npix), -1, np.int64)
    index[0] = k0
    alive = np.ones(npix, bool)
    for j in range(1, n_echoes):
        avail &= np.abs(pos[None, :] - index[j - 1][:, None]) >= guard
        has = avail.any(1)
        masked = np.where(avail, key, np.float32(-np.inf))
        best = masked.argmax(1)                                          # the first of equal keys, -0 == +0
        # admitted keys of -Inf only: argmax cannot tell them from the mask
        best = np.where(np.isneginf(masked.max(1)), avail.argmax(1), best)
        alive &= has
        index[j] = np.where(alive, best, -1)
    parts = [vertex_model(x, index[j]) for j in range(n_echoes)]
    value, offset, bar, ok = (np.stack([p[q] for p in parts]) for q in range(4))
    return dict(index=index, count=(index >= 0).sum(0), value=value, offset=offset, bar=bar, ok=ok)


def layer_model(index, offset, mode, scale, ref_index=0, ref_offset=0.0):
    """thz_layer_map on (K, npix) index / offset maps, f32 in the header's operation order -> (thickness, delay), each
    (K - 1, npix) for mode 0 and (1, npix) for mode 1"""
    index = np.asarray(index, np.int32)
    offset = np.asarray(offset, np.float32)
    scale = np.asarray(scale, np.float32)
    K, npix = index.shape
    with np.errstate(all="ignore"):
        if mode == 1:
            delay = (index[0] - np.int32(ref_index)).astype(np.float32) + (offset[0] - np.float32(ref_offset))
            return (scale[0] * delay)[None, :], delay[None, :]
        order = np.argsort(np.where(index >= 0, index, INT_MAX), axis=0, kind="stable")
        si, so = np.take_along_axis(index, order, 0), np.take_along_axis(offset, order, 0)
        n = (index >= 0).sum(0)
        delay = np.full((K - 1, npix), np.nan, np.float32)
        thick = np.full((K - 1, npix), np.nan, np.float32)
        for l in range(K - 1):
            d = (si[l + 1] - si[l]).astype(np.float32) + (so[l + 1] - so[l])
            have = l + 1 < n
            delay[l] = np.where(have, d, np.float32(np.nan))
            thick[l] = np.where(have, scale[l] * d, np.float32(np.nan))
    return thick, delay


def pulse(z):
    return -z * np.exp(-z * z)


def wedge_scan(nx, ny, nt, n_index=1.5, d0_mm=0.6, d1_mm=1.4, noise=0.01, seed=5, dt=0.05, tau=0.35, back=0.5):
    """a reflection scan of a wedge: per pixel a front-surface pulse and a back-surface pulse `back` times as large,
    2 n d / c later, d rising linearly over the grid from d0 to d1 mm; `noise` of the unit amplitude
    -> (time f32, cube (nx, ny, nt) f32, thickness (nx, ny) fp64 mm, the front pulse alone as a reference trace f32)"""
    rng = np.random.default_rng(seed)
    t = (1000.0 + dt * np.arange(nt)).astype(np.float32)
    ramp = (np.arange(nx)[:, None] * ny + np.arange(ny)[None, :]) / (nx * ny - 1)
    d = d0_mm + (d1_mm - d0_mm) * ramp
    t_front = float(t[0]) + 0.2 * nt * dt + 0.3 * rng.random((nx, ny))
    t_back = t_front + 2.0 * n_index * d / C_MM_PER_PS
    tt = t[None, None, :].astype(np.float64)
    s = pulse((tt - t_front[:, :, None]) / tau) + back * pulse((tt - t_back[:, :, None]) / tau)
    s = s + noise * rng.standard_normal((nx, ny, nt))
    reference = pulse((t.astype(np.float64) - (float(t[0]) + 0.2 * nt * dt)) / tau).astype(np.float32)
    return t, s.astype(np.float32), d, reference
