"""Unmixing on the device (csrc/unmix.hip, unmix_api.cpp) against the numpy model of unmix_model.py and
the library's own host twin.

- exact case   indicator endmembers over disjoint blocks of 4 columns and small integers: every product and partial sum
               is an integer below 2^24, so projections, abundances, residual and kkt are the planted numbers bit for bit.
               (kkt is 0 at the pixel's negative block, where b = -12: the gradient +12 there is the multiplier of a
               constraint that holds, not a violation — tests/test_unmix_host.py has the note.)
- real data    |b - exact| <= (ceil(L / 64) + 8) 2^-24 sum_j |u E|, exact the f64 sum over the f32 inputs; abundances and
               kkt bit for bit thz_host_unmix_solve's from the DOWNLOADED b (-0 and +0 compared as numbers); the residual
               as derived below.
- purpose      the planted Gaussian-line mixtures against scipy.optimize.nnls in f64 at 1e-5 of the pixel's largest
               abundance (tests/test_unmix_host.py: the model alone is 7x inside).
- session      the planted three-material scan: the session call is the stage call on the session's buffer, the resident
               centroids are the explicit ones, and every pixel's largest abundance belongs to its k-means label.
- groups       same-device groups of 2 and 3 members: the members' maps stacked are one session's.

The residual's bound.  With a the device's own abundances, r_j = u_j - m_j and M_j = sum_c |a_c E_cj| in exact
arithmetic, the device forms mh_j by K fmaf (K roundings: |mh_j - m_j| <= K eps M_j to first order, eps = 2^-24), then
rh_j = fl(u_j - mh_j) and the sum of rh_j^2 in f32.  The roundings of the subtraction, of each square inside its fmaf
and of the L - 1 additions, in whatever order, are covered by (L + K + 8) eps sum_j r_j^2, the bar the definition sets.
What the rounding of m adds is sum_j ((r_j - e_j)^2 - r_j^2) with |e_j| <= K eps M_j:
    2 K eps sum_j |r_j| M_j + (K eps)^2 sum_j M_j^2,
carried through the same summation, i.e. times (1 + (L + K + 8) eps).  It is not small against the first term when the
fit is good: r is then noise while M is the whole signal."""
import ctypes
import functools
import math

import numpy as np
import pytest

import cluster_model
import unmix_model as model
import thz_image_explorer_amd as pkg
from test_gpu_cluster import _bits, _flat, _layouts
from test_gpu_helper_sizes import Dev

pytestmark = pytest.mark.gpu

EPS = model.EPS
LENGTHS = [1, 63, 64, 65, 512]
ENDMEMBERS = [1, 2, 8, 16]
PIXELS = [1, 63, 65, 1000]
BAR = 1e-5


def _same_numbers(a, b):
    """bit for bit, -0 and +0 compared as numbers"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and bool(np.all((_bits(a) == _bits(b)) | ((a == 0) & (b == 0))))


def _run(engine, d, x, layout, e, sweeps, ref=None, proj=True, resid=True, kkt=True):
    """one thz_unmix on the matrix x laid out as `layout` -> dict(a (npix, K), b, resid, kkt; None where not asked for)"""
    npix, n = x.shape
    k = e.shape[0]
    row_stride, col_step, off = layout
    dx = d.put(_flat(x, row_stride, col_step, np.nan), off)
    da = d.new((k, npix))
    db = d.new((k, npix), 4) if proj else None
    dr = d.new(npix, 4) if resid else None
    dk = d.new(npix) if kkt else None
    engine.unmix(npix, n, dx, row_stride, col_step, e, da, sweeps, ref=ref, proj=db, resid=dr, kkt=dk)
    return dict(a=d.get(da, (k, npix)).T.copy(), b=d.get(db, (k, npix)).T.copy() if proj else None,
                resid=d.get(dr, npix) if resid else None, kkt=d.get(dk, npix) if kkt else None)


def _host_solve(b, e, sweeps):
    """thz_host_unmix_prepare + thz_host_unmix_solve of every row of b -> (a (npix, K), kkt (npix))"""
    rc, g, rd = pkg.host_unmix_prepare(e)
    assert rc == 0
    lib = pkg.load_library()
    b = np.ascontiguousarray(b, np.float32)
    a, kkt, one = np.zeros_like(b), np.zeros(b.shape[0], np.float32), ctypes.c_float()
    for p in range(b.shape[0]):
        assert lib.thz_host_unmix_solve(b[p].ctypes.data, g.ctypes.data, rd.ctypes.data, b.shape[1], sweeps, a[p].ctypes.data,
                                        ctypes.byref(one)) == 0
        kkt[p] = one.value
    return a, kkt


def _resid_bound(u64, a, e, du=None):
    """-> (want f64 (npix), bound f64 (npix)) of the residual for the device's own abundances a; du: what each element
    of u may be off by (absorbance), which moves r like the rounding of m does"""
    n, k = u64.shape[1], e.shape[0]
    a64, e64 = a.astype(np.float64), e.astype(np.float64)
    r = u64 - a64 @ e64
    big = np.abs(a64) @ np.abs(e64)
    off = k * EPS * big + (0.0 if du is None else du)
    want = (r * r).sum(axis=1)
    first = (n + k + 8) * EPS
    return want, first * want + (1.0 + first) * (2.0 * (np.abs(r) * off).sum(axis=1) + (off * off).sum(axis=1))


def _check(got, x, e, sweeps, tag, ref=None):
    u, u64 = model.element(x, ref)
    exact, mag = model.project_exact(u64, e)
    slack = 0.0 if ref is None else model.element_bound(x, ref) @ np.abs(e.astype(np.float64)).T
    err = np.abs(got["b"] - exact)
    bound = model.proj_bound(x.shape[1]) * mag + slack
    assert np.all(err <= bound), (tag, float((err / bound)[bound > 0].max()))
    a, kkt = _host_solve(got["b"], e, sweeps)
    assert _same_numbers(got["a"], a), (tag, np.flatnonzero((got["a"] != a).any(axis=1))[:8])
    assert _same_numbers(got["kkt"], kkt), (tag, np.flatnonzero(got["kkt"] != kkt)[:8])
    want, rb = _resid_bound(u64, got["a"], e, None if ref is None else model.element_bound(x, ref))
    rerr = np.abs(got["resid"] - want)
    assert np.all(rerr <= rb), (tag, float((rerr / rb)[rb > 0].max()))
    with np.errstate(all="ignore"):
        return float(np.nanmax(np.where(bound > 0, err / bound, 0.0))), float(np.nanmax(np.where(rb > 0, rerr / rb, 0.0)))


# ---- the stage call -------------------------------------------------------------------------------------------------
def test_exact_block_case(engine):
    with Dev(engine) as d:
        for case, (k, npix) in enumerate(((4, 9), (16, 65), (1, 1), (2, 1000))):
            x, e, planted = model.block_case(k, npix, seed=case)
            got = _run(engine, d, x, _layouts(4 * k, npix)[case % 4], e, 1)
            negative = planted < 0
            assert np.array_equal(_bits(got["b"]), _bits(4 * planted)), (k, npix)
            assert np.array_equal(_bits(got["a"]), _bits(np.where(negative, 0, planted).astype(np.float32))), (k, npix)
            assert np.array_equal(got["resid"], np.full(npix, 36, np.float32)) and not got["kkt"].any(), (k, npix)
            assert np.all(got["b"][negative] == -12.0)
            # no sweep at all: zeros, the whole row left over, and the condition violated by the largest positive b
            got = _run(engine, d, x, (4 * k, 1, 0), e, 0)
            assert not got["a"].any() and np.array_equal(got["resid"], (x.astype(np.float64) ** 2).sum(axis=1).astype(np.float32))
            assert np.array_equal(got["kkt"], np.fmax(4 * planted, 0).max(axis=1))


@pytest.mark.parametrize("n", LENGTHS)
def test_random_data_inside_the_bounds(engine, n):
    rng = np.random.default_rng(7000 + n)
    with Dev(engine) as d:
        for case, k in enumerate(ENDMEMBERS):
            npix = PIXELS[(case + LENGTHS.index(n)) % 4]
            layout = _layouts(n, npix)[(case + n) % 4]
            e = (rng.random((k, n)) + 0.2 * rng.standard_normal((k, n))).astype(np.float32)
            mix = rng.uniform(0, 2, (npix, k)) * (rng.random((npix, k)) < 0.6)
            x = (mix @ e + 0.3 * rng.standard_normal((npix, n))).astype(np.float32)
            got = _run(engine, d, x, layout, e, 32)
            worst = _check(got, x, e, 32, (n, k, npix, layout))
            print(f"L = {n}, K = {k}, npix = {npix}: projection error / bound {worst[0]:.3g}, residual error / bound {worst[1]:.3g}")
            assert np.all(got["a"] >= 0)


def test_more_pixels_than_one_grid_pass_stage_time_and_same_bits(engine):
    """1024 blocks x 8 waves cover 8192 pixels: the 9001 here take a second trip of the two wave-per-pixel kernels'
    pixel loops, and 36 blocks of the lane-per-pixel solve, the last one with 215 lanes beyond the end"""
    npix, n, k = 9001, 65, 3
    rng = np.random.default_rng(5)
    e = (rng.random((k, n)) + 0.1).astype(np.float32)
    x = (rng.uniform(0, 2, (npix, k)) @ e + 0.1 * rng.standard_normal((npix, n))).astype(np.float32)
    with Dev(engine) as d:
        engine.enable_timing(1)
        try:
            a = _run(engine, d, x, (n + 1, 1, 4), e, 16)
            assert engine.stage_time_ns(pkg.STAGE_PCA) > 0
        finally:
            engine.enable_timing(0)
        _check(a, x, e, 16, "9001 pixels")
        b = _run(engine, d, x, (n + 1, 1, 4), e, 16)
        for key in ("a", "b", "resid", "kkt"):
            assert np.array_equal(_bits(a[key]), _bits(b[key])), key


@functools.lru_cache(maxsize=None)
def _lines(n, k, w):
    x, e, planted = model.line_mixtures(n, k, w, 200, seed=n + k)
    return x, e, model.nnls_rows(x.astype(np.float64), e)


@pytest.mark.parametrize("n,k,w", [(512, 16, 14), (65, 2, 10)])
def test_planted_lines_against_scipy_nnls(engine, n, k, w):
    pytest.importorskip("scipy")
    x, e, ref = _lines(n, k, w)
    with Dev(engine) as d:
        got = _run(engine, d, x, (n, 1, 0), e, 256)
    err = float((np.abs(got["a"] - ref).max(axis=1) / ref.max(axis=1)).max())
    kkt = float((got["kkt"] / np.abs(got["b"]).max(axis=1)).max())
    print(f"L = {n}, K = {k}, 256 sweeps: error vs nnls {err:.3g}, kkt / |b| {kkt:.3g}")
    assert err <= BAR


def test_absorbance_mode(engine):
    """u = log(ref) - log(X): Beer-Lambert mixtures of absorbance spectra.  Prints the largest error of the device's
    projection in units of the stated bound, 2 ulp of |log X| per element included"""
    n, k, npix = 129, 3, 300
    rng = np.random.default_rng(12)
    e = model.line_endmembers(n, k, 9.0)
    ref = rng.uniform(0.5, 2.0, n).astype(np.float32)
    mix = rng.uniform(0, 1.5, (npix, k)) * (rng.random((npix, k)) < 0.7)
    x = (ref[None, :] * np.exp(-(mix @ e.astype(np.float64))) * (1.0 + 0.01 * rng.standard_normal((npix, n)))).astype(np.float32)
    with Dev(engine) as d:
        got = _run(engine, d, x, (n + 1, 1, 4), e, 128, ref=ref)
        worst = _check(got, x, e, 128, "absorbance", ref=ref)
        print(f"absorbance: projection error / bound {worst[0]:.3g}, residual error / bound {worst[1]:.3g}")
        assert np.all(np.abs(got["a"] - mix) <= 0.05)                     # the planted fractions, to the noise
        plain = _run(engine, d, x, (n + 1, 1, 4), e, 128)                  # absorbance == 0 does not read the reference
        assert not np.array_equal(plain["b"], got["b"])
        _check(plain, x, e, 128, "plain")


def test_nan_row_leaves_its_neighbours_alone(engine):
    n, k, npix = 129, 4, 300
    rng = np.random.default_rng(9)
    e = (rng.random((k, n)) + 0.1).astype(np.float32)
    x = (rng.uniform(0, 2, (npix, k)) @ e + 0.1 * rng.standard_normal((npix, n))).astype(np.float32)
    bad = x.copy()
    bad[10, 70] = np.nan
    bad[77, :] = np.inf
    bad[299, 0] = -np.inf
    others = np.delete(np.arange(npix), [10, 77, 299])
    with Dev(engine) as d:
        clean = _run(engine, d, x, (n, 1, 0), e, 64)
        got = _run(engine, d, bad, (n, 1, 0), e, 64)
    for key in ("a", "b", "resid", "kkt"):
        assert np.array_equal(_bits(got[key][others]), _bits(clean[key][others])), key


def test_null_optional_outputs(engine):
    n, k, npix = 65, 8, 63
    rng = np.random.default_rng(3)
    e = (rng.random((k, n)) + 0.1).astype(np.float32)
    x = (rng.uniform(0, 2, (npix, k)) @ e + 0.1 * rng.standard_normal((npix, n))).astype(np.float32)
    with Dev(engine) as d:
        full = _run(engine, d, x, (n, 1, 0), e, 32)
        for proj, resid, kkt in ((False, True, True), (True, False, True), (True, True, False), (False, False, False)):
            got = _run(engine, d, x, (n, 1, 0), e, 32, proj=proj, resid=resid, kkt=kkt)
            for key in ("a", "b", "resid", "kkt"):
                assert got[key] is None or np.array_equal(_bits(got[key]), _bits(full[key])), (key, proj, resid, kkt)


def test_refusals_and_empty_input(engine):
    x = np.ones((8, 16), np.float32)
    e = np.ones((2, 16), np.float32)
    e[1, :8] = 0.0
    ref = np.ones(16, np.float32)
    with Dev(engine) as d:
        dx, da = d.put(x), d.put(np.full((2, 8), 5, np.float32))
        ok = lambda **kw: engine.unmix(kw.get("npix", 8), kw.get("n", 16), kw.get("x", dx), 16, kw.get("col_step", 1), kw.get("e", e),
                                       kw.get("a", da), kw.get("sweeps", 4), ref=kw.get("ref"), absorbance=kw.get("absorbance"))
        ok()
        ok(ref=ref)
        ok(sweeps=0)
        ok(sweeps=4096)
        nan_e, zero_e = e.copy(), e.copy()
        nan_e[0, 3], zero_e[1] = np.nan, 0.0
        for bad in (dict(n=0), dict(n=513), dict(col_step=0), dict(x=None), dict(a=None), dict(sweeps=-1), dict(sweeps=4097),
                    dict(e=np.ones((17, 16), np.float32)), dict(e=np.ones((0, 16), np.float32)), dict(e=nan_e), dict(e=zero_e),
                    dict(absorbance=True), dict(ref=np.zeros(16, np.float32)), dict(ref=-ref), dict(ref=ref * np.nan), dict(ref=ref * np.inf)):
            with pytest.raises(pkg.ThzError) as err:
                ok(**bad)
            assert err.value.code == -1, bad
        lib, cfg = engine.lib, pkg.UnmixCfg(2, 4, 0)
        full = [engine.ctx, 8, 16, dx, 16, 1, e.ctypes.data, None, ctypes.byref(cfg), da, None, None, None]
        assert lib.thz_unmix(*full) == 0
        for i in (6, 8):
            args = list(full)
            args[i] = None
            assert lib.thz_unmix(*args) == -1, i
        d.eng._check(lib.thz_memcpy_h2d(engine.ctx, da, np.full((2, 8), 5, np.float32).ctypes.data, 64))
        ok(npix=0)
        assert (d.get(da, (2, 8)) == 5).all()                             # nothing was written


# ---- the session ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _scan():
    out = cluster_model.planted_scan()
    out[1].setflags(write=False)
    return out


UNMIX_BUFS = (pkg.BUF_UNMIX_ABUNDANCE, pkg.BUF_UNMIX_PROJ, pkg.BUF_UNMIX_RESID, pkg.BUF_UNMIX_KKT)


def test_session_on_the_planted_scan(engine):
    time, cube, material = _scan()
    nx, ny, nt = cube.shape
    npix, nf = nx * ny, nt // 2 + 1
    first, count = cluster_model.band_bins(time)
    rng = np.random.default_rng(1)
    lib = engine.lib
    sess = pkg.Session(engine, nx, ny, time)
    try:
        sess.upload(cube, subtract_bias=False)
        picked = (np.abs(rng.standard_normal((3, count))) + 0.1).astype(np.float32)
        cfg = pkg.unmix_session_cfg(first, count, 1, 3, 64, endmembers=picked)
        for b in UNMIX_BUFS:                                               # absent until first asked for
            assert not lib.thz_session_buffer(sess.h, b)
            with pytest.raises(pkg.ThzError) as e:
                sess.download(b, npix=1)
            assert e.value.code == -4
        for which in (pkg.BUF_AMPLITUDES, pkg.BUF_PHASES, pkg.BUF_DATA):   # no recompute
            with pytest.raises(pkg.ThzError) as e:
                sess.unmix(which, cfg)
            assert e.value.code == -4, which
        for which in (pkg.BUF_FFT, pkg.BUF_IMG, pkg.BUF_PCA_SCORES, pkg.BUF_CLUSTER_CENTROIDS, 99):
            with pytest.raises(pkg.ThzError) as e:
                sess.unmix(which, cfg)
            assert e.value.code == -1, which
        chain = pkg.chain_cfg_default(time)
        sess.recompute(chain)
        with pytest.raises(pkg.ThzError) as e:                             # no segmentation: no centroids
            sess.unmix(pkg.BUF_AMPLITUDES, pkg.unmix_session_cfg(first, count, 1, 3, 64))
        assert e.value.code == -4
        ref = np.ones(count, np.float32)
        for bad in (pkg.unmix_session_cfg(first, 0, 1, 3, 64, endmembers=picked), pkg.unmix_session_cfg(first, 513, 1, 3, 64, endmembers=picked),
                    pkg.unmix_session_cfg(first, count, 0, 3, 64, endmembers=picked), pkg.unmix_session_cfg(nf - 1, 2, 1, 1, 64, endmembers=picked),
                    pkg.unmix_session_cfg(first, count, 1, 0, 64, endmembers=picked), pkg.unmix_session_cfg(first, count, 1, 17, 64, endmembers=picked),
                    pkg.unmix_session_cfg(first, count, 1, 3, -1, endmembers=picked), pkg.unmix_session_cfg(first, count, 1, 3, 4097, endmembers=picked),
                    pkg.unmix_session_cfg(first, count, 1, 3, 64, endmembers=picked, absorbance=True),
                    pkg.unmix_session_cfg(first, count, 1, 3, 64, endmembers=picked, ref=0 * ref),
                    pkg.unmix_session_cfg(first, count, 1, 3, 64, endmembers=0 * picked)):
            with pytest.raises(pkg.ThzError) as e:
                sess.unmix(pkg.BUF_AMPLITUDES, bad)
            assert e.value.code == -1
        assert not any(lib.thz_session_buffer(sess.h, b) for b in UNMIX_BUFS)
        amp = sess.download(pkg.BUF_AMPLITUDES).reshape(npix, nf)[:, first:first + count]
        a, b, resid, kkt = sess.unmix(pkg.BUF_AMPLITUDES, cfg)
        assert all(lib.thz_session_buffer(sess.h, b_) for b_ in UNMIX_BUFS)
        assert a.shape == (3, nx, ny) and resid.shape == (nx, ny)
        # download ranges over the flattened arrays, and nothing beyond them
        assert np.array_equal(_bits(sess.download(pkg.BUF_UNMIX_ABUNDANCE, pix0=npix + 5, npix=7)), _bits(a.reshape(3, npix)[1, 5:12]))
        for which, total in ((pkg.BUF_UNMIX_ABUNDANCE, 3 * npix), (pkg.BUF_UNMIX_PROJ, 3 * npix), (pkg.BUF_UNMIX_RESID, npix),
                             (pkg.BUF_UNMIX_KKT, npix)):
            sess.download(which, npix=total)
            with pytest.raises(pkg.ThzError) as e:
                sess.download(which, pix0=1, npix=total)
            assert e.value.code == -1
        # the hard labels, then their fractions: the resident centroids are the explicit ones
        out, label, dist2, cent = sess.cluster(pkg.BUF_AMPLITUDES, pkg.cluster_cfg(first, count, 1, 3))
        assert out.converged == 1 and cluster_model.same_partition(label, material.ravel())
        resident = sess.unmix(pkg.BUF_AMPLITUDES, pkg.unmix_session_cfg(first, count, 1, 3, 256))
        explicit = sess.unmix(pkg.BUF_AMPLITUDES, pkg.unmix_session_cfg(first, count, 1, 3, 256, endmembers=cent))
        for u, v in zip(resident, explicit):
            assert np.array_equal(_bits(u), _bits(v))
        for bad in (pkg.unmix_session_cfg(first, count, 1, 2, 256), pkg.unmix_session_cfg(first, count - 1, 1, 3, 256)):
            with pytest.raises(pkg.ThzError) as e:                         # the plane is not n_endmembers x count
                sess.unmix(pkg.BUF_AMPLITUDES, bad)
            assert e.value.code == -1
        assert all(lib.thz_session_buffer(sess.h, b_) for b_ in UNMIX_BUFS)   # a refused call leaves what was resident
        frac = explicit[0].reshape(3, npix).T
        clear = ~cluster_model.margin_is_within(cluster_model.distances(amp, cent), 0.05)
        print(f"planted scan: {int((~clear).sum())} of {npix} pixels left out; the smallest winning abundance {frac.max(axis=1).min():.3f}")
        assert (~clear).sum() <= npix // 20
        assert np.array_equal(frac.argmax(axis=1)[clear], label[clear])
        # every other bin, absorbance against the mean spectrum, the raw cube on the raw grid
        ok = (amp > 0).all(axis=0)                                         # the first run of bins the band pass leaves alone
        lo = int(np.argmax(ok))
        live = int(np.argmin(ok[lo:])) or count - lo
        top = amp.max(axis=0)[lo:lo + live:2] * np.float32(1.5)
        lines = (np.log(top.astype(np.float64))[None, :] - np.log(cent[:, lo:lo + live:2].astype(np.float64))).astype(np.float32)
        half = sess.unmix(pkg.BUF_AMPLITUDES, pkg.unmix_session_cfg(first + lo, lines.shape[1], 2, 3, 64, endmembers=lines, ref=top))
        assert half[0].shape == (3, nx, ny) and all(np.isfinite(p).all() for p in half) and live >= 16
        raw = sess.unmix(pkg.BUF_RAW, pkg.unmix_session_cfg(150, 100, 2, 2, 16, endmembers=np.abs(rng.standard_normal((2, 100))) + 0.1))
        assert raw[0].shape == (2, nx, ny)
        # the next recompute still leaves the right out-of-band zeros
        fresh = pkg.Session(engine, nx, ny, time)
        try:
            sess.recompute(chain)
            fresh.upload(cube, subtract_bias=False)
            fresh.recompute(chain)
            for which in (pkg.BUF_AMPLITUDES, pkg.BUF_FFT):
                assert np.array_equal(sess.download(which).view(np.uint32), fresh.download(which).view(np.uint32)), which
        finally:
            fresh.close()
        # the session call is the stage call on the session's own buffer
        a, b, resid, kkt = sess.unmix(pkg.BUF_AMPLITUDES, cfg)
        ptr = lib.thz_session_buffer(sess.h, pkg.BUF_AMPLITUDES)
        with Dev(engine) as d:
            da, db, dr, dk = d.new((3, npix)), d.new((3, npix)), d.new(npix), d.new(npix)
            engine.unmix(npix, count, ptr + 4 * first, nf, 1, picked, da, 64, proj=db, resid=dr, kkt=dk)
            assert np.array_equal(_bits(d.get(da, (3, nx, ny))), _bits(a)) and np.array_equal(_bits(d.get(db, (3, nx, ny))), _bits(b))
            assert np.array_equal(_bits(d.get(dr, (nx, ny))), _bits(resid)) and np.array_equal(_bits(d.get(dk, (nx, ny))), _bits(kkt))
        model_b, _ = model.project_exact(amp.astype(np.float64), picked)
        assert np.all(np.abs(b.reshape(3, npix).T - model_b) <= model.proj_bound(count) * (np.abs(amp.astype(np.float64)) @ picked.T.astype(np.float64)))
        # a new upload voids the maps
        sess.upload(cube, subtract_bias=False)
        assert not any(lib.thz_session_buffer(sess.h, b_) for b_ in UNMIX_BUFS)
    finally:
        sess.close()


@pytest.mark.parametrize("members", [2, 3])
def test_same_device_group_matches_one_session(engine, members):
    nx, ny, nt = 17, 12, 1001
    time, cube, material = cluster_model.planted_scan(nx, ny, nt, seed=members)
    first, count = cluster_model.band_bins(time)
    rng = np.random.default_rng(members)
    e = (np.abs(rng.standard_normal((4, count))) + 0.1).astype(np.float32)
    cfg = pkg.unmix_session_cfg(first, count, 1, 4, 64, endmembers=e)
    raw_cfg = pkg.unmix_session_cfg(20, 65, 3, 4, 64, endmembers=e[:, :65])
    chain = pkg.chain_cfg_default(time)
    sess = pkg.Session(engine, nx, ny, time)
    try:
        sess.upload(cube, subtract_bias=False)
        sess.recompute(chain)
        one, one_raw = sess.unmix(pkg.BUF_AMPLITUDES, cfg), sess.unmix(pkg.BUF_RAW, raw_cfg)
    finally:
        sess.close()
    with pkg.Group(devices=[0] * members) as g:
        gs = pkg.GroupSession(g, nx, ny, time)
        try:
            gs.upload(cube, subtract_bias=False)
            gs.recompute(chain)
            parts = [gs.member(i).unmix(pkg.BUF_AMPLITUDES, cfg) for i in range(members) if gs.member(i).nx]
            parts_raw = [gs.member(i).unmix(pkg.BUF_RAW, raw_cfg) for i in range(members) if gs.member(i).nx]
        finally:
            gs.close()
    for whole, slabs in ((one, parts), (one_raw, parts_raw)):
        assert sum(p[2].shape[0] for p in slabs) == nx
        for plane in range(4):                                             # (K, gx, gy) and (gx, gy): the slabs are rows of x
            stacked = np.concatenate([p[plane] for p in slabs], axis=-2)
            assert np.array_equal(_bits(stacked), _bits(whole[plane])), plane
