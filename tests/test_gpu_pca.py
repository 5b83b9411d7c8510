"""Principal components on the device (csrc/pca.hip, pca_api.cpp) against the numpy model of pca_model.py:
column sums, the Gram matrix on the f32 matrix instruction, the score images, the session form on the planted
two-material scan and same-device groups against one session.

With eps = 2^-24 and T = pkg.PCA_CHAIN (the products one f32 accumulator takes before it is added into f64):
- exact case   small integers, mu NULL, npix <= 4096: every product and every partial sum is an integer below 2^24, so
               the Gram matrix equals the int64 one bit for bit and is exactly symmetric.  A wrong lane map, a misplaced
               or a mirrored tile cannot hide: every column has its own scale, so no two tiles look alike.
- sums         |sum_j - want| <= (T + 2) eps sum_p |X_pj|   (the kernel adds in f64: far inside)
- Gram         |G_ij - want| <= (T + 2) eps sum_p |a_pi a_pj|, want the f64 Gram of the f32-subtracted values: the worst case
               of a T-long fmaf chain plus the f64 adds.
- scores       |S - want| <= (ceil(L / 64) + 8) eps sum_j |a_j v_j|: a lane's fmaf chain of at most ceil(L / 64) terms, six
               steps of the lane tree (DESIGN.md 4.7's S).
- components   sin(angle to the model's) <= (2 ||E||_F + r) / gap + 2^-23: Davis-Kahan with E the measured difference of
               the two covariances, r the host test's residual bar and gap the model's eigenvalue gap; 2^-23 for the f32
               rounding of both vectors.
- eigenvalues  |lambda - model's| <= ||E||_F + the host test's eigenvalue bar (Weyl).
Every test prints its largest error / bar."""
import functools
import math

import numpy as np
import pytest

import pca_model as model
import thz_image_explorer_amd as pkg
from test_gpu_helper_sizes import Dev

pytestmark = pytest.mark.gpu

EPS = model.EPS
T = pkg.PCA_CHAIN
LENGTHS = [1, 2, 31, 32, 33, 64, 65, 127, 128, 129, 240, 512]
PIXELS = [1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T + 3]
MASKS = ("none", "ones", "zeros", "random")


def _layouts(n):
    """(row_stride, col_step, byte offset): rows packed, one float apart and 2049 floats long; columns 1, 2 and 3 apart;
    the pointer on and 4 bytes off a 16-byte boundary.  Columns further apart than the stride reach into later rows:
    the matrix is a view, and the model reads the same view"""
    return [(n, 1, 0), (n + 1, 2, 4), (2049, 3, 0), (n, 3, 4), (2049, 1, 4), (n + 1, 1, 0)]


def _mask(kind, npix, rng):
    if kind == "none":
        return None
    if kind == "ones":
        return np.full(npix, 7, np.uint8)          # any non-zero byte keeps the pixel
    if kind == "zeros":
        return np.zeros(npix, np.uint8)
    return (rng.random(npix) < 0.6).astype(np.uint8)


def _flat(rng, npix, n, row_stride, col_step):
    size = (npix - 1) * row_stride + (n - 1) * col_step + 1
    return (rng.standard_normal(size) * np.exp(rng.uniform(-2, 2, size))).astype(np.float32)


def _ratio(err, bar):
    with np.errstate(all="ignore"):
        r = np.where(bar > 0, err / bar, np.where(err == 0, 0.0, np.inf))
    return float(np.max(r)) if r.size else 0.0


@pytest.mark.parametrize("n", [65, 129, 512])
def test_gram_of_small_integers_is_exact(engine, n):
    rng = np.random.default_rng(n)
    worst_sym = 0
    with Dev(engine) as d:
        for npix, row_stride, off, kind in ((4096, n, 0, "none"), (2 * T + 3, n + 1, 4, "random"), (T + 1, 2049, 4, "none")):
            scale = 1 + (np.arange(n) * 7 + np.arange(n) // 32) % 3                  # 1, 2, 3: a column's own scale
            sign = np.where((np.arange(n) // 5) % 2 == 0, 1, -1)                     # ... and sign pattern
            x = rng.integers(-8, 9, (npix, n)) * (scale * sign)[None, :]
            x[:, ::9] = np.abs(x[:, ::9])                                            # one-signed columns: large sums
            flat = np.zeros((npix - 1) * row_stride + n, np.float32)
            flat[(np.arange(npix)[:, None] * row_stride + np.arange(n)[None, :]).ravel()] = x.ravel()
            m = _mask(kind, npix, rng)
            keep = model.keep(npix, m)
            xi = x[keep].astype(np.int64)
            want = xi.T @ xi
            assert np.abs(xi).max() <= 24 and want.max() < 2 ** 24 * (npix // T + 1)
            got = engine.pca_gram(npix, n, d.put(flat, off), row_stride, 1, None if m is None else d.put(m))
            assert np.array_equal(got, got.T), (n, npix)
            bad = np.argwhere(got != want.astype(np.float64))
            assert bad.size == 0, (n, npix, row_stride, bad[:8], got[tuple(bad[0])], want[tuple(bad[0])])
            s, cnt = engine.pca_sums(npix, n, d.put(flat, off), row_stride, 1, None if m is None else d.put(m))
            assert cnt == int(keep.sum()) and np.array_equal(s, xi.sum(axis=0).astype(np.float64))
            worst_sym = max(worst_sym, int(np.abs(got - got.T).max()))
    assert worst_sym == 0


@pytest.mark.parametrize("n", LENGTHS)
def test_sums_and_gram_against_the_model(engine, n):
    rng = np.random.default_rng(1000 + n)
    worst_sum = worst_gram = 0.0
    layouts = _layouts(n)
    with Dev(engine) as d:
        case = 0
        for npix in PIXELS:
            for rep in range(2):
                row_stride, col_step, off = layouts[(case + rep * 3) % len(layouts)]
                kind = MASKS[(case + rep) % 4]
                with_mu = (case + rep) % 3 != 0
                case += 1
                flat = _flat(rng, npix, n, row_stride, col_step)
                x = model.view(flat, npix, n, row_stride, col_step)
                m = _mask(kind, npix, rng)
                dx, dm = d.put(flat, off), None if m is None else d.put(m)
                tag = (n, npix, row_stride, col_step, off, kind, with_mu)
                want_sum, abs_sum, want_cnt = model.sums(x, m)
                got_sum, got_cnt = engine.pca_sums(npix, n, dx, row_stride, col_step, dm)
                assert got_cnt == want_cnt, tag
                err = np.abs(got_sum - want_sum)
                assert np.all(err <= (T + 2) * EPS * abs_sum), (tag, err.max())
                worst_sum = max(worst_sum, _ratio(err, (T + 2) * EPS * abs_sum))
                mu = None
                if with_mu:                                              # the mean where there is one, any vector otherwise
                    mu = model.mean_of(want_sum, want_cnt) if want_cnt else rng.standard_normal(n).astype(np.float32)
                want, abs_g = model.gram(model.centred(x, mu, m))
                got = engine.pca_gram(npix, n, dx, row_stride, col_step, dm, mu)
                assert got.shape == (n, n) and np.array_equal(got, got.T), tag
                err = np.abs(got - want)
                bar = (T + 2) * EPS * abs_g
                assert np.all(err <= bar), (tag, np.argwhere(err > bar)[:8], err.max())
                worst_gram = max(worst_gram, _ratio(err, bar))
                if kind == "zeros":
                    assert got_cnt == 0 and not got.any() and not got_sum.any(), tag
                again = engine.pca_gram(npix, n, dx, row_stride, col_step, dm, mu)
                assert np.array_equal(got.view(np.uint64), again.view(np.uint64)), tag
    print(f"L = {n}: largest error / bar, sums {worst_sum:.3g}, Gram {worst_gram:.3g}")


def test_nan_propagates_along_its_row_and_column_only(engine):
    n, npix, j0, p0 = 129, 2 * T + 3, 70, T + 5
    rng = np.random.default_rng(8)
    x = rng.standard_normal((npix, n)).astype(np.float32)
    clean = model.gram(x)[0]
    x[p0, j0] = np.nan
    with Dev(engine) as d:
        got = engine.pca_gram(npix, n, d.put(x), n)
        hit = np.zeros((n, n), bool)
        hit[j0, :] = hit[:, j0] = True
        assert np.isnan(got[hit]).all() and np.isfinite(got[~hit]).all()
        bar = (T + 2) * EPS * model.gram(np.nan_to_num(x))[1]
        assert np.all(np.abs(got - clean)[~hit] <= bar[~hit])
        s, cnt = engine.pca_sums(npix, n, d.put(x), n)
        assert cnt == npix and np.isnan(s[j0]) and np.isfinite(np.delete(s, j0)).all()
        # the same pixel masked out: its NaN is not part of anything
        m = np.ones(npix, np.uint8)
        m[p0] = 0
        got = engine.pca_gram(npix, n, d.put(x), n, 1, d.put(m))
        s, cnt = engine.pca_sums(npix, n, d.put(x), n, 1, d.put(m))
        assert np.isfinite(got).all() and np.isfinite(s).all() and cnt == npix - 1
        # Inf propagates too: Inf on the diagonal, Inf or NaN along the row
        x[p0, j0] = np.inf
        got = engine.pca_gram(npix, n, d.put(x), n)
        assert got[j0, j0] == np.inf and not np.isfinite(got[j0]).any() and np.isfinite(got[~hit]).all()


def test_refusals_and_empty_input(engine):
    x = np.ones((8, 16), np.float32)
    with Dev(engine) as d:
        dx, ds = d.put(x), d.new(8 * 8)
        v = np.eye(2, 16, dtype=np.float32)
        for bad in (lambda: engine.pca_sums(8, 0, dx, 16), lambda: engine.pca_sums(8, 513, dx, 16), lambda: engine.pca_sums(8, 16, dx, 16, 0),
                    lambda: engine.pca_sums(8, 16, None, 16), lambda: engine.pca_gram(8, 0, dx, 16), lambda: engine.pca_gram(8, 513, dx, 16),
                    lambda: engine.pca_gram(8, 16, dx, 16, 0), lambda: engine.pca_gram(8, 16, None, 16),
                    lambda: engine.pca_scores(8, 0, dx, 16, 1, None, v, ds), lambda: engine.pca_scores(8, 513, dx, 16, 1, None, v, ds),
                    lambda: engine.pca_scores(8, 16, dx, 16, 0, None, v, ds), lambda: engine.pca_scores(8, 16, None, 16, 1, None, v, ds),
                    lambda: engine.pca_scores(8, 16, dx, 16, 1, None, v, None),
                    lambda: engine.pca_scores(8, 16, dx, 16, 1, None, np.zeros((9, 16), np.float32), ds)):
            with pytest.raises(pkg.ThzError) as e:
                bad()
            assert e.value.code == -1
        lib = engine.lib
        assert lib.thz_pca_sums(engine.ctx, 8, 16, dx, 16, 1, None, None, None) == -1
        assert lib.thz_pca_gram(engine.ctx, 8, 16, dx, 16, 1, None, None, None) == -1
        assert lib.thz_pca_scores(engine.ctx, 8, 16, dx, 16, 1, None, None, 2, ds) == -1
        s, cnt = engine.pca_sums(0, 16, dx, 16)
        assert cnt == 0 and not s.any() and not engine.pca_gram(0, 16, dx, 16).any()
        engine.pca_scores(0, 16, dx, 16, 1, None, v, ds)
        assert np.isnan(d.get(ds, 64)).all()                              # nothing was written


def _asymmetric_components(rng, k, n):
    """not orthonormal, every entry different: a component <-> column swap, or a transposed table, shows"""
    return (rng.standard_normal((k, n)) * (1.0 + np.arange(k)[:, None]) + 0.01 * np.arange(n)[None, :]).astype(np.float32)


@pytest.mark.parametrize("n", [1, 2, 33, 64, 65, 129, 240, 512])
def test_scores_against_the_model(engine, n):
    rng = np.random.default_rng(2000 + n)
    worst = 0.0
    layouts = _layouts(n)
    with Dev(engine) as d:
        for case, npix in enumerate((1, 65, T + 1)):
            row_stride, col_step, off = layouts[case % len(layouts)]
            flat = _flat(rng, npix, n, row_stride, col_step)
            x = model.view(flat, npix, n, row_stride, col_step)
            dx = d.put(flat, off)
            mu = model.mean_of(*model.sums(x)[::2])
            k = min(n, pkg.PCA_MAX_COMPONENTS)
            own = model.pca(x, k)["components"] if npix > 1 else np.eye(k, n, dtype=np.float32)
            for comps, use_mu in ((own, True), (_asymmetric_components(rng, min(3, n), n), True), (_asymmetric_components(rng, 1, n), False)):
                kk = comps.shape[0]
                ds = d.new(kk * npix)
                engine.pca_scores(npix, n, dx, row_stride, col_step, mu if use_mu else None, comps, ds)
                got = d.get(ds, (kk, npix))
                want, abs_s = model.scores(model.centred(x, mu if use_mu else None), comps)
                bar = (math.ceil(n / 64) + 8) * EPS * abs_s
                err = np.abs(got - want)
                assert np.all(err <= bar), ((n, npix, kk, use_mu), np.argwhere(err > bar)[:8], err.max())
                worst = max(worst, _ratio(err, bar))
                ds2 = d.new(kk * npix)
                engine.pca_scores(npix, n, dx, row_stride, col_step, mu if use_mu else None, comps, ds2)
                assert np.array_equal(got.view(np.uint32), d.get(ds2, (kk, npix)).view(np.uint32))
    print(f"L = {n}: scores, largest error / bar {worst:.3g}")


def test_more_pixels_than_one_grid_pass_and_stage_time(engine):
    """2048 blocks x 4 waves cover 8192 pixels: the 9001 here take a second trip of the score kernel's pixel loop, and
    nine chunks of the Gram kernel"""
    npix, n = 9001, 64
    rng = np.random.default_rng(3)
    x = rng.standard_normal((npix, n)).astype(np.float32)
    comps = _asymmetric_components(rng, 2, n)
    with Dev(engine) as d:
        dx, ds = d.put(x), d.new(2 * npix)
        engine.enable_timing(1)
        try:
            got_g = engine.pca_gram(npix, n, dx, n)
            assert engine.stage_time_ns(pkg.STAGE_PCA) > 0
            engine.pca_scores(npix, n, dx, n, 1, None, comps, ds)
            assert engine.stage_time_ns(pkg.STAGE_PCA) > 0
        finally:
            engine.enable_timing(0)
        want, abs_s = model.scores(x, comps)
        assert np.all(np.abs(d.get(ds, (2, npix)) - want) <= (1 + 8) * EPS * abs_s)
        want_g, abs_g = model.gram(x)
        assert np.all(np.abs(got_g - want_g) <= (T + 2) * EPS * abs_g)


# ---- the session ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _scan():
    out = model.planted_scan()
    out[1].setflags(write=False)
    return out


def _compare_with_model(x, got, k, mask, tag, gram_dev):
    """got = (eigenvalues, total variance, count, scores (k, npix), components (k, L), mean (L)) against the model run
    on the matrix x (the session's own downloaded values); gram_dev: the session's Gram matrix for got's mean (the call
    is deterministic: the bits thz_session_pca took its eigenvectors of)"""
    ev, tot, cnt, sc, comp, mean = got
    n = x.shape[1]
    total, abs_sum, want_cnt = model.sums(x, mask)
    assert cnt == want_cnt, tag
    want = model.pca(x, k, mask=mask)
    # the mean: (float)(sum / count) of a sum inside its bar
    mean_bar = (T + 2) * EPS * abs_sum / cnt + EPS * np.abs(want["mu"])
    assert np.all(np.abs(mean.astype(np.float64) - total / cnt) <= mean_bar), tag
    # the covariance the device's eigenvalues belong to: its Gram bar, taken with the device's own mean
    a = model.centred(x, mean, mask)
    g, abs_g = model.gram(a)
    g_err, g_bar = np.abs(gram_dev - g), (T + 2) * EPS * abs_g
    assert np.all(g_err <= g_bar), (tag, g_err.max())
    e_fro = float(np.sqrt((((gram_dev / (cnt - 1) - want["cov"]) ** 2).sum())))     # the measured difference
    fro = float(np.sqrt((want["cov"] ** 2).sum()))
    w = want["all_eigenvalues"]
    ev_bar = e_fro + 8 * n * 2.0 ** -52 * fro
    assert np.all(np.abs(ev - want["eigenvalues"]) <= ev_bar), (tag, ev, want["eigenvalues"], ev_bar)
    assert abs(tot - want["total_variance"]) <= math.sqrt(n) * e_fro + n * 2.0 ** -52 * fro, tag
    r_bar = 4 * model.residual(want["cov"], want["eigenvalues"], want["components"]) + model.residual_floor(want["cov"])
    worst_angle = 0.0
    for i in range(k):
        gap = min(w[i - 1] - w[i] if i else np.inf, w[i] - w[i + 1])
        assert gap > 0, (tag, i)
        bound = (2 * e_fro + r_bar) / gap + 2.0 ** -23
        v, u = comp[i].astype(np.float64), want["vectors"][i]
        cos = abs(float(v @ u)) / math.sqrt(float(v @ v) * float(u @ u))
        sin = math.sqrt(max(0.0, 1.0 - min(cos, 1.0) ** 2))
        assert sin <= bound, (tag, i, sin, bound)
        worst_angle = max(worst_angle, sin / bound)
    # the scores: the device's own components and mean, against the f64 sums of the same f32 values
    s_want, abs_s = model.scores(model.centred(x, mean), comp)
    bar = (math.ceil(n / 64) + 8) * EPS * abs_s
    err = np.abs(sc.reshape(k, -1) - s_want)
    assert np.all(err <= bar), (tag, err.max())
    print(f"{tag}: Gram error / bar {_ratio(g_err, g_bar):.3g}; eigenvalues {ev}, error / bar {_ratio(np.abs(ev - want['eigenvalues']), np.full(k, ev_bar)):.3g}; "
          f"angle / bound {worst_angle:.3g}; scores {_ratio(err, bar):.3g}")
    return want


def test_session_on_the_planted_scan(engine):
    time, cube, a1, a2 = _scan()
    nx, ny, nt = cube.shape
    npix = nx * ny
    first, count = model.band_bins(time)
    cfg = pkg.pca_cfg(first, count, 1, 3)
    bufs = (pkg.BUF_PCA_SCORES, pkg.BUF_PCA_COMPONENTS, pkg.BUF_PCA_MEAN)
    lib = engine.lib
    sess = pkg.Session(engine, nx, ny, time)
    fresh = pkg.Session(engine, nx, ny, time)
    try:
        sess.upload(cube, subtract_bias=False)
        for b in bufs:                                                     # absent until first asked for
            assert not lib.thz_session_buffer(sess.h, b)
            with pytest.raises(pkg.ThzError) as e:
                sess.download(b, npix=1)
            assert e.value.code == -4
        for which in (pkg.BUF_AMPLITUDES, pkg.BUF_PHASES, pkg.BUF_DATA):   # no recompute has run
            with pytest.raises(pkg.ThzError) as e:
                sess.pca(which, cfg)
            assert e.value.code == -4
        for which in (pkg.BUF_FFT, pkg.BUF_IMG, pkg.BUF_AVG_AMPLITUDES, 99):
            with pytest.raises(pkg.ThzError) as e:
                sess.pca(which, cfg)
            assert e.value.code == -1
        chain = pkg.chain_cfg_default(time)
        sess.recompute(chain)
        nf = nt // 2 + 1
        for bad in (pkg.pca_cfg(first, 0, 1, 3), pkg.pca_cfg(first, 513, 1, 3), pkg.pca_cfg(first, count, 0, 3),
                    pkg.pca_cfg(nf - 1, 2, 1, 1), pkg.pca_cfg(1, 251, 2, 3), pkg.pca_cfg(first, count, 1, 0),
                    pkg.pca_cfg(first, count, 1, 9), pkg.pca_cfg(first, 2, 1, 3)):
            with pytest.raises(pkg.ThzError) as e:
                sess.pca(pkg.BUF_AMPLITUDES, bad)
            assert e.value.code == -1
        assert not any(lib.thz_session_buffer(sess.h, b) for b in bufs)
        amp = sess.download(pkg.BUF_AMPLITUDES).reshape(npix, nf)
        got = sess.pca(pkg.BUF_AMPLITUDES, cfg)
        assert all(lib.thz_session_buffer(sess.h, b) for b in bufs)
        want = _compare_with_model(amp[:, first:first + count], got, 3, None, "amplitudes 0.2 .. 5 THz",
                                   sess.pca_gram(pkg.BUF_AMPLITUDES, cfg, got[5]))
        w = want["all_eigenvalues"]
        assert w[0] - w[1] > 0.1 * w[0] and w[1] - w[2] > 0.1 * w[0]       # the planted directions stand apart
        sc = got[3]
        r1, r2 = model.explained(a1, sc[:2]), model.explained(a2, sc[:2])
        print(f"device score images: R^2 {r1:.5f} and {r2:.5f} of the abundance maps")
        # flattened download ranges, and nothing beyond them
        assert np.array_equal(sess.download(pkg.BUF_PCA_SCORES, pix0=npix + 3, npix=5).view(np.uint32), sc[1].ravel()[3:8].view(np.uint32))
        assert np.array_equal(sess.download(pkg.BUF_PCA_COMPONENTS, pix0=count + 2, npix=4).view(np.uint32), got[4][1, 2:6].view(np.uint32))
        assert np.array_equal(sess.download(pkg.BUF_PCA_MEAN, pix0=7, npix=3).view(np.uint32), got[5][7:10].view(np.uint32))
        for which, total in ((pkg.BUF_PCA_SCORES, 3 * npix), (pkg.BUF_PCA_COMPONENTS, 3 * count), (pkg.BUF_PCA_MEAN, count)):
            sess.download(which, npix=total)
            with pytest.raises(pkg.ThzError) as e:
                sess.download(which, pix0=1, npix=total)
            assert e.value.code == -1
        # the next recompute still leaves the right out-of-band zeros: everything as in a session that never ran this
        sess.recompute(chain)
        fresh.upload(cube, subtract_bias=False)
        fresh.recompute(chain)
        for which in (pkg.BUF_AMPLITUDES, pkg.BUF_FFT, pkg.BUF_PHASES, pkg.BUF_DATA):
            assert np.array_equal(sess.download(which).view(np.uint32), fresh.download(which).view(np.uint32)), which
        # a mask, every other bin, not centred: the mean buffer holds zeros
        rng = np.random.default_rng(4)
        m = (rng.random(npix) < 0.7).astype(np.uint8)
        with Dev(engine) as d:
            cfg2 = pkg.pca_cfg(first, count // 2, 2, 2, center=True, mask=d.put(m))
            got = sess.pca(pkg.BUF_AMPLITUDES, cfg2)
            assert got[2] == int(m.sum()) and got[3].shape == (2, nx, ny)
            _compare_with_model(amp[:, first:first + count:2][:, :count // 2], got, 2, m, "masked, every other bin",
                                sess.pca_gram(pkg.BUF_AMPLITUDES, cfg2, got[5]))
            cfg3 = pkg.pca_cfg(first, 33, 3, 2, center=False, mask=d.put(m))
            ev, tot, cnt, sc, comp, mean = sess.pca(pkg.BUF_AMPLITUDES, cfg3)
            assert not mean.any() and cnt == int(m.sum())
            x = amp[:, first:first + 99:3]
            g, abs_g = model.gram(model.centred(x, None, m))
            mo = model.components(g, cnt, 2)
            assert np.all(np.abs(ev - mo["eigenvalues"]) <= np.sqrt((((T + 2) * EPS * abs_g / (cnt - 1)) ** 2).sum()) + 8 * 33 * 2.0 ** -52 * np.sqrt((mo["cov"] ** 2).sum()))
            s_want, abs_s = model.scores(x, comp)
            assert np.all(np.abs(sc.reshape(2, -1) - s_want) <= (1 + 8) * EPS * abs_s)
        # the other sources: phases and final traces on the recompute's grid, the raw cube on the raw grid
        data = sess.download(pkg.BUF_DATA).reshape(npix, nt)
        cfg4, cfg5 = pkg.pca_cfg(150, 200, 1, 2), pkg.pca_cfg(150, 100, 2, 2)
        got = sess.pca(pkg.BUF_DATA, cfg4)
        _compare_with_model(data[:, 150:350], got, 2, None, "final traces", sess.pca_gram(pkg.BUF_DATA, cfg4, got[5]))
        got = sess.pca(pkg.BUF_RAW, cfg5)
        _compare_with_model(cube.reshape(npix, nt)[:, 150:350:2], got, 2, None, "raw traces", sess.pca_gram(pkg.BUF_RAW, cfg5, got[5]))
        ph = sess.download(pkg.BUF_PHASES).reshape(npix, nf)
        s, cnt = sess.pca_sums(pkg.BUF_PHASES, pkg.pca_cfg(first, 40, 1, 1))
        want_s, abs_s, _ = model.sums(ph[:, first:first + 40])
        assert cnt == npix and np.all(np.abs(s - want_s) <= (T + 2) * EPS * abs_s)
        # behind a scaling stage the matrix has the block grid's pixels
        chain.scale_factor = 2
        sess.recompute(chain)
        gx, gy = sess.grid()[:2]
        assert (gx, gy) == (nx // 2, ny // 2)
        amp2 = sess.download(pkg.BUF_AMPLITUDES).reshape(gx * gy, -1)
        got = sess.pca(pkg.BUF_AMPLITUDES, cfg)
        assert got[3].shape == (3, gx, gy) and got[2] == gx * gy
        _compare_with_model(amp2[:, first:first + count], got, 3, None, "scale_factor 2", sess.pca_gram(pkg.BUF_AMPLITUDES, cfg, got[5]))
        with pytest.raises(pkg.ThzError) as e:
            sess.download(pkg.BUF_PCA_SCORES, npix=3 * gx * gy + 1)
        assert e.value.code == -1
        assert sess.pca(pkg.BUF_RAW, cfg)[3].shape == (3, nx, ny)          # the raw grid again
        sess.upload(cube, subtract_bias=False)                             # a new upload voids the buffers
        assert not any(lib.thz_session_buffer(sess.h, b) for b in bufs)
    finally:
        sess.close()
        fresh.close()


@pytest.mark.parametrize("members", [2, 3])
def test_same_device_group_matches_one_session(engine, members):
    """what GpuEngine::pca does, over the members of a same-device group: sums and Gram matrices per member, added on the
    host in member order, the components once, the projection per member"""
    nx, ny, nt = 17, 12, 1001
    time, cube, _, _ = model.planted_scan(nx, ny, nt, seed=members)
    first, count = model.band_bins(time)
    k = 3
    rng = np.random.default_rng(members)
    mask = (rng.random((nx, ny)) < 0.8).astype(np.uint8)
    chain = pkg.chain_cfg_default(time)
    with Dev(engine) as d:
        sess = pkg.Session(engine, nx, ny, time)
        try:
            sess.upload(cube, subtract_bias=False)
            sess.recompute(chain)
            one = sess.pca(pkg.BUF_AMPLITUDES, pkg.pca_cfg(first, count, 1, k, mask=d.put(mask)))
            amp = sess.download(pkg.BUF_AMPLITUDES).reshape(nx * ny, -1)[:, first:first + count]
        finally:
            sess.close()
        with pkg.Group(devices=[0] * members) as g:
            gs = pkg.GroupSession(g, nx, ny, time)
            try:
                gs.upload(cube, subtract_bias=False)
                gs.recompute(chain)
                total, cnt, cfgs, x0 = np.zeros(count), 0, [], 0
                for i in range(members):
                    m = gs.member(i)
                    rows = m.grid()[0]
                    cfgs.append(pkg.pca_cfg(first, count, 1, k, mask=d.put(mask[x0:x0 + rows])))
                    x0 += rows
                    s, c = m.pca_sums(pkg.BUF_AMPLITUDES, cfgs[i])
                    total += s
                    cnt += c
                assert x0 == nx and cnt == one[2] == int(mask.sum())       # counts and masks: bit for bit
                mu = (total / cnt).astype(np.float32)
                assert np.all(np.abs(mu - one[5]) <= 2.0 ** -23 * np.abs(mu))      # f64 sums in another order: an ulp at the most
                gram = np.zeros((count, count))
                for i in range(members):
                    gram += gs.member(i).pca_gram(pkg.BUF_AMPLITUDES, cfgs[i], mu)
                rc, comp, ev, tot = pkg.host_pca_components(gram, cnt, k)
                assert rc == 0
                scores = np.concatenate([gs.member(i).pca_project(pkg.BUF_AMPLITUDES, cfgs[i], mu, comp) for i in range(members)], axis=1)
            finally:
                gs.close()
    # the two Gram matrices are both within the bar of the exact one: eigenvalues within twice the bar's norm
    a = model.centred(amp, mu, mask.ravel())
    g_want, abs_g = model.gram(a)
    assert np.all(np.abs(gram - g_want) <= (T + 2) * EPS * abs_g)
    e_fro = float(np.sqrt((((T + 2) * EPS * abs_g / (cnt - 1)) ** 2).sum()))
    fro = float(np.sqrt(((g_want / (cnt - 1)) ** 2).sum()))
    assert np.all(np.abs(ev - one[0]) <= 2 * e_fro + 8 * count * 2.0 ** -52 * fro), (ev, one[0])
    assert abs(tot - one[1]) <= 2 * math.sqrt(count) * e_fro + count * 2.0 ** -52 * fro
    # scores: each side within its bar of the f64 scores of its own components and mean
    bars = []
    for sc, v, m in ((scores, comp, mu), (one[3], one[4], one[5])):
        s_want, abs_s = model.scores(model.centred(amp, m), v)
        bars.append((math.ceil(count / 64) + 8) * EPS * abs_s)
        assert np.all(np.abs(sc.reshape(k, -1) - s_want) <= bars[-1])
    # ... and the two sides against each other: components within the Davis-Kahan bound of the two Gram bars (both
    # matrices lie within the bar of the exact one), scores within |a_p| |v - u| <= 2 |a_p| sin(angle) plus both bars
    w = model.components(g_want, cnt, k)["all_eigenvalues"]
    norms = np.sqrt((model.centred(amp, mu).astype(np.float64) ** 2).sum(axis=1))
    for i in range(k):
        gap = min(w[i - 1] - w[i] if i else np.inf, w[i] - w[i + 1])
        bound = 2 * (2 * e_fro) / gap + 2.0 ** -22
        v, u = comp[i].astype(np.float64), one[4][i].astype(np.float64)
        cos = abs(float(v @ u)) / math.sqrt(float(v @ v) * float(u @ u))
        assert math.sqrt(max(0.0, 1.0 - min(cos, 1.0) ** 2)) <= bound, i
        if bound < 0.5:
            assert float(v @ u) > 0                                         # the sign rule gives both sides one sign
            diff = np.abs(scores[i].ravel().astype(np.float64) - one[3][i].ravel())
            assert np.all(diff <= 2 * norms * bound + bars[0][i] + bars[1][i] + 2.0 ** -22 * norms), (i, diff.max())
