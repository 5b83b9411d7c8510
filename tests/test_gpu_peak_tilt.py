"""Pulse arrival times and the tilt they imply, on the device (csrc/peak.hip, peak_api.cpp, group_tilt.cpp): the
per-trace peak against a numpy fp64 model at the lengths where the kernel's loops change shape, the arrival-plane
moments and fit against np.linalg.lstsq on the GPU's own maps, planted tilts through a session and back through the
Tilt Compensation stage, same-device groups against one session, and the session's bookkeeping of the three maps.

Bars (peak_tilt_model.py holds the model):
- index and value: bit for bit.
- offset: within 8 eps_f32 (|y-| + 2 |y0| + |y+|) / |y- - 2 y0 + y+| of the fp64 parabola — the rounding of the f32
  formula itself (three additions, a product, a quotient, each half an ulp of terms that size) — and exactly 0 where the
  definition says so.
- slopes of the fit: 1e-9 of max(|slope|, rms / half-width); t0: 1e-9 of max(|t0|, rms).  At least four orders above the
  f64 rounding of the sums, far below any indexing or weighting error.
- planted tilts: the estimate's error as delay at the grid's edge < 0.1 sample (the model alone: <= 0.03); after a
  recompute with the estimated angles the residual edge delay < 1 sample (the floor of the reference's integer shift)
  and the spread of the peak index over the participating pixels <= 4.  The chain between the raw cube and
  THZ_BUF_DATA is the default one (windows, 0.2 - 5 THz band pass): through the CPU oracle it leaves <= 0.08 sample and
  a spread of 2 on these cubes."""
import numpy as np
import pytest

import peak_tilt_model as model
import thz_image_explorer_amd as pkg
from thz_image_explorer_amd.binding import STAGE_PEAK
from test_gpu_helper_sizes import Dev

pytestmark = pytest.mark.gpu

NX, NY = 17, 19          # 323 traces: odd, no multiple of the four waves of a block
PEAK_NT = [1, 2, 63, 64, 200, 1001, 1024, 1027, 4099]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _peak_cube(nt, seed):
    """noise + the traces the definition's corner cases need -> (npix, nt) f32"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((NX * NY, nt)).astype(np.float32)
    tail0 = nt & ~3
    x[0, 0] = 60.0                                   # the peak at index 0 ...
    x[1, nt - 1] = 60.0                              # ... at nt - 1 ...
    x[2, tail0 if tail0 < nt else nt - 1] = -60.0    # ... in the nt % 4 tail (a minimum: modes 0 and 2)
    x[3, nt - 1 if nt % 4 == 0 else tail0] = 60.0
    # equal maxima: the lowest index wins, whichever lane holds it (253 is lane 63's, 256 lane 0's second quad)
    ties = sorted({int(f * (nt - 1)) for f in (0.26, 0.5, 0.77)} | ({253, 256} if nt > 256 else set()))
    x[4, ties] = 50.0
    x[5, ties] = -50.0
    x[6, ties[:len(ties) // 2 + 1]] = 50.0           # |x| ties between +50 and -50
    x[6, ties[len(ties) // 2 + 1:]] = -50.0
    x[7] = -np.abs(x[7]) - 1.0                       # all negative
    x[8, rng.random(nt) < 0.3] = np.nan              # NaNs among the samples
    x[9] = np.nan                                    # nothing but NaNs: index 0
    x[10] = 2.5                                      # constant: every sample ties, the parabola has no vertex
    if nt > 4:
        x[11, nt // 2] = 70.0                        # a NaN next to the winner: offset 0
        x[11, nt // 2 + 1] = np.nan
        x[12, nt // 3] = np.inf                      # an infinite winner: offset 0
        x[13] = -np.inf                              # a NaN in front of a row of -Inf: the first NUMBER wins
        x[13, 0] = np.nan
        x[14, [1, nt - 2]] = 80.0                    # winners one sample inside the ends do have neighbours
        x[15, nt // 2] = 0.0                         # +0 and -0 are one value: the lower index wins
        x[15, nt // 2 - 1] = -0.0
        x[15, np.arange(nt) < nt // 2 - 1] = -1.0
        x[15, np.arange(nt) > nt // 2] = -2.0
    return x


@pytest.mark.parametrize("nt", PEAK_NT)
def test_peak_map(engine, nt):
    npix = NX * NY
    x = _peak_cube(nt, nt)
    want = {mode: model.peak_model(x, mode) for mode in (0, 1, 2)}
    with Dev(engine) as d:
        for off in (0, 4):                           # ... and a cube that starts 4 bytes behind a 16-byte boundary
            dx = d.put(x, off)
            for mode in (0, 1, 2):
                di, do, dv = d.new(npix, dtype=np.int32), d.new(npix), d.new(npix)
                engine.peak_map(npix, nt, dx, mode, di, do, dv)
                idx, offs, val = d.get(di, npix, np.int32), d.get(do, npix), d.get(dv, npix)
                k, off64, value, bar, ok = want[mode]
                tag = (nt, mode, off)
                assert np.array_equal(idx, k), (tag, np.flatnonzero(idx != k)[:8])
                assert np.array_equal(_bits(val), _bits(value)), tag
                assert np.all(offs[~ok] == 0.0) and not np.signbit(offs[~ok]).any(), tag
                assert np.all(np.abs(offs) <= 0.5), tag
                err = np.abs(offs.astype(np.float64) - off64)
                print(f"peak_map nt={nt} mode={mode} +{off}B: offset error {err.max():.3e}, largest error / bar {np.max(err[ok] / bar[ok]) if ok.any() else 0:.3f}")
                assert np.all(err <= bar), (tag, np.flatnonzero(err > bar)[:8])
        # any output may be left out; nothing at all is a no-op
        di = d.new(npix, dtype=np.int32)
        engine.peak_map(npix, nt, dx, 1, di, None, None)
        assert np.array_equal(d.get(di, npix, np.int32), want[1][0])
        dv = d.new(npix)
        engine.peak_map(npix, nt, dx, 2, None, None, dv)
        assert np.array_equal(_bits(d.get(dv, npix)), _bits(want[2][2]))
        engine.peak_map(npix, nt, dx, 0, None, None, None)
        for bad in (-1, 3):
            with pytest.raises(pkg.ThzError) as e:
                engine.peak_map(npix, nt, dx, bad, di, None, None)
            assert e.value.code == -1


def test_peak_map_more_traces_than_one_grid_pass_and_stage_time(engine):
    """2048 blocks x 4 waves cover 8192 traces: the 8300 here take a second trip of the trace loop"""
    npix, nt = 8300, 37
    x = np.random.default_rng(3).standard_normal((npix, nt)).astype(np.float32)
    k, off64, value, bar, ok = model.peak_model(x, 0)
    with Dev(engine) as d:
        di, do, dv = d.new(npix, dtype=np.int32), d.new(npix), d.new(npix)
        engine.enable_timing(1)
        try:
            engine.peak_map(npix, nt, d.put(x), 0, di, do, dv)
            assert engine.stage_time_ns(STAGE_PEAK) > 0
        finally:
            engine.enable_timing(0)
        assert np.array_equal(d.get(di, npix, np.int32), k)
        assert np.array_equal(_bits(d.get(dv, npix)), _bits(value))
        assert np.all(np.abs(d.get(do, npix).astype(np.float64) - off64) <= bar)


def _check_fit(fit, want):
    assert fit.n_used == want["n_used"]
    for name in ("slope_x_ps_per_mm", "slope_y_ps_per_mm"):
        tol = 1e-9 * max(abs(want[name]), want["rms_ps"] / want["half_width"])
        assert abs(getattr(fit, name) - want[name]) <= tol, (name, getattr(fit, name), want[name])
    assert abs(fit.t0_ps - want["t0_ps"]) <= 1e-9 * max(abs(want["t0_ps"]), want["rms_ps"])
    assert abs(fit.rms_ps - want["rms_ps"]) <= 1e-6 * want["rms_ps"]
    assert fit.tilt_x_deg == pytest.approx(want["tilt_x_deg"], rel=1e-8, abs=1e-12)
    assert fit.tilt_y_deg == pytest.approx(want["tilt_y_deg"], rel=1e-8, abs=1e-12)


def test_moments_and_fit_on_the_gpus_own_maps(engine):
    nt, dx, dy, r = 200, 0.5, 0.25, 0.25
    time, cube, _, _, live = model.planted_cube(NX, NY, nt, dx, dy, 2.0, 1.0, dead=0.2, seed=4)
    cube[3, 5] = np.nan                                  # a pixel whose value is no number takes no part
    cube[4, 7, 17] = np.inf                              # ... nor one whose value is infinite, and neither sets vmax
    dt = model.mean_step(time)
    npix = NX * NY
    with Dev(engine) as d:
        di, do, dv = d.new(npix, dtype=np.int32), d.new(npix), d.new(npix)
        engine.peak_map(npix, nt, d.put(cube.reshape(npix, nt)), 1, di, do, dv)
        idx, off, val = (d.get(p, npix, t).reshape(NX, NY) for p, t in ((di, np.int32), (do, np.float32), (dv, np.float32)))
        m1 = engine.arrival_plane_moments(NX, NY, dx, dy, dt, di, do, dv, r)
        m2 = engine.arrival_plane_moments(NX, NY, dx, dy, dt, di, do, dv, r)
    assert np.array_equal(m1.view(np.uint64), m2.view(np.uint64))          # two runs: the same bits
    want_m = model.plane_moments(idx, off, val, dx, dy, dt, r)
    assert m1[0] == want_m[0] == (live & np.isfinite(val)).sum()
    assert np.allclose(m1, want_m, rtol=1e-12, atol=1e-9)
    rc, fit = pkg.host_arrival_plane_fit(m1)
    assert rc == 0
    _check_fit(fit, model.plane_lstsq(idx, off, val, dx, dy, dt, r))


def test_moments_of_more_pixels_than_the_launch_has_threads(engine):
    """64 x 256 threads: the 150 x 120 pixels here give every thread a second pixel; uploaded maps, no cube"""
    nx, ny, dx, dy, dt, r = 150, 120, 0.3, 0.7, 0.05, 0.5
    rng = np.random.default_rng(8)
    U, V = model.plane_coords(nx, ny, dx, dy)
    tau = 400.0 + 2.0 * U - 1.5 * V + rng.standard_normal((nx, ny))
    idx = np.floor(tau + 0.5).astype(np.int32)
    off = (tau - idx).astype(np.float32)
    val = (rng.random((nx, ny)) * np.where(rng.random((nx, ny)) < 0.5, -1, 1)).astype(np.float32)
    val[7, 9], val[100, 3] = np.nan, -np.inf
    with Dev(engine) as d:
        di, do, dv = d.put(idx), d.put(off), d.put(val)
        m1 = engine.arrival_plane_moments(nx, ny, dx, dy, dt, di, do, dv, r)
        m2 = engine.arrival_plane_moments(nx, ny, dx, dy, dt, di, do, dv, r)
        m0 = engine.arrival_plane_moments(nx, ny, dx, dy, dt, di, do, dv, 0.0)
    assert np.array_equal(m1.view(np.uint64), m2.view(np.uint64))
    want = model.plane_moments(idx, off, val, dx, dy, dt, r)
    assert m1[0] == want[0] and 0.3 * nx * ny < m1[0] < 0.7 * nx * ny
    assert m0[0] == nx * ny - 2                          # threshold 0: every finite pixel
    assert np.allclose(m1, want, rtol=1e-12, atol=1e-9)
    rc, fit = pkg.host_arrival_plane_fit(m1)
    assert rc == 0
    _check_fit(fit, model.plane_lstsq(idx, off, val, dx, dy, dt, r))


# cube, dx, dy (mm), planted tilt (degrees), dead pixels, trace length behind the Tilt stage
PLANTED = [((24, 20, 256), 1.0, 1.0, (1.2, -0.7), 0.0, 304),
           ((17, 19, 1001), 0.5, 0.5, (2.0, 1.0), 0.2, 1031),        # the one-launch tilted chain
           ((33, 16, 1024), 0.25, 1.0, (-3.0, 0.5), 0.1, 1062),
           ((16, 16, 200), 1.0, 1.0, (0.0, 0.0), 0.0, 200)]


@pytest.mark.parametrize("shape,dx,dy,tilt,dead,nt_out", PLANTED)
def test_planted_tilt_through_a_session(engine, shape, dx, dy, tilt, dead, nt_out):
    nx, ny, nt = shape
    time, cube, u, v, live = model.planted_cube(nx, ny, nt, dx, dy, tilt[0], tilt[1], dead)
    sess = pkg.Session(engine, nx, ny, time, dx, dy)
    try:
        sess.upload(cube, subtract_bias=False)
        rc, fit = sess.estimate_tilt(pkg.BUF_RAW, pkg.PEAK_MAX, 0.25)
        assert rc == 0
        idx, off, val = (sess.download(b, npix=nx * ny).reshape(nx, ny) for b in (pkg.BUF_PEAK_INDEX, pkg.BUF_PEAK_OFFSET, pkg.BUF_PEAK_VALUE))
        k, off64, value, bar, ok = model.peak_model(cube, 1)
        assert np.array_equal(idx, k) and np.array_equal(_bits(val), _bits(value)) and np.all(np.abs(off - off64) <= bar)
        assert np.array_equal(model.plane_mask(val, 0.25), live)           # the mask drops the dead pixels, no others
        _check_fit(fit, model.plane_lstsq(idx, off, val, dx, dy, model.mean_step(time), 0.25))
        err = model.edge_delay_samples(fit.tilt_x_deg - tilt[0], fit.tilt_y_deg - tilt[1], u, v)
        print(f"{shape}: estimate {fit.tilt_x_deg:.4f} / {fit.tilt_y_deg:.4f} deg, edge delay error {err:.4f} samples, rms {fit.rms_ps:.4f} ps")
        assert err < 0.1
        # flatten with the estimate, look again
        cfg = pkg.chain_cfg_default(time)
        cfg.tilt_x_deg, cfg.tilt_y_deg = fit.tilt_x_deg, fit.tilt_y_deg
        sess.recompute(cfg)
        assert sess.nt_out == nt_out
        if nt_out == 1031:
            assert engine.kernel_variant().startswith("fbp-")
        rc, res = sess.estimate_tilt(pkg.BUF_DATA, pkg.PEAK_MAX, 0.25)
        assert rc == 0 and res.n_used == live.sum()
        idx2, off2, val2 = (sess.download(b, npix=nx * ny).reshape(nx, ny) for b in (pkg.BUF_PEAK_INDEX, pkg.BUF_PEAK_OFFSET, pkg.BUF_PEAK_VALUE))
        data = sess.download(pkg.BUF_DATA).reshape(nx, ny, nt_out)
        k2, off64_2, value2, bar2, _ = model.peak_model(data, 1)
        assert np.array_equal(idx2, k2) and np.array_equal(_bits(val2), _bits(value2)) and np.all(np.abs(off2 - off64_2) <= bar2)
        _check_fit(res, model.plane_lstsq(idx2, off2, val2, dx, dy, model.mean_step(sess.time_out()), 0.25))
        w = model.plane_mask(val2, 0.25)
        assert np.array_equal(w, live)
        resid = model.edge_delay_samples(res.tilt_x_deg, res.tilt_y_deg, u, v)
        spread = int(idx2[w].max() - idx2[w].min())
        print(f"{shape}: residual {res.tilt_x_deg:.4f} / {res.tilt_y_deg:.4f} deg, edge delay {resid:.4f} samples, index spread {spread}")
        assert resid < 1.0
        assert spread <= 4
    finally:
        sess.close()


@pytest.mark.parametrize("members,nx", [(2, 17), (3, 17), (2, 33), (3, 33)])
def test_same_device_group_matches_one_session(engine, members, nx):
    ny, nt, dx, dy = 16, 200, 0.5, 1.0
    time, cube, _, _, _ = model.planted_cube(nx, ny, nt, dx, dy, 1.5, -1.0, dead=0.1, seed=members + nx)
    cfg = pkg.chain_cfg_default(time)
    cfg.tilt_x_deg, cfg.tilt_y_deg = 1.4, -1.1
    want = {}
    sess = pkg.Session(engine, nx, ny, time, dx, dy)
    try:
        sess.upload(cube, subtract_bias=False)
        for which in (pkg.BUF_RAW, pkg.BUF_DATA):
            if which == pkg.BUF_DATA:
                sess.recompute(cfg)
            rc, fit = sess.estimate_tilt(which, pkg.PEAK_ABS, 0.25)
            maps = [sess.download(b, npix=nx * ny) for b in (pkg.BUF_PEAK_INDEX, pkg.BUF_PEAK_OFFSET, pkg.BUF_PEAK_VALUE)]
            want[which] = (rc, fit.as_tuple(), maps)
    finally:
        sess.close()
    assert want[pkg.BUF_RAW][0] == 0 and want[pkg.BUF_RAW][1][6] > 0.8 * nx * ny
    with pkg.Group(devices=[0] * members) as g:
        gs = pkg.GroupSession(g, nx, ny, time, dx, dy)
        try:
            gs.upload(cube, subtract_bias=False)
            with pytest.raises(pkg.ThzError) as e:                         # nothing recomputed yet
                gs.estimate_tilt(pkg.BUF_DATA, pkg.PEAK_ABS, 0.25)
            assert e.value.code == -4
            for which in (pkg.BUF_RAW, pkg.BUF_DATA):
                if which == pkg.BUF_DATA:
                    gs.recompute(cfg)
                rc, fit = gs.estimate_tilt(which, pkg.PEAK_ABS, 0.25)
                assert rc == want[which][0]
                assert np.array_equal(np.array(fit.as_tuple()[:6]).view(np.uint64), np.array(want[which][1][:6]).view(np.uint64))
                assert fit.n_used == want[which][1][6]
                for got, ref in zip(gs.peak_maps(nx * ny), want[which][2]):
                    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
        finally:
            gs.close()


def test_session_bookkeeping(engine):
    nx, ny, nt, dx, dy = 12, 10, 256, 0.5, 0.75
    time, cube, _, _, _ = model.planted_cube(nx, ny, nt, dx, dy, 1.0, 0.5, seed=2)
    lib = engine.lib
    peak_bufs = (pkg.BUF_PEAK_INDEX, pkg.BUF_PEAK_OFFSET, pkg.BUF_PEAK_VALUE)
    sess = pkg.Session(engine, nx, ny, time, dx, dy)
    try:
        sess.upload(cube, subtract_bias=False)
        for b in peak_bufs:                                                # absent until first asked for
            assert not lib.thz_session_buffer(sess.h, b)
            with pytest.raises(pkg.ThzError) as e:
                sess.download(b, npix=nx * ny)
            assert e.value.code == -4
        for call in (lambda: sess.peak_map(pkg.BUF_DATA, 1), lambda: sess.estimate_tilt(pkg.BUF_DATA, 1, 0.25)):
            with pytest.raises(pkg.ThzError) as e:                         # no recompute has run
                call()
            assert e.value.code == -4
        for bad in (lambda: sess.peak_map(pkg.BUF_IMG, 1), lambda: sess.peak_map(pkg.BUF_RAW, 3)):
            with pytest.raises(pkg.ThzError) as e:
                bad()
            assert e.value.code == -1
        idx, off, val = sess.peak_map(pkg.BUF_RAW, pkg.PEAK_MIN)
        assert idx.shape == (nx, ny) and all(lib.thz_session_buffer(sess.h, b) for b in peak_bufs)
        assert np.array_equal(idx, model.peak_model(cube, 2)[0])
        with pytest.raises(pkg.ThzError) as e:                             # the maps hold nx * ny pixels
            sess.download(pkg.BUF_PEAK_VALUE, pix0=1, npix=nx * ny)
        assert e.value.code == -1
        # behind a scaling stage the maps and the fit live on the block grid, with its pixel sizes
        cfg = pkg.chain_cfg_default(time)
        cfg.scale_factor = 2
        sess.recompute(cfg)
        gx, gy, gdx, gdy = sess.grid()
        assert (gx, gy, gdx, gdy) == (nx // 2, ny // 2, 2 * dx, 2 * dy)
        rc, fit = sess.estimate_tilt(pkg.BUF_DATA, pkg.PEAK_MAX, 0.25)
        idx, off, val = (sess.download(b, npix=gx * gy).reshape(gx, gy) for b in peak_bufs)
        data = sess.download(pkg.BUF_DATA).reshape(gx, gy, sess.nt_out)
        assert np.array_equal(idx, model.peak_model(data, 1)[0])
        assert rc == 0 and fit.n_used == gx * gy
        _check_fit(fit, model.plane_lstsq(idx, off, val, gdx, gdy, model.mean_step(sess.time_out()), 0.25))
        assert abs(fit.tilt_x_deg - 1.0) < 0.1 and abs(fit.tilt_y_deg - 0.5) < 0.1     # block means keep the plane
        with pytest.raises(pkg.ThzError) as e:
            sess.download(pkg.BUF_PEAK_INDEX, npix=gx * gy + 1)
        assert e.value.code == -1
        # the raw grid again; a new upload voids the maps
        assert sess.peak_map(pkg.BUF_RAW, pkg.PEAK_ABS)[0].shape == (nx, ny)
        sess.upload(cube, subtract_bias=False)
        assert not any(lib.thz_session_buffer(sess.h, b) for b in peak_bufs)
    finally:
        sess.close()
