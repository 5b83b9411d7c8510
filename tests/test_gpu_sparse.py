"""Sparse deconvolution on the device (csrc/sparse.hip, sparse_api.cpp) against thz_host_sparse_trace and the numpy model
of sparse_model.py: the kernel at the trace lengths and tap counts where its chunks, its padded tap tables and its LDS
image change, the session's bookkeeping, the loop the feature closes (spike trains -> echo map -> layer map -> optical
maps without the thickness image leaving the device) and same-device groups against one session.

A lane owns 16 consecutive outputs and a wave 1024 a trip, taps are padded to multiples of 16 behind a lead of
(shift % 16) zeros: the lengths straddle 16, 64, 256, 1024 and 4096, the tap counts 64 and 256, the centres are the first,
the middle and the last tap, and every cube carries samples at 0, nt - 1 and on either side of every 16- and 1024-output
boundary.

Bars:
- against thz_host_sparse_trace: value for value (np.array_equal, so -0 equals +0), the count of spikes exact, the residual
  within 1e-5 relative of the f64 sum taken on the returned x.
- exact-arithmetic inputs against the model: np.array_equal.
- tolerance configurations: per trace against the f64 model and that trace's own largest |x|, within 8 x the largest
  deviation of the numpy f32 form from the f64 form over the batch (floor 16 * 2^-24): from the two models alone.
- the thin wedge: the delay within one sample of the planted one at every pixel."""
import itertools

import numpy as np
import pytest

import echo_map_model
import sparse_model as model
import thz_image_explorer_amd as pkg
from test_gpu_helper_sizes import Dev

pytestmark = pytest.mark.gpu

NPIX = 23
NTS = (1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1001, 1023, 1024, 1025, 1027, 4096, 4608)
TAPS = (1, 2, 5, 63, 64, 65, 255, 256)


def _cover():
    """every (P, centre kind) pair twice, every length at least twice, P > nt included: 50 of the 432 combinations"""
    out = []
    for j, (P, kind) in enumerate(itertools.product(TAPS, range(3))):
        c = (0, P // 2, P - 1)[kind]
        out.append((NTS[j % len(NTS)], P, c))
        out.append((NTS[(7 * j + 5) % len(NTS)], P, c))
    # ... and the largest LDS image, the benchmark's shape, and the most taps on the shortest trace
    return sorted(set(out + [(4608, 256, 255), (4608, 256, 0), (1001, 64, 32), (1, 256, 128)]))


COVER = _cover()
assert {nt for nt, _, _ in COVER} == set(NTS) and {P for _, P, _ in COVER} == set(TAPS)
assert any(P > nt for nt, P, _ in COVER)


def _plant(y, values):
    """samples at 0, nt - 1 and on either side of every 16-output and 1024-output boundary, in the first rows of y"""
    nt = y.shape[1]
    lo, hi = values
    y[0, 0], y[0, nt - 1] = hi, lo
    y[1, 15::16] = hi
    y[2, 16::16] = lo
    y[3, 15::16], y[3, 16::16] = lo, hi
    y[4, 1023::1024] = hi
    y[5, 1024::1024] = lo
    y[6, :] = 0
    y[6, 0] = hi                     # a lone sample at either end
    y[7, :] = 0
    y[7, nt - 1] = lo
    return y


def _device(engine, y, h, cfg, off=0, in_place=False, resid=True, nnz=True):
    """thz_sparse_deconv on a cube `off` bytes behind a 16-byte boundary -> (x, resid or None, nnz or None)"""
    y = np.ascontiguousarray(y, np.float32)
    npix, nt = y.shape
    with Dev(engine) as d:
        src = d.put(y, off)
        out = src if in_place else d.new((npix, nt), off)
        dr = d.new(npix) if resid else None
        dn = d.put(np.full(npix, -7, np.int32)) if nnz else None
        engine.sparse_deconv(npix, nt, src, h, cfg, out, dr, dn)
        return (d.get(out, (npix, nt)), d.get(dr, npix).astype(np.float64) if resid else None,
                d.get(dn, npix, np.int32) if nnz else None)


def _host(y, h, cfg):
    xs, rs, ns = [], [], []
    for row in np.ascontiguousarray(y, np.float32):
        rc, x, resid, nnz = pkg.host_sparse_trace(row, h, cfg)
        assert rc == 0
        xs.append(x.copy())
        rs.append(resid)
        ns.append(nnz)
    return np.array(xs), np.array(rs, np.float64), np.array(ns, np.int32)


def _check_resid_nnz(y, h, c, x, resid, nnz, tag):
    want = model.resid_of(y, h, c, x)
    assert np.all(np.abs(resid - want) <= 1e-5 * want + 1e-30), (tag, resid, want)
    assert np.array_equal(nnz, (x != 0).sum(axis=1)), tag


def _real_case(nt, P, seed):
    """noise with planted samples and random taps -> (h, step, y)"""
    rng = np.random.default_rng(seed)
    h = rng.standard_normal(P).astype(np.float32)
    y = _plant(rng.standard_normal((NPIX, nt)).astype(np.float32), (-9.0, 9.0))
    return h, np.float32(1.0 / np.abs(h.astype(np.float64)).sum() ** 2), y


@pytest.mark.parametrize("nt,P,c", COVER)
def test_device_against_host_and_model(engine, nt, P, c):
    # exact-arithmetic inputs: the model, value for value
    h, y = model.exact_case(P, c, nt, npix=NPIX)
    y = _plant(y, (-8.0, 8.0))
    for n_iter, accelerate in ((2, 0), (2, 1), (1, 1), (0, 0)):
        want, want_nnz = model.exact_solution(h, c, y, n_iter, accelerate)
        cfg = pkg.sparse_cfg(P, c, n_iter, accelerate, model.EXACT_STEP, model.EXACT_REL, 0.0)
        x, resid, nnz = _device(engine, y, h, cfg)
        tag = (nt, P, c, n_iter, accelerate)
        assert np.array_equal(x, want), (tag, np.argwhere(x != want)[:8])
        assert np.array_equal(nnz, want_nnz), tag
        _check_resid_nnz(y, h, c, x, resid, nnz, tag)
    # real data: the host function, value for value
    h, step, y = _real_case(nt, P, 1000 * nt + P)
    for n_iter, accelerate in ((4, 1), (3, 0)):
        cfg = pkg.sparse_cfg(P, c, n_iter, accelerate, step, 0.05, 0.0)
        hx, hr, hn = _host(y, h, cfg)
        x, resid, nnz = _device(engine, y, h, cfg)
        tag = (nt, P, c, n_iter, accelerate, "host")
        assert np.array_equal(x, hx), (tag, np.argwhere(x != hx)[:8])
        assert np.array_equal(nnz, hn), tag
        _check_resid_nnz(y, h, c, x, resid, nnz, tag)
        assert np.all(np.abs(resid - hr) <= 1e-5 * hr + 1e-30), tag


@pytest.mark.parametrize("nt,P,c", [(1001, 64, 32), (257, 65, 0), (17, 5, 4)])
def test_alignment_in_place_and_optional_outputs(engine, nt, P, c):
    h, step, y = _real_case(nt, P, 77 + nt)
    cfg = pkg.sparse_cfg(P, c, 5, 1, step, 0.05, 0.0)
    hx, hr, hn = _host(y, h, cfg)
    for kw in (dict(off=4), dict(in_place=True), dict(off=4, in_place=True), dict(resid=False), dict(nnz=False),
               dict(resid=False, nnz=False, in_place=True)):
        x, resid, nnz = _device(engine, y, h, cfg, **kw)
        assert np.array_equal(x, hx), kw
        assert nnz is None or np.array_equal(nnz, hn), kw
        assert resid is None or np.all(np.abs(resid - hr) <= 1e-5 * hr), kw


def test_a_row_with_nan_leaves_its_neighbours_alone(engine):
    nt, P, c = 300, 64, 20
    h, step, y = _real_case(nt, P, 5)
    cfg = pkg.sparse_cfg(P, c, 6, 1, step, 0.05, 0.0)
    want = _device(engine, y, h, cfg)
    bad = y.copy()
    bad[11, 150] = np.nan
    bad[13, :] = np.inf
    got = _device(engine, bad, h, cfg)
    keep = np.array([r not in (11, 13) for r in range(NPIX)])
    assert np.array_equal(got[0][keep], want[0][keep])
    assert np.array_equal(got[1][keep], want[1][keep]) and np.array_equal(got[2][keep], want[2][keep])


def test_more_traces_than_one_grid_pass_and_stage_time(engine):
    """a launch has at most 256 x 16 waves: the 9001 traces here take a second and a third trip of the trace loop"""
    npix, nt, P, c = 9001, 64, 33, 16
    h, y = model.exact_case(P, c, nt, npix=npix)
    want, want_nnz = model.exact_solution(h, c, y, 2, 1)
    cfg = pkg.sparse_cfg(P, c, 2, 1, model.EXACT_STEP, model.EXACT_REL, 0.0)
    engine.enable_timing(1)
    try:
        x, resid, nnz = _device(engine, y, h, cfg)
        assert engine.stage_time_ns(pkg.STAGE_ECHO) > 0
    finally:
        engine.enable_timing(0)
    assert np.array_equal(x, want) and np.array_equal(nnz, want_nnz)
    _check_resid_nnz(y[:64], h, c, x[:64], resid[:64], nnz[:64], "9001 x 64")


@pytest.mark.parametrize("P,c,nt,n_iter,accelerate", model.TOLERANCE_CONFIGS)
def test_tolerance_configurations(engine, P, c, nt, n_iter, accelerate):
    h, step, y = model.tolerance_case(P, c, nt)
    ref, bar = model.reference_and_bar(y, h, c, n_iter, accelerate, step)
    cfg = pkg.sparse_cfg(P, c, n_iter, accelerate, step, 0.05, 0.0)
    x, resid, nnz = _device(engine, y, h, cfg)
    dev = model.deviation(x, ref["x"])
    print(f"P {P} c {c} nt {nt} n_iter {n_iter} accelerate {accelerate}: worst {dev.max():.3e} of bar {bar:.3e} = {dev.max() / bar:.3f}")
    assert np.all(dev <= bar), (dev.max(), bar)
    _check_resid_nnz(y, h, c, x, resid, nnz, (P, c, nt))
    hx, _, hn = _host(y, h, cfg)
    assert np.array_equal(x, hx) and np.array_equal(nnz, hn)


def test_refusals_launch_nothing(engine):
    nt, P, c = 33, 5, 2
    h, y = model.exact_case(P, c, nt, npix=NPIX)
    ok = dict(n_taps=P, center=c, n_iter=2, accelerate=1, step=0.01, rel_lambda=0.05, min_lambda=0.0)
    bad = [dict(n_taps=0), dict(n_taps=pkg.SPARSE_MAX_TAPS + 1), dict(center=-1), dict(center=P), dict(n_iter=-1),
           dict(n_iter=pkg.SPARSE_MAX_ITER + 1), dict(accelerate=2), dict(step=0.0), dict(step=np.inf), dict(step=np.nan),
           dict(rel_lambda=-0.1), dict(rel_lambda=np.nan), dict(min_lambda=-1.0), dict(min_lambda=np.inf)]
    big = np.ones(pkg.SPARSE_MAX_TAPS + 1, np.float32)
    with Dev(engine) as d:
        src, out, dr, dn = d.put(y), d.new((NPIX, nt)), d.new(NPIX), d.put(np.full(NPIX, -7, np.int32))

        def untouched():
            return np.isnan(d.get(out, (NPIX, nt))).all() and np.isnan(d.get(dr, NPIX)).all() and np.all(d.get(dn, NPIX, np.int32) == -7)

        def refused(call):
            with pytest.raises(pkg.ThzError) as e:
                call()
            assert e.value.code == -1 and untouched()

        for change in bad:
            refused(lambda: engine.sparse_deconv(NPIX, nt, src, big, pkg.sparse_cfg(**{**ok, **change}), out, dr, dn))
        for value in (np.nan, np.inf):
            taps = h.copy()
            taps[1] = value
            refused(lambda: engine.sparse_deconv(NPIX, nt, src, taps, pkg.sparse_cfg(**ok), out, dr, dn))
        cfg = pkg.sparse_cfg(**ok)
        refused(lambda: engine.sparse_deconv(NPIX, 0, src, h, cfg, out, dr, dn))
        refused(lambda: engine.sparse_deconv(NPIX, pkg.SPARSE_MAX_NT + 1, src, h, cfg, out, dr, dn))
        refused(lambda: engine.sparse_deconv(NPIX, nt, None, h, cfg, out, dr, dn))
        refused(lambda: engine.sparse_deconv(NPIX, nt, src, h, cfg, None, dr, dn))
        refused(lambda: engine._check(engine.lib.thz_sparse_deconv(engine.ctx, NPIX, nt, src, None, None, out, dr, dn)))
        engine.sparse_deconv(0, nt, src, h, cfg, out, dr, dn)   # no traces: a no-op
        assert untouched()
        engine.sparse_deconv(NPIX, nt, src, h, cfg, out, dr, dn)
        assert not untouched()


def test_session_bookkeeping(engine):
    nx, ny, nt, dx, dy = 12, 10, 384, 0.5, 0.75
    time, cube, gap, h, step = model.thin_wedge_scan(nx, ny, nt)
    lib = engine.lib
    bufs = (pkg.BUF_SPARSE, pkg.BUF_SPARSE_RESID, pkg.BUF_SPARSE_NNZ)
    cfg = pkg.sparse_cfg(64, 32, 40, 1, step, 0.05, 0.0)
    npix = nx * ny
    sess = pkg.Session(engine, nx, ny, time, dx, dy)
    try:
        sess.upload(cube, subtract_bias=False)
        for b in bufs:                                                      # absent until first asked for
            assert not lib.thz_session_buffer(sess.h, b)
            assert lib.thz_session_download(sess.h, b, 0, 1, np.zeros(nt, np.float32).ctypes.data) == -4
        for call in (lambda: sess.peak_map(pkg.BUF_SPARSE), lambda: sess.echo_map(pkg.BUF_SPARSE, pkg.echo_cfg(0, 2, 4, 0.3)),
                     lambda: sess.estimate_tilt(pkg.BUF_SPARSE), lambda: sess.sparse_deconv(pkg.BUF_DATA, h, cfg)):
            with pytest.raises(pkg.ThzError) as e:                          # no spike trains yet; no recompute has run
                call()
            assert e.value.code == -4
        for call in (lambda: sess.sparse_deconv(pkg.BUF_IMG, h, cfg), lambda: sess.sparse_deconv(pkg.BUF_SPARSE, h, cfg),
                     lambda: sess.sparse_deconv(pkg.BUF_RAW, h, pkg.sparse_cfg(64, 64, 40, 1, step, 0.05, 0.0)),
                     lambda: sess.sparse_deconv(pkg.BUF_RAW, h, pkg.sparse_cfg(64, 32, 40, 1, 0.0, 0.05, 0.0)),
                     lambda: engine._check(lib.thz_session_sparse_deconv(sess.h, pkg.BUF_RAW, None, cfg))):
            with pytest.raises(pkg.ThzError) as e:
                call()
            assert e.value.code == -1
        assert not any(lib.thz_session_buffer(sess.h, b) for b in bufs)
        x, resid, nnz = sess.sparse_deconv(pkg.BUF_RAW, h, cfg)
        assert x.shape == (nx, ny, nt) and resid.shape == (nx, ny) and nnz.dtype == np.int32
        assert all(lib.thz_session_buffer(sess.h, b) for b in bufs)
        hx, hr, hn = _host(cube.reshape(npix, nt), h, cfg)
        assert np.array_equal(x.reshape(npix, nt), hx) and np.array_equal(nnz.ravel(), hn)
        # downloads count pixels; nothing beyond the grid
        assert np.array_equal(sess.download(pkg.BUF_SPARSE, pix0=7, npix=3), hx[7:10])
        assert np.array_equal(sess.download(pkg.BUF_SPARSE_NNZ, pix0=npix - 2, npix=2), hn[-2:])
        assert np.array_equal(sess.download(pkg.BUF_SPARSE_RESID, pix0=5, npix=4), resid.ravel()[5:9])
        for b in bufs:
            with pytest.raises(pkg.ThzError) as e:
                sess.download(b, pix0=1, npix=npix)
            assert e.value.code == -1
        # the per-trace maps run on the spike trains, on the raw grid
        idx, off, val = sess.peak_map(pkg.BUF_SPARSE, pkg.PEAK_ABS)
        assert idx.shape == (nx, ny) and np.array_equal(idx.ravel(), np.abs(hx).argmax(axis=1))
        assert np.array_equal(val.ravel(), hx[np.arange(npix), np.abs(hx).argmax(axis=1)])
        found = sess.echo_map(pkg.BUF_SPARSE, pkg.echo_cfg(0, 2, 4, 0.3))
        want = echo_map_model.echo_model(hx, 0, 2, 4, 0.3)
        assert found[0].shape == (2, nx, ny) and np.array_equal(found[0].reshape(2, -1), want["index"])
        assert sess.estimate_tilt(pkg.BUF_SPARSE)[0] in (0, 1)
        # behind a scaling stage the spike trains live on the block grid, with the output's time axis
        chain = pkg.chain_cfg_default(time)
        chain.scale_factor = 2
        sess.recompute(chain)
        gx, gy = sess.grid()[:2]
        assert (gx, gy) == (nx // 2, ny // 2)
        x2, resid2, nnz2 = sess.sparse_deconv(pkg.BUF_DATA, h, cfg)
        nto = sess.nt_out
        assert x2.shape == (gx, gy, nto)
        data = sess.download(pkg.BUF_DATA).reshape(gx * gy, nto)
        hx2, _, hn2 = _host(data, h, cfg)
        assert np.array_equal(x2.reshape(gx * gy, nto), hx2) and np.array_equal(nnz2.ravel(), hn2)
        assert sess.peak_map(pkg.BUF_SPARSE)[0].shape == (gx, gy)
        with pytest.raises(pkg.ThzError) as e:
            sess.download(pkg.BUF_SPARSE, pix0=0, npix=gx * gy + 1)
        assert e.value.code == -1
        # the raw grid again; a new upload voids the spike trains
        assert sess.sparse_deconv(pkg.BUF_RAW, h, cfg)[0].shape == (nx, ny, nt)
        sess.upload(cube, subtract_bias=False)
        assert not any(lib.thz_session_buffer(sess.h, b) for b in bufs)
        with pytest.raises(pkg.ThzError) as e:
            sess.echo_map(pkg.BUF_SPARSE, pkg.echo_cfg(0, 2, 4, 0.3))
        assert e.value.code == -4
    finally:
        sess.close()


def test_session_closes_the_loop_from_a_thin_coating_to_optical_maps(engine):
    nx, ny, nt = 16, 12, 384
    time, cube, gap, h, step = model.thin_wedge_scan(nx, ny, nt)
    npix = nx * ny
    scale = np.float32(0.005)
    ref_pulse = np.zeros(nt, np.float32)
    ref_pulse[150 - 32:150 + 32] = h
    _, ref_amp, ref_phase = engine.reference_spectrum(time, time, ref_pulse)
    sess = pkg.Session(engine, nx, ny, time)
    try:
        sess.upload(cube, subtract_bias=False)
        # on the traces themselves the two pulses are one wavelet
        raw = sess.echo_map(pkg.BUF_RAW, pkg.echo_cfg(0, 2, 4, 0.3))[0].reshape(2, -1)
        raw_err = np.abs(np.abs(raw[1] - raw[0]) - gap.ravel())
        assert (raw_err > 1).mean() > 0.8
        sess.sparse_deconv(pkg.BUF_RAW, h, pkg.sparse_cfg(64, 32, 300, 1, step, 0.05, 0.0))
        idx, off, val, cnt = sess.echo_map(pkg.BUF_SPARSE, pkg.echo_cfg(0, 2, 4, 0.3))
        thick, delay = sess.layer_map(pkg.layer_cfg(pkg.LAYER_BETWEEN, scale))
        assert np.array_equal(cnt, np.full((nx, ny), 2))
        # the delay between the two spikes, in samples as the echo map finds them: within one of the planted gap everywhere
        err = np.abs(np.abs(idx[1] - idx[0]) - gap)
        assert np.all(err <= 1), np.argwhere(err > 1)[:8]
        # the layer map adds the two parabola offsets (each within half a sample) to it: the model's f32 operations
        t_want, d_want = echo_map_model.layer_model(idx.reshape(2, -1), off.reshape(2, -1), 0, [scale] * 4)
        assert np.array_equal(thick.reshape(1, -1).view(np.uint32), t_want.view(np.uint32))
        assert np.array_equal(delay.reshape(1, -1).view(np.uint32), d_want.view(np.uint32))
        sub = np.abs(delay[0].astype(np.float64) - gap)
        print(f"thin wedge, gaps {gap.min()} .. {gap.max()} samples: largest delay error {err.max()} samples "
              f"({sub.max():.3f} with the sub-sample offsets); on the raw traces {raw_err.max()}")
        assert np.all(sub <= err + 1.0)
        # into the optical maps without leaving the device, against the same image uploaded by the test
        sess.recompute(pkg.chain_cfg_default(time))
        f = pkg.host_frequency_axis(time)
        k = np.flatnonzero((f >= 0.5) & (f <= 1.5))
        band = (int(k[0]), int(k[-1]) + 1)
        ocfg = pkg.optical_cfg(1.0, band, [band, (band[0], band[0] + 5)])
        resident = engine.lib.thz_session_buffer(sess.h, pkg.BUF_LAYER_THICKNESS)
        assert resident
        a = sess.optical_maps(ref_amp, ref_phase, ocfg, thickness=resident)
        with Dev(engine) as d:
            b = sess.optical_maps(ref_amp, ref_phase, ocfg, thickness=d.put(thick[0]))
        for got, ref in zip(a, b):
            assert got.shape == ref.shape and np.array_equal(got.view(np.uint32), ref.view(np.uint32))
        c = sess.optical_maps(ref_amp, ref_phase, ocfg)                     # ... and the image does matter
        assert not np.array_equal(a[0].view(np.uint32), c[0].view(np.uint32))
    finally:
        sess.close()


@pytest.mark.parametrize("members", [2, 3])
def test_same_device_group_matches_one_session(engine, members):
    nx, ny, nt = 17, 12, 384
    time, cube, gap, h, step = model.thin_wedge_scan(nx, ny, nt, seed=members)
    cfg = pkg.sparse_cfg(64, 32, 30, 1, step, 0.05, 0.0)
    ecfg = pkg.echo_cfg(0, 2, 4, 0.3)
    sess = pkg.Session(engine, nx, ny, time)
    try:
        sess.upload(cube, subtract_bias=False)
        want = sess.sparse_deconv(pkg.BUF_RAW, h, cfg)
        want_echo = sess.echo_map(pkg.BUF_SPARSE, ecfg)
    finally:
        sess.close()
    with pkg.Group(devices=[0] * members) as g:
        gs = pkg.GroupSession(g, nx, ny, time)
        try:
            gs.upload(cube, subtract_bias=False)
            parts, echoes = [], []
            for i in range(members):
                m = gs.member(i)
                parts.append(m.sparse_deconv(pkg.BUF_RAW, h, cfg))
                echoes.append(m.echo_map(pkg.BUF_SPARSE, ecfg))
            assert sum(p[0].shape[0] for p in parts) == nx
            for q in range(3):                                             # the slabs' rows one after the other
                got = np.concatenate([p[q] for p in parts], axis=0)
                assert np.array_equal(got, want[q]), q
            for q in range(3):
                got = np.concatenate([e[q] for e in echoes], axis=1)
                assert np.array_equal(got.view(np.uint32), want_echo[q].view(np.uint32)), q
            rc, fit = gs.estimate_tilt(pkg.BUF_SPARSE)                     # the group's tilt runs on the spike trains too
            assert rc in (0, 1)
        finally:
            gs.close()
