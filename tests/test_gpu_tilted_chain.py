"""A tilted scan's whole recompute as one launch from the raw cube (thz_pipeline_tilted; fft_fbp.hpp TILT / CM / SUMS):
the C ABI entry point against the oracle and against the staged path, its fallback at a length without an FBP plan,
the session with a real and a complex Frequency-domain plugin, a region of interest and a plot, and same-device groups."""
import os

import numpy as np
import pytest

import oracle_binding as ob
import synth
import thz_image_explorer_amd as pkg
import trace_isolation as ti
from thz_image_explorer_amd.binding import STAGE_PIPELINE
from test_gpu_parity import TOL, phase_ok, rel
from test_gpu_session import check, oracle_chain
from test_gpu_trace_isolation import _wiener_cmask

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")

# grid, dx = dy (mm), tilt (degrees), steps, nt_out — the oracle's plan for a 1001-sample scan
CASES = [((4, 4), 5.0, (2.0, 0.0), 23, 1047),
         ((4, 4), 5.0, (4.0, 3.5), 87, 1175),
         ((9, 7), 3.0, (-2.5, 2.0), 63, 1127),
         ((16, 12), 2.0, (3.0, -1.5), 76, 1153),
         ((33, 31), 1.0, (1.2, 1.0), 41, 1083),
         ((4, 4), 5.0, (0.3, 0.0), 3, 1007)]      # NOT an FBP length: the staged form inside the entry point


def _multipliers(cfg, new_time):
    """the session's multiplier vectors for a tilted chain: Time Band Pass x fft window, band pass, Time Band Pass after"""
    pre = pkg.host_td_bandpass(new_time, cfg.td_before_low, cfg.td_before_high, cfg.td_before_width)[0]
    pre = (pre * pkg.host_fft_window(new_time, cfg.fft_window.type, cfg.fft_window.lower, cfg.fft_window.upper)).astype(np.float32)
    mask = pkg.host_fd_bandpass(pkg.host_frequency_axis(new_time), cfg.fd_low, cfg.fd_high, cfg.fd_width)[0]
    post = pkg.host_td_bandpass(new_time, cfg.td_after_low, cfg.td_after_high, cfg.td_after_width)[0]
    return pre, mask, post


def _strong_share(amp_unmasked):
    strong = amp_unmasked > 0.05 * amp_unmasked.max(axis=-1, keepdims=True)
    return strong.reshape(-1, strong.shape[-1]).mean(axis=1)


def _mean_phase_ok(got, ref_avg_ph, ref_avg_amp, npix):
    """equal up to whole turns of single pixels on noise bins (phase_ok's rule for one trace), on the strong bins"""
    strong = ref_avg_amp > 0.05 * ref_avg_amp.max()
    assert strong.mean() >= 0.10
    d = got.astype(np.float64) - ref_avg_ph
    turn = 2 * np.pi / npix
    return np.abs(d - turn * np.round(d / turn))[strong].max() < 3e-3


@pytest.mark.parametrize("grid,d,tilt,steps,nt_out", CASES)
def test_pipeline_tilted_c_abi(engine, grid, d, tilt, steps, nt_out):
    nx, ny = grid
    npix, nt_in, nf = nx * ny, 1001, nt_out // 2 + 1
    time, cube = synth.make_cube(nx, ny, nt_in)
    got_steps, new_time, ins = pkg.host_tilt_plan(time, nx, ny, tilt[0], tilt[1], d, d)
    assert int(got_steps) == steps and new_time.size == nt_out
    cfg = pkg.chain_cfg_default(time)
    cfg.tilt_x_deg, cfg.tilt_y_deg = tilt
    ref = oracle_chain(cube, time, cfg, d, d)
    assert np.array_equal(ref["time"], new_time)
    pre, mask, post = _multipliers(cfg, new_time)
    taper = pkg.host_adapted_blackman(time, 0.0, 7.0)
    e = engine
    e.set_time_axis(new_time)
    assert e.kernel_variant().startswith("fbp-") == (1024 < nt_out <= 1280)
    shapes = ((npix, nf, 2), (npix, nf), (npix, nf), (npix, nt_out), (npix,))
    ins_b = e.to_device(np.ascontiguousarray(ins, np.int32))
    bufs = [e.to_device(a) for a in (cube.reshape(npix, nt_in), taper, pre, mask, post)]
    d_src, d_tap, d_pre, d_mask, d_post = bufs
    outs = [e.empty(s) for s in shapes]
    outs2 = [e.empty(s) for s in shapes]
    d_sums, d_ssum, d_ext = e.empty((2 * nf,)), e.empty((nt_out,)), e.empty((npix, nt_out))
    d_avg = e.empty((nf, 2))
    try:
        e.pipeline_tilted(npix, d_src, nt_in, d_tap, ins_b, d_pre, d_mask, None, d_post, *outs, sums=d_sums, src_sum=d_ssum)
        fft, amp, ph, out, img = (b.download(s, np.float32) for b, s in zip(outs, shapes))
        sums, ssum = d_sums.download((2 * nf,), np.float32), d_ssum.download((nt_out,), np.float32)
        # the staged path: thz_tilt_apply + thz_pipeline_ex, bit for bit
        e.tilt_apply(npix, d_src, nt_in, d_tap, ins_b, nt_out, d_ext)
        e.pipeline_ex(npix, d_ext, d_pre, d_mask, None, d_post, *outs2)
        for name, a, b, s in zip(("fft", "amp", "ph", "out", "img"), (fft, amp, ph, out, img), outs2, shapes):
            assert np.array_equal(a, b.download(s, np.float32)), name
        ext = d_ext.download((npix, nt_out), np.float32)
        # the mean spectrum by linearity: mask * FFT(pre * mean re-laid trace)
        d_mean = e.to_device((ssum.astype(np.float64) / npix).astype(np.float32))
        e.fft(1, d_mean, d_pre, None, None, d_avg, None, None, d_mask)
        avg_fft = d_avg.download((nf, 2), np.float32)
        d_mean.free()
        with pytest.raises(pkg.ThzError) as err:      # the traces are re-laid on the context's axis: nt_in <= nt
            e.pipeline_tilted(npix, d_src, nt_out + 1, d_tap, ins_b, d_pre, d_mask, None, d_post, *outs)
        assert err.value.code == -1
    finally:
        for b in bufs + outs + outs2 + [ins_b, d_sums, d_ssum, d_ext, d_avg]:
            b.free()
    scale = np.abs(ref["fft"]).max()
    assert rel(fft.reshape(nx, ny, nf, 2), ref["fft"], scale) < TOL
    assert rel(amp.reshape(nx, ny, nf), ref["amp"], scale) < TOL
    assert rel(out.reshape(nx, ny, nt_out), ref["data"]) < TOL
    assert rel(img.reshape(nx, ny), ref["img"]) < TOL
    # phase_ok pins the turn count on the bins above 5 % of a trace's largest amplitude: never an empty set
    assert _strong_share(ref["amp_unmasked"]).min() >= 0.10
    assert phase_ok(ph.reshape(nx, ny, nf), ref["ph"], ref["amp_unmasked"])
    assert np.array_equal(ext.reshape(nx, ny, nt_out), ob.tilt(cube, time, tilt[0], tilt[1], d, d)[2])
    # sums of the launch against float64 sums of what it stored; the re-laid traces' sum
    for got, arr in ((sums[:nf], amp), (sums[nf:], ph), (ssum, ext)):
        want = arr.astype(np.float64).sum(0)
        assert np.abs(got - want).max() <= 2e-6 * np.abs(want).max()
    assert rel(sums[:nf] / npix, ref["avg"]["amp"]) < TOL
    assert rel(avg_fft, ref["avg"]["fft"], np.abs(ref["avg"]["fft"]).max()) < TOL
    assert _mean_phase_ok(sums[nf:] / npix, ref["avg"]["ph"], ref["avg"]["amp"], npix)


def _filters(new_time):
    nf = new_time.size // 2 + 1
    freq = pkg.host_frequency_axis(new_time)
    lines = np.loadtxt(os.path.join(GOLD, "water_lines.csv"), dtype=np.float32)
    return pkg.host_water_line_mask(freq, lines, 0.01), _wiener_cmask(new_time, nf)


def _filtered_reference(ref, notch, H, post):
    """float64: the oracle chain's band-passed spectra times the two plugins, amplitudes, C2R, Time Band Pass, image"""
    nt = ref["time"].size
    Y = ti.as_complex(ref["fft"]) * notch.astype(np.float64) * (H[:, 0].astype(np.float64) + 1j * H[:, 1])
    amp = np.abs(Y)
    Y[..., 0] = Y[..., 0].real
    if nt % 2 == 0:
        Y[..., -1] = Y[..., -1].real
    data = np.fft.irfft(Y, n=nt, axis=-1) * post.astype(np.float64)
    return dict(fft=Y, amp=amp, data=data, img=(data ** 2).sum(-1), avg_fft=Y.mean(axis=(0, 1)), avg_amp=amp.mean(axis=(0, 1)))


def _near(a, b, tol=TOL):
    return np.abs(np.asarray(a, np.float64) - b).max() <= tol * max(np.abs(b).max(), 1e-30)


def test_tilted_session_with_plugins_region_and_plot(engine):
    nx, ny, nt, d, tilt = 16, 12, 1001, 2.0, (3.0, -1.5)
    npix = nx * ny
    time, cube = synth.make_cube(nx, ny, nt)
    cfg = pkg.chain_cfg_default(time)
    cfg.tilt_x_deg, cfg.tilt_y_deg = tilt
    assert cfg.want_means == 1
    ref = oracle_chain(cube, time, cfg, d, d)
    new_time = ref["time"]
    nto, nf = new_time.size, new_time.size // 2 + 1
    assert 1152 < nto <= 1280
    notch, H = _filters(new_time)
    _, _, post = _multipliers(cfg, new_time)
    fr = _filtered_reference(ref, notch, H, post)
    poly = np.array([[1, 1], [8, 2], [10, 9], [3, 11], [0, 5]], np.uint64)
    px, py = 5, 7
    res = {}
    sess = pkg.Session(engine, nx, ny, time, dx=d, dy=d)
    try:
        sess.upload(cube, subtract_bias=False)
        sess.set_rois([poly])
        sess.set_fd_filters(notch, H)
        for family in (0, 2):   # one launch from the raw cube; the staged path (k_tilt over the whole cube, F core)
            engine.set_kernel_family(family)
            engine.enable_timing(2)
            for stage in range(12):
                engine.timing_collect(stage)
            sess.recompute(cfg)
            calls = engine.timing_collect(STAGE_PIPELINE)[1]
            engine.enable_timing(0)
            assert engine.kernel_variant().startswith("fbp-" if family == 0 else "fb2-")
            if family == 0:
                assert calls == 1
            res[family] = dict(fft=sess.download(pkg.BUF_FFT), amp=sess.download(pkg.BUF_AMPLITUDES), ph=sess.download(pkg.BUF_PHASES),
                               data=sess.download(pkg.BUF_DATA), img=sess.download(pkg.BUF_IMG), avg_fft=sess.download(pkg.BUF_AVG_FFT),
                               avg_amp=sess.download(pkg.BUF_AVG_AMPLITUDES), avg_ph=sess.download(pkg.BUF_AVG_PHASES),
                               roi=sess.roi(0), plot=sess.plot(px, py), time=sess.time_out())
    finally:
        engine.enable_timing(0)
        engine.set_kernel_family(0)
        sess.close()
    for family, g in res.items():
        assert np.array_equal(g["time"], new_time)
        scale = np.abs(fr["fft"]).max()
        assert np.abs(ti.as_complex(g["fft"].reshape(nx, ny, nf, 2)) - fr["fft"]).max() / scale < TOL, family
        assert _near(g["amp"].reshape(nx, ny, nf), fr["amp"]), family
        assert _near(g["data"].reshape(nx, ny, nto), fr["data"]), family
        assert _near(g["img"].reshape(nx, ny), fr["img"]), family
        assert np.abs(ti.as_complex(g["avg_fft"]) - fr["avg_fft"]).max() / np.abs(fr["avg_fft"]).max() < TOL, family
        assert _near(g["avg_amp"], fr["avg_amp"]), family
        assert _strong_share(ref["amp_unmasked"]).min() >= 0.10
        assert phase_ok(g["ph"].reshape(nx, ny, nf), ref["ph"], ref["amp_unmasked"]), family
        assert _mean_phase_ok(g["avg_ph"], ref["avg"]["ph"], ref["avg"]["amp"], npix), family
        # the region: oracle's average_polygon_roi on the reference arrays
        r = g["roi"]
        mask, _ = ob.roi_mask(poly, 1, nx, ny)
        assert r["count"] == int(mask.sum()) > 0
        assert _near(r["signal_fft"], ob.average_polygon_roi(fr["amp"].astype(np.float32), poly)), family
        assert _near(r["signal"], ob.average_polygon_roi(fr["data"].astype(np.float32), poly)), family
        _, _, ext = ob.tilt(cube, time, tilt[0], tilt[1], d, d)
        dd, _, _ = ob.td_bandpass(ext, new_time, cfg.td_before_low, cfg.td_before_high, cfg.td_before_width)
        st = ob.fft_stage(dd, new_time, cfg.fft_window.type, cfg.fft_window.lower, cfg.fft_window.upper)
        assert _near(r["roi_data"], ob.average_polygon_roi(st["data"], poly)), family
        # the plot of one pixel: the fft stage's own amplitudes / phases (no band pass), the filtered vectors, the means
        p = g["plot"]
        assert np.array_equal(p["signal"], cube[px, py])
        assert _near(p["signal_fft"], st["amplitudes"][px, py]), family
        assert phase_ok(p["phase_fft"][None], st["phases"][px, py][None], st["amplitudes"][px, py][None]), family
        assert _near(p["filtered_signal"], fr["data"][px, py]) and _near(p["filtered_signal_fft"], fr["amp"][px, py]), family
        assert np.array_equal(p["filtered_phase_fft"], g["ph"].reshape(nx, ny, nf)[px, py])
        assert np.array_equal(p["avg_signal_fft"], g["avg_amp"]) and np.array_equal(p["avg_phase_fft"], g["avg_ph"])
        assert _near(p["avg_signal"], fr["data"].mean(axis=(0, 1))), family
    # roi_data and the plot's signal_fft come from the on-demand extended traces only: against the staged path
    a, b = res[0]["roi"]["roi_data"], res[2]["roi"]["roi_data"]
    assert np.abs(a.astype(np.float64) - b).max() <= 2e-6 * np.abs(b).max()
    assert _near(res[0]["plot"]["signal_fft"], res[2]["plot"]["signal_fft"].astype(np.float64))


@pytest.mark.parametrize("members", [2, 3])
def test_tilted_group_matches_one_session(engine, members):
    nx, ny, nt, d, tilt = 13, 6, 1001, 2.0, (3.0, 1.0)
    time, cube = synth.make_cube(nx, ny, nt)
    cfg = pkg.chain_cfg_default(time)
    cfg.tilt_x_deg, cfg.tilt_y_deg = tilt
    bufs = (pkg.BUF_IMG, pkg.BUF_DATA, pkg.BUF_FFT, pkg.BUF_AMPLITUDES, pkg.BUF_PHASES)
    avgs = (pkg.BUF_AVG_FFT, pkg.BUF_AVG_AMPLITUDES, pkg.BUF_AVG_PHASES)
    single = pkg.Session(engine, nx, ny, time, d, d)
    try:
        single.upload(cube, subtract_bias=False)
        single.recompute(cfg)
        nto = single.nt_out
        assert nto == 1001 + 2 * 52 and 1024 < nto <= 1280
        assert engine.kernel_variant().startswith("fbp-")
        want = {w: single.download(w) for w in bufs + avgs}
    finally:
        single.close()
    ref = oracle_chain(cube, time, cfg, d, d)
    with pkg.Group(devices=[0] * members) as g:
        gs = pkg.GroupSession(g, nx, ny, time, d, d)
        try:
            gs.upload(cube, subtract_bias=False)
            gs.recompute(cfg, 1, pkg.GATHER_ALL)
            assert g.engine(0).kernel_variant().startswith("fbp-")
            # traces are transformed in pairs: a slab that starts at an odd trace pairs them differently
            for w in bufs:
                got = gs.download(w, nt_out=nto)
                if w == pkg.BUF_PHASES:
                    dd = got.astype(np.float64) - want[w]
                    assert np.abs(dd - 2 * np.pi * np.round(dd / (2 * np.pi))).max() < 3e-3
                else:
                    assert rel(got, want[w]) < 2e-6, w
            for w in (pkg.BUF_AVG_FFT, pkg.BUF_AVG_AMPLITUDES):
                assert rel(gs.download(w, nt_out=nto), want[w]) < 2e-6, w
            assert _mean_phase_ok(gs.download(pkg.BUF_AVG_PHASES, nt_out=nto), ref["avg"]["ph"], ref["avg"]["amp"], nx * ny)
        finally:
            gs.close()
