"""FBP kernels (fft_fbp.hpp) on the device, through the C ABI: the trace lengths a tilted 1001-sample scan lands on
(1024 < nt <= 1280) run their chirp-z convolution on the mixed-radix core at M = 2304 / 2560; thz_set_kernel_family(2)
keeps them on the kernels over the F core (M = 4096), which is the A/B switch and the cross-check here."""
import numpy as np
import pytest

import oracle_binding as ob
import synth
import thz_image_explorer_amd as pkg
import trace_isolation as ti
from test_gpu_parity import TOL, gpu_fft_stage, phase_ok, rel
from test_gpu_session import check, oracle_chain
from test_gpu_trace_isolation import _check_all, _setup, _stages, _wiener_cmask

pytestmark = pytest.mark.gpu

LENGTHS = [1041, 1101, 1152, 1153, 1201, 1280]


def _prefix(nt, family):
    if family != 0:
        return "fb2-"
    return "fbp-bluestein-mixed-radix-12x12x16" if nt <= 1152 else "fbp-bluestein-mixed-radix-16x16x10"


@pytest.mark.parametrize("nt", LENGTHS)
def test_variant_by_family(engine, nt):
    time = synth.make_time(nt)
    try:
        for family in (0, 2):
            engine.set_kernel_family(family)
            engine.set_time_axis(time)
            assert engine.kernel_variant().startswith(_prefix(nt, family)), (family, engine.kernel_variant())
    finally:
        engine.set_kernel_family(0)


def test_neighbouring_lengths_keep_their_kernels(engine):
    for nt, prefix in ((1281, "fb2-"), (1502, "fb2-"), (1200, "p-mixed-radix"), (1023, "fb-bluestein"), (1024, "f-regs")):
        engine.set_time_axis(synth.make_time(nt))
        assert engine.kernel_variant().startswith(prefix), (nt, engine.kernel_variant())


# one trace, an odd count, more pairs than the grid has waves' worth of one trip per block
@pytest.mark.parametrize("family", [0, 2])
@pytest.mark.parametrize("grid", [(1, 1), (5, 3), (37, 19)])
@pytest.mark.parametrize("nt", LENGTHS)
def test_fused_pipeline_and_stages(engine, nt, grid, family):
    """the fused chain, fft with its windowed-trace output, the ifft round trip and the ifft of the stored spectrum — same
    oracle and tolerances in both families"""
    nx, ny = grid
    time = synth.make_time(nt)
    cube = synth.make_traces(np.arange(nx * ny) + 5, nt).reshape(nx, ny, nt).copy()
    engine.set_kernel_family(family)
    try:
        engine.set_time_axis(time)
        assert engine.kernel_variant().startswith(_prefix(nt, family))
        got = synth.run_gpu_pipeline(engine, cube, synth.default_chain(time))
        st_g = gpu_fft_stage(engine, cube, pkg.host_fft_window(time, 0, 1.0, 7.0))
        d_f = engine.to_device(st_g["fft"]); d_o = engine.empty((nx * ny, nt)); d_i = engine.empty((nx * ny,))
        engine.ifft(nx * ny, d_f, None, d_o, d_i)
        back = d_o.download((nx, ny, nt), np.float32)
        # Filter(6 / 7): the stand-alone inverse on the stored (masked) spectrum
        d_f.upload(got["fft"])
        d_w = engine.to_device(synth.default_chain(time)["w_post"])
        engine.ifft(nx * ny, d_f, d_w, d_o, d_i)
        again = d_o.download((nx, ny, nt), np.float32)
        again_img = d_i.download((nx, ny), np.float32)
        for b in (d_f, d_o, d_i, d_w):
            b.free()
    finally:
        engine.set_kernel_family(0)
    chain = synth.oracle_chain(time)
    ref = ob.run_pipeline(cube, time, chain)
    scale = np.abs(ref["fft"]).max()
    assert rel(got["fft"], ref["fft"], scale) < TOL
    assert rel(got["amplitudes"], ref["amplitudes"], scale) < TOL
    assert rel(got["data"], ref["data"]) < TOL
    assert rel(got["img"], ref["img"]) < TOL
    st = ob.fft_stage(cube * chain["w_tilt"] * chain["w_td_before"], time, 0, 1.0, 7.0)
    assert phase_ok(got["phases"], ref["phases"], st["amplitudes"])
    st_o = ob.fft_stage(cube, time, 0, 1.0, 7.0)
    assert np.array_equal(st_g["data"], st_o["data"])
    assert rel(st_g["fft"], st_o["fft"], np.abs(st_o["fft"]).max()) < TOL
    assert phase_ok(st_g["phases"], st_o["phases"], st_o["amplitudes"])
    assert rel(back, st_o["data"]) < TOL   # C2R(R2C(w x)) / nt = w x
    if family == 0:   # one launch: it inverts exactly the spectrum it stored
        assert np.array_equal(again, got["data"]) and np.array_equal(again_img, got["img"])
        assert np.all(got["fft"][..., 0, 1] == 0.0) and not np.signbit(got["fft"][..., 0, 1]).any()
        if nt % 2 == 0:
            assert np.all(got["fft"][..., -1, 1] == 0.0) and not np.signbit(got["fft"][..., -1, 1]).any()
    else:
        assert rel(again, ref["data"]) < TOL


ISO = [(1101, 0, "fbp-"), (1201, 0, "fbp-")]


@pytest.mark.parametrize("nt,family,prefix", ISO)
def test_every_trace_to_its_own_scale(engine, nt, family, prefix):
    try:
        chain = _setup(engine, nt, family, prefix)
        x = ti.make_cube(nt)
        bad = _check_all(nt, x, chain, _stages(engine, nt, x, chain))
        assert not bad, "; ".join(bad[:12])
    finally:
        engine.set_kernel_family(0)


@pytest.mark.parametrize("nt,family,prefix", ISO)
def test_partner_independence(engine, nt, family, prefix):
    """a trace scaled by 2^k (k = -30, -10, 10) leaves its partner's outputs bit-identical and comes out scaled by 2^k"""
    try:
        chain = _setup(engine, nt, family, prefix)
        factors = [1.0, 1e-3, 1e-4, 1.0, 1.0, 1.0, 1e2, 1.0, 1.0]
        x0 = ti.make_cube(nt, factors)
        base = synth.run_gpu_pipeline(engine, x0.reshape(-1, 1, nt), chain)
        keys = ("fft", "amplitudes", "phases", "data", "img")
        n = x0.shape[0]
        for moved in (0, 1):
            idx = np.arange(moved, n, 2)
            others = np.setdiff1d(np.arange(n), idx)
            others = others[(others ^ 1) < n]
            for k in (-30, -10, 10):
                x = x0.copy()
                x[idx] *= np.float32(2.0 ** k)
                got = synth.run_gpu_pipeline(engine, x.reshape(-1, 1, nt), chain)
                for key in keys:
                    a, b = got[key].reshape(n, -1), base[key].reshape(n, -1)
                    assert np.array_equal(a[others].view(np.uint32), b[others].view(np.uint32)), (moved, k, key)
                s = 2.0 ** k
                st = ["live" if i in idx else "skip" for i in range(n)]
                bad = ti.check("fft", ti.as_complex(got["fft"].reshape(n, -1, 2)), ti.as_complex(base["fft"].reshape(n, -1, 2)) * s, st)
                bad += ti.check("out", got["data"].reshape(n, -1), base["data"].reshape(n, -1).astype(np.float64) * s, st)
                bad += ti.check_intensity(got["img"].reshape(n), base["img"].reshape(n).astype(np.float64) * s * s, st)
                assert not bad, (moved, k, bad[:6])
    finally:
        engine.set_kernel_family(0)


def test_complex_multiplier_second_pass(engine):
    """thz_pipeline_ex with a complex multiplier at 1101: forward launch, launch_fd_cmask over the stored spectrum,
    inverse launch — each trace against float64 of X m H"""
    nt = 1101
    chain = _setup(engine, nt, 0, "fbp-")
    n, nf = 7, nt // 2 + 1
    x = np.ascontiguousarray(synth.make_traces(np.arange(n) + 3, nt), np.float32)
    H = _wiener_cmask(chain["time"], nf)
    e = engine
    bufs = [e.to_device(a) for a in (x, chain["w_pre"], chain["fd_mask"], H, chain["w_post"])]
    outs = [e.empty((n, nf, 2)), e.empty((n, nf)), e.empty((n, nf)), e.empty((n, nt)), e.empty((n,))]
    try:
        e.pipeline_ex(n, bufs[0], bufs[1], bufs[2], bufs[3], bufs[4], *outs, None)
        fft, amp, ph, out, img = (b.download(s, np.float32) for b, s in
                                  zip(outs, ((n, nf, 2), (n, nf), (n, nf), (n, nt), (n,))))
    finally:
        for b in bufs + outs:
            b.free()
    st = ["live"] * n
    ref = ti.forward_ref(x * chain["w_pre"], None, chain["fd_mask"], H)
    y, en = ti.inverse_ref(ref["fft"], nt, chain["w_post"])
    bad = ti.check("fft", ti.as_complex(fft), ref["fft"], st) + ti.check("amp", amp, ref["amp"], st)
    bad += ti.check("out", out, y, st) + ti.check_intensity(img, en, st)
    assert not bad, "; ".join(bad[:12])


# a 1001-sample scan on a 4 x 4 grid, dx = dy = 5 mm: (2, 0) degrees -> 23 steps -> 1047 samples (M = 2304),
# (4, 3.5) degrees -> 87 steps -> 1175 samples (M = 2560)
@pytest.mark.parametrize("tilt,lo,hi,radices", [((2.0, 0.0), 1024, 1152, "12x12x16"), ((4.0, 3.5), 1152, 1280, "16x16x10")])
def test_tilted_session(engine, tilt, lo, hi, radices):
    nx, ny, nt = 4, 4, 1001
    time, cube = synth.make_cube(nx, ny, nt)
    steps = pkg.host_tilt_plan(time, nx, ny, tilt[0], tilt[1], 5.0, 5.0)[0]
    assert lo < nt + 2 * int(steps) <= hi
    sess = pkg.Session(engine, nx, ny, time, dx=5.0, dy=5.0)
    try:
        sess.upload(cube, subtract_bias=False)
        cfg = pkg.chain_cfg_default(time)
        cfg.tilt_x_deg, cfg.tilt_y_deg = tilt
        ref = oracle_chain(cube, time, cfg, 5.0, 5.0)
        for want_means in (1, 2):
            cfg.want_means = want_means
            sess.recompute(cfg)
            assert lo < sess.nt_out <= hi
            assert engine.kernel_variant().startswith("fbp-bluestein-mixed-radix-" + radices)
            check(sess, ref, nx, ny)   # spectra, amplitudes, samples, image, mean spectrum and mean amplitudes
            # mean phases on the strong bins: equal up to whole turns of single pixels on noise bins in front of them
            # (phase_ok's rule for one trace), i.e. modulo 2 pi / npix
            strong = ref["avg"]["amp"] > 0.05 * ref["avg"]["amp"].max()
            d = sess.download(pkg.BUF_AVG_PHASES).astype(np.float64) - ref["avg"]["ph"]
            turn = 2 * np.pi / (nx * ny)
            assert np.abs(d - turn * np.round(d / turn))[strong].max() < 3e-3
        # Filter(7): the tail on the resident spectrum writes exactly what the full chain writes
        cfg.td_after_high = float(sess.time_out()[-1]) - 6.0
        sess.recompute(cfg, 7)
        tail, tail_img = sess.download(pkg.BUF_DATA).copy(), sess.download(pkg.BUF_IMG).copy()
        sess.recompute(cfg, 1)
        assert np.array_equal(tail, sess.download(pkg.BUF_DATA)) and np.array_equal(tail_img, sess.download(pkg.BUF_IMG))
        ref7 = oracle_chain(cube, time, cfg, 5.0, 5.0)
        check(sess, ref7, nx, ny)
        # the same session on the kernels over the F core
        engine.set_kernel_family(2)
        sess.recompute(cfg)
        assert engine.kernel_variant().startswith("fb2-")
        check(sess, ref7, nx, ny)
    finally:
        engine.set_kernel_family(0)
        sess.close()
