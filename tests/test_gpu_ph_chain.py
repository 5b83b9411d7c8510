"""The half-length chain of 2002-, 2400-, 3000- and 4000-sample scans with the complex per-bin multiplier and the pixel
sums inside its one launch (fft_ph.hpp: k_ph<P, kPipe, CM, SUMS>): thz_pipeline_ex against the numpy fp64 model of
test_fused_pipeline_ex, the number of launches it takes, the stand-alone inverse on the stored spectrum, ragged trace
counts, the order of the additions, and a session and a group with a reference open."""
import os

import numpy as np
import pytest

import oracle_binding as ob
import synth
import thz_image_explorer_amd as pkg
import trace_isolation as ti
from thz_image_explorer_amd.binding import STAGE_MEAN, STAGE_PIPELINE
from test_gpu_parity import TOL, phase_ok, rel
from test_gpu_session import oracle_chain

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
SUM_TOL = 2e-6   # include/thzgpu.h, d_sums
GRID = 256       # blocks of a full launch: one per CU

_FACTORS = {1001: (7, 11, 13), 1000: (10, 10, 10), 1200: (10, 10, 12), 1500: (10, 10, 15), 2000: (10, 10, 20)}


def _ph_waves(nt, sums):
    """waves per block of the PH kernel of an nt-sample scan — PHLayout<P>::waves(sums) of fft_ph.hpp: what 160 KB of
    LDS hold behind the tables (with the sums: and in front of the accumulators), 13 to 15 become 12, and the cap of
    the plan's widest butterfly"""
    n = nt // 2
    r1, r2, r3 = _FACTORS[n]
    m1 = r2 * r3
    t1, t2, we = n, m1 + (m1 & 1), n + 2

    def lds(w):
        if not sums:
            return (t1 + t2 + w * we) * 8
        return ((t1 + t2 + w * we + 1) & ~1) * 8 + (2 * 256 * ((n + 1 + 255) // 256) + 16) * 4

    w = 16
    while w > 1 and lds(w) > 160 * 1024:
        w -= 1
    if 13 <= w < 16:
        w = 12
    return min(w, 8 if r3 >= 20 else 12 if r3 >= 15 else 16)


def test_waves_helper_matches_the_documented_table():
    assert [_ph_waves(nt, False) for nt in (2002, 2400, 3000, 4000)] == [16, 12, 12, 8]
    assert [_ph_waves(nt, True) for nt in (2002, 2400, 3000, 4000)] == [16, 12, 11, 8]


def _wiener(time, nf):
    """K13 multiplier of a synthetic reference pulse: H = conj(R) / (|R|^2 + eps max|R|^2), numpy fp64 -> f32"""
    z = ((time - time[0] - 11.0) / 0.35).astype(np.float64)
    ref = -z * np.exp(-z * z)
    w = pkg.host_fft_window(time, 0, 1.0, 7.0).astype(np.float64)
    R = np.fft.rfft(ref * w)
    H = np.conj(R) / (np.abs(R) ** 2 + 1e-2 * (np.abs(R) ** 2).max())
    return np.ascontiguousarray(np.stack([H.real, H.imag], -1), np.float32)


def _reset_timing(e):
    e.enable_timing(2)
    for stage in range(12):
        e.timing_collect(stage)


class _Chain:
    """device buffers of one thz_pipeline_ex call on (npix, nt)"""

    def __init__(self, e, npix, nt, chain, H=None, sums=False, raw=None):
        nf = nt // 2 + 1
        self.e, self.npix, self.nt, self.nf = e, npix, nt, nf
        self.d_raw = e.to_device(raw) if raw is not None else e.empty((npix, nt))
        self.d_pre, self.d_fd, self.d_post = (e.to_device(chain[k]) for k in ("w_pre", "fd_mask", "w_post"))
        self.d_H = e.to_device(H) if H is not None else None
        self.d_fft, self.d_amp, self.d_ph = e.empty((npix, nf, 2)), e.empty((npix, nf)), e.empty((npix, nf))
        self.d_out, self.d_img = e.empty((npix, nt)), e.empty((npix,))
        self.d_sums = e.empty((2 * nf,)) if sums else None

    def run(self, npix=None):
        self.e.pipeline_ex(self.npix if npix is None else npix, self.d_raw, self.d_pre, self.d_fd, self.d_H, self.d_post,
                           self.d_fft, self.d_amp, self.d_ph, self.d_out, self.d_img, self.d_sums)
        self.e.sync()

    def get(self, npix=None):
        n, nt, nf = self.npix if npix is None else npix, self.nt, self.nf
        res = dict(fft=self.d_fft.download((self.npix, nf, 2), np.float32)[:n], amp=self.d_amp.download((self.npix, nf), np.float32)[:n],
                   ph=self.d_ph.download((self.npix, nf), np.float32)[:n], out=self.d_out.download((self.npix, nt), np.float32)[:n],
                   img=self.d_img.download((self.npix,), np.float32)[:n])
        if self.d_sums is not None:
            res["sums"] = self.d_sums.download((2 * nf,), np.float32)
        return res

    def free(self):
        for b in (self.d_raw, self.d_pre, self.d_fd, self.d_post, self.d_H, self.d_fft, self.d_amp, self.d_ph, self.d_out,
                  self.d_img, self.d_sums):
            if b is not None:
                b.free()


def _check_sums(sums, amp, ph, nf, tag=""):
    assert np.isfinite(sums).all(), tag
    sa, sp = amp.astype(np.float64).sum(0), ph.astype(np.float64).sum(0)
    assert np.abs(sums[:nf] - sa).max() <= SUM_TOL * np.abs(sa).max(), tag
    assert np.abs(sums[nf:] - sp).max() <= SUM_TOL * max(np.abs(sp).max(), 1.0), tag


def _check_against_model(g, cube, time, chain, H, shape):
    """the model and tolerances of test_fused_pipeline_ex"""
    nx, ny, nt = shape
    npix, nf = nx * ny, nt // 2 + 1
    fft, amp, ph, out, img = g["fft"], g["amp"], g["ph"], g["out"], g["img"]
    ref = ob.run_pipeline(cube, time, chain)
    if H is None:
        scale = np.abs(ref["fft"]).max()
        assert rel(fft, ref["fft"].reshape(npix, nf, 2), scale) < TOL
        assert rel(amp, ref["amplitudes"].reshape(npix, nf), scale) < TOL
        assert rel(out, ref["data"].reshape(npix, nt)) < TOL
        assert rel(img, ref["img"].ravel()) < TOL
    else:
        pre = chain["w_tilt"].astype(np.float64) * chain["w_td_before"] * chain["w_fft"]
        X = np.fft.rfft(cube.reshape(npix, nt).astype(np.float64) * pre, axis=1)
        Y = X * ((H[:, 0].astype(np.float64) + 1j * H[:, 1]) * chain["fd_mask"])
        a_ref = np.abs(Y)
        Y[:, 0] = Y[:, 0].real
        Y[:, -1] = Y[:, -1].real
        t_ref = np.fft.irfft(Y, n=nt, axis=1) * chain["w_post"]
        assert np.abs(ti.as_complex(fft) - Y).max() / np.abs(Y).max() < TOL
        assert np.all(fft[:, 0, 1] == 0) and np.all(fft[:, -1, 1] == 0)   # C2R precondition
        assert not np.signbit(fft[:, 0, 1]).any() and not np.signbit(fft[:, -1, 1]).any()
        assert np.abs(amp - a_ref).max() / a_ref.max() < TOL
        assert np.abs(out - t_ref).max() / np.abs(t_ref).max() < TOL
        assert np.abs(img - (t_ref ** 2).sum(1)).max() / (t_ref ** 2).sum(1).max() < TOL
    st = ob.fft_stage(cube * chain["w_tilt"] * chain["w_td_before"], time, 0, 1.0, 7.0)
    assert phase_ok(ph.reshape(nx, ny, nf), ref["phases"], st["amplitudes"])   # phases are those of X in every mode
    if "sums" in g:
        _check_sums(g["sums"], amp, ph, nf)


@pytest.mark.parametrize("mode", ["cmask", "sums", "cmask+sums", "cmask+sums+passes"])
@pytest.mark.parametrize("shape", [(3, 3, 2002), (5, 1, 2400), (7, 2, 3000), (3, 3, 4000)])
def test_pipeline_ex_parity_and_launch_counts(engine, shape, mode, monkeypatch):
    nx, ny, nt = shape
    if "passes" in mode:
        monkeypatch.setenv("THZ_NO_FUSED_SUMS", "1")
    time, cube = synth.make_cube(nx, ny, nt)
    e = engine
    e.set_time_axis(time)
    assert e.kernel_variant().startswith("ph-half-length-mixed-radix")
    chain_p, chain = synth.default_chain(time), synth.oracle_chain(time)
    npix, nf = nx * ny, nt // 2 + 1
    H = _wiener(time, nf) if "cmask" in mode else None
    c = _Chain(e, npix, nt, chain_p, H, "sums" in mode, raw=cube)
    try:
        _reset_timing(e)
        c.run()
        pipe_calls, mean_calls = e.timing_collect(STAGE_PIPELINE)[1], e.timing_collect(STAGE_MEAN)[1]
        e.enable_timing(0)
        g = c.get()
        # the staged chirp-z path as a control, in the same buffers
        e.set_kernel_family(2)
        assert not e.kernel_variant().startswith("ph-")
        c.run()
        control = c.get()
    finally:
        e.enable_timing(0)
        e.set_kernel_family(0)
        c.free()
    assert pipe_calls == 1
    # the sums ride in the launch and one small pass adds the blocks' rows; forced out of it they are two passes over
    # the stored arrays (which is what they were at these lengths before the kernel took them)
    assert mean_calls == (0 if "sums" not in mode else 2 if "passes" in mode else 1)
    _check_against_model(g, cube, time, chain, H, shape)
    _check_against_model(control, cube, time, chain, H, shape)


@pytest.mark.parametrize("shape", [(3, 3, 2002), (2, 1, 4000)])
def test_stand_alone_inverse_lands_on_the_fused_samples(engine, shape):
    """a Filter(6 / 7) partial recompute runs thz_ifft on the resident spectrum: with the multiplier in the launch that
    spectrum is X (H m), and the launch must have inverted exactly what it stored"""
    nx, ny, nt = shape
    time, cube = synth.make_cube(nx, ny, nt)
    e = engine
    e.set_time_axis(time)
    assert e.kernel_variant().startswith("ph-")
    npix, nf = nx * ny, nt // 2 + 1
    c = _Chain(e, npix, nt, synth.default_chain(time), _wiener(time, nf), raw=cube)
    d_out2, d_img2 = e.empty((npix, nt)), e.empty((npix,))
    try:
        c.run()
        e.ifft(npix, c.d_fft, c.d_post, d_out2, d_img2)
        e.sync()
        g = c.get()
        out2, img2 = d_out2.download((npix, nt), np.float32), d_img2.download((npix,), np.float32)
    finally:
        c.free()
        d_out2.free()
        d_img2.free()
    assert np.abs(g["out"]).max() > 0
    assert np.array_equal(g["out"], out2)
    assert np.array_equal(g["img"], img2)


def _ragged_counts(nt):
    w = _ph_waves(nt, True)
    return {2002: (1, w - 1, w + 1, GRID * w + 1), 4000: (1, w + 1, GRID * w + 3, 2 * GRID * w + 1)}[nt]


@pytest.mark.parametrize("nt", [2002, 4000])
def test_in_launch_sums_ragged_trace_counts(engine, nt):
    """fewer traces than a block has waves, one more than its waves, a few more than whole trips of the whole grid: waves
    and whole blocks that never see a trace, and a last trip that most waves stay away from"""
    e = engine
    time = synth.make_time(nt)
    e.set_time_axis(time)
    assert e.kernel_variant().startswith("ph-")
    nf = nt // 2 + 1
    counts = _ragged_counts(nt)
    nmax = max(counts)
    c = _Chain(e, nmax, nt, synth.default_chain(time), None, True)
    d_t = e.to_device(time)
    try:
        e.synth_cube(c.d_raw, nmax, 0, d_t)
        for npix in counts:
            c.run(npix)
            g = c.get(npix)
            _check_sums(g["sums"], g["amp"], g["ph"], nf, npix)
    finally:
        c.free()
        d_t.free()


def test_in_launch_sums_are_deterministic(engine):
    """the tickets fix the order of every bin's additions, so repeated launches give the same bits — three launches over
    three trips of the whole grid and a ragged fourth"""
    nt = 3000
    npix = 3 * GRID * _ph_waves(nt, True) + 5
    e = engine
    time = synth.make_time(nt)
    e.set_time_axis(time)
    nf = nt // 2 + 1
    c = _Chain(e, npix, nt, synth.default_chain(time), _wiener(time, nf), True)
    d_t = e.to_device(time)
    try:
        e.synth_cube(c.d_raw, npix, 0, d_t)
        got = []
        for _ in range(3):
            c.run()
            got.append(c.d_sums.download((2 * nf,), np.float32))
    finally:
        c.free()
        d_t.free()
    assert np.isfinite(got[0]).all() and np.abs(got[0]).max() > 0
    assert np.array_equal(got[0], got[1]) and np.array_equal(got[0], got[2])


# ---- session and group: a reference open (K13), a notch (K14), one region, the default want_means -----------------------
def _filters(time):
    nf = time.size // 2 + 1
    freq = pkg.host_frequency_axis(time)
    lines = np.loadtxt(os.path.join(GOLD, "water_lines.csv"), dtype=np.float32)
    return pkg.host_water_line_mask(freq, lines, 0.01), _wiener(time, nf)


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


def _mean_phase_ok(got, ref_avg_ph, ref_avg_amp, npix):
    """equal up to whole turns of single pixels on noise bins (phase_ok's rule for one trace), on the strong bins"""
    strong = ref_avg_amp > 0.05 * ref_avg_amp.max()
    assert strong.mean() >= 0.10
    d = got.astype(np.float64) - ref_avg_ph
    turn = 2 * np.pi / npix
    return np.abs(d - turn * np.round(d / turn))[strong].max() < 3e-3


BUFS = (pkg.BUF_IMG, pkg.BUF_DATA, pkg.BUF_FFT, pkg.BUF_AMPLITUDES, pkg.BUF_PHASES)
AVGS = (pkg.BUF_AVG_FFT, pkg.BUF_AVG_AMPLITUDES, pkg.BUF_AVG_PHASES)


def test_session_and_group_with_a_reference_open(engine):
    nx, ny, nt = 6, 5, 2002
    npix, nf = nx * ny, nt // 2 + 1
    time, cube = synth.make_cube(nx, ny, nt)
    cfg = pkg.chain_cfg_default(time)
    assert cfg.want_means == 1
    ref = oracle_chain(cube, time, cfg)
    assert ref["time"].size == nt
    notch, H = _filters(time)
    post = pkg.host_td_bandpass(time, cfg.td_after_low, cfg.td_after_high, cfg.td_after_width)[0]
    fr = _filtered_reference(ref, notch, H, post)
    poly = np.array([[1, 1], [4, 1], [5, 3], [2, 4], [0, 2]], np.uint64)
    sess = pkg.Session(engine, nx, ny, time)
    try:
        sess.upload(cube, subtract_bias=False)
        sess.set_rois([poly])
        sess.set_fd_filters(notch, H)
        _reset_timing(engine)
        sess.recompute(cfg)
        calls = engine.timing_collect(STAGE_PIPELINE)[1]
        engine.enable_timing(0)
        assert engine.kernel_variant().startswith("ph-half-length-mixed-radix")
        assert calls == 1
        g = {w: sess.download(w) for w in BUFS + AVGS}
        roi = sess.roi(0)
        # Filter(7): the Time Band Pass after the inverse, from the resident spectrum
        sess.recompute(cfg, start_stage=7)
        assert np.array_equal(sess.download(pkg.BUF_DATA), g[pkg.BUF_DATA])
    finally:
        engine.enable_timing(0)
        sess.close()
    scale = np.abs(fr["fft"]).max()
    assert np.abs(ti.as_complex(g[pkg.BUF_FFT].reshape(nx, ny, nf, 2)) - fr["fft"]).max() / scale < TOL
    assert _near(g[pkg.BUF_AMPLITUDES].reshape(nx, ny, nf), fr["amp"])
    assert _near(g[pkg.BUF_DATA].reshape(nx, ny, nt), fr["data"])
    assert _near(g[pkg.BUF_IMG].reshape(nx, ny), fr["img"])
    assert np.abs(ti.as_complex(g[pkg.BUF_AVG_FFT]) - fr["avg_fft"]).max() / np.abs(fr["avg_fft"]).max() < TOL
    assert _near(g[pkg.BUF_AVG_AMPLITUDES], fr["avg_amp"])
    assert phase_ok(g[pkg.BUF_PHASES].reshape(nx, ny, nf), ref["ph"], ref["amp_unmasked"])
    assert _mean_phase_ok(g[pkg.BUF_AVG_PHASES], ref["avg"]["ph"], ref["avg"]["amp"], npix)
    mask, _ = ob.roi_mask(poly, 1, nx, ny)
    assert roi["count"] == int(mask.sum()) > 0
    assert _near(roi["signal_fft"], ob.average_polygon_roi(fr["amp"].astype(np.float32), poly))
    assert _near(roi["signal"], ob.average_polygon_roi(fr["data"].astype(np.float32), poly))

    # the same through a two-member group on one device: one trace per wave, so a slab's traces are the session's bits
    with pkg.Group(devices=[0, 0]) as grp:
        gs = pkg.GroupSession(grp, nx, ny, time)
        try:
            gs.upload(cube, subtract_bias=False)
            for i in range(2):
                gs.member(i).set_fd_filters(notch, H)
            gs.recompute(cfg, 1, pkg.GATHER_ALL)
            assert grp.engine(0).kernel_variant().startswith("ph-")
            for w in BUFS:
                assert np.array_equal(gs.download(w), g[w]), w
        finally:
            gs.close()
