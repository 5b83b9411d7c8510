"""Regions of interest across call sequences of a session and a group (thz_session_set_rois, thz_session_recompute_from,
thz_group_session_*): new regions followed by a recompute that re-runs only the chain's tail (chain position 6 or 7,
the same front settings) must give what a fresh session with those regions and one full recompute gives.

The tail re-runs the ifft stage and what follows it, and the regions' sums are then taken afresh: the sums of the
fft stage's input traces (roi_data) need the multipliers in front of the transform one by one (want_means == 2), which
only a full recompute builds.  Each sequence below ends in such a recompute and is checked after every recompute:

- counts equal the fresh session's, and every vector is within 2e-6 of it (the tail path against the full path, as in
  test_session_recompute_from_each_chain_position; for a group also the slabs' sums, as in
  test_group_roi_equals_single_session);
- a session with want_means == 2: signal_fft, phase_fft and signal are the reference-order means of its resident
  arrays bit for bit, and roi_data is that of the oracle's windowed input traces;
- otherwise (want_means == 1, or a group's all-reduced slab sums): the same means within 2e-6.

Which path ran is pinned through the stage timers: a tail-only recompute runs no forward transform."""
import os

import numpy as np
import pytest

import oracle_binding as ob
import synth
import thz_image_explorer_amd as pkg
from test_gpu_roi import near, windowed_input

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
# 3 slabs of 12 rows (6 behind a scaling by 2); ny even: every slab starts at an even trace, so the paired-trace
# kernels (nt 1001, any tilted length) pair the traces as one session does
NX, NY, DX = 36, 32, 0.5
POLY_A = np.array([[2, 2], [20, 3], [25, 22], [9, 33], [0, 17]], np.uint64)
POLY_B = np.array([[12, 5], [31, 9], [27, 35], [15, 25]], np.uint64)
POLY_C = np.array([[3, 8], [29, 8], [16, 34]], np.uint64)
KEYS = ("signal_fft", "phase_fft", "signal", "roi_data")
FRONT = (pkg.binding.STAGE_FFT, pkg.binding.STAGE_PIPELINE)


def _copy(cfg):
    return type(cfg).from_buffer_copy(cfg)


def _tail_edit(cfg, time):
    """a Time Band Pass (after) slider: what chain position 7 re-runs"""
    c = _copy(cfg)
    c.td_after_high = float(time[-1]) - 3.0
    return c


def _fd_mask(nf):
    return (0.6 + 0.4 * np.cos(np.linspace(0.0, 7.0, nf))).astype(np.float32)


class _Target:
    """a Session, or a 3-member same-device GroupSession, behind one interface"""

    def __init__(self, kind, engine, time, cube):
        self.kind, self.g = kind, None
        if kind == "session":
            self.s = pkg.Session(engine, NX, NY, time, DX, DX)
            self.engs = [engine]
        else:
            self.g = pkg.Group(devices=[0] * 3)
            self.s = pkg.GroupSession(self.g, NX, NY, time, DX, DX)
            self.engs = [self.g.engine(i) for i in range(3)]
        self.s.upload(cube, subtract_bias=False)
        for e in self.engs:
            e.enable_timing(2)

    def drain(self):
        """(forward transforms, inverse transforms) run since the last drain, over every member"""
        counts = [sum(e.timing_collect(st)[1] for e in self.engs) for st in range(pkg.binding.STAGE_PROBE + 1)]
        return sum(counts[st] for st in FRONT), counts[pkg.binding.STAGE_IFFT]

    def recompute(self, cfg, stage):
        self.drain()
        if self.g is None:
            self.s.recompute(cfg, stage)
        else:
            self.s.recompute(cfg, stage, pkg.GATHER_ALL)
        return self.drain()

    def set_rois(self, polys):
        self.s.set_rois(polys)

    def set_fd_filters(self, mask):
        for s in [self.s] if self.g is None else [self.s.member(i) for i in range(3)]:
            s.set_fd_filters(mask)

    def deconvolve(self, psf, dcfg):
        return self.s.deconvolve(psf, dcfg)

    @property
    def nt_out(self):
        return self.s.nt_out if self.g is None else self.s.member(0).nt_out

    def roi(self, i):
        return self.s.roi(i) if self.g is None else self.s.roi(i, nt_out=self.nt_out)

    def arrays(self):
        nto = self.nt_out
        nf = nto // 2 + 1
        gx, gy = self.s.grid()[:2]
        get = (lambda w: self.s.download(w)) if self.g is None else (lambda w: self.s.download(w, nt_out=nto))
        return (get(pkg.BUF_AMPLITUDES).reshape(gx, gy, nf), get(pkg.BUF_PHASES).reshape(gx, gy, nf),
                get(pkg.BUF_DATA).reshape(gx, gy, nto))

    def close(self):
        self.drain()
        for e in self.engs:
            e.enable_timing(0)
        self.s.close()
        if self.g is not None:
            self.g.close()


def _fresh(engine, time, cube, cfg, polys, fd_mask):
    s = pkg.Session(engine, NX, NY, time, DX, DX)
    try:
        s.upload(cube, subtract_bias=False)
        if fd_mask is not None:
            s.set_fd_filters(fd_mask)
        s.set_rois(polys)
        s.recompute(cfg)
        return [s.roi(i) for i in range(len(polys))]
    finally:
        s.close()


def _check(t, engine, time, cube, cfg, polys, fd_mask=None):
    want = _fresh(engine, time, cube, cfg, polys, fd_mask)
    amp, ph, data = t.arrays()
    gx, gy = amp.shape[:2]
    scale = max(int(cfg.scale_factor), 1)
    src = ob.scale3d(cube, scale) if scale > 1 else cube
    win = windowed_input(src, time, cfg, DX * scale, DX * scale)
    assert win.shape == data.shape
    exact = cfg.want_means == 2 and t.g is None
    for i, poly in enumerate(polys):
        r = t.roi(i)
        assert r["count"] == want[i]["count"], i
        assert r["count"] > 0
        for k in KEYS:
            assert near(r[k], want[i][k].astype(np.float64), 2e-6), (i, k)
        mask, _ = ob.roi_mask(poly, scale, gx, gy)
        sel = np.flipud(mask).astype(bool)          # mask position (x, y) samples pixel [shape0 - y - 1, x]
        for k, arr in (("signal_fft", amp), ("phase_fft", ph), ("signal", data), ("roi_data", win)):
            if exact:    # the reference's order over the resident arrays, bit for bit
                assert np.array_equal(r[k], ob.average_polygon_roi(arr, poly, scale)), (i, k)
            else:
                assert near(r[k], arr[sel].astype(np.float64).mean(0), 2e-6), (i, k)


SEQUENCES = ["regions_after_a_full_recompute", "regions_replaced", "fd_filters_then_regions", "deconvolve_then_regions",
             "tilted_scaled"]


@pytest.mark.parametrize("nt", [1024, 1001])
@pytest.mark.parametrize("want_means", [2, 1])
@pytest.mark.parametrize("kind", ["session", "group"])
@pytest.mark.parametrize("seq", SEQUENCES)
def test_roi_call_sequences(engine, seq, kind, want_means, nt):
    time, cube = synth.make_cube(NX, NY, nt)
    cfg = pkg.chain_cfg_default(time)
    cfg.want_means = want_means
    cfg.td_before_low = float(time[0]) + 4.0    # every multiplier in front of the transform differs from 1
    if seq == "tilted_scaled":
        cfg.scale_factor, cfg.tilt_x_deg, cfg.tilt_y_deg = 2, 1.5, -1.0
    t = _Target(kind, engine, time, cube)
    try:
        if seq in ("regions_after_a_full_recompute", "tilted_scaled"):
            # 1 / 5: the last full recompute saw no regions
            front, _ = t.recompute(cfg, 1)
            assert front > 0
            if seq == "tilted_scaled":
                assert t.nt_out > nt                  # the tilt extends the traces
            t.set_rois([POLY_A, POLY_B])
            cfg7 = _tail_edit(cfg, time)
            front, inv = t.recompute(cfg7, 7)
            assert front == 0 and inv > 0             # the tail only
            _check(t, engine, time, cube, cfg7, [POLY_A, POLY_B])
        elif seq == "regions_replaced":
            # 2: the last full recompute had other regions
            t.set_rois([POLY_A, POLY_B])
            t.recompute(cfg, 1)
            _check(t, engine, time, cube, cfg, [POLY_A, POLY_B])
            t.set_rois([POLY_C])
            front, inv = t.recompute(cfg, 6)
            assert front == 0 and inv > 0
            _check(t, engine, time, cube, cfg, [POLY_C])
        elif seq == "fd_filters_then_regions":
            # 3: new Frequency-domain multipliers force the next recompute to start at the front, whatever it asks for
            t.recompute(cfg, 1)
            mask = _fd_mask(nt // 2 + 1)
            t.set_fd_filters(mask)
            t.set_rois([POLY_B])
            front, _ = t.recompute(cfg, 7)
            assert front > 0
            _check(t, engine, time, cube, cfg, [POLY_B], fd_mask=mask)
        else:
            # 4: the Deconvolution stage's output is the chain's final output until the tail runs again
            t.recompute(cfg, 1)
            psf = pkg.psf_from_npz(np.load(os.path.join(HERE, "golden", "psf_sample.npz")))
            assert t.deconvolve(psf, pkg.DeconvCfg(20, 5, 0.4, 3.0, 0.5)) == 0
            t.set_rois([POLY_A, POLY_C])
            cfg7 = _tail_edit(cfg, time)
            front, inv = t.recompute(cfg7, 7)
            assert front == 0 and inv > 0
            _check(t, engine, time, cube, cfg7, [POLY_A, POLY_C])
    finally:
        t.close()


def test_group_copy_outs_follow_a_tilt(engine):
    """GroupSession.roi() and .download() without nt_out: sized like the tilted chain's output traces, equal to one
    session's (the bars of test_group_session_shards_what_it_used_to_refuse for paired-trace lengths)"""
    from test_gpu_parity import rel
    nt = 1024
    time, cube = synth.make_cube(NX, NY, nt)
    cfg = pkg.chain_cfg_default(time)
    cfg.tilt_x_deg, cfg.tilt_y_deg, cfg.want_means = 1.5, -1.0, 2
    bufs = (pkg.BUF_IMG, pkg.BUF_DATA, pkg.BUF_FFT, pkg.BUF_AMPLITUDES, pkg.BUF_PHASES)
    avgs = (pkg.BUF_AVG_FFT, pkg.BUF_AVG_AMPLITUDES, pkg.BUF_AVG_PHASES)
    s = pkg.Session(engine, NX, NY, time, DX, DX)
    try:
        s.upload(cube, subtract_bias=False)
        s.set_rois([POLY_A])
        s.recompute(cfg)
        nto = s.nt_out
        want = {w: s.download(w) for w in bufs + avgs}
        want_roi = s.roi(0)
    finally:
        s.close()
    assert nto > nt
    with pkg.Group(devices=[0] * 3) as g:
        gs = pkg.GroupSession(g, NX, NY, time, DX, DX)
        try:
            gs.upload(cube, subtract_bias=False)
            gs.set_rois([POLY_A])
            gs.recompute(cfg, 1, pkg.GATHER_ALL)
            for w in bufs + avgs:
                got = gs.download(w)
                assert got.shape == want[w].shape, w
                if w == pkg.BUF_PHASES:       # last-bit inputs may flip a 2 pi decision on a noise bin
                    d = got.astype(np.float64) - want[w]
                    assert np.abs(d - 2 * np.pi * np.round(d / (2 * np.pi))).max() < 3e-3, w
                else:
                    assert rel(got, want[w]) < 2e-6, w
            r = gs.roi(0)
            assert r["count"] == want_roi["count"]
            for k in KEYS:
                assert r[k].shape == want_roi[k].shape, k
                assert near(r[k], want_roi[k].astype(np.float64), 2e-6), k
        finally:
            gs.close()
