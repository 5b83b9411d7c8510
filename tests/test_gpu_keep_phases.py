"""A session keeps its unwrapped phases between recomputes that leave them unchanged (session.hpp phases_known;
fft_f.hpp "kept phases"): the phases are those of FFT(pre x), so a recompute that moves the Frequency Band Pass, a
plugin or the post Time Band Pass is told to leave d_ph — and the phase half of the in-launch sums — alone.

One session of 29 x 71 = 2 059 traces of 4096 samples (several blocks' sum rows take part) is driven through a sequence
of recomputes; a second one is driven identically with THZ_F_KEEP_PHASES=0 around its calls, so that every launch of
it computes and writes phases.  After every step all per-pixel buffers, the three mean vectors and one region's means
must be np.array_equal to the reference session's, and — where the oracle models the step — match the oracle at
test_gpu_session.py's tolerances.  After every recompute the launcher's record says whether the fused launch kept the
phases (thz::g_f_last_phases_kept, next to thz::g_f_last_cfg); the sequence fixes the expected value of each.

Then the core of the sequence on a same-device group of two members with everything gathered: the mean phases behind
the group's all-reduce must equal the reference group's."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

import synth
import thz_image_explorer_amd as pkg
from test_gpu_parity import phase_ok
from test_gpu_session import check, oracle_chain

pytestmark = pytest.mark.gpu

NX, NY, NT = 29, 71, 4096
NF = NT // 2 + 1
PER_PIXEL = (pkg.BUF_FFT, pkg.BUF_AMPLITUDES, pkg.BUF_PHASES, pkg.BUF_DATA, pkg.BUF_IMG)
MEANS = (pkg.BUF_AVG_FFT, pkg.BUF_AVG_AMPLITUDES, pkg.BUF_AVG_PHASES)


def _kept():
    """whether this thread's latest fused launch left the phases alone: a thread-local of the library, not part of its
    C ABI (a group's members launch one after the other on the caller's thread: the last member's)"""
    return C.c_int.in_dll(pkg.load_library(), "_ZN3thz20g_f_last_phases_keptE").value


@contextlib.contextmanager
def computing_phases(on):
    """THZ_F_KEEP_PHASES=0 around a call (the library reads it at every recompute)"""
    if on:
        os.environ["THZ_F_KEEP_PHASES"] = "0"
    try:
        yield
    finally:
        os.environ.pop("THZ_F_KEEP_PHASES", None)


def pentagon(nx, ny):
    return np.array([[1, 1], [nx - 2, 0], [nx - 1, ny - 2], [nx // 2, ny - 1], [0, ny // 2]], np.int64)


class One:
    """a plain session; ref: every launch computes phases"""

    def __init__(self, eng, time, ref):
        self.s, self.eng, self.ref = pkg.Session(eng, NX, NY, time), eng, ref

    def upload(self, cube):
        self.s.upload(cube, subtract_bias=False)

    def recompute(self, cfg, start=1):
        with computing_phases(self.ref):
            self.s.recompute(cfg, start)
        return _kept()

    def set_fd_filters(self, real=None, cmask=None):
        self.s.set_fd_filters(real, cmask)

    def set_rois(self, polys):
        self.s.set_rois(polys)

    def deconvolve(self, psf, dcfg):
        return self.s.deconvolve(psf, dcfg)

    def poison_phases(self):
        """what a caller holding the pointer may do: NaN over all the phases"""
        nx, ny = self.s.grid()[:2]
        ptr = self.eng.lib.thz_session_buffer(self.s.h, pkg.BUF_PHASES)
        assert ptr
        junk = np.full(nx * ny * NF, np.nan, np.float32)
        self.eng._check(self.eng.lib.thz_memcpy_h2d(self.eng.ctx, ptr, junk.ctypes.data, junk.nbytes))
        self.eng.sync()

    def snapshot(self, means=True):
        out = {w: self.s.download(w) for w in PER_PIXEL + (MEANS if means else ())}
        if means:
            r = self.s.roi(0, want=["signal_fft", "phase_fft", "signal"])
            out["roi_fft"], out["roi_ph"], out["roi"], out["roi_n"] = r["signal_fft"], r["phase_fft"], r["signal"], r["count"]
        return out

    def close(self):
        self.s.close()


class Two:
    """a same-device group of two members, everything gathered"""

    def __init__(self, group, time, ref):
        self.g, self.ref = group, ref
        self.gs = pkg.GroupSession(group, NX, NY, time)

    def upload(self, cube):
        self.gs.upload(cube, subtract_bias=False)

    def recompute(self, cfg, start=1):
        with computing_phases(self.ref):
            self.gs.recompute(cfg, start, pkg.GATHER_ALL)
        return _kept()

    def set_fd_filters(self, real=None, cmask=None):
        for i in range(2):
            self.gs.member(i).set_fd_filters(real, cmask)

    def set_rois(self, polys):
        self.gs.set_rois(polys)

    def snapshot(self, means=True):
        out = {w: self.gs.download(w) for w in PER_PIXEL + (MEANS if means else ())}
        if means:
            r = self.gs.roi(0, want=["signal_fft", "phase_fft", "signal"])
            out["roi_fft"], out["roi_ph"], out["roi"], out["roi_n"] = r["signal_fft"], r["phase_fft"], r["signal"], r["count"]
        return out

    def close(self):
        self.gs.close()


def same(a, b, step):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k]), f"step '{step}': {k} differs from the session that computes phases every time"


def _copy(cfg):
    c = pkg.ChainCfg()
    C.memmove(C.byref(c), C.byref(cfg), C.sizeof(c))
    return c


class Driver:
    """runs a step on the session under test and on the reference, compares, and checks the record"""

    def __init__(self, a, b, time, check_oracle):
        self.a, self.b, self.time, self.check_oracle = a, b, time, check_oracle
        self.cube = None

    def both(self, act):
        act(self.a)
        act(self.b)

    def upload(self, cube):
        self.cube = cube
        self.both(lambda d: d.upload(cube))

    def rec(self, name, cfg, kept, oracle=True, start=1, means=True):
        c = _copy(cfg)
        got = self.a.recompute(c, start)
        ref = self.b.recompute(c, start)
        if start == 1:
            assert got == kept, f"step '{name}': the launch {'kept' if got else 'computed'} the phases"
            assert ref == 0, f"step '{name}': the reference session kept phases"
        sa = self.a.snapshot(means)
        same(sa, self.b.snapshot(means), name)
        if oracle and self.check_oracle:
            ref = oracle_chain(self.cube, self.time, c)
            check(self.a.s, ref, NX, NY)
        return sa


def _cubes():
    time, cube = synth.make_cube(NX, NY, NT)
    ids = np.arange(NX * NY, dtype=np.uint64) + 5000
    cube2 = synth.make_traces(ids, NT, subtract_bias=True).reshape(NX, NY, NT)
    return time, cube, cube2


def _plugins():
    notch = np.ones(NF, np.float32)
    notch[NF // 8:NF // 8 + 9] = 0.0
    notch[NF // 3] = 0.5
    H = np.empty((NF, 2), np.float32)
    H[:, 0] = 0.8 + 0.1 * np.cos(np.arange(NF) * 0.03)
    H[:, 1] = 0.2 * np.sin(np.arange(NF) * 0.05)
    return notch, H


def test_session_keeps_its_phases_where_they_cannot_change(engine):
    time, cube, cube2 = _cubes()
    notch, H = _plugins()
    a, b = One(engine, time, False), One(engine, time, True)
    d = Driver(a, b, time, True)
    try:
        cfg = pkg.chain_cfg_default(time)
        d.upload(cube)
        d.both(lambda s: s.set_rois([pentagon(NX, NY)]))
        # the region's pixel list is built by the first recompute that has the region, behind its launch, and a rebuilt
        # list starts a new source generation (as a changed grid does: the scale factor steps below)
        d.rec("the recompute that builds the region's list", cfg, 0)
        d.upload(cube)
        d.rec("first recompute after the upload", cfg, 0)
        d.rec("same configuration again", cfg, 1)
        cfg.fd_low, cfg.fd_high = 0.6, 2.5
        d.rec("other Frequency Band Pass limits", cfg, 1)
        d.both(lambda s: s.set_fd_filters(notch, None))
        d.rec("a real plugin", cfg, 1, oracle=False)
        d.both(lambda s: s.set_fd_filters(None, H))
        d.rec("a complex multiplier", cfg, 1, oracle=False)
        d.both(lambda s: s.set_fd_filters(None, None))
        cfg.td_after_low = float(time[0]) + 2.0
        d.rec("the post Time Band Pass changed", cfg, 1)
        cfg.td_after_low = float(time[0]) + 3.0
        d.rec("tail only", cfg, None, start=6)
        d.rec("a full recompute after the tail", cfg, 1)
        psf = pkg.psf_from_npz(np.load(os.path.join(os.path.dirname(__file__), "golden", "psf_sample.npz")))
        dcfg = pkg.DeconvCfg(2, 2, 0.4, 3.0, 0.5)
        d.both(lambda s: s.deconvolve(psf, dcfg))
        d.rec("after deconvolve", cfg, 1)
        cfg.fft_window.lower, cfg.fft_window.upper = 2.0, 6.0
        d.rec("fft window bounds changed", cfg, 0)
        d.rec("fft window bounds, repeated", cfg, 1)
        cfg.td_before_active = 0 if cfg.td_before_active else 1
        d.rec("td_before toggled", cfg, 0)
        d.rec("td_before toggled, repeated", cfg, 1)
        assert cfg.tilt_x_deg == 0.0 and cfg.tilt_y_deg == 0.0
        cfg.tilt_active = 0 if cfg.tilt_active else 1
        d.rec("tilt_active toggled at 0 degrees", cfg, 0)
        d.rec("tilt_active toggled, repeated", cfg, 1)
        cfg.scale_factor = 2
        d.rec("scale factor 2", cfg, 0, oracle=False)
        cfg.scale_factor = 1
        d.rec("scale factor 1 again", cfg, 0)
        cfg.want_means = 0
        # (the grid is the raw one again: the region's list was rebuilt behind the launch above)
        d.rec("without means", cfg, 0, oracle=False, means=False)
        d.rec("without means, repeated", cfg, 1, oracle=False, means=False)
        cfg.want_means = 1
        d.rec("the first with means: the phases in place came without their sums", cfg, 0)
        d.rec("the next with means", cfg, 1)
        d.both(lambda s: s.poison_phases())
        sa = d.rec("after NaN over the phases through thz_session_buffer", cfg, 0)
        assert np.isfinite(sa[pkg.BUF_PHASES]).all(), "the NaNs are gone"
        d.upload(cube2)
        sa = d.rec("a different cube of the same shape", cfg, 0)
        ref = oracle_chain(cube2, time, cfg)
        assert phase_ok(sa[pkg.BUF_PHASES].reshape(NX, NY, NF), ref["ph"], ref["amp_unmasked"]), "the phases are the new cube's"
        d.rec("the new cube, repeated", cfg, 1)
        cfg.fd_low, cfg.fd_high = 0.2, 7.0   # ends above bin N/2 + M1 = 1152 (5.6 THz): no pruned build, no kept phases
        d.rec("a band ending above N/2 + M1", cfg, 0)
    finally:
        a.close()
        b.close()


def test_group_of_two_keeps_its_phases_and_their_sums():
    time, cube, cube2 = _cubes()
    notch, H = _plugins()
    with pkg.Group(devices=[0, 0]) as g:
        a, b = Two(g, time, False), Two(g, time, True)
        d = Driver(a, b, time, False)
        try:
            cfg = pkg.chain_cfg_default(time)
            d.upload(cube)
            d.both(lambda s: s.set_rois([pentagon(NX, NY)]))
            d.rec("the recompute that builds the region's list", cfg, 0)
            d.upload(cube)
            d.rec("first recompute after the upload", cfg, 0)
            d.rec("same configuration again", cfg, 1)
            cfg.fd_low, cfg.fd_high = 0.6, 2.5
            d.rec("other Frequency Band Pass limits", cfg, 1)
            d.both(lambda s: s.set_fd_filters(notch, None))
            d.rec("a real plugin", cfg, 1)
            d.both(lambda s: s.set_fd_filters(None, H))
            d.rec("a complex multiplier", cfg, 1)
            d.both(lambda s: s.set_fd_filters(None, None))
            cfg.td_after_low = float(time[0]) + 2.0
            d.rec("the post Time Band Pass changed", cfg, 1)
            cfg.fft_window.lower, cfg.fft_window.upper = 2.0, 6.0
            d.rec("fft window bounds changed", cfg, 0)
            d.rec("fft window bounds, repeated", cfg, 1)
            d.upload(cube2)
            d.rec("a different cube of the same shape", cfg, 0)
            d.rec("the new cube, repeated", cfg, 1)
        finally:
            a.close()
            b.close()
