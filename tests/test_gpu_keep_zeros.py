"""A session leaves the out-of-band zeros of its spectrum and amplitudes in place between recomputes (fft_f.hpp "keep
range", session.hpp zeros_known): one session is driven through a sequence of recomputes that moves, drops and
re-establishes the Frequency Band Pass's range, and after every step ALL its outputs must equal those of a second
session driven identically with THZ_F_KEEP_ZEROS=0 (every launch writes everything) — np.array_equal, so a stale
value anywhere in a row shows, and -0 equals +0 — and, wherever the oracle models the step, the oracle at the
tolerances of test_gpu_session.py."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

import synth
import thz_image_explorer_amd as pkg
from test_gpu_session import check, oracle_chain

pytestmark = pytest.mark.gpu

PER_PIXEL = (pkg.BUF_FFT, pkg.BUF_AMPLITUDES, pkg.BUF_PHASES, pkg.BUF_DATA, pkg.BUF_IMG)
MEANS = (pkg.BUF_AVG_FFT, pkg.BUF_AVG_AMPLITUDES, pkg.BUF_AVG_PHASES)


@contextlib.contextmanager
def full_writes(on):
    """THZ_F_KEEP_ZEROS=0 around a call (the library reads it at every recompute)"""
    if on:
        os.environ["THZ_F_KEEP_ZEROS"] = "0"
    try:
        yield
    finally:
        os.environ.pop("THZ_F_KEEP_ZEROS", None)


class One:
    """a plain session"""

    def __init__(self, eng, nx, ny, time, full):
        self.s, self.eng, self.full = pkg.Session(eng, nx, ny, time), eng, full

    def upload(self, cube):
        self.s.upload(cube, subtract_bias=False)

    def recompute(self, cfg, start=1):
        with full_writes(self.full):
            self.s.recompute(cfg, start)

    def set_fd_filters(self, real=None, cmask=None):
        self.s.set_fd_filters(real, cmask)

    def set_rois(self, polys):
        self.s.set_rois(polys)

    def poison(self):
        """what a caller holding the pointers may do: NaN over the whole spectrum and all amplitudes"""
        nx, ny = self.s.grid()[:2]
        nf = self.s.nt_out // 2 + 1
        for which, per in ((pkg.BUF_FFT, 2 * nf), (pkg.BUF_AMPLITUDES, nf)):
            ptr = self.eng.lib.thz_session_buffer(self.s.h, which)
            assert ptr
            junk = np.full(nx * ny * per, np.nan, np.float32)
            self.eng._check(self.eng.lib.thz_memcpy_h2d(self.eng.ctx, ptr, junk.ctypes.data, junk.nbytes))
        self.eng.sync()

    def snapshot(self):
        out = {w: self.s.download(w) for w in PER_PIXEL + MEANS}
        r = self.s.roi(0, want=["signal_fft", "signal"])
        out["roi_fft"], out["roi"], out["roi_n"] = r["signal_fft"], r["signal"], r["count"]
        return out

    def close(self):
        self.s.close()


class Two:
    """a same-device group of two members, everything gathered"""

    def __init__(self, group, nx, ny, time, full):
        self.g, self.full = group, full
        self.gs = pkg.GroupSession(group, nx, ny, time)

    def upload(self, cube):
        self.gs.upload(cube, subtract_bias=False)

    def recompute(self, cfg, start=1):
        with full_writes(self.full):
            self.gs.recompute(cfg, start, pkg.GATHER_ALL)

    def set_fd_filters(self, real=None, cmask=None):
        for i in range(2):
            self.gs.member(i).set_fd_filters(real, cmask)

    def set_rois(self, polys):
        self.gs.set_rois(polys)

    def poison(self):
        for i in range(2):
            m = self.gs.member(i)
            nx, ny = m.grid()[:2]
            nf = m.nt_out // 2 + 1
            for which, per in ((pkg.BUF_FFT, 2 * nf), (pkg.BUF_AMPLITUDES, nf)):
                ptr = self.gs.member_buffer(i, which)
                assert ptr
                junk = np.full(nx * ny * per, np.nan, np.float32)
                m.eng._check(m.eng.lib.thz_memcpy_h2d(m.eng.ctx, ptr, junk.ctypes.data, junk.nbytes))
            m.eng.sync()

    def snapshot(self):
        out = {w: self.gs.download(w) for w in PER_PIXEL + MEANS}
        r = self.gs.roi(0, want=["signal_fft", "signal"])
        out["roi_fft"], out["roi"], out["roi_n"] = r["signal_fft"], r["signal"], r["count"]
        return out

    def close(self):
        self.gs.close()


def same(a, b, step, nan_ok=False):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=nan_ok), f"step '{step}': {k} differs from the full-write session"


def sequence(time, cube, cube2):
    """(name, action(driver), cfg or None when the oracle does not model the step, cube) — cfg objects are copies"""
    nf = time.size // 2 + 1
    cfg = pkg.chain_cfg_default(time)
    steps = []

    def snap():
        c = pkg.ChainCfg()
        C.memmove(C.byref(c), C.byref(cfg), C.sizeof(c))
        return c

    def rec(name, oracle=True, start=1, which=cube):
        c = snap()
        steps.append((name, lambda d, c=c, start=start: d.recompute(c, start), c if oracle else None, which))

    rec("default band")
    cfg.fd_low, cfg.fd_high = 0.6, 2.5
    rec("narrower band")
    cfg.fd_low, cfg.fd_high = 0.1, 7.0
    rec("wider band")
    cfg.fd_low, cfg.fd_high = 7.5, 9.0
    rec("shifted band, no overlap")
    cfg.fd_low, cfg.fd_high = 0.2, 5.0
    rec("back to the default band")
    cfg.fd_active = 0
    rec("band pass off")
    cfg.fd_active = 1
    rec("band pass on again")
    notch = np.ones(nf, np.float32)
    notch[nf // 8:nf // 8 + 9] = 0.0
    notch[nf // 3] = 0.5
    steps.append(("K14 plugin set", lambda d: d.set_fd_filters(notch, None), None, None))
    rec("with a K14 real plugin", oracle=False)
    H = np.empty((nf, 2), np.float32)
    H[:, 0] = 0.8 + 0.1 * np.cos(np.arange(nf) * 0.03)
    H[:, 1] = 0.2 * np.sin(np.arange(nf) * 0.05)
    steps.append(("complex multiplier set", lambda d: d.set_fd_filters(None, H), None, None))
    rec("with a complex multiplier", oracle=False)
    cfg.fd_low, cfg.fd_high = 0.5, 3.0
    rec("complex multiplier, narrower band", oracle=False)
    steps.append(("multipliers cleared", lambda d: d.set_fd_filters(None, None), None, None))
    rec("multipliers cleared, same band")
    cfg.scale_factor = 2
    rec("scale factor 2", oracle=False)
    cfg.scale_factor = 1
    rec("scale factor 1 again")
    cfg.td_after_low = float(time[0]) + 2.0
    rec("tail only", start=6)
    cfg.fd_low, cfg.fd_high = 0.2, 5.0
    rec("default band after the tail")
    steps.append(("new upload", lambda d: d.upload(cube2), None, None))
    rec("after the new upload", which=cube2)
    cfg.fd_low, cfg.fd_high = 0.8, 2.0
    rec("narrower band on the new cube", which=cube2)
    steps.append(("poison", lambda d: d.poison(), None, None))
    rec("after the poison", which=cube2)
    cfg.fd_low, cfg.fd_high = 1.0, 1.8
    rec("narrower still", which=cube2)
    return steps


def pentagon(nx, ny):
    return np.array([[1, 1], [nx - 2, 0], [nx - 1, ny - 2], [nx // 2, ny - 1], [0, ny // 2]], np.int64)


def drive(make, nx, ny, nt, check_oracle):
    time, cube = synth.make_cube(nx, ny, nt)
    ids = np.arange(nx * ny, dtype=np.uint64) + 1000
    cube2 = synth.make_traces(ids, nt, subtract_bias=True).reshape(nx, ny, nt)
    a, b = make(time, False), make(time, True)
    try:
        for d in (a, b):
            d.upload(cube)
            d.set_rois([pentagon(nx, ny)])
        for name, act, cfg, which in sequence(time, cube, cube2):
            act(a)
            act(b)
            if which is None:
                continue   # a setter: the next recompute shows it
            same(a.snapshot(), b.snapshot(), name)
            if cfg is not None and check_oracle:
                check(a.s, oracle_chain(which, time, cfg), nx, ny)
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("shape", [(6, 8, 1024), (4, 6, 2048), (3, 6, 4096)])
def test_session_sequence_matches_full_writes_and_oracle(engine, shape):
    nx, ny, nt = shape
    drive(lambda time, full: One(engine, nx, ny, time, full), nx, ny, nt, True)


def test_group_of_two_sequence_matches_full_writes():
    nx, ny, nt = 8, 6, 1024
    with pkg.Group(devices=[0, 0]) as g:
        drive(lambda time, full: Two(g, nx, ny, time, full), nx, ny, nt, False)


@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_non_finite_trace_is_written_in_full_every_time(engine, bad):
    nx, ny, nt = 5, 4, 4096
    time, cube = synth.make_cube(nx, ny, nt)
    cube = cube.copy()
    cube[2, 1, nt // 5] = bad
    a, b = One(engine, nx, ny, time, False), One(engine, nx, ny, time, True)
    try:
        cfg = pkg.chain_cfg_default(time)
        for d in (a, b):
            d.upload(cube)
            d.set_rois([pentagon(nx, ny)])
        for i, band in enumerate([(0.2, 5.0), (0.6, 2.5), (0.2, 5.0)]):
            cfg.fd_low, cfg.fd_high = band
            a.recompute(cfg)
            b.recompute(cfg)
            sa, sb = a.snapshot(), b.snapshot()
            same(sa, sb, f"recompute {i}", nan_ok=True)
            nf = nt // 2 + 1
            row = sa[pkg.BUF_FFT].reshape(nx * ny, nf, 2)[2 * ny + 1]
            # (a component can stay finite — the imaginary parts of bin 0 and of the Nyquist bin are forced to zero, and
            # a bin reached through trivial twiddles only keeps one — but no bin is finite)
            assert not np.isfinite(row).all(axis=1).any(), "the bad trace's spectrum is non-finite in every bin, out of band too"
            assert not np.isfinite(sa[pkg.BUF_AMPLITUDES].reshape(nx * ny, nf)[2 * ny + 1]).any()
    finally:
        a.close()
        b.close()
