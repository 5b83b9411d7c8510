"""GroupSession.roi() / download() size their host arrays like the chain's OUTPUT traces.

A tilt extends the traces to nt_out = nt + 2 * steps, and thz_group_session_roi / thz_group_session_download write
nt_out-long vectors (and nt_out / 2 + 1 bins) into the caller's memory: the C calls take no length.  These tests drive
the binding with a stub library and a stub member that reports nt_out = nt + 6, so nothing is written anywhere: every
array the binding hands to the library must be sized from nt_out unless the caller passes nt_out itself."""
import ctypes as C

import numpy as np

import thz_image_explorer_amd as pkg
from thz_image_explorer_amd.binding import THZ_OK, GroupSession

NX, NY, NT, EXTRA = 5, 3, 64, 6


class _StubLib:
    """records what the binding hands over; writes nothing through the pointers"""

    def __init__(self):
        self.calls = []

    def thz_group_session_grid(self, h, nx, ny):
        nx._obj.value, ny._obj.value = NX, NY
        return THZ_OK

    def thz_group_session_roi(self, h, index, ro):
        r = ro._obj
        self.calls.append(("roi", index, {k: getattr(r, k) for k in ("signal_fft", "phase_fft", "signal", "roi_data")}))
        return THZ_OK

    def thz_group_session_download(self, h, which, pix0, npix, out):
        self.calls.append(("download", which, pix0, npix, out))
        return THZ_OK

    def thz_group_last_error(self, h):
        return b"stub"


class _StubGroup:
    def __init__(self, lib):
        self.lib, self.world, self.ranks = lib, 1, [0]

    def _check(self, rc):
        assert rc == THZ_OK


class _StubMember:
    nt_out = NT + EXTRA


def _group_session():
    lib = _StubLib()
    gs = GroupSession.__new__(GroupSession)
    gs.g, gs.nx, gs.ny, gs.nt, gs.h = _StubGroup(lib), NX, NY, NT, C.c_void_p(1)
    gs.member = lambda i: _StubMember()
    return gs, lib


def test_group_roi_arrays_follow_nt_out():
    gs, lib = _group_session()
    nto = NT + EXTRA
    nf = nto // 2 + 1
    res = gs.roi(0)
    (_, index, ptrs), = lib.calls
    assert index == 0
    want = dict(signal_fft=nf, phase_fft=nf, signal=nto, roi_data=nto)
    for key, n in want.items():
        assert res[key].shape == (n,), key
        assert ptrs[key] == res[key].ctypes.data, key   # the array handed over is the one returned
    # a subset, and an explicit nt_out, are honoured as before
    res = gs.roi(0, want=["signal"])
    assert set(res) == {"signal", "count"} and res["signal"].shape == (nto,)
    assert gs.roi(0, nt_out=NT)["roi_data"].shape == (NT,)


def test_group_download_arrays_follow_nt_out():
    gs, lib = _group_session()
    nto = NT + EXTRA
    nf = nto // 2 + 1
    npix = NX * NY
    want = {pkg.BUF_IMG: (npix,), pkg.BUF_DATA: (npix, nto), pkg.BUF_FFT: (npix, nf, 2), pkg.BUF_AMPLITUDES: (npix, nf),
            pkg.BUF_PHASES: (npix, nf), pkg.BUF_AVG_FFT: (nf, 2), pkg.BUF_AVG_AMPLITUDES: (nf,), pkg.BUF_AVG_PHASES: (nf,)}
    for which, shape in want.items():
        lib.calls.clear()
        out = gs.download(which)
        (_, w, pix0, n, ptr), = lib.calls
        assert w == which and pix0 == 0
        assert out.shape == shape and out.dtype == np.float32, (which, out.shape, shape)
        assert ptr == out.ctypes.data, which
        assert n == (npix if which in (pkg.BUF_IMG, pkg.BUF_DATA, pkg.BUF_FFT, pkg.BUF_AMPLITUDES, pkg.BUF_PHASES) else 1)
    # an explicit nt_out is honoured as before
    assert gs.download(pkg.BUF_DATA, nt_out=NT).shape == (npix, NT)
    assert gs.download(pkg.BUF_AVG_AMPLITUDES, nt_out=NT).shape == (NT // 2 + 1,)
