"""The fused F chain's keep range (fft_f.hpp: FArgs::keep_lo4 / keep_n) on the host-thread emulation: a launch told to
store only the bins [lo4, lo4 + n) of the spectrum and the amplitudes must leave every other bin of the two arrays
untouched, store inside the range what the full-write launch stores, bit for bit, and change nothing else — phases,
time traces, image and pixel sums.  A trace with a NaN or an Inf sample is written in full whatever the range says.

All three F plans (nt = 1024, 2048, 4096), real and complex multiplier, with and without the in-launch sums; the grid
is capped at one block of eight waves, so that the traces take it through several rounds, the last one ragged.

Builds its own shared object from the kernels, emu_harness.cpp and tests/emu/emu_keep_harness.cpp, once."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import synth

HERE = os.path.dirname(os.path.abspath(__file__))
EMU = os.path.join(HERE, "emu")
CSRC = os.path.join(HERE, "..", "thz_image_explorer_amd", "csrc")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
_P = C.c_void_p
SENT = np.float32(-12345.678)   # what the spectrum and the amplitudes hold before a launch
NPIX = 19                       # one block of 8 waves: rounds of 8, 8 and 3 traces


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    cxx = CLANG if os.path.exists(CLANG) else "g++"
    so = str(tmp_path_factory.mktemp("emu_keep") / "libthz_emu_keep.so")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-DTHZ_EMU", "-fPIC", "-shared", f"-I{EMU}", f"-I{CSRC}", "-x", "c++",
                        os.path.join(CSRC, "kernels.hip"), os.path.join(CSRC, "voxel.hip"), os.path.join(EMU, "emu_harness.cpp"),
                        os.path.join(EMU, "emu_keep_harness.cpp"), "-lpthread", "-lm", "-o", so],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout[-4000:]
    lib = C.CDLL(so)
    lib.emu_set_grid_cap(1)
    lib.emu_set_f_bar(3)
    return lib


def _p(a):
    return None if a is None else a.ctypes.data_as(_P)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _ranges(N):
    """(lo4, n) — multiples of 4, edges off the multiples of 128 and 256 wherever an edge is inside the row"""
    return {
        "from_bin_0": (0, 44),
        "to_bin_N": (N - 100, 104),          # reaches the Nyquist bin
        "no_whole_group": (200, 100),        # [200, 300): parts of two 128-bin stores and two 256-bin groups, none whole
        "default_band": (40, N // 2 - 36 + 4),
        "nyquist_only": (N, 4),
        "nothing": (N // 2 + 4, 0),
    }


def _inputs(nt, cmask):
    tm = synth.make_time(nt)
    rng = np.random.default_rng(nt + (7 if cmask else 0))
    x = rng.standard_normal((NPIX, nt)).astype(np.float32)
    x[5, nt // 3] = np.nan     # round 0
    x[17, 11] = np.inf         # the ragged last round
    chain = synth.default_chain(tm)
    nf = nt // 2 + 1
    H = None
    if cmask:
        H = np.empty((nf, 2), np.float32)
        H[:, 0] = 0.7 + 0.2 * np.cos(np.arange(nf) * 0.01)
        H[:, 1] = 0.3 * np.sin(np.arange(nf) * 0.02)
    nz = np.nonzero(chain["fd_mask"])[0]
    return x, chain, H, (int(nz[0]), int(nz[-1]) + 1)


def _launch(lib, nt, x, chain, H, band, sums, keep):
    nf = nt // 2 + 1
    fft = np.full((NPIX, nf, 2), SENT, np.float32)
    amp = np.full((NPIX, nf), SENT, np.float32)
    ph = np.full((NPIX, nf), np.nan, np.float32)
    out = np.full((NPIX, nt), np.nan, np.float32)
    img = np.full(NPIX, np.nan, np.float32)
    s = np.full(2 * nf, np.nan, np.float32) if sums else None
    lo4, n = keep if keep is not None else (0, -1)
    # the band goes along where it selects a kernel of its own: complex multiplier with the sums (kCfgBand at nt = 4096)
    b = band if (H is not None and sums) else (0, 0)
    rc = lib.emu_pipeline_keep(nt, C.c_size_t(NPIX), _p(x), _p(chain["w_pre"]), _p(chain["fd_mask"]), _p(H), _p(chain["w_post"]),
                               _p(fft), _p(amp), _p(ph), _p(out), _p(img), _p(s), b[0], b[1], lo4, n)
    assert rc >= 0, rc
    assert (rc > 0) == sums
    return fft, amp, ph, out, img, s


@pytest.mark.parametrize("sums", [False, True], ids=["nosums", "sums"])
@pytest.mark.parametrize("cmask", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("nt", [1024, 2048, 4096])
def test_keep_range_stores_exactly_its_bins(lib, nt, cmask, sums):
    N, nf = nt // 2, nt // 2 + 1
    x, chain, H, band = _inputs(nt, cmask)
    full = _launch(lib, nt, x, chain, H, band, sums, None)
    assert not (_bits(full[0]) == _bits(SENT)).any() and not (_bits(full[1]) == _bits(SENT)).any(), "a full write leaves no bin out"
    finite = np.isfinite(x).all(axis=1)
    assert (~finite).sum() == 2
    for name, (lo4, n) in _ranges(N).items():
        got = _launch(lib, nt, x, chain, H, band, sums, (lo4, n))
        inside = np.zeros(nf, bool)
        inside[lo4:min(lo4 + n, nf)] = True
        for what, g, f in (("spectrum", got[0], full[0]), ("amplitudes", got[1], full[1])):
            gb, fb = _bits(g), _bits(f)
            # finite traces: inside the range the full write's bits, outside the sentinel
            assert np.array_equal(gb[finite][:, inside], fb[finite][:, inside]), (name, what, "inside the range")
            assert (gb[finite][:, ~inside] == _bits(SENT)).all(), (name, what, "outside the range")
            # the NaN trace and the Inf trace: written in full
            assert np.array_equal(gb[~finite], fb[~finite]), (name, what, "non-finite traces")
        for what, g, f in (("phases", got[2], full[2]), ("data", got[3], full[3]), ("image", got[4], full[4])):
            assert np.array_equal(_bits(g), _bits(f)), (name, what)
        if sums:
            assert np.array_equal(_bits(got[5]), _bits(full[5])), (name, "sums")
