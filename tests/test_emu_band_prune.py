"""The fused F chain's band pruning (fft_f.hpp: a launch with a keep range that is also told where its multiplier is
zero, both ending at or below bin N/2 + M1, runs the kCfgLow build, whose f_inverse_input leaves out the products with
those zeros) on the host-thread emulation, nt = 4096.  Every pruned launch is compared with the full-write launch of the same inputs: spectrum and amplitudes
inside the keep range, phases, sums and image bit for bit; time traces as floats, and bit for bit wherever the sample
is not zero (the pruned form takes X H where the full one adds a product +-0 to it: the sign of an exact zero is the
one thing that may differ).  Non-finite traces are computed and written in full.

Real and complex multiplier, with and without the in-launch sums; the grid is capped at one block of eight waves, so
that the 19 traces take it through rounds of 8, 8 and 3.  Which build ran is read back from the launcher.

Builds its own shared object from the kernels, emu_harness.cpp and tests/emu/emu_prune_harness.cpp, once."""
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
NT, N, NF = 4096, 2048, 2049
TOP = N // 2 + 128              # N/2 + M1: the last band / keep-range end the kCfgLow build takes
CFG_KEEP, CFG_LOW = 32, 64      # fft_f.hpp


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    cxx = CLANG if os.path.exists(CLANG) else "g++"
    so = str(tmp_path_factory.mktemp("emu_prune") / "libthz_emu_prune.so")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-DTHZ_EMU", "-fPIC", "-shared", f"-I{EMU}", f"-I{CSRC}", "-x", "c++",
                        os.path.join(CSRC, "kernels.hip"), os.path.join(CSRC, "voxel.hip"), os.path.join(EMU, "emu_harness.cpp"),
                        os.path.join(EMU, "emu_prune_harness.cpp"), "-lpthread", "-lm", "-o", so],
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


# name: (band [lo, hi), keep range (lo4, n), the kCfgLow build must run)
CASES = {
    "default_band": (None, None, True),                        # the default chain's own band, the range its hull
    "from_bin_0": ((0, 700), (0, 700), True),
    "ends_at_top": ((128, TOP), (128, TOP - 128), True),       # the last band that qualifies (1024 bins: the band-limited
                                                               # table of the complex multiplier with sums still holds it)
    "four_past_top": ((132, TOP + 4), (132, TOP - 128), False),  # takes the keep build
    "edges_inside": ((330, 843), (328, 516), True),            # inside groups and inside 128-bin j1 blocks
    "range_wider": ((300, 900), (200, TOP - 200), True),       # zeros stored where the range asks; group 0 left out
    "range_to_N": ((300, 900), (200, NF + 3 - 200), False),    # range past the top: takes the keep build
}


def _inputs(cmask, clean):
    tm = synth.make_time(NT)
    rng = np.random.default_rng(4096 + (7 if cmask else 0))
    x = rng.standard_normal((NPIX, NT)).astype(np.float32)
    x[3] = 0.0                     # an all-zero trace
    if not clean:
        x[5, NT // 3] = np.nan     # round 0
        x[17, 11] = np.inf         # the ragged last round
    chain = synth.default_chain(tm)
    H = None
    if cmask:
        H = np.empty((NF, 2), np.float32)
        H[:, 0] = 0.7 + 0.2 * np.cos(np.arange(NF) * 0.01)
        H[:, 1] = 0.3 * np.sin(np.arange(NF) * 0.02)
    return x, chain, H


def _mask(chain, band):
    """a real multiplier that is +0 outside the band and not zero inside"""
    if band is None:
        m = np.ascontiguousarray(chain["fd_mask"], np.float32)
        nz = np.nonzero(m)[0]
        band = (int(nz[0]), int(nz[-1]) + 1)
        assert band[1] <= TOP and not m[:band[0]].any() and not m[band[1]:].any()
        return m, band
    m = np.zeros(NF, np.float32)
    k = np.arange(band[0], band[1])
    m[k] = (0.6 + 0.4 * np.cos(k * 0.013)).astype(np.float32)
    return m, band


def _launch(lib, x, chain, mask, H, band, sums, keep):
    fft = np.full((NPIX, NF, 2), SENT, np.float32)
    amp = np.full((NPIX, NF), SENT, np.float32)
    ph = np.full((NPIX, NF), np.nan, np.float32)
    out = np.full((NPIX, NT), np.nan, np.float32)
    img = np.full(NPIX, np.nan, np.float32)
    s = np.full(2 * NF, np.nan, np.float32) if sums else None
    lo4, n = keep if keep is not None else (0, -1)
    cfg = C.c_int(-1)
    rc = lib.emu_pipeline_prune(NT, C.c_size_t(NPIX), _p(x), _p(chain["w_pre"]), _p(mask), _p(H), _p(chain["w_post"]),
                                _p(fft), _p(amp), _p(ph), _p(out), _p(img), _p(s), band[0], band[1], lo4, n, C.byref(cfg))
    assert rc >= 0, rc
    assert (rc > 0) == sums
    return (fft, amp, ph, out, img, s), cfg.value


def _compare(name, got, full, keep, finite, sums):
    lo4, n = keep
    inside = np.zeros(NF, bool)
    inside[lo4:min(lo4 + n, NF)] = True
    for what, g, f in (("spectrum", got[0], full[0]), ("amplitudes", got[1], full[1])):
        gb, fb = _bits(g), _bits(f)
        assert np.array_equal(gb[finite][:, inside], fb[finite][:, inside]), (name, what, "inside the range")
        assert (gb[finite][:, ~inside] == _bits(SENT)).all(), (name, what, "outside the range")
        assert np.array_equal(gb[~finite], fb[~finite]), (name, what, "non-finite traces")
    for what, g, f in (("phases", got[2], full[2]), ("image", got[4], full[4])):
        assert np.array_equal(_bits(g), _bits(f)), (name, what)
    g, f = got[3], full[3]
    assert np.array_equal(g, f, equal_nan=True), (name, "data as floats")
    nz = (f != 0) | (g != 0)
    assert np.array_equal(_bits(g)[nz], _bits(f)[nz]), (name, "data, bits of the samples that are not zero")
    assert np.array_equal(_bits(g)[~finite], _bits(f)[~finite]), (name, "data of the non-finite traces")
    assert not g[3].any() and not got[1][3][inside].any() and not got[0][3][inside].any(), (name, "the all-zero trace")
    if sums:
        # a NaN sum compares as a NaN: the two launches are different builds, and which operand's NaN an addition of
        # two hands on is the host compiler's choice in each (test_pruned_sums_of_finite_traces compares real sums)
        gn, fn = np.isnan(got[5]), np.isnan(full[5])
        assert np.array_equal(gn, fn) and np.array_equal(_bits(got[5])[~gn], _bits(full[5])[~fn]), (name, "sums")


@pytest.mark.parametrize("sums", [False, True], ids=["nosums", "sums"])
@pytest.mark.parametrize("cmask", [False, True], ids=["real", "complex"])
def test_pruned_launch_equals_the_full_write(lib, cmask, sums):
    x, chain, H = _inputs(cmask, clean=False)
    finite = np.isfinite(x).all(axis=1)
    assert (~finite).sum() == 2
    for name, (band, keep, low) in CASES.items():
        mask, band = _mask(chain, band)
        if keep is None:
            keep = (band[0] & ~3, ((band[1] + 3) & ~3) - (band[0] & ~3))
        # the full write: the band goes along only where it selects the table of its own (complex multiplier with sums)
        full, cfg_full = _launch(lib, x, chain, mask, H, band if (cmask and sums) else (0, 0), sums, None)
        assert not cfg_full & (CFG_KEEP | CFG_LOW), name
        assert not (_bits(full[0]) == _bits(SENT)).any() and not (_bits(full[1]) == _bits(SENT)).any(), "a full write leaves no bin out"
        got, cfg = _launch(lib, x, chain, mask, H, band, sums, keep)
        assert cfg & CFG_KEEP and bool(cfg & CFG_LOW) == low, (name, cfg)
        _compare(name, got, full, keep, finite, sums)
        if not low:
            continue
        # the same launch without the band: the keep build, nothing pruned — the same bits
        if not (cmask and sums):
            plain, cfg_plain = _launch(lib, x, chain, mask, H, (0, 0), sums, keep)
            assert cfg_plain & CFG_KEEP and not cfg_plain & CFG_LOW, name
            _compare(name + " (keep build)", plain, full, keep, finite, sums)


@pytest.mark.parametrize("cmask", [False, True], ids=["real", "complex"])
def test_pruned_sums_of_finite_traces(lib, cmask):
    """the sums of a cube without a NaN (a non-finite trace makes every sum NaN, which compares nothing)"""
    x, chain, H = _inputs(cmask, clean=True)
    finite = np.ones(NPIX, bool)
    for name in ("default_band", "edges_inside", "range_wider", "range_to_N"):
        band, keep, low = CASES[name]
        mask, band = _mask(chain, band)
        if keep is None:
            keep = (band[0] & ~3, ((band[1] + 3) & ~3) - (band[0] & ~3))
        full, _ = _launch(lib, x, chain, mask, H, band if cmask else (0, 0), True, None)
        assert np.isfinite(full[5]).all()
        got, cfg = _launch(lib, x, chain, mask, H, band, True, keep)
        assert bool(cfg & CFG_LOW) == low, (name, cfg)
        _compare(name, got, full, keep, finite, True)


def test_multiplier_of_minus_zero_outside_the_band(lib):
    """a real plugin that is negative outside the band makes the multiplier -0 there: still a zero, the session keeps
    its range and the launch is pruned; the amplitudes a range wider than the band asks for are the full write's -0"""
    x, chain, _ = _inputs(False, clean=False)
    finite = np.isfinite(x).all(axis=1)
    mask, band = _mask(chain, (300, 900))
    mask[mask == 0] = np.float32(-0.0)
    keep = (200, TOP - 200)
    full, _ = _launch(lib, x, chain, mask, None, (0, 0), False, None)
    assert np.signbit(full[1][0, 250]) and full[1][0, 250] == 0, "the full write stores |X| * -0"
    got, cfg = _launch(lib, x, chain, mask, None, band, False, keep)
    assert cfg & CFG_LOW
    _compare("minus zero", got, full, keep, finite, False)
