"""The fused F chain's kept phases (fft_f.hpp: a launch that is told its phase output already holds the phases runs the
kCfgKeepPhases form of the kCfgLow builds, without the arctangents, the unwrap, the phase store and the phase half of
the sums) on the host-thread emulation, nt = 4096.  A launch that computes phases is followed by one that is told to
keep them, on a phase array overwritten with a sentinel: no word of that array may change, and spectrum, amplitudes,
traces, image and amplitude sums must be the first launch's, word for word.  A launch that cannot keep them (a band
that does not fit the kCfgLow builds, no keep range) says so and writes phases.

19 traces through one block of eight waves (rounds of 8, 8 and 3), with a NaN trace, an Inf trace and an all-zero
trace; real and complex multiplier, with and without the in-launch sums; the default chain's band [40, 1028).

The block rows of a launch that keeps the phases are nf floats long (amplitude sums) and sit packed at the start of the
row buffer; the final pass writes the first nf floats of the sums.  What lies behind — the rest of the row buffer, the
phase half of the sums — must come back untouched.

Builds its own shared object from the kernels, emu_harness.cpp and tests/emu/emu_phases_harness.cpp, once."""
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
SENT = np.float32(-12345.678)   # spectrum and amplitudes before a launch; the phase array before the second launch
NPIX = 19                       # one block of 8 waves: rounds of 8, 8 and 3 traces
NT, N, NF = 4096, 2048, 2049
TOP = N // 2 + 128              # N/2 + M1: the last band / keep-range end the kCfgLow builds take
CFG_KEEP, CFG_LOW, CFG_KEEP_PHASES = 32, 64, 128   # fft_f.hpp
BAND = (40, 1028)               # the default chain's Frequency Band Pass, 0.2 - 5 THz


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    cxx = CLANG if os.path.exists(CLANG) else "g++"
    so = str(tmp_path_factory.mktemp("emu_phases") / "libthz_emu_phases.so")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-DTHZ_EMU", "-fPIC", "-shared", f"-I{EMU}", f"-I{CSRC}", "-x", "c++",
                        os.path.join(CSRC, "kernels.hip"), os.path.join(CSRC, "voxel.hip"), os.path.join(EMU, "emu_harness.cpp"),
                        os.path.join(EMU, "emu_phases_harness.cpp"), "-lpthread", "-lm", "-o", so],
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


def _inputs(cmask, clean):
    tm = synth.make_time(NT)
    rng = np.random.default_rng(2049 + (5 if cmask else 0))
    x = rng.standard_normal((NPIX, NT)).astype(np.float32)
    x[3] = 0.0                     # an all-zero trace
    if not clean:
        x[6, NT // 3] = np.nan     # round 0
        x[18, 7] = np.inf          # the ragged last round
    chain = synth.default_chain(tm)
    H = None
    if cmask:
        H = np.empty((NF, 2), np.float32)
        H[:, 0] = 0.7 + 0.2 * np.cos(np.arange(NF) * 0.01)
        H[:, 1] = 0.3 * np.sin(np.arange(NF) * 0.02)
    return x, chain, H


def _default_mask(chain):
    m = np.ascontiguousarray(chain["fd_mask"], np.float32)
    # (the band pass's own index range; its flanks reach zero a few bins inside it)
    assert m[BAND[0]:BAND[1]].any() and not m[:BAND[0]].any() and not m[BAND[1]:].any()
    return m


def _shifted_mask(band):
    m = np.zeros(NF, np.float32)
    k = np.arange(band[0], band[1])
    m[k] = (0.6 + 0.4 * np.cos(k * 0.013)).astype(np.float32)
    return m


def _launch(lib, x, chain, mask, H, band, sums, keep, keep_phases, ph=None):
    """-> (fft, amp, ph, out, img, sums, partial, rows), cfg bits, phases-kept record"""
    fft = np.full((NPIX, NF, 2), SENT, np.float32)
    amp = np.full((NPIX, NF), SENT, np.float32)
    if ph is None:
        ph = np.full((NPIX, NF), np.nan, np.float32)
    out = np.full((NPIX, NT), np.nan, np.float32)
    img = np.full(NPIX, np.nan, np.float32)
    s = partial = None
    if sums:
        rows = lib.emu_phases_sum_rows(NT, C.c_size_t(NPIX), int(H is not None), band[0], band[1])
        assert rows > 0, rows
        s = np.full(2 * NF, SENT, np.float32)
        partial = np.full(rows * 2 * NF, SENT, np.float32)
    lo4, n = keep if keep is not None else (0, -1)
    cfg, kept = C.c_int(-1), C.c_int(-1)
    rc = lib.emu_pipeline_phases(NT, C.c_size_t(NPIX), _p(x), _p(chain["w_pre"]), _p(mask), _p(H), _p(chain["w_post"]),
                                 _p(fft), _p(amp), _p(ph), _p(out), _p(img), _p(s), _p(partial), band[0], band[1], lo4, n,
                                 int(keep_phases), C.byref(cfg), C.byref(kept))
    assert rc >= 0, rc
    assert (rc > 0) == sums
    return (fft, amp, ph, out, img, s, partial, rc), cfg.value, kept.value


def _same_words(what, a, b):
    assert np.array_equal(_bits(a), _bits(b)), what


def _same_sums(what, a, b):
    """a NaN sum compares as a NaN: the two launches are different builds, and which operand's NaN an addition of two
    hands on is the host compiler's choice in each (the clean cube compares real sums)"""
    an, bn = np.isnan(a), np.isnan(b)
    assert np.array_equal(an, bn) and np.array_equal(_bits(a)[~an], _bits(b)[~bn]), what


def _keep_of(band):
    return (band[0] & ~3, ((band[1] + 3) & ~3) - (band[0] & ~3))


@pytest.mark.parametrize("clean", [False, True], ids=["nonfinite", "clean"])
@pytest.mark.parametrize("sums", [False, True], ids=["nosums", "sums"])
@pytest.mark.parametrize("cmask", [False, True], ids=["real", "complex"])
def test_kept_phases_launch_touches_no_phase_and_changes_nothing_else(lib, cmask, sums, clean):
    x, chain, H = _inputs(cmask, clean)
    mask = _default_mask(chain)
    keep = _keep_of(BAND)
    first, cfg1, kept1 = _launch(lib, x, chain, mask, H, BAND, sums, keep, False)
    assert cfg1 & CFG_KEEP and cfg1 & CFG_LOW and not cfg1 & CFG_KEEP_PHASES, cfg1
    assert kept1 == 0
    finite = np.isfinite(x).all(axis=1)
    assert np.isfinite(first[2][finite]).all(), "the first launch wrote phases"
    if sums:
        rows = first[7]
        assert not (_bits(first[6]) == _bits(SENT)).any(), "a launch that computes phases writes rows of 2 nf floats whole"
        assert not (_bits(first[5]) == _bits(SENT)).any()
        if clean:
            assert np.isfinite(first[5]).all()

    ph = np.full((NPIX, NF), SENT, np.float32)
    second, cfg2, kept2 = _launch(lib, x, chain, mask, H, BAND, sums, keep, True, ph=ph)
    assert cfg2 == cfg1, "the record of the build's bits leaves the phases bit out"
    assert kept2 == 1
    assert (_bits(second[2]) == _bits(SENT)).all(), "a word of the phase array was written"
    for what, i in (("spectrum", 0), ("amplitudes", 1), ("traces", 3), ("image", 4)):
        _same_words(what, second[i], first[i])
    if sums:
        _same_sums("amplitude sums", second[5][:NF], first[5][:NF])
        assert (_bits(second[5][NF:]) == _bits(SENT)).all(), "the phase half of the sums was written"
        got_rows = second[6][:rows * NF].reshape(rows, NF)
        want_rows = first[6].reshape(rows, 2 * NF)[:, :NF]
        _same_sums("the blocks' amplitude rows", got_rows, want_rows)
        assert (_bits(second[6][rows * NF:]) == _bits(SENT)).all(), "the launch wrote behind its rows of nf floats"


@pytest.mark.parametrize("sums", [False, True], ids=["nosums", "sums"])
@pytest.mark.parametrize("cmask", [False, True], ids=["real", "complex"])
def test_launch_that_cannot_keep_phases_writes_them(lib, cmask, sums):
    x, chain, H = _inputs(cmask, clean=True)
    # a band that ends four bins above N/2 + M1: the keep build, which has no form without phases
    band = (132, TOP + 4)
    mask = _shifted_mask(band)
    keep = _keep_of(band)
    ref, cfg_ref, _ = _launch(lib, x, chain, mask, H, band, sums, keep, False)
    ph = np.full((NPIX, NF), SENT, np.float32)
    got, cfg, kept = _launch(lib, x, chain, mask, H, band, sums, keep, True, ph=ph)
    assert cfg == cfg_ref and cfg & CFG_KEEP and not cfg & CFG_LOW, cfg
    assert kept == 0
    for i in range(5):
        _same_words(i, got[i], ref[i])
    if sums:
        _same_words("sums", got[5], ref[5])
    # no keep range: the launch writes everything, phases included, whatever it is told
    mask = _default_mask(chain)
    band_arg = BAND if (cmask and sums) else (0, 0)
    ref, cfg_ref, _ = _launch(lib, x, chain, mask, H, band_arg, sums, None, False)
    ph = np.full((NPIX, NF), SENT, np.float32)
    got, cfg, kept = _launch(lib, x, chain, mask, H, band_arg, sums, None, True, ph=ph)
    assert cfg == cfg_ref and not cfg & (CFG_KEEP | CFG_LOW), cfg
    assert kept == 0
    assert not (_bits(got[2]) == _bits(SENT)).any()
    for i in range(5):
        _same_words(i, got[i], ref[i])
    if sums:
        _same_words("sums", got[5], ref[5])
