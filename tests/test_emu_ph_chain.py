"""The half-length chain with its extras (fft_ph.hpp: k_ph<P, kPipe, CM, SUMS>) on the host-thread emulation: the complex
per-bin multiplier and the pixel sums inside the one launch of a 2002-, 2400-, 3000- or 4000-sample scan.

emu_harness.cpp's fused entry points know the F and P families only, so this module builds its own shared object from
the kernels, that harness and tests/emu/emu_ph_harness.cpp, once.  That harness names the instantiations
k_ph<P, kPipe, CM, SUMS> itself: without the two template parameters it does not compile."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import oracle_binding as ob
import synth
import trace_isolation as ti
from test_gpu_parity import phase_ok
from test_gpu_trace_isolation import _wiener_cmask

HERE = os.path.dirname(os.path.abspath(__file__))
EMU = os.path.join(HERE, "emu")
CSRC = os.path.join(HERE, "..", "thz_image_explorer_amd", "csrc")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
_P = C.c_void_p
SUM_TOL = 2e-6   # include/thzgpu.h, d_sums: the in-launch sums against the sequential ones
MODES = ("cmask", "sums", "cmask+sums")
NAMES = ("fft", "amp", "ph", "out", "img")

# nt, traces: one trace and N odd (the ragged last entry of the inverse); more traces than the block's 12 waves
# (3000: 11 with the sums) and than its 8 (4000)
CASES = [(2002, 1), (2002, 5), (2400, 3), (3000, 14), (4000, 9)]


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    cxx = CLANG if os.path.exists(CLANG) else "g++"
    so = str(tmp_path_factory.mktemp("emu_ph") / "libthz_emu_ph.so")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-DTHZ_EMU", "-fPIC", "-shared", f"-I{EMU}", f"-I{CSRC}", "-x", "c++",
                        os.path.join(CSRC, "kernels.hip"), os.path.join(CSRC, "voxel.hip"), os.path.join(EMU, "emu_harness.cpp"),
                        os.path.join(EMU, "emu_ph_harness.cpp"), "-lpthread", "-lm", "-o", so],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout[-4000:]
    lib = C.CDLL(so)
    lib.emu_allow_f(1)
    lib.emu_allow_p(1)
    lib.emu_set_grid_cap(0)
    return lib


def _p(a):
    return None if a is None else a.ctypes.data_as(_P)


@functools.lru_cache(maxsize=None)
def _case(nt, npix):
    """inputs and references of a case, computed once and left unchanged: the numpy fp64 model of
    test_fused_pipeline_ex with and without the multiplier, and the oracle's phases of X"""
    time, cube = synth.make_cube(npix, 1, nt)
    chain_p, chain = synth.default_chain(time), synth.oracle_chain(time)
    nf = nt // 2 + 1
    H = _wiener_cmask(time, nf)
    x = np.ascontiguousarray(cube.reshape(npix, nt), np.float32)
    pre = chain["w_tilt"].astype(np.float64) * chain["w_td_before"] * chain["w_fft"]
    refs = {}
    for key, h in (("plain", None), ("cmask", H)):
        ref = ti.forward_ref(x, pre, chain["fd_mask"], h)
        y, en = ti.inverse_ref(ref["fft"], nt, chain["w_post"])
        refs[key] = dict(ref, out=y, img=en)
    oracle = ob.run_pipeline(cube, time, chain)
    st = ob.fft_stage(cube * chain["w_tilt"] * chain["w_td_before"], time, 0, 1.0, 7.0)
    for a in (x, H):
        a.setflags(write=False)
    return dict(x=x, H=H, chain=chain_p, refs=refs, ph=oracle["phases"], amp_x=st["amplitudes"])


def _launch(lib, nt, c, mode, direct=1):
    """one launch: (fft, amp, ph, out, img, sums or None, rows)"""
    npix, nf = c["x"].shape[0], nt // 2 + 1
    o = [np.full((npix, nf, 2), np.nan, np.float32), np.full((npix, nf), np.nan, np.float32),
         np.full((npix, nf), np.nan, np.float32), np.full((npix, nt), np.nan, np.float32), np.full(npix, np.nan, np.float32)]
    s = np.full(2 * nf, np.nan, np.float32) if "sums" in mode else None
    ch = c["chain"]
    rc = lib.emu_ph_chain(nt, C.c_size_t(npix), direct, _p(c["x"]), _p(ch["w_pre"]), _p(ch["fd_mask"]),
                          _p(c["H"]) if "cmask" in mode else None, _p(ch["w_post"]), *[_p(a) for a in o], _p(s))
    assert rc >= 0, rc   # -4: a partial-row entry was never written, -5: the launcher's rows are not the grid's
    assert (rc > 0) == ("sums" in mode)
    return (*o, s, rc)


def _check(lib, nt, npix, mode, c):
    nf = nt // 2 + 1
    fft, amp, ph, out, img, s, rows = _launch(lib, nt, c, mode)
    ref = c["refs"]["cmask" if "cmask" in mode else "plain"]
    live = ["live"] * npix
    bad = ti.check("fft", ti.as_complex(fft), ref["fft"], live) + ti.check("amp", amp, ref["amp"], live)
    bad += ti.check("out", out, ref["out"], live) + ti.check_intensity(img, ref["img"], live)
    assert not bad, "; ".join(bad[:12])
    assert phase_ok(ph.reshape(npix, 1, nf), c["ph"], c["amp_x"])   # the phases are those of X in every mode
    # C2R precondition: bins 0 and N are real, with a positive zero
    for k in (0, -1):
        assert np.all(fft[:, k, 1] == 0.0) and not np.signbit(fft[:, k, 1]).any()
    if s is not None:
        a64, p64 = amp.astype(np.float64).sum(0), ph.astype(np.float64).sum(0)
        assert np.isfinite(s).all()
        assert np.abs(s[:nf] - a64).max() <= SUM_TOL * np.abs(a64).max()
        assert np.abs(s[nf:] - p64).max() <= SUM_TOL * np.abs(p64).max()
    # a second launch — through launch_pipeline, as thz_pipeline_ex issues it — gives the same bits
    again = _launch(lib, nt, c, mode, direct=0)
    assert again[6] == rows
    for name, a, b in zip(NAMES + ("sums",), (fft, amp, ph, out, img, s), again):
        assert (a is None and b is None) or np.array_equal(a, b), name
    if mode == "sums":
        # without a multiplier the accumulators ride along: every array is the plain k_ph<P, kPipe>'s bit for bit
        plain = _launch(lib, nt, c, "plain")
        for name, a, b in zip(NAMES, (fft, amp, ph, out, img), plain):
            assert np.array_equal(a, b), name
    if mode == "cmask+sums":
        # ... and the multiplier alone is the same launch without the accumulators
        only = _launch(lib, nt, c, "cmask")
        for name, a, b in zip(NAMES, (fft, amp, ph, out, img), only):
            assert np.array_equal(a, b), name
    return rows


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("nt,npix", CASES)
def test_ph_chain_extras(lib, nt, npix, mode):
    assert lib.emu_half_n(nt) == nt // 2
    rows = _check(lib, nt, npix, mode, _case(nt, npix))
    if "sums" in mode:
        w = lib.emu_ph_waves(nt, 1)
        assert rows == -(-npix // w)   # one row per block


def test_waves_per_block(lib):
    """the plain chain keeps its waves; the accumulators cost N = 1500 its twelfth"""
    assert [lib.emu_ph_waves(nt, 0) for nt in (2002, 2400, 3000, 4000)] == [16, 12, 12, 8]
    assert [lib.emu_ph_waves(nt, 1) for nt in (2002, 2400, 3000, 4000)] == [16, 12, 11, 8]


@pytest.mark.parametrize("mode", MODES)
def test_one_block_three_trips_ragged_last(lib, mode):
    """nt = 4000 on ONE block: 2 x 8 + 3 = 19 traces, every wave takes three trips and the last trip is ragged — the
    ticket order across trips, and waves that stay away from the last one"""
    nt = 4000
    w = lib.emu_ph_waves(nt, 1)
    npix = 2 * w + 3
    assert npix == 19
    lib.emu_set_grid_cap(1)
    try:
        rows = _check(lib, nt, npix, mode, _case(nt, npix))
    finally:
        lib.emu_set_grid_cap(0)
    if "sums" in mode:
        assert rows == 1
