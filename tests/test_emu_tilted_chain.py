"""The tilted chain as ONE launch (fft_fbp.hpp: k_fbp<kPipe, TILT, CM, SUMS>) on the host-thread emulation: the Tilt
stage's re-laying as a gather in the forward loads, the complex multiplier and the pixel sums inside the launch, and the
sum of the re-laid source traces — 1001-sample cubes tilted onto both convolution lengths (M = 2304 / 2560).

emu_harness.cpp's fused entry points know the F and P families only, so this module builds its own shared object from
the kernels, that harness and tests/emu/emu_tilted_harness.cpp, once."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle_binding as ob
import synth
import thz_image_explorer_amd as pkg
import trace_isolation as ti
from test_gpu_trace_isolation import _wiener_cmask

HERE = os.path.dirname(os.path.abspath(__file__))
EMU = os.path.join(HERE, "emu")
CSRC = os.path.join(HERE, "..", "thz_image_explorer_amd", "csrc")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
_P = C.c_void_p
SUM_TOL = 2e-6   # include/thzgpu.h, d_sums: the in-launch sums against the sequential ones

# grid, dx = dy (mm), tilt (degrees), steps, nt_out, M — the plan of the CPU oracle for a 1001-sample scan
CASES = [((4, 4), 5.0, (2.0, 0.0), 23, 1047, 2304),
         ((4, 4), 5.0, (4.0, 3.5), 87, 1175, 2560),
         ((9, 7), 3.0, (-2.5, 2.0), 63, 1127, 2304),      # an odd pixel count
         ((16, 12), 2.0, (3.0, -1.5), 76, 1153, 2560)]    # 96 pairs: more than a block has waves


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    cxx = CLANG if os.path.exists(CLANG) else "g++"
    so = str(tmp_path_factory.mktemp("emu_tilted") / "libthz_emu_tilted.so")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-DTHZ_EMU", "-fPIC", "-shared", f"-I{EMU}", f"-I{CSRC}", "-x", "c++",
                        os.path.join(CSRC, "kernels.hip"), os.path.join(CSRC, "voxel.hip"), os.path.join(EMU, "emu_harness.cpp"),
                        os.path.join(EMU, "emu_tilted_harness.cpp"), "-lpthread", "-lm", "-o", so],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout[-4000:]
    lib = C.CDLL(so)
    lib.emu_allow_f(1)
    lib.emu_allow_p(1)
    lib.emu_set_grid_cap(0)
    return lib


def _p(a):
    return None if a is None else a.ctypes.data_as(_P)


def _outputs(npix, nt):
    nf = nt // 2 + 1
    return [np.full((npix, nf, 2), np.nan, np.float32), np.full((npix, nf), np.nan, np.float32),
            np.full((npix, nf), np.nan, np.float32), np.full((npix, nt), np.nan, np.float32), np.full(npix, np.nan, np.float32)]


def _tilted(lib, nt, x, taper, ins, chain, cmask=None, sums=False, src_sum=False):
    """one tilted launch: (fft, amp, ph, out, img, sums, src_sum, rows)"""
    npix, nt_in = x.shape
    o = _outputs(npix, nt)
    s = np.full(2 * (nt // 2 + 1), np.nan, np.float32) if sums else None
    ss = np.full(nt, np.nan, np.float32) if src_sum else None
    rc = lib.emu_fbp_chain(nt, C.c_size_t(npix), None, _p(x), nt_in, _p(taper), _p(ins), _p(chain["w_pre"]), _p(chain["fd_mask"]),
                           _p(cmask), _p(chain["w_post"]), *[_p(a) for a in o], _p(s), _p(ss))
    assert rc >= 0, rc   # -4: a partial-row entry was never written
    assert (rc > 0) == sums
    return (*o, s, ss, rc)


def _staged(lib, nt, x, taper, ins, chain):
    """emu_tilt into an extended cube, then the fused launch on it"""
    npix, nt_in = x.shape
    ext = np.full((npix, nt), np.nan, np.float32)
    assert lib.emu_tilt(C.c_size_t(npix), nt_in, nt, _p(x), _p(taper), _p(ins), _p(ext)) == 0
    o = _outputs(npix, nt)
    assert lib.emu_pipeline(nt, C.c_size_t(npix), _p(ext), _p(chain["w_pre"]), _p(chain["fd_mask"]), _p(chain["w_post"]),
                            *[_p(a) for a in o]) == 0
    return ext, o


def _relay(x, taper, ins, nt):
    """the Tilt stage's per-pixel copy (tilt_compensation.rs:171-201) in f32"""
    ext = np.zeros((x.shape[0], nt), np.float32)
    for p, i in enumerate(ins):
        n = min(x.shape[1], nt - i)
        ext[p, :i] = x[p, 0]
        ext[p, i:i + n] = (x[p] * taper)[:n]
    return ext


def _check_sums(tag, s, amp, ph, nf):
    a64, p64 = amp.astype(np.float64).sum(0), ph.astype(np.float64).sum(0)
    assert np.abs(s[:nf] - a64).max() <= SUM_TOL * np.abs(a64).max(), tag
    assert np.abs(s[nf:] - p64).max() <= SUM_TOL * np.abs(p64).max(), tag


def _case(grid, d, tilt):
    nx, ny = grid
    time, cube = synth.make_cube(nx, ny, 1001)
    steps, new_time, ins = pkg.host_tilt_plan(time, nx, ny, tilt[0], tilt[1], d, d)
    taper = pkg.host_adapted_blackman(time, 0.0, 7.0)
    x = np.ascontiguousarray(cube.reshape(nx * ny, 1001), np.float32)
    return time, cube, x, int(steps), new_time, np.ascontiguousarray(ins, np.int32), taper


@pytest.mark.parametrize("grid,d,tilt,steps,nt_out,M", CASES)
def test_tilted_launch(lib, grid, d, tilt, steps, nt_out, M):
    time, cube, x, got_steps, new_time, ins, taper = _case(grid, d, tilt)
    assert got_steps == steps and new_time.size == nt_out and (nt_out <= 1152) == (M == 2304)
    assert lib.emu_family(nt_out) == 7
    assert ins.min() >= 0 and ins.max() <= 2 * steps and len(set(ins.tolist())) > 1   # pairs with two insert indices
    nf = nt_out // 2 + 1
    chain = synth.default_chain(new_time)

    # 1. the gathering launch is the staged path bit for bit — with and without the sums riding along
    ext, st = _staged(lib, nt_out, x, taper, ins, chain)
    plain = _tilted(lib, nt_out, x, taper, ins, chain)
    summed = _tilted(lib, nt_out, x, taper, ins, chain, sums=True, src_sum=True)
    for name, a, b, c in zip(("fft", "amp", "ph", "out", "img"), st, plain, summed):
        assert np.array_equal(a, b), name
        assert np.array_equal(a, c), name + " (sums)"
    o_steps, o_time, o_ext = ob.tilt(cube, time, tilt[0], tilt[1], d, d)
    assert o_steps == steps and np.array_equal(o_ext.reshape(ext.shape), ext)

    # 3. sums of what the same launch stored; the re-laid traces' own sum
    _check_sums("plain", summed[5], summed[1], summed[2], nf)
    e64 = o_ext.reshape(ext.shape).astype(np.float64).sum(0)
    assert np.abs(summed[6] - e64).max() <= SUM_TOL * np.abs(e64).max()

    # 2. complex multiplier (and sums): every trace against float64 of X m H and its inverse
    H = _wiener_cmask(new_time, nf)
    fft, amp, ph, out, img, s, ss, rows = _tilted(lib, nt_out, x, taper, ins, chain, cmask=H, sums=True, src_sum=True)
    live = ["live"] * x.shape[0]
    ref = ti.forward_ref(ext * chain["w_pre"], None, chain["fd_mask"], H)
    y, en = ti.inverse_ref(ref["fft"], nt_out, chain["w_post"])
    bad = ti.check("fft", ti.as_complex(fft), ref["fft"], live) + ti.check("amp", amp, ref["amp"], live)
    bad += ti.check("out", out, y, live) + ti.check_intensity(img, en, live) + ti.check_phases(ph, ref, live, factors=None)
    assert not bad, "; ".join(bad[:12])
    assert np.array_equal(ph, st[2])   # the phases are those of X: the multiplier does not touch them
    assert np.all(fft[:, 0, 1] == 0.0) and not np.signbit(fft[:, 0, 1]).any()
    if nt_out % 2 == 0:
        assert np.all(fft[:, -1, 1] == 0.0) and not np.signbit(fft[:, -1, 1]).any()
    _check_sums("cmask", s, amp, ph, nf)
    assert np.array_equal(ss, summed[6])
    # the multiplier alone is the same launch without the accumulators
    only = _tilted(lib, nt_out, x, taper, ins, chain, cmask=H)
    for name, a, b in zip(("fft", "amp", "ph", "out", "img"), (fft, amp, ph, out, img), only):
        assert np.array_equal(a, b), name


def test_untilted_fused_chain_takes_the_multiplier_and_the_sums(lib):
    """thz_pipeline_ex on an FBP plan: the same variants without the gather"""
    nt, n = 1101, 9
    nf = nt // 2 + 1
    time = synth.make_time(nt)
    chain = synth.default_chain(time)
    x = np.ascontiguousarray(synth.make_traces(np.arange(n) + 3, nt), np.float32)
    H = _wiener_cmask(time, nf)
    o = _outputs(n, nt)
    s = np.full(2 * nf, np.nan, np.float32)
    rc = lib.emu_fbp_chain(nt, C.c_size_t(n), _p(x), None, 0, None, None, _p(chain["w_pre"]), _p(chain["fd_mask"]), _p(H),
                           _p(chain["w_post"]), *[_p(a) for a in o], _p(s), None)
    assert rc > 0, rc
    fft, amp, ph, out, img = o
    st = ["live"] * n
    ref = ti.forward_ref(x * chain["w_pre"], None, chain["fd_mask"], H)
    y, en = ti.inverse_ref(ref["fft"], nt, chain["w_post"])
    bad = ti.check("fft", ti.as_complex(fft), ref["fft"], st) + ti.check("amp", amp, ref["amp"], st)
    bad += ti.check("out", out, y, st) + ti.check_intensity(img, en, st)
    assert not bad, "; ".join(bad[:12])
    _check_sums("untilted", s, amp, ph, nf)


@pytest.mark.parametrize("steps", [50, 100])   # 1101 samples (M = 2304), 1201 (M = 2560)
def test_every_tilted_trace_to_its_own_scale(lib, steps):
    """partners 1e6 apart, a zero trace, NaN / Inf traces through the tilted launch with multiplier and sums"""
    nt_in, nt = 1001, 1001 + 2 * steps
    nf = nt // 2 + 1
    assert lib.emu_family(nt) == 7
    time = synth.make_time(nt_in)
    new_time = synth.make_time(nt)
    chain = synth.default_chain(new_time)
    taper = pkg.host_adapted_blackman(time, 0.0, 7.0)
    x = ti.make_cube(nt_in)
    ins = np.ascontiguousarray((np.arange(x.shape[0]) * 7) % (2 * steps + 1), np.int32)
    H = _wiener_cmask(new_time, nf)
    fft, amp, ph, out, img, s, ss, rows = _tilted(lib, nt, x, taper, ins, chain, cmask=H, sums=True, src_sum=True)
    st = ti.status()
    ext = _relay(x, taper, ins, nt)
    ref = ti.forward_ref(ext * chain["w_pre"], None, chain["fd_mask"], H)
    y, en = ti.inverse_ref(ref["fft"], nt, chain["w_post"])
    bad = ti.check("fft", ti.as_complex(fft), ref["fft"], st) + ti.check("amp", amp, ref["amp"], st)
    bad += ti.check("out", out, y, st) + ti.check_intensity(img, en, st) + ti.check_phases(ph, ref, st)
    assert not bad, "; ".join(bad[:12])
    for i in ti.CLEAN_NEXT_TO_BAD:
        assert np.isfinite(fft[i]).all() and np.isfinite(out[i]).all()
    assert not np.isfinite(s).all()   # the NaN / Inf traces are in the sums ...
    keep = np.array([q != "bad" for q in st])
    xg, ig = np.ascontiguousarray(x[keep]), np.ascontiguousarray(ins[keep])
    fft, amp, ph, out, img, s, ss, rows = _tilted(lib, nt, xg, taper, ig, chain, cmask=H, sums=True, src_sum=True)
    assert np.isfinite(s).all() and np.isfinite(ss).all()   # ... and nothing else makes them NaN
    _check_sums("clean", s, amp, ph, nf)
    e64 = _relay(xg, taper, ig, nt).astype(np.float64).sum(0)
    assert np.abs(ss - e64).max() <= SUM_TOL * np.abs(e64).max()
