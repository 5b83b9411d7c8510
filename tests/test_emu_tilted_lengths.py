"""FBP kernels (fft_fbp.hpp) on the host-thread emulation: the trace lengths a tilted 1001-sample scan lands on
(1024 < nt <= 1280) run their chirp-z convolution on the mixed-radix P core at M = 2304 / 2560 — the planner's
choice, parity with the oracle, the stage entry points against the fused launch, and the per-trace error bar."""
import ctypes as C

import numpy as np
import pytest

import oracle_binding as ob
import synth
import trace_isolation as ti
from test_emu_kernels import emu, _p, _iso_chain, _emu_forward, _emu_chain, _iso_check_chain  # noqa: F401 (emu: fixture)

FBP = 7
FBP_LENGTHS = [1025, 1041, 1059, 1101, 1151, 1152, 1153, 1175, 1201, 1279, 1280]


@pytest.fixture
def auto(emu):
    emu.emu_allow_f(1)
    emu.emu_allow_p(1)
    emu.emu_set_p_pairs(0)
    emu.emu_set_grid_cap(0)
    yield emu
    emu.emu_allow_p(1)
    emu.emu_set_grid_cap(0)


def test_planner_routes_the_tilted_lengths(auto):
    emu = auto
    for nt in FBP_LENGTHS:
        assert emu.emu_family(nt) == FBP, nt
    for nt in (1281, 1502, 2047):
        assert emu.emu_family(nt) == 3, nt      # M = 3072 is not a rung: still two F-core runs at M = 4096
    assert emu.emu_family(1200) == 6            # a length with a plan of its own keeps it
    assert emu.emu_family(1023) == 2
    assert emu.emu_family(1024) == 1
    emu.emu_allow_p(0)                          # thz_set_kernel_family(2): the A/B switch back to the F core
    for nt in FBP_LENGTHS:
        assert emu.emu_family(nt) == 3, nt


def _fused(emu, nt, cube):
    npix, nf = cube.shape[0] * cube.shape[1], nt // 2 + 1
    chain = synth.default_chain(synth.make_time(nt))
    fft = np.zeros((npix, nf, 2), np.float32); amp = np.zeros((npix, nf), np.float32)
    ph = np.zeros((npix, nf), np.float32); out = np.zeros((npix, nt), np.float32); img = np.zeros(npix, np.float32)
    assert emu.emu_pipeline(nt, C.c_size_t(npix), _p(cube), _p(chain["w_pre"]), _p(chain["fd_mask"]), _p(chain["w_post"]),
                            _p(fft), _p(amp), _p(ph), _p(out), _p(img)) == 0
    return chain, fft, amp, ph, out, img


# odd and even trace counts, one trace, more pairs than a block has waves (7 at M = 2304, 6 at M = 2560)
@pytest.mark.parametrize("shape", [(5, 1), (2, 3), (1, 1), (17, 1)])
@pytest.mark.parametrize("nt", [1025, 1101, 1152, 1153, 1201, 1280])
def test_fused_chain_vs_oracle(auto, nt, shape):
    emu = auto
    assert emu.emu_family(nt) == FBP
    nx, ny = shape
    time = synth.make_time(nt)
    cube = synth.make_traces(np.arange(nx * ny) + 11, nt).reshape(nx, ny, nt).copy()
    chain, fft, amp, ph, out, img = _fused(emu, nt, cube)
    ref = ob.run_pipeline(cube, time, chain)
    scale = np.abs(ref["fft"]).max()
    assert np.abs(fft.reshape(ref["fft"].shape) - ref["fft"]).max() / scale < 1e-5
    assert np.abs(amp.reshape(ref["amplitudes"].shape) - ref["amplitudes"]).max() / scale < 1e-5
    assert np.abs(out.reshape(ref["data"].shape) - ref["data"]).max() / max(np.abs(ref["data"]).max(), 1e-30) < 1e-5
    assert np.abs(img.reshape(ref["img"].shape) - ref["img"]).max() / max(ref["img"].max(), 1e-30) < 1e-5
    st = ob.fft_stage((cube * chain["w_pre"]).astype(np.float32), time, 0, 0.0, 0.0)
    strong = st["amplitudes"] > 0.05 * st["amplitudes"].max(axis=-1, keepdims=True)
    d = ph.reshape(ref["phases"].shape).astype(np.float64) - ref["phases"]
    assert np.abs(d - 2 * np.pi * np.round(d / (2 * np.pi)))[strong].max() < 3e-3
    assert np.all(fft[:, 0, 1] == 0.0) and not np.signbit(fft[:, 0, 1]).any()
    if nt % 2 == 0:
        assert np.all(fft[:, -1, 1] == 0.0) and not np.signbit(fft[:, -1, 1]).any()


@pytest.mark.parametrize("nt,npix", [(1041, 5), (1152, 4), (1201, 15), (1280, 1)])
def test_stage_entry_points_land_on_the_fused_launch(auto, nt, npix):
    emu = auto
    cube = synth.make_traces(np.arange(npix) + 23, nt).reshape(npix, 1, nt).copy()
    chain, fft, amp, ph, out, img = _fused(emu, nt, cube)
    fft2 = np.zeros_like(fft); amp2 = np.zeros_like(amp); ph2 = np.zeros_like(ph)
    assert emu.emu_fft_fwd(nt, C.c_size_t(npix), _p(cube), _p(chain["w_pre"]), None, None, _p(fft2), _p(amp2), _p(ph2),
                           _p(chain["fd_mask"])) == 0
    assert np.array_equal(fft2, fft) and np.array_equal(amp2, amp) and np.array_equal(ph2, ph)
    out2 = np.zeros_like(out); img2 = np.zeros_like(img)
    assert emu.emu_fft_inv(nt, C.c_size_t(npix), _p(fft), _p(chain["w_post"]), _p(out2), _p(img2)) == 0
    assert np.array_equal(out2, out) and np.array_equal(img2, img)
    # the forward stage with its `data` output: one window, two windows, none — the windowed traces exactly, and the
    # spectrum of exactly those
    x = cube.reshape(npix, nt)
    wa, wb = (chain["w_tilt"] * chain["w_td_before"]).astype(np.float32), chain["w_fft"]
    for a, b in ((wa, wb), (wa, None), (None, wb), (None, None)):
        want = x if a is None else x * a
        want = want if b is None else want * b
        dout = np.full_like(x, np.nan); fft3 = np.zeros_like(fft)
        assert emu.emu_fft_fwd(nt, C.c_size_t(npix), _p(x), _p(a), _p(b), _p(dout), _p(fft3), None, None, None) == 0
        assert np.array_equal(dout, want)
        fft4 = np.zeros_like(fft)
        assert emu.emu_fft_fwd(nt, C.c_size_t(npix), _p(np.ascontiguousarray(want)), None, None, None, _p(fft4), None, None,
                               None) == 0
        assert np.array_equal(fft3, fft4)


@pytest.mark.parametrize("nt", [1101, 1201])
def test_every_trace_to_its_own_scale(auto, nt):
    """partners 1e6 apart, a zero trace exactly zero, NaN / Inf traces next to clean ones: forward (with and without the
    windowed-trace output and second window), inverse and the fused chain, each trace against its own float64 values"""
    emu = auto
    assert emu.emu_family(nt) == FBP
    chain = _iso_chain(nt)
    x = ti.make_cube(nt)
    st = ti.status()
    bad = []
    for with_data_out in (False, True):
        rc, fft, amp, ph, xin = _emu_forward(emu, nt, x, chain, with_data_out)
        assert rc == 0
        ref = ti.forward_ref(xin, None, chain["fd_mask"])
        tag = "+data_out" if with_data_out else ""
        bad += [tag + b for b in ti.check("fft", ti.as_complex(fft), ref["fft"], st)
                + ti.check("amp", amp, ref["amp"], st) + ti.check_phases(ph, ref, st)]
        for i in ti.CLEAN_NEXT_TO_BAD:
            assert np.isfinite(fft[i]).all()
    ref = ti.forward_ref(x * chain["w_pre"], None, chain["fd_mask"])
    Yin = np.nan_to_num(ref["fft"], nan=0.0, posinf=0.0, neginf=0.0)
    fin = np.ascontiguousarray(np.stack([Yin.real, Yin.imag], -1).astype(np.float32))
    for i in ti.BAD:
        fin[i, 5, 0] = np.nan if i == ti.BAD[0] else np.inf
    out = np.zeros_like(x); img = np.zeros(x.shape[0], np.float32)
    assert emu.emu_fft_inv(nt, C.c_size_t(x.shape[0]), _p(fin), _p(chain["w_post"]), _p(out), _p(img)) == 0
    y, e = ti.inverse_ref(ti.as_complex(fin), nt, chain["w_post"])
    bad += ["ifft " + b for b in ti.check("out", out, y, st) + ti.check_intensity(img, e, st)]
    bad += ["pipeline " + b for b in _iso_check_chain(nt, x, chain, _emu_chain(emu, nt, x, chain, "pipeline"))]
    assert not bad, "; ".join(bad[:12])


@pytest.mark.parametrize("nt", [1101, 1201])
def test_partner_independence(auto, nt):
    """a trace scaled by 2^k leaves its partner's outputs bit-identical and comes out scaled by 2^k itself"""
    emu = auto
    chain = _iso_chain(nt)
    factors = [1.0, 1e-3, 1e-4, 1.0, 1.0, 1.0, 1e2, 1.0, 1.0]
    x0 = ti.make_cube(nt, factors)
    base = _emu_chain(emu, nt, x0, chain, "pipeline")
    base_f = _emu_forward(emu, nt, x0, chain, False)
    for moved in (0, 1):
        for k in (-30, -10, 10):
            x = x0.copy()
            idx = np.arange(moved, x.shape[0], 2)
            x[idx] *= np.float32(2.0 ** k)
            res = _emu_chain(emu, nt, x, chain, "pipeline")
            res_f = _emu_forward(emu, nt, x, chain, False)
            others = np.setdiff1d(np.arange(x.shape[0]), idx)
            others = others[(others ^ 1) < x.shape[0]]
            for a, b in list(zip(res[:5], base[:5])) + list(zip(res_f[1:4], base_f[1:4])):
                assert np.array_equal(np.asarray(a)[others].view(np.uint32), np.asarray(b)[others].view(np.uint32)), \
                    f"moved={moved} k={k}: a partner's outputs changed"
            s = 2.0 ** k
            st = ["live" if i in idx else "skip" for i in range(x.shape[0])]
            bad = ti.check("fft", ti.as_complex(res[0]), ti.as_complex(base[0]) * s, st)
            bad += ti.check("amp", res[1], base[1].astype(np.float64) * s, st)
            bad += ti.check("out", res[3], base[3].astype(np.float64) * s, st)
            bad += ti.check_intensity(res[4], base[4].astype(np.float64) * s * s, st)
            d = np.abs(res[2][idx].astype(np.float64) - base[2][idx])
            assert not bad and d.max() < 1e-3, f"moved={moved} k={k}: " + "; ".join(bad[:8]) + f" phase {d.max():.1e}"
