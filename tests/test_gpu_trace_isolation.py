"""Every trace to its own scale on the device: the FFT kernels that pack two real traces into one complex transform (P,
fft_p.hpp; chirp-z FB / FB2 / FB4 / FB8, fft_fb.hpp) against numpy float64 of the same f32 inputs, 1e-5 of each
trace's own largest value, across partners up to 1e6 apart, zero traces and non-finite samples (trace_isolation.py).
The one-trace-per-wave families (F, PH, global scratch) are the controls.  Two pairs per wave (THZ_P_PAIRS=2) run in
a child process: the knob is read in the launcher."""
import os
import subprocess
import sys

import numpy as np
import pytest

import synth
import thz_image_explorer_amd as pkg
import trace_isolation as ti

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CASES = [  # (nt, kernel family: 0 = auto, 2 = chirp-z instead of P, variant prefix)
    (1001, 0, "p-mixed-radix"), (1000, 0, "p-mixed-radix"), (1200, 0, "p-mixed-radix"), (1500, 0, "p-mixed-radix"),
    (2000, 0, "p-mixed-radix"), (640, 0, "fb-bluestein"), (777, 0, "fb-bluestein"), (1023, 0, "fb-bluestein"),
    (1502, 0, "fb2-"), (2047, 0, "fb2-"), (3001, 0, "fb4-"), (5000, 0, "fb8-"), (8191, 0, "fb8-"),
    (1001, 2, "fb-bluestein"),
    (1024, 0, "f-regs"), (4096, 0, "f-regs"), (2002, 0, "ph-half-length"), (4000, 0, "ph-half-length"),
    (10000, 0, "g-"),
]
IDS = [f"{nt}-fam{f}" for nt, f, _ in CASES]


def _setup(engine, nt, family, prefix):
    engine.set_kernel_family(family)
    time = synth.make_time(nt)
    engine.set_time_axis(time)
    v = engine.kernel_variant()
    assert v.startswith(prefix), v
    if nt == 10000:
        assert "global-scratch" in v
    return synth.default_chain(time)


def _stages(engine, nt, x, chain):
    """fft without and with data_out / win_b, ifft of finite f32 spectra, the fused pipeline and pipeline_ex in its
    modes -> {name: (fft, amp, ph, out, img, H, xin)}; None entries where a stage has no such output"""
    n, nf = x.shape[0], nt // 2 + 1
    d_x = engine.to_device(x)
    bufs = [d_x]

    def dev(a):
        b = engine.to_device(np.ascontiguousarray(a, np.float32)); bufs.append(b); return b

    def emp(shape):
        b = engine.empty(shape); bufs.append(b); return b

    res = {}
    try:
        for with_out in (False, True):
            d_f, d_a, d_p = emp((n, nf, 2)), emp((n, nf)), emp((n, nf))
            if with_out:
                wa = (chain["w_tilt"] * chain["w_td_before"]).astype(np.float32)
                d_o = emp((n, nt))
                engine.fft(n, d_x, dev(wa), dev(chain["w_fft"]), d_o, d_f, d_a, d_p, dev(chain["fd_mask"]))
                xin = (x * wa) * chain["w_fft"]
            else:
                engine.fft(n, d_x, dev(chain["w_pre"]), None, None, d_f, d_a, d_p, dev(chain["fd_mask"]))
                xin = x * chain["w_pre"]
            res["fft+data_out" if with_out else "fft"] = (d_f.download((n, nf, 2), np.float32), d_a.download((n, nf), np.float32),
                                                          d_p.download((n, nf), np.float32), None, None, None, xin)
        ref = ti.forward_ref(x * chain["w_pre"], None, chain["fd_mask"])
        Yin = np.nan_to_num(ref["fft"], nan=0.0, posinf=0.0, neginf=0.0)
        fin = np.ascontiguousarray(np.stack([Yin.real, Yin.imag], -1).astype(np.float32))
        fin[ti.BAD[0], 5, 0] = np.nan
        fin[ti.BAD[1], 5, 0] = np.inf
        d_o, d_i = emp((n, nt)), emp((n,))
        engine.ifft(n, dev(fin), dev(chain["w_post"]), d_o, d_i)
        res["ifft"] = (fin, None, None, d_o.download((n, nt), np.float32), d_i.download((n,), np.float32), None, None)
        modes = ["pipeline", "ex-sums", "ex-cmask", "ex-cmask+sums"]
        for mode in modes:
            H = _wiener_cmask(chain["time"], nf) if "cmask" in mode else None
            d_f, d_a, d_p, d_o, d_i = emp((n, nf, 2)), emp((n, nf)), emp((n, nf)), emp((n, nt)), emp((n,))
            if mode == "pipeline":
                engine.pipeline(n, d_x, dev(chain["w_pre"]), dev(chain["fd_mask"]), dev(chain["w_post"]), d_f, d_a, d_p, d_o, d_i)
            else:
                d_s = emp((2 * nf,)) if "sums" in mode else None
                engine.pipeline_ex(n, d_x, dev(chain["w_pre"]), dev(chain["fd_mask"]), None if H is None else dev(H),
                                   dev(chain["w_post"]), d_f, d_a, d_p, d_o, d_i, d_s)
            res[mode] = (d_f.download((n, nf, 2), np.float32), d_a.download((n, nf), np.float32),
                         d_p.download((n, nf), np.float32), d_o.download((n, nt), np.float32),
                         d_i.download((n,), np.float32), H, x * chain["w_pre"])
    finally:
        for b in bufs:
            b.free()
    return res


def _wiener_cmask(time, nf):
    z = ((time - time[0] - 11.0) / 0.35).astype(np.float64)
    ref = -z * np.exp(-z * z)
    w = pkg.host_fft_window(time, 0, 1.0, 7.0).astype(np.float64)
    R = np.fft.rfft(ref * w)
    H = np.conj(R) / (np.abs(R) ** 2 + 1e-2 * (np.abs(R) ** 2).max())
    return np.ascontiguousarray(np.stack([H.real, H.imag], -1), np.float32)


def _check_all(nt, x, chain, res):
    st = ti.status()
    bad = []
    for name, (fft, amp, ph, out, img, H, xin) in res.items():
        if name == "ifft":
            y, e = ti.inverse_ref(ti.as_complex(fft), nt, chain["w_post"])
            bad += [f"{name} {b}" for b in ti.check("out", out, y, st) + ti.check_intensity(img, e, st)]
            continue
        ref = ti.forward_ref(xin, None, chain["fd_mask"], H)
        b = ti.check("fft", ti.as_complex(fft), ref["fft"], st) + ti.check("amp", amp, ref["amp"], st)
        b += ti.check_phases(ph, ref, st)
        if out is not None:
            y, e = ti.inverse_ref(ref["fft"], nt, chain["w_post"])
            b += ti.check("out", out, y, st) + ti.check_intensity(img, e, st)
        for i in ti.CLEAN_NEXT_TO_BAD:
            if not (np.isfinite(fft[i]).all() and np.isfinite(ph[i]).all() and (out is None or np.isfinite(out[i]).all())):
                b.append(f"clean trace {i} next to a non-finite one is not finite")
        bad += [f"{name} {s}" for s in b]
    return bad


@pytest.mark.parametrize("nt,family,prefix", CASES, ids=IDS)
def test_every_trace_to_its_own_scale(engine, nt, family, prefix):
    try:
        chain = _setup(engine, nt, family, prefix)
        x = ti.make_cube(nt)
        bad = _check_all(nt, x, chain, _stages(engine, nt, x, chain))
        assert not bad, "; ".join(bad[:12])
    finally:
        engine.set_kernel_family(0)


@pytest.mark.parametrize("nt,family,prefix", [c for c in CASES if c[2].startswith(("p-", "fb"))],
                         ids=[i for c, i in zip(CASES, IDS) if c[2].startswith(("p-", "fb"))])
def test_partner_independence(engine, nt, family, prefix):
    """a trace scaled by 2^k (k = -30, -10, 10) leaves its partner's outputs bit-identical and comes out scaled by 2^k"""
    try:
        chain = _setup(engine, nt, family, prefix)
        factors = [1.0, 1e-3, 1e-4, 1.0, 1.0, 1.0, 1e2, 1.0, 1.0]
        x0 = ti.make_cube(nt, factors)
        base = synth.run_gpu_pipeline(engine, x0.reshape(-1, 1, nt), chain)
        keys = ("fft", "amplitudes", "phases", "data", "img")
        for moved in (0, 1):
            idx = np.arange(moved, x0.shape[0], 2)
            others = np.setdiff1d(np.arange(x0.shape[0]), idx)
            others = others[(others ^ 1) < x0.shape[0]]
            for k in (-30, -10, 10):
                x = x0.copy()
                x[idx] *= np.float32(2.0 ** k)
                got = synth.run_gpu_pipeline(engine, x.reshape(-1, 1, nt), chain)
                for key in keys:
                    a = got[key].reshape(x.shape[0], -1)
                    b = base[key].reshape(x.shape[0], -1)
                    assert np.array_equal(a[others].view(np.uint32), b[others].view(np.uint32)), (moved, k, key)
                s = 2.0 ** k
                st = ["live" if i in idx else "skip" for i in range(x.shape[0])]
                n = x.shape[0]
                bad = ti.check("fft", ti.as_complex(got["fft"].reshape(n, -1, 2)), ti.as_complex(base["fft"].reshape(n, -1, 2)) * s, st)
                bad += ti.check("out", got["data"].reshape(n, -1), base["data"].reshape(n, -1).astype(np.float64) * s, st)
                bad += ti.check_intensity(got["img"].reshape(n), base["img"].reshape(n).astype(np.float64) * s * s, st)
                assert not bad, (moved, k, bad[:6])
    finally:
        engine.set_kernel_family(0)


_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import test_gpu_trace_isolation as t
import trace_isolation as ti
from thz_image_explorer_amd import Engine
out = {}
with Engine(0) as eng:
    for nt in (1001, 1000):
        chain = t._setup(eng, nt, 0, "p-mixed-radix")
        x = ti.make_cube(nt)
        bad = t._check_all(nt, x, chain, t._stages(eng, nt, x, chain))
        if bad:
            sys.exit("nt=%d: %s" % (nt, "; ".join(bad[:12])))
print("ok")
"""


def test_two_pairs_per_wave(engine):
    """THZ_P_PAIRS=2 (two pairs of traces per wave, units of four traces) at 1001 and 1000, in a child process"""
    env = dict(os.environ, THZ_P_PAIRS="2")
    try:
        r = subprocess.run([sys.executable, "-c", _CHILD, ROOT], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                           text=True, timeout=300)
    except subprocess.TimeoutExpired as e:
        pytest.fail("THZ_P_PAIRS=2: child timed out\n%s" % e.stderr)
    assert r.returncode == 0, r.stderr[-4000:]
    assert r.stdout.strip().endswith("ok")


def test_polar_ifft_single_trace(engine):
    """polar_ifft (one trace, no partner) against float64 C2R of from_polar, at its own scale"""
    for nt in (1001, 777, 5000):
        time = synth.make_time(nt)
        engine.set_time_axis(time)
        nf = nt // 2 + 1
        X = np.fft.rfft(ti.make_cube(nt, [1e-4])[0].astype(np.float64))
        a, p = np.abs(X).astype(np.float32), np.angle(X).astype(np.float32)
        got = engine.polar_ifft(a, p)
        Y = a.astype(np.float64) * np.exp(1j * p.astype(np.float64))
        ref = np.fft.irfft(Y, n=nt)   # C2R ignores the DC / Nyquist imaginary parts, as realfft does
        assert ti.trace_errors(got[None], ref[None])[0] < ti.TRACE_TOL, nt
        assert nf == a.size
