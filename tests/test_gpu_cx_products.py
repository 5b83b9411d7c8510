"""The batched complex products of fft_f.hpp (cx_mul_batch: two packed instructions per product instead of hipcc's
four) and the fused nt = 4096 chain that runs on them.

test_batched_products_bit_for_bit builds tests/gpu_cx_products.hip and runs it: cx_mul_batch<K>, K = 2, 4, 5, 15, 16,
against cx_mul as hipcc compiles it, the form with the first factor in SGPRs, and the R2C / C2R splits through the
batches against copies of their earlier bodies — same bits for every assignment of +-0, +-denormal, +-Inf and NaN to
the four components, and for random operands (in the splits a NaN compares as a NaN: which of two NaN operands an
instruction hands on follows the operand order, which hipcc chooses anew wherever it inlines the body).

test_fused_4096_chain_on_19_traces: thz_pipeline_ex (every fused build of FPlan<16,16,8> that call can select: real and
complex multiplier, with and without the sums) and a session's first and second recompute (the second is the pruned
kCfgLow build) on 19 traces — one block's rounds of 8, 8 and 3 — among them a NaN trace, an Inf trace, an all-zero trace
and one with negative zeros, against the oracle at test_fused_pipeline_ex's tolerances.  Which build ran is read back
from the launcher after every launch (thz::g_f_last_cfg, the record tests/test_emu_band_prune.py reads on the emulation):
neither keep range nor pruning on the launches that write everything, both on the second recompute, the sums and the
complex multiplier where the case asks for them."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import oracle_binding as ob
import synth
import thz_image_explorer_amd as pkg

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "thz_image_explorer_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

NX, NY, NT = 19, 1, 4096
NF = NT // 2 + 1
NAN_AT, INF_AT, ZERO_AT, NEGZ_AT = 5, 17, 3, 9   # rounds 0, 2, 0, 1 of a block of eight waves
FINITE = np.array([i not in (NAN_AT, INF_AT) for i in range(NX * NY)])
# fft_f.hpp's kCfg bits (kCfgBar, 8, is left to the launcher's default and its developer knob)
CFG_AMP, CFG_CMASK, CFG_SUMS, CFG_BAR, CFG_BAND, CFG_KEEP, CFG_LOW = 1, 2, 4, 8, 16, 32, 64


def _last_cfg():
    """the kCfg bits of this thread's latest fused launch: a thread-local of the library, not part of its C ABI"""
    return C.c_int.in_dll(pkg.load_library(), "_ZN3thz12g_f_last_cfgE")


def test_batched_products_bit_for_bit(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    exe = str(tmp_path / "cx_products")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", f"-I{CSRC}", os.path.join(HERE, "gpu_cx_products.hip"),
                        "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:]
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-4000:]
    assert r.stdout.count("same bits") == 7, r.stdout


@pytest.fixture(scope="module")
def scene():
    time, cube = synth.make_cube(NX, NY, NT)
    cube = cube.copy()
    flat = cube.reshape(NX * NY, NT)
    flat[ZERO_AT] = 0.0
    flat[NEGZ_AT, ::7] = -0.0
    flat[NAN_AT, NT // 3] = np.nan
    flat[INF_AT, 11] = np.inf
    clean = np.where(np.isfinite(cube), cube, 0.0).astype(np.float32)   # the oracle's input for the finite rows
    ref = ob.run_pipeline(clean, time, synth.oracle_chain(time))
    return time, cube, ref


def _check(fft, amp, out, img, ref):
    from test_gpu_parity import TOL, rel
    npix = NX * NY
    scale = np.abs(ref["fft"]).max()
    f = FINITE
    assert rel(fft[f], ref["fft"].reshape(npix, NF, 2)[f], scale) < TOL
    assert rel(amp[f], ref["amplitudes"].reshape(npix, NF)[f], scale) < TOL
    assert rel(out[f], ref["data"].reshape(npix, NT)[f]) < TOL
    assert rel(img[f], ref["img"].ravel()[f]) < TOL
    assert not out[ZERO_AT].any() and not amp[ZERO_AT].any()
    for bad in (NAN_AT, INF_AT):
        assert not np.isfinite(out[bad]).any() and not np.isfinite(fft[bad]).all() and not np.isfinite(amp[bad]).all()


@pytest.mark.parametrize("mode", ["plain", "sums", "cmask", "cmask+sums", "cmask+sums+band"])
def test_fused_4096_chain_on_19_traces(engine, scene, mode):
    from test_gpu_parity import TOL
    time, cube, ref = scene
    e = engine
    e.set_time_axis(time)
    chain_p, chain = synth.default_chain(time), synth.oracle_chain(time)
    npix = NX * NY
    H = None
    if "cmask" in mode:
        H = np.empty((NF, 2), np.float32)
        H[:, 0] = 0.7 + 0.2 * np.cos(np.arange(NF) * 0.01)
        H[:, 1] = 0.3 * np.sin(np.arange(NF) * 0.02)
    bufs = [e.to_device(cube), e.to_device(chain_p["w_pre"]), e.to_device(chain_p["fd_mask"]), e.to_device(chain_p["w_post"]),
            e.empty((npix, NF, 2)), e.empty((npix, NF)), e.empty((npix, NF)), e.empty((npix, NT)), e.empty((npix,))]
    d_raw, d_pre, d_fd, d_post, d_fft, d_amp, d_ph, d_out, d_img = bufs
    d_H = e.to_device(H) if H is not None else None
    d_sums = e.empty((2 * NF,)) if "sums" in mode else None
    try:
        band = None
        if "band" in mode:   # the bins outside are zero in fd_mask: the complex multiplier's band-limited table
            nz = np.nonzero(chain_p["fd_mask"])[0]
            band = (int(nz[0]), int(nz[-1]) + 1)
        _last_cfg().value = -1
        e.pipeline_ex(npix, d_raw, d_pre, d_fd, d_H, d_post, d_fft, d_amp, d_ph, d_out, d_img, d_sums, band)
        cfg = _last_cfg().value
        fft = d_fft.download((npix, NF, 2), np.float32); amp = d_amp.download((npix, NF), np.float32)
        out = d_out.download((npix, NT), np.float32); img = d_img.download((npix,), np.float32)
    finally:
        for b in bufs + [d_H, d_sums]:
            if b is not None:
                b.free()
    # the build of the mode that writes everything: no keep range, no pruning; the band-limited table only where a band is named
    want = CFG_AMP | (CFG_CMASK if "cmask" in mode else 0) | (CFG_SUMS if "sums" in mode else 0) | (CFG_BAND if "band" in mode else 0)
    assert cfg >= 0 and cfg & ~CFG_BAR == want, (mode, cfg)
    if H is None:
        _check(fft, amp, out, img, ref)
        return
    # the complex multiplier is build-defined: a numpy fp64 model, as test_fused_pipeline_ex has it
    f = FINITE
    clean = np.where(np.isfinite(cube), cube, 0.0).reshape(npix, NT).astype(np.float64)
    pre = chain["w_tilt"].astype(np.float64) * chain["w_td_before"] * chain["w_fft"]
    Y = np.fft.rfft(clean * pre, axis=1) * ((H[:, 0].astype(np.float64) + 1j * H[:, 1]) * chain["fd_mask"])
    a_ref = np.abs(Y)
    Y[:, 0] = Y[:, 0].real
    Y[:, -1] = Y[:, -1].real
    t_ref = np.fft.irfft(Y, n=NT, axis=1) * chain["w_post"]
    got = fft[..., 0] + 1j * fft[..., 1]
    assert np.abs(got[f] - Y[f]).max() / np.abs(Y[f]).max() < TOL
    assert np.abs(amp[f] - a_ref[f]).max() / a_ref[f].max() < TOL
    assert np.abs(out[f] - t_ref[f]).max() / np.abs(t_ref[f]).max() < TOL
    assert np.abs(img[f] - (t_ref[f] ** 2).sum(1)).max() / (t_ref[f] ** 2).sum(1).max() < TOL
    for bad in (NAN_AT, INF_AT):
        assert not np.isfinite(out[bad]).any()


@pytest.mark.parametrize("means", [0, 1], ids=["nosums", "sums"])
def test_session_recomputes_on_19_traces(engine, scene, means):
    """the first recompute after an upload writes everything (the plain fused build), the second leaves the out-of-band
    zeros in place and prunes the inverse transform's input (kCfgLow): both against the oracle"""
    from test_gpu_session import oracle_chain
    time, cube, _ = scene
    cfg = pkg.chain_cfg_default(time)
    cfg.want_means = means
    o = oracle_chain(np.where(np.isfinite(cube), cube, 0.0).astype(np.float32), time, cfg)
    ref = dict(fft=o["fft"], amplitudes=o["amp"], data=o["data"], img=o["img"])
    s = pkg.Session(engine, NX, NY, time)
    try:
        s.upload(cube, subtract_bias=False)
        for step in ("first", "pruned"):
            _last_cfg().value = -1
            s.recompute(cfg)
            ran = _last_cfg().value
            want = CFG_AMP | (CFG_SUMS if means else 0) | (CFG_KEEP | CFG_LOW | CFG_BAR if step == "pruned" else 0)
            assert ran >= 0 and ran & ~(0 if step == "pruned" else CFG_BAR) == want, (step, ran)
            npix = NX * NY
            _check(s.download(pkg.BUF_FFT).reshape(npix, NF, 2), s.download(pkg.BUF_AMPLITUDES).reshape(npix, NF),
                   s.download(pkg.BUF_DATA).reshape(npix, NT), s.download(pkg.BUF_IMG).reshape(npix), ref)
    finally:
        s.close()
