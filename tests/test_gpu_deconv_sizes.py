"""The Deconvolution stage at the sizes and trace lengths that switch its code paths, against the oracle
(oracle/thz_oracle_deconv.c) at the bars of test_gpu_deconv.py: the wide bands in three chains (from 1 024 wide
tiles on), k_rl_step_sep's 512- and 256-thread blocks, the padded FIR lengths M = 1024 ... 8192 each filled exactly
and the refusal above them, the chunked recombination at M = 8192, odd pixel counts and traces whose edges are zero.
Every test first asserts, from host_band_psf / host_filter_bank and the tile arithmetic of deconv_api.cpp, that it
reaches the path it is about."""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_binding as ob
import synth
import thz_image_explorer_amd as pkg
from test_gpu_deconv import _bar_target_cube
from test_gpu_parity import TOL, rel

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# kernels.hpp / kernels.hip / deconv_api.cpp constants the path decisions depend on
TAPS = 499                   # kDeconvTaps: FIR length of the bank
SEP_TILE, TILE = 32, 16      # kRlSepTileRows x kRlSepTileCols, kRlTileRows x kRlTileCols
NUM_CU, RL_BATCH = 256, 32   # kNumCU, kRlBatch
SPLIT_WIDE_TILES = 1024      # wide tiles from which the wide bands run in three chains


def _psfs():
    z = np.load(os.path.join(GOLD, "psf_sample.npz"))
    return pkg.psf_from_npz(z), ob.psf_from_npz(z)


def _fir_length(nt):
    """padded FIR transform length M: the next power of two >= nt + TAPS - 1"""
    m = 1
    while m < nt + TAPS - 1:
        m <<= 1
    return m


def _plan(psf, time, cfg, nx, ny, dx, dy, bands=None):
    """the band table and the Richardson-Lucy chains deconv_api.cpp:460-545 build (default knobs): per band its PSF
    shape, kind, tile count and iteration count; per chain its bands (by falling iteration count) and tiles"""
    _, centers = pkg.host_filter_bank(time, cfg)
    wx, wy, _, _ = pkg.host_psf_eval(psf, centers)
    w_min, w_max = np.float32(min(wx.min(), wy.min())), np.float32(max(wx.max(), wy.max()))
    out = []
    for b in range(cfg.n_filters) if bands is None else bands:
        pr, pc = pkg.host_band_psf(psf, centers[b], dx, dy, nx, ny).shape
        wide = pr * pc > 256
        sep = wide or (pr % 2 == 1 and pc % 2 == 1)      # every band PSF's profiles have pr / pc taps
        t = SEP_TILE if sep else TILE
        H, W = nx + 2 * (pr // 2), ny + 2 * (pc // 2)
        fi = np.floor((wx[b] - w_min) / (w_max - w_min) * (np.float32(cfg.n_iterations) - np.float32(1))
                      + np.float32(1))
        out.append(dict(band=b, shape=(pr, pc), wide=wide, sep=sep, tiles=-(-W // t) * -(-H // t), n_iter=int(fi)))
    wide = sorted((b for b in out if b["wide"]), key=lambda b: -b["n_iter"])   # stable, as std::stable_sort
    wide_tiles = sum(b["tiles"] for b in wide)
    cuts = [1, 3, len(wide)] if wide_tiles >= SPLIT_WIDE_TILES else [len(wide)]
    chains, at = [], 0
    for end in cuts:
        end = min(end, len(wide))
        if end > at:
            chains.append(wide[at:end])
            at = end
    for group in ([b for b in out if not b["wide"] and b["sep"]], [b for b in out if not b["sep"]]):
        if group:
            chains.append(sorted(group, key=lambda b: -b["n_iter"]))
    return dict(bands=out, wide_tiles=wide_tiles, chain_tiles=[sum(b["tiles"] for b in c) for c in chains])


def _sep_threads(tiles):
    """k_rl_step_sep's block size for a launch over `tiles` tiles (rl_sep_threads, kernels.hip)"""
    return 512 if tiles > 2 * NUM_CU else 1024


def _engine_deconvolve(eng, psf, cfg, time, cube, dx, dy):
    nx, ny, nt = cube.shape
    eng.set_time_axis(time)
    d_in = eng.to_device(cube); d_out = eng.empty((nx * ny, nt)); d_img = eng.empty((nx * ny,))
    d_g = eng.empty((cfg.n_filters, nx * ny))
    try:
        assert eng.deconvolve(psf, cfg, nx, ny, dx, dy, d_in, d_out, d_img, d_g) == 0
        return (d_out.download((nx, ny, nt), np.float32), d_img.download((nx, ny), np.float32),
                d_g.download((cfg.n_filters, nx, ny), np.float32))
    finally:
        for b in (d_in, d_out, d_img, d_g):
            b.free()


def _oracle(opsf, cfg, time, cube, dx, dy):
    rc, out, img, gains, niter = ob.deconvolution(cube, time, dx, dy, opsf, cfg.n_iterations, cfg.n_filters,
                                                  cfg.start_freq, cfg.end_freq, cfg.win_width)
    assert rc == 0 and niter.max() > 1
    return (out, img, gains), niter


def _rel_errors(res, ref):
    return [float(np.abs(a.astype(np.float64) - b).max() / np.abs(b).max()) for a, b in zip(res, ref)]


def _check_vs_oracle(res, ref, cube, what):
    """(cube, image, gains) within 1e-5 relative max-norm of the oracle's (errors printed for the record), and the
    output is not the input"""
    errs = _rel_errors(res, ref)
    print(f"{what}: cube {errs[0]:.2e}  image {errs[1]:.2e}  gains {errs[2]:.2e}")
    assert np.isfinite(res[0]).all()
    assert max(errs) < 1e-5, (what, errs)
    assert np.abs(res[0] - cube).max() / np.abs(cube).max() > 1e-2


# ------------------------------------------------------------------------------ the production-size default path
PROD = dict(nx=353, ny=347, nt=128, dx=1.0, dy=0.8)


def _prod_cfg():
    return pkg.DeconvCfg(70, 25, 0.1, 10.0, 0.5)   # the reference's bank (25 bands over 0.1-10 THz), 70 iterations


def _float64_stage(cube, time, opsf, cfg, dx, dy, n_iter):
    """the stage in float64 from the oracle's FIR outputs on (thz_oracle_filter_scan: the reference's Complex<f64> FIR):
    band energies, Richardson-Lucy with the 'same' convolution for wide kernels and the correlation for narrow ones
    (deconvolution.rs:432-458, 484-545) as float64 FFT convolutions, gains, recombination -> (cube, image, gains)"""
    from scipy.signal import fftconvolve
    nx, ny, nt = cube.shape
    filters, centers = ob.filter_bank(time, cfg.n_filters, cfg.start_freq, cfg.end_freq, cfg.win_width)
    out = np.zeros(cube.shape, np.float64)
    gains = np.empty((cfg.n_filters, nx, ny), np.float64)
    for b in range(cfg.n_filters):
        k = ob.band_psf(opsf, centers[b], dx, dy, nx, ny).astype(np.float64)
        pr, pc = k.shape
        fwd, back = (k, k[::-1, ::-1]) if pr * pc > 256 else (k[::-1, ::-1], k)
        filt = ob.filter_scan(cube, filters[b]).astype(np.float64)
        energy = (filt ** 2).sum(-1)
        d = np.pad(energy, ((pr // 2, pr // 2), (pc // 2, pc // 2)), mode="reflect")   # the reference's mirror padding
        u = d.copy()
        for _ in range(int(n_iter[b])):
            u = u * fftconvolve(d / (fftconvolve(u, fwd, mode="same") + 1e-12), back, mode="same")
        gains[b] = np.sqrt(np.maximum(u[pr // 2:pr // 2 + nx, pc // 2:pc // 2 + ny], 0.0) / energy)
        out += filt * gains[b][..., None]
    return out, (out ** 2).sum(-1), gains


def test_production_size_three_wide_chains_vs_oracle(engine, monkeypatch):
    """353 x 347 x 128 (odd, not square, dx != dy), the reference's 25 bands: 1 095 wide tiles, so the wide bands run in
    three chains ({b0}, {b1, b2}, the rest: 169 / 338 / 588 tiles) beside the narrow separable chain (2 592 tiles).
    Each chain's batch is one replayed launch sequence over its whole tile list, so the first two wide chains run
    k_rl_step_sep<1024> and the third and the narrow one <512>.  THZ_RL_SPLIT_WIDE=0 (one wide chain of 1 095 tiles:
    <512> for every wide band) and =1 must return the default's bits — the bands never exchange anything, and every
    pixel's sums run the same tap loop whatever the chain or the block size.

    The yardstick.  For wide kernels the reference convolves by FFT; the oracle restates that as sequential f32 sums —
    2 793 of them per pixel for the 49 x 57 band — and after that band's 59 iterations its own gains are 3.1e-5 away
    from a float64 Richardson-Lucy of the same energy images (the f32-FIR floor, scripts/gpu_deconv_error_budget.py's
    quantity, is 7.6e-7 here; the device's gains are 3.9e-6 from the float64 solve).  So cube, image and gains are held
    to 1e-5 of the stage in float64 (_float64_stage); against the oracle, the narrow bands' gains (the reference's
    direct sums, which the oracle repeats in the reference's order) at 1e-5, and everything within 1e-5 plus the
    oracle's own measured distance from the float64 stage."""
    psf, opsf = _psfs()
    nx, ny, nt, dx, dy = (PROD[k] for k in ("nx", "ny", "nt", "dx", "dy"))
    cfg = _prod_cfg()
    time, cube = _bar_target_cube(nx, ny, nt)
    plan = _plan(psf, time, cfg, nx, ny, dx, dy)
    assert plan["wide_tiles"] == 1095 >= SPLIT_WIDE_TILES
    assert plan["chain_tiles"] == [169, 338, 588, 2592]
    assert [_sep_threads(t) for t in plan["chain_tiles"]] == [1024, 1024, 512, 512]
    assert all(b["sep"] for b in plan["bands"])   # no 2-D narrow band, for which THZ_RL_SPLIT_WIDE=1 has no stream left
    n_iter = [b["n_iter"] for b in plan["bands"]]
    assert max(n_iter) > RL_BATCH and min(n_iter) == 1               # several batches; bands that leave early
    # the host's band PSFs are the oracle's, shape and value, at dx != dy
    _, centers = pkg.host_filter_bank(time, cfg)
    for f in centers:
        a, b = pkg.host_band_psf(psf, f, dx, dy, nx, ny), ob.band_psf(opsf, f, dx, dy, nx, ny)
        assert a.shape == b.shape and np.array_equal(a, b), f
    ref, oniter = _oracle(opsf, cfg, time, cube, dx, dy)
    assert list(oniter) == n_iter
    ref64 = _float64_stage(cube, time, opsf, cfg, dx, dy, oniter)
    res = _engine_deconvolve(engine, psf, cfg, time, cube, dx, dy)
    e_dev, e_orc, e_do = _rel_errors(res, ref64), _rel_errors(ref, ref64), _rel_errors(res, ref)
    narrow = [b["band"] for b in plan["bands"] if not b["wide"]]
    e_narrow = float(np.abs(res[2][narrow] - ref[2][narrow]).max() / np.abs(ref[2]).max())
    for what, e in (("device vs float64", e_dev), ("oracle vs float64", e_orc), ("device vs oracle", e_do)):
        print(f"353x347x128 25 bands 70 it, {what}: cube {e[0]:.2e}  image {e[1]:.2e}  gains {e[2]:.2e}")
    print(f"353x347x128 narrow bands' gains, device vs oracle: {e_narrow:.2e}")
    assert np.isfinite(res[0]).all()
    assert max(e_dev) < 1e-5, e_dev
    assert e_narrow < 1e-5
    assert all(a < b + 1e-5 for a, b in zip(e_do, e_orc)), (e_do, e_orc)
    assert np.abs(res[0] - cube).max() / np.abs(cube).max() > 1e-2
    for knob in ("0", "1"):
        monkeypatch.setenv("THZ_RL_SPLIT_WIDE", knob)
        again = _engine_deconvolve(engine, psf, cfg, time, cube, dx, dy)
        for a, b in zip(again, res):
            assert np.array_equal(a, b), knob
    monkeypatch.delenv("THZ_RL_SPLIT_WIDE")


def _group_band_ranges(plan, members):
    """the contiguous band ranges thz_group_session_deconvolve gives its members (dc_band_ranges in group_deconv.cpp: alpha x longest band's
    iterations + beta x iterations x tiles, the slowest member's cost minimised)"""
    bands = plan["bands"]
    nb = len(bands)

    def cost(a, b):
        it = max((bands[k]["n_iter"] for k in range(a, b)), default=0.0)
        return 13.2 * it + 0.0204 * sum(float(bands[k]["n_iter"]) * bands[k]["tiles"] for k in range(a, b))

    best = [[1e300] * (nb + 1) for _ in range(members + 1)]
    cut = [[0] * (nb + 1) for _ in range(members + 1)]
    best[0][0] = 0.0
    for q in range(1, members + 1):
        for b in range(nb + 1):
            for a in range(b + 1):
                if best[q - 1][a] >= 1e300:
                    continue
                v = max(best[q - 1][a], cost(a, b))
                if v < best[q][b]:
                    best[q][b], cut[q][b] = v, a
    ends, b = [], nb
    for q in range(members, 0, -1):
        ends.append(b)
        b = cut[q][b]
    ends = ends[::-1]
    return [(0 if q == 0 else ends[q - 1], ends[q]) for q in range(members)]


def test_group_at_production_size_matches_session(engine):
    """a same-device two-member GroupSession on the production-size cube (chain's default recompute, the deconvolution
    above) against one Session: each member plans the chains of its own band range — here neither reaches 1 024 wide
    tiles, so the group runs one wide chain per member where the single session runs three"""
    psf, _ = _psfs()
    nx, ny, nt, dx, dy = (PROD[k] for k in ("nx", "ny", "nt", "dx", "dy"))
    dcfg = _prod_cfg()
    time, cube = synth.make_cube(nx, ny, nt)
    ranges = _group_band_ranges(_plan(psf, time, dcfg, nx, ny, dx, dy), 2)
    assert ranges[0][0] == 0 and ranges[0][1] == ranges[1][0] and ranges[1][1] == 25 and ranges[0][1] > 0
    member_wide = [_plan(psf, time, dcfg, nx, ny, dx, dy, bands=range(*r))["wide_tiles"] for r in ranges]
    assert _plan(psf, time, dcfg, nx, ny, dx, dy)["wide_tiles"] >= SPLIT_WIDE_TILES
    assert all(0 < w < SPLIT_WIDE_TILES for w in member_wide), member_wide
    cfg = pkg.chain_cfg_default(time)
    single = pkg.Session(engine, nx, ny, time, dx, dy)
    try:
        single.upload(cube, subtract_bias=False)
        single.recompute(cfg)
        assert single.deconvolve(psf, dcfg) == 0
        want_d, want_i = single.download(pkg.BUF_DATA), single.download(pkg.BUF_IMG)
    finally:
        single.close()
    with pkg.Group(devices=[0, 0]) as g:
        gs = pkg.GroupSession(g, nx, ny, time, dx, dy)
        try:
            gs.upload(cube, subtract_bias=False)
            gs.recompute(cfg, 1, pkg.GATHER_TIME)
            assert gs.deconvolve(psf, dcfg) == 0
            ed, ei = rel(gs.download(pkg.BUF_DATA), want_d), rel(gs.download(pkg.BUF_IMG), want_i)
        finally:
            gs.close()
    print(f"group of two vs session, 353x347x128: data {ed:.2e}  image {ei:.2e}  (band ranges {ranges}, "
          f"wide tiles per member {member_wide})")
    assert ed < TOL and ei < TOL


# ------------------------------------------------------------------------------ k_rl_step_sep's block sizes
# one process per THZ_RL_SEP_THREADS value (read once per process): argv = output .npz, then per case
# nx ny nt d n_iter n_filters f0 f1
_SEP_CHILD = r"""
import os, sys
import numpy as np
root = sys.argv[1]
sys.path[:0] = [root, os.path.join(root, "tests")]
import thz_image_explorer_amd as pkg
from test_gpu_deconv import _bar_target_cube
z = np.load(os.path.join(root, "tests", "golden", "psf_sample.npz"))
psf = pkg.psf_from_npz(z)
out = {}
with pkg.Engine(0) as eng:
    for i, a in enumerate(sys.argv[3:]):
        nx, ny, nt, d, n_iter, nb, f0, f1 = a.split(",")
        nx, ny, nt, n_iter, nb, d, f0, f1 = int(nx), int(ny), int(nt), int(n_iter), int(nb), float(d), float(f0), float(f1)
        cfg = pkg.DeconvCfg(n_iter, nb, f0, f1, 0.5)
        time, cube = _bar_target_cube(nx, ny, nt)
        eng.set_time_axis(time)
        d_in = eng.to_device(cube); d_out = eng.empty((nx * ny, nt)); d_img = eng.empty((nx * ny,))
        d_g = eng.empty((nb, nx * ny))
        rc = eng.deconvolve(psf, cfg, nx, ny, d, d, d_in, d_out, d_img, d_g)
        if rc != 0:
            sys.exit("case %d: status %d" % (i, rc))
        out["out%d" % i] = d_out.download((nx, ny, nt), np.float32)
        out["img%d" % i] = d_img.download((nx, ny), np.float32)
        out["gains%d" % i] = d_g.download((nb, nx, ny), np.float32)
        for b in (d_in, d_out, d_img, d_g):
            b.free()
np.savez(sys.argv[2], **out)
"""
_SEP_CASES = [dict(nx=48, ny=40, nt=128, d=1.0, n_iter=100, nb=6, f0=0.25, f1=3.0),    # wide + narrow, 4 batches
              dict(nx=40, ny=36, nt=1001, d=1.0, n_iter=12, nb=4, f0=0.25, f1=2.0)]


def test_separable_block_sizes_change_no_bit(engine, tmp_path):
    """THZ_RL_SEP_THREADS = 256 / 512 / 1024, one child process each (the knob is read once per process), on the
    wide-plus-narrow configuration of test_chain_scheduling_knobs_change_no_bit and a 1001-sample case: the same bits
    as each other and as this process's default (which runs <1024>: every chain here has fewer than 512 tiles), and
    within the oracle's bar"""
    psf, opsf = _psfs()
    default, refs, cubes = [], [], []
    for c in _SEP_CASES:
        cfg = pkg.DeconvCfg(c["n_iter"], c["nb"], c["f0"], c["f1"], 0.5)
        time, cube = _bar_target_cube(c["nx"], c["ny"], c["nt"])
        plan = _plan(psf, time, cfg, c["nx"], c["ny"], c["d"], c["d"])
        assert any(b["wide"] for b in plan["bands"]) and any(not b["wide"] and b["sep"] for b in plan["bands"])
        assert all(_sep_threads(t) == 1024 for t in plan["chain_tiles"])
        default.append(_engine_deconvolve(engine, psf, cfg, time, cube, c["d"], c["d"]))
        refs.append(_oracle(opsf, cfg, time, cube, c["d"], c["d"])[0])
        cubes.append(cube)
    args = [",".join(str(c[k]) for k in ("nx", "ny", "nt", "d", "n_iter", "nb", "f0", "f1")) for c in _SEP_CASES]
    for threads in (256, 512, 1024):   # one child on the GPU at a time; the first that fails ends the test
        path = tmp_path / ("sep%d.npz" % threads)
        env = dict(os.environ, THZ_RL_SEP_THREADS=str(threads))
        try:
            r = subprocess.run([sys.executable, "-c", _SEP_CHILD, ROOT, str(path)] + args, env=env,
                               stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
        except subprocess.TimeoutExpired as e:
            pytest.fail("THZ_RL_SEP_THREADS=%d: child timed out\n%s" % (threads, e.stderr))
        if r.returncode != 0:
            pytest.fail("THZ_RL_SEP_THREADS=%d: child exited %d\n%s" % (threads, r.returncode, r.stderr))
        z = np.load(path)
        for i, c in enumerate(_SEP_CASES):
            got = (z["out%d" % i], z["img%d" % i], z["gains%d" % i])
            for a, b in zip(got, default[i]):
                assert np.array_equal(a, b), (threads, c)
            _check_vs_oracle(got, refs[i], cubes[i], "THZ_RL_SEP_THREADS=%d %dx%dx%d" % (threads, c["nx"], c["ny"], c["nt"]))


# ------------------------------------------------------------------------------ FIR length boundaries
_SMALL = dict(nx=17, ny=19, d=0.5)   # 323 pixels: odd, so one wave of the recombination holds a single pixel


@pytest.mark.parametrize("nt", [526, 527, 1550, 1551, 3598, 3599, 7694])
def test_fir_length_boundaries_vs_oracle(engine, nt):
    """nt = 526 / 1550 / 3598 fill M = 1024 / 2048 / 4096 with the full convolution exactly (Parseval band energies and
    the F-core recombination with zero slack), one sample more takes the next M; 3599 and 7694 (zero slack again) run
    the generic energies and the weight spectra + generic transform of M = 8192"""
    psf, opsf = _psfs()
    nx, ny, d = _SMALL["nx"], _SMALL["ny"], _SMALL["d"]
    cfg = pkg.DeconvCfg(6, 4, 0.4, 3.0, 0.5)
    M = _fir_length(nt)
    assert M == {526: 1024, 527: 2048, 1550: 2048, 1551: 4096, 3598: 4096, 3599: 8192, 7694: 8192}[nt]
    assert (nt + TAPS - 1 == M) == (nt in (526, 1550, 3598, 7694))
    assert (nx * ny) % 2 == 1
    time, cube = _bar_target_cube(nx, ny, nt)
    assert all(b["sep"] for b in _plan(psf, time, cfg, nx, ny, d, d)["bands"])
    ref, _ = _oracle(opsf, cfg, time, cube, d, d)
    res = _engine_deconvolve(engine, psf, cfg, time, cube, d, d)
    _check_vs_oracle(res, ref, cube, f"17x19x{nt} (M = {M})")


def test_traces_too_long_for_the_fir_transform_are_refused(engine):
    """nt = 7695 needs M = 16384: THZ_ERR_UNSUPPORTED (-2) through Engine.deconvolve and Session.deconvolve
    (thzgpu.h promises nothing about the output buffers then, so only the code is pinned)"""
    psf, _ = _psfs()
    nx, ny, d, nt = _SMALL["nx"], _SMALL["ny"], _SMALL["d"], 7695
    assert _fir_length(nt) == 16384
    cfg = pkg.DeconvCfg(6, 4, 0.4, 3.0, 0.5)
    time, cube = _bar_target_cube(nx, ny, nt)
    engine.set_time_axis(time)
    d_in = engine.to_device(cube); d_out = engine.empty((nx * ny, nt))
    with pytest.raises(pkg.ThzError) as e:
        engine.deconvolve(psf, cfg, nx, ny, d, d, d_in, d_out)
    assert e.value.code == -2
    d_in.free(); d_out.free()
    s = pkg.Session(engine, nx, ny, time, d, d)
    try:
        s.upload(cube, subtract_bias=False)
        s.recompute(pkg.chain_cfg_default(time))
        assert s.nt_out == nt
        with pytest.raises(pkg.ThzError) as e:
            s.deconvolve(psf, cfg)
        assert e.value.code == -2
    finally:
        s.close()


def test_chunked_recombination_at_8192_vs_oracle(engine, monkeypatch):
    """97 x 89 x 4000 (M = 8192, no F core): the weight spectra + generic transform run in chunks of 8 190 pixels (256 MiB
    of scratch) — 8 190 + 443 here; THZ_DC_COMBINE_OLD=1 (the one-kernel form) within the same bar"""
    psf, opsf = _psfs()
    nx, ny, nt, d = 97, 89, 4000, 0.5
    cfg = pkg.DeconvCfg(4, 3, 0.4, 3.0, 0.5)
    M = _fir_length(nt)
    nk = M // 2 + 1
    chunk = (256 << 20) // (nk * 8)   # dc_recombine: 256 MiB of complex floats per chunk
    assert M == 8192 and chunk == 8190 and nx * ny - chunk == 443
    time, cube = _bar_target_cube(nx, ny, nt)
    ref, _ = _oracle(opsf, cfg, time, cube, d, d)
    res = _engine_deconvolve(engine, psf, cfg, time, cube, d, d)
    _check_vs_oracle(res, ref, cube, "97x89x4000 chunked")
    monkeypatch.setenv("THZ_DC_COMBINE_OLD", "1")
    old = _engine_deconvolve(engine, psf, cfg, time, cube, d, d)
    monkeypatch.delenv("THZ_DC_COMBINE_OLD")
    _check_vs_oracle(old, ref, cube, "97x89x4000 one kernel")
    assert np.array_equal(old[2], res[2])   # the gains come before the recombination
    print(f"chunked vs one kernel: cube {rel(res[0], old[0]):.2e}  image {rel(res[1], old[1]):.2e}")


# ------------------------------------------------------------------------------ odd pixel counts, zero-edged traces
@pytest.mark.parametrize("case", [dict(nx=21, ny=19, nt=1001), dict(nx=17, ny=21, nt=256)])
def test_odd_pixel_counts_vs_oracle(engine, case):
    """an odd pixel count leaves the last wave of the two-pixel recombination (k_dc_combine_f, M = 2048 / 1024) and of
    the band energies with one pixel.  (17 x 21, not 17 x 15: an image narrower than 16 pixels is the reference's guard)"""
    psf, opsf = _psfs()
    nx, ny, nt, d = case["nx"], case["ny"], case["nt"], 0.5
    assert (nx * ny) % 2 == 1 and min(nx, ny) >= 16 and _fir_length(nt) in (1024, 2048)
    cfg = pkg.DeconvCfg(6, 5, 0.4, 3.0, 0.5)
    time, cube = _bar_target_cube(nx, ny, nt)
    ref, _ = _oracle(opsf, cfg, time, cube, d, d)
    res = _engine_deconvolve(engine, psf, cfg, time, cube, d, d)
    _check_vs_oracle(res, ref, cube, f"{nx}x{ny}x{nt}")


def test_zero_edged_traces_vs_oracle(engine):
    """every other trace has exactly zero first and last 249 samples (its pulse moved into the middle): k_dc_energy_edges
    skips those traces' edge transforms and runs the others' in the same launch"""
    psf, opsf = _psfs()
    nx, ny, nt, d = 21, 19, 1001, 0.5
    shift = (TAPS - 1) // 2
    time, cube = _bar_target_cube(nx, ny, nt)
    flat = cube.reshape(nx * ny, nt)
    moved = np.roll(flat[1::2], 250, axis=1)
    moved[:, :shift] = 0.0
    moved[:, nt - shift:] = 0.0
    flat[1::2] = moved
    edges = np.concatenate([flat[:, :shift], flat[:, nt - shift:]], axis=1)
    assert not edges[1::2].any() and (edges[0::2] != 0).any(axis=1).all() and (flat[1::2] != 0).any(axis=1).all()
    cfg = pkg.DeconvCfg(6, 5, 0.4, 3.0, 0.5)
    ref, _ = _oracle(opsf, cfg, time, cube, d, d)
    res = _engine_deconvolve(engine, psf, cfg, time, cube, d, d)
    _check_vs_oracle(res, ref, cube, "21x19x1001 zero-edged")
