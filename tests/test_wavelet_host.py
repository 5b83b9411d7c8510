"""thz_host_wavelet_trace, thz_host_wavelet_filter and thz_host_wavelet_universal (csrc/wavelet_host.cpp) against the numpy
model of tests/wavelet_model.py, on this machine.

Exact-arithmetic cases: every intermediate is an f32 number (the model asserts it, partial sums included), so no summation
order and no fusing matters and the results compare with np.array_equal.  Tolerance cases (soft shrinkage only: hard
shrinkage is discontinuous at the threshold, so f32 and f64 may decide differently — it is held by the exact cases): per
trace against the f64 model and that trace's own largest |y|; the bar is 8 x the largest deviation of the numpy f32 form
from the f64 form over the batch (floor 16 * 2^-24) — it comes from the two models, never from the library."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import wavelet_model as model
import thz_image_explorer_amd as pkg

HERE = os.path.dirname(os.path.abspath(__file__))
CLANG = shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"


def _host(y, hn, gn, scale, cfg):
    """the host function on every trace of y -> (x (npix, nt), sigma (npix), kept (npix))"""
    xs, ss, ks = [], [], []
    for row in np.atleast_2d(np.ascontiguousarray(y, np.float32)):
        rc, x, sigma, kept = pkg.host_wavelet_trace(row, hn, gn, scale, cfg)
        assert rc == 0
        xs.append(x.copy())
        ss.append(sigma)
        ks.append(kept)
    return np.array(xs), np.array(ss, np.float32), np.array(ks, np.int32)


def _check_exact(y, hn, gn, scale, J, shrink, mode, tag):
    want = model.exact_solution(y, hn, gn, scale, J, shrink, mode)
    got = _host(y, hn, gn, scale, pkg.wavelet_cfg(len(hn), J, shrink, mode))
    for g, w, what in zip(got, want, ("x", "sigma", "kept")):
        assert np.array_equal(g, w), (tag, what)
    return got


def test_names_constants_and_struct_size():
    assert (pkg.BUF_DENOISED, pkg.BUF_DENOISE_SIGMA, pkg.BUF_DENOISE_KEPT) == (37, 38, 39)
    assert (pkg.WAVELET_MAX_TAPS, pkg.WAVELET_MAX_LEVELS, pkg.WAVELET_MAX_NT, pkg.WAVELET_MAX_WORDS) == (16, 6, 4608, 36864)
    assert (pkg.WAVELET_MAX_LEVELS + 2) * pkg.WAVELET_MAX_NT == pkg.WAVELET_MAX_WORDS
    assert C.sizeof(pkg.WaveletCfg) == 16
    assert pkg.STAGE_ECHO == 14 and pkg.load_library().thz_abi_version() == 2
    header = open(os.path.join(HERE, "..", "include", "thzgpu.h")).read()
    for text in ("THZ_BUF_DENOISED = 37", "THZ_BUF_DENOISE_SIGMA = 38", "THZ_BUF_DENOISE_KEPT = 39", "THZ_STAGE_COUNT = 16",
                 "#define THZ_WAVELET_MAX_TAPS   16", "#define THZ_WAVELET_MAX_LEVELS 6", "#define THZ_WAVELET_MAX_NT     4608",
                 "#define THZ_WAVELET_MAX_WORDS  36864"):
        assert text in header, text
    names = [s[0] for s in pkg.SYMBOLS]
    for name in ("thz_wavelet_denoise", "thz_host_wavelet_trace", "thz_host_wavelet_filter", "thz_host_wavelet_universal",
                 "thz_session_wavelet_denoise"):
        assert name in names and hasattr(pkg.load_library(), name)


@pytest.mark.parametrize("order", (1, 2, 3, 4))
def test_filter_helper(order):
    """against the filters the model derives by spectral factorisation, rounded the same way.  The model's doubles are
    good to about 1e-15 and so are the library's literals, so the two f32 roundings agree unless a value lies that close
    to a rounding boundary: one f32 spacing is admitted, nothing more."""
    rc, hn, gn = pkg.host_wavelet_filter(order)
    want_h, want_g = model.analysis_pair(order)
    assert rc == 0 and hn.size == 2 * order == gn.size
    assert np.all(np.abs(hn - want_h) <= np.spacing(np.abs(want_h))) and np.all(np.abs(gn - want_g) <= np.spacing(np.abs(want_g)))
    assert np.array_equal(np.abs(gn), np.abs(hn[::-1])) and np.array_equal(np.sign(gn), np.sign(hn[::-1]) * np.where(np.arange(2 * order) % 2, -1, 1))
    h = np.sqrt(2.0) * hn.astype(np.float64)
    for m in range(order):                                # orthonormal to f32 rounding of the taps
        assert abs(np.dot(h[:h.size - 2 * m], h[2 * m:]) - (m == 0)) < 4e-7, (order, m)
    assert abs(hn.astype(np.float64).sum() - 1.0) < 2e-7 and abs(gn.astype(np.float64).sum()) < 2e-7
    if order == 1:
        assert np.array_equal(hn, model.HAAR[0]) and np.array_equal(gn, model.HAAR[1])


def test_filter_helper_refusals():
    lib = pkg.load_library()
    hn, gn, n = np.full(16, 7, np.float32), np.full(16, 7, np.float32), C.c_int(-3)
    for order in (0, -1, 5, 100):
        assert lib.thz_host_wavelet_filter(order, hn.ctypes.data, gn.ctypes.data, C.byref(n)) == -1
    assert lib.thz_host_wavelet_filter(2, None, gn.ctypes.data, C.byref(n)) == -1
    assert lib.thz_host_wavelet_filter(2, hn.ctypes.data, None, C.byref(n)) == -1
    assert lib.thz_host_wavelet_filter(2, hn.ctypes.data, gn.ctypes.data, None) == -1
    assert np.all(hn == 7) and np.all(gn == 7) and n.value == -3


def test_universal_thresholds():
    """against the formula in f64; the order of the f64 products is the library's own, so one f32 spacing is admitted"""
    for nt in (1, 2, 257, 1001, 4608):
        for J in range(1, 7):
            rc, scale = pkg.host_wavelet_universal(nt, J)
            want = model.universal(nt, J)
            assert rc == 0 and scale.size == J
            assert np.all(np.abs(scale.astype(np.float64) - want) <= np.spacing(want.astype(np.float32))), (nt, J)
    assert pkg.host_wavelet_universal(1, 3)[1].tolist() == [0.0, 0.0, 0.0]
    lib, out = pkg.load_library(), np.full(8, 7, np.float32)
    for nt, J in ((0, 1), (8, 0), (8, 7), (8, -1)):
        assert lib.thz_host_wavelet_universal(nt, J, out.ctypes.data) == -1
    assert lib.thz_host_wavelet_universal(8, 3, None) == -1 and np.all(out == 7)


@pytest.mark.parametrize("nt", (1, 2, 3, 7, 64, 65, 257))
def test_exact_haar(nt):
    y = model.haar_case(nt)
    hn, gn = model.HAAR
    for J in (1, 2, 6):
        for shrink in (0, 1):
            # the thresholds times the median, dyadic factors; and as given
            _check_exact(y, hn, gn, [0.5, 1, 2, 0.25, 4, 1][:J], J, shrink, 0, (nt, J, shrink, 0))
            x, sigma, kept = _check_exact(y, hn, gn, [16, 8.5, 40, 3, 0.75, 100][:J], J, shrink, 1, (nt, J, shrink, 1))
            if nt >= 64:
                assert np.all(kept > 0) and np.all(kept < J * nt)  # the shrinkage acts on both sides
    # nothing shrunk: the trace itself (Haar in halves is exact); everything shrunk: what a_J alone gives
    for shrink in (0, 1):
        x, _, kept = _check_exact(y, hn, gn, [0, 0, 0], 3, shrink, 1, (nt, "all"))
        assert np.array_equal(x, y)
        x, _, kept = _check_exact(y, hn, gn, [1e9] * 3, 3, shrink, 1, (nt, "none"))
        assert not kept.any()


@pytest.mark.parametrize("n_taps", (1, 3, 5, 15, 16))
@pytest.mark.parametrize("nt", (1, 3, 17, 64, 130))
def test_exact_integer_taps(n_taps, nt):
    """small-integer taps; for nt = 3 and 17 the comb s (Lf - 1) passes the trace's end many times over"""
    hn, gn, y, J = model.integer_case(n_taps, nt)
    assert J >= 5
    for shrink, mode, scale in ((0, 1, [3, 9, 40, 100, 700]), (1, 1, [2, 8, 30, 120, 500]), (0, 0, [0.5, 2, 4, 16, 32]),
                                (1, 0, [1, 1, 8, 8, 64])):
        _check_exact(y, hn, gn, scale[:J], J, shrink, mode, (n_taps, nt, shrink, mode))


def test_comb_longer_than_the_trace():
    """N = 3, J = 6, Lf = 16: s (Lf - 1) = 480 >= N at every level"""
    rng = np.random.default_rng(4)
    hn, gn = np.zeros(16, np.float32), np.zeros(16, np.float32)
    hn[0], hn[15], gn[0], gn[15] = 1, 1, 1, -1
    y = rng.integers(-4, 5, (6, 3)).astype(np.float32)
    for shrink in (0, 1):
        _check_exact(y, hn, gn, [1, 2, 4, 8, 16, 32], 6, shrink, 1, ("N3", shrink))
        _check_exact(y, hn, gn, [1, 1, 2, 2, 4, 4], 6, shrink, 0, ("N3 median", shrink))


@pytest.mark.parametrize("n_taps,at", ((1, 0), (4, 3), (16, 15), (16, 7)))
def test_single_tap_is_a_pure_shift(n_taps, at):
    """hn = one tap of 1: a_j is a_{j-1} moved by s at samples around the circle, and the inverse moves it back.  With
    every detail shrunk away the output is the trace itself; with none shrunk, and gn = the same tap, every level
    adds the trace once more"""
    hn = np.zeros(n_taps, np.float32)
    hn[at] = 1
    for nt in (1, 5, 64, 67):
        y = np.random.default_rng(nt).integers(-9, 10, (3, nt)).astype(np.float32)
        for J in (1, 3, 6):
            x, _, kept = _check_exact(y, hn, hn, [1e9] * J, J, 0, 1, (n_taps, at, nt, J))
            assert np.array_equal(x, y) and not kept.any()
            x, _, _ = _check_exact(y, hn, hn, [0] * J, J, 1, 1, (n_taps, at, nt, J, "kept"))
            assert np.array_equal(x, (J + 1) * y)


@pytest.mark.parametrize("order", (1, 2, 3, 4))
def test_perfect_reconstruction(order):
    """hard shrinkage with scale = 0 returns y: per trace against the trace's own largest |y|, within 8 x the largest
    deviation of the numpy f32 form from the f64 form over the batch (floor 16 * 2^-24)"""
    rc, hn, gn = pkg.host_wavelet_filter(order)
    assert rc == 0
    for nt in (1, 2, 3, 7, 64, 65, 1001):
        y = np.random.default_rng(10 * nt + order).standard_normal((6, nt)).astype(np.float32)
        ref, bar = model.reference_and_bar(y, hn, gn, np.zeros(6), 6, 1, 0)
        x, sigma, kept = _host(y, hn, gn, np.zeros(6, np.float32), pkg.wavelet_cfg(2 * order, 6, 1, 0))
        dev = model.deviation(x, y, y)
        print(f"order {order} nt {nt}: worst {dev.max():.3e} of bar {bar:.3e} = {dev.max() / bar:.3f}")
        assert np.all(dev <= bar), (order, nt, dev.max(), bar)
        assert np.all(model.deviation(ref["x"], y, y) <= bar)     # the f64 form itself, with the taps rounded to f32


@pytest.mark.parametrize("order,J,nt", model.TOLERANCE_CONFIGS)
def test_tolerance_cases(order, J, nt):
    rc, hn, gn = pkg.host_wavelet_filter(order)
    rc2, scale = pkg.host_wavelet_universal(nt, J)
    assert rc == 0 and rc2 == 0
    y = model.tolerance_case(nt)
    ref, bar = model.reference_and_bar(y, hn, gn, scale, J, 0, 0)
    x, sigma, kept = _host(y, hn, gn, scale, pkg.wavelet_cfg(2 * order, J, 0, 0))
    dev = model.deviation(x, ref["x"], y)
    print(f"db{order} J {J} nt {nt}: worst {dev.max():.3e} of bar {bar:.3e} = {dev.max() / bar:.3f}")
    assert np.all(dev <= bar), (dev.max(), bar)
    assert np.all(np.abs(sigma - ref["sigma"]) <= bar * np.abs(y).max(axis=1))
    # a coefficient within rounding of its threshold may be counted on either side
    assert np.all(np.abs(kept - ref["kept"]) <= 2) and np.all(kept > 0) and np.all(kept < J * nt // 4)


def test_in_place_and_optional_outputs():
    y = model.haar_case(65)
    hn, gn = model.HAAR
    scale = np.array([0.5, 1, 2], np.float32)
    want = model.exact_solution(y, hn, gn, scale, 3, 0, 0)[0]
    cfg = pkg.wavelet_cfg(2, 3, 0, 0)
    lib = pkg.load_library()
    row = y[0].copy()
    assert lib.thz_host_wavelet_trace(row.ctypes.data, row.size, hn.ctypes.data, gn.ctypes.data, scale.ctypes.data, C.byref(cfg),
                                      row.ctypes.data, None, None) == 0
    assert np.array_equal(row, want[0])


def test_median_is_the_lower_one_and_zeros_compare_as_numbers():
    """N even: rank (N - 1) / 2 is the lower of the two middle elements.  hn = [1], gn = [1]: d_1 = y"""
    one = np.ones(1, np.float32)
    y = np.array([5, -1, 3, -7, 0, 2], np.float32)        # |d_1| sorted: 0 1 2 3 5 7 -> rank 2 -> 2
    rc, x, sigma, kept = pkg.host_wavelet_trace(y, one, one, [1.0], pkg.wavelet_cfg(1, 1, 1, 0))
    assert rc == 0 and sigma == 2.0 and kept == 3          # |d| > 2: 5, 3, -7
    assert np.array_equal(x, y + np.where(np.abs(y) > 2, y, 0))
    y = np.array([-0.0, 0.0, -0.0, 4.0], np.float32)
    rc, x, sigma, kept = pkg.host_wavelet_trace(y, one, one, [0.0], pkg.wavelet_cfg(1, 1, 1, 0))
    assert rc == 0 and sigma == 0.0 and kept == 1 and np.array_equal(x, [0, 0, 0, 8])


def test_refused_configurations():
    hn, gn = model.HAAR
    y = np.ones(33, np.float32)
    ok = dict(n_taps=2, n_levels=3, shrink=0, noise_mode=0)
    scale = np.ones(6, np.float32)
    big = np.ones(pkg.WAVELET_MAX_TAPS + 1, np.float32)
    assert pkg.host_wavelet_trace(y, hn, gn, scale, pkg.wavelet_cfg(**ok))[0] == 0
    for change in (dict(n_taps=0), dict(n_taps=-1), dict(n_taps=pkg.WAVELET_MAX_TAPS + 1), dict(n_levels=0), dict(n_levels=-2),
                   dict(n_levels=pkg.WAVELET_MAX_LEVELS + 1), dict(shrink=2), dict(shrink=-1), dict(noise_mode=2), dict(noise_mode=-1)):
        assert pkg.host_wavelet_trace(y, big, big, np.ones(8, np.float32), pkg.wavelet_cfg(**{**ok, **change}))[0] == -1, change
    for value in (np.nan, np.inf, -np.inf):
        for which in range(3):
            vecs = [hn.copy(), gn.copy(), scale.copy()]
            vecs[which][1] = value
            assert pkg.host_wavelet_trace(y, *vecs, pkg.wavelet_cfg(**ok))[0] == -1, (value, which)
    neg = scale.copy()
    neg[2] = -1e-6
    assert pkg.host_wavelet_trace(y, hn, gn, neg, pkg.wavelet_cfg(**ok))[0] == -1
    neg[2], neg[3] = 1, -1                                # a scale beyond n_levels is not read
    assert pkg.host_wavelet_trace(y, hn, gn, neg, pkg.wavelet_cfg(**ok))[0] == 0
    lib, cfg = pkg.load_library(), pkg.wavelet_cfg(**ok)
    long = np.zeros(pkg.WAVELET_MAX_NT + 1, np.float32)
    x = np.full(pkg.WAVELET_MAX_NT + 1, 7, np.float32)
    p = [a.ctypes.data for a in (hn, gn, scale)]

    def call(yp, nt, h, g, s, c, xp):
        return lib.thz_host_wavelet_trace(yp, nt, h, g, s, c, xp, None, None)

    assert call(long.ctypes.data, long.size, *p, C.byref(cfg), x.ctypes.data) == -1
    assert call(long.ctypes.data, 0, *p, C.byref(cfg), x.ctypes.data) == -1
    assert call(None, 33, *p, C.byref(cfg), x.ctypes.data) == -1
    assert call(y.ctypes.data, 33, None, p[1], p[2], C.byref(cfg), x.ctypes.data) == -1
    assert call(y.ctypes.data, 33, p[0], None, p[2], C.byref(cfg), x.ctypes.data) == -1
    assert call(y.ctypes.data, 33, p[0], p[1], None, C.byref(cfg), x.ctypes.data) == -1
    assert call(y.ctypes.data, 33, *p, None, x.ctypes.data) == -1
    assert call(y.ctypes.data, 33, *p, C.byref(cfg), None) == -1
    assert np.all(x == 7)
    # (J + 2) nt: 36864 runs, 36865 does not
    j6, j4 = pkg.wavelet_cfg(2, 6, 0, 0), pkg.wavelet_cfg(2, 4, 0, 0)
    assert call(long.ctypes.data, 4608, *p, C.byref(j6), x.ctypes.data) == 0
    assert call(long.ctypes.data, 4608, big.ctypes.data, big.ctypes.data, p[2], C.byref(pkg.wavelet_cfg(16, 6, 1, 1)), x.ctypes.data) == 0
    # 36865 = 5 * 7373 has no other factor in 3 .. 8: (J + 2) nt = 36865 needs J = 3 and a trace beyond THZ_WAVELET_MAX_NT
    longer = np.zeros(7373, np.float32)
    assert call(longer.ctypes.data, 7373, *p, C.byref(pkg.wavelet_cfg(2, 3, 0, 0)), longer.ctypes.data) == -1 and not longer.any()
    assert call(long.ctypes.data, 4608, *p, C.byref(j4), x.ctypes.data) == 0


def test_noisy_pulses_are_cleaned():
    """what the feature is for: 32 pulses with an echo and white noise of deviation 0.03; db4, J = 5, hard shrinkage,
    universal thresholds.  At every trace the RMS error against the clean trace is at most half the noisy trace's, and the
    noise estimate m sqrt 2 / 0.6745 lies within [0.8, 1.25] sigma.  The f64 model alone is held to both bars first (it
    gave a worst ratio of 0.30 and estimates of 0.89 .. 1.08 sigma)."""
    sigma0 = 0.03
    clean, noisy = model.noisy_pulses(32, 1001, sigma=sigma0)
    rc, hn, gn = pkg.host_wavelet_filter(4)
    rc2, scale = pkg.host_wavelet_universal(1001, 5)
    assert rc == 0 and rc2 == 0
    before = np.sqrt(((noisy - clean) ** 2).mean(axis=1))

    def held(x, m, who):
        ratio = np.sqrt(((x - clean) ** 2).mean(axis=1)) / before
        est = np.asarray(m, np.float64) * np.sqrt(2.0) / model.MAD / sigma0
        print(f"{who}: worst ratio {ratio.max():.3f}, noise estimate {est.min():.3f} .. {est.max():.3f} sigma")
        assert np.all(ratio <= 0.5), (who, ratio)
        assert np.all((est >= 0.8) & (est <= 1.25)), (who, est)

    ref = model.denoise(noisy, hn, gn, scale, 5, 1, 0)
    held(ref["x"], ref["sigma"], "f64 model")
    x, m, kept = _host(noisy, hn, gn, scale, pkg.wavelet_cfg(8, 5, 1, 0))
    held(x.astype(np.float64), m, "library")
    # the undecimated transform spreads a pulse over every level: still fewer than a tenth of the 5005 coefficients; and
    # a coefficient within rounding of its threshold may be counted on either side
    assert np.all(kept < 500) and np.all(np.abs(kept - ref["kept"]) <= 2)


def test_host_functions_under_sanitizers(tmp_path):
    """tests/emu/wavelet_host_driver.cpp calls the functions of wavelet_host.cpp over the whole Lf, J and N range, the
    corner J = 6, nt = 4608 included, under AddressSanitizer + UBSan, into arrays of exactly the documented sizes: a plain
    executable, nothing loaded into python"""
    csrc = os.path.join(HERE, "..", "thz_image_explorer_amd", "csrc")
    exe = str(tmp_path / "wavelet_host")
    b = subprocess.run([CLANG, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                        os.path.join(HERE, "emu", "wavelet_host_driver.cpp"), os.path.join(csrc, "wavelet_host.cpp"), "-o", exe],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if b.returncode != 0 and "unsupported option" in b.stdout:
        pytest.skip("sanitizer runtime not available")
    assert b.returncode == 0, b.stdout[-3000:]
    r = subprocess.run([exe], env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"),
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and "wavelet_host done" in r.stdout, r.stdout[-4000:]
    assert "runtime error" not in r.stdout and "AddressSanitizer" not in r.stdout, r.stdout[-4000:]
