"""The unmixing layer on the CPU (csrc/unmix_host.cpp, binding.py): names, constants and struct sizes,
thz_host_unmix_prepare and thz_host_unmix_solve against the numpy model of unmix_model.py bit for bit, every refusal,
the exact block case, and what the feature is for — the MODEL alone (f32 projection in lane order, f32 solve in the
written order) against scipy.optimize.nnls in f64.

The bar of the purpose cases is 1e-5 of the pixel's largest abundance, the project's per-trace parity bar.  The model
alone, 200 planted Gaussian-line mixtures with 2 % noise each:

    L    K   w   sweeps   cond(G)   error vs nnls   kkt / |b|
    512  16  14  256      17        6.1e-7          3.1e-8
    65   2   10  256      1.3       1.9e-7          5.7e-8
    512  8   40  4096     47        1.8e-6          5.0e-8
    512  16  14  16       17        1.1e-4          1.7e-5      (not enough: the reason n_sweeps exists)

The planted property of the session test of tests/test_gpu_unmix.py (the model alone on the oracle chain's amplitudes
of the 16 x 12 x 1001 three-material scan, its k-means centroids as endmembers, cond(G) = 32, 256 sweeps): the largest
abundance of every one of the 192 pixels belongs to its k-means label, and no pixel has its best and second-best
distance within 5 % of each other, so none is left out.

The exact block case: the issue that asked for this layer expected kkt = 12 at the pixel's negative block.  By the
definition it gave (and the header has) the term of a coordinate at zero is max(-g, 0), and there g = -b = +12: the
constraint holds with the multiplier 12 and the violation is 0.  The test pins both: b = -12 and g = +12 exactly, kkt 0."""
import ctypes
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import cluster_model
import unmix_model as model
import thz_image_explorer_amd as pkg

HERE = os.path.dirname(os.path.abspath(__file__))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
BAR = 1e-5


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_numbers(a, b):
    """bit for bit, -0 and +0 compared as numbers"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and bool(np.all((_bits(a) == _bits(b)) | ((a == 0) & (b == 0))))


def test_binding_names_constants_and_struct_sizes():
    assert (pkg.BUF_UNMIX_ABUNDANCE, pkg.BUF_UNMIX_PROJ, pkg.BUF_UNMIX_RESID, pkg.BUF_UNMIX_KKT) == (33, 34, 35, 36)
    assert pkg.UNMIX_MAX == 16 == pkg.CLUSTER_MAX and pkg.UNMIX_MAX_SWEEPS == 4096 and pkg.STAGE_PCA == 15
    header = open(os.path.join(os.path.dirname(HERE), "include", "thzgpu.h")).read()
    assert int(re.search(r"#define\s+THZ_UNMIX_MAX\s+(\d+)", header).group(1)) == pkg.UNMIX_MAX
    assert int(re.search(r"#define\s+THZ_UNMIX_MAX_SWEEPS\s+(\d+)", header).group(1)) == pkg.UNMIX_MAX_SWEEPS
    assert int(re.search(r"THZ_STAGE_COUNT\s*=\s*(\d+)", header).group(1)) == 16          # no stage of its own
    for name, value in (("ABUNDANCE", 33), ("PROJ", 34), ("RESID", 35), ("KKT", 36)):
        assert int(re.search(r"THZ_BUF_UNMIX_%s\s*=\s*(\d+)" % name, header).group(1)) == value
    bound = {s[0] for s in pkg.SYMBOLS}
    lib = pkg.load_library()
    for name in ("thz_unmix", "thz_host_unmix_prepare", "thz_host_unmix_solve", "thz_session_unmix"):
        assert name in bound and hasattr(lib, name), name
    assert lib.thz_abi_version() == 2
    assert ctypes.sizeof(pkg.UnmixCfg) == 12 and ctypes.sizeof(pkg.UnmixSessionCfg) == 40
    cfg = pkg.unmix_session_cfg(10, 241)
    assert (cfg.first, cfg.count, cfg.step, cfg.n_endmembers, cfg.n_sweeps, cfg.absorbance, cfg.endmembers, cfg.ref) \
        == (10, 241, 1, 3, 256, 0, None, None)
    given, ref = np.arange(6, dtype=np.float32).reshape(2, 3), np.array([1, 2, 3], np.float32)
    cfg = pkg.unmix_session_cfg(0, 3, 2, 2, 64, endmembers=given, ref=ref)
    assert (cfg.step, cfg.n_endmembers, cfg.n_sweeps, cfg.absorbance) == (2, 2, 64, 1)
    assert np.array_equal(np.ctypeslib.as_array(ctypes.cast(cfg.endmembers, ctypes.POINTER(ctypes.c_float)), (6,)), given.ravel())
    assert np.array_equal(np.ctypeslib.as_array(ctypes.cast(cfg.ref, ctypes.POINTER(ctypes.c_float)), (3,)), ref)
    for s in (pkg.Session.unmix, pkg.Engine.unmix, pkg.host_unmix_prepare, pkg.host_unmix_solve):
        assert callable(s)


def test_fma_of_the_model_is_correctly_rounded():
    """the cases a sum rounded twice gets wrong: x y + z a tie of f32 in f64, broken by what f64 dropped"""
    one, tiny = np.float32(1.0), np.float32(2.0 ** -60)
    x = np.float32(1.0 + 2.0 ** -12)                                   # x x = 1 + 2^-11 + 2^-24: a tie of f32, exact in f64
    low, high = np.float32(1.0 + 2.0 ** -11), np.float32(1.0 + 2.0 ** -11 + 2.0 ** -23)
    assert model.fma32(x, x, np.float32(0.0)) == low                   # the tie itself: to even
    assert model.fma32(x, x, tiny) == high                             # past the tie by what the f64 sum drops
    assert model.fma32(x, x, -tiny) == low
    assert model.fma32(-x, x, -tiny) == -high and model.fma32(-x, x, tiny) == -low
    assert np.float32(float(x) * float(x) + float(tiny)) == low        # ... which a sum rounded twice gets wrong
    rng = np.random.default_rng(0)
    p, q, r = (rng.standard_normal(1000).astype(np.float32) for _ in range(3))
    near = np.abs(model.fma32(p, q, r).astype(np.float64) - (p.astype(np.float64) * q + r))
    assert np.all(near <= 2.0 ** -24 * np.abs(p.astype(np.float64) * q + r) + 1e-45)
    assert np.isnan(model.fma32(np.float32(np.nan), one, one)) and np.isinf(model.fma32(np.float32(np.inf), one, one))


@pytest.mark.parametrize("k", [1, 2, 7, 16])
def test_prepare_against_f64_numpy(k):
    rng = np.random.default_rng(k)
    for n in (1, 63, 512):
        e = (rng.standard_normal((k, n)) * np.exp(rng.uniform(-2, 2, (k, 1)))).astype(np.float32)
        rc, g, rd = pkg.host_unmix_prepare(e)
        assert rc == 0
        want_g, want_rd, g64 = model.prepare(e)
        assert np.array_equal(_bits(g), _bits(want_g)) and np.array_equal(_bits(rd), _bits(want_rd)), (k, n)
        assert np.array_equal(g, g.T)                                  # exactly symmetric
        # and the f64 matrix product, whatever its order of summation
        e64 = e.astype(np.float64)
        assert np.all(np.abs(g.astype(np.float64) - e64 @ e64.T) <= (2.0 ** -24 + n * 2.0 ** -52) * (np.abs(e64) @ np.abs(e64).T))
        assert np.all(np.abs(rd * np.diag(g64) - 1.0) <= 2.0 ** -24)


@pytest.mark.parametrize("k", [1, 2, 7, 16])
@pytest.mark.parametrize("n_sweeps", [0, 1, 64])
def test_solve_against_the_model_bit_for_bit(k, n_sweeps):
    rng = np.random.default_rng(100 * k + n_sweeps)
    e = (rng.random((k, 50)) + 0.1 * rng.standard_normal((k, 50))).astype(np.float32)
    g, rd, _ = model.prepare(e)
    b = (rng.standard_normal((40, k)) * 5).astype(np.float32)
    b[0] = 0.0                                                         # nothing to explain
    b[1] = -np.abs(b[1])                                               # every coordinate stays at zero
    b[2, 0] = np.float32(-0.0)
    a, kkt, _ = model.solve(b, g, rd, n_sweeps)
    for p in range(b.shape[0]):
        rc, got, got_kkt = pkg.host_unmix_solve(b[p], g, rd, n_sweeps)
        assert rc == 0
        assert _same_numbers(got, a[p]) and _same_numbers(np.float32(got_kkt), kkt[p]), (k, n_sweeps, p, got, a[p])
    assert not a[0].any() and not a[1].any() and np.all(a >= 0)
    if n_sweeps == 0:
        assert not a.any() and np.array_equal(kkt, np.fmax(b, 0).max(axis=1))
    # kkt may be NULL
    lib, out = pkg.load_library(), np.zeros(k, np.float32)
    assert lib.thz_host_unmix_solve(b[3].ctypes.data, g.ctypes.data, rd.ctypes.data, k, n_sweeps, out.ctypes.data, None) == 0
    assert _same_numbers(out, a[3])


def test_refusals():
    lib = pkg.load_library()
    e = np.ones((2, 4), np.float32)
    e[1, 2] = 3.0
    g, rd = np.full((2, 2), 7, np.float32), np.full(2, 7, np.float32)
    args = [e.ctypes.data, 2, 4, g.ctypes.data, rd.ctypes.data]
    assert lib.thz_host_unmix_prepare(*args) == 0 and g[0, 0] == 4 and rd[0] == 0.25
    for i in (0, 3, 4):
        bad = list(args)
        bad[i] = None
        assert lib.thz_host_unmix_prepare(*bad) == -1, i
    for k in (0, -1, 17):
        assert lib.thz_host_unmix_prepare(args[0], k, 4, args[3], args[4]) == -1, k
    for n in (0, 513):
        assert lib.thz_host_unmix_prepare(args[0], 2, n, args[3], args[4]) == -1, n
    big, big_g, big_rd = np.ones((16, 512), np.float32), np.zeros((16, 16), np.float32), np.zeros(16, np.float32)
    assert lib.thz_host_unmix_prepare(big.ctypes.data, 16, 512, big_g.ctypes.data, big_rd.ctypes.data) == 0
    assert np.all(big_g == 512) and np.all(big_rd == np.float32(1.0 / 512.0))
    for bad in (np.nan, np.inf, -np.inf):                               # a non-finite entry
        g[:], rd[:] = 7, 7
        e[1, 2] = bad
        assert lib.thz_host_unmix_prepare(*args) == -1
        assert np.all(g == 7) and np.all(rd == 7)                      # refused before anything is written
    e[1] = 0.0                                                         # a zero endmember
    assert lib.thz_host_unmix_prepare(*args) == -1 and np.all(g == 7)
    e[1] = 1e-30                                                       # G64[c][c] = 4e-60: 1 / it is no finite f32
    assert lib.thz_host_unmix_prepare(*args) == -1 and np.all(g == 7)
    e[1] = 3e19                                                        # G64[c][c] = 3.6e39: no finite f32
    assert lib.thz_host_unmix_prepare(*args) == -1 and np.all(g == 7)
    e[1] = 1.0
    assert lib.thz_host_unmix_prepare(*args) == 0
    b, a, kkt = np.ones(2, np.float32), np.zeros(2, np.float32), ctypes.c_float()
    full = [b.ctypes.data, g.ctypes.data, rd.ctypes.data, 2, 4, a.ctypes.data, ctypes.byref(kkt)]
    assert lib.thz_host_unmix_solve(*full) == 0
    for i in (0, 1, 2, 5):
        bad = list(full)
        bad[i] = None
        assert lib.thz_host_unmix_solve(*bad) == -1, i
    for k in (0, -1, 17):
        assert lib.thz_host_unmix_solve(full[0], full[1], full[2], k, 4, full[5], full[6]) == -1, k
    for sweeps in (-1, 4097):
        assert lib.thz_host_unmix_solve(full[0], full[1], full[2], 2, sweeps, full[5], full[6]) == -1, sweeps
    assert lib.thz_host_unmix_solve(full[0], full[1], full[2], 2, 4096, full[5], full[6]) == 0


def test_exact_block_case():
    x, e, planted = model.block_case(k=4, npix=9)
    rc, g, rd = pkg.host_unmix_prepare(e)
    assert rc == 0 and np.array_equal(g, 4 * np.eye(4, dtype=np.float32)) and np.all(rd == 0.25)
    out = model.unmix(x, e, 1)
    assert np.array_equal(out["b"], 4 * planted)                       # small integers: exact in whatever order
    negative = planted < 0
    assert negative.sum(axis=1).tolist() == [1] * 9
    assert np.array_equal(out["a"], np.where(negative, 0, planted)) and np.all(out["resid"] == 36.0)
    for p in range(9):
        rc, a, kkt = pkg.host_unmix_solve(out["b"][p], g, rd, 1)
        assert rc == 0 and np.array_equal(a, out["a"][p]) and kkt == 0.0 == out["kkt"][p]
        # the clamped coordinate: b = -12, so the gradient there is +12 — the multiplier of a constraint that holds
        assert out["b"][p][negative[p]].tolist() == [-12.0]
    grad = model.solve(out["b"], g, rd, 1)[2]
    assert np.array_equal(grad, np.where(negative, 12.0, 0.0))
    # a violated condition does show: no sweep at all leaves kkt = the largest positive b
    assert np.array_equal(model.solve(out["b"], g, rd, 0)[1], (4 * planted).max(axis=1))


CASES = [(512, 16, 14, 256), (65, 2, 10, 256), (512, 8, 40, 4096)]


@functools.lru_cache(maxsize=None)
def _lines(n, k, w, noise):
    x, e, planted = model.line_mixtures(n, k, w, 200, seed=n + k, noise=noise)
    return x, e, planted, model.nnls_rows(x.astype(np.float64), e)


def _worst(a, ref):
    return float((np.abs(a - ref).max(axis=1) / ref.max(axis=1)).max())


@pytest.mark.parametrize("n,k,w,sweeps", CASES)
def test_planted_lines_against_scipy_nnls(n, k, w, sweeps):
    pytest.importorskip("scipy")
    x, e, planted, ref = _lines(n, k, w, 0.02)
    out = model.unmix(x, e, sweeps)
    err = _worst(out["a"], ref)
    kkt = float((out["kkt"] / np.abs(out["b"]).max(axis=1)).max())
    print(f"L = {n}, K = {k}, w = {w}, {sweeps} sweeps: cond(G) {np.linalg.cond(model.prepare(e)[2]):.3g}, "
          f"error vs nnls {err:.3g}, kkt / |b| {kkt:.3g}")
    assert err <= BAR
    # the library's solve from the model's projections is the model's
    g, rd, _ = model.prepare(e)
    got = np.stack([pkg.host_unmix_solve(b, g, rd, sweeps)[1] for b in out["b"]])
    assert _same_numbers(got, out["a"])
    # the residual is the one of nnls's solution to the accuracy of the abundances
    want = ((x.astype(np.float64) - ref @ e.astype(np.float64)) ** 2).sum(axis=1)
    assert np.all(np.abs(out["resid"] - want) <= 1e-4 * want)


def test_sixteen_sweeps_are_not_enough_at_sixteen_endmembers():
    pytest.importorskip("scipy")
    x, e, planted, ref = _lines(512, 16, 14, 0.02)
    err = _worst(model.unmix(x, e, 16)["a"], ref)
    print(f"L = 512, K = 16, 16 sweeps: error vs nnls {err:.3g}")
    assert err > BAR


@pytest.mark.parametrize("n,k,w,sweeps", CASES)
def test_noise_free_mixtures_are_recovered(n, k, w, sweeps):
    _, e, planted, _ = _lines(n, k, w, 0.02)
    x = (planted @ e.astype(np.float64)).astype(np.float32)
    out = model.unmix(x, e, sweeps)
    err = _worst(out["a"], planted)
    print(f"L = {n}, K = {k}, noise-free: error vs the planted abundances {err:.3g}")
    assert err <= BAR


def test_absorbance_element_of_the_model():
    rng = np.random.default_rng(2)
    ref = rng.uniform(0.5, 2.0, 40).astype(np.float32)
    alpha = rng.uniform(0.0, 3.0, (10, 40))
    x = (ref[None, :] * np.exp(-alpha)).astype(np.float32)
    u, u64 = model.element(x, ref)
    assert np.all(np.abs(u - u64) <= model.element_bound(x, ref)) and np.all(np.abs(u64 - alpha) <= 1e-6)
    plain, plain64 = model.element(x)
    assert plain is x and np.array_equal(plain64, x.astype(np.float64))


def test_planted_scan_largest_abundance_is_the_kmeans_label():
    """the model alone on the CPU oracle chain's amplitudes: what makes the session test of test_gpu_unmix.py meaningful"""
    import oracle_binding as ob
    import synth
    time, cube, material = cluster_model.planted_scan()
    amp = ob.run_pipeline(cube, time, synth.oracle_chain(time))["amplitudes"]
    first, count = cluster_model.band_bins(time)
    x = np.ascontiguousarray(amp.reshape(-1, amp.shape[-1])[:, first:first + count])
    km = cluster_model.kmeans(x, 3)
    out = model.unmix(x, km["centroids"], 256)
    clear = ~cluster_model.margin_is_within(km["last"]["d2"], 0.05)
    print(f"planted scan: {int((~clear).sum())} of {clear.size} pixels left out, cond(G) {np.linalg.cond(model.prepare(km['centroids'])[2]):.3g}")
    assert (~clear).sum() <= clear.size // 20
    assert np.array_equal(out["a"].argmax(axis=1)[clear], km["label"][clear])
    assert np.all(out["a"].max(axis=1) > 0.9) and np.all(np.sort(out["a"], axis=1)[:, -2] < 0.1)   # fractions, not labels


@pytest.mark.skipif(not os.path.exists(CLANG), reason="needs clang with the sanitizer runtimes")
def test_host_functions_under_sanitizers(tmp_path):
    """tests/emu/unmix_host_driver.cpp calls the two functions of unmix_host.cpp over the K range under AddressSanitizer +
    UBSan, into arrays of exactly the documented sizes: a plain executable, nothing loaded into python"""
    csrc = os.path.join(HERE, "..", "thz_image_explorer_amd", "csrc")
    exe = str(tmp_path / "unmix_host")
    b = subprocess.run([CLANG, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                        os.path.join(HERE, "emu", "unmix_host_driver.cpp"), os.path.join(csrc, "unmix_host.cpp"), "-o", exe],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if b.returncode != 0 and "unsupported option" in b.stdout:
        pytest.skip("sanitizer runtime not available")
    assert b.returncode == 0, b.stdout[-3000:]
    r = subprocess.run([exe], env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"),
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and "unmix_host done" in r.stdout, r.stdout[-4000:]
    assert "runtime error" not in r.stdout and "AddressSanitizer" not in r.stdout, r.stdout[-4000:]
