"""thz_host_pca_components (csrc/pca_host.cpp) against the numpy model of pca_model.py, on the CPU: Gram
matrices the test builds itself at L = 1, 2, 3, 33, 240, 512 and the covariance of the planted two-material scan's
amplitudes from the CPU oracle chain.

Bars (C = gram / (count - 1), floor = L 2^-52 ||C||_F, the rounding of one L-term product row):
- residual       max |C v - lambda v| <= 4 x what numpy.linalg.eigh leaves on the same matrix through the same interface
                 (its vectors after the sign rule, rounded to f32) + floor.  The factor 4 covers a different but also
                 backward-stable algorithm.  Measured: the two residuals are equal to six digits at every L (ratio to the
                 bar 0.25), because the f32 rounding of the vectors is most of either.
- orthogonality  max |V V^T - I| <= 4 x the model's + floor / ||C||_F.  Measured ratio 0.25 likewise.
- eigenvalues    the f64 outputs are where the solver itself shows: two backward-stable solvers each return the exact
                 eigenvalues of a matrix within c L 2^-53 ||C||_2 of C, so by Weyl's inequality they differ by at most twice
                 that; with c = 4 and ||C||_2 <= ||C||_F the bar is 8 L 2^-52 ||C||_F.  Measured: 0.034 of it at the most.
- components     the f32 components equal the model's to 4 ulp of the largest entry wherever the model's eigenvalue gap
                 is wide (measured: identical).
- total variance |trace| to L 2^-52 sum |C_ii|.

The planted property (the model alone on the oracle chain's amplitudes of the 16 x 12 x 1001 scan, 0.2 .. 5 THz, 241
bins): a constant and the first two score images explain R^2 = 0.99899 of the first abundance map and 0.99938 of the
second; the first score image alone 0.476 of the first map — it takes both.  Eigenvalues 16.96, 5.71, then the noise
from 0.0274 down.  Not a bar for the device."""
import functools
import os
import time as clock

import numpy as np
import pytest

import pca_model as model
import thz_image_explorer_amd as pkg

LENGTHS = [1, 2, 3, 33, 240, 512]


def _gram_for(n):
    """columns of decaying scale, more pixels than columns -> (G f64, count)"""
    rng = np.random.default_rng(n)
    count = 2 * n + 5
    a = rng.standard_normal((count, n)) * np.exp(-np.arange(n) / (n / 6 + 1))
    return a.T @ a, count


def _check_against_model(g, count, k, tag):
    rc, comp, ev, tot = pkg.host_pca_components(g, count, k)
    assert rc == 0, tag
    want = model.components(g, count, k)
    c = want["cov"]
    n = c.shape[0]
    fro = float(np.sqrt((c * c).sum()))
    floor = model.residual_floor(c)
    assert np.all(np.diff(ev) <= 0), (tag, ev)
    assert abs(tot - want["total_variance"]) <= n * 2.0 ** -52 * np.abs(np.diag(c)).sum(), tag
    ev_err = float(np.abs(ev - want["eigenvalues"]).max())
    ev_bar = 8 * n * 2.0 ** -52 * fro
    r_got, r_model = model.residual(c, ev, comp), model.residual(c, want["eigenvalues"], want["components"])
    o_got, o_model = model.orthogonality(comp), model.orthogonality(want["components"])
    r_bar, o_bar = 4 * r_model + floor, 4 * o_model + (floor / fro if fro > 0 else 0.0)
    print(f"{tag}: eigenvalue error / bar {ev_err / ev_bar if ev_bar else 0:.3g}, residual / bar {r_got / r_bar if r_bar else 0:.3g}, "
          f"orthogonality / bar {o_got / o_bar if o_bar else 0:.3g}")
    assert ev_err <= ev_bar, (tag, ev_err, ev_bar)
    assert r_got <= r_bar, (tag, r_got, r_bar)
    assert o_got <= o_bar, (tag, o_got, o_bar)
    # the sign rule, on the library's own vectors
    for v in comp:
        top = int(np.argmax(np.abs(v)))
        assert v[top] > 0, (tag, top)
        assert abs(float((v.astype(np.float64) ** 2).sum()) - 1.0) <= (n + 2) * 2.0 ** -24, tag
    # ... and the vectors themselves where the model's gaps say they are determined
    w = want["all_eigenvalues"]
    for i in range(k):
        gap = min(w[i - 1] - w[i] if i else np.inf, w[i] - w[i + 1] if i + 1 < n else np.inf)
        if gap > 1e-6 * max(abs(w[0]), 1e-300):
            assert np.abs(comp[i] - want["components"][i]).max() <= 4 * 2.0 ** -23 * np.abs(want["components"][i]).max(), (tag, i)
    return comp, ev, want


@pytest.mark.parametrize("n", LENGTHS)
def test_components_of_built_grams(n):
    g, count = _gram_for(n)
    _check_against_model(g, count, min(n, pkg.PCA_MAX_COMPONENTS), f"L = {n}")
    if n > 1:
        _check_against_model(g, count, 1, f"L = {n}, K = 1")


def test_sign_rule_with_ties():
    # eigenvectors (1, 1) / sqrt 2 and (1, -1) / sqrt 2: both entries tie, the lowest index is made positive
    rc, comp, ev, _ = pkg.host_pca_components(np.array([[2.0, 1.0], [1.0, 2.0]]) * 9.0, 10, 2)
    assert rc == 0 and np.allclose(ev, [3.0, 1.0], rtol=1e-15)
    r = np.float32(np.sqrt(0.5))
    assert np.array_equal(comp, np.array([[r, r], [r, -r]], np.float32)), comp
    # the same with the sign of the coupling turned: the leading vector is (1, -1) / sqrt 2
    rc, comp, ev, _ = pkg.host_pca_components(np.array([[2.0, -1.0], [-1.0, 2.0]]) * 9.0, 10, 2)
    assert rc == 0 and np.array_equal(comp, np.array([[r, -r], [r, r]], np.float32)), comp
    # a tie between entries 1 and 3 of a four-vector, entry 1 negative in the raw vector
    v = np.array([0.1, -0.7, 0.1, 0.7])
    v /= np.sqrt((v * v).sum())
    g = 5.0 * np.outer(v, v) + 0.5 * np.eye(4)
    rc, comp, ev, _ = pkg.host_pca_components(g * 3.0, 4, 1)
    assert rc == 0 and comp[0, 1] > 0 and comp[0, 3] < 0 and comp[0, 1] == -comp[0, 3]
    assert np.array_equal(comp, model.components(g * 3.0, 4, 1)["components"])
    # a diagonal matrix: unit vectors, in the order of the eigenvalues
    rc, comp, ev, tot = pkg.host_pca_components(np.diag([1.0, 4.0, 2.0]), 2, 3)
    assert rc == 0 and np.array_equal(ev, [4.0, 2.0, 1.0]) and tot == 7.0
    assert np.array_equal(comp, np.eye(3, dtype=np.float32)[[1, 2, 0]])


def test_refusals_and_termination():
    g, count = _gram_for(16)
    for bad_count in (0, 1):
        assert pkg.host_pca_components(g, bad_count, 2)[0] == -1
    for bad_k in (0, -1, 9, 17):
        assert pkg.host_pca_components(g, count, bad_k)[0] == -1
    assert pkg.host_pca_components(g[:3, :3], count, 4)[0] == -1                      # K > L
    assert pkg.host_pca_components(g[:8, :8], count, 8)[0] == 0
    lib = pkg.load_library()
    assert lib.thz_host_pca_components(None, 4, 10, 1, None, None, None) == -1
    big, n = _gram_for(512)
    for bad in (np.nan, np.inf, -np.inf):
        h = big.copy()
        h[300, 17] = h[17, 300] = bad
        t0 = clock.perf_counter()
        assert pkg.host_pca_components(h, n, 4)[0] == -1
        assert clock.perf_counter() - t0 < 1.0                                       # refused before any sweep
    # finite entries whose squares overflow: it returns, with eigenvalues or with a refusal
    rc, comp, ev, _ = pkg.host_pca_components(g * 1e300, 2, 3)
    assert rc in (0, -1)
    if rc == 0:
        assert np.all(np.isfinite(ev)) and np.all(np.diff(ev) <= 0)
    assert pkg.host_pca_components(np.zeros((5, 5)), 7, 2)[0] == 0                    # the zero matrix has eigenvectors too
    tiny = pkg.host_pca_components(g * 1e-300, count, 3)
    assert tiny[0] == 0 and np.all(np.diff(tiny[2]) <= 0)


def test_binding_names_and_constants():
    assert (pkg.PCA_MAX_LEN, pkg.PCA_MAX_COMPONENTS) == (512, 8)
    assert 1 <= pkg.PCA_CHAIN <= 4096
    assert (pkg.BUF_PCA_SCORES, pkg.BUF_PCA_COMPONENTS, pkg.BUF_PCA_MEAN) == (24, 25, 26)
    assert pkg.STAGE_PCA == 15
    import re
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "thzgpu.h")).read()
    for name, value in (("THZ_PCA_MAX_LEN", pkg.PCA_MAX_LEN), ("THZ_PCA_MAX_COMPONENTS", pkg.PCA_MAX_COMPONENTS),
                        ("THZ_PCA_CHAIN", pkg.PCA_CHAIN)):
        assert int(re.search(r"#define\s+%s\s+(\d+)" % name, header).group(1)) == value, name
    assert int(re.search(r"THZ_STAGE_COUNT\s*=\s*(\d+)", header).group(1)) == 16
    bound = {s[0] for s in pkg.SYMBOLS}
    lib = pkg.load_library()
    for name in ("thz_pca_sums", "thz_pca_gram", "thz_host_pca_components", "thz_pca_scores", "thz_session_pca",
                 "thz_session_pca_sums", "thz_session_pca_gram", "thz_session_pca_project"):
        assert name in bound and hasattr(lib, name), name
    import ctypes
    assert ctypes.sizeof(pkg.PcaCfg) == 32 and ctypes.sizeof(pkg.PcaOut) == 80
    cfg = pkg.pca_cfg(10, 241, 1, 3)
    assert (cfg.first, cfg.count, cfg.step, cfg.n_components, cfg.center, cfg.d_mask) == (10, 241, 1, 3, 1, None)


@functools.lru_cache(maxsize=None)
def _planted():
    import oracle_binding as ob
    import synth
    time, cube, a1, a2 = model.planted_scan()
    amp = ob.run_pipeline(cube, time, synth.oracle_chain(time))["amplitudes"]
    first, count = model.band_bins(time)
    x = np.ascontiguousarray(amp.reshape(-1, amp.shape[-1])[:, first:first + count])
    return x, a1, a2, model.pca(x, 3)


def test_planted_scan_model_separates_the_abundances():
    x, a1, a2, out = _planted()
    assert x.shape == (16 * 12, 241)
    s = out["scores"].reshape(3, 16, 12)
    r1, r2, r1_alone = model.explained(a1, s[:2]), model.explained(a2, s[:2]), model.explained(a1, s[:1])
    w = out["all_eigenvalues"]
    print(f"planted scan: R^2 {r1:.5f} and {r2:.5f} from two score images, {r1_alone:.3f} from one; eigenvalues {w[:4]}")
    assert r1 > 0.99 and r2 > 0.99 and r1_alone < 0.9
    assert w[1] > 100 * w[2]                                        # two planted directions above the noise


def test_components_of_the_planted_covariance():
    x, _, _, out = _planted()
    comp, ev, want = _check_against_model(out["gram"], out["count"], 3, "planted scan")
    assert np.array_equal(comp[:2], want["components"][:2])
