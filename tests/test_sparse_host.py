"""thz_host_sparse_trace and thz_host_sparse_kernel (csrc/sparse_host.cpp) against the numpy model of
tests/sparse_model.py, on this machine.

Exact-arithmetic cases: every intermediate is an f32 number (the model asserts it), so no summation order matters and the
results compare with np.array_equal.  Tolerance cases: per trace against the f64 model and that trace's own largest |x|;
the bar is 8 x the largest deviation of the numpy f32 form from the f64 form over the batch of 24 traces (floor
16 * 2^-24) — it comes from the two models, never from the library.  The residual is held to 1e-5 relative of the f64 sum
taken on the returned x, the count of spikes is exact."""
import ctypes as C

import numpy as np
import pytest

import echo_map_model
import sparse_model as model
import thz_image_explorer_amd as pkg


def _host(y, h, cfg):
    """the host function on every trace of y -> (x (npix, nt), resid (npix), nnz (npix))"""
    y = np.atleast_2d(np.ascontiguousarray(y, np.float32))
    xs, rs, ns = [], [], []
    for row in y:
        rc, x, resid, nnz = pkg.host_sparse_trace(row, h, cfg)
        assert rc == 0
        xs.append(x.copy())
        rs.append(resid)
        ns.append(nnz)
    return np.array(xs), np.array(rs, np.float64), np.array(ns)


def _check_resid_nnz(y, h, c, x, resid, nnz):
    want = model.resid_of(y, h, c, x)
    assert np.all(np.abs(resid - want) <= 1e-5 * want + 1e-30), (resid, want)
    assert np.array_equal(nnz, (x != 0).sum(axis=1))


@pytest.mark.parametrize("P,c,nt", model.EXACT_SHAPES)
@pytest.mark.parametrize("accelerate", (0, 1))
def test_exact_cases(P, c, nt, accelerate):
    h, y = model.exact_case(P, c, nt)
    for n_iter in (0, 1, 2):
        want, want_nnz = model.exact_solution(h, c, y, n_iter, accelerate)
        cfg = pkg.sparse_cfg(P, c, n_iter, accelerate, model.EXACT_STEP, model.EXACT_REL, 0.0)
        x, resid, nnz = _host(y, h, cfg)
        assert np.array_equal(x, want), (P, c, nt, accelerate, n_iter)
        assert np.array_equal(nnz, want_nnz)
        _check_resid_nnz(y, h, c, x, resid, nnz)
        if n_iter == 0:
            assert not x.any() and not nnz.any()
        if n_iter == 2 and nt >= 33:
            assert 0.5 < (x != 0).mean() < 0.95  # the cases exercise the shrinkage on both sides


@pytest.mark.parametrize("P,c,shift", ((5, 2, 1), (5, 2, 4), (9, 8, 0), (16, 0, 15), (1, 0, 0)))
def test_pure_shift_and_identity(P, c, shift):
    """one non-zero tap: H moves a trace by shift - c samples and scales it by 3 (shift == c: three times the identity)"""
    taps = np.zeros(P, np.float32)
    taps[shift] = 3
    nt = 33
    h, y = model.exact_case(P, c, nt, taps=taps)
    for accelerate in (0, 1):
        for n_iter in (1, 2):
            want, want_nnz = model.exact_solution(h, c, y, n_iter, accelerate)
            x, resid, nnz = _host(y, h, pkg.sparse_cfg(P, c, n_iter, accelerate, model.EXACT_STEP, model.EXACT_REL, 0.0))
            assert np.array_equal(x, want) and np.array_equal(nnz, want_nnz)
    # one iteration without a threshold is step * H^T y: the trace moved back by shift - c samples
    x, _, _ = _host(y, h, pkg.sparse_cfg(P, c, 1, 0, 1.0, 0.0, 0.0))
    d = shift - c
    moved = np.zeros_like(y)
    if d >= 0:
        moved[:, :nt - d] = 3 * y[:, d:]
    else:
        moved[:, -d:] = 3 * y[:, :nt + d]
    assert np.array_equal(x, moved)


@pytest.mark.parametrize("P,c,nt,n_iter,accelerate", model.TOLERANCE_CONFIGS)
def test_tolerance_cases(P, c, nt, n_iter, accelerate):
    h, step, y = model.tolerance_case(P, c, nt)
    ref, bar = model.reference_and_bar(y, h, c, n_iter, accelerate, step)
    x, resid, nnz = _host(y, h, pkg.sparse_cfg(P, c, n_iter, accelerate, step, 0.05, 0.0))
    dev = model.deviation(x, ref["x"])
    print(f"P {P} c {c} nt {nt} n_iter {n_iter} accelerate {accelerate}: worst {dev.max():.3e} of bar {bar:.3e} = {dev.max() / bar:.3f}")
    assert np.all(dev <= bar), (dev.max(), bar)
    _check_resid_nnz(y, h, c, x, resid, nnz)
    assert np.all(nnz >= 2) and np.all(nnz < nt // 2)  # sparse, and both spikes present


def test_in_place_and_optional_outputs():
    h, y = model.exact_case(5, 2, 33)
    cfg = pkg.sparse_cfg(5, 2, 2, 1, model.EXACT_STEP, model.EXACT_REL, 0.0)
    want, _ = model.exact_solution(h, 2, y, 2, 1)
    lib = pkg.load_library()
    row = y[0].copy()
    assert lib.thz_host_sparse_trace(row.ctypes.data, row.size, h.ctypes.data, C.byref(cfg), row.ctypes.data, None, None) == 0
    assert np.array_equal(row, want[0])


def test_adjoint_identity():
    """<H x, r> == <x, H^T r>, each product through a one-iteration call without a threshold (step 1: x1 = H^T y); H of
    (h, c) is H^T of the reversed taps with centre P - 1 - c.  Integers throughout: both sides are exact."""
    rng = np.random.default_rng(23)
    for P, c, nt in ((5, 2, 33), (64, 0, 130), (33, 16, 257), (40, 39, 20)):
        h = rng.integers(-3, 4, P).astype(np.float32)
        x = rng.integers(-8, 9, nt).astype(np.float32)
        r = rng.integers(-8, 9, nt).astype(np.float32)
        rc, htr, _, _ = pkg.host_sparse_trace(r, h, pkg.sparse_cfg(P, c, 1, 0, 1.0, 0.0, 0.0))
        assert rc == 0
        rc, hx, _, _ = pkg.host_sparse_trace(x, h[::-1].copy(), pkg.sparse_cfg(P, P - 1 - c, 1, 0, 1.0, 0.0, 0.0))
        assert rc == 0
        T = model.toeplitz(h, c, nt)
        assert np.array_equal(hx.astype(np.float64), T @ x) and np.array_equal(htr.astype(np.float64), T.T @ r)
        assert np.dot(hx.astype(np.float64), r) == np.dot(x.astype(np.float64), htr)


def test_min_lambda_and_threshold():
    """lam = max(rel_lambda * gmax, min_lambda): a large min_lambda silences everything, and it wins only when larger"""
    h, y = model.exact_case(5, 2, 33)
    x, _, nnz = _host(y, h, pkg.sparse_cfg(5, 2, 2, 1, model.EXACT_STEP, model.EXACT_REL, 1e9))
    assert not x.any() and not nnz.any()
    a, _, _ = _host(y, h, pkg.sparse_cfg(5, 2, 2, 1, model.EXACT_STEP, model.EXACT_REL, 2.0 ** -20))
    want, _ = model.exact_solution(h, 2, y, 2, 1)
    assert np.array_equal(a, want)
    g0max = np.abs(y.astype(np.float64) @ model.toeplitz(h, 2, 33)).max(axis=1)
    lam = float(2 * model.EXACT_REL * g0max.max())  # above rel_lambda * gmax of every trace
    b, _, _ = _host(y, h, pkg.sparse_cfg(5, 2, 1, 0, model.EXACT_STEP, model.EXACT_REL, lam))
    want = model.solve(y, h, 2, 1, 0, model.EXACT_STEP, 0.0, lam, np.float64, check_exact=True)["x"]
    assert np.array_equal(b, want.astype(np.float32))


def test_refused_configurations():
    h = np.ones(5, np.float32)
    y = np.ones(33, np.float32)
    ok = dict(n_taps=5, center=2, n_iter=2, accelerate=1, step=0.01, rel_lambda=0.05, min_lambda=0.0)
    assert pkg.host_sparse_trace(y, h, pkg.sparse_cfg(**ok))[0] == 0
    bad = [dict(n_taps=0), dict(n_taps=pkg.SPARSE_MAX_TAPS + 1), dict(center=-1), dict(center=5), dict(n_iter=-1),
           dict(n_iter=pkg.SPARSE_MAX_ITER + 1), dict(accelerate=2), dict(accelerate=-1), dict(step=0.0), dict(step=-1.0),
           dict(step=np.inf), dict(step=np.nan), dict(rel_lambda=-0.1), dict(rel_lambda=np.nan), dict(rel_lambda=np.inf),
           dict(min_lambda=-1.0), dict(min_lambda=np.nan), dict(min_lambda=np.inf)]
    big = np.ones(pkg.SPARSE_MAX_TAPS + 1, np.float32)
    for change in bad:
        cfg = pkg.sparse_cfg(**{**ok, **change})
        assert pkg.host_sparse_trace(y, big, cfg)[0] == -1, change
    for value in (np.nan, np.inf, -np.inf):
        taps = h.copy()
        taps[3] = value
        assert pkg.host_sparse_trace(y, taps, pkg.sparse_cfg(**ok))[0] == -1
    lib, cfg = pkg.load_library(), pkg.sparse_cfg(**ok)
    x = np.zeros(pkg.SPARSE_MAX_NT + 1, np.float32)
    long = np.zeros(pkg.SPARSE_MAX_NT + 1, np.float32)
    assert lib.thz_host_sparse_trace(long.ctypes.data, long.size, h.ctypes.data, C.byref(cfg), x.ctypes.data, None, None) == -1
    assert lib.thz_host_sparse_trace(long.ctypes.data, long.size - 1, h.ctypes.data, C.byref(cfg), x.ctypes.data, None, None) == 0
    assert lib.thz_host_sparse_trace(long.ctypes.data, 0, h.ctypes.data, C.byref(cfg), x.ctypes.data, None, None) == -1
    assert lib.thz_host_sparse_trace(None, 33, h.ctypes.data, C.byref(cfg), x.ctypes.data, None, None) == -1
    assert lib.thz_host_sparse_trace(y.ctypes.data, 33, None, C.byref(cfg), x.ctypes.data, None, None) == -1
    assert lib.thz_host_sparse_trace(y.ctypes.data, 33, h.ctypes.data, None, x.ctypes.data, None, None) == -1
    assert lib.thz_host_sparse_trace(y.ctypes.data, 33, h.ctypes.data, C.byref(cfg), None, None, None) == -1
    # the largest configuration the limits admit
    cfg = pkg.sparse_cfg(pkg.SPARSE_MAX_TAPS, 255, 1, 1, 1e-3, 0.05, 0.0)
    assert pkg.host_sparse_trace(np.ones(pkg.SPARSE_MAX_NT, np.float32), np.ones(pkg.SPARSE_MAX_TAPS, np.float32), cfg)[0] == 0


def test_taps_longer_than_the_trace():
    """P > nt: most taps never meet a sample"""
    h, y = model.exact_case(65, 64, 17)
    for c, taps in ((64, h), (0, h), (30, h)):
        taps = taps.copy()
        taps[c] = 3
        for accelerate in (0, 1):
            want, want_nnz = model.exact_solution(taps, c, y, 2, accelerate)
            x, resid, nnz = _host(y, taps, pkg.sparse_cfg(65, c, 2, accelerate, model.EXACT_STEP, model.EXACT_REL, 0.0))
            assert np.array_equal(x, want) and np.array_equal(nnz, want_nnz)


def test_sparse_kernel():
    ref = np.zeros(50, np.float32)
    ref[20:25] = (1, -2, 5, 3, -1)
    rc, taps, step = pkg.host_sparse_kernel(ref, 7, 3)
    assert rc == 0 and np.array_equal(taps, (0, 1, -2, 5, 3, -1, 0))
    assert step == np.float32(1.0 / 12.0 ** 2)
    # a tie goes to the lowest index, the sign does not count
    ref[30] = -5
    assert np.array_equal(pkg.host_sparse_kernel(ref, 3, 1)[1], (-2, 5, 3))
    ref[10] = -5
    assert np.array_equal(pkg.host_sparse_kernel(ref, 3, 1)[1], (0, -5, 0))
    # the peak at either end of the vector: zeros outside [0, nref)
    edge = np.zeros(9, np.float32)
    edge[0], edge[1] = 4, 1
    assert np.array_equal(pkg.host_sparse_kernel(edge, 5, 2)[1], (0, 0, 4, 1, 0))
    assert np.array_equal(pkg.host_sparse_kernel(edge, 5, 4)[1], (0, 0, 0, 0, 4))
    assert np.array_equal(pkg.host_sparse_kernel(edge, 3, 0)[1], (4, 1, 0))
    edge = np.zeros(9, np.float32)
    edge[8], edge[7] = -4, 1
    rc, taps, step = pkg.host_sparse_kernel(edge, 5, 2)
    assert rc == 0 and np.array_equal(taps, (0, 1, -4, 0, 0)) and step == np.float32(1.0 / 25.0)
    assert np.array_equal(pkg.host_sparse_kernel(edge, 5, 0)[1], (-4, 0, 0, 0, 0))
    # more taps than the reference has samples
    rc, taps, step = pkg.host_sparse_kernel(np.array([1, 2], np.float32), 6, 3)
    assert rc == 0 and np.array_equal(taps, (0, 0, 1, 2, 0, 0)) and step == np.float32(1.0 / 9.0)
    # the step is taken in double
    h = model.pulse((np.arange(200) - 100) * 0.05).astype(np.float32)
    rc, taps, step = pkg.host_sparse_kernel(h, 64, 32)
    k0 = int(np.argmax(np.abs(h)))
    assert rc == 0 and np.array_equal(taps, h[k0 - 32:k0 + 32])
    assert step == np.float32(1.0 / np.abs(taps.astype(np.float64)).sum() ** 2)
    # refusals
    assert pkg.host_sparse_kernel(np.zeros(9, np.float32), 5, 2)[0] == -1
    for n_taps, center in ((0, 0), (pkg.SPARSE_MAX_TAPS + 1, 0), (5, -1), (5, 5)):
        assert pkg.host_sparse_kernel(ref, n_taps, center)[0] == -1
    lib, s, t = pkg.load_library(), C.c_float(), np.zeros(5, np.float32)
    assert lib.thz_host_sparse_kernel(None, 9, 5, 2, t.ctypes.data, C.byref(s)) == -1
    assert lib.thz_host_sparse_kernel(ref.ctypes.data, 0, 5, 2, t.ctypes.data, C.byref(s)) == -1
    assert lib.thz_host_sparse_kernel(ref.ctypes.data, 9, 5, 2, None, C.byref(s)) == -1
    assert lib.thz_host_sparse_kernel(ref.ctypes.data, 9, 5, 2, t.ctypes.data, None) == -1


def test_binding_constants():
    assert (pkg.BUF_SPARSE, pkg.BUF_SPARSE_RESID, pkg.BUF_SPARSE_NNZ) == (30, 31, 32)
    assert pkg.binding.STAGE_PCA == 15 and pkg.STAGE_ECHO == 14  # THZ_STAGE_COUNT stays 16
    assert (pkg.SPARSE_MAX_TAPS, pkg.SPARSE_MAX_NT, pkg.SPARSE_MAX_ITER) == (256, 4608, 4096)
    assert C.sizeof(pkg.SparseCfg) == 28
    assert pkg.load_library().thz_abi_version() == 2
    header = open(pkg.binding.__file__.replace("thz_image_explorer_amd/binding.py", "include/thzgpu.h")).read()
    for text in ("THZ_BUF_SPARSE = 30", "THZ_BUF_SPARSE_RESID = 31", "THZ_BUF_SPARSE_NNZ = 32", "THZ_STAGE_COUNT = 16",
                 "#define THZ_SPARSE_MAX_TAPS 256", "#define THZ_SPARSE_MAX_NT   4608", "#define THZ_SPARSE_MAX_ITER 4096"):
        assert text in header, text


def test_overlapping_echoes_are_resolved():
    """what the feature is for: a unit pulse and a +-0.6 echo 8 .. 39 samples behind it, closer than the pulse is wide.
    300 FISTA iterations, then the echo model (mode 0, two ranks, guard 4, threshold 0.3) on the spike trains: the delay
    is within one sample of the planted one at every pixel.  The same selection on the raw traces is off by more than a
    sample at more than 80 % of them."""
    h, step, y, gaps = model.thin_coating_traces()
    assert y.shape == (64, 384)
    x, resid, nnz = _host(y, h, pkg.sparse_cfg(64, 32, 300, 1, step, 0.05, 0.0))
    found = echo_map_model.echo_model(x, 0, 2, 4, 0.3)
    assert np.all(found["count"] == 2)
    delay = np.abs(found["index"][1] - found["index"][0])
    err = np.abs(delay - gaps)
    print("delay errors on the spike trains:", err.tolist())
    assert np.all(err <= 1), err
    raw = echo_map_model.echo_model(y, 0, 2, 4, 0.3)
    raw_err = np.abs(np.abs(raw["index"][1] - raw["index"][0]) - gaps)
    print("delay errors on the raw traces:  ", raw_err.tolist())
    assert (raw_err > 1).mean() > 0.8
    assert np.all(nnz < 40)
