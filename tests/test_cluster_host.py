"""The k-means layer on the CPU (csrc/cluster_host.cpp, binding.py): names, constants and struct sizes,
thz_host_cluster_update against the numpy model of cluster_model.py, and the planted three-material scan through the CPU
oracle chain and the MODEL alone.

The planted property (the model alone on the oracle chain's amplitudes of the 16 x 12 x 1001 scan, 0.2 .. 5 THz, 241
bins, K = 3, farthest-first): the loop converges and the labels are the planted partition exactly, up to a permutation.
That is the condition that makes the session test of tests/test_gpu_cluster.py meaningful; it is not a bar for the
device."""
import ctypes
import functools
import os
import re

import numpy as np

import cluster_model as model
import thz_image_explorer_amd as pkg


def test_binding_names_constants_and_struct_sizes():
    assert (pkg.BUF_CLUSTER_LABELS, pkg.BUF_CLUSTER_DIST, pkg.BUF_CLUSTER_CENTROIDS) == (27, 28, 29)
    assert pkg.CLUSTER_MAX == 16 and pkg.STAGE_PCA == 15
    assert (pkg.CLUSTER_INIT_GIVEN, pkg.CLUSTER_INIT_FARTHEST) == (0, 1)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "thzgpu.h")).read()
    assert int(re.search(r"#define\s+THZ_CLUSTER_MAX\s+(\d+)", header).group(1)) == pkg.CLUSTER_MAX
    assert int(re.search(r"THZ_STAGE_COUNT\s*=\s*(\d+)", header).group(1)) == 16          # no stage of its own
    for name, value in (("LABELS", 27), ("DIST", 28), ("CENTROIDS", 29)):
        assert int(re.search(r"THZ_BUF_CLUSTER_%s\s*=\s*(\d+)" % name, header).group(1)) == value
    bound = {s[0] for s in pkg.SYMBOLS}
    lib = pkg.load_library()
    for name in ("thz_cluster_step", "thz_host_cluster_update", "thz_session_cluster", "thz_session_cluster_step",
                 "thz_session_cluster_row"):
        assert name in bound and hasattr(lib, name), name
    assert lib.thz_abi_version() == 2
    assert ctypes.sizeof(pkg.ClusterCfg) == 40 and ctypes.sizeof(pkg.ClusterOut) == 152
    cfg = pkg.cluster_cfg(10, 241)
    assert (cfg.first, cfg.count, cfg.step, cfg.n_clusters, cfg.init, cfg.max_iter, cfg.d_mask, cfg.centroids) == (10, 241, 1, 3, 1, 100, None, None)
    given = np.arange(6, dtype=np.float32).reshape(2, 3)
    cfg = pkg.cluster_cfg(0, 3, 2, 2, pkg.CLUSTER_INIT_GIVEN, 7, centroids=given)
    assert (cfg.step, cfg.n_clusters, cfg.init, cfg.max_iter) == (2, 2, 0, 7)
    assert np.array_equal(np.ctypeslib.as_array(ctypes.cast(cfg.centroids, ctypes.POINTER(ctypes.c_float)), (6,)), given.ravel())
    for s in (pkg.Session.cluster, pkg.Session.cluster_step, pkg.Session.cluster_row, pkg.Engine.cluster_step):
        assert callable(s)


def test_update_against_the_model():
    rng = np.random.default_rng(1)
    for k, n in ((1, 1), (2, 3), (3, 241), (16, 512), (8, 65)):
        sums = rng.standard_normal((k, n)) * 1e3
        counts = rng.integers(1, 5000, k).astype(np.uint64)
        counts[::3] = 0                                            # empty clusters, the first among them
        if k > 1:
            counts[1] = 1                                          # a single pixel: the centroid is that pixel, rounded
        prev = rng.standard_normal((k, n)).astype(np.float32)
        prev[0, 0] = np.float32(-0.0)                              # bit for bit: the sign of a zero stays
        rc, got = pkg.host_cluster_update(sums, counts, prev)
        assert rc == 0
        want = model.update(sums, counts, prev)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (k, n)
        assert np.array_equal(got[0].view(np.uint32), prev[0].view(np.uint32))
    # exactly (float)(sum / count) in f64: a quotient that rounds differently when formed in f32
    rc, got = pkg.host_cluster_update(np.array([[1.0, 16777217.0]]), [3], np.zeros((1, 2), np.float32))
    assert rc == 0 and got[0, 0] == np.float32(1.0 / 3.0) and got[0, 1] == np.float32(16777217.0 / 3.0)
    # in place: previous and centroids the same array
    lib = pkg.load_library()
    sums, counts = np.array([[2.0, 4.0], [9.0, 9.0]]), np.array([2, 0], np.uint64)
    both = np.array([[7, 7], [5, 6]], np.float32)
    assert lib.thz_host_cluster_update(sums.ctypes.data, counts.ctypes.data, 2, 2, both.ctypes.data, both.ctypes.data) == 0
    assert np.array_equal(both, [[1, 2], [5, 6]])


def test_update_refusals():
    lib = pkg.load_library()
    sums, counts = np.ones((2, 4)), np.array([1, 1], np.uint64)
    prev, out = np.zeros((2, 4), np.float32), np.full((2, 4), 3, np.float32)
    args = [sums.ctypes.data, counts.ctypes.data, 2, 4, prev.ctypes.data, out.ctypes.data]
    assert lib.thz_host_cluster_update(*args) == 0
    for i in (0, 1, 4, 5):
        bad = list(args)
        bad[i] = None
        assert lib.thz_host_cluster_update(*bad) == -1, i
    for k in (0, -1, 17):
        assert lib.thz_host_cluster_update(args[0], args[1], k, 4, args[4], args[5]) == -1, k
    for n in (0, 513):
        assert lib.thz_host_cluster_update(args[0], args[1], 2, n, args[4], args[5]) == -1, n
    big_s, big_n = np.ones((16, 512)), np.ones(16, np.uint64)
    big_p, big_o = np.zeros((16, 512), np.float32), np.zeros((16, 512), np.float32)
    assert lib.thz_host_cluster_update(big_s.ctypes.data, big_n.ctypes.data, 16, 512, big_p.ctypes.data, big_o.ctypes.data) == 0
    for bad in (np.nan, np.inf, -np.inf):
        out[:] = 3
        sums[1, 2] = bad
        assert lib.thz_host_cluster_update(*args) == -1
        assert np.all(out == 3)                                    # refused before anything is written
    sums[1, 2] = 1.0


def test_model_rules_on_a_hand_made_case():
    """the label, tie, NaN and farthest rules of the model itself, on numbers small enough to check by eye"""
    x = np.array([[0, 0], [2, 0], [1, 0], [np.nan, 0], [5, 5], [5, 5]], np.float32)
    cent = np.array([[0, 0], [2, 0], [2, 0]], np.float32)
    out = model.step(x, cent, prev_label=[0, 0, 0, 0, 0, 0], mask=[1, 1, 1, 1, 1, 0])
    assert out["label"].tolist() == [0, 1, 0, -1, 1, 1]           # a tie goes to the lowest c; duplicates stay empty
    assert np.isnan(out["dist2"][3]) and out["dist2"][[0, 1, 2, 4]].tolist() == [0, 0, 1, 34]
    assert out["counts"].tolist() == [2, 2, 0] and out["changed"] == 4 and out["farthest"] == 4
    assert out["inertia"] == 35 and np.array_equal(out["sums"], [[1, 0], [7, 5], [0, 0]])
    assert model.step(x[3:4], cent)["farthest"] == 1              # none: npix
    assert model.same_partition([0, 0, 1, 2], [2, 2, 0, 1]) and not model.same_partition([0, 0, 1, 2], [2, 1, 0, 0])
    assert not model.same_partition([0, 1, 1], [0, 0, 1])


@functools.lru_cache(maxsize=None)
def _planted():
    import oracle_binding as ob
    import synth
    time, cube, material = model.planted_scan()
    amp = ob.run_pipeline(cube, time, synth.oracle_chain(time))["amplitudes"]
    first, count = model.band_bins(time)
    return np.ascontiguousarray(amp.reshape(-1, amp.shape[-1])[:, first:first + count]), material


def test_planted_scan_model_recovers_the_materials():
    x, material = _planted()
    assert x.shape == (16 * 12, 241) and sorted(np.unique(material).tolist()) == [0, 1, 2]
    out = model.kmeans(x, 3)
    print(f"planted scan: {out['iterations']} steps, counts {out['counts'].tolist()}, inertia {out['inertia']:.6g}")
    assert out["converged"] == 1 and out["iterations"] <= 10
    assert model.same_partition(out["label"], material)
    assert sorted(out["counts"].tolist()) == sorted(np.bincount(material.ravel()).tolist())
    # the seeds already lie one in each material, and no label sits near a tie
    seeds = model.seeds(x, 3)
    assert model.same_partition(model.step(x, seeds)["label"], material)
    assert not model.margin_is_within(out["last"]["d2"], 0.05).any()
