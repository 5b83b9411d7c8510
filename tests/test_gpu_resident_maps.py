"""The lifecycle of every family of per-pixel results that stays resident in a session (csrc/session.hpp, ResidentMaps):
arrival times, optical-property maps, echo maps, layer maps, principal components, k-means and spike trains, all held to
one contract — absent before the first call; equal bit for bit to a fresh session's after a small call, a larger one that
makes the block grow, and the small one again; bounded by the last call's entries, not by the block's capacity; untouched
by a call refused for its arguments and by other families' calls; absent again after an upload.

Shapes: a 6 x 4 scan of 64 samples behind scale_factor = 2, so that THZ_BUF_DATA is a 3 x 2 grid and THZ_BUF_RAW the
6 x 4 one.  Every call here is deterministic (given centroids, given components), so equality needs no tolerance."""
import collections
import ctypes

import numpy as np
import pytest

import echo_map_model
import sparse_model
import thz_image_explorer_amd as pkg

pytestmark = pytest.mark.gpu

NX, NY, NT = 6, 4, 64
NF = NT // 2 + 1
NPIX = (3 * 2, NX * NY)                 # pixels of the small call's grid and of the large one's
INVALID, NOT_READY = -1, -4
PCA_COLS, CLUSTER_COLS, CLUSTER_K = 16, 8, 2
BANDS = ((2, 10), (10, 20), (20, 30))
ANCHOR = (2, 12)


@pytest.fixture(scope="module")
def scan(engine):
    time, cube, _, front = echo_map_model.wedge_scan(NX, NY, NT)
    _, ref_amp, ref_phase = engine.reference_spectrum(time, time, front)
    taps, step = sparse_model.pulse_taps(16, 8)
    rng = np.random.default_rng(3)
    return dict(time=time, cube=cube, ref_amp=ref_amp, ref_phase=ref_phase, taps=taps, step=step,
                components=rng.standard_normal((3, PCA_COLS)).astype(np.float32),
                mu=rng.standard_normal(PCA_COLS).astype(np.float32),
                centroids=rng.standard_normal((CLUSTER_K, CLUSTER_COLS)).astype(np.float32),
                score_centroids=np.array([[-1.0], [1.0]], np.float32), fresh={})


def _open(engine, x):
    sess = pkg.Session(engine, NX, NY, x["time"])
    sess.upload(x["cube"], subtract_bias=False)
    chain = pkg.chain_cfg_default(x["time"])
    chain.scale_factor = 2
    sess.recompute(chain)                # leaves spectra and final traces resident, on the 3 x 2 grid
    assert sess.grid()[:2] == (3, 2) and sess.nt_out == NT
    return sess


def _cube(big):
    return pkg.BUF_RAW if big else pkg.BUF_DATA


# ---- per family: the call at its small (big = 0) and its larger (big = 1) size, the planes (id, entries, words per
# entry) that call leaves, a call its argument rules refuse, and the call it makes as ANOTHER family's neighbour
def _peak(s, x, big, mode=pkg.PEAK_ABS):
    s.peak_map(_cube(big), mode)


def _peak_planes(big):
    return [(b, NPIX[big], 1) for b in (pkg.BUF_PEAK_INDEX, pkg.BUF_PEAK_OFFSET, pkg.BUF_PEAK_VALUE)]


def _optical(s, x, big, bands=None):
    bands = BANDS[:3 if big else 1] if bands is None else bands
    s.optical_maps(x["ref_amp"], x["ref_phase"], pkg.optical_cfg(1e-3, ANCHOR, bands))


def _optical_planes(big):
    nb = 3 if big else 1
    return ([(b, nb * NPIX[0], 1) for b in (pkg.BUF_OPT_N, pkg.BUF_OPT_ALPHA, pkg.BUF_OPT_KAPPA)]
            + [(pkg.BUF_OPT_WRAPS, NPIX[0], 1), (pkg.BUF_OPT_SLOPE, NPIX[0], 1)])


def _echo_ranks(big):
    return pkg.ECHO_MAX if big else 1


def _echo(s, x, big, ranks=None):
    s.echo_map(pkg.BUF_RAW, pkg.echo_cfg(pkg.PEAK_ABS, _echo_ranks(big) if ranks is None else ranks, 4, 0.1))


def _echo_planes(big):
    k = _echo_ranks(big)
    return ([(b, k * NPIX[1], 1) for b in (pkg.BUF_ECHO_INDEX, pkg.BUF_ECHO_OFFSET, pkg.BUF_ECHO_VALUE)]
            + [(pkg.BUF_ECHO_COUNT, NPIX[1], 1)])


def _layer(s, x, big, mode=None):
    """one row against a fixed arrival on one rank; ECHO_MAX - 1 rows between ECHO_MAX ranks"""
    _echo(s, x, big)
    s.layer_map(pkg.layer_cfg((pkg.LAYER_BETWEEN if big else pkg.LAYER_REFERENCE) if mode is None else mode, 0.005, 20, 0.25))


def _layer_planes(big):
    rows = pkg.ECHO_MAX - 1 if big else 1
    return [(b, rows * NPIX[1], 1) for b in (pkg.BUF_LAYER_THICKNESS, pkg.BUF_LAYER_DELAY)]


def _layer_neighbour(s, x):
    """of whichever echo maps are resident: the echo family's planes stay what they are"""
    if not s.eng.lib.thz_session_buffer(s.h, pkg.BUF_ECHO_INDEX):
        _echo(s, x, 0)
    s.layer_map(pkg.layer_cfg(pkg.LAYER_REFERENCE, 0.005, 20, 0.25))


def _pca(s, x, big, k=None):
    k = (3 if big else 1) if k is None else k
    s.pca_project(pkg.BUF_RAW, pkg.pca_cfg(10, PCA_COLS, 2, k), x["mu"], x["components"][:max(k, 1)])


def _pca_planes(big):
    k = 3 if big else 1
    return [(pkg.BUF_PCA_SCORES, k * NPIX[1], 1), (pkg.BUF_PCA_COMPONENTS, k * PCA_COLS, 1), (pkg.BUF_PCA_MEAN, PCA_COLS, 1)]


def _cluster(s, x, big, k=CLUSTER_K):
    s.cluster(_cube(big), pkg.cluster_cfg(5, CLUSTER_COLS, 3, k, pkg.CLUSTER_INIT_GIVEN, 1, centroids=x["centroids"]))


def _cluster_planes(big):
    return [(pkg.BUF_CLUSTER_LABELS, NPIX[big], 1), (pkg.BUF_CLUSTER_DIST, NPIX[big], 1),
            (pkg.BUF_CLUSTER_CENTROIDS, CLUSTER_K * CLUSTER_COLS, 1)]


def _cluster_neighbour(s, x):
    """k-means may read THZ_BUF_PCA_SCORES: on the first component's scores, which stay what they are"""
    assert s.eng.lib.thz_session_buffer(s.h, pkg.BUF_PCA_SCORES)
    cfg = pkg.cluster_cfg(0, 1, 1, CLUSTER_K, pkg.CLUSTER_INIT_GIVEN, 1, centroids=x["score_centroids"])
    out = pkg.ClusterOut()
    s.eng._check(s.eng.lib.thz_session_cluster(s.h, pkg.BUF_PCA_SCORES, ctypes.byref(cfg), ctypes.byref(out)))
    assert out.count == NPIX[1] and s.eng.lib.thz_session_buffer(s.h, pkg.BUF_CLUSTER_LABELS)


def _sparse(s, x, big, n_taps=16):
    s.sparse_deconv(_cube(big), x["taps"], pkg.sparse_cfg(n_taps, 8, 12, 1, x["step"], 0.05, 0.0))


def _sparse_planes(big):
    return [(pkg.BUF_SPARSE, NPIX[big], NT), (pkg.BUF_SPARSE_RESID, NPIX[big], 1), (pkg.BUF_SPARSE_NNZ, NPIX[big], 1)]


Family = collections.namedtuple("Family", "call planes refused neighbour")
FAMILIES = {
    "peak": Family(_peak, _peak_planes, lambda s, x: _peak(s, x, 1, mode=3), lambda s, x: _peak(s, x, 0)),
    "optical": Family(_optical, _optical_planes, lambda s, x: _optical(s, x, 1, bands=[(0, 4)]), lambda s, x: _optical(s, x, 0)),
    "echo": Family(_echo, _echo_planes, lambda s, x: _echo(s, x, 1, ranks=0), lambda s, x: _echo(s, x, 0)),
    "layer": Family(_layer, _layer_planes, lambda s, x: _layer(s, x, 0, mode=3), _layer_neighbour),
    "pca": Family(_pca, _pca_planes, lambda s, x: _pca(s, x, 1, k=0), lambda s, x: _pca(s, x, 0)),
    "cluster": Family(_cluster, _cluster_planes, lambda s, x: _cluster(s, x, 1, k=0), _cluster_neighbour),
    "sparse": Family(_sparse, _sparse_planes, lambda s, x: _sparse(s, x, 1, n_taps=0), lambda s, x: _sparse(s, x, 0)),
}
ALL_IDS = [b for f in FAMILIES.values() for b, _, _ in f.planes(0)]
assert sorted(ALL_IDS) == list(range(pkg.BUF_PEAK_INDEX, pkg.BUF_SPARSE_NNZ + 1))


def _download(s, which, entries, per):
    """-> (status, the words as uint32)"""
    out = np.full(max(entries * per, 1), 0xdeadbeef, np.uint32)
    return s.eng.lib.thz_session_download(s.h, which, 0, entries, out.ctypes.data), out[:entries * per]


def _absent(s, ids):
    for b in ids:
        assert not s.eng.lib.thz_session_buffer(s.h, b), b
        assert _download(s, b, 1, NT)[0] == NOT_READY, b


def _read(s, planes):
    """every plane in full, and nothing beyond its entries"""
    got = []
    for b, entries, per in planes:
        assert s.eng.lib.thz_session_buffer(s.h, b), b
        rc, words = _download(s, b, entries, per)
        assert rc == 0, (b, rc)
        assert _download(s, b, entries + 1, per)[0] == INVALID, b
        got.append(words)
    return got


def _fresh(engine, x, name, big):
    """what a session that has made no other call gives: computed once, shared, never changed"""
    if (name, big) not in x["fresh"]:
        s = _open(engine, x)
        try:
            FAMILIES[name].call(s, x, big)
            x["fresh"][name, big] = _read(s, FAMILIES[name].planes(big))
        finally:
            s.close()
    return x["fresh"][name, big]


def _same(got, want, tag):
    assert len(got) == len(want)
    for q, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and np.array_equal(g, w), (tag, q)


@pytest.mark.parametrize("name", list(FAMILIES))
def test_lifecycle(engine, scan, name):
    x, fam = scan, FAMILIES[name]
    ids = [b for b, _, _ in fam.planes(0)]
    s = _open(engine, x)
    try:
        _absent(s, ids)                                                     # 1: before the first call
        fam.call(s, x, 0)
        small = _read(s, fam.planes(0))
        _same(small, _fresh(engine, x, name, 0), "small")                   # 2: the smallest result
        fam.call(s, x, 1)
        _same(_read(s, fam.planes(1)), _fresh(engine, x, name, 1), "large")  # 3: the block has grown
        fam.call(s, x, 0)
        _same(_read(s, fam.planes(0)), small, "small again")                # 4: bounded by the result, not the capacity
        with pytest.raises(pkg.ThzError) as e:                              # 5: refused for its arguments
            fam.refused(s, x)
        assert e.value.code == INVALID
        _same(_read(s, fam.planes(0)), small, "after a refused call")
        # 6: the other families' calls, in an order that has the echo maps resident for the layer maps and the scores
        # for k-means.  The layer maps are made of the echo maps resident at the time and a later echo call does not
        # void them; k-means on THZ_BUF_PCA_SCORES leaves the principal components what they were.
        for other, f in FAMILIES.items():
            if other != name:
                f.neighbour(s, x)
        _same(_read(s, fam.planes(0)), small, "after the other families' calls")
        assert all(s.eng.lib.thz_session_buffer(s.h, b) for b in ALL_IDS)
        s.upload(x["cube"], subtract_bias=False)                            # 7: an upload voids every family
        _absent(s, ALL_IDS)
    finally:
        s.close()


def test_optical_maps_without_bands(engine, scan):
    """no band: the three band-major maps are absent, wraps and slope are there"""
    s = _open(engine, scan)
    try:
        _optical(s, scan, 1)
        _optical(s, scan, 0, bands=[])
        _absent(s, [pkg.BUF_OPT_N, pkg.BUF_OPT_ALPHA, pkg.BUF_OPT_KAPPA])
        got = _read(s, [(pkg.BUF_OPT_WRAPS, NPIX[0], 1), (pkg.BUF_OPT_SLOPE, NPIX[0], 1)])
        _same(got, _fresh(engine, scan, "optical", 0)[3:], "wraps and slope do not depend on the bands")
    finally:
        s.close()
