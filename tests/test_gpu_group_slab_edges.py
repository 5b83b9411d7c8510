"""Group slabs at the edge of the scale factor (include/thzgpu.h, thz_group_session): a block of s x s pixels whose rows
lie in two slabs is finished by the slab that holds its last row, and a split with a slab shorter than s is refused.

The rule depends on (nx, ny, world, s) alone, so every rank reaches the same answer before any exchange: scaling is
the identity when s <= 1, nx / s == 0 or ny / s == 0; otherwise the recompute is refused with THZ_ERR_UNSUPPORTED
exactly when nx / world < s (the smallest slab thz_host_slab cuts).  Everything the rule admits must equal one session
over the same cube: the grid, the per-pixel outputs bit for bit at a power-of-two length (the bars of
test_group_session_shards_what_it_used_to_refuse at 1001), the pixel means and a region of interest.  A refusal leaves
the group usable: the outputs stay those of the last recompute, and the next admitted recompute is one session's."""
import numpy as np
import pytest

import synth
import thz_image_explorer_amd as pkg
from test_gpu_parity import rel

pytestmark = pytest.mark.gpu

THZ_ERR_UNSUPPORTED = -2
NY = 7          # ragged in y for every scale factor below
BUFS = (pkg.BUF_IMG, pkg.BUF_DATA, pkg.BUF_FFT, pkg.BUF_AMPLITUDES, pkg.BUF_PHASES)
AVGS = (pkg.BUF_AVG_FFT, pkg.BUF_AVG_AMPLITUDES, pkg.BUF_AVG_PHASES)


def refused(nx, ny, world, sf):
    if sf <= 1 or nx // sf == 0 or ny // sf == 0:
        return False
    return nx // world < sf


def _poly(nx):
    return np.array([[0, 1], [7, 0], [3, nx], [0, nx // 2]], np.uint64)


def _cfg(time, sf, want_means):
    cfg = pkg.chain_cfg_default(time)
    cfg.scale_factor, cfg.want_means = sf, want_means
    return cfg


def _single(engine, nx, time, cube, cfg):
    s = pkg.Session(engine, nx, NY, time, 0.5, 0.5)
    try:
        s.upload(cube, subtract_bias=False)
        s.set_rois([_poly(nx)])
        s.recompute(cfg)
        want = {w: s.download(w) for w in BUFS + AVGS}
        want.update(grid=s.grid()[:2], nto=s.nt_out, roi=s.roi(0))
        return want
    finally:
        s.close()


def _assert_equals_single(gs, want, want_means, what):
    nto = want["nto"]
    assert gs.grid() == want["grid"], what
    pairs = nto & (nto - 1) != 0        # transformed in pairs of traces: a slab may pair them otherwise (last bits)
    for w in BUFS:
        got = gs.download(w)
        assert got.shape == want[w].shape, (what, w)
        if w == pkg.BUF_PHASES and pairs:
            d = got.astype(np.float64) - want[w]
            assert np.abs(d - 2 * np.pi * np.round(d / (2 * np.pi))).max() < 3e-3, (what, w)
        elif pairs:
            assert rel(got, want[w]) < 2e-6, (what, w)
        else:
            assert np.array_equal(got, want[w]), (what, w)
    for w in AVGS:
        got = gs.download(w)
        if want_means == 2 and not pairs:
            assert np.array_equal(got, want[w]), (what, w)       # the reference's order, slab after slab
        else:
            assert rel(got, want[w]) < 2e-6 or (w == pkg.BUF_AVG_PHASES and pairs), (what, w)
    r = gs.roi(0)
    assert r["count"] == want["roi"]["count"], what
    for k in ("signal_fft", "signal", "roi_data") + (() if pairs else ("phase_fft",)):
        ref = want["roi"][k]
        assert np.abs(r[k].astype(np.float64) - ref).max() <= 2e-6 * max(np.abs(ref).max(), 1e-30), (what, k)


def _sweep(engine, world, sf, nxs, nt):
    admitted = 0
    with pkg.Group(devices=[0] * world) as g:
        for nx in nxs:
            time, cube = synth.make_cube(nx, NY, nt)
            gs = pkg.GroupSession(g, nx, NY, time, 0.5, 0.5)
            try:
                gs.upload(cube, subtract_bias=False)
                gs.set_rois([_poly(nx)])
                if refused(nx, NY, world, sf):
                    for want_means in (1, 2):
                        with pytest.raises(pkg.ThzError) as e:
                            gs.recompute(_cfg(time, sf, want_means), 1, pkg.GATHER_ALL)
                        assert e.value.code == THZ_ERR_UNSUPPORTED, (nx, want_means)
                    # still usable: unscaled, it is one session; refused again, its outputs stay
                    cfg1 = _cfg(time, 1, 2)
                    want = _single(engine, nx, time, cube, cfg1)
                    gs.recompute(cfg1, 1, pkg.GATHER_ALL)
                    _assert_equals_single(gs, want, 2, (nx, "unscaled after a refusal"))
                    with pytest.raises(pkg.ThzError) as e:
                        gs.recompute(_cfg(time, sf, 2), 7, pkg.GATHER_ALL)
                    assert e.value.code == THZ_ERR_UNSUPPORTED, nx
                    _assert_equals_single(gs, want, 2, (nx, "refused after an unscaled recompute"))
                else:
                    admitted += 1
                    for want_means in (1, 2):
                        cfg = _cfg(time, sf, want_means)
                        want = _single(engine, nx, time, cube, cfg)
                        gs.recompute(cfg, 1, pkg.GATHER_ALL)
                        _assert_equals_single(gs, want, want_means, (nx, want_means))
            finally:
                gs.close()
    return admitted


@pytest.mark.parametrize("sf", [2, 3, 4])
@pytest.mark.parametrize("world", [2, 3, 4])
def test_group_slab_edges_sweep(engine, world, sf):
    """every nx from max(sf, world) to world * sf + 2 (ny 7, nt 256): refused exactly where the rule says, else one
    session's results.  The admitted splits include the smallest slabs (nx = world * sf) and blocks that cross slab
    edges (nx = world * sf + 1, + 2)."""
    nxs = range(max(sf, world), world * sf + 3)
    assert _sweep(engine, world, sf, nxs, 256) == 3


@pytest.mark.parametrize("world,sf,nxs", [(3, 3, (8, 10)), (4, 2, (7, 9, 10)), (2, 4, (9,))])
def test_group_slab_edges_odd_length(engine, world, sf, nxs):
    """the same at nt 1001: the paired-trace kernels, with the bars of test_group_session_shards_what_it_used_to_refuse"""
    _sweep(engine, world, sf, nxs, 1001)

