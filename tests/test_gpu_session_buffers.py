"""Every device buffer a session or a group session keeps is allocated, grown, shrunk and reused by ONE long-lived
object driven through a sequence of configurations; after every step all it hands out must equal — np.array_equal —
what a FRESH object computes from the same cube, filters and regions under that step's configuration alone.  A block
of the wrong size, a stale flag over a new block or a kept value that outlived its buffer shows as a difference.
After three of the steps the identical recompute is repeated and no buffer may move: a steady state allocates nothing.

The grids are below the Deconvolution stage's 16 x 16 guard: the stage sizes its output buffers and passes its input
through (status 1), which is what the buffers are checked on here; its arithmetic has tests of its own."""
import ctypes as C
import os

import numpy as np
import pytest

import synth
import thz_image_explorer_amd as pkg
from test_gpu_keep_zeros import MEANS, PER_PIXEL, One, Two, same

pytestmark = pytest.mark.gpu

TILT_A, TILT_B = (2.0, -1.0), (3.0, 1.0)   # test_session_tilted_scan_changes_trace_length's, and a second length
PLOT_PIXEL = (1, 1)                        # inside the first block of every scale factor used, and of a group's first slab
MAX_INSTANCES = 500                        # fewer than either grid's voxels: the threshold comes from the select walk
POINTERS = (pkg.BUF_RAW,) + PER_PIXEL + MEANS


def copy_cfg(cfg):
    c = pkg.ChainCfg()
    C.memmove(C.byref(c), C.byref(cfg), C.sizeof(c))
    return c


def member_sessions(d):
    return [d.s] if isinstance(d, One) else [d.gs.member(i) for i in range(2)]


def snapshot(d, n_rois):
    """all per-pixel outputs, the three means, every region's means and count, one pixel's plot copy-out"""
    src = d.s if isinstance(d, One) else d.gs
    out = {w: src.download(w) for w in PER_PIXEL + MEANS}
    for r in range(n_rois):
        for k, v in src.roi(r).items():
            out[f"roi{r}_{k}"] = np.asarray(v)
    for k, v in member_sessions(d)[0].plot(*PLOT_PIXEL).items():
        out[f"plot_{k}"] = v
    return out


def voxel_snapshot(d, vcfg):
    """count, threshold, the records and the opacity cube(s)"""
    if isinstance(d, One):
        inst, thr, dims = d.s.voxels(vcfg, max_instances=MAX_INSTANCES)
        count = len(inst)
    else:
        inst, thr, dims, count = d.gs.voxels(vcfg, max_instances=MAX_INSTANCES)
    out = dict(count=np.asarray(count), threshold=np.asarray(thr), dims=np.asarray(dims))
    for f in inst.dtype.names:
        out[f"inst_{f}"] = inst[f]
    for i, m in enumerate(member_sessions(d)):
        out[f"opacity{i}"] = m.download(pkg.BUF_OPACITY)
    return out


def pointers(d):
    if isinstance(d, One):
        return [d.eng.lib.thz_session_buffer(d.s.h, w) for w in POINTERS]
    return [d.gs.member_buffer(i, w) for i in range(2) for w in POINTERS] + \
           [d.g.lib.thz_group_session_result(d.gs.h, w) for w in PER_PIXEL]


def deconvolve(d, psf, dcfg):
    return (d.s if isinstance(d, One) else d.gs).deconvolve(psf, dcfg)


def drive(make, nx, ny, nt, nt_out_ok):
    time, cube = synth.make_cube(nx, ny, nt)
    cube = (cube * np.float32(4.0)).astype(np.float32)   # envelope maxima above the opacity threshold (test_session_voxels)
    ids = np.arange(nx * ny, dtype=np.uint64) + 1000
    cube2 = synth.make_traces(ids, nt, subtract_bias=True).reshape(nx, ny, nt)
    small = np.array([[1, 1], [3, 1], [3, 3], [1, 3]], np.int64)
    large = np.array([[0, 0], [nx - 1, 0], [nx - 1, ny - 1], [0, ny - 1]], np.int64)
    corner = np.array([[nx - 3, 0], [nx - 1, 0], [nx - 1, 2]], np.int64)
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", "psf_sample.npz"))
    psf, dcfg = pkg.psf_from_npz(z), pkg.DeconvCfg(20, 6, 0.4, 3.0, 0.5)   # test_session_deconvolution_stage's
    vcfg = pkg.voxel_cfg_default()

    state = dict(cube=cube, rois=[], cfg=pkg.chain_cfg_default(time))
    long_lived = make(time)
    long_lived.upload(cube)

    def fresh_after(then):
        """a fresh object brought to the current cube, regions and configuration; `then` runs on both"""
        f = make(time)
        try:
            f.upload(state["cube"])
            f.set_rois(state["rois"])
            f.recompute(copy_cfg(state["cfg"]))
            return then(f)
        finally:
            f.close()

    def step(name, steady=False, **changes):
        if "rois" in changes:
            state["rois"] = changes.pop("rois")
            long_lived.set_rois(state["rois"])
        if "tilt" in changes:
            tilt = changes.pop("tilt")
            state["cfg"].tilt_x_deg, state["cfg"].tilt_y_deg = tilt if tilt else (0.0, 0.0)
        for k, v in changes.items():
            setattr(state["cfg"], k, v)
        long_lived.recompute(copy_cfg(state["cfg"]))
        n = len(state["rois"])
        same(snapshot(long_lived, n), fresh_after(lambda f: snapshot(f, n)), name)
        if steady:   # (asking for the pointers voids the kept zeros and phases: the first repeat writes everything again)
            before = pointers(long_lived)
            for _ in range(3):
                long_lived.recompute(copy_cfg(state["cfg"]))
            assert pointers(long_lived) == before, f"step '{name}': a buffer moved in the steady state"
            assert all(before), f"step '{name}': a buffer is absent"
            same(snapshot(long_lived, n), fresh_after(lambda f: snapshot(f, n)), name + ", repeated")

    def nt_out():
        return member_sessions(long_lived)[0].nt_out

    try:
        step("1 default chain", steady=True)
        step("2 scale factor 2", scale_factor=2)
        step("3 scale factor 3, ragged", scale_factor=3)
        step("4 scale factor 1", steady=True, scale_factor=1)
        step("5 tilt on", tilt=TILT_A)
        n_a = nt_out()
        assert nt_out_ok(n_a), n_a
        step("6 another tilt angle", tilt=TILT_B)
        assert nt_out_ok(nt_out()) and nt_out() != n_a, (n_a, nt_out())
        step("7 tilt off", steady=True, tilt=None)
        assert nt_out() == nt
        step("8 one region", rois=[small])
        step("9 three regions", rois=[small, large, corner])
        step("10 reference-order means with the regions", want_means=2)
        step("11 tilt on with the regions", tilt=TILT_A)
        step("12 no regions", rois=[])

        def deconvolved(d):
            status = deconvolve(d, psf, dcfg)
            return dict(snapshot(d, 0), status=np.asarray(status))

        same(deconvolved(long_lived), fresh_after(deconvolved), "13 deconvolve on the full grid")
        step("14a scale factor 2", scale_factor=2)
        same(deconvolved(long_lived), fresh_after(deconvolved), "14b deconvolve again")
        same(voxel_snapshot(long_lived, vcfg), fresh_after(lambda f: voxel_snapshot(f, vcfg)), "15a voxels on that grid")
        step("15b scale factor 1", scale_factor=1)
        same(voxel_snapshot(long_lived, vcfg), fresh_after(lambda f: voxel_snapshot(f, vcfg)), "15c voxels again")
        state["cube"], state["cfg"] = cube2, pkg.chain_cfg_default(time)
        long_lived.upload(cube2)
        step("16 a second cube, default chain")
    finally:
        long_lived.close()


SHAPES = [
    # the fused family: kept zeros and kept phases meet a reallocation, a tilt gives a one-launch chain
    pytest.param((8, 6, 1024), lambda n: 1025 <= n <= 1280, id="8x6x1024"),
    # the generic kernels: a tilt takes the staged path and builds the extended cube
    pytest.param((6, 4, 64), lambda n: n > 64, id="6x4x64"),
]


@pytest.mark.parametrize("shape, nt_out_ok", SHAPES)
def test_session_buffers_through_every_resize(engine, shape, nt_out_ok):
    nx, ny, nt = shape
    drive(lambda time: One(engine, nx, ny, time, False), nx, ny, nt, nt_out_ok)


def test_group_of_two_buffers_through_every_resize():
    """the gathered copies' growth, the carry rows over the slab edge (4 rows per slab admit the scale factors 2 and
    3) and the two sizing functions the group shares with a session"""
    nx, ny, nt = 8, 6, 1024
    with pkg.Group(devices=[0, 0]) as g:
        drive(lambda time: Two(g, nx, ny, time, False), nx, ny, nt, lambda n: 1025 <= n <= 1280)
