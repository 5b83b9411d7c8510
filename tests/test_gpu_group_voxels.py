"""The 3-D tab's voxel instances over the WHOLE grid of a group session (thz_group_session_voxels).

The bar is one session over the same cube: the same threshold bits, the same count, the same records (raw bytes), and
nothing written past min(count, capacity).  "The same cube" is the group's final trace cube gathered to rank 0: the
reference runs thz_voxel_opacity / thz_voxel_threshold / thz_voxel_instances on it whole, on one context — exactly
what thz_session_voxels does.  Where a single Session's final cube equals the group's bit for bit (no trace pairs cut
by a slab edge), the group must also equal that Session's own voxels."""
import ctypes as C
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import oracle_binding as ob
import synth
import thz_image_explorer_amd as pkg
from test_gpu_group import _variant_cfg

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
MOCK_DIR = os.path.join(HERE, "mock_rccl")
MOCK = os.path.join(MOCK_DIR, "librccl_mock.so")
SELFTEST = os.path.join(ROOT, "thz_image_explorer_amd", "engine_voxel_selftest")
SENTINEL = 0xAB
SLACK = 8
GAIN = np.float32(20.0)   # the synthetic scans x 20: band-passed traces strong enough for the opacity rule's 1e-6 floor
THZ_OK, ERR_INVALID, ERR_NOT_READY = 0, -1, -4     # THZ_OK, THZ_ERR_INVALID, THZ_ERR_NOT_READY


def group_voxels_raw(gs, cfg, max_instances, scaling, orig, capacity, with_buffer=True):
    """thz_group_session_voxels through ctypes with SLACK records of sentinel bytes behind the capacity
    -> (rc, records (capacity + SLACK), count, threshold, dims)"""
    n, thr = C.c_uint64(), C.c_float()
    dims = np.zeros(3, np.float32)
    buf = np.full((capacity + SLACK) * pkg.VOXEL_INSTANCE.itemsize, SENTINEL, np.uint8)
    rc = gs.g.lib.thz_group_session_voxels(gs.h, C.byref(cfg), max_instances, scaling, orig[0], orig[1], orig[2],
                                           buf.ctypes.data if with_buffer else None, capacity, C.byref(n),
                                           C.byref(thr), dims.ctypes.data)
    return rc, buf.view(pkg.VOXEL_INSTANCE), n.value, thr.value, tuple(float(x) for x in dims)


def whole_cube_voxels(engine, data, span, cfg, max_instances, scaling, orig):
    """one context over the whole (gx, gy, nt) cube -> (records, threshold, dims, opacity)"""
    gx, gy, nt = data.shape
    d_in = engine.to_device(np.ascontiguousarray(data, np.float32))
    d_op = engine.empty(data.shape)
    try:
        engine.voxel_opacity(gx * gy, nt, d_in, cfg, d_op)
        thr = engine.voxel_threshold(d_op, data.size, max_instances)
        count, dims = engine.voxel_instances(d_op, gx, gy, nt, thr, span, scaling, orig, None, 0)
        d_rec = engine.alloc(max(count, 1) * pkg.VOXEL_INSTANCE.itemsize)
        count2, _ = engine.voxel_instances(d_op, gx, gy, nt, thr, span, scaling, orig, d_rec, count)
        assert count2 == count
        rec = d_rec.download((count,), pkg.VOXEL_INSTANCE)
        op = d_op.download(data.shape, np.float32)
        d_rec.free()
    finally:
        d_in.free()
        d_op.free()
    return rec, thr, dims, op


def live_cfg():
    """the default configuration without its opacity threshold: the synthetic scans' final traces are weak, and at
    0.1 every trace would be dead (all opacities 0)"""
    cfg = pkg.voxel_cfg_default()
    cfg.opacity_threshold = 0.0
    return cfg


def dense_cfg():
    """opacities > 0 almost everywhere (contrast 1 as well): selections at any k"""
    cfg = live_cfg()
    cfg.contrast = 1.0
    return cfg


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def f32_bits(x):
    return np.float32(x).view(np.uint32)


class Case:
    """a same-device group of `members` and one Session over the same cube and chain"""

    def __init__(self, engine, members, shape, cfg_fn=None, cube_fn=None, deconv=False):
        nx, ny, nt = shape
        self.engine, self.shape = engine, shape
        self.time, cube = synth.make_cube(nx, ny, nt)
        cube = cube * GAIN
        if cube_fn:
            cube = cube_fn(cube)
        self.cube = cube
        self.cfg = cfg_fn(self.time) if cfg_fn else pkg.chain_cfg_default(self.time)
        self.group = pkg.Group(devices=[0] * members)
        self.gs = pkg.GroupSession(self.group, nx, ny, self.time, 0.5, 0.5)
        self.single = pkg.Session(engine, nx, ny, self.time, 0.5, 0.5)
        self.deconv = deconv
        self.recompute()

    def recompute(self):
        self.gs.upload(self.cube, subtract_bias=False)
        self.gs.recompute(self.cfg, 1, pkg.GATHER_TIME)
        self.single.upload(self.cube, subtract_bias=False)
        self.single.recompute(self.cfg)
        if self.deconv:
            psf = pkg.psf_from_npz(np.load(os.path.join(HERE, "golden", "psf_sample.npz")))
            dcfg = pkg.DeconvCfg(20, 5, 0.4, 3.0, 0.5)
            assert self.gs.deconvolve(psf, dcfg) == 0
            assert self.single.deconvolve(psf, dcfg) == 0
        self.nt_out = self.gs.member(0).nt_out
        self.gx, self.gy = self.gs.grid()
        self.data = self.gs.download(pkg.BUF_DATA, nt_out=self.nt_out).reshape(self.gx, self.gy, self.nt_out)
        t = self.gs.member(0).time_out()
        self.span = float(t[-1] - t[0])
        self.orig = (self.shape[0], self.shape[1], self.nt_out)
        self.single_equal = same_bits(self.single.download(pkg.BUF_DATA).reshape(self.data.shape), self.data)

    def slab_rows(self):
        """rows of the outputs' grid per rank, in rank order"""
        rows = []
        for i in range(len(self.group.ranks)):
            gx_i, gy_i, _, _ = self.gs.member(i).grid()
            rows.append(gx_i)
        assert sum(rows) == self.gx
        return rows

    def live(self, vcfg):
        """voxels with an opacity > 0 in the whole cube (a max_instances below it selects a threshold > 0)"""
        _, _, _, op = whole_cube_voxels(self.engine, self.data, self.span, vcfg, 1, 1, self.orig)
        return int((op > 0).sum())

    def check(self, vcfg, max_instances, capacity=None):
        """group == whole cube (== Session where the cubes agree); returns (reference records, threshold, opacity)"""
        scaling = self.cfg.scale_factor if self.cfg.scale_factor > 1 else 1
        ref, thr, dims, op = whole_cube_voxels(self.engine, self.data, self.span, vcfg, max_instances, scaling, self.orig)
        cap = len(ref) if capacity is None else capacity
        rc, got, count, gthr, gdims = group_voxels_raw(self.gs, vcfg, max_instances, scaling, self.orig, cap)
        assert rc == THZ_OK, self.group.lib.thz_group_last_error(self.group.h).decode()
        assert f32_bits(gthr) == f32_bits(thr)
        assert count == len(ref)
        assert gdims == dims
        k = min(count, cap)
        assert same_bits(got[:k], ref[:k])
        assert np.all(got[k:].view(np.uint8) == SENTINEL), "records written past min(count, capacity)"
        if self.single_equal:
            inst, sthr, sdims = self.single.voxels(vcfg, max_instances, scaling, self.orig)
            assert f32_bits(sthr) == f32_bits(gthr) and len(inst) == count and sdims == gdims
            assert same_bits(got[:k], inst[:k])
        # the binding: counts first, then the whole list
        inst_b, thr_b, dims_b, count_b = self.gs.voxels(vcfg, max_instances, scaling, self.orig)
        assert count_b == count and f32_bits(thr_b) == f32_bits(thr) and dims_b == dims and same_bits(inst_b, ref)
        return ref, thr, op

    def close(self):
        self.gs.close()
        self.single.close()
        self.group.close()


@pytest.fixture
def case(engine):
    made = []

    def make(*a, **kw):
        c = Case(engine, *a, **kw)
        made.append(c)
        return c

    yield make
    for c in made:
        c.close()


def _scaled(s):
    return lambda t: _variant_cfg(t, f"scale{s}")


CHAINS = [
    (2, (8, 6, 1001), None, "nt 1001"),
    (3, (7, 6, 1001), None, "nt 1001, 3 members"),
    (2, (6, 4, 4096), None, "nt 4096"),
    (4, (11, 6, 1024), None, "nx 11 over 4 members"),
    (3, (10, 5, 256), None, "nx 10 over 3, odd ny"),
    (3, (10, 6, 256), lambda t: _variant_cfg(t, "tilt"), "tilt"),
    (2, (13, 6, 256), _scaled(2), "scale 2"),
    (3, (17, 8, 1024), _scaled(3), "scale 3"),
    (4, (17, 6, 256), _scaled(2), "scale 2 over 4 members"),
]


@pytest.mark.parametrize("members,shape,cfg_fn,label", CHAINS, ids=[c[3] for c in CHAINS])
def test_group_voxels_equal_one_session(case, members, shape, cfg_fn, label):
    c = case(members, shape, cfg_fn)
    if cfg_fn is not None and "tilt" in label:
        assert c.nt_out > shape[2]
    if cfg_fn is not None and "scale" in label:
        assert c.gx < shape[0]
    vcfg = live_cfg()
    n_total = c.gx * c.gy * c.nt_out
    ref, thr, _ = c.check(vcfg, n_total)              # everything fits: threshold 0.0, every voxel
    assert thr == 0.0 and len(ref) == n_total
    k = c.live(vcfg) // 2
    ref, thr, _ = c.check(vcfg, k)                    # a selection over the whole cube
    assert thr > 0.0 and len(ref) >= k
    vcfg = dense_cfg()
    vcfg.radius, vcfg.sigma = 20, 8.0                 # the wide-kernel opacity path
    ref, thr, _ = c.check(vcfg, n_total // 3)
    assert thr > 0.0


@pytest.mark.parametrize("members", [2, 3])
def test_group_voxels_after_group_deconvolution(case, members):
    c = case(members, (36, 32, 256), deconv=True)
    vcfg = live_cfg()
    ref, thr, _ = c.check(vcfg, c.live(vcfg) // 2)
    assert thr > 0.0


def test_threshold_comes_from_the_whole_cube(case):
    """every slab's n <= max_instances < n_total: a per-slab rule would give 0.0"""
    c = case(3, (9, 6, 256))
    vcfg = dense_cfg()
    rows = c.slab_rows()
    slab_n = max(rows) * c.gy * c.nt_out
    n_total = c.gx * c.gy * c.nt_out
    assert slab_n < n_total
    ref, thr, _ = c.check(vcfg, slab_n)
    assert thr > 0.0
    # the per-member call (what GpuEngine::voxels used to show) disagrees with the whole-cube answer
    inst0, thr0, _ = c.gs.member(0).voxels(vcfg, slab_n, 1, c.orig)
    assert thr0 == 0.0 != thr
    assert not same_bits(inst0, ref[:len(inst0)])


def test_kth_largest_in_another_slab(case):
    """member 0's rows are dead (zero traces): the threshold and every instance lie in the other slabs"""
    def dead_first_slab(cube):
        cube = cube.copy()
        cube[:3] = 0.0
        return cube

    c = case(3, (9, 6, 1024), cube_fn=dead_first_slab)
    vcfg = live_cfg()
    ref, thr, op = c.check(vcfg, c.live(vcfg) // 2)
    assert thr > 0.0
    assert op[:3].max() < thr                      # nothing of slab 0 reaches it
    live = (op >= thr).reshape(c.gx, -1).any(axis=1)
    assert not live[:3].any() and live[3:].any()


def test_ties_at_the_threshold(case):
    """max_instances below the number of live traces: the threshold is 1.0 (every live trace has a 1.0) and the
    count exceeds max_instances"""
    c = case(2, (8, 6, 256))
    vcfg = live_cfg()
    ref, thr, op = c.check(vcfg, 10)
    assert thr == 1.0 and len(ref) > 10
    assert len(ref) == int((op == 1.0).sum())


def test_capacity_cuts(case):
    c = case(3, (12, 6, 1024))
    vcfg = live_cfg()
    k = c.live(vcfg) // 2
    ref, thr, op = c.check(vcfg, k)
    rows = c.slab_rows()
    edges = np.cumsum([0] + rows)
    per = [int((op[edges[r]:edges[r + 1]] >= thr).sum()) for r in range(3)]
    assert sum(per) == len(ref) and all(per)
    for cap in (0, per[0] // 2, per[0] + per[1] // 2, len(ref) + 5):
        c.check(vcfg, k, capacity=cap)
    # count only: capacity 0 with no buffer
    rc, _, count, t, _ = group_voxels_raw(c.gs, vcfg, k, 1, c.orig, 0, with_buffer=False)
    assert rc == THZ_OK and count == len(ref) and f32_bits(t) == f32_bits(thr)


def test_slab_without_instances(case):
    """the middle slab's rows are dead: it contributes no record, the records after it follow on"""
    def dead_middle(cube):
        cube = cube.copy()
        cube[4:8] = 0.0
        return cube

    c = case(3, (12, 6, 256), cube_fn=dead_middle)
    vcfg = live_cfg()
    k = c.live(vcfg) // 2
    ref, thr, op = c.check(vcfg, k)
    assert thr > 0.0 and op[4:8].max() < thr and (op[8:] >= thr).any()
    c.check(vcfg, k, capacity=int((op[:4] >= thr).sum()) + 3)   # ends in slab 2, slab 1 empty


def test_errors_agree_and_the_group_recovers(engine):
    nx, ny, nt = 9, 6, 256
    time, cube = synth.make_cube(nx, ny, nt)
    cube = cube * GAIN
    vcfg = live_cfg()
    with pkg.Group(devices=[0, 0, 0]) as g:
        gs = pkg.GroupSession(g, nx, ny, time)
        try:
            gs.upload(cube, subtract_bias=False)
            rc, *_ = group_voxels_raw(gs, vcfg, 1000, 1, (nx, ny, nt), 0, with_buffer=False)
            assert rc == ERR_NOT_READY
            gs.recompute(pkg.chain_cfg_default(time), 1, pkg.GATHER_TIME)
            rc, *_ = group_voxels_raw(gs, vcfg, 1000, 1, (nx, ny, nt), 10, with_buffer=False)
            assert rc == ERR_INVALID
            gs.recompute(pkg.chain_cfg_default(time), 1, pkg.GATHER_TIME)
            data = gs.download(pkg.BUF_DATA).reshape(nx, ny, nt)
            ref, thr, dims, _ = whole_cube_voxels(engine, data, float(time[-1] - time[0]), vcfg, 1000, 1, (nx, ny, nt))
            rc, got, count, t, d = group_voxels_raw(gs, vcfg, 1000, 1, (nx, ny, nt), len(ref))
            assert rc == THZ_OK and count == len(ref) and f32_bits(t) == f32_bits(thr) and d == dims
            assert same_bits(got[:count], ref)
        finally:
            gs.close()


def test_group_voxels_vs_oracle(case):
    """once against the oracle on the final cube (tolerances of test_envelope_to_instances_flow)"""
    c = case(2, (12, 10, 1024))
    vcfg = live_cfg()
    max_inst = c.live(vcfg) // 2
    ref, thr, op = c.check(vcfg, max_inst)
    assert np.abs(op - ob.voxel_opacity(c.data)).max() < 1e-5
    assert thr == ob.voxel_threshold(op, max_inst)
    want, wdims = ob.voxel_instances(op, thr, c.span, 1, c.orig)
    inst, t, dims, count = c.gs.voxels(vcfg, max_inst, 1, c.orig)
    assert count == len(want) >= max_inst and dims == wdims
    assert np.array_equal(inst["position"], want["position"])
    assert np.array_equal(inst["scale"], want["scale"])
    assert np.array_equal(inst["color"][:, 3], want["color"][:, 3])
    assert np.abs(inst["color"][:, :3] - want["color"][:, :3]).max() < 1e-6


# ---- rank processes (the pattern of tests/test_gpu_group_two_ranks.py)

def _build_mock():
    src = os.path.join(MOCK_DIR, "mock_rccl.cpp")
    if os.path.exists(MOCK) and os.path.getmtime(MOCK) >= os.path.getmtime(src):
        return
    subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", src, "-o", MOCK,
                    "-L/opt/rocm/lib", "-lamdhip64", "-lpthread", "-lrt"], check=True)


RANK_SCRIPT = textwrap.dedent('''
    import os, sys, time
    sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
    import numpy as np
    import thz_image_explorer_amd as pkg
    import synth
    rank, world, uid_file, out_file = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4]
    nx, ny, nt = {shape!r}
    if rank == 0:
        uid = pkg.group_unique_id()
        with open(uid_file + ".tmp", "wb") as f:
            f.write(uid)
        os.rename(uid_file + ".tmp", uid_file)
    else:
        for _ in range(3000):
            if os.path.exists(uid_file):
                break
            time.sleep(0.01)
        uid = open(uid_file, "rb").read()
    time_axis, cube = synth.make_cube(nx, ny, nt)
    cube = cube * np.float32({gain!r})
    res = {{}}
    with pkg.Group(device=0, rank=rank, world=world, uid=uid) as g:
        gs = pkg.GroupSession(g, nx, ny, time_axis, 0.5, 0.5)
        try:
            gs.upload(cube, subtract_bias=False)
            gs.recompute(pkg.chain_cfg_default(time_axis), 1, pkg.GATHER_SMALL)
            vcfg = pkg.voxel_cfg_default()
            vcfg.opacity_threshold = 0.0
            for tag, k in (("all", nx * ny * nt), ("sel", {max_inst!r})):
                inst, thr, dims, count = gs.voxels(vcfg, k, 1, (nx, ny, nt))
                res["count_%s" % tag] = np.array([count], np.uint64)
                res["thr_%s" % tag] = np.array([thr], np.float32)
                res["dims_%s" % tag] = np.array(dims, np.float32)
                res["inst_%s" % tag] = inst.view(np.uint8)
        finally:
            gs.close()
    np.savez(out_file, **res)
''')


@pytest.mark.parametrize("world,shape", [(2, (7, 6, 1024)), (3, (8, 6, 256))])
def test_rank_processes_group_voxels(engine, tmp_path, world, shape):
    _build_mock()
    nx, ny, nt = shape
    time_axis, cube = synth.make_cube(nx, ny, nt)
    cube = cube * GAIN
    vcfg = live_cfg()
    s = pkg.Session(engine, nx, ny, time_axis, 0.5, 0.5)
    try:
        s.upload(cube, subtract_bias=False)
        s.recompute(pkg.chain_cfg_default(time_axis))
        s.voxels(vcfg, nx * ny * nt, 1, (nx, ny, nt), capacity=0)
        max_inst = int((s.download(pkg.BUF_OPACITY) > 0).sum()) // 2
        want = {tag: s.voxels(vcfg, k, 1, (nx, ny, nt)) for tag, k in (("all", nx * ny * nt), ("sel", max_inst))}
    finally:
        s.close()
    script = tmp_path / "rank.py"
    script.write_text(RANK_SCRIPT.format(root=ROOT, tests=HERE, shape=shape, max_inst=max_inst, gain=float(GAIN)))
    uid_file = str(tmp_path / "uid.bin")
    env = dict(os.environ, THZ_RCCL_LIB=MOCK, HSA_ENABLE_IPC_MODE_LEGACY="0")
    procs = [subprocess.Popen([sys.executable, str(script), str(r), str(world), uid_file, str(tmp_path / f"out{r}.npz")], env=env,
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(world)]
    outs = []
    for p in procs:
        try:
            o, _ = p.communicate(timeout=240)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()          # the exact children started above
            pytest.fail("a rank process did not finish: the ranks' calls do not pair up")
        outs.append(o)
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, f"rank {r}:\n{o[-3000:]}"
    res = [np.load(str(tmp_path / f"out{r}.npz")) for r in range(world)]
    for tag in ("all", "sel"):
        inst, thr, dims = want[tag]
        assert same_bits(res[0][f"inst_{tag}"].view(pkg.VOXEL_INSTANCE), inst)
        for r in range(world):
            assert int(res[r][f"count_{tag}"][0]) == len(inst)
            assert f32_bits(res[r][f"thr_{tag}"][0]) == f32_bits(thr)
            assert tuple(float(x) for x in res[r][f"dims_{tag}"]) == dims
            if r:
                assert res[r][f"inst_{tag}"].size == 0       # only rank 0 receives records
    assert float(res[0]["thr_sel"][0]) > 0.0


def test_group_voxels_through_real_rccl_single_rank(engine, monkeypatch):
    """THZ_GROUP_FORCE_RCCL: the all-reduces and the gather of the call go through librccl with one rank"""
    monkeypatch.setenv("THZ_GROUP_FORCE_RCCL", "1")
    nx, ny, nt = 6, 5, 1024
    time_axis, cube = synth.make_cube(nx, ny, nt)
    cube = cube * GAIN
    vcfg = live_cfg()
    s = pkg.Session(engine, nx, ny, time_axis)
    try:
        s.upload(cube, subtract_bias=False)
        s.recompute(pkg.chain_cfg_default(time_axis))
        s.voxels(vcfg, nx * ny * nt, 1, (nx, ny, nt), capacity=0)
        max_inst = int((s.download(pkg.BUF_OPACITY) > 0).sum()) // 2
        inst, thr, dims = s.voxels(vcfg, max_inst, 1, (nx, ny, nt))
    finally:
        s.close()
    with pkg.Group(device=0, rank=0, world=1, uid=pkg.group_unique_id()) as g:
        gs = pkg.GroupSession(g, nx, ny, time_axis)
        try:
            gs.upload(cube, subtract_bias=False)
            gs.recompute(pkg.chain_cfg_default(time_axis), 1, pkg.GATHER_SMALL)
            ginst, gthr, gdims, count = gs.voxels(vcfg, max_inst, 1, (nx, ny, nt))
            assert count == len(inst) and f32_bits(gthr) == f32_bits(thr) and gdims == dims and thr > 0.0
            assert same_bits(ginst, inst)
        finally:
            gs.close()


def test_engine_twin_voxel_selftest():
    assert os.path.exists(SELFTEST), "build it: make -C thz_image_explorer_amd/host"
    r = subprocess.run([SELFTEST], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and "ENGINE VOXEL SELFTEST OK" in r.stdout, r.stdout[-3000:]
