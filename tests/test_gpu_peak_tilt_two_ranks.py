"""thz_group_session_estimate_tilt with two RANKS, one process each, on one GPU through tests/mock_rccl (see
test_gpu_group_two_ranks.py for what the mock is and is not): the gather of the three maps to rank 0 — the int32 image
as its bits —, the fit on rank 0 alone and its way back to the other rank through the u64 all-reduce.  Every field on
both ranks, and the gathered maps on rank 0, are one session's bit for bit."""
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import peak_tilt_model as model
from test_gpu_group_two_ranks import HERE, MOCK, ROOT, _build_mock

pytestmark = pytest.mark.gpu

NX, NY, NT, DX, DY = 17, 6, 200, 0.5, 1.0
TILT = (1.4, -1.1)       # of the recompute between the two estimates

RANK_SCRIPT = textwrap.dedent('''
    import os, sys, time
    sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
    import numpy as np
    import thz_image_explorer_amd as pkg
    import peak_tilt_model as model
    rank, world, uid_file, out_file = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4]
    nx, ny, nt, dx, dy = {geom!r}
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
    time_axis, cube, _, _, _ = model.planted_cube(nx, ny, nt, dx, dy, 1.5, -1.0, dead=0.1, seed=6)
    res = {{}}
    with pkg.Group(device=0, rank=rank, world=world, uid=uid) as g:
        gs = pkg.GroupSession(g, nx, ny, time_axis, dx, dy)
        try:
            gs.upload(cube, subtract_bias=False)
            cfg = pkg.chain_cfg_default(time_axis)
            cfg.tilt_x_deg, cfg.tilt_y_deg = {tilt!r}
            for name, which in (("raw", pkg.BUF_RAW), ("data", pkg.BUF_DATA)):
                if which == pkg.BUF_DATA:
                    gs.recompute(cfg)
                rc, fit = gs.estimate_tilt(which, pkg.PEAK_MAX, 0.25)
                res[name + "_rc"] = np.array([rc])
                res[name + "_fit"] = np.array(fit.as_tuple()[:6], np.float64)
                res[name + "_n"] = np.array([fit.n_used], np.uint64)
                if rank == 0:
                    res[name + "_index"], res[name + "_offset"], res[name + "_value"] = gs.peak_maps(nx * ny)
        finally:
            gs.close()
    np.savez(out_file, **res)
''')


def _single_session(engine):
    import thz_image_explorer_amd as pkg
    time_axis, cube, _, _, _ = model.planted_cube(NX, NY, NT, DX, DY, 1.5, -1.0, dead=0.1, seed=6)
    want = {}
    s = pkg.Session(engine, NX, NY, time_axis, DX, DY)
    try:
        s.upload(cube, subtract_bias=False)
        cfg = pkg.chain_cfg_default(time_axis)
        cfg.tilt_x_deg, cfg.tilt_y_deg = TILT
        for name, which in (("raw", pkg.BUF_RAW), ("data", pkg.BUF_DATA)):
            if which == pkg.BUF_DATA:
                s.recompute(cfg)
            rc, fit = s.estimate_tilt(which, pkg.PEAK_MAX, 0.25)
            want[name] = (rc, np.array(fit.as_tuple()[:6], np.float64), fit.n_used,
                          [s.download(b, npix=NX * NY) for b in (pkg.BUF_PEAK_INDEX, pkg.BUF_PEAK_OFFSET, pkg.BUF_PEAK_VALUE)])
    finally:
        s.close()
    return want


def test_two_rank_processes_match_single_session(engine, tmp_path):
    _build_mock()
    want = _single_session(engine)
    world = 2
    script = tmp_path / "rank.py"
    script.write_text(RANK_SCRIPT.format(root=ROOT, tests=HERE, geom=(NX, NY, NT, DX, DY), tilt=TILT))
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
    for name in ("raw", "data"):
        rc, fit, n, maps = want[name]
        assert rc == 0 and n > 0.8 * NX * NY
        for r in range(world):
            assert int(res[r][name + "_rc"][0]) == rc, (name, r)
            assert np.array_equal(res[r][name + "_fit"].view(np.uint64), fit.view(np.uint64)), (name, r)
            assert int(res[r][name + "_n"][0]) == n, (name, r)
        for key, ref in zip(("_index", "_offset", "_value"), maps):
            assert np.array_equal(res[0][name + key].view(np.uint32), ref.view(np.uint32)), (name, key)
            assert name + key not in res[1].files                       # the maps live on rank 0 alone
