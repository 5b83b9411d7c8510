"""A session's steady-state recompute leaves out the inverse transform's products with the zeros of its band pass
(fft_f.hpp "band pruning": the kCfgLow build of the inverse transform's input).
One nt = 4096 session of 2 059 traces — a full round of 256 blocks x 8 waves plus a ragged second one — is driven
through upload -> recompute (writes everything) -> recompute (pruned) -> a wider band (past bin N/2 + M1: the keep
build) -> the default band again (the keep range is still the wide one) -> once more (pruned again), and after every
step its outputs must be those of a session driven identically with THZ_F_KEEP_ZEROS=0 in a process of its own, which
writes and computes everything: spectrum, amplitudes, phases, image and means bit for bit (the spectrum's out-of-band
zeros up to their sign, which the keep range leaves as an earlier launch stored it: canon_fft), time traces bit for bit
once -0 is read as +0 (the one thing pruning may change is the sign of an exact zero), NaNs compared as NaNs.  The two
pruned recomputes must agree in every bit (the in-launch sums are deterministic), a handful of rows must match the
oracle at the tolerances of test_gpu_session.py, and a same-device group of two must give the single session's rows."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))

import pytest

import synth
import thz_image_explorer_amd as pkg

pytestmark = pytest.mark.gpu

NX, NY, NT = 29, 71, 4096          # 2 059 traces
NF = NT // 2 + 1
PER_PIXEL = (("fft", pkg.BUF_FFT), ("amplitudes", pkg.BUF_AMPLITUDES), ("phases", pkg.BUF_PHASES), ("data", pkg.BUF_DATA),
             ("img", pkg.BUF_IMG))
MEANS = (("avg_fft", pkg.BUF_AVG_FFT), ("avg_amplitudes", pkg.BUF_AVG_AMPLITUDES), ("avg_phases", pkg.BUF_AVG_PHASES))
NAN_AT, INF_AT = 700, 2053         # first round / ragged second round
# name: (complex multiplier, want_means, non-finite traces — their NaNs make every mean a NaN, so the means get a clean cube)
# "negative_plugin": a real plugin that is negative at every bin, so the multiplier is -0 outside the band — still a zero:
# the session keeps its range and prunes
VARIANTS = {"real": (False, 0, True), "complex": (True, 0, True), "real_means": (False, 1, False), "complex_means": (True, 1, False),
            "negative_plugin": (False, 1, False)}
STEPS = (("first recompute", (0.2, 5.0)), ("pruned", (0.2, 5.0)), ("wider band", (0.1, 7.0)), ("default band again", (0.2, 5.0)),
         ("pruned again", (0.2, 5.0)))


def cube_of(bad):
    time, cube = synth.make_cube(NX, NY, NT)
    cube = cube.copy()
    if bad:
        flat = cube.reshape(NX * NY, NT)
        flat[NAN_AT, NT // 5] = np.nan
        flat[INF_AT, 17] = np.inf
    return time, cube


def multiplier():
    H = np.empty((NF, 2), np.float32)
    H[:, 0] = 0.8 + 0.1 * np.cos(np.arange(NF) * 0.03)
    H[:, 1] = 0.2 * np.sin(np.arange(NF) * 0.05)
    return H


def canon(a, zero_sign_free):
    """the array's bits with every NaN made the same one, and -0 made +0 where the sign of a zero is free"""
    a = np.ascontiguousarray(a, np.float32)
    if zero_sign_free:
        a = a + np.float32(0.0)
    b = a.view(np.uint32).copy()
    b[np.isnan(a)] = 0x7FC00000
    return b


def canon_fft(fft, amp):
    """the spectrum's bits, -0 read as +0 in the bins whose stored amplitude is zero: the bins the band pass zeroes.
    There a full write stores X times a zero, whose sign follows the staged multiplier table — the band-limited table
    (kCfgBand) holds (+0, +0) outside the band, the full one H * 0, which is -0 where H is negative — while a launch
    with a keep range leaves the zero an earlier launch stored.  The two sessions run different tables in the 'wider
    band' step with the complex multiplier and the means; the keep range has always left that sign open
    (test_gpu_keep_zeros.py).  Every other bin, and every bin of a non-finite trace, is compared bit for bit."""
    fft = np.ascontiguousarray(fft, np.float32).reshape(-1, 2)
    dead = np.ascontiguousarray(amp, np.float32).reshape(-1) == 0
    b = canon(fft, False)
    b[dead] = canon(fft[dead], True)
    return b


def digests(snap):
    out = {k: hashlib.sha1(canon(v, k == "data").tobytes()).hexdigest() for k, v in snap.items() if k != "fft"}
    out["fft"] = hashlib.sha1(canon_fft(snap["fft"], snap["amplitudes"]).tobytes()).hexdigest()
    return out


def snapshot(dl, means):
    return {k: dl(w) for k, w in PER_PIXEL + (MEANS if means else ())}


def run_variant(eng, name, each=None):
    """drives one session through STEPS; -> {step: digests}; each(step, snapshot, session) sees every step"""
    cm, means, bad = VARIANTS[name]
    time, cube = cube_of(bad)
    s = pkg.Session(eng, NX, NY, time)
    out = {}
    try:
        s.upload(cube, subtract_bias=False)
        if cm:
            s.set_fd_filters(None, multiplier())
        if name == "negative_plugin":
            s.set_fd_filters(-multiplier()[:, 0].copy(), None)
        cfg = pkg.chain_cfg_default(time)
        cfg.want_means = means
        for step, (lo, hi) in STEPS:
            cfg.fd_low, cfg.fd_high = lo, hi
            s.recompute(cfg)
            snap = snapshot(s.download, means)
            out[step] = digests(snap)
            if each:
                each(step, snap, cfg)
    finally:
        s.close()
    return out


@pytest.fixture(scope="module")
def full_writes(tmp_path_factory):
    """every variant from a process of its own with THZ_F_KEEP_ZEROS=0: no keep range, nothing pruned"""
    out = str(tmp_path_factory.mktemp("band_prune") / "full.json")
    env = dict(os.environ, THZ_F_KEEP_ZEROS="0")
    r = subprocess.run([sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), out], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:]
    with open(out) as f:
        return json.load(f)


def oracle_rows(cube, time, cfg, rows):
    from test_gpu_session import oracle_chain
    return oracle_chain(cube.reshape(NX * NY, 1, NT)[rows], time, cfg)


@pytest.mark.parametrize("name", list(VARIANTS))
def test_pruned_session_equals_full_writes(engine, full_writes, name):
    from test_gpu_parity import TOL, rel
    assert "THZ_F_KEEP_ZEROS" not in os.environ and "THZ_F_LOW" not in os.environ
    cm, means, bad = VARIANTS[name]
    time, cube = cube_of(bad)
    rows = np.array([0, 1, NAN_AT - 1, NAN_AT + 1, 1030, 2047, 2048, INF_AT + 1, NX * NY - 1])

    def each(step, snap, cfg):
        if bad:
            for k in ("fft", "amplitudes", "data"):
                v = snap[k].reshape(NX * NY, -1)
                assert not np.isfinite(v[NAN_AT]).all() and not np.isfinite(v[INF_AT]).all(), (step, k, "the non-finite traces")
                assert np.isfinite(np.delete(v, [NAN_AT, INF_AT], axis=0)).all(), (step, k, "every other trace")
        if name == "negative_plugin" and step == "pruned":
            amp = snap["amplitudes"].reshape(NX * NY, NF)
            assert (amp[:, 1100:] == 0).all() and np.signbit(amp[:, 1100:]).all(), "the amplitudes outside the band are |X| * -0"
        if cm or name == "negative_plugin" or step not in ("pruned", "wider band"):
            return  # (the oracle has no complex multiplier and no plugin)
        ref = oracle_rows(cube, time, cfg, rows)
        scale = np.abs(ref["fft"]).max()
        assert rel(snap["fft"].reshape(NX * NY, NF, 2)[rows], ref["fft"].reshape(len(rows), NF, 2), scale) < TOL, step
        assert rel(snap["amplitudes"].reshape(NX * NY, NF)[rows], ref["amp"].reshape(len(rows), NF), scale) < TOL, step
        assert rel(snap["data"].reshape(NX * NY, NT)[rows], ref["data"].reshape(len(rows), NT)) < TOL, step
        assert rel(snap["img"].reshape(NX * NY)[rows], ref["img"].reshape(len(rows))) < TOL, step

    got = run_variant(engine, name, each)
    for step, _ in STEPS:
        for k, d in got[step].items():
            assert d == full_writes[name][step][k], f"{name}, step '{step}': {k} differs from the session that computes everything"
    assert got["pruned"] == got["pruned again"], "two pruned recomputes of the same configuration"


def test_group_of_two_gives_the_single_sessions_rows(engine):
    time, cube = cube_of(False)
    cfg = pkg.chain_cfg_default(time)
    cfg.want_means = 1
    s = pkg.Session(engine, NX, NY, time)
    try:
        s.upload(cube, subtract_bias=False)
        with pkg.Group(devices=[0, 0]) as g:
            gs = pkg.GroupSession(g, NX, NY, time)
            try:
                gs.upload(cube, subtract_bias=False)
                for step in ("first recompute", "pruned"):
                    s.recompute(cfg)
                    gs.recompute(cfg, 1, pkg.GATHER_ALL)
                    one, two = snapshot(s.download, False), snapshot(gs.download, False)
                    for k in one:
                        assert np.array_equal(canon(one[k], k == "data"), canon(two[k], k == "data")), (step, k)
                    # the group adds its members' sums: another order of the same 2 059 non-negative terms, n eps at the most
                    a1, a2 = s.download(pkg.BUF_AVG_AMPLITUDES), gs.download(pkg.BUF_AVG_AMPLITUDES)
                    assert np.allclose(a1, a2, rtol=NX * NY * 2.0 ** -24, atol=0.0), step
            finally:
                gs.close()
    finally:
        s.close()


if __name__ == "__main__":
    assert os.environ.get("THZ_F_KEEP_ZEROS") == "0"
    eng = pkg.Engine(0)
    try:
        res = {name: run_variant(eng, name) for name in VARIANTS}
    finally:
        eng.close()
    with open(sys.argv[1], "w") as f:
        json.dump(res, f)
