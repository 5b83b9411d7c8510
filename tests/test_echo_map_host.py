"""thz_host_echo_trace (csrc/echo_api.cpp) against the numpy model of tests/echo_map_model.py, on this machine: the
definition of the echo maps in every corner the header names, rank 0 against the arrival-time model, the refused
configurations, the binding's bookkeeping, and a property on the synthetic cube every other test uses.

Bars: indices, counts and values bit for bit; offsets within the arrival-time maps' bar,
8 eps_f32 (|y-| + 2 |y0| + |y+|) / |y- - 2 y0 + y+| of the fp64 parabola, and exactly 0 where the definition says so.

The property (a second pulse at every pixel, no third, its delay within 4 samples of the planted one) is taken with modes
1 and 2 only.  Mode 0 is left out on purpose: with |x| the two lobes of a derivative-of-Gaussian pulse tie, the main
pulse and its echo may settle on different lobes, and the delay is then off by the lobes' distance, about 10 samples."""
import numpy as np
import pytest

import echo_map_model as model
import peak_tilt_model as peak
import synth
import thz_image_explorer_amd as pkg


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _check(x, mode, k, guard, rel, tag=""):
    """one host call against the model; -> the host's (index, offset, value, count)"""
    x = np.ascontiguousarray(x, np.float32)
    idx, off, val, n = pkg.host_echo_trace(x, pkg.echo_cfg(mode, k, guard, rel))
    want = model.echo_model(x[None, :], mode, k, guard, rel)
    tag = (tag, mode, k, guard, rel)
    assert np.array_equal(idx, want["index"][:, 0]), (tag, idx, want["index"][:, 0])
    assert n == want["count"][0] and 1 <= n <= k, tag
    assert np.array_equal(_bits(val), _bits(want["value"][:, 0])), tag
    ok = want["ok"][:, 0]
    assert np.all(off[~ok] == 0.0) and not np.signbit(off[~ok]).any(), tag
    assert np.all(np.abs(off.astype(np.float64) - want["offset"][:, 0]) <= want["bar"][:, 0]), tag
    return idx, off, val, n


def _bump(x, at, height):
    """a three-sample pulse: height at `at`, half of it on either side"""
    x[at] = height
    if at > 0:
        x[at - 1] = max(x[at - 1], height / 2)
    if at + 1 < x.size:
        x[at + 1] = max(x[at + 1], height / 2)


def corner_traces(nt=96, guard=7):
    """name -> trace; written so that the interesting samples are where the name says"""
    out = {}
    x = np.zeros(nt, np.float32)
    for at in (20, 40, 60, 80):
        _bump(x, at, 5.0)
    out["equal pulses"] = x
    x = np.zeros(nt, np.float32)
    _bump(x, 15, 9.0)
    x[50:55] = 4.0                                   # a plateau: its lowest index, once
    out["plateau"] = x
    for gap in (guard - 1, guard, guard + 1):
        x = np.zeros(nt, np.float32)
        x[30], x[30 + gap] = 9.0, 6.0                # single-sample pulses, so that nothing else is a candidate
        out[f"gap {gap}"] = x
    x = np.full(nt, -1.0, np.float32)
    x[0], x[nt - 1], x[nt // 2] = 3.0, 2.0, 8.0
    out["candidates at 0 and nt-1"] = x
    x = np.zeros(nt, np.float32)
    x[25], x[70] = 8.0, np.float32(0.25) * np.float32(8.0)       # key == thr at rel 0.25: admitted
    out["key equals thr"] = x
    x = np.zeros(nt, np.float32)
    x[40 - guard:40 + guard + 1] = 10.0 - np.abs(np.arange(-guard, guard + 1))   # a wide pulse: 3.0 at the guard's edge
    x[75] = 2.5                                       # the true second pulse is smaller than the shoulder
    out["shoulder at the guard's edge"] = x
    x = np.sin(np.arange(nt) * 0.7).astype(np.float32)
    x[nt // 2] = np.nan
    out["NaN in the middle"] = x
    out["NaNs"] = np.full(nt, np.nan, np.float32)
    out["zeros"] = np.zeros(nt, np.float32)
    out["all equal"] = np.full(nt, 2.5, np.float32)
    x = np.sin(np.arange(nt) * 0.9).astype(np.float32)
    x[10], x[50], x[51] = np.inf, -np.inf, -np.inf
    out["+-Inf"] = x
    out["-Inf"] = np.full(nt, -np.inf, np.float32)
    x = np.full(nt, -np.inf, np.float32)
    x[0] = np.nan
    x[7] = np.nan
    out["NaN in front of -Inf"] = x
    x = np.full(nt, -2.0, np.float32)
    x[33], x[34], x[60], x[70] = -0.0, 0.0, 0.0, -0.0   # four zeros of either sign: one value, the lowest index first
    x[:33] = -1.0
    out["signed zeros"] = x
    return out


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_corner_traces(mode, k):
    guard = 7
    for name, x in corner_traces(guard=guard).items():
        for rel in (0.0, 0.2, 0.25):
            _check(x, mode, k, guard, rel, name)
            _check(-x, mode, k, guard, rel, "-" + name)


def test_corner_traces_say_what_their_names_say():
    """the model agrees with the host everywhere above; here the definition itself, by hand"""
    t = corner_traces(guard=7)
    idx, _, val, n = _check(t["equal pulses"], 1, 4, 7, 0.2)
    assert list(idx) == [20, 40, 60, 80] and n == 4                       # the lowest index first
    idx, _, _, n = _check(t["plateau"], 1, 3, 7, 0.2)
    assert list(idx) == [15, 50, -1] and n == 2                           # one candidate per plateau
    assert list(_check(t["gap 6"], 1, 2, 7, 0.2)[0]) == [30, -1]          # guard - 1 apart: inside the guard
    assert list(_check(t["gap 7"], 1, 2, 7, 0.2)[0]) == [30, 37]          # exactly the guard: reported
    assert list(_check(t["gap 8"], 1, 2, 7, 0.2)[0]) == [30, 38]
    idx, off, _, _ = _check(t["candidates at 0 and nt-1"], 1, 3, 7, 0.2)
    assert list(idx) == [48, 0, 95] and off[1] == 0.0 and off[2] == 0.0
    assert list(_check(t["key equals thr"], 1, 2, 7, 0.25)[0]) == [25, 70]
    assert list(_check(t["key equals thr"], 1, 2, 7, 0.2500001)[0]) == [25, -1]
    idx, _, val, _ = _check(t["shoulder at the guard's edge"], 1, 2, 7, 0.2)
    assert list(idx) == [40, 75] and val[1] == 2.5                        # not the shoulder's 3.0 at 33 or 47
    idx, off, val, n = _check(t["NaNs"], 0, 3, 7, 0.2)
    assert list(idx) == [0, -1, -1] and n == 1 and list(off) == [0, 0, 0] and np.isnan(val[0]) and list(val[1:]) == [0, 0]
    assert _check(t["zeros"], 0, 4, 7, 0.0)[3] == 1                       # no sample rises above the one in front ...
    assert list(_check(t["all equal"], 1, 2, 7, 0.0)[0]) == [0, -1]       # ... and sample 0 is rank 0 already
    assert list(_check(t["all equal"], 1, 2, 200, 0.0)[0]) == [0, -1]
    assert list(_check(t["signed zeros"], 1, 4, 7, 0.0)[0]) == [33, 60, 70, -1]   # -0 and +0 are one value


@pytest.mark.parametrize("nt", [1, 2, 3, 5])
def test_short_traces_and_wide_guards(nt):
    rng = np.random.default_rng(nt)
    for trial in range(40):
        x = rng.standard_normal(nt).astype(np.float32)
        if trial % 5 == 0:
            x[rng.integers(nt)] = np.nan
        if trial % 7 == 0:
            x[:] = x[0]
        for mode in (0, 1, 2):
            for k in (1, 2, 3, 4):
                for guard in (1, 2, nt, nt + 3, 2 ** 31 - 1):
                    idx, _, _, n = _check(x, mode, k, guard, 0.0, f"nt {nt} trial {trial}")
                    if guard >= nt:
                        assert n == 1 and np.all(idx[1:] == -1)           # rank 0 only


def test_random_traces():
    """noise with planted pulses, lengths around nothing in particular: the host loop against the vectorised model"""
    rng = np.random.default_rng(11)
    for nt in (17, 64, 257, 1001):
        for trial in range(6):
            x = rng.standard_normal(nt).astype(np.float32)
            for at in rng.integers(0, nt, 4):
                x[at] += rng.choice([-1, 1]) * rng.uniform(3, 9)
            for mode in (0, 1, 2):
                for guard in (1, 7, 300):
                    for rel in (0.0, 0.2):
                        _check(x, mode, 4, guard, rel, f"nt {nt} trial {trial}")


def test_rank0_is_the_peak_model():
    rng = np.random.default_rng(5)
    cases = list(corner_traces().values()) + [rng.standard_normal(n).astype(np.float32) for n in (1, 2, 3, 5, 64, 1001)]
    for x in cases:
        for mode in (0, 1, 2):
            idx, off, val, _ = pkg.host_echo_trace(x, pkg.echo_cfg(mode, 3, 5, 0.1))
            k, off64, value, bar, ok = peak.peak_model(x[None, :], mode)
            assert idx[0] == k[0] and _bits(val[:1])[0] == _bits(value)[0]
            assert abs(float(off[0]) - off64[0]) <= bar[0] and (ok[0] or off[0] == 0.0)


def test_bad_configurations():
    x = np.arange(8, dtype=np.float32)
    bad = [(-1, 2, 3, 0.2), (3, 2, 3, 0.2), (1, 0, 3, 0.2), (1, pkg.ECHO_MAX + 1, 3, 0.2), (1, 2, 0, 0.2), (1, 2, -4, 0.2),
           (1, 2, 3, -0.1), (1, 2, 3, float("nan")), (1, 2, 3, float("inf"))]
    for mode, k, guard, rel in bad:
        with pytest.raises(pkg.ThzError) as e:
            pkg.host_echo_trace(x, pkg.echo_cfg(mode, k, guard, rel))
        assert e.value.code == -1, (mode, k, guard, rel)
    with pytest.raises(pkg.ThzError) as e:                                # nt == 0
        pkg.host_echo_trace(np.zeros(0, np.float32), pkg.echo_cfg(1, 2, 3, 0.2))
    assert e.value.code == -1
    lib = pkg.load_library()
    assert lib.thz_host_echo_trace(None, 8, None, None, None, None, None) == -1
    # any output may be left out
    cfg = pkg.echo_cfg(1, 2, 3, 0.0)
    assert lib.thz_host_echo_trace(x.ctypes.data, x.size, cfg, None, None, None, None) == 0


def test_symbols_and_exports():
    bound = {s[0] for s in pkg.SYMBOLS}
    lib = pkg.load_library()
    for fn in ("thz_echo_map", "thz_layer_map", "thz_host_echo_trace", "thz_session_echo_map", "thz_session_layer_map"):
        assert fn in bound and hasattr(lib, fn), fn
    for name in ("EchoCfg", "LayerCfg", "echo_cfg", "layer_cfg", "host_echo_trace", "ECHO_MAX", "STAGE_ECHO", "BUF_ECHO_INDEX",
                 "BUF_ECHO_OFFSET", "BUF_ECHO_VALUE", "BUF_ECHO_COUNT", "BUF_LAYER_THICKNESS", "BUF_LAYER_DELAY"):
        assert hasattr(pkg, name), name
    assert (pkg.BUF_ECHO_INDEX, pkg.BUF_ECHO_OFFSET, pkg.BUF_ECHO_VALUE, pkg.BUF_ECHO_COUNT, pkg.BUF_LAYER_THICKNESS,
            pkg.BUF_LAYER_DELAY) == (18, 19, 20, 21, 22, 23)
    assert pkg.STAGE_ECHO == 14 and pkg.ECHO_MAX == 4
    for name in ("echo_map", "layer_map"):
        assert callable(getattr(pkg.Engine, name)) and callable(getattr(pkg.Session, name))
    import ctypes
    assert ctypes.sizeof(pkg.EchoCfg) == 16 and ctypes.sizeof(pkg.LayerCfg) == 28


def _planted_delay_samples(nx, ny):
    """the echo's delay behind the main pulse in synth.make_traces, in samples of the 0.05 ps axis"""
    ids = np.arange(nx * ny, dtype=np.uint64)
    _, _, r2, _ = synth.philox4x32(ids & synth.MASK32, ids >> np.uint64(32), 0, 1)
    delta = np.float32(3.0) + np.float32(17.0) * synth._u01(r2)
    return delta.astype(np.float64) / 0.05


@pytest.mark.parametrize("nt", [1024, 1001])
@pytest.mark.parametrize("mode", [1, 2])
def test_synthetic_cube_second_pulse(nt, mode):
    nx = ny = 12
    _, cube = synth.make_cube(nx, ny, nt)
    planted = _planted_delay_samples(nx, ny)
    cfg = pkg.echo_cfg(mode, 3, 30, 0.2)
    inside = found = thirds = 0
    worst = 0.0
    for p, x in enumerate(cube.reshape(nx * ny, nt)):
        idx, off, _, n = pkg.host_echo_trace(x, cfg)
        if idx[0] + planted[p] + 30 >= nt:                                 # the planted echo lies outside the trace
            continue
        inside += 1
        found += n >= 2
        thirds += n >= 3
        if n >= 2:
            delay = (float(idx[1]) + float(off[1])) - (float(idx[0]) + float(off[0]))
            worst = max(worst, abs(delay - planted[p]))
    print(f"nt {nt} mode {mode}: {found} of {inside} pixels with a second pulse, {thirds} thirds, worst delay error {worst:.2f} samples")
    assert inside == nx * ny and found == inside and thirds == 0
    assert worst <= 4.0
