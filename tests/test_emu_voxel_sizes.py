"""The voxel envelope's kernels (csrc/voxel.hip, K15) in host-thread emulation at the sizes, radii and alignments that
switch their paths: the tables, references and bars of voxel_sizes.py through emu_voxel_opacity, emu_select_hist
and emu_voxel_instances.  test_gpu_voxel_sizes.py runs the same tables on the device.  Every opacity case's margins
(voxel_sizes.check_margins) are proven here, on the reference alone, before anything goes to a GPU.

What the emulation skips, and why (the device file runs all of it):
- OPACITY_LDS_CASES (nt 8192 radius 1100, nt 4100 radius 4096): the emulation's LDS has no limit, the block a launch
  gets shows nothing; test_lds_fit checks the launcher's arithmetic instead;
- the multi-trip cases trips-nt8 (8197 traces), trips-nt2052 (2051), trips-nt4100-r1 and trips-nt4100-r13 (1027
  each) and the isolation cases poison-nt8, poison-nt2052 and poison-nt4100: thousands of traces at a few
  milliseconds of barriers each; trips-nt4097 (the non-prefetching loop's second trip) and poison-nt4097 (its
  third) run.  Their inputs' margins are still proven here (test_opacity_margins_of_the_device_only_cases);
- select histograms above 257 values other than 4099 (every pattern) and 4095, 4096, 4097, 16387 (`rows`), the
  second, accumulating call above 257 values, and the k-th largest above 1285 values: a ballot is 64 exchanges of
  two barriers here, a histogram of 16 384 values takes 20 s;
- INSTANCE_TILE_CASES other than the 2049 traces (40 s each), INSTANCE_CARRY_CASE (526 337 traces: the grid cap and
  the scan's carry are its point); the capacities run at the tie threshold only, the other thresholds with the exact
  capacity.

Instances of k_voxel_opacity<NQ, VEC, WIDE> run here: all 24 (test_opacity_sizes); k_voxel_count / k_voxel_emit:
both forms, one and several 256-sample trips (test_instances_depths)."""
import ctypes as C

import numpy as np
import pytest

import thz_image_explorer_amd as pkg
import voxel_sizes as vs
from test_voxel_cpu import emu  # noqa: F401  (the fixture that builds and loads the emulation)

_P = C.c_void_p


def aligned_f32(n, off_bytes=0, fill=vs.SENTINEL):
    """n floats that start off_bytes behind a 16-byte boundary, inside an array filled with `fill`, guard floats on
    both sides -> (whole array, first index)"""
    raw = np.full(n + 24, fill, np.float32)
    first = ((-raw.ctypes.data // 4) % 4) + 8 + off_bytes // 4
    assert (raw.ctypes.data + 4 * first) % 16 == off_bytes
    return raw, first


def _ptr(raw, first):
    return C.c_void_p(raw.ctypes.data + 4 * first)


def emu_opacity(emu, case, cube, thr):
    """the emulated kernel on a case's cube -> output (npix, nt); guards and sentinels checked"""
    n = cube.size
    src, s0 = aligned_f32(n, 4 if case.form == "in+4" else 0)
    dst, d0 = aligned_f32(n, 4 if case.form == "out+4" else 0)
    src[s0:s0 + n] = cube.ravel()
    keep = src.copy()
    k = vs.gaussian_taps(case.radius)
    rc = emu.emu_voxel_opacity(C.c_size_t(case.npix), case.nt, _ptr(src, s0), k.ctypes.data_as(_P), case.radius,
                               C.c_float(case.contrast), C.c_float(thr), _ptr(dst, d0))
    assert rc == 0
    assert np.array_equal(src, keep, equal_nan=True)
    assert np.all(dst[:d0] == vs.SENTINEL) and np.all(dst[d0 + n:] == vs.SENTINEL), "written outside [0, npix * nt)"
    return dst[d0:d0 + n].reshape(case.npix, case.nt).copy()


# ---- launch arithmetic -------------------------------------------------------------------------------------------
def test_lds_fit():
    """the fitted block never asks for more than 160 KiB; blocks of 4 waves at every shape (the launcher before it
    fitted its block) do"""
    assert vs.lds_violations(vs.opacity_lds_bytes) == []
    before = vs.lds_violations(vs.opacity_lds_bytes_4_waves)
    assert (8192, 1025, 163968) in before and (4096, 3073, 163968) in before and (8192, 4096, 262144) in before
    assert not any(r <= 1012 for _, r, _ in before)
    assert vs.opacity_waves_per_block(8192, 1100) == 2 and vs.opacity_waves_per_block(4100, 4096) == 2
    assert vs.opacity_waves_per_block(8192, 1024) == 4 and vs.opacity_grid_traces(1024, 9) == 4 * 256 * 8


def test_tables_cover_the_paths():
    inst = sorted({c.instance for c in vs.OPACITY_SIZE_CASES})
    assert len(inst) == 24
    print("opacity instances:", inst)
    print("multi-trip:", [(c.id, c.instance, "prefetch" if vs.opacity_prefetch(c.nt) else "no prefetch")
                          for c in vs.OPACITY_MULTI_TRIP_CASES])


# ---- opacity ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", vs.OPACITY_SIZE_CASES, ids=lambda c: c.id)
def test_opacity_sizes(emu, case):
    cube, thr, ref = vs.opacity_case_input(case)
    vs.check_opacity(emu_opacity(emu, case, cube, thr), ref, case.id)


@pytest.mark.parametrize("case", vs.OPACITY_MULTI_TRIP_CASES + vs.OPACITY_LDS_CASES + vs.OPACITY_ISOLATION_CASES,
                         ids=lambda c: c.id)
def test_opacity_margins_of_the_device_only_cases(case):
    """the inputs of the cases that only the device runs keep away from the rules' edges as well"""
    vs.opacity_case_input(case)


@pytest.mark.parametrize("case", [c for c in vs.OPACITY_MULTI_TRIP_CASES if c.nt == 4097], ids=lambda c: c.id)
def test_opacity_multi_trip(emu, case):
    cube, thr, ref = vs.opacity_case_input(case)
    vs.check_opacity(emu_opacity(emu, case, cube, thr), ref, case.id)


@pytest.mark.parametrize("case", [c for c in vs.OPACITY_ISOLATION_CASES if c.nt == 4097], ids=lambda c: c.id)
def test_opacity_isolation(emu, case):
    """a trace of NaN, +Inf and 3e38 between two clean trips of the same wave changes no other trace"""
    cube, thr, ref = vs.opacity_case_input(case)
    grid = vs.opacity_grid_traces(case.nt, case.radius)
    bad = grid + 1
    assert bad - grid >= 0 and bad + grid < case.npix
    clean = emu_opacity(emu, case, cube, thr)
    vs.check_opacity(clean, ref, case.id)
    dirty_in = vs.poisoned(cube, bad)
    dirty = emu_opacity(emu, case, dirty_in, thr)
    others = np.arange(case.npix) != bad
    assert np.array_equal(dirty[others], clean[others])
    pref = vs.ob.voxel_opacity(dirty_in[bad:bad + 1], float(max(case.radius, 1)), case.radius, case.contrast, float(thr))
    vs.check_poisoned_trace(dirty[bad], pref[0], case.id)


@pytest.mark.parametrize("nt,radius,form", vs.EDGE_SHAPES)
@pytest.mark.parametrize("contrast", [1.0, 2.0])
def test_opacity_threshold_rule_at_its_edge(emu, nt, radius, form, contrast):
    """threshold == maximum keeps the line, one float more zeroes it; bit for bit against the oracle"""
    cube, mx = vs.edge_threshold_lines(nt, radius, contrast)
    case = vs.OpacityCase(nt, radius, contrast, npix=cube.shape[0], form=form)
    for thr, kept in ((mx, [True] * (cube.shape[0] - 1) + [False]),
                      (np.nextafter(mx, np.float32(np.inf)), [False] * (cube.shape[0] - 2) + [True, False])):
        out = emu_opacity(emu, case, cube, thr)
        ref = vs.ob.voxel_opacity(cube, float(max(radius, 1)), radius, contrast, float(thr))
        assert np.array_equal(ref.max(axis=1) == 1.0, kept)
        assert np.array_equal(out, ref), (thr, np.nonzero(out != ref))


@pytest.mark.parametrize("nt,radius,form", [(516, vs.FLAT_WINDOW_RADIUS, "aligned"), (513, vs.FLAT_WINDOW_RADIUS, "aligned"),
                                            (516, vs.FLAT_WIDE_RADIUS, "in+4"), (516, vs.FLAT_WIDE_RADIUS, "aligned")])
def test_opacity_flat_rule_at_its_edge(emu, nt, radius, form):
    """max - min one float below 1e-6f and at it: zero; one float above: kept; bit for bit against the oracle"""
    cube, kept = vs.edge_flat_lines(nt, radius)
    case = vs.OpacityCase(nt, radius, 1.0, npix=cube.shape[0], form=form)
    out = emu_opacity(emu, case, cube, np.float32(0.0))
    ref = vs.ob.voxel_opacity(cube, float(max(radius, 1)), radius, 1.0, 0.0)
    assert np.array_equal(ref.max(axis=1) == 1.0, kept)
    assert np.array_equal(out, ref)


# ---- select histogram ----------------------------------------------------------------------------------------------
def emu_hist(emu, v, level, prefix, hist=None):
    raw, first = aligned_f32(v.size, 0, np.float32(0))
    raw[first:first + v.size] = v
    hist = np.zeros(2048, np.uint64) if hist is None else hist
    emu.emu_select_hist(_ptr(raw, first), C.c_size_t(v.size), level, C.c_uint32(prefix), hist.ctypes.data_as(_P))
    return hist


@pytest.mark.parametrize("pattern,n", [(p, n) for p in vs.SELECT_PATTERNS for n in vs.SELECT_SIZES
                                       if n <= 257 or n == 4099 or (p == "rows" and n in (4095, 4096, 4097, 16387))])
def test_select_histogram(emu, pattern, n):
    v = vs.select_pattern(pattern, n)
    for level, prefix, what in vs.select_levels(v):
        ref = vs.select_hist_ref(v, level, prefix)
        assert (what == "absent") == (ref.sum() == 0)
        hist = emu_hist(emu, v, level, prefix)
        assert np.array_equal(hist, ref), (level, prefix, what, np.nonzero(hist != ref)[0][:8])
        if what != "absent" and n <= 257:
            assert np.array_equal(emu_hist(emu, v, level, prefix, hist), 2 * ref), "a second call accumulates"


@pytest.mark.parametrize("n", [257, 1285])
def test_kth_largest_structured(emu, n):
    """select_walk's steps (floor first, level 0 again when the walk ends in the lump) over the emulated histograms"""
    from thz_image_explorer_amd import shard

    for v, k, what in vs.kth_cases(n):
        levels = []

        def local_hist(level, prefix):
            levels.append((level, prefix))
            return emu_hist(emu, v, level, prefix)

        bins = shard.select_kth_largest(local_hist, k)
        assert pkg.host_select_value(*bins) == np.sort(v)[::-1][k - 1], what
        if what.startswith("lump"):
            assert levels[:2] == [(0, vs.SELECT_FLOOR_BIN), (0, 0)]


# ---- count, scan, emit ----------------------------------------------------------------------------------------------
def emu_instances(emu, op, gw, gh, gd, thr, cap, off=0, x0=0, total_shape=None, null_out=False):
    """-> (count, records array of cap + 3 with sentinel scale -7 where nothing was written)"""
    raw, first = aligned_f32(op.size, off)
    raw[first:first + op.size] = op.ravel()
    geom = vs.emu_geom(total_shape or (gw, gh, gd), thr)
    out = np.zeros(cap + 3, pkg.VOXEL_INSTANCE)
    out["scale"] = vs.SENTINEL
    total = C.c_ulonglong(0)
    emu.emu_voxel_instances(C.c_size_t(gw * gh), gd, C.c_size_t(gh), _ptr(raw, first), geom.ctypes.data_as(_P),
                            C.c_size_t(x0), None if null_out else out.ctypes.data_as(_P), C.c_ulonglong(cap),
                            C.byref(total))
    return total.value, out


def _instances_case(emu, case, thresholds, all_caps):
    op = vs.quantised_cube(case)
    worst = 0.0
    for what, thr in thresholds:
        ref = vs.instances_ref(op, thr)
        assert len(ref) == int((op >= np.float32(thr)).sum())
        assert (what != "all" or len(ref) == op.size) and (what != "none" or len(ref) == 0)
        caps = vs.instance_capacities(len(ref), case.gd) if all_caps(what) else [len(ref)]
        for cap in caps:
            count, out = emu_instances(emu, op, case.gw, case.gh, case.gd, thr, cap, case.off, null_out=cap == 0)
            assert count == len(ref), (what, cap)
            worst = max(worst, vs.check_instances(out[:cap], ref[:cap], f"{case.id} {what} cap {cap}"))
            assert np.all(out[cap:]["scale"] == vs.SENTINEL) and np.all(out[cap:]["color"] == 0)
    print(f"{case.id}: colours at most {worst:.3f} of the bar")


@pytest.mark.parametrize("case", vs.INSTANCE_DEPTH_CASES, ids=lambda c: c.id)
def test_instances_depths(emu, case):
    _instances_case(emu, case, vs.INSTANCE_THRESHOLDS, lambda what: what == "tie")


@pytest.mark.parametrize("case", [c for c in vs.INSTANCE_TILE_CASES if c.npix == 2049], ids=lambda c: c.id)
def test_instances_around_the_scan_tile(emu, case):
    _instances_case(emu, case, vs.INSTANCE_THRESHOLDS[1:2], lambda what: False)


@pytest.mark.parametrize("case,cut", vs.INSTANCE_SLAB_CASES, ids=lambda c: getattr(c, "id", str(c)))
def test_instances_slabs(emu, case, cut):
    """two x-slabs, the second one starting off a 16-byte boundary where the cube allows it, give the whole list"""
    op = vs.quantised_cube(case)
    ref = vs.instances_ref(op, 0.5)
    parts = []
    for x0, gw in ((0, cut), (cut, case.gw - cut)):
        slab = op[x0:x0 + gw]
        start = (case.off + 4 * x0 * case.gh * case.gd) % 16
        count, out = emu_instances(emu, slab, gw, case.gh, case.gd, 0.5, len(ref), start, x0=x0, total_shape=op.shape)
        parts.append(out[:count])
    if case.gd % 2:
        assert (4 * cut * case.gh * case.gd) % 16 != 0
    vs.check_instances(np.concatenate(parts), ref, case.id)
