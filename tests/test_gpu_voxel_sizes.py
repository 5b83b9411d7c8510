"""The voxel envelope (csrc/voxel.hip, K15) on the device, through the C ABI, at the sizes, radii, alignments and trace
counts that switch its kernels' paths: the tables, references and bars of voxel_sizes.py — the comparisons of
test_emu_voxel_sizes.py plus what only the chip shows: more traces than one pass of the persistent grid (the wave
loop's second and third trip, with and without prefetch), blocks fitted to the LDS limit, the scan's carry over more
than 256 tiles, 16-byte forms against pointers 4 bytes off.

Which test runs which branch:
- k_voxel_opacity<NQ, VEC, WIDE>, all 24 instances: test_opacity_sizes; the exp2/log2 power in its `exp2-` cases
- the wave loop's later trips: test_opacity_multi_trip (NQ 1, 16 with prefetch, 32 without: scalar, vector, wide),
  test_opacity_isolation
- blocks of 2 waves: test_opacity_lds_fit
- the two line rules on their edges: test_opacity_threshold_rule_at_its_edge, test_opacity_flat_rule_at_its_edge
- k_select_hist's weight-4 round, partly filled waves, floor lump, tail: test_select_histogram;
  select_walk's repeat of level 0: test_kth_largest_structured
- k_voxel_count / k_voxel_emit <true | false> with one and several 256-sample trips: test_instances_depths;
  k_scan_* around one tile and over more than 256: test_instances_around_the_scan_tile, test_instances_scan_carry"""
import numpy as np
import pytest

import thz_image_explorer_amd as pkg
import voxel_sizes as vs

pytestmark = pytest.mark.gpu

GUARD = 8   # floats in front of and behind every payload (allocations start 256-byte aligned)


def gpu_opacity(eng, case, cube, thr, bufs=None):
    """thz_voxel_opacity on a case's cube -> output (npix, nt); the input, the guards and the sentinels checked"""
    n = cube.size
    s0 = GUARD + (1 if case.form == "in+4" else 0)
    d0 = GUARD + (1 if case.form == "out+4" else 0)
    src = np.full(n + 3 * GUARD, vs.SENTINEL, np.float32)
    src[s0:s0 + n] = cube.ravel()
    blank = np.full(n + 3 * GUARD, vs.SENTINEL, np.float32)
    own = bufs is None
    d_in, d_out = (eng.alloc(src.nbytes), eng.alloc(src.nbytes)) if own else bufs
    assert d_in.ptr % 16 == 0 and d_out.ptr % 16 == 0
    d_in.upload(src)
    d_out.upload(blank)
    cfg = pkg.voxel_cfg_default()
    cfg.radius, cfg.contrast, cfg.sigma, cfg.opacity_threshold = case.radius, case.contrast, float(max(case.radius, 1)), float(thr)
    try:
        eng.voxel_opacity(case.npix, case.nt, d_in.ptr + 4 * s0, cfg, d_out.ptr + 4 * d0)
        dst = d_out.download(src.shape, np.float32)
        assert np.array_equal(d_in.download(src.shape, np.float32), src, equal_nan=True)
    finally:
        if own:
            d_in.free(); d_out.free()
    assert np.all(dst[:d0] == vs.SENTINEL) and np.all(dst[d0 + n:] == vs.SENTINEL), "written outside [0, npix * nt)"
    return dst[d0:d0 + n].reshape(case.npix, case.nt)


def _oracle(cube, case, thr):
    return vs.ob.voxel_opacity(cube, float(max(case.radius, 1)), case.radius, case.contrast, float(thr))


# ---- opacity ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", vs.OPACITY_SIZE_CASES, ids=lambda c: c.id)
def test_opacity_sizes(engine, case):
    cube, thr, ref = vs.opacity_case_input(case)      # the margins are asserted in there, on the reference alone
    vs.check_opacity(gpu_opacity(engine, case, cube, thr), ref, f"{case.id} {case.instance}")


@pytest.mark.parametrize("case", vs.OPACITY_MULTI_TRIP_CASES, ids=lambda c: c.id)
def test_opacity_multi_trip(engine, case):
    """a few traces more than one pass of the grid, every trace against the oracle"""
    assert case.trips == 2
    cube, thr, ref = vs.opacity_case_input(case)
    vs.check_opacity(gpu_opacity(engine, case, cube, thr), ref, f"{case.id} {case.instance}")


@pytest.mark.parametrize("case", vs.OPACITY_LDS_CASES, ids=lambda c: c.id)
def test_opacity_lds_fit(engine, case):
    """radii whose slices fit a block only two waves at a time"""
    assert vs.opacity_waves_per_block(case.nt, case.radius) == 2 and vs.opacity_lds_bytes(case.nt, case.radius) <= vs.LDS_LIMIT
    cube, thr, ref = vs.opacity_case_input(case)
    vs.check_opacity(gpu_opacity(engine, case, cube, thr), ref, case.id)


@pytest.mark.parametrize("case", vs.OPACITY_ISOLATION_CASES, ids=lambda c: c.id)
def test_opacity_isolation(engine, case):
    """a trace of NaN, +Inf and 3e38 that a wave takes between two clean ones changes no other trace's output by a
    bit (the registers and the LDS slice it leaves behind); the trace itself agrees with the oracle.  Radii 12 and
    13: below 12 the register window multiplies the samples beyond the radius by zero taps, which an infinite sample
    turns into NaN up to 12 samples away where the reference skips them."""
    cube, thr, ref = vs.opacity_case_input(case)
    grid = vs.opacity_grid_traces(case.nt, case.radius)
    bad = grid + 1
    assert bad + grid < case.npix
    nbytes = 4 * (cube.size + 3 * GUARD)
    bufs = (engine.alloc(nbytes), engine.alloc(nbytes))
    try:
        clean = gpu_opacity(engine, case, cube, thr, bufs)
        vs.check_opacity(clean, ref, case.id)
        dirty_in = vs.poisoned(cube, bad)
        dirty = gpu_opacity(engine, case, dirty_in, thr, bufs)
    finally:
        for b in bufs:
            b.free()
    others = np.arange(case.npix) != bad
    assert np.array_equal(dirty[others], clean[others])
    vs.check_poisoned_trace(dirty[bad], _oracle(dirty_in[bad:bad + 1], case, thr)[0], case.id)


@pytest.mark.parametrize("nt,radius,form", vs.EDGE_SHAPES)
@pytest.mark.parametrize("contrast", [1.0, 2.0])
def test_opacity_threshold_rule_at_its_edge(engine, nt, radius, form, contrast):
    """threshold == maximum keeps the line, one float more zeroes it; bit for bit against the oracle"""
    cube, mx = vs.edge_threshold_lines(nt, radius, contrast)
    case = vs.OpacityCase(nt, radius, contrast, npix=cube.shape[0], form=form)
    for thr, kept in ((mx, [True] * (cube.shape[0] - 1) + [False]),
                      (np.nextafter(mx, np.float32(np.inf)), [False] * (cube.shape[0] - 2) + [True, False])):
        out = gpu_opacity(engine, case, cube, thr)
        ref = _oracle(cube, case, thr)
        assert np.array_equal(ref.max(axis=1) == 1.0, kept)
        assert np.array_equal(out, ref), (thr, np.nonzero(out != ref))


@pytest.mark.parametrize("nt,radius,form", [(516, vs.FLAT_WINDOW_RADIUS, "aligned"), (513, vs.FLAT_WINDOW_RADIUS, "aligned"),
                                            (516, vs.FLAT_WIDE_RADIUS, "in+4"), (516, vs.FLAT_WIDE_RADIUS, "aligned")])
def test_opacity_flat_rule_at_its_edge(engine, nt, radius, form):
    """max - min one float below 1e-6f and at it: zero; one float above: kept; bit for bit against the oracle"""
    cube, kept = vs.edge_flat_lines(nt, radius)
    case = vs.OpacityCase(nt, radius, 1.0, npix=cube.shape[0], form=form)
    out = gpu_opacity(engine, case, cube, np.float32(0.0))
    ref = _oracle(cube, case, 0.0)
    assert np.array_equal(ref.max(axis=1) == 1.0, kept)
    assert np.array_equal(out, ref)


# ---- select histogram ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", vs.SELECT_SIZES)
@pytest.mark.parametrize("pattern", vs.SELECT_PATTERNS)
def test_select_histogram(engine, pattern, n):
    v = vs.select_pattern(pattern, n)
    d = engine.to_device(v)
    d_hist = engine.alloc(2048 * 8)
    assert d.ptr % 16 == 0
    try:
        for level, prefix, what in vs.select_levels(v):
            ref = vs.select_hist_ref(v, level, prefix)
            assert (what == "absent") == (ref.sum() == 0)
            d_hist.zero()
            engine.select_histogram(d, n, level, prefix, d_hist)
            hist = d_hist.download((2048,), np.uint64)
            assert np.array_equal(hist, ref), (level, prefix, what, np.nonzero(hist != ref)[0][:8])
            engine.select_histogram(d, n, level, prefix, d_hist)      # the histogram accumulates
            assert np.array_equal(d_hist.download((2048,), np.uint64), 2 * ref), (level, prefix, what)
    finally:
        d.free(); d_hist.free()


@pytest.mark.parametrize("n", [257, 4099, 16387, 49153])
def test_kth_largest_structured(engine, n):
    for v, k, what in vs.kth_cases(n):
        want = np.sort(v)[::-1][k - 1]
        d = engine.to_device(v)
        try:
            assert engine.kth_largest(d, n, k) == want, what
            assert engine.voxel_threshold(d, n, max_instances=k) == (want if k < n else 0.0), what
        finally:
            d.free()


# ---- count, scan, emit ----------------------------------------------------------------------------------------------
def gpu_instances(eng, d_op, gw, gh, gd, thr, cap, x0=0, gw_total=None):
    """-> (count, cap + 3 records; scale -7 and zeros where nothing was written); capacity 0 passes a NULL buffer"""
    blank = np.zeros(cap + 3, pkg.VOXEL_INSTANCE)
    blank["scale"] = vs.SENTINEL
    d_inst = eng.to_device(blank)
    total = gw if gw_total is None else gw_total
    try:
        count, _ = eng.voxel_instances(d_op, gw, gh, gd, thr, vs.TIME_SPAN, 1, (total, gh, gd), d_inst if cap else None,
                                       cap, x0=x0, gw_total=total)
        out = d_inst.download(blank.shape, pkg.VOXEL_INSTANCE)
    finally:
        d_inst.free()
    return count, out


def _instances_case(eng, case, thresholds, all_caps):
    op = vs.quantised_cube(case)
    raw = np.full(op.size + 3 * GUARD, vs.SENTINEL, np.float32)
    first = GUARD + case.off // 4
    raw[first:first + op.size] = op.ravel()
    d_raw = eng.to_device(raw)
    worst = 0.0
    try:
        for what, thr in thresholds:
            ref = vs.instances_ref(op, thr)
            assert len(ref) == int((op >= np.float32(thr)).sum())
            assert (what != "all" or len(ref) == op.size) and (what != "none" or len(ref) == 0)
            for cap in (vs.instance_capacities(len(ref), case.gd) if all_caps(what) else [len(ref)]):
                count, out = gpu_instances(eng, d_raw.ptr + 4 * first, case.gw, case.gh, case.gd, thr, cap)
                assert count == len(ref), (what, cap)
                worst = max(worst, vs.check_instances(out[:cap], ref[:cap], f"{case.id} {what} cap {cap}"))
                assert np.all(out[cap:]["scale"] == vs.SENTINEL) and np.all(out[cap:]["color"] == 0), \
                    f"{case.id} {what}: written past min(count, capacity) = {cap}"
    finally:
        d_raw.free()
    print(f"{case.id} ({'vector' if case.vec else 'scalar'}, {case.trips} trips): colours at most {worst:.3f} of the bar")


@pytest.mark.parametrize("case", vs.INSTANCE_DEPTH_CASES, ids=lambda c: c.id)
def test_instances_depths(engine, case):
    _instances_case(engine, case, vs.INSTANCE_THRESHOLDS, lambda what: True)


@pytest.mark.parametrize("case", vs.INSTANCE_TILE_CASES, ids=lambda c: c.id)
def test_instances_around_the_scan_tile(engine, case):
    _instances_case(engine, case, vs.INSTANCE_THRESHOLDS, lambda what: what == "tie")


def test_instances_scan_carry(engine):
    """more than 256 scan tiles (k_scan_tile_offsets carries from one round of 256 to the next) and more traces than
    one grid pass of k_voxel_count and k_voxel_emit"""
    _instances_case(engine, vs.INSTANCE_CARRY_CASE, vs.INSTANCE_THRESHOLDS[:2], lambda what: what == "tie")


@pytest.mark.parametrize("case,cut", vs.INSTANCE_SLAB_CASES, ids=lambda c: getattr(c, "id", str(c)))
def test_instances_slabs(engine, case, cut):
    """two x-slabs, the second one starting off a 16-byte boundary where the cube allows it, give the whole list"""
    op = vs.quantised_cube(case)
    ref = vs.instances_ref(op, 0.5)
    raw = np.full(op.size + 3 * GUARD, vs.SENTINEL, np.float32)
    first = GUARD + case.off // 4
    raw[first:first + op.size] = op.ravel()
    d_raw = engine.to_device(raw)
    parts = []
    try:
        for x0, gw in ((0, cut), (cut, case.gw - cut)):
            ptr = d_raw.ptr + 4 * (first + x0 * case.gh * case.gd)
            count, out = gpu_instances(engine, ptr, gw, case.gh, case.gd, 0.5, len(ref), x0=x0, gw_total=case.gw)
            parts.append(out[:count])
    finally:
        d_raw.free()
    if case.gd % 2:
        assert (4 * cut * case.gh * case.gd) % 16 != 0
    vs.check_instances(np.concatenate(parts), ref, case.id)
