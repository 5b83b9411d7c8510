"""Case tables, plain references and bars shared by test_emu_voxel_sizes.py (the kernels of csrc/voxel.hip on host
threads) and test_gpu_voxel_sizes.py (the same kernels through the C ABI): the voxel envelope (K15) at the trace
lengths, radii, pointer alignments and trace counts at which its launchers pick another kernel or another loop.

Bars (the project's existing ones, nothing new):
- opacities: max |out - oracle| < 1e-5 (OPACITY_BAR), the set of all-zero lines identical, every kept line with
  maximum exactly 1.0 and minimum exactly 0.0, nothing written outside [0, npix * nt);
- histograms, k-th largest, counts, positions, scales and alphas: bit for bit;
- colours: 1e-6 (COLOUR_BAR).

The opacity comparison holds only while no line sits on one of the two line rules by accident: check_margins proves,
on the reference alone, that every trace's envelope maximum is a relative 1e-3 away from the opacity threshold and
that its range is below 1e-7 or above 1e-5.  The rules' edges themselves are tested with lines that have one sample
(edge_threshold_lines, edge_flat_lines), where kernel and oracle perform the same single rounding."""
import functools

import numpy as np

import oracle_binding as ob

OPACITY_BAR = 1e-5
COLOUR_BAR = 1e-6
SENTINEL = np.float32(-7.0)

# ---- launch decisions of voxel.hip, restated ---------------------------------------------------------------------
VOX_PAD = 12                 # kVoxPad: the register window's radius
VOX_MAX_NT = 8192            # kVoxMaxNt
VOX_MAX_RADIUS = 4096        # thz_voxel_opacity's bound
LDS_LIMIT = 160 * 1024       # bytes of LDS a block may ask for (and a CU has)
NQ_STEPS = (1, 2, 4, 8, 16, 32)
SCAN_TILE = 2048             # kScanTile
COUNT_EMIT_GRID_TRACES = 256 * 16 * 4   # launch_voxel_count / launch_voxel_emit: blocks x waves


def opacity_nq(nt):
    return next(n for n in NQ_STEPS if (nt + 255) // 256 <= n)


def opacity_instance(nt, radius, aligned):
    """(NQ, VEC, WIDE) of the k_voxel_opacity instance launch_voxel_opacity picks; aligned: both pointers on 16 bytes"""
    return opacity_nq(nt), bool(nt % 4 == 0 and aligned), radius > VOX_PAD


def opacity_pad(radius):
    return (radius + 3) & ~3 if radius > VOX_PAD else VOX_PAD


def opacity_lds_bytes_4_waves(nt, radius):
    """dynamic LDS of a block of 4 waves: what the launcher asked for at every shape before it fitted its block"""
    return 4 * (opacity_nq(nt) * 256 + 2 * opacity_pad(radius)) * 4


def opacity_waves_per_block(nt, radius):
    """4, then 2, then 1 wave: the largest block whose LDS fits"""
    for wpb in (4, 2, 1):
        if wpb * (opacity_nq(nt) * 256 + 2 * opacity_pad(radius)) * 4 <= LDS_LIMIT:
            return wpb
    raise AssertionError(f"no block fits nt {nt} radius {radius}")


def opacity_lds_bytes(nt, radius):
    return opacity_waves_per_block(nt, radius) * (opacity_nq(nt) * 256 + 2 * opacity_pad(radius)) * 4


def opacity_grid_traces(nt, radius):
    """traces one pass of the persistent grid takes: waves per block x 256 x min(8, blocks whose LDS a CU holds)"""
    return opacity_waves_per_block(nt, radius) * 256 * min(8, LDS_LIMIT // opacity_lds_bytes(nt, radius))


def opacity_prefetch(nt):
    """the next trace is loaded before the taps (NQ <= 16) or after the stores (NQ 32)"""
    return opacity_nq(nt) <= 16


LDS_CHECK_RADII = (0, 12, 13, 1012, 1013, 1024, 1025, 3072, 3073, 4096)
LDS_CHECK_LENGTHS = tuple(sorted({1, VOX_MAX_NT} | {256 * n + d for n in NQ_STEPS for d in (0, 1)} - {VOX_MAX_NT + 1}))


def lds_violations(lds_bytes):
    """the (nt, radius, bytes) of every accepted shape, over the NQ edges and LDS_CHECK_RADII, for which the formula
    `lds_bytes` asks for more than a block may have"""
    return [(nt, r, lds_bytes(nt, r)) for nt in LDS_CHECK_LENGTHS for r in LDS_CHECK_RADII
            if lds_bytes(nt, r) > LDS_LIMIT]


assert lds_violations(opacity_lds_bytes) == []


def count_emit_vec(gd, aligned):
    """k_voxel_count<VEC> / k_voxel_emit<VEC>: 16-byte loads when the depth is a multiple of 4 and the cube aligned"""
    return bool(gd % 4 == 0 and aligned)


def scan_tiles(npix):
    return (npix + SCAN_TILE - 1) // SCAN_TILE


# ---- opacity: inputs and references ------------------------------------------------------------------------------
def gaussian_taps(radius):
    """the taps of every case here: sigma = max(radius, 1), so the outermost tap weighs exp(-1/2) of the centre one"""
    return ob.gaussian_kernel1d(float(max(radius, 1)), radius)


def powered(cube, contrast):
    """(v^2)^contrast in float32, the product forms for contrast 1 and 2"""
    q = cube * cube
    if contrast == 2.0:
        return q * q
    if contrast == 1.0:
        return q
    with np.errstate(divide="ignore"):
        return np.power(q, np.float32(contrast), dtype=np.float32)


def envelope_f64(cube, radius, contrast):
    """float64 convolution (zeros outside the trace) of the float32 powered samples, (npix, nt)"""
    p = powered(cube.reshape(-1, cube.shape[-1]), contrast).astype(np.float64)
    k = gaussian_taps(radius).astype(np.float64)
    nt = p.shape[1]
    acc = np.zeros_like(p)
    for j in range(2 * radius + 1):
        sh = j - radius
        lo, hi = max(0, -sh), min(nt, nt - sh)
        if lo < hi:
            acc[:, lo:hi] += p[:, lo + sh:hi + sh] * k[j]
    return acc


def pulse_cube(npix, nt, seed, spikes=False):
    """envelope_cube's pulses (test_voxel_cpu.py) with amplitudes 3 .. 6, as (npix, nt): every fourth trace from the
    second on is weak (x 0.25: its envelope lies below the threshold opacity_case_input picks), the third trace and
    the last one are flat zeros, so a wave of a multi-trip case meets every kind of line.

    spikes: one non-zero sample per trace instead.  A trace much shorter than the Gaussian has an almost flat
    envelope whatever its samples are (nt 3 under sigma 13: max - min is 1.2 % of the maximum at most), and the
    division by max - min multiplies every float32 rounding by maximum / (max - min): no float32 convolution holds
    1e-5 there, the oracle's own included.  With one sample each output is a single rounded product in the kernel
    and in the oracle alike, so the bar still tells a wrong or shifted tap from a right one."""
    rng = np.random.default_rng(seed)
    z = np.arange(nt, dtype=np.float32)[None, :]
    pos = rng.uniform(0.1 * nt, 0.9 * nt, (npix, 1)).astype(np.float32)
    amp = rng.uniform(3.0, 6.0, (npix, 1)).astype(np.float32)
    if spikes:
        cube = np.zeros((npix, nt), np.float32)
        cube[np.arange(npix), rng.integers(0, nt, npix)] = amp[:, 0] * rng.choice(np.float32([-1, 1]), npix)
    else:
        u = (z - pos) / np.float32(7.0)
        w = -u * np.exp(-u * u)
        cube = amp * w + 0.3 * amp * np.roll(w, 40, axis=-1)
        cube = (cube + 0.01 * rng.standard_normal((npix, nt))).astype(np.float32)
    cube[1::4] *= np.float32(0.25)
    cube[2::1031] = 0.0
    cube[-1] = 0.0
    return cube


def pick_threshold(env):
    """opacity threshold in the widest gap (in ratio) between the envelope maxima of the traces: from the input's
    float64 reference alone"""
    mx = np.unique(env.max(axis=1))
    mx = mx[mx > 0]
    if mx.size < 2:
        return np.float32(0.5 * mx[0]) if mx.size else np.float32(0.1)
    g = int(np.argmax(mx[1:] / mx[:-1]))
    return np.float32(np.sqrt(mx[g] * mx[g + 1]))


def check_margins(env, thr, what=""):
    """the stated condition of every opacity comparison: no line on a rule's edge by accident"""
    mx = env.max(axis=1)
    rng_ = mx - env.min(axis=1)
    rel = np.abs(mx - np.float64(thr)) / np.float64(thr) if thr > 0 else np.full(mx.shape, np.inf)
    assert (rel >= 1e-3).all(), f"{what}: trace {int(rel.argmin())} has its maximum {rel.min():.2e} from the threshold"
    bad = (rng_ >= 1e-7) & (rng_ <= 1e-5)
    assert not bad.any(), f"{what}: trace {int(np.nonzero(bad)[0][0])} has range {rng_[bad][0]:.3e}"
    return float(rel.min())


class OpacityCase:
    """nt, radius, contrast, npix and form ('aligned', 'in+4', 'out+4': that pointer 4 bytes off a 16-byte boundary)"""

    def __init__(self, nt, radius, contrast, npix=6, form="aligned", tag=""):
        self.nt, self.radius, self.contrast, self.npix, self.form, self.tag = nt, radius, contrast, npix, form, tag
        self.instance = opacity_instance(nt, radius, form == "aligned")
        self.trips = -(-npix // opacity_grid_traces(nt, radius))

    @property
    def id(self):
        return f"{self.tag}nt{self.nt}-r{self.radius}-c{self.contrast:g}-n{self.npix}-{self.form}"

    @property
    def seed(self):
        return self.nt * 131 + self.radius * 7 + self.npix


OPACITY_LENGTHS = (1, 3, 4, 255, 256, 257, 260, 512, 513, 516, 1024, 1025, 1028, 2048, 2049, 2052, 4096, 4097, 4100,
                   8191, 8192)
WINDOW_RADII = (0, 1, 11, 12)
WIDE_RADII = (13, 14, 15, 16, 17, 50)


def _size_cases():
    """every length, every form it has, once with a window radius and once with a wide one (the radii and the two
    product contrasts taken in turn)"""
    out = []
    for i, nt in enumerate(OPACITY_LENGTHS):
        forms = ("aligned", "in+4", "out+4") if nt % 4 == 0 else ("aligned",)
        for j, form in enumerate(forms):
            out.append(OpacityCase(nt, WINDOW_RADII[(i + j) % 4], (2.0, 1.0)[(i + j) % 2], form=form))
            out.append(OpacityCase(nt, WIDE_RADII[(i + j) % 6], (1.0, 2.0)[(i + j) % 2], form=form))
    out.append(OpacityCase(3, 13, 2.0, tag="radius>=nt-"))
    out.append(OpacityCase(260, 300, 1.0, tag="radius>=nt-"))
    # exp2/log2 form of the power: once per access form
    for nt, form in ((516, "aligned"), (516, "in+4"), (513, "aligned")):
        out.append(OpacityCase(nt, 9, 0.37, form=form, tag="exp2-"))
        out.append(OpacityCase(nt, 13, 0.7, form=form, tag="exp2-"))
    return out


OPACITY_SIZE_CASES = _size_cases()

# a few traces more than one pass of the grid: the wave loop's second trip
OPACITY_MULTI_TRIP_CASES = (
    OpacityCase(8, 1, 2.0, npix=8197, tag="trips-"),                       # NQ 1
    OpacityCase(2052, 12, 1.0, npix=2051, tag="trips-"),                   # NQ 16, prefetch
    OpacityCase(4097, 11, 2.0, npix=1027, tag="trips-"),                   # NQ 32, no prefetch, scalar
    OpacityCase(4100, 1, 1.0, npix=1027, tag="trips-"),                    # NQ 32, no prefetch, vector
    OpacityCase(4100, 13, 2.0, npix=1027, tag="trips-"),                   # NQ 32, wide
)
# blocks of fewer than 4 waves: 4 waves would ask for more LDS than a block may have (3 traces each)
OPACITY_LDS_CASES = (OpacityCase(8192, 1100, 2.0, npix=3, tag="lds-"), OpacityCase(4100, 4096, 1.0, npix=3, tag="lds-"))
# three trips of one wave: the poisoned trace is its second (radius 12 and 13: every tap is a real one, see
# test_*_isolation)
OPACITY_ISOLATION_CASES = (
    OpacityCase(8, 12, 2.0, npix=2 * 8192 + 3, tag="poison-"),
    OpacityCase(2052, 12, 2.0, npix=2 * 2048 + 3, tag="poison-"),          # prefetch
    OpacityCase(4097, 12, 1.0, npix=2 * 1024 + 3, tag="poison-"),          # no prefetch, window
    OpacityCase(4100, 13, 2.0, npix=2 * 1024 + 3, tag="poison-"),          # no prefetch, wide
)

# coverage the tables owe
assert {c.instance for c in OPACITY_SIZE_CASES} == {(q, v, w) for q in NQ_STEPS for v in (False, True)
                                                    for w in (False, True)}, "not all 24 k_voxel_opacity instances"
assert any(c.trips > 1 and opacity_prefetch(c.nt) for c in OPACITY_MULTI_TRIP_CASES)
assert any(c.trips > 1 and not opacity_prefetch(c.nt) for c in OPACITY_MULTI_TRIP_CASES)
assert all(c.trips == 2 for c in OPACITY_MULTI_TRIP_CASES) and all(c.trips == 3 for c in OPACITY_ISOLATION_CASES)
assert all(opacity_lds_bytes_4_waves(c.nt, c.radius) > LDS_LIMIT for c in OPACITY_LDS_CASES)
assert {c.radius for c in OPACITY_SIZE_CASES} >= set(WINDOW_RADII + WIDE_RADII)
assert {c.nt for c in OPACITY_SIZE_CASES} >= set(OPACITY_LENGTHS)


@functools.lru_cache(maxsize=2)
def opacity_case_input(case):
    """(cube (npix, nt), threshold, oracle's opacities) of a case, its margins proven; computed once and shared"""
    cube = pulse_cube(case.npix, case.nt, case.seed, spikes=case.nt < 16 and case.radius > case.nt)
    env = envelope_f64(cube, case.radius, case.contrast)
    thr = pick_threshold(env)
    check_margins(env, thr, case.id)
    ref = ob.voxel_opacity(cube, float(max(case.radius, 1)), case.radius, case.contrast, float(thr))
    for a in (cube, ref):
        a.setflags(write=False)
    return cube, thr, ref


def check_opacity(out, ref, what=""):
    """the bars of an opacity comparison over every trace; returns error / bar"""
    nt = ref.shape[-1]
    o, r = out.reshape(-1, nt), ref.reshape(-1, nt)
    assert np.isfinite(o).all(), f"{what}: non-finite or unwritten output"
    err = float(np.abs(o - r).max())
    live = r.max(axis=1) > 0
    assert np.array_equal((o != 0).any(axis=1), live), f"{what}: zero lines differ at {np.nonzero((o != 0).any(axis=1) != live)[0][:8]}"
    if live.any():
        assert np.all(o[live].max(axis=1) == 1.0) and np.all(o[live].min(axis=1) == 0.0), f"{what}: a kept line does not span [0, 1]"
    print(f"{what}: max err {err:.3e}, {err / OPACITY_BAR:.3f} of the bar, {int(live.sum())} of {live.size} lines kept")
    assert err < OPACITY_BAR, f"{what}: {err:.3e}"
    return err / OPACITY_BAR


POISON = (np.float32(np.nan), np.float32(np.inf), np.float32(3e38))


def poisoned(cube, trace):
    """a copy whose trace `trace` holds NaN, +Inf and 3e38 samples, three of each, away from each other"""
    nt = cube.shape[1]
    c = cube.copy()
    for i, v in enumerate(POISON * 3):
        c[trace, (nt * (2 * i + 1)) // 18] = v
    return c


def check_poisoned_trace(out, ref, what=""):
    """the poisoned trace against the oracle: equal NaN positions, the rest within the bar"""
    assert np.array_equal(np.isnan(out), np.isnan(ref)), \
        f"{what}: NaN at {int(np.isnan(out).sum())} samples, the oracle at {int(np.isnan(ref).sum())}"
    ok = ~np.isnan(ref)
    err = float(np.abs(out[ok] - ref[ok]).max()) if ok.any() else 0.0
    print(f"{what}: poisoned trace, {int((~ok).sum())} NaN, max err of the rest {err:.3e}")
    assert err < OPACITY_BAR


# ---- the line rules at their edges -------------------------------------------------------------------------------
EDGE_SHAPES = ((516, 9, "aligned"), (516, 9, "in+4"), (516, 13, "aligned"), (513, 13, "aligned"), (4100, 17, "out+4"))


def single_sample_max(a, radius, contrast):
    """envelope maximum of a line whose one non-zero sample is a: round(p * centre tap), every other addend is zero"""
    return (powered(np.float32(a), contrast) * gaussian_taps(radius)[radius]).astype(np.float32)


def edge_threshold_lines(nt, radius, contrast):
    """(cube, mx): lines with one sample of 1.5 at the ends, around a lane's quad and a 256-sample border, one line
    with a larger sample (1.5625), one with a smaller (1.4375); a^4 is exact in float32 for all three, so powf of the
    oracle and the kernel's products agree.  With the threshold at mx the 1.5 lines are kept, one float above they
    are zero."""
    assert nt > 2 * radius + 1
    spots = [0, 1, 3, 4, nt // 2, min(255, nt - 1), min(256, nt - 1), nt - 2, nt - 1]
    cube = np.zeros((len(spots) + 2, nt), np.float32)
    for t, s in enumerate(spots):
        cube[t, s] = 1.5
    cube[-2, nt // 3] = 1.5625
    cube[-1, nt // 3] = 1.4375
    return cube, single_sample_max(1.5, radius, contrast)


@functools.lru_cache(maxsize=None)
def flat_rule_amplitudes(radius):
    """amplitudes whose single-sample envelope maximum (contrast 1, so the power is the one product a * a) is the
    float below float32(1e-6), that float, and the float above it — None where a target falls between two amplitudes"""
    kc = gaussian_taps(radius)[radius]
    t0 = np.float32(1e-6)
    found = []
    for target in (np.nextafter(t0, np.float32(0)), t0, np.nextafter(t0, np.float32(1))):
        a0 = np.sqrt(np.float64(target) / np.float64(kc)).astype(np.float32)
        cand = (a0.view(np.uint32).astype(np.int64) + np.arange(-64, 65)).astype(np.uint32).view(np.float32)
        hit = cand[((cand * cand) * kc).astype(np.float32) == target]
        if hit.size == 0:
            return None
        found.append(hit[0])
    return tuple(found)


def flat_rule_radius(candidates):
    """the first radius of `candidates` at which all three targets of the flat rule have an amplitude"""
    for r in candidates:
        if flat_rule_amplitudes(r) is not None:
            return r
    raise AssertionError(f"no radius of {candidates} reaches the three floats around 1e-6")


FLAT_WINDOW_RADIUS = flat_rule_radius(range(1, VOX_PAD + 1))
FLAT_WIDE_RADIUS = flat_rule_radius(range(VOX_PAD + 1, 64))


def edge_flat_lines(nt, radius):
    """(cube, kept): threshold 0, contrast 1; per amplitude of flat_rule_amplitudes lines with the sample at several
    places.  max - min is the maximum itself (nt > 2 radius + 1, so some output is 0): zero at <= 1e-6f, kept above"""
    assert nt > 2 * radius + 1
    amps = flat_rule_amplitudes(radius)
    spots = (0, 5, nt // 2, nt - 1)
    cube = np.zeros((len(amps) * len(spots), nt), np.float32)
    kept = np.zeros(cube.shape[0], bool)
    for i, a in enumerate(amps):
        for j, s in enumerate(spots):
            cube[i * len(spots) + j, s] = a
            kept[i * len(spots) + j] = i == 2
    assert single_sample_max(amps[1], radius, 1.0) == np.float32(1e-6) < single_sample_max(amps[2], radius, 1.0)
    return cube, kept


# ---- select histogram ----------------------------------------------------------------------------------------------
SELECT_FLOOR_BIN = 0xBA800000 >> 21     # key of 2^-10: select_walk's first level-0 pass lumps everything below
SELECT_SIZES = (1, 2, 3, 4, 5, 255, 256, 257, 4095, 4096, 4097, 4099, 16381, 16384, 16387, 49153)
SELECT_PATTERNS = ("mix", "rows", "half_waves", "runs", "specials")


def float_keys(v):
    b = np.ascontiguousarray(v, np.float32).view(np.uint32)
    return np.where(b & 0x80000000, ~b, b | 0x80000000).astype(np.uint32)


def select_hist_ref(v, level, prefix):
    """numpy.bincount of the level's bins: level 0 over every key with the bins below `prefix` lumped into it,
    levels 1 and 2 over the keys whose higher bits equal `prefix`"""
    keys = float_keys(v)
    if level == 0:
        bins = np.maximum(keys >> 21, np.uint32(prefix))
    elif level == 1:
        bins = (keys[(keys >> 21) == prefix] >> 10) & 2047
    else:
        bins = keys[(keys >> 10) == prefix] & 1023
    return np.bincount(bins.astype(np.int64), minlength=2048).astype(np.uint64)


def _ramp(n):
    """n values inside one level-0 bin ([0.5, 0.625): sign, exponent and two mantissa bits), over many level-1 bins"""
    return (np.float32(0.5) + np.float32(0.125) * (np.arange(n) % 1000).astype(np.float32) / np.float32(1000)).astype(np.float32)


def select_pattern(name, n):
    """n values of a pattern.  A wave of k_select_hist holds 256 consecutive values, four to a lane."""
    rng = np.random.default_rng(n * 31 + len(name))
    if name in ("mix", "specials"):
        v = rng.random(n).astype(np.float32)
        v[rng.random(n) < 0.35] = 0.0
        v[rng.random(n) < 0.15] = np.float32(0.75)
        if name == "specials":
            sp = np.array([np.nan, np.inf, -np.inf, -0.0, 1e-40, -1e-42, -1.5, -3e38, 1.17549435e-38, 2.0 ** -10],
                          np.float32)
            where = rng.random(n) < 0.2
            v[where] = sp[rng.integers(0, sp.size, int(where.sum()))]
        return v
    if name == "rows":      # rows of 256 m identical (or same-bin) values: every lane's four values share a bin
        v = np.empty(n + 3 * 256 * 3, np.float32)
        at, i = 0, 0
        while at < n:
            m = 256 * (1 + i % 3)
            v[at:at + m] = (0.0, 1.0, 0.0)[i % 3] if i % 4 != 3 else _ramp(m)
            at, i = at + m, i + 1
        return v[:n].copy()
    if name == "half_waves":  # lanes 0 .. 31 hold uniform quads (one value per lane), lanes 32 .. 63 do not
        m = -(-n // 256)
        v = rng.random((m, 64, 4)).astype(np.float32)
        v[:, :32, :] = np.round(v[:, :32, :1] * 8) / np.float32(8)
        v[1::2, :32, :] = 0.0
        return v.reshape(-1)[:n].copy()
    if name == "runs":      # equal values in runs that begin at lane 0, end at lane 63 and cross a wave's border
        vals = (0.0, 1.0, 0.75, 0.0, 0.3, 1.0)
        lens = (256, 252, 8, 260, 4, 120, 136, 512, 3, 5, 248, 1, 7, 1024, 12)
        v = np.empty(n + 1024, np.float32)
        at, i = 0, 0
        while at < n:
            v[at:at + lens[i % len(lens)]] = vals[i % len(vals)]
            at, i = at + lens[i % len(lens)], i + 1
        return v[:n].copy()
    raise KeyError(name)


def select_levels(v):
    """the (level, prefix, what) list of a histogram check: level 0 in full and with the walk's floor, levels 1 and 2
    with the prefixes of the true walk to the (n // 3 + 1)-th largest key and with a prefix no key has"""
    keys = np.sort(float_keys(v))[::-1]
    key = int(keys[min(v.size // 3, v.size - 1)])
    out = [(0, 0, "full"), (0, SELECT_FLOOR_BIN, "floor"), (1, key >> 21, "walk"), (2, key >> 10, "walk")]
    absent1 = next(b for b in range(2047, -1, -1) if not np.any((keys >> 21) == b))
    absent2 = next(p for p in range((key >> 10) + 1, (key >> 10) + 4096) if not np.any((keys >> 10) == p))
    return out + [(1, absent1, "absent"), (2, absent2, "absent")]


def small_positive_cube(n):
    """mostly zeros, a few ones, the rest positive below 2^-10: the k-th largest inside the small values lies in
    select_walk's lump, so level 0 runs twice"""
    rng = np.random.default_rng(n)
    v = np.zeros(n, np.float32)
    small = rng.random(n) < 0.4
    v[small] = (rng.random(int(small.sum())) * 2.0 ** -11 + 2.0 ** -20).astype(np.float32)
    v[rng.random(n) < 0.01] = 1.0
    k = int((v == 1.0).sum()) + max(1, int(small.sum()) // 2)
    assert 0 < np.sort(v)[::-1][k - 1] < 2.0 ** -10
    return v, k


def kth_cases(n):
    """[(values, k, what)]: ranks on both sides of each tie block of the structured patterns, inside the zeros, and
    in the lump"""
    out = []
    for name in ("rows", "runs", "half_waves"):
        v = select_pattern(name, n)
        ones, zeros = int((v == 1.0).sum()), int((v == 0.0).sum())
        ks = {1, n, ones, ones + 1, n - zeros, n - zeros + 1, n - zeros // 2}
        out += [(v, k, f"{name} k={k}") for k in sorted(ks) if 1 <= k <= n]
    v, k = small_positive_cube(n)
    return out + [(v, k, f"lump k={k}")]


# ---- count, scan, emit ----------------------------------------------------------------------------------------------
INSTANCE_DEPTHS = (1, 3, 4, 255, 256, 257, 260, 1001, 1028)
TIME_SPAN = 51.15


class InstanceCase:
    """a (gw, gh, gd) opacity cube, `off` bytes behind a 16-byte boundary"""

    def __init__(self, gw, gh, gd, off=0, tag=""):
        self.gw, self.gh, self.gd, self.off, self.tag = gw, gh, gd, off, tag
        self.npix = gw * gh
        self.vec = count_emit_vec(gd, off == 0)
        self.trips = -(-gd // 256)

    @property
    def id(self):
        return f"{self.tag}{self.gw}x{self.gh}x{self.gd}+{self.off}"


INSTANCE_DEPTH_CASES = [InstanceCase(3, 5, gd, off) for gd in INSTANCE_DEPTHS for off in ((0, 4) if gd % 4 == 0 else (0,))]
# trace counts around the scan's tile of 2048 (depth 3: scalar, depth 4: vector)
INSTANCE_TILE_CASES = [InstanceCase(1, 2047, 3, tag="tile-"), InstanceCase(1, 2048, 4, tag="tile-"),
                       InstanceCase(3, 683, 4, tag="tile-"), InstanceCase(17, 241, 3, tag="tile-")]
assert [c.npix for c in INSTANCE_TILE_CASES] == [2047, 2048, 2049, 4097]
# more than 256 tiles (the carry of k_scan_tile_offsets) and more than one grid pass of count and emit
INSTANCE_CARRY_CASE = InstanceCase(2048 * 256 + 2049, 1, 2, tag="carry-")
assert scan_tiles(INSTANCE_CARRY_CASE.npix) > 256 and INSTANCE_CARRY_CASE.npix > COUNT_EMIT_GRID_TRACES
# both forms of count and emit with more than one 256-sample trip
assert {c.vec for c in INSTANCE_DEPTH_CASES if c.trips > 1} == {False, True}
assert {c.vec for c in INSTANCE_DEPTH_CASES} == {False, True}


def quantised_cube(case, empty_share=0.5):
    """opacities that are multiples of 1/8 (thresholds tie with many voxels), with runs of all-zero traces, the first
    and the last trace among them"""
    rng = np.random.default_rng(case.npix * 7 + case.gd)
    op = (rng.integers(0, 9, (case.npix, case.gd)) / 8.0).astype(np.float32)
    op[rng.random((case.npix, case.gd)) < 0.3] = 0.0
    run = max(1, case.npix // 16)
    dead = np.repeat(rng.random(case.npix // run + 1) < empty_share, run)[:case.npix]
    dead[0] = dead[-1] = True
    if case.npix > 2:
        dead[case.npix // 2] = False
    op[dead] = 0.0
    return op.reshape(case.gw, case.gh, case.gd)


INSTANCE_THRESHOLDS = (("all", 0.0), ("tie", 0.5), ("one", 1.0), ("none", 1.125))


def instance_capacities(count, gd):
    """NULL buffer; a cut inside a lane's four samples; a cut inside a 256-sample trip; exactly the count"""
    return sorted({0, min(2, count), min(131 if gd < 512 else 256 + 131, count), count})


def instances_ref(op, thr):
    """the oracle's instance list of a (gw, gh, gd) cube at scaling 1"""
    return ob.voxel_instances(op, thr, TIME_SPAN, 1, op.shape)[0]


# x-slab tiles (the multi-GPU layout): (case, first row of the second slab).  The vector form needs a depth that is a
# multiple of 4, and then every slab starts on 16 bytes when the cube does; a slab that starts off 16 bytes is
# therefore one of a scalar cube (odd gh * gd) or of a cube that is itself 4 bytes off.
INSTANCE_SLAB_CASES = ((InstanceCase(5, 3, 257, tag="slab-"), 1), (InstanceCase(5, 3, 260, 4, tag="slab-"), 2),
                       (InstanceCase(4, 3, 260, tag="slab-"), 3))


def emu_geom(shape, thr):
    """the eight floats of VoxelGeom for a whole cube `shape` at scaling 1 (voxel_layout of the engine, restated in
    float32)"""
    gw, gh, gd = shape
    dims = ob.voxel_instances(np.zeros((1, 1, 1), np.float32), 2.0, TIME_SPAN, 1, (1, 1, 1))[1]
    depth = np.float32(dims[2])
    full_d = np.float32(np.float32(gd) * depth)
    return np.array([gw * 0.25 / gw, gh * 0.25 / gh, full_d / np.float32(gd), gw * 0.25 / 2, gh * 0.25 / 2,
                     full_d / np.float32(2), 1.0, thr], np.float32)


def check_instances(got, ref, what=""):
    """records against the oracle's: positions, scale and alpha bit for bit, colours within the bar (NaN where the
    oracle has NaN: threshold 1.0 divides 0 by 0); returns colour error / bar"""
    assert len(got) == len(ref)
    if len(ref) == 0:
        return 0.0
    assert np.array_equal(got["position"], ref["position"]), f"{what}: positions"
    assert np.array_equal(got["scale"], ref["scale"]), f"{what}: scale"
    assert np.array_equal(got["color"][:, 3], ref["color"][:, 3]), f"{what}: alpha"
    g, r = got["color"][:, :3], ref["color"][:, :3]
    assert np.array_equal(np.isnan(g), np.isnan(r)), f"{what}: NaN colours"
    ok = ~np.isnan(r)
    err = float(np.abs(g[ok] - r[ok]).max()) if ok.any() else 0.0
    assert err < COLOUR_BAR, f"{what}: colours {err:.3e}"
    return err / COLOUR_BAR
