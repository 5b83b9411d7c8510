"""The bandwidth-shaped helper kernels of csrc/kernels.hip on the host-thread emulation, at every size where a launcher
picks another kernel form or a loop changes its body: window multiply, bias / intensity, pixel sums and means,
pixel-list sums, block means and their slab-edge partials, the tilt re-laying and its column sums, the vector quotient.

Every case runs the product's own launcher (tests/emu/emu_harness.cpp) and is compared with a plain numpy restatement
(helper_sizes.py): bit for bit where the order of the operations is fixed, within the project's 2e-6 x sum |a| for the
order-free sums and 1e-5 for intensities.  The emulation sees index arithmetic, path choice and unwritten outputs; what
only the chip shows (contraction, alignment faults, more work than one grid pass) is test_gpu_helper_sizes.py's part.

Which test runs which branch:
- k_colsum_partial<1|2|3|5|8>, one and two levels, ragged tail, the ordered walk below 64 rows and above 8195 floats,
  with and without a list: test_pixel_sum (ids rows-length-list);  the tail's row stride over more than 64 rows of a
  block: test_colsum_partial_many_rows_per_block
- k_sum_axis0's unrolled body, carry and divide: test_sum_axis0;  k_sum_rows_f64: test_sum_rows_f64
- k_scale3d: test_scale3d;  k_scale_rows_partial: test_scale_rows_partial, test_scale_rows_partial_continues_scale3d
- k_gather_sum_w: test_gather_sum_w;  k_div_vec: test_div_vec
- k_tilt, k_tilt_sum<5|8>: test_tilt_and_tilt_sum;  the refusal above 2048 samples: test_tilt_sum_refuses_long_axes
- k_td_window_regs<1|2|4|8|16>, k_td_window<true|false>: test_td_window;  k_intensity<true|false>: test_intensity"""
import ctypes as C
import itertools

import numpy as np
import pytest

import helper_sizes as hs
import oracle_binding as ob
from test_emu_kernels import _p, emu  # noqa: F401  (the fixture builds the emulation when it is stale)

_SZ = C.c_size_t


def _buf(shape, misalign=0, fill=None, dtype=np.float32):
    """an array whose first element sits `misalign` bytes behind a 16-byte boundary (0: aligned — the launchers pick
    their 16-byte forms by the pointers' alignment, which numpy's allocator leaves open)"""
    n = int(np.prod(shape))
    raw = np.empty(n + 8, dtype)
    off = ((-raw.ctypes.data) % 16 + misalign) % 16 // raw.itemsize
    a = raw[off:off + n].reshape(shape)
    assert a.ctypes.data % 16 == misalign
    if fill is not None:
        a[...] = fill
    return a


def _put(a, misalign=0):
    b = _buf(a.shape, misalign, dtype=a.dtype)
    b[...] = a
    return b


# ---- pixel sums --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_list", [False, True], ids=["all", "list"])
@pytest.mark.parametrize("nrows,L", hs.pixel_sum_cases())
def test_pixel_sum(emu, nrows, L, with_list):
    rng = np.random.default_rng(1000 * nrows + L)
    a, lst, rows = hs.pixel_sum_input(rng, nrows, L, with_list)
    out = np.full(L, np.nan, np.float32)
    assert emu.emu_pixel_sum_list(_SZ(nrows), _SZ(L), _p(a), _p(lst), _p(out)) == 0
    hs.check_parallel_sum(out, rows, f"{nrows} x {L} (KC {hs.colsum_kc(L)})")
    if nrows < 64 or hs.colsum_kc(L) == 0:   # the ordered walk: sequential float32, bit for bit
        assert np.array_equal(out, hs.seq_sum_f32(rows))


@pytest.mark.parametrize("with_list", [False, True], ids=["all", "list"])
@pytest.mark.parametrize("nrows,L,max_groups", hs.COLSUM_LEVEL_CASES)
def test_colsum_partial_many_rows_per_block(emu, nrows, L, max_groups, with_list):
    """one level with few row groups: a block adds more than 64 rows, so the lanes that split the ragged tail's rows
    walk on by 64 row groups a second and a third time (on the device: more than 64 x 2048 rows, the GPU file's
    test_pixel_sum_tail_lanes_second_trip).  Every partial row that is promised is written, and each is within the bar
    of the float64 sum of its block's rows"""
    rng = np.random.default_rng(nrows * 7 + L)
    a, lst, rows = hs.pixel_sum_input(rng, nrows, L, with_list)
    part = np.full((max_groups, L), np.nan, np.float32)
    emu.emu_colsum_partial.restype = _SZ
    groups = emu.emu_colsum_partial(_SZ(nrows), _SZ(L), _p(a), _p(lst), _SZ(max_groups), _p(part))
    assert groups == max_groups and nrows > 64 * groups + groups
    assert np.isfinite(part).all()
    for g in range(groups):   # block g adds the rows g, g + groups, ...: row by row, a row in the wrong block shows
        hs.check_parallel_sum(part[g], rows[g::groups], f"{nrows} x {L}, row group {g} of {groups}")


def test_pixel_sum_lengths_cover_every_kernel_form(emu):
    """the length list reaches each KC on both sides of its switch, and the refusal; helper_sizes.colsum_kc is the
    launcher's own choice at every length, and that choice holds the row (KC x 256 chunks of 4 floats and the tail)"""
    for L in range(1, 8300):
        kc = emu.emu_colsum_kc(_SZ(L))
        assert kc == hs.colsum_kc(L), L
        assert kc in (1, 2, 3, 5, 8) and kc * 1024 + 3 >= L or kc == 0 and L > 8195, L
    kcs = [hs.colsum_kc(L) for L in hs.PIXEL_SUM_LENGTHS]
    assert set(kcs) == {0, 1, 2, 3, 5, 8}
    switches = {(hs.colsum_kc(L), hs.colsum_kc(L + 1)) for L in range(1, 8300) if hs.colsum_kc(L) != hs.colsum_kc(L + 1)}
    assert switches == {(1, 2), (2, 3), (3, 5), (5, 8), (8, 0)}
    for lo, hi in ((1027, 2048), (2050, 3002), (3072, 3076), (5120, 5124), (8195, 8196)):
        assert lo in hs.PIXEL_SUM_LENGTHS and hi in hs.PIXEL_SUM_LENGTHS and hs.colsum_kc(lo) != hs.colsum_kc(hi)


# ---- ordered sums ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("div", [False, True], ids=["sum", "mean"])
@pytest.mark.parametrize("carry", [False, True], ids=["fresh", "carry"])
@pytest.mark.parametrize("inner", hs.SUM_AXIS0_INNER)
@pytest.mark.parametrize("n0", hs.SUM_AXIS0_N0)
def test_sum_axis0(emu, n0, inner, carry, div):
    rng = np.random.default_rng(n0 * 100003 + inner)
    a = rng.standard_normal((n0, inner)).astype(np.float32)
    c = rng.standard_normal(inner).astype(np.float32) if carry else None
    d = float(n0 + 3) if div else 0.0
    ref = hs.seq_sum_f32(a, c, d)
    out = np.full(inner, np.nan, np.float32)
    assert emu.emu_sum_axis0(_p(a), _SZ(n0), _SZ(inner), C.c_float(d), _p(c), _p(out)) == 0
    assert np.array_equal(out, ref)
    if carry:   # the carry may be the output itself (a group's slab continues the sum in place)
        io = c.copy()
        assert emu.emu_sum_axis0(_p(a), _SZ(n0), _SZ(inner), C.c_float(d), _p(io), _p(io)) == 0
        assert np.array_equal(io, ref)


@pytest.mark.parametrize("inner", hs.SUM_AXIS0_INNER)
@pytest.mark.parametrize("n0", hs.SUM_AXIS0_N0)
def test_sum_rows_f64(emu, n0, inner):
    rng = np.random.default_rng(n0 * 100003 + inner + 1)
    a = (rng.standard_normal((n0, inner)) * 10.0 ** rng.integers(-3, 4, (n0, 1))).astype(np.float32)
    out = np.full(inner, np.nan, np.float32)
    assert emu.emu_sum_rows_f64(_p(a), _SZ(n0), _SZ(inner), _p(out)) == 0
    assert np.array_equal(out, hs.seq_sum_f64(a))              # the float64 sum in row order, rounded once


# ---- block means -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("misalign", [0, 4], ids=["aligned", "base+4"])
@pytest.mark.parametrize("nx,ny,L,s", hs.SCALE3D_CASES)
def test_scale3d(emu, nx, ny, L, s, misalign):
    rng = np.random.default_rng(nx * 1000 + L)
    a = _put(rng.standard_normal((nx, ny, L)).astype(np.float32), misalign)
    o = _buf((nx // s, ny // s, L), 0, np.nan)
    assert emu.emu_scale3d(_p(a), _SZ(nx), _SZ(ny), _SZ(L), _SZ(s), _p(o)) == 0
    assert np.array_equal(o, ob.scale3d(a, s))


@pytest.mark.parametrize("div", [False, True], ids=["sum", "mean"])
@pytest.mark.parametrize("carry", [False, True], ids=["fresh", "carry"])
@pytest.mark.parametrize("m,ny,L,s", [(1, 70, 1001, 3), (2, 70, 1001, 3), (3, 66, 1026, 4), (1, 300, 257, 2), (4, 5, 4096, 5),
                                      (6, 200, 8, 7), (1, 3, 257, 3)])
def test_scale_rows_partial(emu, m, ny, L, s, carry, div):
    assert m < s
    rng = np.random.default_rng(m * 7919 + L)
    rows = rng.standard_normal((m, ny, L)).astype(np.float32)
    nh = ny // s
    c = rng.standard_normal((nh, L)).astype(np.float32) if carry else None
    d = float(s * s) if div else 0.0
    out = np.full((nh, L), np.nan, np.float32)
    assert emu.emu_scale_rows_partial(_p(rows), _SZ(m), _SZ(ny), _SZ(L), _SZ(s), _p(c), C.c_float(d), _p(out)) == 0
    assert np.array_equal(out, hs.scale_rows_partial_ref(rows, s, c, d))


@pytest.mark.parametrize("nx,ny,L,s", hs.SCALE3D_CASES)
def test_scale_rows_partial_continues_scale3d(emu, nx, ny, L, s):
    """what the group layer relies on at a slab edge: the first m rows of a block summed by one slab, the rest added to
    that carry and divided by the next == the block row k_scale3d computes from the whole block, bit for bit"""
    rng = np.random.default_rng(nx * 1000 + L + 5)
    ny = min(ny, 4 * s + 1)                                      # (a few block columns and a ragged one: the identity is per column)
    blk = rng.standard_normal((s, ny, L)).astype(np.float32)     # one block row of the cube
    nh = ny // s
    whole = ob.scale3d(blk, s)[0]
    for m in sorted({1, s // 2, s - 1} - {0}):
        part = np.full((nh, L), np.nan, np.float32)
        head, tail = np.ascontiguousarray(blk[:m]), np.ascontiguousarray(blk[m:])
        assert emu.emu_scale_rows_partial(_p(head), _SZ(m), _SZ(ny), _SZ(L), _SZ(s), None, C.c_float(0.0), _p(part)) == 0
        out = np.full((nh, L), np.nan, np.float32)
        assert emu.emu_scale_rows_partial(_p(tail), _SZ(s - m), _SZ(ny), _SZ(L), _SZ(s), _p(part), C.c_float(float(s * s)), _p(out)) == 0
        assert np.array_equal(out, whole), m


# ---- region-of-interest sums of the windowed source --------------------------------------------------------------
@pytest.mark.parametrize("count", hs.GATHER_W_COUNTS)
@pytest.mark.parametrize("ln", hs.GATHER_W_LENGTHS)
def test_gather_sum_w(emu, ln, count):
    rng = np.random.default_rng(ln * 1009 + count)
    a = rng.standard_normal((count + 29, ln)).astype(np.float32)
    lst = rng.permutation(count + 29)[:count].astype(np.uint32)
    w = [(0.5 + rng.random(ln)).astype(np.float32) for _ in range(3)]
    for on in itertools.product((False, True), repeat=3):      # all 8 subsets of the three factors
        ws = [w[i] if on[i] else None for i in range(3)]
        for div in (0.0, float(count)):
            out = np.full(ln, np.nan, np.float32)
            assert emu.emu_gather_sum_w(_p(a), _SZ(ln), _p(lst), C.c_uint32(count), C.c_float(div), _p(ws[0]), _p(ws[1]), _p(ws[2]),
                                        _p(out)) == 0
            assert np.array_equal(out, hs.gather_sum_w_ref(a, lst, ws, div)), (on, div)


@pytest.mark.parametrize("factor", [False, True], ids=["plain", "factor"])
@pytest.mark.parametrize("n", hs.DIV_VEC_N)
def test_div_vec(emu, n, factor):
    rng = np.random.default_rng(n)
    a = rng.standard_normal(n).astype(np.float32)
    w = rng.random(n).astype(np.float32) if factor else None
    for d in (1.0, 3.0, 63.0, 4097.0):
        out = np.full(n, np.nan, np.float32)
        assert emu.emu_div_vec(_p(a), _p(w), C.c_float(d), _SZ(n), _p(out)) == 0
        assert np.array_equal(out, (a * w if factor else a) / np.float32(d))


# ---- tilt re-laying ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("npix,nt_in,nt_out,max_ins", hs.TILT_CASES)
def test_tilt_and_tilt_sum(emu, npix, nt_in, nt_out, max_ins):
    rng = np.random.default_rng(npix * 31 + nt_out)
    x, taper, ins = hs.tilt_input(rng, npix, nt_in, nt_out, max_ins)
    ref = hs.tilt_ref(x, taper, ins, nt_out)
    o = np.full((npix, nt_out), np.nan, np.float32)
    assert emu.emu_tilt(_SZ(npix), nt_in, nt_out, _p(x), _p(taper), _p(ins), _p(o)) == 0
    assert np.array_equal(o, ref)
    s = np.full(nt_out, np.nan, np.float32)
    rows = emu.emu_tilt_sum(_SZ(npix), nt_in, nt_out, _p(x), _p(taper), _p(ins), _p(s))
    assert rows == min(npix, 1024)                             # tilt_sum_rows: 4 blocks per compute unit at most
    hs.check_parallel_sum(s, ref, f"tilt_sum {npix} x {nt_out}")


@pytest.mark.parametrize("npix", [1, 2, 3, 1025])
def test_tilt_sum_pixel_counts_around_the_row_count(emu, npix):
    """a block's trips take two pixels, rows apart: counts that leave the second pixel of the last trip missing for
    every block, for none, and (1025 pixels over 1024 rows) for all but the first"""
    nt_in, nt_out, max_ins = 60, 70, 10
    rng = np.random.default_rng(npix)
    x, taper, ins = hs.tilt_input(rng, npix, nt_in, nt_out, max_ins)
    s = np.full(nt_out, np.nan, np.float32)
    assert emu.emu_tilt_sum(_SZ(npix), nt_in, nt_out, _p(x), _p(taper), _p(ins), _p(s)) > 0
    hs.check_parallel_sum(s, hs.tilt_ref(x, taper, ins, nt_out), f"tilt_sum {npix}")


@pytest.mark.parametrize("nt_out", [2049, 2304, 4096])
def test_tilt_sum_refuses_long_axes(emu, nt_out):
    """a thread of k_tilt_sum holds 8 x 256 samples of the axis at most: a longer axis is refused, not cut short"""
    npix, nt_in = 3, 1001
    rng = np.random.default_rng(nt_out)
    x, taper, ins = hs.tilt_input(rng, npix, nt_in, nt_out, 40)
    s = np.full(nt_out, np.nan, np.float32)
    assert emu.emu_tilt_sum(_SZ(npix), nt_in, nt_out, _p(x), _p(taper), _p(ins), _p(s)) == -2
    assert np.isnan(s).all()                                   # nothing launched
    s = np.full(hs.TILT_SUM_MAX_NT, np.nan, np.float32)
    x, taper, ins = hs.tilt_input(rng, npix, nt_in, hs.TILT_SUM_MAX_NT, 40)
    assert emu.emu_tilt_sum(_SZ(npix), nt_in, hs.TILT_SUM_MAX_NT, _p(x), _p(taper), _p(ins), _p(s)) == npix
    hs.check_parallel_sum(s, hs.tilt_ref(x, taper, ins, hs.TILT_SUM_MAX_NT), "tilt_sum 2048")


# ---- window multiply, bias / intensity ---------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["aligned", "in_place", "in+4", "out+4", "win+4"])
@pytest.mark.parametrize("npix", hs.TD_WINDOW_NPIX)
@pytest.mark.parametrize("nt", hs.TD_WINDOW_NT)
def test_td_window(emu, nt, npix, form):
    rng = np.random.default_rng(nt * 41 + npix)
    x0 = rng.standard_normal((npix, nt)).astype(np.float32)
    w0 = rng.random(nt).astype(np.float32)
    ref = x0 * w0
    x = _put(x0, 4 if form == "in+4" else 0)
    w = _put(w0, 4 if form == "win+4" else 0)
    out = x if form == "in_place" else _buf((npix, nt), 4 if form == "out+4" else 0, np.nan)
    assert emu.emu_td_window(_SZ(npix), nt, _p(x), _p(w), _p(out)) == 0
    assert np.array_equal(out, ref)
    if form != "in_place":
        assert np.array_equal(x, x0)


@pytest.mark.parametrize("bias", [0, 1], ids=["intensity", "subtract_bias"])
@pytest.mark.parametrize("nt", hs.INTENSITY_NT)
def test_intensity(emu, nt, bias):
    npix = 37
    rng = np.random.default_rng(nt)
    raw = (rng.standard_normal((npix, nt)) + 0.3).astype(np.float32)
    want = ob.subtract_bias(raw) if bias else raw
    imgs = []
    for misalign in (0, 4):
        d = _put(raw, misalign)
        img = np.full(npix, np.nan, np.float32)
        assert emu.emu_intensity(_SZ(npix), nt, _p(d), _p(img), bias) == 0
        assert np.array_equal(d, want)                         # the data bit for bit (untouched without the bias)
        hs.check_intensity(img, want, f"nt {nt}")
        imgs.append(img)
        if bias:   # the image is optional
            d2 = _put(raw, misalign)
            assert emu.emu_intensity(_SZ(npix), nt, _p(d2), None, 1) == 0
            assert np.array_equal(d2, want)
    assert np.array_equal(imgs[0], imgs[1])                    # the same image wherever the traces start
