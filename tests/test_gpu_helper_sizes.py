"""The bandwidth-shaped helper kernels of csrc/kernels.hip on the device, through the C ABI, at the sizes where their
launchers and loops change path — the comparisons of test_emu_helper_sizes.py (same size lists, references and bars,
helper_sizes.py) plus what only the chip shows: 16-byte forms against pointers 4 bytes off, more work than one grid
pass, fused multiply-adds inside ordered sums.

Left to the emulation, because no entry point reaches them: trace length 1 (a context's axis has two samples at
least), pixel sums of a list at every row length (a region's rows are nt or nf long: the session test below),
k_gather_sum_w without the fft window's factor (a session always has one), k_tilt_sum<8> (the one-launch tilted
chain ends at 1280 samples), k_scale_rows_partial and the carry of k_sum_axis0 (the group layer's:
test_gpu_group_slab_edges.py runs them).

Which test runs which branch:
- k_td_window_regs<1|2|4|8|16>, k_td_window<true|false>: test_td_window, test_td_window_more_traces_than_one_grid_pass
- k_intensity<true|false>: test_intensity, test_intensity_more_traces_than_one_grid_pass
- k_colsum_partial<1|2|3|5|8>, levels, ragged tail, the ordered walk: test_pixel_sum, test_pixel_sum_many_rows,
  test_pixel_sum_tail_lanes_second_trip
- k_sum_axis0's unrolled body and divide: test_pixel_mean, test_pixel_mean_more_columns_than_one_grid_pass;
  k_gather_sum's batches: test_roi_mean_counts
- k_scale3d<true|false>: test_scale3d, test_scale3d_more_pixels_than_one_grid_pass
- k_tilt: test_tilt_apply;  k_tilt_sum<5> (+ k_sum_rows_f64): test_tilt_sum_through_the_tilted_chain
- k_colsum_partial with a list, k_gather_sum_w, k_div_vec: test_session_roi_counts_and_factors"""
import numpy as np
import pytest

import helper_sizes as hs
import oracle_binding as ob
import synth
import thz_image_explorer_amd as pkg
from test_gpu_roi import windowed_input

pytestmark = pytest.mark.gpu


class Dev:
    """device arrays at a chosen byte offset behind an allocation's (256-byte aligned) start; outputs start as NaN"""

    def __init__(self, eng):
        self.eng, self.bufs = eng, []

    def __enter__(self):
        return self

    def __exit__(self, *a):
        for b in self.bufs:
            b.free()

    def put(self, a, off=0):
        a = np.ascontiguousarray(a)
        b = self.eng.alloc(a.nbytes + 16)
        self.bufs.append(b)
        assert b.ptr % 16 == 0
        self.eng._check(self.eng.lib.thz_memcpy_h2d(self.eng.ctx, b.ptr + off, a.ctypes.data, a.nbytes))
        return b.ptr + off

    def new(self, shape, off=0, dtype=np.float32):
        return self.put(np.full(shape, np.nan if np.dtype(dtype).kind == "f" else 0, dtype), off)

    def get(self, ptr, shape, dtype=np.float32):
        out = np.empty(shape, dtype)
        self.eng._check(self.eng.lib.thz_memcpy_d2h(self.eng.ctx, out.ctypes.data, ptr, out.nbytes))
        return out


# ---- window multiply -------------------------------------------------------------------------------------------
def _td_window(engine, nt, npix, form, rng):
    x0 = rng.standard_normal((npix, nt)).astype(np.float32)
    w0 = rng.random(nt).astype(np.float32)
    with Dev(engine) as d:
        x = d.put(x0, 4 if form == "in+4" else 0)
        w = d.put(w0, 4 if form == "win+4" else 0)
        out = x if form == "in_place" else d.new((npix, nt), 4 if form == "out+4" else 0)
        engine.apply_td_window(npix, x, w, out)
        assert np.array_equal(d.get(out, (npix, nt)), x0 * w0), (nt, npix, form)
        if form != "in_place":
            assert np.array_equal(d.get(x, (npix, nt)), x0)


@pytest.mark.parametrize("form", ["aligned", "in_place", "in+4", "out+4", "win+4"])
@pytest.mark.parametrize("nt", [n for n in hs.TD_WINDOW_NT if n >= 2])
def test_td_window(engine, nt, form):
    engine.set_time_axis(synth.make_time(nt))
    rng = np.random.default_rng(nt * 41)
    for npix in hs.TD_WINDOW_NPIX:
        _td_window(engine, nt, npix, form, rng)


@pytest.mark.parametrize("form", ["aligned", "in+4"])
@pytest.mark.parametrize("nt", [256, 260, 1001])
def test_td_window_more_traces_than_one_grid_pass(engine, nt, form):
    """2048 blocks of 4 waves at most: 16 387 traces are two passes and three traces of a third"""
    engine.set_time_axis(synth.make_time(nt))
    _td_window(engine, nt, 2 * 2048 * 4 + 3, form, np.random.default_rng(nt))


# ---- bias / intensity --------------------------------------------------------------------------------------------
def _intensity(engine, nt, npix, bias, off, rng):
    raw = (rng.standard_normal((npix, nt)) + 0.3).astype(np.float32)
    want = ob.subtract_bias(raw) if bias else raw
    with Dev(engine) as d:
        x = d.put(raw, off)
        img = d.new((npix,))
        if bias:
            engine.subtract_bias(npix, x, img)
        else:
            engine.intensity(npix, x, img)
        assert np.array_equal(d.get(x, (npix, nt)), want)       # the data bit for bit (untouched without the bias)
        got = d.get(img, (npix,))
        err, bar = hs.check_intensity(got, want, f"nt {nt}")
        print(f"intensity nt={nt} npix={npix} bias={bias} off={off}: max err {err:.3e}, bar {bar:.3e}")
        if bias:   # the image is optional
            x2 = d.put(raw, off)
            engine.subtract_bias(npix, x2, None)
            assert np.array_equal(d.get(x2, (npix, nt)), want)
        return got


@pytest.mark.parametrize("bias", [0, 1], ids=["intensity", "subtract_bias"])
@pytest.mark.parametrize("nt", [n for n in hs.INTENSITY_NT if n >= 2])
def test_intensity(engine, nt, bias):
    engine.set_time_axis(synth.make_time(nt))
    a = _intensity(engine, nt, 37, bias, 0, np.random.default_rng(nt))
    b = _intensity(engine, nt, 37, bias, 4, np.random.default_rng(nt))    # base + 4
    assert np.array_equal(a, b)                                # the same image wherever the traces start


@pytest.mark.parametrize("bias", [0, 1], ids=["intensity", "subtract_bias"])
@pytest.mark.parametrize("nt", [256, 1001])
def test_intensity_more_traces_than_one_grid_pass(engine, nt, bias):
    engine.set_time_axis(synth.make_time(nt))
    _intensity(engine, nt, 2 * 2048 * 4 + 3, bias, 0, np.random.default_rng(nt + 1))


# ---- pixel sums and means ------------------------------------------------------------------------------------------
def _pixel_sum(engine, nrows, L, rng):
    a = rng.standard_normal((nrows, L)).astype(np.float32)
    with Dev(engine) as d:
        got = []
        for off in (0, 4):   # base + 4: the same chunks at addresses no 16-byte access may assume
            p = d.put(a, off)
            o = d.new((L,), off)
            engine.pixel_sum(nrows, L, 1, p, o)
            got.append(d.get(o, (L,)))
    err, bar = hs.check_parallel_sum(got[0], a, f"{nrows} x {L} (KC {hs.colsum_kc(L)})")
    print(f"pixel_sum {nrows} x {L} KC={hs.colsum_kc(L)}: max err {err:.3e}, bar {bar:.3e}")
    assert np.array_equal(got[0], got[1])
    if nrows < 64 or hs.colsum_kc(L) == 0:   # the ordered walk: sequential float32, bit for bit
        assert np.array_equal(got[0], hs.seq_sum_f32(a))


@pytest.mark.parametrize("nrows,L", hs.pixel_sum_cases(hs.PIXEL_SUM_LENGTHS))
def test_pixel_sum(engine, nrows, L):
    _pixel_sum(engine, nrows, L, np.random.default_rng(1000 * nrows + L))


@pytest.mark.parametrize("nrows,L", [(2049 * 2, 129), (2049 * 2 + 1, 1026), (10007, 258), (2049 * 2, 4098)])
def test_pixel_sum_many_rows(engine, nrows, L):
    """more rows than twice the 2048 row groups: every block adds several rows, some an odd one more"""
    _pixel_sum(engine, nrows, L, np.random.default_rng(nrows + L))


@pytest.mark.parametrize("nrows,L", [(65 * 2048 + 1, 5), (65 * 2048 + 3, 7)])
def test_pixel_sum_tail_lanes_second_trip(engine, nrows, L):
    """more than 64 x 2048 rows (the 512 x 512 cube's): wave 0's lanes, which split a block's rows for the ragged
    tail columns, walk on by 64 row groups a second time — a block has 65 rows, the first ones 66"""
    _pixel_sum(engine, nrows, L, np.random.default_rng(nrows + L))


def test_pixel_sum_two_components(engine):
    rng = np.random.default_rng(3)
    a = rng.standard_normal((300, 513, 2)).astype(np.float32)
    with Dev(engine) as d:
        o = d.new((1026,))
        engine.pixel_sum(300, 513, 2, d.put(a), o)
        hs.check_parallel_sum(d.get(o, (1026,)), a.reshape(300, 1026), "300 x 513 x 2")


@pytest.mark.parametrize("ncomp", [1, 2])
@pytest.mark.parametrize("nf", [129, 501, 2049])
def test_pixel_mean(engine, nf, ncomp):
    """k_sum_axis0 twice (over x with / nx, over y with / ny) in the reference's order: row counts around the 16-row
    unrolled body, ny * nf * ncomp columns — up to 135 234, many blocks in one pass of the grid"""
    rng = np.random.default_rng(nf + ncomp)
    for nx in (15, 16, 17, 33):
        for ny in (15, 16, 17, 33):
            a = rng.standard_normal((nx, ny, nf) + ((2,) if ncomp == 2 else ())).astype(np.float32)
            with Dev(engine) as d:
                o = d.new((nf * ncomp,))
                engine.pixel_mean(nx, ny, nf, ncomp, d.put(a), o)
                assert np.array_equal(d.get(o, (nf * ncomp,)), ob.pixel_mean(a, ncomp).ravel()), (nx, ny)


def test_pixel_mean_more_columns_than_one_grid_pass(engine):
    """k_sum_axis0's grid is 4096 blocks of 256 columns at most: 257 x 2049 x 2 = 1 053 186 columns of the sum over x
    take a second trip of the grid-stride loop for the last 4610"""
    nx, ny, nf = 3, 257, 2049
    assert ny * nf * 2 > 4096 * 256
    a = np.random.default_rng(77).standard_normal((nx, ny, nf, 2)).astype(np.float32)
    with Dev(engine) as d:
        o = d.new((nf * 2,))
        engine.pixel_mean(nx, ny, nf, 2, d.put(a), o)
        assert np.array_equal(d.get(o, (nf * 2,)), ob.pixel_mean(a, 2).ravel())


# ---- regions of interest ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ln", [33, 257])
@pytest.mark.parametrize("count", [1, 63, 64, 65, 4097])
def test_roi_mean_counts(engine, count, ln):
    """k_gather_sum's 64-pixel batches: masks holding exactly `count` pixels, the mean and the bare sum against a
    sequential float32 sum in the reference's order (y outer, x inner, row shape0 - y - 1)"""
    s0, s1 = 67, 71
    rng = np.random.default_rng(count + ln)
    data = rng.standard_normal((s0, s1, ln)).astype(np.float32)
    mask = np.zeros(s0 * s1, np.uint8)
    mask[rng.permutation(s0 * s1)[:count]] = 1
    mask = mask.reshape(s0, s1)
    acc = np.zeros(ln, np.float32)
    for y in range(s0):
        for x in range(s1):
            if mask[y, x]:
                acc = acc + data[s0 - y - 1, x]
    with Dev(engine) as d:
        p, m = d.put(data), d.put(mask)
        for sum_only in (False, True):
            o, c = d.new((ln,)), d.new((1,), dtype=np.uint32)
            engine.roi_mean(p, s0, s1, ln, m, o, c, sum_only=sum_only)
            assert int(d.get(c, (1,), np.uint32)[0]) == count
            assert np.array_equal(d.get(o, (ln,)), acc if sum_only else acc / np.float32(count)), sum_only


# the regions of the session test on a 40 x 40 grid: exactly 63, 64, 129 and 1200 pixels (the oracle's mask rule)
ROI_POLYS = {63: [[3, 4], [10, 4], [10, 13], [3, 13]], 64: [[20, 2], [28, 2], [28, 10], [20, 10]],
             129: [[2, 20], [18, 20], [18, 28], [3, 28], [3, 29], [2, 29]], 1200: [[5, 0], [35, 0], [35, 40], [5, 40]]}


@pytest.mark.parametrize("td_before", [0, 1], ids=["no_td", "td"])
@pytest.mark.parametrize("tilt", [0, 1], ids=["no_taper", "taper"])
@pytest.mark.parametrize("want_means", [1, 2])
def test_session_roi_counts_and_factors(engine, want_means, tilt, td_before):
    """the kernels without an entry point of their own, at the pixel counts around their batches: want_means 1 — the
    parallel list sums (k_gather_sum below 64 pixels, k_colsum_partial with a list from there, two levels above 128)
    and k_div_vec with the composed multiplier; want_means 2 — k_gather_sum_w, bit for bit the oracle's ROI mean of the
    windowed traces, with the Tilt stage's taper (a tilt of zero degrees multiplies, it does not re-lay) and the Time
    Band Pass each present and absent.  test_gpu_roi.py and test_gpu_roi_sequences.py run every factor present and the
    re-laid case on the golden polygons."""
    nx = ny = 40
    nt = 1001
    time, cube = synth.make_cube(nx, ny, nt)
    counts = sorted(ROI_POLYS)
    polys = [np.array(ROI_POLYS[c], np.uint64) for c in counts]
    cfg = pkg.chain_cfg_default(time)
    cfg.want_means, cfg.tilt_active, cfg.td_before_active = want_means, tilt, td_before
    cfg.tilt_x_deg = cfg.tilt_y_deg = 0.0
    cfg.td_before_low = float(time[0]) + 4.0       # the Time Band Pass differs from 1 inside the traces
    sess = pkg.Session(engine, nx, ny, time)
    try:
        sess.upload(cube, subtract_bias=False)
        sess.set_rois(polys)
        sess.recompute(cfg)
        assert sess.nt_out == nt
        nf = nt // 2 + 1
        arrays = dict(signal_fft=sess.download(pkg.BUF_AMPLITUDES).reshape(nx, ny, nf),
                      phase_fft=sess.download(pkg.BUF_PHASES).reshape(nx, ny, nf),
                      signal=sess.download(pkg.BUF_DATA).reshape(nx, ny, nt), roi_data=windowed_input(cube, time, cfg))
        for i, (count, poly) in enumerate(zip(counts, polys)):
            r = sess.roi(i)
            assert r["count"] == count
            mask, _ = ob.roi_mask(poly, 1, nx, ny)
            sel = np.flipud(mask).astype(bool)     # mask position (x, y) samples pixel [shape0 - y - 1, x]
            for key, arr in arrays.items():
                if want_means == 2:
                    assert np.array_equal(r[key], ob.average_polygon_roi(arr, poly, 1)), (count, key)
                else:
                    rows = arr[sel].astype(np.float64)
                    assert np.isfinite(r[key]).all()
                    err = float(np.abs(r[key] - rows.mean(0)).max())
                    bar = hs.SUM_BAR * float(np.abs(rows).sum(0).max()) / count
                    print(f"roi {count} px {key}: max err {err:.3e}, bar {bar:.3e}")
                    assert err <= bar, (count, key, err, bar)
    finally:
        sess.close()


# ---- block means ---------------------------------------------------------------------------------------------------
def _scale3d(engine, nx, ny, L, s, rng):
    a = rng.standard_normal((nx, ny, L)).astype(np.float32)
    ref = ob.scale3d(a, s)
    with Dev(engine) as d:
        for off_in, off_out in ((0, 0), (4, 0), (0, 4), (4, 4)):
            o = d.new(ref.shape, off_out)
            engine.scale3d(d.put(a, off_in), nx, ny, L, 1, s, o)
            assert np.array_equal(d.get(o, ref.shape), ref), (off_in, off_out)


@pytest.mark.parametrize("nx,ny,L,s", hs.SCALE3D_CASES)
def test_scale3d(engine, nx, ny, L, s):
    _scale3d(engine, nx, ny, L, s, np.random.default_rng(nx * 1000 + L))


@pytest.mark.parametrize("nx,ny,L,s", [(323, 321, 8, 2), (323, 321, 6, 2), (1121, 1131, 4, 7)])
def test_scale3d_more_pixels_than_one_grid_pass(engine, nx, ny, L, s):
    """2048 blocks of 4 waves, a wave per output pixel: 161 x 160 = 25 760 and 160 x 161 pixels are three passes and a
    bit at a short L, with a ragged edge on both axes; the last case with a large s"""
    assert (nx // s) * (ny // s) >= 3 * 256 * 8 * 4 and nx % s and ny % s
    _scale3d(engine, nx, ny, L, s, np.random.default_rng(nx + L))


def test_scale3d_two_components(engine):
    rng = np.random.default_rng(9)
    a = rng.standard_normal((65, 66, 513, 2)).astype(np.float32)
    ref = ob.scale3d(a, 4, 2)
    with Dev(engine) as d:
        o = d.new(ref.shape)
        engine.scale3d(d.put(a), 65, 66, 513, 2, 4, o)
        assert np.array_equal(d.get(o, ref.shape), ref)


# ---- tilt re-laying --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("npix,nt_in,nt_out,max_ins", hs.TILT_CASES)
def test_tilt_apply(engine, npix, nt_in, nt_out, max_ins):
    rng = np.random.default_rng(npix * 31 + nt_out)
    x, taper, ins = hs.tilt_input(rng, npix, nt_in, nt_out, max_ins)
    with Dev(engine) as d:
        o = d.new((npix, nt_out))
        engine.tilt_apply(npix, d.put(x), nt_in, d.put(taper), d.put(ins), nt_out, o)
        assert np.array_equal(d.get(o, (npix, nt_out)), hs.tilt_ref(x, taper, ins, nt_out))


def test_tilt_apply_more_traces_than_one_grid_pass(engine):
    npix, nt_in, nt_out, max_ins = 2 * 2048 * 4 + 3, 60, 70, 10
    x, taper, ins = hs.tilt_input(np.random.default_rng(5), npix, nt_in, nt_out, max_ins)
    with Dev(engine) as d:
        o = d.new((npix, nt_out))
        engine.tilt_apply(npix, d.put(x), nt_in, d.put(taper), d.put(ins), nt_out, o)
        assert np.array_equal(d.get(o, (npix, nt_out)), hs.tilt_ref(x, taper, ins, nt_out))


@pytest.mark.parametrize("npix", [1, 1023, 1025, 2500])
@pytest.mark.parametrize("nt_out", [1025, 1280])
def test_tilt_sum_through_the_tilted_chain(engine, nt_out, npix):
    """k_tilt_sum<5> behind thz_pipeline_tilted's source sum: 1024 partial rows at most, two pixels per trip — 1025
    pixels leave the second pixel of the last trip missing for every block but the first, 2500 for the blocks from 452.
    Against float64 column sums of the cube thz_tilt_apply writes from the same inputs (itself bit for bit k_tilt's
    restatement)."""
    nt_in = 1001
    nf = nt_out // 2 + 1
    rng = np.random.default_rng(npix * 31 + nt_out)
    x, taper, ins = hs.tilt_input(rng, npix, nt_in, nt_out, nt_out - nt_in)
    engine.set_time_axis(synth.make_time(nt_out))
    assert engine.kernel_variant().startswith("fbp-")          # the one-launch form: the sum is k_tilt_sum's
    with Dev(engine) as d:
        src, tap, idx = d.put(x), d.put(taper), d.put(ins)
        ones_t, ones_f = d.put(np.ones(nt_out, np.float32)), d.put(np.ones(nf, np.float32))
        outs = [d.new(s) for s in ((npix, nf, 2), (npix, nf), (npix, nf), (npix, nt_out), (npix,))]
        ssum, ext = d.new((nt_out,)), d.new((npix, nt_out))
        engine.pipeline_tilted(npix, src, nt_in, tap, idx, ones_t, ones_f, None, ones_t, *outs, src_sum=ssum)
        engine.tilt_apply(npix, src, nt_in, tap, idx, nt_out, ext)
        cube = d.get(ext, (npix, nt_out))
        got = d.get(ssum, (nt_out,))
    assert np.array_equal(cube, hs.tilt_ref(x, taper, ins, nt_out))
    err, bar = hs.check_parallel_sum(got, cube, f"tilt_sum {npix} x {nt_out}")
    print(f"tilt_sum {npix} x {nt_out}: max err {err:.3e}, bar {bar:.3e}")
