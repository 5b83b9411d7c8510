"""Size lists, plain references and bars shared by test_emu_helper_sizes.py (the kernels on host threads) and
test_gpu_helper_sizes.py (the same kernels through the C ABI): the bandwidth-shaped helpers of csrc/kernels.hip at
the sizes where their launchers and loops change path.

Bars (the project's existing ones, nothing new):
- ordered sums, copies, multiplies and exact quotients: bit for bit against a float32 numpy restatement that performs
  the same IEEE operations in the same order;
- parallel (order-free) sums: |got - float64 sum| <= 2e-6 x max over columns of sum |a| (SUM_BAR);
- intensities: 1e-5 of the float64 image's maximum (TOL of test_gpu_parity.py)."""
import numpy as np

SUM_BAR = 2e-6
TOL = 1e-5

# ---- pixel sums (launch_pixel_sum_rows -> k_colsum_partial<KC> / k_sum_axis0 / k_gather_sum)
# rows: 63 the ordered walk, 64 the first parallel size, 129 the first with a second level (more than 128 row groups),
# 300, 4097 more rows than the 2048 row groups (several rows per block, an odd one left for the tail loop)
PIXEL_SUM_ROWS = (63, 64, 129, 300, 4097)
# row lengths: 16-byte chunks per thread = ceil((L / 4) / 256) picks KC: <= 1024 + 3 -> 1, <= 2051 -> 2, <= 3075 -> 3,
# <= 5123 -> 5, <= 8195 -> 8, above: the ordered walk; L % 4 != 0 leaves a ragged tail to wave 0
PIXEL_SUM_LENGTHS = (1, 3, 4, 5, 1023, 1024, 1025, 1027, 2048, 2050, 3002, 3072, 3076, 4098, 5120, 5124, 8191, 8194,
                     8195, 8196, 8200)
PIXEL_SUM_TALL_LENGTHS = (1, 3, 4, 5, 1025)   # the emulation runs the tallest row count only at these (its run time)


def pixel_sum_cases(tall_lengths=PIXEL_SUM_TALL_LENGTHS):
    return [(r, L) for r in PIXEL_SUM_ROWS for L in PIXEL_SUM_LENGTHS if r < 4097 or L in tall_lengths]


# one level with the row groups capped (nrows, L, max_groups): more than 64 rows to a block, L % 4 of 1, 2 and 3, KC 1 and 2
COLSUM_LEVEL_CASES = ((300, 5, 2), (131, 7, 1), (517, 1026, 3))


def colsum_kc(L):
    """the k_colsum_partial<KC> launch_colsum_partial picks for rows of L floats (0: it refuses, the ordered walk runs)"""
    chunks = (L // 4 + 255) // 256
    for kc in (1, 2, 3, 5, 8):
        if chunks <= kc:
            return kc
    return 0


def pixel_sum_input(rng, nrows, L, with_list):
    """(array, list or None, the rows that are summed): the list is a permutation prefix of a taller array"""
    tall = nrows + 41 if with_list else nrows
    a = rng.standard_normal((tall, L)).astype(np.float32)
    if not with_list:
        return a, None, a
    lst = rng.permutation(tall)[:nrows].astype(np.uint32)
    return a, lst, a[lst]


def check_parallel_sum(got, rows, what=""):
    """order-free float32 column sums of `rows` against float64: finite everywhere, within SUM_BAR x max_col sum |a|.
    Returns (worst error, bar)."""
    assert np.isfinite(got).all(), f"{what}: unwritten or non-finite columns {np.nonzero(~np.isfinite(got))[0][:8]}"
    r64 = rows.astype(np.float64)
    err = float(np.abs(got - r64.sum(0)).max())
    bar = SUM_BAR * float(np.abs(r64).sum(0).max())
    assert err <= bar, f"{what}: {err:.3e} > {bar:.3e}"
    return err, bar


# ---- ordered sums
SUM_AXIS0_N0 = (1, 15, 16, 17, 31, 32, 33, 100)      # around the 16-row unrolled body
SUM_AXIS0_INNER = (1, 255, 256, 257, 70000)           # around one block of 256 columns; 70000: 274 blocks, a ragged last one


def seq_sum_f32(rows, carry=None, div=0.0):
    """k_sum_axis0 / k_gather_sum: sequential float32 sum over axis 0 from `carry` (or 0), then / div when div > 0"""
    s = np.zeros(rows.shape[1:], np.float32) if carry is None else carry.astype(np.float32).copy()
    for r in rows:
        s = s + r
    return s / np.float32(div) if div > 0 else s


def seq_sum_f64(rows):
    """k_sum_rows_f64: the rows added in double in row order, rounded to float32 once"""
    s = np.zeros(rows.shape[1:], np.float64)
    for r in rows:
        s = s + r.astype(np.float64)
    return s.astype(np.float32)


# ---- block means
SCALE3D_CASES = ((64, 70, 1001, 3), (65, 66, 1026, 4), (9, 300, 2002, 2), (5, 5, 4096, 5), (40, 3, 257, 3), (200, 200, 8, 7))


def scale_rows_partial_ref(rows, s, carry=None, div=0.0):
    """k_scale_rows_partial: rows (m, ny, L) of a block of s rows -> (ny // s, L): the adds row by row, column by
    column from `carry`, the exact quotient by div when div > 0"""
    m, ny, L = rows.shape
    nh = ny // s
    acc = np.zeros((nh, L), np.float32) if carry is None else carry.astype(np.float32).copy()
    for i in range(m):
        for j in range(s):
            acc = acc + rows[i, j:nh * s:s, :]
    return acc / np.float32(div) if div > 0 else acc


# ---- region-of-interest sums of the windowed source
GATHER_W_LENGTHS = (1, 63, 64, 65, 1001)
GATHER_W_COUNTS = (1, 63, 64, 65, 129, 300)          # around the 64-pixel load batch


def gather_sum_w_ref(arr, lst, ws, div=0.0):
    """k_gather_sum_w: sum in list order of arr[p] * w1 * w2 * w3, one float32 rounding per multiply and per add"""
    s = np.zeros(arr.shape[1], np.float32)
    for p in lst:
        v = arr[p]
        for w in ws:
            if w is not None:
                v = v * w
        s = s + v
    return s / np.float32(div) if div > 0 else s


# ---- tilt re-laying: (npix, nt_in, nt_out, largest insert index)
TILT_CASES = ((1, 1001, 1025, 24), (700, 1001, 1280, 279), (2500, 1001, 1281, 280), (33, 1500, 2048, 548),
              (5, 1001, 1001, 0), (9, 64, 64, 20))   # the last one clips at the end of the axis
TILT_SUM_MAX_NT = 2048


def tilt_input(rng, npix, nt_in, nt_out, max_ins):
    x = rng.standard_normal((npix, nt_in)).astype(np.float32)
    taper = rng.random(nt_in).astype(np.float32)
    ins = rng.integers(0, max_ins + 1, npix).astype(np.int32)
    ins[0] = max_ins                                   # the extreme is present whatever the draw
    if npix > 1:
        ins[-1] = 0
    return x, taper, ins


def tilt_ref(x, taper, ins, nt_out):
    """k_tilt: the front filled with the first sample, the tapered trace at its insert index, clipped, zeros behind"""
    npix, nt_in = x.shape
    ref = np.zeros((npix, nt_out), np.float32)
    xt = x * taper
    for p in range(npix):
        i = int(ins[p])
        ref[p, :i] = x[p, 0]
        n = min(nt_in, nt_out - i)
        ref[p, i:i + n] = xt[p, :n]
    return ref


# ---- window multiply, bias / intensity, vector quotient
TD_WINDOW_NT = (1, 3, 4, 255, 256, 512, 768, 1024, 2048, 2304, 4096, 4100, 8192)   # regs<1|2|4|8|16>, vector, scalar
TD_WINDOW_NPIX = (1, 5, 37)
INTENSITY_NT = (1, 3, 4, 63, 64, 255, 256, 260, 1001, 4096)
DIV_VEC_N = (1, 255, 257, 70000)


def intensity_f64(data):
    return (data.astype(np.float64) ** 2).sum(-1)


def check_intensity(img, data, what=""):
    ref = intensity_f64(data)
    err = float(np.abs(img - ref).max())
    bar = TOL * float(ref.max())
    assert err <= bar, f"{what}: {err:.3e} > {bar:.3e}"
    return err, bar
