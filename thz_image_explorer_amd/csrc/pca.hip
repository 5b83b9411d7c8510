// pca.hip — K19: principal components of a scan: column sums, the Gram matrix of the centred columns
// on the exact-f32 matrix instruction, and the score images.
//
//   k_pca_sums      column sums over the unmasked pixels in f64, a slab of pixels per block row; entry L of every row
//                   of partials is the slab's count (a column of ones)
//   k_pca_fold      adds the slabs' partial rows in slab order
//   k_pca_gram      G = a^T a, a = X - mu with masked pixels as zero rows.  A block owns a 128 x 128 block tile of the
//                   upper triangle and a slab of pixel chunks; each of its four waves owns 2 x 2 tiles of 32 x 32, each
//                   tile one v_mfma_f32_32x32x2_f32 accumulator whose k is the pixel index.  The block stages 32 pixels
//                   x 128 columns of a (once for a block tile on the diagonal, twice otherwise) in LDS; lane l of a wave
//                   reads a[pixel k + (l >> 5)][column (l & 31)] of its two row tiles and its two column tiles — on a
//                   diagonal tile the same registers are both operands.  After THZ_PCA_CHAIN pixels at the most the
//                   f32 accumulators are added into f64 registers and start again from zero; at the end the f64
//                   tiles go out as this slab's partials.  Tiles below the diagonal are never computed.
//   k_pca_gram_fold adds the slabs' partial tiles in slab order and writes G with its lower triangle as the mirror
//   k_pca_scores    one wave per pixel: lane l adds j = l, l + 64, ... with fmaf, then the lanes as a fixed tree
//
// No floating-point atomics anywhere: the same inputs give the same bits on every run.
#include "pca.hpp"
#include "kernels.hpp"
#include "thz_device.hpp"

#include "../../include/thzgpu.h"

namespace thz {

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kChain = THZ_PCA_CHAIN;  // products one f32 accumulator takes before it is added into f64
constexpr int kStage = 32;             // pixels staged per round
constexpr int kStrip = 128;            // columns of a block tile's side
// LDS row pitch: the two pixels of one instruction (lanes 0..31 and 32..63) fall on different halves of the 64 banks
constexpr int kPitch = kStrip + 32;
constexpr int kMuFloats = THZ_PCA_MAX_LEN;
static_assert(kChain % kStage == 0 && kChain <= 4096, "a chunk is a whole number of staging rounds");

__device__ __forceinline__ bool pixel_on(const PcaView &v, size_t p) { return !v.mask || v.mask[p] != 0; }

// block tile number -> (bi, bj), bi <= bj, row by row of the upper triangle of an nb x nb grid
__device__ __forceinline__ void upper_pair(int t, int nb, int &bi, int &bj)
{
    bi = 0;
    while (t >= nb - bi) {
        t -= nb - bi;
        ++bi;
    }
    bj = bi + t;
}
// ... and the number of tile (ti, tj), ti <= tj, in that order
__host__ __device__ __forceinline__ int upper_index(int ti, int tj, int n) { return ti * n - ti * (ti - 1) / 2 + (tj - ti); }

}  // namespace

// ---------------------------------------------------------------- sums

// blockDim 256 = rows x cw threads (cw: the power of two >= L + 1, at most 256): thread (r, c) adds column c of the
// pixels p0 + r, p0 + r + rows, ... of its slab, four accumulators deep; the rows are then added in row order.
__global__ __launch_bounds__(256) void k_pca_sums(PcaView v, int cw, size_t slab_pix, double *__restrict__ partial)
{
    __shared__ double red[256];
    const int n = v.L + 1;
    const int rows = 256 / cw;
    const int c = (int)blockIdx.x * cw + (int)(threadIdx.x % cw), r = (int)(threadIdx.x / cw);
    const size_t p0 = (size_t)blockIdx.y * slab_pix;
    const size_t p1 = p0 + slab_pix < v.npix ? p0 + slab_pix : v.npix;
    const bool ones = c == v.L;
    const float *col = v.x + (size_t)(c < v.L ? c : 0) * v.col_step;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    if (c < n) {
        const size_t step = (size_t)rows;
        for (size_t p = p0 + (size_t)r; p < p1; p += 4 * step) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const size_t pu = p + (size_t)u * step;
                if (pu < p1) {
                    const float x = ones ? 1.0f : col[pu * v.row_stride];
                    s[u] += pixel_on(v, pu) ? (double)x : 0.0;
                }
            }
        }
    }
    red[threadIdx.x] = (s[0] + s[1]) + (s[2] + s[3]);
    __syncthreads();
    if (r == 0 && c < n) {
        double t = 0.0;
        for (int q = 0; q < rows; ++q) t += red[q * cw + (int)(threadIdx.x % cw)];
        partial[(size_t)blockIdx.y * (size_t)n + (size_t)c] = t;
    }
}

__global__ __launch_bounds__(256) void k_pca_fold(const double *__restrict__ partial, int slabs, int n, double *__restrict__ out)
{
    const int e = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (e >= n) return;
    double t = 0.0;
    for (int s = 0; s < slabs; ++s) t += partial[(size_t)s * (size_t)n + (size_t)e];
    out[e] = t;
}

namespace {

struct SumsPlan {
    int cw, col_blocks, slabs;
    size_t slab_pix;
};
SumsPlan sums_plan(size_t npix, int L)
{
    SumsPlan q;
    const int n = L + 1;
    q.cw = 1;
    while (q.cw < n && q.cw < 256) q.cw <<= 1;
    q.col_blocks = (n + q.cw - 1) / q.cw;
    const size_t want = (npix + 1023) / 1024;  // about a thousand pixels of a column per thread row
    q.slabs = (int)(want < 1 ? 1 : (want > 1024 ? 1024 : want));
    q.slab_pix = (npix + (size_t)q.slabs - 1) / (size_t)q.slabs;
    if (q.slab_pix < 1) q.slab_pix = 1;
    q.slabs = (int)((npix + q.slab_pix - 1) / q.slab_pix);
    if (q.slabs < 1) q.slabs = 1;
    return q;
}

}  // namespace

size_t pca_sums_ws_bytes(size_t npix, int L)
{
    const SumsPlan q = sums_plan(npix, L);
    return ((size_t)q.slabs + 1) * (size_t)(L + 1) * sizeof(double);
}

void launch_pca_sums(hipStream_t st, const PcaView &v, void *ws)
{
    const SumsPlan q = sums_plan(v.npix, v.L);
    double *out = static_cast<double *>(ws), *partial = out + (v.L + 1);
    THZ_LAUNCH(k_pca_sums, dim3((unsigned)q.col_blocks, (unsigned)q.slabs), 256, 0, st, v, q.cw, q.slab_pix, partial);
    THZ_LAUNCH(k_pca_fold, (unsigned)((v.L + 1 + 255) / 256), 256, 0, st, partial, q.slabs, v.L + 1, out);
}

// ---------------------------------------------------------------- Gram matrix

namespace {

// 32 pixels x 128 columns of a = X - mu into a staging strip: thread t takes column (t & 127) of the rows (t >> 7) + 2 i.
// Columns beyond L, pixels beyond the chunk and masked pixels are zeros.
__device__ __forceinline__ void stage_strip(float *dst, const PcaView &v, const float *mu, int col0, size_t q, size_t p1)
{
    const int c = (int)(threadIdx.x & (kStrip - 1)), r0 = (int)(threadIdx.x >> 7);
    const int col = col0 + c;
    const bool col_on = col < v.L;
    const float m = col_on ? mu[col] : 0.0f;
    const float *src = v.x + (size_t)(col_on ? col : 0) * v.col_step;
    float x[kStage / 2];
#pragma unroll
    for (int i = 0; i < kStage / 2; ++i) {
        const size_t p = q + (size_t)(r0 + 2 * i);
        const bool on = col_on && p < p1 && pixel_on(v, p);
        x[i] = on ? src[p * v.row_stride] - m : 0.0f;
    }
#pragma unroll
    for (int i = 0; i < kStage / 2; ++i) dst[(r0 + 2 * i) * kPitch + c] = x[i];
}

struct TileSet {
    bool on[2][2];
};

// One staged round of a wave's 2 x 2 tiles: A and B are the wave's 64 columns of the row strip and of the column strip.
// SAME: the wave sits on the diagonal — its row tiles ARE its column tiles, and both operands are the same registers.
template <bool SAME>
__device__ __forceinline__ void round_mfma(const float *A, const float *B, int lane, const TileSet &t, f32x16 (&acc)[2][2])
{
    const int at = (lane >> 5) * kPitch + (lane & 31);
#pragma unroll 4
    for (int k = 0; k < kStage; k += 2) {
        const int o = k * kPitch + at;
        const float a0 = A[o], a1 = A[o + 32];
        const float b0 = SAME ? a0 : B[o], b1 = SAME ? a1 : B[o + 32];
        if (t.on[0][0]) acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
        if (t.on[0][1]) acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
        if (t.on[1][0]) acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
        if (t.on[1][1]) acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
    }
}

}  // namespace

// grid: (block tiles of the upper triangle, slabs).  partial: [slab][tile (ti <= tj)][32 rows][32 columns] doubles.
__global__ __launch_bounds__(256) void k_pca_gram(PcaView v, const float *__restrict__ mu, size_t slab_chunks,
                                                  double *__restrict__ partial)
{
    __shared__ float sA[kStage * kPitch], sB[kStage * kPitch];
    const int lane = lane_id();
    const int wave = THZ_UNIFORM((int)(threadIdx.x >> 6));
    const int n32 = (v.L + 31) / 32, nb = (v.L + kStrip - 1) / kStrip;
    int bi, bj;
    upper_pair((int)blockIdx.x, nb, bi, bj);
    const bool diag_block = bi == bj;
    const int wi = wave >> 1, wj = wave & 1;
    const int ti0 = bi * 4 + wi * 2, tj0 = bj * 4 + wj * 2;  // the first of this wave's 2 x 2 tiles
    TileSet t;
    bool any = false;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            t.on[a][b] = ti0 + a <= tj0 + b && tj0 + b < n32;  // the upper triangle, inside the matrix
            any = any || t.on[a][b];
        }
    const bool same = diag_block && wi == wj;
    const float *A = sA + wi * 64, *B = (diag_block ? sA : sB) + wj * 64;

    const size_t chunks = (v.npix + (size_t)kChain - 1) / (size_t)kChain;
    const size_t c0 = (size_t)blockIdx.y * slab_chunks;
    const size_t c1 = c0 + slab_chunks < chunks ? c0 + slab_chunks : chunks;
    double sum[2][2][16];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int e = 0; e < 16; ++e) sum[a][b][e] = 0.0;

    for (size_t c = c0; c < c1; ++c) {
        const size_t p0 = c * (size_t)kChain;
        const size_t p1 = p0 + (size_t)kChain < v.npix ? p0 + (size_t)kChain : v.npix;
        f32x16 acc[2][2];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[a][b][e] = 0.0f;
        for (size_t q = p0; q < p1; q += kStage) {
            __syncthreads();  // the round before has been read
            stage_strip(sA, v, mu, bi * kStrip, q, p1);
            if (!diag_block) stage_strip(sB, v, mu, bj * kStrip, q, p1);
            __syncthreads();
            if (any) {
                if (same) round_mfma<true>(A, A, lane, t, acc);
                else round_mfma<false>(A, B, lane, t, acc);
            }
        }
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int e = 0; e < 16; ++e) sum[a][b][e] += (double)acc[a][b][e];
    }

    // C/D map of the 32 x 32 shapes: column = lane & 31, row = (e & 3) + 8 (e >> 2) + 4 (lane >> 5)
    const int ntri = n32 * (n32 + 1) / 2;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            if (!t.on[a][b]) continue;
            double *dst = partial + ((size_t)blockIdx.y * (size_t)ntri + (size_t)upper_index(ti0 + a, tj0 + b, n32)) * 1024;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int row = (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
                dst[row * 32 + (lane & 31)] = sum[a][b][e];
            }
        }
}

// grid: (tiles of the upper triangle), 256 threads, four entries of the tile each
__global__ __launch_bounds__(256) void k_pca_gram_fold(const double *__restrict__ partial, int slabs, int L, double *__restrict__ G)
{
    const int n32 = (L + 31) / 32;
    const int ntri = n32 * (n32 + 1) / 2;
    int ti, tj;
    upper_pair((int)blockIdx.x, n32, ti, tj);
    for (int e = (int)threadIdx.x; e < 1024; e += 256) {
        const int row = e >> 5, col = e & 31;
        const int i = ti * 32 + row, j = tj * 32 + col;
        if (i >= L || j >= L || (ti == tj && row > col)) continue;
        double s = 0.0;
        for (int k = 0; k < slabs; ++k) s += partial[((size_t)k * (size_t)ntri + (size_t)blockIdx.x) * 1024 + (size_t)e];
        G[(size_t)i * (size_t)L + (size_t)j] = s;
        G[(size_t)j * (size_t)L + (size_t)i] = s;
    }
}

namespace {

struct GramPlan {
    int block_tiles, tiles, slabs;
    size_t slab_chunks;
};
GramPlan gram_plan(size_t npix, int L)
{
    GramPlan q;
    const int nb = (L + kStrip - 1) / kStrip, n32 = (L + 31) / 32;
    q.block_tiles = nb * (nb + 1) / 2;
    q.tiles = n32 * (n32 + 1) / 2;
    const size_t chunks = (npix + (size_t)kChain - 1) / (size_t)kChain;
    size_t slabs = ((size_t)2 * kNumCU + (size_t)q.block_tiles - 1) / (size_t)q.block_tiles;  // two blocks for every CU
    if (slabs > chunks) slabs = chunks;
    if (slabs < 1) slabs = 1;
    q.slab_chunks = (chunks + slabs - 1) / slabs;
    if (q.slab_chunks < 1) q.slab_chunks = 1;
    q.slabs = (int)((chunks + q.slab_chunks - 1) / q.slab_chunks);
    if (q.slabs < 1) q.slabs = 1;
    return q;
}

}  // namespace

size_t pca_gram_mu_offset(int L) { return (size_t)L * (size_t)L * sizeof(double); }

size_t pca_gram_ws_bytes(size_t npix, int L)
{
    const GramPlan q = gram_plan(npix, L);
    return pca_gram_mu_offset(L) + kMuFloats * sizeof(float) + (size_t)q.slabs * (size_t)q.tiles * 1024 * sizeof(double);
}

void launch_pca_gram(hipStream_t st, const PcaView &v, void *ws)
{
    const GramPlan q = gram_plan(v.npix, v.L);
    unsigned char *base = static_cast<unsigned char *>(ws);
    double *G = reinterpret_cast<double *>(base);
    const float *mu = reinterpret_cast<const float *>(base + pca_gram_mu_offset(v.L));
    double *partial = reinterpret_cast<double *>(base + pca_gram_mu_offset(v.L) + kMuFloats * sizeof(float));
    THZ_LAUNCH(k_pca_gram, dim3((unsigned)q.block_tiles, (unsigned)q.slabs), 256, 0, st, v, mu, q.slab_chunks, partial);
    THZ_LAUNCH(k_pca_gram_fold, (unsigned)q.tiles, 256, 0, st, partial, q.slabs, v.L, G);
}

// ---------------------------------------------------------------- scores

// tab = [mu: L | V: K x L] goes into LDS once per block; the order of a pixel's sum depends on L alone
template <int K>
__global__ __launch_bounds__(256) void k_pca_scores(PcaView v, const float *__restrict__ tab, float *__restrict__ scores)
{
    THZ_DYN_LDS(lds);
    float *s_mu = reinterpret_cast<float *>(lds), *s_v = s_mu + v.L;
    for (int i = (int)threadIdx.x; i < (K + 1) * v.L; i += (int)blockDim.x) s_mu[i] = tab[i];
    __syncthreads();
    const int lane = lane_id();
    const int wib = (int)(threadIdx.x >> 6), wpb = (int)(blockDim.x >> 6);
    for (size_t p = (size_t)blockIdx.x * wpb + wib; p < v.npix; p += (size_t)gridDim.x * wpb) {
        const float *row = v.x + p * v.row_stride;
        float acc[K];
#pragma unroll
        for (int c = 0; c < K; ++c) acc[c] = 0.0f;
        for (int j = lane; j < v.L; j += kWave) {
            const float a = row[(size_t)j * v.col_step] - s_mu[j];
#pragma unroll
            for (int c = 0; c < K; ++c) acc[c] = __builtin_fmaf(a, s_v[c * v.L + j], acc[c]);
        }
#pragma unroll
        for (int c = 0; c < K; ++c) {
            const float s = wave_reduce_add(acc[c]);
            if (lane == 0) scores[(size_t)c * v.npix + p] = s;
        }
    }
}

void launch_pca_scores(hipStream_t st, const PcaView &v, const float *d_tab, int K, float *scores)
{
    const size_t blocks = (v.npix * kWave + 255) / 256;
    const unsigned grid = (unsigned)(blocks < 1 ? 1 : (blocks > (size_t)kNumCU * 8 ? (size_t)kNumCU * 8 : blocks));
    const size_t lds = (size_t)(K + 1) * (size_t)v.L * sizeof(float);
    switch (K) {
    case 1: THZ_LAUNCH(k_pca_scores<1>, grid, 256, lds, st, v, d_tab, scores); break;
    case 2: THZ_LAUNCH(k_pca_scores<2>, grid, 256, lds, st, v, d_tab, scores); break;
    case 3: THZ_LAUNCH(k_pca_scores<3>, grid, 256, lds, st, v, d_tab, scores); break;
    case 4: THZ_LAUNCH(k_pca_scores<4>, grid, 256, lds, st, v, d_tab, scores); break;
    case 5: THZ_LAUNCH(k_pca_scores<5>, grid, 256, lds, st, v, d_tab, scores); break;
    case 6: THZ_LAUNCH(k_pca_scores<6>, grid, 256, lds, st, v, d_tab, scores); break;
    case 7: THZ_LAUNCH(k_pca_scores<7>, grid, 256, lds, st, v, d_tab, scores); break;
    default: THZ_LAUNCH(k_pca_scores<8>, grid, 256, lds, st, v, d_tab, scores); break;
    }
}

}  // namespace thz
