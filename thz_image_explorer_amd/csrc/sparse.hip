// sparse.hip — K21: sparse deconvolution of every trace, y = h * x + noise with x sparse, by iterative shrinkage
// (ISTA, or FISTA with the host's momentum table).  include/thzgpu.h, "Sparse deconvolution", is the definition.
//
//   k_sparse_deconv   one wave per trace (a block IS a wave: no __syncthreads, no atomics), one read of the cube from HBM
//                     and one write, whatever n_iter: y, z, r and x of the trace live in LDS for the whole solve, z and
//                     r between zeros so that the tap loop tests no bound.  A lane owns 16 consecutive outputs of a chunk
//                     of 1024: 16 accumulators and a sliding window of samples, so a tap costs two ds_read_b32 (the
//                     sample that enters the window, once for each pairing), one tap from scalar memory and eight
//                     v_pk_fma_f32.
//
// LDS image: entry q of an array stands at word q + q / 16.  A lane's window starts at q = 16 (lane + b) + k, word
// 17 (lane + b) + k: the 32 lanes of a half read words 17 apart — 17 is odd, so they are 32 different banks of the 32 a
// ds_read_b32 has (bank = word % 32, counted per 32-lane half).  Predicted conflicts of the tap loop and of the own-entry
// accesses: none.  Only the strided fill and copy-out (word = e + e / 16, e consecutive over the lanes: lanes l and
// l + 30 .. 31 of a half meet) are 2-way, once per trace.
//
// Every sum is ONE fmaf chain from +0 in ascending order of the sample it reads — the order thz_host_sparse_trace uses,
// with zero taps and zero samples executed here and skipped there (the same value for finite data).  Built with
// -ffp-contract=off.
#include "sparse.hpp"
#include "kernels.hpp"
#include "thz_device.hpp"
#include "../../include/thzgpu.h"

#include <math.h>

namespace thz {

namespace {

constexpr int kSparseChunk = kSparseOut * kWave;  // outputs of one trip of the wave

__device__ __forceinline__ int sp_word(int q) { return q + (q >> 4); }

// Two outputs' chains go through one v_pk_fma_f32 (two independent fused multiply-adds: the bits of fmaf).  The
// instruction takes its operands from aligned register pairs, and a tap moves the window by ONE sample, so 16 entries of
// the window are kept twice: as the pairs (2k, 2k + 1) for the even taps and as the pairs (2k + 1, 2k + 2) for the odd
// ones, each read from LDS into place — left to the compiler, the odd pairs are made with a v_mov per fused multiply-add.
typedef float sp_f2 __attribute__((ext_vector_type(2)));
struct SpSeg {
    sp_f2 e[kSparseOut / 2], o[kSparseOut / 2];
};
// the 16 entries whose words start at p; the last odd pair ends with the next 16's first entry, one unused word further
__device__ __forceinline__ void sp_load(const float *p, SpSeg &s)
{
#pragma unroll
    for (int k = 0; k < kSparseOut / 2; ++k) {
        s.e[k] = sp_f2{p[2 * k], p[2 * k + 1]};
        s.o[k] = sp_f2{p[2 * k + 1], p[2 * k + 2 < kSparseOut ? 2 * k + 2 : kSparseOut + 1]};
    }
}
// 16 taps on the window a | b: acc[j] holds outputs 2j and 2j + 1, tap u reads entries u + 2j and u + 2j + 1
__device__ __forceinline__ void sp_block(const SpSeg &a, const SpSeg &b, const float *__restrict__ taps, sp_f2 (&acc)[kSparseOut / 2])
{
#pragma unroll
    for (int u = 0; u < kSparseOut; ++u) {
        const float h = taps[u];
#pragma unroll
        for (int j = 0; j < kSparseOut / 2; ++j) {
            const int k = u / 2 + j;
            const sp_f2 w = (u & 1) ? (k < kSparseOut / 2 ? a.o[k] : b.o[k - kSparseOut / 2])
                                    : (k < kSparseOut / 2 ? a.e[k] : b.e[k - kSparseOut / 2]);
            acc[j] = __builtin_elementwise_fma(sp_f2{h, h}, w, acc[j]);
        }
    }
}

// out[o] = taps[0] buf[q0 + o] + taps[1] buf[q0 + o + 1] + ... in that order, o = 0 .. 15; q0 and ntaps multiples of 16.
// Reads entries q0 .. q0 + ntaps + 16.  Two blocks of 16 taps per trip, the window's halves changing roles, so that no
// entry is moved between registers.
__device__ __forceinline__ void sp_product(const float *buf, int q0, const float *__restrict__ taps, int ntaps, float (&out)[kSparseOut])
{
    const float *p = buf + sp_word(q0);
    sp_f2 acc[kSparseOut / 2];
#pragma unroll
    for (int j = 0; j < kSparseOut / 2; ++j) acc[j] = sp_f2{0.0f, 0.0f};
    SpSeg s0, s1;
    sp_load(p, s0);
    int t0 = 0;
    for (; t0 + 2 * kSparseOut <= ntaps; t0 += 2 * kSparseOut) {
        sp_load(p + (kSparseOut + 1), s1);
        sp_block(s0, s1, taps + t0, acc);
        THZ_SCHED_FENCE();  // the second block's taps are fetched behind the first's products: 16 scalars in flight, not 32
        p += 2 * (kSparseOut + 1);
        sp_load(p, s0);
        sp_block(s1, s0, taps + t0 + kSparseOut, acc);
    }
    if (t0 < ntaps) {
        sp_load(p + (kSparseOut + 1), s1);
        sp_block(s0, s1, taps + t0, acc);
    }
#pragma unroll
    for (int j = 0; j < kSparseOut / 2; ++j) {
        out[2 * j] = acc[j].x;
        out[2 * j + 1] = acc[j].y;
    }
}

}  // namespace

__global__ __launch_bounds__(kWave) void k_sparse_deconv(size_t npix, SparseGeom g, const float *data,
                                                         const float *__restrict__ table, float *out,
                                                         float *__restrict__ resid, int *__restrict__ nnz)
{
    THZ_DYN_LDS(lds_raw);
    const int lane = lane_id();
    const int nt = g.nt, ntp = g.ntp, front = g.front;
    const int zw = g.len + (g.len >> 4), yw = ntp + (ntp >> 4);
    float *Z = reinterpret_cast<float *>(lds_raw);
    float *R = Z + zw;
    float *Y = R + zw;
    float *X = Y + yw;
    const float *taps_h = table, *taps_t = table + g.h_taps, *beta = table + g.h_taps + g.t_taps;
    // the zeros around z and r, once: nothing but the entries of samples 0 .. ntp - 1 is written afterwards
    for (int w = lane; w < 2 * zw; w += kWave) Z[w] = 0.0f;
    const int own = 17 * lane;  // sp_word(16 lane)
    for (size_t p = blockIdx.x; p < npix; p += gridDim.x) {
        const float *src = data + p * (size_t)nt;
        for (int e = lane; e < ntp; e += kWave) {
            const float v = e < nt ? src[e] : 0.0f;
            Y[sp_word(e)] = v;
            R[sp_word(front + e)] = v;
            Z[sp_word(front + e)] = 0.0f;
            X[sp_word(e)] = 0.0f;
        }
        wave_sync();
        // g0 = H^T y and the threshold
        float gm = 0.0f;
        for (int i0 = kSparseOut * lane; i0 < ntp; i0 += kSparseChunk) {
            float acc[kSparseOut];
            sp_product(R, i0 + 16 * g.t_block, taps_t, g.t_taps, acc);
#pragma unroll
            for (int o = 0; o < kSparseOut; ++o) gm = i0 + o < nt ? fmaxf(gm, fabsf(acc[o])) : gm;
        }
        const float gmax = __builtin_bit_cast(float, wave_reduce_max_u32(__builtin_bit_cast(unsigned, gm)));
        const float lam = fmaxf(g.rel_lambda * gmax, g.min_lambda);
        const float th = g.step * lam;
        wave_sync();
        for (int n = 0; n < g.n_iter; ++n) {
            // r = y - H z
            for (int i0 = kSparseOut * lane, cw = own; i0 < ntp; i0 += kSparseChunk, cw += 17 * kWave) {
                float acc[kSparseOut];
                sp_product(Z, i0 + 16 * g.h_block, taps_h, g.h_taps, acc);
                float *ro = R + sp_word(front) + cw;
                const float *yo = Y + cw;
#pragma unroll
                for (int o = 0; o < kSparseOut; ++o) ro[o] = i0 + o < nt ? yo[o] - acc[o] : 0.0f;
            }
            wave_sync();
            // x = shrink(z + step H^T r), z = x + beta (x - x before)
            const float b = g.accelerate ? beta[n] : 0.0f;
            for (int i0 = kSparseOut * lane, cw = own; i0 < ntp; i0 += kSparseChunk, cw += 17 * kWave) {
                float acc[kSparseOut];
                sp_product(R, i0 + 16 * g.t_block, taps_t, g.t_taps, acc);
                float *zo = Z + sp_word(front) + cw;
                float *xo = X + cw;
#pragma unroll
                for (int o = 0; o < kSparseOut; ++o) {
                    const float v = fmaf(g.step, acc[o], zo[o]);
                    const float a = fabsf(v) - th;
                    const float xn = (a > 0.0f && i0 + o < nt) ? copysignf(a, v) : 0.0f;
                    zo[o] = g.accelerate ? fmaf(b, xn - xo[o], xn) : xn;
                    xo[o] = xn;
                }
            }
            wave_sync();
        }
        float *dst = out + p * (size_t)nt;
        float count = 0.0f;  // at most 72 a lane, 4608 a trace: exact
        for (int e = lane; e < nt; e += kWave) {
            const float v = X[sp_word(e)];
            dst[e] = v;
            count += v != 0.0f ? 1.0f : 0.0f;
        }
        if (nnz) {
            count = wave_reduce_add(count);
            if (lane == 0) nnz[p] = (int)count;
        }
        if (resid) {
            // sum of (y - H x)^2: x between z's zeros, one more product
            for (int e = lane; e < ntp; e += kWave) Z[sp_word(front + e)] = X[sp_word(e)];
            wave_sync();
            float s = 0.0f;
            for (int i0 = kSparseOut * lane, cw = own; i0 < ntp; i0 += kSparseChunk, cw += 17 * kWave) {
                float acc[kSparseOut];
                sp_product(Z, i0 + 16 * g.h_block, taps_h, g.h_taps, acc);
                const float *yo = Y + cw;
#pragma unroll
                for (int o = 0; o < kSparseOut; ++o) {
                    const float d = yo[o] - acc[o];
                    s = i0 + o < nt ? fmaf(d, d, s) : s;
                }
            }
            s = wave_reduce_add(s);
            if (lane == 0) resid[p] = s;
        }
        wave_sync();
    }
}

bool sparse_geom(int nt, int P, int c, int n_iter, int accelerate, float step, float rel_lambda, float min_lambda, SparseGeom *g)
{
    if (nt < 1 || nt > THZ_SPARSE_MAX_NT || P < 1 || P > THZ_SPARSE_MAX_TAPS || c < 0 || c >= P || n_iter < 0 || n_iter > THZ_SPARSE_MAX_ITER)
        return false;
    g->nt = nt;
    g->ntp = sparse_up16(nt);
    g->front = sparse_up16(P - 1);
    g->len = g->front + g->ntp + sparse_up16(P + 15) + 16;
    const int shift_h = g->front + c - (P - 1), shift_t = g->front - c;  // entry of the first sample output 0 reads
    g->h_block = shift_h / 16;
    g->h_taps = sparse_up16(P + shift_h % 16);
    g->t_block = shift_t / 16;
    g->t_taps = sparse_up16(P + shift_t % 16);
    g->n_iter = n_iter;
    g->accelerate = accelerate;
    g->step = step;
    g->rel_lambda = rel_lambda;
    g->min_lambda = min_lambda;
    // the last entry a product reads: the last chunk's window start, its taps, and the first entry behind the 16 loaded
    // behind them
    const int last_h = g->ntp - 16 + 16 * g->h_block + g->h_taps + 16, last_t = g->ntp - 16 + 16 * g->t_block + g->t_taps + 16;
    return shift_h >= 0 && shift_t >= 0 && last_h < g->len && last_t < g->len;
}

void sparse_fill_table(const SparseGeom &g, const float *taps, int P, int c, float *table)
{
    const int lead_h = (g.front + c - (P - 1)) % 16, lead_t = (g.front - c) % 16;
    for (int t = 0; t < g.h_taps + g.t_taps; ++t) table[t] = 0.0f;
    for (int k = 0; k < P; ++k) {
        table[lead_h + k] = taps[P - 1 - k];
        table[g.h_taps + lead_t + k] = taps[k];
    }
    sparse_momentum(g.n_iter, table + g.h_taps + g.t_taps);
}

size_t sparse_lds_bytes(const SparseGeom &g)
{
    return sizeof(float) * (2 * (size_t)(g.len + g.len / 16) + 2 * (size_t)(g.ntp + g.ntp / 16));
}

hipError_t launch_sparse_deconv(hipStream_t st, size_t npix, const SparseGeom &g, const float *data, const float *table,
                                float *out, float *resid, int32_t *nnz)
{
    constexpr size_t kLdsPerCu = 160 * 1024;
    const size_t lds = sparse_lds_bytes(g);
    if (lds > kLdsPerCu) return hipErrorInvalidValue;
    if (lds > 64 * 1024) {  // beyond the default limit of a block's dynamic LDS
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k_sparse_deconv),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    // as many waves as a CU's LDS holds at once (in 2 KiB steps), at most four per SIMD
    size_t per_cu = kLdsPerCu / ((lds + 2047) & ~(size_t)2047);
    per_cu = per_cu < 1 ? 1 : (per_cu > 16 ? 16 : per_cu);
    const size_t most = (size_t)kNumCU * per_cu;
    const unsigned grid = (unsigned)(npix < most ? npix : most);
    THZ_LAUNCH(k_sparse_deconv, grid, kWave, lds, st, npix, g, data, table, out, resid, nnz);
    return hipGetLastError();
}

}  // namespace thz
