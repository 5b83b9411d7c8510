// wavelet.hip — K23: translation-invariant wavelet shrinkage of every trace (undecimated transform with periodic
// extension, threshold from the median of the finest details).  include/thzgpu.h, "Denoising every trace", is the
// definition.
//
//   k_wavelet_denoise   one block of 256 threads per trace, one read of the cube from HBM and one write, whatever J: the
//                       ping-pong pair of approximations and the J planes of shrunk details live in LDS for the whole
//                       solve.  A thread owns the outputs i = tid, tid + 256, ...: per tap one sample from LDS feeds
//                       both analysis chains (two for the synthesis, one per plane), the taps sit in registers (the
//                       kernel is instantiated per tap count, its tap loops unrolled: no register array is indexed at
//                       run time), and the index walks the circle by one conditional subtraction.
//                       The median is a 4 x 8-bit radix select on the bit patterns of |d_1|: integer LDS atomics into
//                       256 bins, one bin per thread, a wave scan and the waves' totals — counts are order-free, so the
//                       same inputs give the same bits on every run.  No floating-point atomics.
//
// LDS image: plane q of a trace stands at words q nt .. q nt + nt - 1 behind 264 scratch words, unpadded.  At every
// level the 32 lanes of a half read a[(i + s k) mod N] for 32 consecutive i: 32 consecutive words, 32 different banks
// of the 32 a ds_read_b32 / ds_write_b32 has, whatever s and k.  Predicted conflicts per level: none, but for the one
// wave instruction per tap whose 32 outputs straddle the wrap (words N - c .. N - 1 and 0 .. 31 - c: 2-way on a few
// banks when N is no multiple of 32; at N = 1001 with 8 taps 263 LDS cycles where 256 are conflict-free, DESIGN.md
// 4.13).  The histogram's atomics conflict as the data's digits do.
//
// Every chain is ONE fmaf chain from +0 over ascending k — the order thz_host_wavelet_trace uses.  Built with
// -ffp-contract=off.
#include "wavelet.hpp"
#include "kernels.hpp"
#include "thz_device.hpp"

#include <math.h>

namespace thz {

namespace {

__device__ __forceinline__ float wv_shrink(float d, float th, int hard)
{
    const float t = fabsf(d) - th;
    const float soft = t > 0.0f ? copysignf(t, d) : 0.0f;
    const float kept = fabsf(d) > th ? d : 0.0f;
    return hard ? kept : soft;
}

}  // namespace

// LF = w.n_taps: the tap loops are unrolled and the taps stay in registers for the whole launch — vector ones: 32 scalars
// next to the loops' own are more than a wave has, and the compiler would park them in lanes of vector registers
template <int LF>
__global__ __launch_bounds__(kWaveletBlock) void k_wavelet_denoise(size_t npix, WaveletParams w, const float *data, float *out,
                                                                   float *__restrict__ sigma, int *__restrict__ kept)
{
    THZ_DYN_LDS(lds_raw);
    unsigned *hist = reinterpret_cast<unsigned *>(lds_raw);  // 256 bins
    unsigned *wsum = hist + 256;                              // the waves' totals
    unsigned *sel = hist + 260;                               // [the bits found so far | the rank among those that share them]
    unsigned *nkept = hist + 262;
    float *A = reinterpret_cast<float *>(hist + kWaveletScratchWords);
    const int tid = (int)threadIdx.x, lane = lane_id(), wave = tid / kWave;
    const int nt = w.nt, J = w.n_levels, hard = w.shrink;
    float *D = A + 2 * nt;
    float hn[LF], gn[LF];
#pragma unroll
    for (int k = 0; k < LF; ++k) {
        hn[k] = launder_f(w.hn[k]);
        gn[k] = launder_f(w.gn[k]);
    }
    for (size_t p = blockIdx.x; p < npix; p += gridDim.x) {
        const float *src = data + p * (size_t)nt;
        for (int i = tid; i < nt; i += kWaveletBlock) A[i] = src[i];
        if (tid == 0) *nkept = 0u;
        block_lds_barrier();
        float m = 0.0f, count = 0.0f;  // at most 108 a thread, 27648 a trace: exact
        for (int j = 1; j <= J; ++j) {
            const float *a = A + ((j - 1) & 1) * nt;
            float *an = A + (j & 1) * nt, *dj = D + (j - 1) * nt;
            const int step = (int)((1u << (j - 1)) % (unsigned)nt);
            const float th = w.noise_mode ? w.scale[j - 1] : w.scale[j - 1] * m;
            for (int i = tid; i < nt; i += kWaveletBlock) {
                float ah = 0.0f, ag = 0.0f;
                int idx = i;
#pragma unroll
                for (int k = 0; k < LF; ++k) {
                    const float v = a[idx];
                    ah = fmaf(hn[k], v, ah);
                    ag = fmaf(gn[k], v, ag);
                    idx += step;
                    idx = idx >= nt ? idx - nt : idx;
                }
                an[i] = ah;
                if (j > 1) {
                    ag = wv_shrink(ag, th, hard);
                    count += ag != 0.0f ? 1.0f : 0.0f;
                }
                dj[i] = ag;
            }
            block_lds_barrier();
            if (j > 1) continue;
            // the element of rank (nt - 1) / 2 of |d_1|, a digit of 8 bits per pass from the top
            unsigned prefix = 0u, rank = (unsigned)(nt - 1) / 2u;
            for (int pass = 0; pass < 4; ++pass) {
                const int shift = 24 - 8 * pass;
                const unsigned himask = pass ? 0xffffffffu << (shift + 8) : 0u;
                hist[tid] = 0u;
                block_lds_barrier();
                for (int i = tid; i < nt; i += kWaveletBlock) {
                    const unsigned b = abs_bits(dj[i]);
                    if ((b & himask) == prefix) atomicAdd(&hist[(b >> shift) & 255u], 1u);
                }
                block_lds_barrier();
                const unsigned c = hist[tid];
                unsigned incl = (unsigned)wave_scan_add((float)c);  // at most 4608: exact
                if (lane == kWave - 1) wsum[wave] = incl;
                block_lds_barrier();
                for (int q = 0; q < wave; ++q) incl += wsum[q];
                const unsigned excl = incl - c;
                if (excl <= rank && rank < incl) {  // one thread: the bins' counts add up to what the rank counts among
                    sel[0] = prefix | ((unsigned)tid << shift);
                    sel[1] = rank - excl;
                }
                block_lds_barrier();
                prefix = sel[0];
                rank = sel[1];
            }
            m = __builtin_bit_cast(float, prefix);
            if (sigma && tid == 0) sigma[p] = m;
            const float th1 = w.noise_mode ? w.scale[0] : w.scale[0] * m;
            for (int i = tid; i < nt; i += kWaveletBlock) {
                const float d = wv_shrink(dj[i], th1, hard);
                dj[i] = d;
                count += d != 0.0f ? 1.0f : 0.0f;
            }
            block_lds_barrier();
        }
        for (int j = J; j >= 1; --j) {
            const float *r = A + (j & 1) * nt, *dj = D + (j - 1) * nt;
            float *rn = A + ((j - 1) & 1) * nt;
            const int step = (int)((1u << (j - 1)) % (unsigned)nt);
            for (int i = tid; i < nt; i += kWaveletBlock) {
                float ch = 0.0f, cg = 0.0f;
                int idx = i;
#pragma unroll
                for (int k = 0; k < LF; ++k) {
                    ch = fmaf(hn[k], r[idx], ch);
                    cg = fmaf(gn[k], dj[idx], cg);
                    idx -= step;
                    idx = idx < 0 ? idx + nt : idx;
                }
                rn[i] = ch + cg;
            }
            block_lds_barrier();
        }
        float *dst = out + p * (size_t)nt;
        for (int i = tid; i < nt; i += kWaveletBlock) dst[i] = A[i];
        if (kept) {
            count = wave_reduce_add(count);
            if (lane == 0) atomicAdd(nkept, (unsigned)count);
        }
        block_lds_barrier();  // ... and A is free for the next trace
        if (kept && tid == 0) kept[p] = (int)*nkept;
    }
}

namespace {

typedef void (*WaveletKernel)(size_t, WaveletParams, const float *, float *, float *, int *);
const WaveletKernel kWaveletKernels[THZ_WAVELET_MAX_TAPS] = {
    k_wavelet_denoise<1>,  k_wavelet_denoise<2>,  k_wavelet_denoise<3>,  k_wavelet_denoise<4>,
    k_wavelet_denoise<5>,  k_wavelet_denoise<6>,  k_wavelet_denoise<7>,  k_wavelet_denoise<8>,
    k_wavelet_denoise<9>,  k_wavelet_denoise<10>, k_wavelet_denoise<11>, k_wavelet_denoise<12>,
    k_wavelet_denoise<13>, k_wavelet_denoise<14>, k_wavelet_denoise<15>, k_wavelet_denoise<16>};

}  // namespace

hipError_t launch_wavelet_denoise(hipStream_t st, size_t npix, const WaveletParams &w, const float *data, float *out,
                                  float *sigma, int32_t *kept)
{
    constexpr size_t kLdsPerCu = 160 * 1024;
    const size_t lds = wavelet_lds_bytes(w);
    if (w.nt < 1 || w.n_taps < 1 || w.n_taps > THZ_WAVELET_MAX_TAPS || lds > kLdsPerCu) return hipErrorInvalidValue;
    const WaveletKernel kernel = kWaveletKernels[w.n_taps - 1];
    if (lds > 64 * 1024) {  // beyond the default limit of a block's dynamic LDS
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    // as many blocks as a CU's LDS holds at once (in 2 KiB steps), at most eight: 32 waves
    size_t per_cu = kLdsPerCu / ((lds + 2047) & ~(size_t)2047);
    per_cu = per_cu < 1 ? 1 : (per_cu > 8 ? 8 : per_cu);
    const size_t most = (size_t)kNumCU * per_cu;
    const unsigned grid = (unsigned)(npix < most ? npix : most);
    THZ_LAUNCH(kernel, grid, kWaveletBlock, lds, st, npix, w, data, out, sigma, kept);
    return hipGetLastError();
}

}  // namespace thz
