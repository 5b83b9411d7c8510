// unmix.hip — K22: non-negative least squares of every pixel's row against K endmembers on the
// strided (npix x L) view of pca.hpp.
//
//   k_unmix_project  one wave per pixel, E (and lref) in LDS once per block: lane l adds fmaf(u, E[c, j], acc[c]) over
//                    j = l, l + 64, ... for its K accumulators, and the lanes are added as k_pca_scores adds them — the
//                    order depends on L alone.  Lane 0 stores.
//   k_unmix_solve    one lane per pixel: the solve is n_sweeps K (K + 3) dependent operations that every lane of a
//                    wave-per-pixel kernel would repeat.  b is read coalesced from the endmember-major plane, Gt and rd
//                    sit in LDS (every lane reads the same address: a broadcast), a[K] and g[K] in registers — K is a
//                    template parameter and every loop over c and i fully unrolled, so no register array is indexed
//                    at run time.  A wave whose last full sweep changed no lane's a stops: the remaining sweeps would
//                    repeat it.
//   k_unmix_resid    one wave per pixel, the pixel's K abundances read uniformly: the second pass over the row
//
// No atomics: the same inputs give the same bits on every run.
#include "unmix.hpp"
#include "kernels.hpp"
#include "thz_device.hpp"

#include "../../include/thzgpu.h"

namespace thz {

namespace {

// the element both passes over the row see: one f32 subtraction of the library's logf from the host's (float)log(ref)
__device__ __forceinline__ float unmix_element(float x, float lref, bool absorbance) { return absorbance ? lref - logf(x) : x; }

}  // namespace

// ---------------------------------------------------------------- projection

// tab = [E: K x L | lref: L] goes into LDS once per block
template <int K>
__global__ __launch_bounds__(512) void k_unmix_project(PcaView v, const float *__restrict__ tab, int absorbance, float *__restrict__ proj)
{
    THZ_DYN_LDS(lds);
    float *s_e = reinterpret_cast<float *>(lds), *s_lref = s_e + K * v.L;
    for (int i = (int)threadIdx.x; i < (K + 1) * v.L; i += (int)blockDim.x) s_e[i] = tab[i];
    __syncthreads();
    const int lane = lane_id();
    const int wib = (int)(threadIdx.x >> 6), wpb = (int)(blockDim.x >> 6);
    const bool absorb = absorbance != 0;
    for (size_t p = (size_t)blockIdx.x * wpb + wib; p < v.npix; p += (size_t)gridDim.x * wpb) {
        const float *row = v.x + p * v.row_stride;
        float acc[K];
#pragma unroll
        for (int c = 0; c < K; ++c) acc[c] = 0.0f;
        for (int j = lane; j < v.L; j += kWave) {
            const float u = unmix_element(row[(size_t)j * v.col_step], s_lref[j], absorb);
#pragma unroll
            for (int c = 0; c < K; ++c) acc[c] = __builtin_fmaf(u, s_e[c * v.L + j], acc[c]);
        }
#pragma unroll
        for (int c = 0; c < K; ++c) {
            const float s = wave_reduce_add(acc[c]);
            if (lane == 0) proj[(size_t)c * v.npix + p] = s;
        }
    }
}

// ---------------------------------------------------------------- solve

// tab = [Gt: K x K | rd: K]
template <int K>
__global__ __launch_bounds__(256) void k_unmix_solve(size_t npix, const float *__restrict__ tab, int n_sweeps, const float *__restrict__ proj,
                                                     float *__restrict__ abund, float *__restrict__ kkt)
{
    __shared__ float s_gt[K * K + K];
    for (int i = (int)threadIdx.x; i < K * K + K; i += (int)blockDim.x) s_gt[i] = tab[i];
    __syncthreads();
    const float *s_rd = s_gt + K * K;
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool on = p < npix;  // a lane beyond the last pixel solves b = 0: nothing moves, nothing is stored
    float a[K], g[K];
#pragma unroll
    for (int c = 0; c < K; ++c) {
        a[c] = 0.0f;
        g[c] = -(on ? proj[(size_t)c * npix + p] : 0.0f);
    }
    for (int s = 0; s < n_sweeps; ++s) {
        bool moved = false;
#pragma unroll
        for (int c = 0; c < K; ++c) {
            const float an = fmaxf(__builtin_fmaf(-g[c], s_rd[c], a[c]), 0.0f);
            const float d = an - a[c];
            moved = moved || d != 0.0f;
#pragma unroll
            for (int i = 0; i < K; ++i) g[i] = __builtin_fmaf(s_gt[c * K + i], d, g[i]);
            a[c] = an;
        }
        if (!wave_any(moved)) break;
    }
    if (!on) return;
    float worst = 0.0f;
#pragma unroll
    for (int c = 0; c < K; ++c) {
        worst = fmaxf(worst, a[c] > 0.0f ? fabsf(g[c]) : fmaxf(-g[c], 0.0f));
        abund[(size_t)c * npix + p] = a[c];
    }
    if (kkt) kkt[p] = worst;
}

// ---------------------------------------------------------------- residual

template <int K>
__global__ __launch_bounds__(512) void k_unmix_resid(PcaView v, const float *__restrict__ tab, int absorbance, const float *__restrict__ abund,
                                                     float *__restrict__ resid)
{
    THZ_DYN_LDS(lds);
    float *s_e = reinterpret_cast<float *>(lds), *s_lref = s_e + K * v.L;
    for (int i = (int)threadIdx.x; i < (K + 1) * v.L; i += (int)blockDim.x) s_e[i] = tab[i];
    __syncthreads();
    const int lane = lane_id();
    const int wib = THZ_UNIFORM((int)(threadIdx.x >> 6)), wpb = (int)(blockDim.x >> 6);
    const bool absorb = absorbance != 0;
    for (size_t p = (size_t)blockIdx.x * wpb + wib; p < v.npix; p += (size_t)gridDim.x * wpb) {
        const float *row = v.x + p * v.row_stride;
        float a[K];
#pragma unroll
        for (int c = 0; c < K; ++c) a[c] = abund[(size_t)c * v.npix + p];
        float acc = 0.0f;
        for (int j = lane; j < v.L; j += kWave) {
            const float u = unmix_element(row[(size_t)j * v.col_step], s_lref[j], absorb);
            float m = 0.0f;
#pragma unroll
            for (int c = 0; c < K; ++c) m = __builtin_fmaf(a[c], s_e[c * v.L + j], m);
            const float r = u - m;
            acc = __builtin_fmaf(r, r, acc);
        }
        const float s = wave_reduce_add(acc);
        if (lane == 0) resid[p] = s;
    }
}

// ---------------------------------------------------------------- launches

namespace {

// The two wave-per-pixel kernels run blocks of 512 threads: eight waves share one LDS image of E, so that at K = 16
// (34 KiB) four blocks still fill a CU's 32 wave slots — with 256 threads the image's size held a CU at 16 waves and
// the K = 16 passes ran a third slower.  8192 pixels per trip of the grid, as k_pca_scores.
constexpr int kRowBlock = 512;
unsigned wave_per_pixel_grid(size_t npix)
{
    const size_t blocks = (npix * kWave + kRowBlock - 1) / kRowBlock;
    return (unsigned)(blocks < 1 ? 1 : (blocks > (size_t)kNumCU * 4 ? (size_t)kNumCU * 4 : blocks));
}

}  // namespace

// one case per K: the kernels keep K values in registers, indexed at compile time
#define THZ_UNMIX_EACH_K(X) \
    X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) X(14) X(15) X(16)

void launch_unmix_project(hipStream_t st, const PcaView &v, const UnmixTable &t, int K, bool absorbance, float *proj)
{
    const unsigned grid = wave_per_pixel_grid(v.npix);
    const size_t lds = (size_t)(K + 1) * (size_t)v.L * sizeof(float);
    switch (K) {
#define THZ_UNMIX_CASE(k) \
    case k: THZ_LAUNCH(k_unmix_project<k>, grid, kRowBlock, lds, st, v, t.e, (int)absorbance, proj); break;
        THZ_UNMIX_EACH_K(THZ_UNMIX_CASE)
#undef THZ_UNMIX_CASE
    default: break;
    }
}

void launch_unmix_solve(hipStream_t st, size_t npix, const UnmixTable &t, int K, int n_sweeps, const float *proj, float *abund, float *kkt)
{
    const unsigned grid = (unsigned)((npix + 255) / 256);
    switch (K) {
#define THZ_UNMIX_CASE(k) \
    case k: THZ_LAUNCH(k_unmix_solve<k>, grid, 256, 0, st, npix, t.gt, n_sweeps, proj, abund, kkt); break;
        THZ_UNMIX_EACH_K(THZ_UNMIX_CASE)
#undef THZ_UNMIX_CASE
    default: break;
    }
}

void launch_unmix_resid(hipStream_t st, const PcaView &v, const UnmixTable &t, int K, bool absorbance, const float *abund, float *resid)
{
    const unsigned grid = wave_per_pixel_grid(v.npix);
    const size_t lds = (size_t)(K + 1) * (size_t)v.L * sizeof(float);
    switch (K) {
#define THZ_UNMIX_CASE(k) \
    case k: THZ_LAUNCH(k_unmix_resid<k>, grid, kRowBlock, lds, st, v, t.e, (int)absorbance, abund, resid); break;
        THZ_UNMIX_EACH_K(THZ_UNMIX_CASE)
#undef THZ_UNMIX_CASE
    default: break;
    }
}

}  // namespace thz
