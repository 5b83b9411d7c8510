// peak.hip — K16: when the pulse arrives at each pixel, and the plane through those arrival times.
//
//   k_peak_map        per trace: position of the extreme sample (largest |x|, maximum or minimum), its signed value
//                     and the sub-sample vertex of the parabola through it and its two neighbours
//                     (HBM: 4 nt B/trace, the traffic of k_intensity; one wave per trace like it)
//   k_plane_vmax / k_plane_moments / k_plane_finish
//                     the ten weighted sums of a least-squares plane tau(u, v) over the three images, in double, on a
//                     launch geometry that depends on nothing: the same images give the same ten doubles on every run
//                     and on every device
//
// Built with -ffp-contract=off: the parabola's offset is the f32 formula as written, one rounding per operation.
#include "peak.hpp"
#include "kernels.hpp"
#include "thz_device.hpp"
#include "fft_f.hpp"  // load_f4: a 16-byte load that promises 4-byte alignment only

#include <math.h>

namespace thz {

// kPeakBatch: 16-byte loads a lane has in flight before it looks at the first.  Measured at 1, 2, 4, 8 and 16 on
// 512 x 512 x 1001 and 1024 x 1024 x 4096 (profiles/peak_map_timing.txt): 2 is the fastest or level with the fastest at
// both; larger batches cost registers and, on short traces, loads of the last quad over again.
template <int MODE, int kPeakBatch>
__global__ __launch_bounds__(256) void k_peak_map(size_t npix, int nt, const float *__restrict__ data,
                                                  int *__restrict__ index, float *__restrict__ offset,
                                                  float *__restrict__ value)
{
    const int lane = lane_id();
    const int wib = (int)(threadIdx.x >> 6);
    const int wpb = (int)(blockDim.x >> 6);
    const int nt4 = nt & ~3;
    for (size_t p = (size_t)blockIdx.x * wpb + wib; p < npix; p += (size_t)gridDim.x * wpb) {
        const float *x = data + p * (size_t)nt;
        float best = -INFINITY;
        int best_i = -1;
        for (int e0 = 4 * lane; e0 < nt4; e0 += 4 * kWave * kPeakBatch) {
            // A quad behind the trace's last whole one is read as that last quad again, under its true indices: a
            // sample met twice changes nothing (its key is not above itself), so no load waits for a branch.
            float4 v[kPeakBatch];
            int at[kPeakBatch];
#pragma unroll
            for (int u = 0; u < kPeakBatch; ++u) {
                const int e = e0 + 4 * kWave * u;
                at[u] = e < nt4 ? e : nt4 - 4;
                load_f4(x + at[u], v[u].x, v[u].y, v[u].z, v[u].w);
            }
#pragma unroll
            for (int u = 0; u < kPeakBatch; ++u) {
                peak_take<MODE>(v[u].x, at[u], best, best_i);
                peak_take<MODE>(v[u].y, at[u] + 1, best, best_i);
                peak_take<MODE>(v[u].z, at[u] + 2, best, best_i);
                peak_take<MODE>(v[u].w, at[u] + 3, best, best_i);
            }
        }
        // the nt % 4 samples behind the last whole quad: above every index the lane has seen
        if (nt4 + lane < nt) peak_take<MODE>(x[nt4 + lane], nt4 + lane, best, best_i);
        int k = peak_wave_winner(best, best_i);
        if (k < 0) k = peak_first_number<MODE>(x, nt, lane);  // (wave-uniform, cold) no key above -Inf
        if (lane == 0) {
            float y0;
            const float off = peak_vertex(x, k, nt, y0);
            if (index) index[p] = k;
            if (offset) offset[p] = off;
            if (value) value[p] = y0;
        }
    }
}

// ---- arrival-plane moments.  kPlaneBlocks x kPlaneThreads threads, pixel p belongs to thread p mod (blocks x
// threads) and is added in ascending p; lanes, waves and blocks are then added as fixed trees.
constexpr int kPlaneBlocks = 64, kPlaneThreads = 256, kPlaneSums = 10;

__device__ __forceinline__ bool plane_finite(float v) { return abs_bits(v) < 0x7f800000u; }

__device__ __forceinline__ unsigned plane_wave_max(unsigned v)
{
    for (int m = 1; m < kWave; m <<= 1) v = umax(v, (unsigned)__shfl_xor((int)v, m, kWave));
    return v;
}

// pass 1: per block the largest finite |value|, as its bits (the unsigned order of |float| bits is the floats')
__global__ __launch_bounds__(kPlaneThreads) void k_plane_vmax(size_t npix, const float *__restrict__ value,
                                                              unsigned *__restrict__ block_max)
{
    __shared__ unsigned s_max[kPlaneThreads / kWave];
    unsigned m = 0u;
    for (size_t p = (size_t)blockIdx.x * kPlaneThreads + threadIdx.x; p < npix; p += (size_t)kPlaneBlocks * kPlaneThreads) {
        const float v = value[p];
        if (plane_finite(v)) m = umax(m, abs_bits(v));
    }
    m = plane_wave_max(m);
    if (lane_id() == 0) s_max[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kPlaneThreads / kWave; ++w) m = umax(m, s_max[w]);
        block_max[blockIdx.x] = m;
    }
}

// pass 2: per block the ten sums over its pixels with |value| finite and >= rel_threshold * vmax (f32 product and
// compare): 1, u, v, uu, uv, vv, t, ut, vt, tt with u = (i - nx / 2) dx, v = (j - ny / 2) dy, t = (index + offset) dt
__global__ __launch_bounds__(kPlaneThreads) void k_plane_moments(size_t nx, size_t ny, double dx, double dy, double dt,
                                                                 const int *__restrict__ index,
                                                                 const float *__restrict__ offset,
                                                                 const float *__restrict__ value, float rel_threshold,
                                                                 const unsigned *__restrict__ block_max,
                                                                 double *__restrict__ block_sums)
{
    __shared__ double s_sum[kPlaneThreads / kWave][kPlaneSums];
    unsigned vm = block_max[lane_id()];  // kPlaneBlocks == kWave: one block maximum per lane
    vm = plane_wave_max(vm);
    const float thr = rel_threshold * __builtin_bit_cast(float, vm);
    const double cx = (double)nx / 2.0, cy = (double)ny / 2.0;
    double a[kPlaneSums];
#pragma unroll
    for (int q = 0; q < kPlaneSums; ++q) a[q] = 0.0;
    const size_t npix = nx * ny;
    for (size_t p = (size_t)blockIdx.x * kPlaneThreads + threadIdx.x; p < npix; p += (size_t)kPlaneBlocks * kPlaneThreads) {
        const float val = value[p];
        if (!(plane_finite(val) && fabsf(val) >= thr)) continue;
        const double u = ((double)(p / ny) - cx) * dx, v = ((double)(p % ny) - cy) * dy;
        const double t = ((double)index[p] + (double)offset[p]) * dt;
        a[0] += 1.0;
        a[1] += u;
        a[2] += v;
        a[3] += u * u;
        a[4] += u * v;
        a[5] += v * v;
        a[6] += t;
        a[7] += u * t;
        a[8] += v * t;
        a[9] += t * t;
    }
#pragma unroll
    for (int q = 0; q < kPlaneSums; ++q)
        for (int m = 1; m < kWave; m <<= 1) a[q] += __shfl_xor(a[q], m, kWave);  // a + b = b + a: every lane the same sum
    if (lane_id() == 0)
#pragma unroll
        for (int q = 0; q < kPlaneSums; ++q) s_sum[threadIdx.x >> 6][q] = a[q];
    __syncthreads();
    if (threadIdx.x < kPlaneSums) {
        double t = s_sum[0][threadIdx.x];
        for (int w = 1; w < kPlaneThreads / kWave; ++w) t += s_sum[w][threadIdx.x];
        block_sums[(size_t)blockIdx.x * kPlaneSums + threadIdx.x] = t;
    }
}

// pass 3 (one wave): the blocks' rows, one per lane, added as the same butterfly
__global__ __launch_bounds__(kWave) void k_plane_finish(const double *__restrict__ block_sums, double *__restrict__ out)
{
    static_assert(kPlaneBlocks == kWave, "one block row per lane");
    for (int q = 0; q < kPlaneSums; ++q) {
        double t = block_sums[(size_t)lane_id() * kPlaneSums + q];
        for (int m = 1; m < kWave; m <<= 1) t += __shfl_xor(t, m, kWave);
        if (lane_id() == 0) out[q] = t;
    }
}

void launch_peak_map(hipStream_t st, size_t npix, int nt, const float *data, int mode, int *index, float *offset,
                     float *value)
{
    const size_t blocks = (npix * kWave + 255) / 256;
    const unsigned grid = (unsigned)(blocks < 1 ? 1 : (blocks > (size_t)kNumCU * 8 ? (size_t)kNumCU * 8 : blocks));
#define THZ_PEAK(M) THZ_LAUNCH((k_peak_map<M, 2>), grid, 256, 0, st, npix, nt, data, index, offset, value)
    switch (mode) {
    case 0: THZ_PEAK(0); break;
    case 1: THZ_PEAK(1); break;
    default: THZ_PEAK(2); break;
    }
#undef THZ_PEAK
}

size_t plane_moments_ws_bytes() { return (size_t)kPlaneBlocks * (kPlaneSums + 1) * sizeof(double) + kPlaneSums * sizeof(double); }

void launch_plane_moments(hipStream_t st, size_t nx, size_t ny, double dx, double dy, double dt, const int *index,
                          const float *offset, const float *value, float rel_threshold, void *ws)
{
    double *out = static_cast<double *>(ws);                 // [10] the result
    double *block_sums = out + kPlaneSums;                   // [blocks][10]
    unsigned *block_max = reinterpret_cast<unsigned *>(block_sums + (size_t)kPlaneBlocks * kPlaneSums);  // [blocks]
    THZ_LAUNCH(k_plane_vmax, kPlaneBlocks, kPlaneThreads, 0, st, nx * ny, value, block_max);
    THZ_LAUNCH(k_plane_moments, kPlaneBlocks, kPlaneThreads, 0, st, nx, ny, dx, dy, dt, index, offset, value, rel_threshold,
               block_max, block_sums);
    THZ_LAUNCH(k_plane_finish, 1, kWave, 0, st, block_sums, out);
}

}  // namespace thz
