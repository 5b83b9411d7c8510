// cluster.hip — K20: k-means of the pixels of a scan on the strided (npix x L) view of pca.hpp.
//
//   k_cluster_assign  one wave per pixel, the K x L centroids in LDS: a lane keeps its at most 8 values of the row in
//                     registers (the row is read once), adds fmaf(d, d, acc) with d = x - m over j = lane, lane + 64,
//                     ... for one centroid after the other, and the lanes are added as k_pca_scores adds them — the
//                     order depends on L alone.  Label: the lowest c with the smallest distance, a NaN never wins.
//                     Lane 0 reads the label that is there, counts the change and writes label and distance; the
//                     wave's count goes into one integer atomic at its end.
//   k_cluster_sums    k_pca_sums with one f64 accumulator per cluster, chosen by compare-select: thread (r, c) adds
//                     column c of the pixels p0 + r, p0 + r + rows, ... of its slab; column L is a column of ones
//   k_cluster_stats   per slab: the sum of dist2 in f64 and the largest finite dist2 with the lowest index
//   k_cluster_fold    adds the slabs' partials in a fixed order: runs of slabs in slab order, then the runs in order
//
// No floating-point atomics: the same inputs give the same bits on every run.
#include "cluster.hpp"
#include "kernels.hpp"
#include "thz_device.hpp"

#include "../../include/thzgpu.h"

namespace thz {

namespace {

__device__ __forceinline__ bool pixel_on(const PcaView &v, size_t p) { return !v.mask || v.mask[p] != 0; }

}  // namespace

// ---------------------------------------------------------------- assign

// NJ = ceil(L / 64): the row values a lane holds
template <int NJ>
__global__ __launch_bounds__(256) void k_cluster_assign(PcaView v, const float *__restrict__ cent, int K, int32_t *__restrict__ label,
                                                        float *__restrict__ dist2, unsigned long long *__restrict__ changed)
{
    THZ_DYN_LDS(lds);
    float *s_m = reinterpret_cast<float *>(lds);
    for (int i = (int)threadIdx.x; i < K * v.L; i += (int)blockDim.x) s_m[i] = cent[i];
    __syncthreads();
    const int lane = lane_id();
    const int wib = (int)(threadIdx.x >> 6), wpb = (int)(blockDim.x >> 6);
    unsigned moved = 0;
    for (size_t p = (size_t)blockIdx.x * wpb + wib; p < v.npix; p += (size_t)gridDim.x * wpb) {
        const float *row = v.x + p * v.row_stride;
        float x[NJ];
#pragma unroll
        for (int u = 0; u < NJ; ++u) {
            const int j = lane + u * kWave;
            x[u] = j < v.L ? row[(size_t)j * v.col_step] : 0.0f;
        }
        float best = 0.0f;
        int lab = -1;
        for (int c = 0; c < K; ++c) {
            const float *m = s_m + c * v.L;
            float acc = 0.0f;
#pragma unroll
            for (int u = 0; u < NJ; ++u) {
                const int j = lane + u * kWave;
                if (j < v.L) {
                    const float d = x[u] - m[j];
                    acc = __builtin_fmaf(d, d, acc);
                }
            }
            const float s = wave_reduce_add(acc);
            if (lab < 0 ? s == s : s < best) {  // the first that is no NaN, then only a smaller one
                best = s;
                lab = c;
            }
        }
        if (lane == 0) {
            moved += label[p] != lab ? 1u : 0u;
            label[p] = lab;
            dist2[p] = lab < 0 ? __builtin_nanf("") : best;
        }
    }
    if (lane == 0 && moved) atomicAdd(changed, (unsigned long long)moved);
}

// ---------------------------------------------------------------- per-cluster sums

// blockDim 256 = rows x cw threads (cw: the power of two >= L + 1, at most 256), KC >= K accumulators per thread.
// partial: [slab][cluster][L + 1]
template <int KC>
__global__ __launch_bounds__(256) void k_cluster_sums(PcaView v, const int32_t *__restrict__ label, int K, int cw, size_t slab_pix,
                                                      double *__restrict__ partial)
{
    __shared__ double red[256];
    const int n = v.L + 1;
    const int rows = 256 / cw;
    const int c = (int)blockIdx.x * cw + (int)(threadIdx.x % cw), r = (int)(threadIdx.x / cw);
    const size_t p0 = (size_t)blockIdx.y * slab_pix;
    const size_t p1 = p0 + slab_pix < v.npix ? p0 + slab_pix : v.npix;
    const bool ones = c == v.L;
    const float *col = v.x + (size_t)(c < v.L ? c : 0) * v.col_step;
    double s[KC];
#pragma unroll
    for (int k = 0; k < KC; ++k) s[k] = 0.0;
    if (c < n) {
        const size_t step = (size_t)rows;
        for (size_t p = p0 + (size_t)r; p < p1; p += 4 * step) {
            float x[4];
            int lab[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const size_t pu = p + (size_t)u * step;
                x[u] = 0.0f;
                lab[u] = -1;
                if (pu < p1) {
                    x[u] = ones ? 1.0f : col[pu * v.row_stride];
                    lab[u] = pixel_on(v, pu) ? label[pu] : -1;
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int k = 0; k < KC; ++k) s[k] += lab[u] == k ? (double)x[u] : 0.0;
        }
    }
#pragma unroll
    for (int k = 0; k < KC; ++k) {
        __syncthreads();
        red[threadIdx.x] = s[k];
        __syncthreads();
        if (r == 0 && c < n && k < K) {
            double t = 0.0;
            for (int q = 0; q < rows; ++q) t += red[q * cw + (int)(threadIdx.x % cw)];
            partial[((size_t)blockIdx.y * (size_t)K + (size_t)k) * (size_t)n + (size_t)c] = t;
        }
    }
}

// One block per slab.  partial: [slab][inertia | largest finite dist2, -1 for none | its index, npix for none]
__global__ __launch_bounds__(256) void k_cluster_stats(size_t npix, const uint8_t *__restrict__ mask, const int32_t *__restrict__ label,
                                                       const float *__restrict__ dist2, size_t slab_pix, double *__restrict__ partial)
{
    __shared__ double r_sum[256];
    __shared__ float r_val[256];
    __shared__ unsigned long long r_idx[256];
    const size_t p0 = (size_t)blockIdx.x * slab_pix;
    const size_t p1 = p0 + slab_pix < npix ? p0 + slab_pix : npix;
    double sum = 0.0;
    float val = -1.0f;
    unsigned long long idx = npix;
    for (size_t p = p0 + threadIdx.x; p < p1; p += 256) {
        if ((mask && mask[p] == 0) || label[p] < 0) continue;
        const float d = dist2[p];
        sum += (double)d;
        if (d > val && d < __builtin_inff()) {  // ascending p: the first of equal ones stays
            val = d;
            idx = p;
        }
    }
    const int t = (int)threadIdx.x;
    r_sum[t] = sum;
    r_val[t] = val;
    r_idx[t] = idx;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (t < h) {
            r_sum[t] += r_sum[t + h];
            const float bv = r_val[t + h];
            const unsigned long long bi = r_idx[t + h];
            if (bv > r_val[t] || (bv == r_val[t] && bi < r_idx[t])) {
                r_val[t] = bv;
                r_idx[t] = bi;
            }
        }
        __syncthreads();
    }
    if (t == 0) {
        partial[3 * (size_t)blockIdx.x] = r_sum[0];
        partial[3 * (size_t)blockIdx.x + 1] = (double)r_val[0];
        partial[3 * (size_t)blockIdx.x + 2] = (double)r_idx[0];
    }
}

// blockDim 256 = 32 groups of slabs x 8 entries.  Block b < ceil(n / 8): entries 8 b .. 8 b + 7 of out — group g adds
// its run of consecutive slabs in slab order, four accumulators deep, and the groups are added in group order (the
// order depends on the number of slabs alone).  The block behind them: the inertia and the farthest pixel, thread t
// taking the slabs t, t + 256, ... and the threads the tree of k_cluster_stats.
__global__ __launch_bounds__(256) void k_cluster_fold(const double *__restrict__ psum, int slabs, int n, const double *__restrict__ pstat,
                                                      int stat_slabs, size_t npix, double *__restrict__ out)
{
    __shared__ double r_sum[256], r_val[256], r_idx[256];
    const int t = (int)threadIdx.x;
    if ((int)blockIdx.x * 8 < n) {
        const int el = t & 7, g = t >> 3;
        const int e = (int)blockIdx.x * 8 + el;
        const int per = (slabs + 31) / 32;
        const int s0 = g * per, s1 = s0 + per < slabs ? s0 + per : slabs;
        double a[4] = {0.0, 0.0, 0.0, 0.0};
        if (e < n) {
            for (int s = s0; s < s1; s += 4) {
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (s + u < s1) a[u] += psum[(size_t)(s + u) * (size_t)n + (size_t)e];
            }
        }
        r_sum[t] = (a[0] + a[1]) + (a[2] + a[3]);
        __syncthreads();
        if (g == 0 && e < n) {
            double r = 0.0;
            for (int q = 0; q < 32; ++q) r += r_sum[q * 8 + el];
            out[e] = r;
        }
        return;
    }
    double inertia = 0.0, val = -1.0, idx = (double)npix;
    for (int s = t; s < stat_slabs; s += 256) {
        inertia += pstat[3 * (size_t)s];
        if (pstat[3 * (size_t)s + 1] > val) {  // ascending slabs: the first of equal ones stays
            val = pstat[3 * (size_t)s + 1];
            idx = pstat[3 * (size_t)s + 2];
        }
    }
    r_sum[t] = inertia;
    r_val[t] = val;
    r_idx[t] = idx;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (t < h) {
            r_sum[t] += r_sum[t + h];
            if (r_val[t + h] > r_val[t] || (r_val[t + h] == r_val[t] && r_idx[t + h] < r_idx[t])) {
                r_val[t] = r_val[t + h];
                r_idx[t] = r_idx[t + h];
            }
        }
        __syncthreads();
    }
    if (t == 0) {
        out[n] = r_sum[0];
        out[n + 1] = r_idx[0];
    }
}

__global__ __launch_bounds__(256) void k_cluster_row(PcaView v, size_t pixel, float *__restrict__ out)
{
    const int j = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (j < v.L) out[j] = v.x[pixel * v.row_stride + (size_t)j * v.col_step];
}

namespace {

struct StepPlan {
    int cw, col_blocks, slabs, stat_slabs;
    size_t slab_pix, stat_slab_pix;
};
void split(size_t npix, size_t want, size_t most, int &slabs, size_t &slab_pix)
{
    want = want < 1 ? 1 : (want > most ? most : want);
    slab_pix = (npix + want - 1) / want;
    if (slab_pix < 1) slab_pix = 1;
    slabs = (int)((npix + slab_pix - 1) / slab_pix);
    if (slabs < 1) slabs = 1;
}
StepPlan step_plan(size_t npix, int L, int K)
{
    StepPlan q;
    const int n = L + 1;
    q.cw = 1;
    while (q.cw < n && q.cw < 256) q.cw <<= 1;
    q.col_blocks = (n + q.cw - 1) / q.cw;
    // 128 pixels of a column per thread row, as long as the partials stay below 16 MiB
    size_t most = ((size_t)1 << 21) / ((size_t)K * (size_t)n);
    most = most < 1 ? 1 : (most > 4096 ? 4096 : most);
    split(npix, (npix + 127) / 128, most, q.slabs, q.slab_pix);
    split(npix, (npix + 1023) / 1024, 1024, q.stat_slabs, q.stat_slab_pix);
    return q;
}

}  // namespace

ClusterWs cluster_ws(void *ws, size_t npix, int L, int K)
{
    const StepPlan q = step_plan(npix, L, K);
    const size_t n = (size_t)K * (size_t)(L + 1);
    unsigned char *base = static_cast<unsigned char *>(ws);
    ClusterWs w;
    size_t at = 0;
    w.out = reinterpret_cast<double *>(base + at);
    at += (n + 2) * sizeof(double);
    w.changed = reinterpret_cast<unsigned long long *>(base + at);
    at += sizeof(unsigned long long);
    at = (at + 15) & ~(size_t)15;
    w.cent = reinterpret_cast<float *>(base + at);
    at += (size_t)K * (size_t)L * sizeof(float);
    at = (at + 15) & ~(size_t)15;
    w.psum = reinterpret_cast<double *>(base + at);
    at += (size_t)q.slabs * n * sizeof(double);
    w.pstat = reinterpret_cast<double *>(base + at);
    at += (size_t)q.stat_slabs * 3 * sizeof(double);
    w.bytes = at;
    return w;
}

void launch_cluster_step(hipStream_t st, const PcaView &v, int K, const ClusterWs &w, int32_t *label, float *dist2)
{
    const StepPlan q = step_plan(v.npix, v.L, K);
    const size_t blocks = (v.npix * kWave + 255) / 256;
    const unsigned grid = (unsigned)(blocks < 1 ? 1 : (blocks > (size_t)kNumCU * 8 ? (size_t)kNumCU * 8 : blocks));
    const size_t lds = (size_t)K * (size_t)v.L * sizeof(float);
    switch ((v.L + kWave - 1) / kWave) {
    case 1: THZ_LAUNCH(k_cluster_assign<1>, grid, 256, lds, st, v, w.cent, K, label, dist2, w.changed); break;
    case 2: THZ_LAUNCH(k_cluster_assign<2>, grid, 256, lds, st, v, w.cent, K, label, dist2, w.changed); break;
    case 3: THZ_LAUNCH(k_cluster_assign<3>, grid, 256, lds, st, v, w.cent, K, label, dist2, w.changed); break;
    case 4: THZ_LAUNCH(k_cluster_assign<4>, grid, 256, lds, st, v, w.cent, K, label, dist2, w.changed); break;
    case 5: THZ_LAUNCH(k_cluster_assign<5>, grid, 256, lds, st, v, w.cent, K, label, dist2, w.changed); break;
    case 6: THZ_LAUNCH(k_cluster_assign<6>, grid, 256, lds, st, v, w.cent, K, label, dist2, w.changed); break;
    case 7: THZ_LAUNCH(k_cluster_assign<7>, grid, 256, lds, st, v, w.cent, K, label, dist2, w.changed); break;
    default: THZ_LAUNCH(k_cluster_assign<8>, grid, 256, lds, st, v, w.cent, K, label, dist2, w.changed); break;
    }
    const dim3 sgrid((unsigned)q.col_blocks, (unsigned)q.slabs);
    if (K <= 2) THZ_LAUNCH(k_cluster_sums<2>, sgrid, 256, 0, st, v, label, K, q.cw, q.slab_pix, w.psum);
    else if (K <= 4) THZ_LAUNCH(k_cluster_sums<4>, sgrid, 256, 0, st, v, label, K, q.cw, q.slab_pix, w.psum);
    else if (K <= 8) THZ_LAUNCH(k_cluster_sums<8>, sgrid, 256, 0, st, v, label, K, q.cw, q.slab_pix, w.psum);
    else THZ_LAUNCH(k_cluster_sums<16>, sgrid, 256, 0, st, v, label, K, q.cw, q.slab_pix, w.psum);
    THZ_LAUNCH(k_cluster_stats, (unsigned)q.stat_slabs, 256, 0, st, v.npix, v.mask, label, dist2, q.stat_slab_pix, w.pstat);
    const int n = K * (v.L + 1);
    THZ_LAUNCH(k_cluster_fold, (unsigned)((n + 7) / 8 + 1), 256, 0, st, w.psum, q.slabs, n, w.pstat, q.stat_slabs, v.npix, w.out);
}

void launch_cluster_row(hipStream_t st, const PcaView &v, size_t pixel, float *out)
{
    THZ_LAUNCH(k_cluster_row, (unsigned)((v.L + 255) / 256), 256, 0, st, v, pixel, out);
}

}  // namespace thz
