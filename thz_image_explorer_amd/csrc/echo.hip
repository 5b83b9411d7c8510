// echo.hip — K18: the strongest separated pulses of every trace, and the layer thicknesses their delays give.
//
//   k_echo_map   per trace: rank 0 is k_peak_map's winner; ranks 1 .. K-1 are, round after round, the largest local
//                maximum of the key that reaches the threshold and keeps the guard distance to every earlier rank.
//                One wave per trace, one pass over HBM (4 nt B/trace): the rounds behind the first work on the quads
//                the lanes kept in registers (traces of 4 .. 4099 samples) or read the trace again through the
//                cache it has just passed through.  A sample's neighbours come from the lanes next door (registers) or
//                from two more loads (cache): the local-maximum test crosses quad, lane and batch boundaries.
//   k_layer_map  per pixel: the found ranks in time order, their delays and scale * delay
//
// Every winner is the ordered-key maximum followed by the complemented-index maximum of peak.hpp: it depends on the data
// alone, never on which lane held what.  Built with -ffp-contract=off: offsets and delays are the f32 formulas as written.
#include "echo.hpp"
#include "peak.hpp"
#include "kernels.hpp"
#include "thz_device.hpp"
#include "fft_f.hpp"  // load_f4: a 16-byte load that promises 4-byte alignment only
#include "../../include/thzgpu.h"

#include <math.h>

namespace thz {

namespace {

// quads a lane keeps between the rounds, by kernel form: NB batches of 64 lanes x 4 samples, and the nt % 4 samples
// behind the last whole quad.  Two forms, so that a 1001-sample trace does not pay for sixteen batches.
constexpr int kEchoRegSmall = 4, kEchoRegLarge = 16;
constexpr int echo_reg_nt(int nb) { return 4 * kWave * nb + 3; }

// a NaN key is ordered as -Inf
__device__ __forceinline__ float echo_low(float key) { return key == key ? key : -INFINITY; }

// Sample x0 with its neighbours (xm, xp; has_m / has_p: they exist) -> its key in peak_ordered's form when it is an
// admitted candidate, 0 when not.  A candidate rises from the sample in front and does not fall short of the one behind:
// a plateau gives its lowest index once.  `key >= thr` is false for a NaN key and for a NaN threshold.
template <int MODE>
__device__ __forceinline__ unsigned echo_cand(float xm, bool has_m, float x0, float xp, bool has_p, float thr)
{
    const float key = peak_key<MODE>(x0);
    const float km = echo_low(peak_key<MODE>(xm)), kp = echo_low(peak_key<MODE>(xp));
    const bool ok = (!has_m || key > km) && (!has_p || key >= kp) && key >= thr;
    return peak_ordered(key, ok);
}

// the quad at e with the sample in front of it and the one behind
template <int MODE>
__device__ __forceinline__ uint4 echo_cand_quad(float4 v, float xm, float xp, int e, int nt, float thr)
{
    uint4 c;
    c.x = echo_cand<MODE>(xm, e > 0, v.x, v.y, true, thr);
    c.y = echo_cand<MODE>(v.x, true, v.y, v.z, true, thr);
    c.z = echo_cand<MODE>(v.y, true, v.z, v.w, true, thr);
    c.w = echo_cand<MODE>(v.z, true, v.w, xp, e + 4 < nt, thr);
    return c;
}

// |i - k| >= g  <=>  (unsigned)(i + (g - 1 - k)) >= 2 g - 1, with g = min(guard, nt): a sample in front of the window
// wraps to a large value.  kEchoFar in place of g - 1 - k keeps every sample.
constexpr int kEchoFar = (int)0x80000000u;
__device__ __forceinline__ bool echo_far(int i, int c, unsigned lim) { return (unsigned)(i + c) >= lim; }

// A round's look at one sample the lane holds: a candidate inside the newest rank's guard is dropped for good (the
// earlier ranks' guards have been applied by the rounds before), the others compete.  A lane walks its samples in
// ascending order, so `>` keeps the lowest index of equal keys; 0 never wins.
__device__ __forceinline__ void echo_sweep(unsigned &ku, int i, int c, unsigned lim, unsigned &best, int &best_i)
{
    ku = echo_far(i, c, lim) ? ku : 0u;
    const bool take = ku > best;
    best = take ? ku : best;
    best_i = take ? i : best_i;
}

// v, where it stands: the compiler takes what follows from it for new at every use of this function, so that the sixty-four
// indices, masks and addresses of a lane's samples are made where a phase needs them and not once in front of the trace
// loop, where they would hold a register each for the whole kernel.
__device__ __forceinline__ int echo_here(int v)
{
    asm volatile("" : "+v"(v));
    return v;
}

// a sample as the key the lane keeps.  Mode 2's negation is made here, once: left to the compiler it moves into every
// use, and the sixteen-batch form no longer fits its registers.
template <int MODE>
__device__ __forceinline__ float echo_key_kept(float x)
{
    float key = peak_key<MODE>(x);
    if (MODE == 2) asm volatile("" : "+v"(key));
    return key;
}

}  // namespace

// NB > 0: the register form for 4 <= nt <= echo_reg_nt(NB), straight-line over the NB batches (a quad behind the trace's
// last whole one is that one again, as in k_peak_map, and holds no candidate).  NB == 0: the streaming form for every nt;
// its first pass is k_peak_map's loop, its rounds read the trace again.  n_echoes >= 2: one rank is k_peak_map's own work.
// A wave takes its trace's steps one after the other — loads, maximum, candidates, sweep, maximum, re-read, store — so
// the kernel is as fast as a CU has waves.  Hence 80 scalar registers at most (a few live in lanes of one vector register
// instead): beyond 80 a CU admits seven 256-thread blocks, beyond 96 six.  The sixteen-batch form is held to three waves
// per SIMD (168 vector registers): twelve waves of 16 KiB each keep a CU's loads in flight.
template <int MODE, int NB>
__global__ __launch_bounds__(256, NB > kEchoRegSmall ? 3 : 1) __attribute__((amdgpu_num_sgpr(80)))
void k_echo_map(size_t npix, int nt, const float *__restrict__ data, int n_echoes, int guard, float rel_threshold,
                int *__restrict__ index, float *__restrict__ offset, float *__restrict__ value, int *__restrict__ count)
{
    constexpr bool REG = NB > 0;
    constexpr int kBatch = 2;  // the streaming form's loads in flight: k_peak_map's
    const int lane = lane_id();
    const int wib = (int)(threadIdx.x >> 6);
    const int wpb = (int)(blockDim.x >> 6);
    const int nt4 = nt & ~3;
    const int g = guard < nt ? guard : nt;  // |i - k| < nt: a guard of nt or more admits nothing, as does nt itself
    const unsigned lim = 2u * (unsigned)g - 1u;
    for (size_t p = (size_t)blockIdx.x * wpb + wib; p < npix; p += (size_t)gridDim.x * wpb) {
        const float *x = data + p * (size_t)nt;
        float best = -INFINITY;
        int best_i = -1;
        float4 v[REG ? NB : 1];
        if constexpr (REG) {
            // every quad of the trace at once, then the winner among them
            const int e0 = echo_here(4 * lane);
#pragma unroll
            for (int u = 0; u < NB; ++u) {
                const int e = e0 + 4 * kWave * u;
                load_f4(x + (e < nt4 ? e : nt4 - 4), v[u].x, v[u].y, v[u].z, v[u].w);
            }
            // kept as keys (the values are read again where a rank is written): from here on the quads are mode 1's
#pragma unroll
            for (int u = 0; u < NB; ++u)
                v[u] = float4{echo_key_kept<MODE>(v[u].x), echo_key_kept<MODE>(v[u].y), echo_key_kept<MODE>(v[u].z), echo_key_kept<MODE>(v[u].w)};
#pragma unroll
            for (int u = 0; u < NB; ++u) {
                const int e = e0 + 4 * kWave * u;
                const int at = e < nt4 ? e : nt4 - 4;
                peak_take<1>(v[u].x, at, best, best_i);
                peak_take<1>(v[u].y, at + 1, best, best_i);
                peak_take<1>(v[u].z, at + 2, best, best_i);
                peak_take<1>(v[u].w, at + 3, best, best_i);
            }
        } else {
            for (int e0 = 4 * lane; e0 < nt4; e0 += 4 * kWave * kBatch) {
                float4 q[kBatch];
                int at[kBatch];
#pragma unroll
                for (int u = 0; u < kBatch; ++u) {
                    const int e = e0 + 4 * kWave * u;
                    at[u] = e < nt4 ? e : nt4 - 4;
                    load_f4(x + at[u], q[u].x, q[u].y, q[u].z, q[u].w);
                }
#pragma unroll
                for (int u = 0; u < kBatch; ++u) {
                    peak_take<MODE>(q[u].x, at[u], best, best_i);
                    peak_take<MODE>(q[u].y, at[u] + 1, best, best_i);
                    peak_take<MODE>(q[u].z, at[u] + 2, best, best_i);
                    peak_take<MODE>(q[u].w, at[u] + 3, best, best_i);
                }
            }
        }
        float xt = 0.0f;  // the lane's sample behind the last whole quad
        if (nt4 + lane < nt) {
            xt = x[nt4 + lane];
            peak_take<MODE>(xt, nt4 + lane, best, best_i);
        }
        const unsigned top0 = wave_reduce_max_u32(peak_ordered(best, best_i >= 0));
        int k0 = peak_wave_lowest(peak_ordered(best, best_i >= 0), top0, best_i);
        if (top0 == 0u) k0 = peak_first_number<MODE>(x, nt, lane);  // (wave-uniform, cold) no key above -Inf
        // ranks 1 .. K-1 (wave-uniform throughout): a round that finds nothing ends the search
        int k1 = -1, k2 = -1, k3 = -1, n = 1;
        if (n_echoes > 1) {
            // the winner's key back from its ordered form (a -0 comes back as +0, which no comparison below tells apart);
            // on the cold path it is -Inf or NaN, from the trace
            const float thr = rel_threshold * (top0 ? peak_unordered(top0) : peak_key<MODE>(x[k0]));
            // Once per trace: every sample the lane holds becomes its key if it is an admitted candidate and 0 if not.
            // The sample in front of a quad is the last of the lane below — for lane 0 lane 63's of the batch before —
            // and the one behind it the first of the lane above — for lane 63 lane 0's of the next batch.
            uint4 c[REG ? NB : 1];
            if constexpr (REG) {
                const int e0 = echo_here(4 * lane);
#pragma unroll
                for (int u = 0; u < NB; ++u) {
                    const int e = e0 + 4 * kWave * u;
                    const float up = (u > 0 && lane == kWave - 1) ? v[u > 0 ? u - 1 : 0].w : v[u].w;
                    const float dn = lane == 0 ? v[u + 1 < NB ? u + 1 : u].x : v[u].x;
                    const float xm = wave_shfl(up, (lane + kWave - 1) & (kWave - 1));
                    float xp = wave_shfl(dn, (lane + 1) & (kWave - 1));
                    if (e + 4 == nt4 && nt4 < nt) xp = peak_key<MODE>(x[nt4]);  // behind the last whole quad: the tail's first sample
                    const uint4 cq = echo_cand_quad<1>(v[u], xm, xp, e, nt, thr);
                    const bool in = e < nt4;
                    c[u] = uint4{in ? cq.x : 0u, in ? cq.y : 0u, in ? cq.z : 0u, in ? cq.w : 0u};
                }
            }
            unsigned ct = 0u;
            {
                const int i = nt4 + lane;
                if (i < nt) ct = echo_cand<MODE>(x[i > 0 ? i - 1 : 0], i > 0, xt, x[i + 1 < nt ? i + 1 : i], i + 1 < nt, thr);
            }
            int c0 = kEchoFar, c1 = kEchoFar, c2 = kEchoFar;  // g - 1 - index of the ranks found so far (the streaming form)
            for (int j = 1; j < n_echoes; ++j) {
                const int cn = g - 1 - (j == 1 ? k0 : (j == 2 ? k1 : k2));  // the newest rank's
                c0 = j == 1 ? cn : c0;
                c1 = j == 2 ? cn : c1;
                c2 = j == 3 ? cn : c2;
                unsigned top = 0u;
                int top_i = -1;
                if constexpr (REG) {
                    const int e0 = echo_here(4 * lane);
#pragma unroll
                    for (int u = 0; u < NB; ++u) {
                        const int e = e0 + 4 * kWave * u;
                        echo_sweep(c[u].x, e, cn, lim, top, top_i);
                        echo_sweep(c[u].y, e + 1, cn, lim, top, top_i);
                        echo_sweep(c[u].z, e + 2, cn, lim, top, top_i);
                        echo_sweep(c[u].w, e + 3, cn, lim, top, top_i);
                    }
                } else {
                    // the trace again, through the cache it has just passed through: a quad and the samples on either
                    // side of it, with every earlier rank's guard
                    for (int e = 4 * lane; e < nt4; e += 4 * kWave) {
                        float4 q;
                        load_f4(x + e, q.x, q.y, q.z, q.w);
                        const float xm = x[e > 0 ? e - 1 : 0], xp = x[e + 4 < nt ? e + 4 : e];
                        const uint4 cq = echo_cand_quad<MODE>(q, xm, xp, e, nt, thr);
                        const unsigned ku[4] = {cq.x, cq.y, cq.z, cq.w};
#pragma unroll
                        for (int q4 = 0; q4 < 4; ++q4) {
                            const int i = e + q4;
                            const bool take = ku[q4] > top && echo_far(i, c0, lim) && echo_far(i, c1, lim) && echo_far(i, c2, lim);
                            top = take ? ku[q4] : top;
                            top_i = take ? i : top_i;
                        }
                    }
                }
                echo_sweep(ct, nt4 + lane, cn, lim, top, top_i);
                const int k = peak_wave_winner_ordered(top, top_i);
                if (k < 0) break;
                k1 = j == 1 ? k : k1;
                k2 = j == 2 ? k : k2;
                k3 = j == 3 ? k : k3;
                n = j + 1;
            }
        }
        static_assert(THZ_ECHO_MAX == 4, "ranks k0 .. k3");
        // lane j writes rank j: value and vertex from the trace again, as k_peak_map's lane 0 does
        if (lane < n_echoes) {
            const int k = lane == 0 ? k0 : (lane == 1 ? k1 : (lane == 2 ? k2 : k3));
            float y0 = 0.0f, off = 0.0f;
            if (k >= 0) off = peak_vertex(x, k, nt, y0);
            const size_t o = (size_t)lane * npix + p;
            if (index) index[o] = k;
            if (offset) offset[o] = off;
            if (value) value[o] = y0;
        }
        if (lane == 0 && count) count[p] = n;
    }
}

__global__ __launch_bounds__(256) void k_echo_count_one(size_t npix, int *__restrict__ count)
{
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p < npix) count[p] = 1;
}

// One thread per pixel.  The ranks that were found (index >= 0) in ascending index order — an insertion sort that moves
// a pair only in front of a strictly larger index — then the differences of neighbours.
__global__ __launch_bounds__(256) void k_layer_map(size_t npix, LayerGeom g, const int *__restrict__ index,
                                                   const float *__restrict__ offset, float *__restrict__ thickness,
                                                   float *__restrict__ delay)
{
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npix) return;
    if (g.mode == 1) {
        const float d = (float)(int)((unsigned)index[p] - (unsigned)g.ref_index) + (offset[p] - g.ref_offset);
        if (delay) delay[p] = d;
        if (thickness) thickness[p] = g.scale[0] * d;
        return;
    }
    int idx[THZ_ECHO_MAX];
    float off[THZ_ECHO_MAX];
    int n = 0;
#pragma unroll
    for (int j = 0; j < THZ_ECHO_MAX; ++j) {
        const bool in = j < g.n_echoes;
        const int i = in ? index[(size_t)j * npix + p] : -1;
        idx[j] = i >= 0 ? i : 0x7fffffff;  // an absent rank sorts behind every found one
        off[j] = in ? offset[(size_t)j * npix + p] : 0.0f;
        n += i >= 0 ? 1 : 0;
    }
#pragma unroll
    for (int a = 1; a < THZ_ECHO_MAX; ++a)
#pragma unroll
        for (int b = a; b > 0; --b) {
            const bool swap = idx[b - 1] > idx[b];
            const int ti = idx[b];
            const float to = off[b];
            idx[b] = swap ? idx[b - 1] : ti;
            off[b] = swap ? off[b - 1] : to;
            idx[b - 1] = swap ? ti : idx[b - 1];
            off[b - 1] = swap ? to : off[b - 1];
        }
#pragma unroll
    for (int l = 0; l + 1 < THZ_ECHO_MAX; ++l) {
        if (l + 1 < g.n_echoes) {
            const bool have = l + 1 < n;
            const float d = have ? (float)(idx[l + 1] - idx[l]) + (off[l + 1] - off[l]) : NAN;
            if (delay) delay[(size_t)l * npix + p] = d;
            if (thickness) thickness[(size_t)l * npix + p] = have ? g.scale[l] * d : NAN;
        }
    }
}

void launch_echo_map(hipStream_t st, size_t npix, int nt, const float *data, int mode, int n_echoes, int guard,
                     float rel_threshold, int *index, float *offset, float *value, int *count)
{
    const size_t blocks = (npix * kWave + 255) / 256;
    const unsigned grid = (unsigned)(blocks < 1 ? 1 : (blocks > (size_t)kNumCU * 8 ? (size_t)kNumCU * 8 : blocks));
    // One rank is the arrival-time map itself, and every trace has it
    if (n_echoes == 1) {
        if (index || offset || value) launch_peak_map(st, npix, nt, data, mode, index, offset, value);
        if (count) THZ_LAUNCH(k_echo_count_one, (unsigned)((npix + 255) / 256), 256, 0, st, npix, count);
        return;
    }
    // A trace without a whole quad has nothing to keep, a long one does not fit: the streaming form.  Otherwise the
    // smallest register form that holds the trace.
    const int nb = (nt < 4 || nt > echo_reg_nt(kEchoRegLarge)) ? 0
                   : (nt <= echo_reg_nt(kEchoRegSmall) ? kEchoRegSmall : kEchoRegLarge);
#define THZ_ECHO(M, NB) \
    THZ_LAUNCH((k_echo_map<M, NB>), grid, 256, 0, st, npix, nt, data, n_echoes, guard, rel_threshold, index, offset, value, count)
#define THZ_ECHO_FORMS(M) \
    if (nb == 0) THZ_ECHO(M, 0); else if (nb == kEchoRegSmall) THZ_ECHO(M, kEchoRegSmall); else THZ_ECHO(M, kEchoRegLarge)
    switch (mode) {
    case 0: THZ_ECHO_FORMS(0); break;
    case 1: THZ_ECHO_FORMS(1); break;
    default: THZ_ECHO_FORMS(2); break;
    }
#undef THZ_ECHO_FORMS
#undef THZ_ECHO
}

void launch_layer_map(hipStream_t st, size_t npix, const LayerGeom &g, const int *index, const float *offset,
                      float *thickness, float *delay)
{
    THZ_LAUNCH(k_layer_map, (unsigned)((npix + 255) / 256), 256, 0, st, npix, g, index, offset, thickness, delay);
}

}  // namespace thz
