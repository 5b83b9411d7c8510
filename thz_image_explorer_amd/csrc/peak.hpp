// peak.hpp — K16 arrival times: the launches of peak.hip, and the per-trace pieces that echo.hip (K18) shares with it
#pragma once
#include "thz_device.hpp"

#include <math.h>
#include <stddef.h>

namespace thz {

// per trace of a (npix, nt) cube: position, sub-sample offset and signed value of the extreme sample.
// mode 0 largest |x|, 1 maximum, 2 minimum; any output may be null
void launch_peak_map(hipStream_t st, size_t npix, int nt, const float *data, int mode, int *index, float *offset,
                     float *value);
// the ten sums of the arrival plane's normal equations, as doubles at the front of `ws` (plane_moments_ws_bytes() of
// device memory); three launches of a fixed geometry
size_t plane_moments_ws_bytes();
void launch_plane_moments(hipStream_t st, size_t nx, size_t ny, double dx, double dy, double dt, const int *index,
                          const float *offset, const float *value, float rel_threshold, void *ws);

#ifndef THZ_EMU
// ---- device pieces of one trace's winner (k_peak_map, k_echo_map)

// A key's bits mapped so that unsigned order is the floats' order (-0 counted as +0) and no number maps to 0: 0 is
// "no candidate", what a lane that saw nothing above -Inf hands in.  The wave's winner is then two maxima — of the
// mapped keys, and among the lanes that hold that key of the complemented indices (the LOWEST index is the largest) —
// and a maximum does not depend on which lane held what.
__device__ __forceinline__ unsigned peak_ordered(float key, bool have)
{
    unsigned b = __builtin_bit_cast(unsigned, key);
    if (b == 0x80000000u) b = 0u;
    const unsigned ordered = (b & 0x80000000u) ? ~b : (b | 0x80000000u);  // -Inf -> 0x007fffff, the smallest
    return have ? ordered : 0u;
}

template <int MODE>
__device__ __forceinline__ float peak_key(float x)
{
    return MODE == 0 ? fabsf(x) : (MODE == 1 ? x : -x);
}

// A lane walks its own samples in ascending order, so `>` alone keeps the lowest index of equal keys; a NaN key compares
// false and never wins.  Neither does a key of -Inf against the initial -Inf: a trace that holds nothing above -Inf is
// settled on the cold path of the kernel.
template <int MODE>
__device__ __forceinline__ void peak_take(float x, int i, float &best, int &best_i)
{
    const float key = peak_key<MODE>(x);
    const bool take = key > best;
    best = take ? key : best;
    best_i = take ? i : best_i;
}

// the wave's winner from every lane's (best, best_i; best_i < 0: none): the index in every lane, -1 when no lane has one
// the inverse of peak_ordered for a key that is there (ordered != 0)
__device__ __forceinline__ float peak_unordered(unsigned ordered)
{
    return __builtin_bit_cast(float, (ordered & 0x80000000u) ? (ordered & 0x7fffffffu) : ~ordered);
}
// the lowest index among the lanes that hold the wave's largest ordered key `top`
__device__ __forceinline__ int peak_wave_lowest(unsigned mine, unsigned top, int best_i)
{
    return (int)(0xffffffffu - wave_reduce_max_u32(mine == top ? 0xffffffffu - (unsigned)best_i : 0u));
}
__device__ __forceinline__ int peak_wave_winner_ordered(unsigned mine, int best_i)
{
    const unsigned top = wave_reduce_max_u32(mine);
    const int k = peak_wave_lowest(mine, top, best_i);
    return top == 0u ? -1 : k;
}
__device__ __forceinline__ int peak_wave_winner(float best, int best_i)
{
    return peak_wave_winner_ordered(peak_ordered(best, best_i >= 0), best_i);
}

// (wave-uniform, cold) a trace with no key above -Inf: the first sample that is a number — its key is -Inf, a tie of all
// such samples — or, in a trace of NaNs, sample 0
template <int MODE>
__device__ __forceinline__ int peak_first_number(const float *x, int nt, int lane)
{
    unsigned first = 0u;  // 0xffffffff - index of the lane's first number (never 0); 0: none
    for (int i = lane; i < nt; i += kWave) {
        const float key = peak_key<MODE>(x[i]);
        if (key == key && first == 0u) first = 0xffffffffu - (unsigned)i;
    }
    first = wave_reduce_max_u32(first);
    return first ? (int)(0xffffffffu - first) : 0;
}

// value and sub-sample vertex at sample k of x[0 .. nt): the winner and its neighbours as three loads that do not wait
// for each other (at the trace's ends a neighbour's place is taken by the winner itself, unused)
__device__ __forceinline__ float peak_vertex(const float *x, int k, int nt, float &y0)
{
    const bool inner = k > 0 && k < nt - 1;
    y0 = x[k];
    const float ym = x[inner ? k - 1 : k], yp = x[inner ? k + 1 : k];
    float off = 0.0f;
    const float den = ym - 2.0f * y0 + yp;
    // (`&`, not `&&`: a test that could end early would let the compiler put the third load behind the first two's wait)
    if ((int)inner & (int)isfinite(ym) & (int)isfinite(y0) & (int)isfinite(yp) & (int)(den != 0.0f)) {
        off = 0.5f * (ym - yp) / den;
        off = isfinite(off) ? fminf(fmaxf(off, -0.5f), 0.5f) : 0.0f;
    }
    return off;
}
#endif  // !THZ_EMU

}  // namespace thz
