// wavelet.hpp — K23 wavelet shrinkage of every trace (undecimated transform, periodic extension): the launch of
// wavelet.hip and the record both sides of it agree on
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/thzgpu.h"

// wavelet_host.cpp: the argument rules of thz_wavelet_denoise and thz_host_wavelet_trace — the reason for
// THZ_ERR_INVALID, or null
const char *wavelet_cfg_error(const thz_wavelet_cfg *cfg, size_t nt, const float *hn, const float *gn, const float *scale);

namespace thz {

constexpr int kWaveletBlock = 256;  // threads of the block that works on one trace
// LDS words in front of the planes: the 256 bins of the median's radix select, the waves' bin totals, the digit found
// and the rank inside it, the trace's count of kept coefficients
constexpr int kWaveletScratchWords = 256 + 8;

// What one launch works with; it travels as a kernel argument, so the taps are read from scalar memory.
struct WaveletParams {
    int nt, n_taps, n_levels, shrink, noise_mode;
    float hn[THZ_WAVELET_MAX_TAPS], gn[THZ_WAVELET_MAX_TAPS];
    float scale[THZ_WAVELET_MAX_LEVELS];
};
// LDS of one block: the scratch words, the ping-pong pair of approximations and n_levels detail planes, nt words each
inline size_t wavelet_lds_bytes(const WaveletParams &w)
{
    return sizeof(float) * ((size_t)kWaveletScratchWords + (size_t)(w.n_levels + 2) * (size_t)w.nt);
}

// One block per trace; d_out == d_data is allowed.  sigma / kept may be null.  Returns what hipFuncSetAttribute or the
// launch said.
hipError_t launch_wavelet_denoise(hipStream_t st, size_t npix, const WaveletParams &w, const float *data, float *out,
                                  float *sigma, int32_t *kept);

}  // namespace thz
