// peak.hpp — K16 arrival times: the launches of peak.hip
#pragma once
#include <hip/hip_runtime.h>

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

}  // namespace thz
