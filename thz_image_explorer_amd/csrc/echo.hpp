// echo.hpp — K18 echoes and layer thickness: the launches of echo.hip
#pragma once
#include <hip/hip_runtime.h>

#include <stddef.h>
#include <stdint.h>

namespace thz {

// per trace of a (npix, nt) cube: the n_echoes strongest separated pulses (include/thzgpu.h, "Echoes and layer
// thickness").  index, offset, value: (n_echoes, npix) rank-major; count: (npix); any output may be null.
// mode 0..2, 1 <= n_echoes <= THZ_ECHO_MAX, guard >= 1 — checked by the caller
void launch_echo_map(hipStream_t st, size_t npix, int nt, const float *data, int mode, int n_echoes, int guard,
                     float rel_threshold, int *index, float *offset, float *value, int *count);

struct LayerGeom {
    int mode;         // 0: consecutive pulses in time order, n_echoes - 1 rows; 1: rank 0 against (ref_index, ref_offset), one row
    int n_echoes;
    float scale[4];
    int ref_index;
    float ref_offset;
};
// delays and thicknesses from (n_echoes, npix) index and offset maps; either output may be null
void launch_layer_map(hipStream_t st, size_t npix, const LayerGeom &g, const int *index, const float *offset,
                      float *thickness, float *delay);

}  // namespace thz
