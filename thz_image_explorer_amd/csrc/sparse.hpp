// sparse.hpp — K21 sparse deconvolution of every trace (ISTA / FISTA): the launch of sparse.hip and the layout both
// sides of it agree on
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

struct thz_sparse_cfg;
// sparse_host.cpp: the argument rules of thz_sparse_deconv and thz_host_sparse_trace — the reason for THZ_ERR_INVALID, or null
const char *sparse_cfg_error(const thz_sparse_cfg *cfg, size_t nt, const float *taps);

namespace thz {

constexpr int kSparseOut = 16;  // consecutive outputs a lane owns in a chunk; a chunk is kWave of them

inline int sparse_up16(int v) { return (v + 15) & ~15; }

// What one launch works with.  The two products are the same loop: acc[o] = sum over t of taps[t] * buf[q0 + o + t]
// in ascending t, with q0 a multiple of 16.  A product's own shift (c for H, P - 1 - c for H^T) is not a multiple of
// 16, so its taps stand behind `shift % 16` zero taps and are filled up with zeros to a multiple of 16: terms with a
// zero tap are executed, which the definition admits.
struct SparseGeom {
    int nt, ntp;            // samples of a trace; rounded up to 16
    int front;              // zeros in front of sample 0 in the z and r images: up16(P - 1)
    int len;                // entries of a z or r image: front + ntp + up16(P + 15) + 16, a multiple of 16
    int h_block, h_taps;    // H:   q0 = i0 + 16 h_block, h_taps taps at table[0 ..)
    int t_block, t_taps;    // H^T: q0 = j0 + 16 t_block, t_taps taps at table[h_taps ..)
    int n_iter, accelerate; // beta[n] at table[h_taps + t_taps + n]
    float step, rel_lambda, min_lambda;
};
// false: outside the limits of thz_sparse_cfg (the caller has checked them; this is the launch's own guard)
bool sparse_geom(int nt, int P, int c, int n_iter, int accelerate, float step, float rel_lambda, float min_lambda, SparseGeom *g);
inline size_t sparse_table_floats(const SparseGeom &g) { return (size_t)g.h_taps + (size_t)g.t_taps + (size_t)g.n_iter; }
// [H's taps: h[P - 1 - k] behind its zeros | H^T's: h[k] behind its zeros | beta[0 .. n_iter)]
void sparse_fill_table(const SparseGeom &g, const float *taps, int P, int c, float *table);
// LDS of one wave: the z and r images with their zeros, y and x without, every 16 entries followed by one unused word
size_t sparse_lds_bytes(const SparseGeom &g);

// beta[n] = (float)((t_n - 1) / t_{n+1}), t_0 = 1, t_{n+1} = (1 + sqrt(1 + 4 t_n^2)) / 2, in double (sparse_host.cpp):
// the one table of the device and of thz_host_sparse_trace
void sparse_momentum(int n_iter, float *beta);

// One wave per trace; d_out == d_data is allowed.  resid / nnz may be null.  Returns what hipFuncSetAttribute or the
// launch said.
hipError_t launch_sparse_deconv(hipStream_t st, size_t npix, const SparseGeom &g, const float *data, const float *table,
                                float *out, float *resid, int32_t *nnz);

}  // namespace thz
