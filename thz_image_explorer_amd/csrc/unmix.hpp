// unmix.hpp — K22 non-negative least squares per pixel: the launches of unmix.hip
#pragma once
#include "pca.hpp"

namespace thz {

// What the three launches read besides the cube, one block of floats on the device, filled once per call:
// [E: K x L | lref: L (zeros without absorbance) | Gt: K x K, Gt[c * K + i] = G[i][c] | rd: K]
inline size_t unmix_table_floats(int L, int K) { return (size_t)(K + 1) * (size_t)L + (size_t)K * (size_t)K + (size_t)K; }
struct UnmixTable {
    const float *e, *lref, *gt, *rd;
};
inline UnmixTable unmix_table(const float *d_tab, int L, int K)
{
    UnmixTable t;
    t.e = d_tab;
    t.lref = t.e + (size_t)K * (size_t)L;
    t.gt = t.lref + L;
    t.rd = t.gt + (size_t)K * (size_t)K;
    return t;
}

// proj[c * npix + p] = sum_j u[p, j] E[c, j], u = X or lref - logf(X): one wave per pixel (the mask of v is not read)
void launch_unmix_project(hipStream_t st, const PcaView &v, const UnmixTable &t, int K, bool absorbance, float *proj);
// abund[c * npix + p] and kkt[p] (or null) from proj, Gt and rd: one lane per pixel, n_sweeps sweeps at the most
void launch_unmix_solve(hipStream_t st, size_t npix, const UnmixTable &t, int K, int n_sweeps, const float *proj, float *abund,
                        float *kkt);
// resid[p] = sum_j (u[p, j] - sum_c abund[c, p] E[c, j])^2: one wave per pixel, the second pass over the row
void launch_unmix_resid(hipStream_t st, const PcaView &v, const UnmixTable &t, int K, bool absorbance, const float *abund,
                        float *resid);

}  // namespace thz
