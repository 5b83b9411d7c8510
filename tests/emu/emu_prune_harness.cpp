// emu_prune_harness.cpp — the fused F chain with a keep range AND the band outside which its multiplier is zero
// (fft_f.hpp, "band pruning") on the host-thread emulation.  TEST INFRASTRUCTURE ONLY, linked next to emu_harness.cpp by
// tests/test_emu_band_prune.py.
#include "plan_host.hpp"

using namespace thz;

namespace thz { extern thread_local int g_f_last_cfg; }

// One fused launch, as emu_pipeline_keep runs it (emu_keep_harness.cpp); band_hi > band_lo: the multiplier is zero
// outside [band_lo, band_hi).  *cfg_bits: the kCfg bits of the k_f build that ran.  Returns the number of block rows
// (0 without sums), negative on error.
extern "C" int emu_pipeline_prune(int nt, size_t npix, const float *raw, const float *pre, const float *mask, const float *cmask,
                                  const float *post, float *fft, float *amp, float *ph, float *out, float *img, float *sums,
                                  int band_lo, int band_hi, int keep_lo4, int keep_n, int *cfg_bits)
{
    PlanHost H;
    if (!build_plan((size_t)nt, H, true, true)) return -2;
    if (H.family != kFamilyF) return -2;
    std::vector<float> ones((size_t)H.nf, 1.0f);
    PlanDev D = plan_dev(H, H.tw.data(), H.tw_split.data(), H.chirp_conj.data(), H.bfft.data(), H.f_t1.data(), H.f_t2.data(),
                         H.f_w2n.data(), ones.data(), nullptr, nullptr, nullptr);
    if (!pipeline_keeps_range(D)) return -2;
    int lo4 = 0, n = 0;
    if (band_hi > band_lo) {
        lo4 = band_lo & ~3;
        n = ((band_hi + 3) & ~3) - lo4;
    }
    size_t rows = 0;
    std::vector<float> partial;
    if (sums) {
        rows = pipeline_sum_rows(D, npix, cmask != nullptr, lo4, n);
        if (rows == 0) return -3;
        partial.assign(rows * 2 * (size_t)D.nf, -777.0f);  // every entry must be written by the kernel
    }
    g_f_last_cfg = -1;
    launch_pipeline(nullptr, D, npix, raw, pre, mask, post, (c32 *)fft, amp, ph, out, img, (const c32 *)cmask,
                    sums ? partial.data() : nullptr, lo4, n, keep_lo4, keep_n);
    if (cfg_bits) *cfg_bits = g_f_last_cfg;
    if (sums) launch_sum_rows_f64(nullptr, partial.data(), rows, 2 * (size_t)D.nf, sums);
    return (int)rows;
}
