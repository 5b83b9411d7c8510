// emu_keep_harness.cpp — the fused F chain with a keep range (fft_f.hpp: FArgs::keep_lo4 / keep_n) on the host-thread
// emulation.  TEST INFRASTRUCTURE ONLY, linked next to emu_harness.cpp by tests/test_emu_keep_range.py.
#include "plan_host.hpp"

using namespace thz;

// One fused launch.  sums != null: the pixel sums inside the launch (block rows + the final pass), as thz_pipeline_ex
// runs it; band_hi > band_lo: the real multiplier's non-zero range (kCfgBand at nt = 4096 with cmask and sums).
// keep_n < 0: every bin.  Returns the number of block rows (0 without sums), negative on error.
extern "C" int emu_pipeline_keep(int nt, size_t npix, const float *raw, const float *pre, const float *mask, const float *cmask,
                                 const float *post, float *fft, float *amp, float *ph, float *out, float *img, float *sums,
                                 int band_lo, int band_hi, int keep_lo4, int keep_n)
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
    launch_pipeline(nullptr, D, npix, raw, pre, mask, post, (c32 *)fft, amp, ph, out, img, (const c32 *)cmask,
                    sums ? partial.data() : nullptr, lo4, n, keep_lo4, keep_n);
    if (sums) launch_sum_rows_f64(nullptr, partial.data(), rows, 2 * (size_t)D.nf, sums);
    return (int)rows;
}
