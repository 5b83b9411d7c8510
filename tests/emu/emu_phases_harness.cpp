// emu_phases_harness.cpp — the fused F chain told that its phase output already holds the phases (fft_f.hpp, "kept
// phases") on the host-thread emulation.  TEST INFRASTRUCTURE ONLY, linked next to emu_harness.cpp by
// tests/test_emu_keep_phases.py.
#include "plan_host.hpp"

using namespace thz;

namespace thz {
extern thread_local int g_f_last_cfg;
extern thread_local int g_f_last_phases_kept;
}

static bool phases_plan(int nt, PlanHost &H, std::vector<float> &ones, PlanDev &D)
{
    if (!build_plan((size_t)nt, H, true, true)) return false;
    if (H.family != kFamilyF) return false;
    ones.assign((size_t)H.nf, 1.0f);
    D = plan_dev(H, H.tw.data(), H.tw_split.data(), H.chirp_conj.data(), H.bfft.data(), H.f_t1.data(), H.f_t2.data(),
                 H.f_w2n.data(), ones.data(), nullptr, nullptr, nullptr);
    return pipeline_keeps_range(D);
}

static void band4(int band_lo, int band_hi, int *lo4, int *n)
{
    *lo4 = *n = 0;
    if (band_hi > band_lo) {
        *lo4 = band_lo & ~3;
        *n = ((band_hi + 3) & ~3) - *lo4;
    }
}

// the block rows a launch with sums leaves (each 2 nf floats, or nf with the phases kept); negative on error
extern "C" int emu_phases_sum_rows(int nt, size_t npix, int cmask, int band_lo, int band_hi)
{
    PlanHost H;
    std::vector<float> ones;
    PlanDev D;
    if (!phases_plan(nt, H, ones, D)) return -2;
    int lo4, n;
    band4(band_lo, band_hi, &lo4, &n);
    return (int)pipeline_sum_rows(D, npix, cmask != 0, lo4, n);
}

// One fused launch, as emu_pipeline_prune runs it (emu_prune_harness.cpp), with keep_phases handed to launch_pipeline.
// partial (with sums): the caller's rows x 2 nf floats for the block rows, so that it can see what the launch wrote
// there.  *cfg_bits: g_f_last_cfg; *kept: g_f_last_phases_kept — and the final pass over the rows takes them as the
// launch left them: nf floats each and the first nf floats of sums with the phases kept, 2 nf otherwise.
extern "C" int emu_pipeline_phases(int nt, size_t npix, const float *raw, const float *pre, const float *mask, const float *cmask,
                                   const float *post, float *fft, float *amp, float *ph, float *out, float *img, float *sums,
                                   float *partial, int band_lo, int band_hi, int keep_lo4, int keep_n, int keep_phases,
                                   int *cfg_bits, int *kept)
{
    PlanHost H;
    std::vector<float> ones;
    PlanDev D;
    if (!phases_plan(nt, H, ones, D)) return -2;
    int lo4, n;
    band4(band_lo, band_hi, &lo4, &n);
    size_t rows = 0;
    if (sums) {
        rows = pipeline_sum_rows(D, npix, cmask != nullptr, lo4, n);
        if (rows == 0 || !partial) return -3;
    }
    g_f_last_cfg = -1;
    g_f_last_phases_kept = -1;
    launch_pipeline(nullptr, D, npix, raw, pre, mask, post, (c32 *)fft, amp, ph, out, img, (const c32 *)cmask,
                    sums ? partial : nullptr, lo4, n, keep_lo4, keep_n, keep_phases != 0);
    if (cfg_bits) *cfg_bits = g_f_last_cfg;
    if (kept) *kept = g_f_last_phases_kept;
    if (pipeline_kept_phases() != (g_f_last_phases_kept == 1)) return -4;
    if (sums) launch_sum_rows_f64(nullptr, partial, rows, (pipeline_kept_phases() ? 1 : 2) * (size_t)D.nf, sums);
    return (int)rows;
}
