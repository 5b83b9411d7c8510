// emu_tilted_harness.cpp — C entry points over the FBP kernels' fused chain with its extras (fft_fbp.hpp: the Tilt
// stage's re-laying as a gather in the loads, the complex multiplier, the in-launch pixel sums), built with -DTHZ_EMU
// next to emu_harness.cpp.  TEST INFRASTRUCTURE ONLY (tests/test_emu_tilted_chain.py, tests/emu/tsan_tilted_driver.cpp).
#include "plan_host.hpp"

using namespace thz;

static std::vector<float> t_ones;
static PlanDev tilted_plan(PlanHost &H)
{
    t_ones.assign((size_t)H.nf, 1.0f);
    return plan_dev(H, H.tw.data(), H.tw_split.data(), H.chirp_conj.data(), H.bfft.data(),
                    H.f_t1.empty() ? nullptr : H.f_t1.data(), H.f_t2.empty() ? nullptr : H.f_t2.data(),
                    H.f_w2n.empty() ? nullptr : H.f_w2n.data(), t_ones.data(), H.p_t1.empty() ? nullptr : H.p_t1.data(),
                    H.p_t2.empty() ? nullptr : H.p_t2.data(), nullptr);
}

static const float kSentinel = -777.0f;

extern "C" {

// thz_pipeline_tilted's launches for an FBP plan, as api.cpp issues them.  src == nullptr: the un-tilted fused chain
// (thz_pipeline_ex) on `raw` (npix x nt) instead.  sums (2 nf) / src_sum (nt) may be null.  Returns the number of
// partial rows of the sums (0 without them); -2 not an FBP plan, -4 a partial-row entry was left unwritten.
int emu_fbp_chain(int nt, size_t npix, const float *raw, const float *src, int nt_in, const float *taper, const int *ins,
                  const float *pre, const float *mask, const float *cmask, const float *post, float *fft, float *amp,
                  float *ph, float *out, float *img, float *sums, float *src_sum)
{
    PlanHost H;
    if (!build_plan((size_t)nt, H, true, true)) return -2;
    if (H.family != kFamilyFBP) return -2;
    PlanDev D = tilted_plan(H);
    const size_t nf = (size_t)D.nf;
    const size_t rows = sums ? pipeline_sum_rows(D, npix, cmask != nullptr) : 0;
    if (sums && rows == 0) return -3;
    std::vector<float> partial(rows * 2 * nf, kSentinel);  // every entry must be written by the kernel
    float *part = rows ? partial.data() : nullptr;
    if (src) {
        const FBPTilt TL{src, taper, ins, nt_in};
        if (!launch_pipeline_tilted(nullptr, D, npix, TL, pre, mask, post, (c32 *)fft, amp, ph, out, img, (const c32 *)cmask, part))
            return -2;
        if (src_sum) {
            const size_t srows = tilt_sum_rows(npix);
            std::vector<float> sp(srows * (size_t)nt, kSentinel);
            if (!launch_tilt_sum(nullptr, npix, nt, TL, sp.data(), src_sum)) return -2;
            for (float v : sp)
                if (v == kSentinel) return -4;
        }
    } else {
        launch_pipeline(nullptr, D, npix, raw, pre, mask, post, (c32 *)fft, amp, ph, out, img, (const c32 *)cmask, part);
    }
    for (float v : partial)
        if (v == kSentinel) return -4;
    if (rows) launch_sum_rows_f64(nullptr, partial.data(), rows, 2 * nf, sums);
    return (int)rows;
}
}
