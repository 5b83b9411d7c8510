// emu_ph_harness.cpp — C entry points over the PH kernels' fused chain with its extras (fft_ph.hpp: the complex
// multiplier and the in-launch pixel sums of k_ph<P, kPipe, CM, SUMS>), built with -DTHZ_EMU next to emu_harness.cpp.
// TEST INFRASTRUCTURE ONLY (tests/test_emu_ph_chain.py, tests/emu/tsan_ph_driver.cpp).
#include "plan_host.hpp"
#include "fft_f.hpp"
#include "fft_fb.hpp"
#include "fft_p.hpp"
#include "fft_ph.hpp"

using namespace thz;

namespace thz { extern int g_grid_cap_override; }

static std::vector<float> ph_ones;
static PlanDev ph_plan(PlanHost &H)
{
    ph_ones.assign((size_t)H.nf, 1.0f);
    return plan_dev(H, H.tw.data(), H.tw_split.data(), H.chirp_conj.data(), H.bfft.data(),
                    H.f_t1.empty() ? nullptr : H.f_t1.data(), H.f_t2.empty() ? nullptr : H.f_t2.data(),
                    H.f_w2n.empty() ? nullptr : H.f_w2n.data(), ph_ones.data(), H.p_t1.empty() ? nullptr : H.p_t1.data(),
                    H.p_t2.empty() ? nullptr : H.p_t2.data(), nullptr);
}

static const float kSentinel = -777.0f;

// the launch of kernels.hip's launch_ph for the named instantiation; returns the blocks of the grid
template <class PL, bool CM, bool SUMS>
static size_t ph_launch(const PlanDev &D, FBArgs &A)
{
    const unsigned waves = (unsigned)PHLayout<PL>::waves(SUMS);
    size_t g = (A.npix + waves - 1) / waves;
    if (g > (size_t)kNumCU) g = kNumCU;
    if (g_grid_cap_override > 0 && g > (size_t)g_grid_cap_override) g = (size_t)g_grid_cap_override;
    if (g < 1) g = 1;
    const size_t lds = PHLayout<PL>::lds_bytes((int)waves, SUMS);
    PHTables T{reinterpret_cast<const cx *>(D.p_t1), reinterpret_cast<const cx *>(D.p_t2),
               reinterpret_cast<const cx *>(D.p_t2) + PL::T2_ENTRIES};
    THZ_LAUNCH((k_ph<PL, kPipe, CM, SUMS>), (unsigned)g, waves * kWave, lds, nullptr, A, T);
    return g;
}

template <class PL>
static size_t ph_variant(const PlanDev &D, FBArgs &A)
{
    if (A.cmask && A.sum_partial) return ph_launch<PL, true, true>(D, A);
    if (A.sum_partial) return ph_launch<PL, false, true>(D, A);
    if (A.cmask) return ph_launch<PL, true, false>(D, A);
    return ph_launch<PL, false, false>(D, A);
}

template <class PL>
static size_t ph_rows(size_t npix)
{
    const unsigned waves = (unsigned)PHLayout<PL>::waves(true);
    size_t g = (npix + waves - 1) / waves;
    if (g > (size_t)kNumCU) g = kNumCU;
    if (g_grid_cap_override > 0 && g > (size_t)g_grid_cap_override) g = (size_t)g_grid_cap_override;
    return g < 1 ? 1 : g;
}

extern "C" {

// waves per block of the PH kernel of an nt-sample plan, with or without the in-launch sums; -2: not a PH plan
int emu_ph_waves(int nt, int sums)
{
    PlanHost H;
    if (!build_plan((size_t)nt, H, true, true) || !H.half_n) return -2;
    switch (H.half_n) {
    case 1001: return PHLayout<PPlan1001>::waves(sums != 0);
    case 1200: return PHLayout<PPlan1200>::waves(sums != 0);
    case 1500: return PHLayout<PPlan1500>::waves(sums != 0);
    case 2000: return PHLayout<PPlan2000>::waves(sums != 0);
    default: return PHLayout<PPlan1000>::waves(sums != 0);
    }
}

// One launch of k_ph<P, kPipe, CM, SUMS> for an nt-sample PH plan: CM when cmask is given, SUMS when sums (2 nf) is.
// direct != 0: the kernel is launched here by name; 0: through launch_pipeline, as thz_pipeline_ex issues it (its
// routing and pipeline_sum_rows are then part of what is checked).  The partial rows are added up in row order in
// double (launch_sum_rows_f64).  Returns the number of partial rows (0 without sums); -2 not a PH plan, -3 the plan
// offers no in-launch sums, -4 a partial-row entry was left unwritten, -5 the two row counts disagree.
int emu_ph_chain(int nt, size_t npix, int direct, const float *raw, const float *pre, const float *mask, const float *cmask,
                 const float *post, float *fft, float *amp, float *ph, float *out, float *img, float *sums)
{
    PlanHost H;
    if (!build_plan((size_t)nt, H, true, true) || !H.half_n) return -2;
    PlanDev D = ph_plan(H);
    const size_t nf = (size_t)D.nf;
    size_t rows = 0;
    if (sums) {
        rows = pipeline_sum_rows(D, npix, cmask != nullptr);
        if (rows == 0) return -3;
    }
    std::vector<float> partial(rows * 2 * nf, kSentinel);  // every entry must be written by the kernel
    float *part = rows ? partial.data() : nullptr;
    if (direct) {
        FBArgs A{};
        A.npix = npix; A.nt = D.nt; A.nf = D.nf; A.in = raw; A.pre_win = pre; A.mask = mask ? mask : D.ones; A.post_win = post;
        A.fft_out = reinterpret_cast<cx *>(fft); A.amp_out = amp; A.ph_out = ph; A.data_out = out; A.img = img;
        A.cmask = reinterpret_cast<const cx *>(cmask);
        A.sum_partial = part;
        size_t g = 0, want = 0;
        switch (H.half_n) {
        case 1001: g = ph_variant<PPlan1001>(D, A); want = ph_rows<PPlan1001>(npix); break;
        case 1200: g = ph_variant<PPlan1200>(D, A); want = ph_rows<PPlan1200>(npix); break;
        case 1500: g = ph_variant<PPlan1500>(D, A); want = ph_rows<PPlan1500>(npix); break;
        case 2000: g = ph_variant<PPlan2000>(D, A); want = ph_rows<PPlan2000>(npix); break;
        default: g = ph_variant<PPlan1000>(D, A); want = ph_rows<PPlan1000>(npix); break;
        }
        if (sums && (g != rows || want != rows)) return -5;
    } else {
        launch_pipeline(nullptr, D, npix, raw, pre, mask, post, (c32 *)fft, amp, ph, out, img, (const c32 *)cmask, part);
    }
    for (float v : partial)
        if (v == kSentinel) return -4;
    if (rows) launch_sum_rows_f64(nullptr, partial.data(), rows, 2 * nf, sums);
    return (int)rows;
}
}
