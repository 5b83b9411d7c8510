// tsan_tilted_driver.cpp — runs the emulated tilted chain (fft_fbp.hpp: k_fbp<kPipe, TILT, CM, SUMS>, and the small
// pass that sums the re-laid source traces) under a sanitizer, every lane a host thread.  TEST INFRASTRUCTURE ONLY;
// built and run by tests/test_sanitizers_tilted_chain.py the way tests/test_sanitizers_tilted.py runs its driver.
#include <cstdint>
#include <cstdio>
#include <vector>

extern "C" {
int emu_family(int nt);
int emu_fbp_chain(int nt, size_t npix, const float *raw, const float *src, int nt_in, const float *taper, const int *ins,
                  const float *pre, const float *mask, const float *cmask, const float *post, float *fft, float *amp,
                  float *ph, float *out, float *img, float *sums, float *src_sum);
void emu_allow_f(int on);
void emu_allow_p(int on);
}

static std::vector<float> noise(size_t n, unsigned seed, float lo = -1.0f, float hi = 1.0f)
{
    std::vector<float> v(n);
    uint32_t s = seed * 2654435761u + 12345u;
    for (size_t i = 0; i < n; ++i) {
        s = s * 1664525u + 1013904223u;
        v[i] = lo + (hi - lo) * (float)(s >> 8) / 16777216.0f;
    }
    return v;
}

// 1001-sample traces re-laid on nt samples, every pixel with an insert index of its own (the first at 0, the last at
// the largest one), complex multiplier, pixel sums and the source sum; then the un-tilted chain with the same extras
static int chain(int nt, size_t npix)
{
    if (emu_family(nt) != 7) {
        std::printf("nt=%d is not planned for the FBP kernels\n", nt);
        return 1;
    }
    const int nt_in = 1001;
    const size_t nf = (size_t)nt / 2 + 1;
    auto x = noise(npix * nt_in, (unsigned)nt), raw = noise(npix * nt, (unsigned)nt + 1);
    auto taper = noise((size_t)nt_in, 5, 0.0f, 1.0f), pre = noise((size_t)nt, 1, 0.5f, 1.0f), post = noise((size_t)nt, 2, 0.5f, 1.0f),
         mask = noise(nf, 3, 0.0f, 1.0f), cmask = noise(2 * nf, 4);
    std::vector<int> ins(npix);
    for (size_t p = 0; p < npix; ++p) ins[p] = npix > 1 ? (int)((size_t)(nt - nt_in) * p / (npix - 1)) : nt - nt_in;
    std::vector<float> fft(npix * nf * 2), amp(npix * nf), ph(npix * nf), out(npix * nt), img(npix), sums(2 * nf), ssum((size_t)nt);
    int rc = emu_fbp_chain(nt, npix, nullptr, x.data(), nt_in, taper.data(), ins.data(), pre.data(), mask.data(), cmask.data(),
                           post.data(), fft.data(), amp.data(), ph.data(), out.data(), img.data(), sums.data(), ssum.data());
    int rc2 = emu_fbp_chain(nt, npix, raw.data(), nullptr, 0, nullptr, nullptr, pre.data(), mask.data(), cmask.data(), post.data(),
                            fft.data(), amp.data(), ph.data(), out.data(), img.data(), sums.data(), nullptr);
    const int bad = (rc <= 0 || rc2 <= 0) ? 1 : 0;
    std::printf("tilted chain nt=%d npix=%zu rows=%d/%d rc=%d done\n", nt, npix, rc, rc2, bad);
    std::fflush(stdout);
    return bad;
}

int main()
{
    emu_allow_f(1);
    emu_allow_p(1);
    // an odd trace count (the last pair has one member), more pairs than a block has waves (7 at M = 2304, 6 at 2560),
    // and the longest trace of each convolution length
    int rc = chain(1101, 17) | chain(1201, 15) | chain(1152, 3) | chain(1280, 2);
    std::printf("tilted driver finished rc=%d\n", rc);
    return rc;
}
