// tsan_fbp_driver.cpp — runs the emulated FBP kernels (fft_fbp.hpp: chirp-z over the mixed-radix core, the lengths
// of a tilted 1001-sample scan) under a sanitizer, every lane a host thread.  TEST INFRASTRUCTURE ONLY; built and run
// by tests/test_sanitizers_tilted.py the way tests/emu/run_tsan.sh builds tsan_driver.cpp.
#include <cstdint>
#include <cstdio>
#include <vector>

extern "C" {
int emu_family(int nt);
int emu_fft_fwd(int nt, size_t npix, const float *in, const float *wa, const float *wb, float *data_out, float *fft,
                float *amp, float *ph, const float *mask);
int emu_fft_inv(int nt, size_t npix, const float *fft, const float *win, float *out, float *img);
int emu_pipeline(int nt, size_t npix, const float *raw, const float *pre, const float *mask, const float *post,
                 float *fft, float *amp, float *ph, float *out, float *img);
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

// the fused chain, then the forward stage (two windows and the windowed-trace output) and the inverse stage
static int chain(int nt, size_t npix)
{
    if (emu_family(nt) != 7) {
        std::printf("nt=%d is not planned for the FBP kernels\n", nt);
        return 1;
    }
    const size_t nf = (size_t)nt / 2 + 1;
    auto x = noise(npix * nt, (unsigned)nt);
    auto pre = noise((size_t)nt, 1, 0.5f, 1.0f), pre2 = noise((size_t)nt, 4, 0.5f, 1.0f), post = noise((size_t)nt, 2, 0.5f, 1.0f),
         mask = noise(nf, 3, 0.0f, 1.0f);
    std::vector<float> fft(npix * nf * 2), amp(npix * nf), ph(npix * nf), out(npix * nt), img(npix), dat(npix * nt);
    int rc = emu_pipeline(nt, npix, x.data(), pre.data(), mask.data(), post.data(), fft.data(), amp.data(), ph.data(), out.data(),
                          img.data());
    rc |= emu_fft_fwd(nt, npix, x.data(), pre.data(), pre2.data(), dat.data(), fft.data(), amp.data(), ph.data(), mask.data());
    rc |= emu_fft_inv(nt, npix, fft.data(), post.data(), out.data(), img.data());
    std::printf("fbp chain nt=%d npix=%zu rc=%d done\n", nt, npix, rc);
    std::fflush(stdout);
    return rc;
}

int main()
{
    emu_allow_f(1);
    emu_allow_p(1);
    // an odd trace count (the last pair has one member), more pairs than a block has waves (7 at M = 2304, 6 at 2560),
    // and the longest trace of each convolution length
    int rc = chain(1101, 17) | chain(1201, 15) | chain(1152, 3) | chain(1280, 2);
    std::printf("fbp driver finished rc=%d\n", rc);
    return rc;
}
