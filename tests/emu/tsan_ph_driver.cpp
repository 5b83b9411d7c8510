// tsan_ph_driver.cpp — runs the emulated half-length chain with its extras (fft_ph.hpp: k_ph<P, kPipe, CM, SUMS>: the
// complex multiplier and the ticket-ordered pixel sums) under a sanitizer, every lane a host thread.  TEST
// INFRASTRUCTURE ONLY; built and run by tests/test_sanitizers_ph_chain.py.
#include <cstdint>
#include <cstdio>
#include <vector>

extern "C" {
int emu_half_n(int nt);
int emu_ph_chain(int nt, size_t npix, int direct, const float *raw, const float *pre, const float *mask, const float *cmask,
                 const float *post, float *fft, float *amp, float *ph, float *out, float *img, float *sums);
void emu_allow_f(int on);
void emu_allow_p(int on);
void emu_set_grid_cap(int blocks);
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

// the cmask + sums variant on npix traces of nt samples; grid_cap blocks at the most (0: as many as the launcher takes)
static int chain(int nt, size_t npix, int grid_cap)
{
    if (emu_half_n(nt) != nt / 2) {
        std::printf("nt=%d is not planned for the PH kernels\n", nt);
        return 1;
    }
    const size_t nf = (size_t)nt / 2 + 1;
    auto raw = noise(npix * nt, (unsigned)nt + 1);
    auto pre = noise((size_t)nt, 1, 0.5f, 1.0f), post = noise((size_t)nt, 2, 0.5f, 1.0f), mask = noise(nf, 3, 0.0f, 1.0f),
         cmask = noise(2 * nf, 4);
    std::vector<float> fft(npix * nf * 2), amp(npix * nf), ph(npix * nf), out(npix * nt), img(npix), sums(2 * nf);
    emu_set_grid_cap(grid_cap);
    const int rc = emu_ph_chain(nt, npix, 1, raw.data(), pre.data(), mask.data(), cmask.data(), post.data(), fft.data(), amp.data(),
                                ph.data(), out.data(), img.data(), sums.data());
    emu_set_grid_cap(0);
    const int bad = rc <= 0 ? 1 : 0;
    std::printf("ph chain nt=%d npix=%zu rows=%d rc=%d done\n", nt, npix, rc, bad);
    std::fflush(stdout);
    return bad;
}

int main()
{
    emu_allow_f(1);
    emu_allow_p(1);
    // one block of sixteen waves over 19 traces: two trips, the second ragged (N odd: the inverse's last entry too);
    // ten traces on two blocks of eight waves, the second with two
    int rc = chain(2002, 19, 1) | chain(4000, 10, 0);
    std::printf("ph driver finished rc=%d\n", rc);
    return rc;
}
