// wavelet_host_driver.cpp — csrc/wavelet_host.cpp under AddressSanitizer + UBSan (tests/test_wavelet_host.py builds it
// with -fsanitize=address,undefined and runs it as a plain executable): thz_host_wavelet_trace over the whole range of
// taps, levels and trace lengths, the corner J = 6, nt = 4608 included, and the two helpers, every array on the heap with
// exactly the documented size, so that an index past nt, Lf or J is a report.  No HIP runtime, no GPU.
#include "../../include/thzgpu.h"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#define CHECK(cond, what)                                               \
    do {                                                                \
        if (!(cond)) {                                                  \
            std::printf("FAILED %s (line %d)\n", what, __LINE__);       \
            return 1;                                                   \
        }                                                               \
    } while (0)

namespace {

uint32_t state = 12345u;
float rnd()  // in [-1, 1)
{
    state = state * 1664525u + 1013904223u;
    return (float)(state >> 8) / 8388608.0f - 1.0f;
}

}  // namespace

int main()
{
    const size_t lengths[] = {1, 2, 3, 7, 63, 64, 65, 1001, 4096, THZ_WAVELET_MAX_NT};
    for (int Lf = 1; Lf <= THZ_WAVELET_MAX_TAPS; ++Lf)
        for (int J = 1; J <= THZ_WAVELET_MAX_LEVELS; ++J)
            for (size_t nt : lengths) {
                if ((size_t)(J + 2) * nt > THZ_WAVELET_MAX_WORDS) continue;
                if (nt > 1001 && Lf != 1 && Lf != 8 && Lf != THZ_WAVELET_MAX_TAPS) continue;  // the long traces at three tap counts
                std::vector<float> y(nt), x(nt), hn((size_t)Lf), gn((size_t)Lf), scale((size_t)J);
                for (float &v : y) v = rnd();
                for (float &v : hn) v = rnd();
                for (float &v : gn) v = rnd();
                for (float &v : scale) v = 0.5f * (rnd() + 1.0f);
                for (int mode = 0; mode < 4; ++mode) {
                    const thz_wavelet_cfg cfg{Lf, J, mode & 1, mode >> 1};
                    float sigma = -1.0f;
                    int32_t kept = -1;
                    CHECK(thz_host_wavelet_trace(y.data(), nt, hn.data(), gn.data(), scale.data(), &cfg, x.data(), &sigma, &kept) == THZ_OK, "trace");
                    CHECK(sigma >= 0.0f && kept >= 0 && (size_t)kept <= (size_t)J * nt, "sigma and kept");
                    for (float v : x) CHECK(std::isfinite(v), "a finite output");
                }
                const thz_wavelet_cfg cfg{Lf, J, 0, 0};
                CHECK(thz_host_wavelet_trace(y.data(), nt, hn.data(), gn.data(), scale.data(), &cfg, y.data(), nullptr, nullptr) == THZ_OK, "in place");
                // a non-finite sample stays inside its own arrays
                y[nt / 2] = std::numeric_limits<float>::quiet_NaN();
                y[0] = std::numeric_limits<float>::infinity();
                CHECK(thz_host_wavelet_trace(y.data(), nt, hn.data(), gn.data(), scale.data(), &cfg, x.data(), nullptr, nullptr) == THZ_OK, "a non-finite trace");
            }
    CHECK((size_t)(THZ_WAVELET_MAX_LEVELS + 2) * THZ_WAVELET_MAX_NT == THZ_WAVELET_MAX_WORDS, "the corner is the limit");
    // the helpers, into arrays of exactly 2 * order and n_levels entries
    for (int order = 1; order <= 4; ++order) {
        std::vector<float> hn((size_t)(2 * order)), gn((size_t)(2 * order));
        int n = 0;
        CHECK(thz_host_wavelet_filter(order, hn.data(), gn.data(), &n) == THZ_OK && n == 2 * order, "filter");
        double sum = 0.0;
        for (float v : hn) sum += v;
        CHECK(std::fabs(sum - 1.0) < 1e-6, "hn sums to 1");
    }
    for (int J = 1; J <= THZ_WAVELET_MAX_LEVELS; ++J) {
        std::vector<float> scale((size_t)J);
        CHECK(thz_host_wavelet_universal(1001, J, scale.data()) == THZ_OK && scale[(size_t)J - 1] > 0.0f, "universal");
        CHECK(thz_host_wavelet_universal(1, J, scale.data()) == THZ_OK && scale[0] == 0.0f, "universal of one sample");
    }
    // refusals write nothing
    std::vector<float> one(1, 1.0f);
    int n = 0;
    const thz_wavelet_cfg ok{1, 1, 0, 0}, taps17{THZ_WAVELET_MAX_TAPS + 1, 1, 0, 0}, levels7{1, THZ_WAVELET_MAX_LEVELS + 1, 0, 0};
    CHECK(thz_host_wavelet_trace(one.data(), 1, one.data(), one.data(), one.data(), &ok, one.data(), nullptr, nullptr) == THZ_OK, "the smallest call");
    CHECK(thz_host_wavelet_trace(one.data(), 1, one.data(), one.data(), one.data(), &taps17, one.data(), nullptr, nullptr) == THZ_ERR_INVALID, "17 taps");
    CHECK(thz_host_wavelet_trace(one.data(), 1, one.data(), one.data(), one.data(), &levels7, one.data(), nullptr, nullptr) == THZ_ERR_INVALID, "7 levels");
    CHECK(thz_host_wavelet_trace(one.data(), 0, one.data(), one.data(), one.data(), &ok, one.data(), nullptr, nullptr) == THZ_ERR_INVALID, "nt = 0");
    CHECK(thz_host_wavelet_trace(one.data(), THZ_WAVELET_MAX_NT + 1, one.data(), one.data(), one.data(), &ok, one.data(), nullptr, nullptr) == THZ_ERR_INVALID, "nt = 4609");
    CHECK(thz_host_wavelet_filter(0, one.data(), one.data(), &n) == THZ_ERR_INVALID, "order 0");
    CHECK(thz_host_wavelet_filter(5, one.data(), one.data(), &n) == THZ_ERR_INVALID, "order 5");
    CHECK(thz_host_wavelet_universal(0, 1, one.data()) == THZ_ERR_INVALID, "universal of no sample");
    CHECK(thz_host_wavelet_universal(8, THZ_WAVELET_MAX_LEVELS + 1, one.data()) == THZ_ERR_INVALID, "universal of 7 levels");
    std::printf("wavelet_host done\n");
    return 0;
}
