// unmix_host_driver.cpp — csrc/unmix_host.cpp under AddressSanitizer + UBSan (tests/test_unmix_host.py builds it with
// -fsanitize=address,undefined and runs it as a plain executable): thz_host_unmix_prepare and thz_host_unmix_solve over
// the whole K range, every array on the heap with exactly the documented size, so that an index past K x L, K x K or K
// is a report.  No HIP runtime, no GPU.
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
float rnd()  // in [0, 1)
{
    state = state * 1664525u + 1013904223u;
    return (float)(state >> 8) / 16777216.0f;
}

}  // namespace

int main()
{
    const size_t lengths[] = {1, 63, 64, 65, THZ_PCA_MAX_LEN};
    const int sweeps[] = {0, 1, 64, THZ_UNMIX_MAX_SWEEPS};
    for (int K = 1; K <= THZ_UNMIX_MAX; ++K)
        for (size_t L : lengths) {
            std::vector<float> e((size_t)K * L), G((size_t)K * K), rd((size_t)K), b((size_t)K), a((size_t)K);
            for (float &v : e) v = rnd() + 0.05f;
            CHECK(thz_host_unmix_prepare(e.data(), K, L, G.data(), rd.data()) == THZ_OK, "prepare");
            for (int i = 0; i < K; ++i) {
                CHECK(rd[(size_t)i] > 0.0f && std::isfinite(rd[(size_t)i]), "rd");
                for (int c = 0; c < K; ++c) CHECK(G[(size_t)(i * K + c)] == G[(size_t)(c * K + i)], "G is symmetric");
            }
            for (int n : sweeps) {
                for (float &v : b) v = 10.0f * rnd() - 3.0f;
                float kkt = -1.0f;
                CHECK(thz_host_unmix_solve(b.data(), G.data(), rd.data(), K, n, a.data(), &kkt) == THZ_OK, "solve");
                CHECK(kkt >= 0.0f, "kkt");
                for (float v : a) CHECK(v >= 0.0f && std::isfinite(v), "abundance");
                CHECK(thz_host_unmix_solve(b.data(), G.data(), rd.data(), K, n, a.data(), nullptr) == THZ_OK, "solve without kkt");
            }
            // a non-finite projection stays inside its own arrays
            b[0] = std::numeric_limits<float>::quiet_NaN();
            b[(size_t)K - 1] = std::numeric_limits<float>::infinity();
            float kkt = 0.0f;
            CHECK(thz_host_unmix_solve(b.data(), G.data(), rd.data(), K, 8, a.data(), &kkt) == THZ_OK, "solve of a non-finite row");
            // refusals write nothing
            e[(size_t)K * L - 1] = std::numeric_limits<float>::infinity();
            CHECK(thz_host_unmix_prepare(e.data(), K, L, G.data(), rd.data()) == THZ_ERR_INVALID, "a non-finite endmember");
            for (size_t j = 0; j < L; ++j) e[(size_t)(K - 1) * L + j] = 0.0f;
            CHECK(thz_host_unmix_prepare(e.data(), K, L, G.data(), rd.data()) == THZ_ERR_INVALID, "a zero endmember");
        }
    std::vector<float> one(1, 1.0f);
    CHECK(thz_host_unmix_prepare(one.data(), 0, 1, one.data(), one.data()) == THZ_ERR_INVALID, "K = 0");
    CHECK(thz_host_unmix_prepare(one.data(), THZ_UNMIX_MAX + 1, 1, one.data(), one.data()) == THZ_ERR_INVALID, "K = 17");
    CHECK(thz_host_unmix_prepare(one.data(), 1, THZ_PCA_MAX_LEN + 1, one.data(), one.data()) == THZ_ERR_INVALID, "L = 513");
    CHECK(thz_host_unmix_prepare(nullptr, 1, 1, one.data(), one.data()) == THZ_ERR_INVALID, "NULL endmembers");
    CHECK(thz_host_unmix_solve(one.data(), one.data(), one.data(), 1, THZ_UNMIX_MAX_SWEEPS + 1, one.data(), nullptr) == THZ_ERR_INVALID,
          "too many sweeps");
    CHECK(thz_host_unmix_solve(one.data(), one.data(), one.data(), THZ_UNMIX_MAX + 1, 1, one.data(), nullptr) == THZ_ERR_INVALID, "K = 17");
    std::printf("unmix_host done\n");
    return 0;
}
