// Stand-alone program of tests/test_gpu_cx_products.py: the batched complex products of fft_f.hpp (cx_mul_batch /
// cx_mul2_batch, two packed instructions per product) against cx_mul as hipcc compiles it, bit for bit, and the batched
// routes through the R2C / C2R splits against copies of the bodies r2c_pair and c2r_swapped_pm had before the batches.
// Operands: every assignment of {+-0, +-denormal, +-Inf, NaN} to (a.x, a.y, b.x, b.y), then random values over many
// binades.  Prints one line per check and exits 1 if any bit differs (the splits: NaNs compare as NaNs, see compare()).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "fft_f.hpp"

using thz::cx;

#define CHECK(x)                                                                     \
    do {                                                                             \
        hipError_t e_ = (x);                                                         \
        if (e_ != hipSuccess) {                                                      \
            std::printf("%s: %s\n", #x, hipGetErrorString(e_));                      \
            return 2;                                                                \
        }                                                                            \
    } while (0)

// the split's bodies as they were when every product was the compiler's
__device__ __forceinline__ void r2c_pair_before(cx a, cx b, cx w2, cx &xk, cx &xn)
{
    const cx p = a + b, m = a - b;
    const cx bs = {-w2.y, w2.x};
    const cx t = m.xx * w2 + p.yy * bs;
    xk = cx{fmaf(p.x, 0.5f, t.x), fmaf(m.y, 0.5f, t.y)};
    xn = cx{fmaf(p.x, 0.5f, -t.x), fmaf(-m.y, 0.5f, t.y)};
}
__device__ __forceinline__ cx c2r_swapped_pm_before(cx p, cx m, cx wc)
{
    const cx bs = {-wc.y, wc.x};
    const cx t = m.xx * wc + p.yy * bs;
    return cx{fmaf(2.0f, t.y, m.y), fmaf(2.0f, t.x, p.x)};
}

// thread i owns the K products [K i, K i + K)
template <int K>
__global__ void k_batch(const cx *a, const cx *b, cx *got, cx *want, int n)
{
    const int i = K * (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i + K > n) return;
    cx x[K], y[K], o[K];
#pragma unroll
    for (int j = 0; j < K; ++j) {
        x[j] = a[i + j];
        y[j] = b[i + j];
    }
    thz::cx_mul_batch<K>(o, x, y);
#pragma unroll
    for (int j = 0; j < K; ++j) {
        got[i + j] = o[j];
        want[i + j] = thz::cx_mul(x[j], y[j]);
    }
}

// wave-uniform compile-time a (the compact pass 1's W_N^k1) in SGPRs
__global__ void k_batch_const_a(const cx *b, cx *got, cx *want, int n)
{
    const int i = 4 * (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i + 4 > n) return;
    cx x[4], y[4], o[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        x[j] = cx{thz::f_unit_re(j + 1, 2048), thz::f_unit_im(j + 1, 2048)};
        y[j] = b[i + j];
    }
    thz::cx_mul_batch<4, true>(o, x, y);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        got[i + j] = o[j];
        want[i + j] = thz::cx_mul(x[j], y[j]);
    }
}

// the splits, four at a time: (a, b) a pair of bins, w the split twiddle
__global__ void k_splits(const cx *a, const cx *b, const cx *w, cx *got, cx *want, int n)
{
    const int i = 4 * (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i + 4 > n) return;
    cx p[4], m[4], w4[4], t[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        p[j] = a[i + j] + b[i + j];
        m[j] = a[i + j] - b[i + j];
        w4[j] = w[i + j];
    }
    thz::cx_mul2_batch<4>(t, m, p, w4);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        cx xk, xn, xk0, xn0;
        thz::r2c_tail(p[j], m[j], t[j], xk, xn);
        r2c_pair_before(a[i + j], b[i + j], w4[j], xk0, xn0);
        got[3 * (i + j)] = xk;
        got[3 * (i + j) + 1] = xn;
        want[3 * (i + j)] = xk0;
        want[3 * (i + j) + 1] = xn0;
        got[3 * (i + j) + 2] = thz::c2r_swapped_tail(p[j], m[j], t[j]);
        want[3 * (i + j) + 2] = c2r_swapped_pm_before(p[j], m[j], w4[j]);
    }
}

// Every 32-bit word must be the same on both sides, NaNs included, with one exemption under nan_sign (the splits only):
// a word that is a NaN on BOTH sides and differs in nothing but the sign bit passes, and is counted.  In the splits
// p = a + b and m = a - b bring NaNs of both signs into one instruction, which hands on the operand it names first —
// and hipcc commutes the operands of its own multiplies from one inlining context to the next, so the compiler's form
// itself fixes such a NaN's sign no further.  Everything else fails with or without nan_sign: a NaN on one side and a
// number on the other (the NaNs sit in the same places), NaNs of different payload, numbers that differ in any bit.
static int compare(const char *what, const std::vector<cx> &got, const std::vector<cx> &want, bool nan_sign = false)
{
    size_t bad = 0, first = 0, nans = 0;
    for (size_t i = 0; i < got.size(); ++i) {
        if (std::memcmp(&got[i], &want[i], sizeof(cx)) == 0) continue;
        bool differ = false;
        for (int c = 0; c < 2; ++c) {
            const float g = c ? got[i].y : got[i].x, w = c ? want[i].y : want[i].x;
            uint32_t gb, wb;
            std::memcpy(&gb, &g, 4);
            std::memcpy(&wb, &w, 4);
            if (gb == wb) continue;
            if (nan_sign && g != g && w != w && (gb ^ wb) == 0x80000000u) ++nans;
            else differ = true;
        }
        if (differ && bad++ == 0) first = i;
    }
    if (nans) std::printf("%s: %zu words are NaNs of another sign on the two sides\n", what, nans);
    if (bad) {
        uint32_t g[2], w[2];
        std::memcpy(g, &got[first], 8);
        std::memcpy(w, &want[first], 8);
        std::printf("%s: %zu of %zu differ, first at %zu: got %08x %08x, want %08x %08x\n", what, bad, got.size(), first, g[0], g[1],
                    w[0], w[1]);
        return 1;
    }
    std::printf("%s: %zu values, same bits\n", what, got.size());
    return 0;
}

template <int K>
static int run_batch(const cx *da, const cx *db, cx *dg, cx *dw, int n)
{
    std::vector<cx> got(n), want(n);
    CHECK(hipMemset(dg, 0xff, n * sizeof(cx)));
    CHECK(hipMemset(dw, 0x00, n * sizeof(cx)));
    hipLaunchKernelGGL(k_batch<K>, dim3((n / K + 255) / 256), dim3(256), 0, 0, da, db, dg, dw, n);
    CHECK(hipDeviceSynchronize());
    CHECK(hipMemcpy(got.data(), dg, n * sizeof(cx), hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(want.data(), dw, n * sizeof(cx), hipMemcpyDeviceToHost));
    char what[32];
    std::snprintf(what, sizeof what, "cx_mul_batch<%d>", K);
    return compare(what, got, want);
}

int main()
{
    const float inf = __builtin_inff(), nan = __builtin_nanf(""), den = 1e-41f;
    const float special[7] = {0.0f, -0.0f, den, -den, inf, -inf, nan};
    constexpr int n = 240 * 28;  // a multiple of 2, 4, 5, 15 and 16
    std::vector<cx> a(n), b(n), w(n);
    int at = 0;
    for (int i = 0; i < 7; ++i)
        for (int j = 0; j < 7; ++j)
            for (int k = 0; k < 7; ++k)
                for (int l = 0; l < 7; ++l, ++at) {
                    a[at] = cx{special[i], special[j]};
                    b[at] = cx{special[k], special[l]};
                }
    std::mt19937 rng(4096);
    std::uniform_real_distribution<float> mant(-2.0f, 2.0f);
    std::uniform_int_distribution<int> expo(-60, 60);
    auto rnd = [&]() { return std::ldexp(mant(rng), expo(rng)); };
    for (; at < n; ++at) {
        a[at] = cx{rnd(), rnd()};
        b[at] = cx{rnd(), rnd()};
    }
    for (int i = 0; i < n; ++i) w[i] = i < 2401 ? b[(i * 53) % 2401] : cx{mant(rng), mant(rng)};
    cx *da, *db, *dw3, *dg, *dw;
    CHECK(hipMalloc(&da, n * sizeof(cx)));
    CHECK(hipMalloc(&db, n * sizeof(cx)));
    CHECK(hipMalloc(&dw3, n * sizeof(cx)));
    CHECK(hipMalloc(&dg, 3 * n * sizeof(cx)));
    CHECK(hipMalloc(&dw, 3 * n * sizeof(cx)));
    CHECK(hipMemcpy(da, a.data(), n * sizeof(cx), hipMemcpyHostToDevice));
    CHECK(hipMemcpy(db, b.data(), n * sizeof(cx), hipMemcpyHostToDevice));
    CHECK(hipMemcpy(dw3, w.data(), n * sizeof(cx), hipMemcpyHostToDevice));
    int rc = 0;
    rc |= run_batch<2>(da, db, dg, dw, n);
    rc |= run_batch<4>(da, db, dg, dw, n);
    rc |= run_batch<5>(da, db, dg, dw, n);
    rc |= run_batch<15>(da, db, dg, dw, n);
    rc |= run_batch<16>(da, db, dg, dw, n);
    {
        std::vector<cx> got(n), want(n);
        CHECK(hipMemset(dg, 0xff, n * sizeof(cx)));
        CHECK(hipMemset(dw, 0x00, n * sizeof(cx)));
        hipLaunchKernelGGL(k_batch_const_a, dim3((n / 4 + 255) / 256), dim3(256), 0, 0, db, dg, dw, n);
        CHECK(hipDeviceSynchronize());
        CHECK(hipMemcpy(got.data(), dg, n * sizeof(cx), hipMemcpyDeviceToHost));
        CHECK(hipMemcpy(want.data(), dw, n * sizeof(cx), hipMemcpyDeviceToHost));
        rc |= compare("cx_mul_batch<4>, a in SGPRs", got, want);
    }
    {
        std::vector<cx> got(3 * n), want(3 * n);
        CHECK(hipMemset(dg, 0xff, 3 * n * sizeof(cx)));
        CHECK(hipMemset(dw, 0x00, 3 * n * sizeof(cx)));
        hipLaunchKernelGGL(k_splits, dim3((n / 4 + 255) / 256), dim3(256), 0, 0, da, db, dw3, dg, dw, n);
        CHECK(hipDeviceSynchronize());
        CHECK(hipMemcpy(got.data(), dg, 3 * n * sizeof(cx), hipMemcpyDeviceToHost));
        CHECK(hipMemcpy(want.data(), dw, 3 * n * sizeof(cx), hipMemcpyDeviceToHost));
        rc |= compare("r2c / c2r splits through cx_mul2_batch<4>", got, want, true);
    }
    for (cx *d : {da, db, dw3, dg, dw}) CHECK(hipFree(d));
    return rc;
}
