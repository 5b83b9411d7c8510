// pca_host.cpp — thz_host_pca_components (include/thzgpu.h, "Principal components of a scan"): the leading eigenpairs
// of a covariance matrix in plain f64 C++, no GPU, no context, no LAPACK.
//
// Householder reduction to tridiagonal form with the transformations accumulated, then implicit QL with Wilkinson
// shifts (the EISPACK pair tred2 / tql2 as Wilkinson & Reinsch, Handbook for Automatic Computation II, give them):
// O(L^3), backward stable, and a fraction of a second at L = 512 where cyclic Jacobi takes several.  The QL sweeps of
// one eigenvalue are counted, so the call returns on any input.
#include "../../include/thzgpu.h"

#include <algorithm>
#include <cmath>
#include <numeric>
#include <vector>

namespace {

// a: n x n symmetric, row-major; on return row-major Q with a = Q T Q^T, T = tridiag(e[1..n-1], d, e[1..n-1])
void tridiagonalise(std::vector<double> &a, int n, std::vector<double> &d, std::vector<double> &e)
{
    auto V = [&](int r, int c) -> double & { return a[(size_t)r * (size_t)n + (size_t)c]; };
    for (int j = 0; j < n; ++j) d[j] = V(n - 1, j);
    for (int i = n - 1; i > 0; --i) {
        double scale = 0.0, h = 0.0;
        for (int k = 0; k < i; ++k) scale += std::fabs(d[k]);
        if (scale == 0.0) {
            e[i] = d[i - 1];
            for (int j = 0; j < i; ++j) {
                d[j] = V(i - 1, j);
                V(i, j) = 0.0;
                V(j, i) = 0.0;
            }
        } else {
            for (int k = 0; k < i; ++k) {
                d[k] /= scale;
                h += d[k] * d[k];
            }
            double f = d[i - 1];
            double g = std::sqrt(h);
            if (f > 0.0) g = -g;
            e[i] = scale * g;
            h -= f * g;
            d[i - 1] = f - g;
            for (int j = 0; j < i; ++j) e[j] = 0.0;
            for (int j = 0; j < i; ++j) {
                f = d[j];
                V(j, i) = f;
                g = e[j] + V(j, j) * f;
                for (int k = j + 1; k <= i - 1; ++k) {
                    g += V(k, j) * d[k];
                    e[k] += V(k, j) * f;
                }
                e[j] = g;
            }
            f = 0.0;
            for (int j = 0; j < i; ++j) {
                e[j] /= h;
                f += e[j] * d[j];
            }
            const double hh = f / (h + h);
            for (int j = 0; j < i; ++j) e[j] -= hh * d[j];
            for (int j = 0; j < i; ++j) {
                f = d[j];
                g = e[j];
                for (int k = j; k <= i - 1; ++k) V(k, j) -= f * e[k] + g * d[k];
                d[j] = V(i - 1, j);
                V(i, j) = 0.0;
            }
        }
        d[i] = h;
    }
    for (int i = 0; i < n - 1; ++i) {
        V(n - 1, i) = V(i, i);
        V(i, i) = 1.0;
        const double h = d[i + 1];
        if (h != 0.0) {
            for (int k = 0; k <= i; ++k) d[k] = V(k, i + 1) / h;
            for (int j = 0; j <= i; ++j) {
                double g = 0.0;
                for (int k = 0; k <= i; ++k) g += V(k, i + 1) * V(k, j);
                for (int k = 0; k <= i; ++k) V(k, j) -= g * d[k];
            }
        }
        for (int k = 0; k <= i; ++k) V(k, i + 1) = 0.0;
    }
    for (int j = 0; j < n; ++j) {
        d[j] = V(n - 1, j);
        V(n - 1, j) = 0.0;
    }
    V(n - 1, n - 1) = 1.0;
    e[0] = 0.0;
}

// zt: Q transposed (row r = column r of Q), so that a rotation of two columns of Q runs over two contiguous rows.
// On return d holds the eigenvalues and row r of zt the eigenvector of d[r].  false: an eigenvalue took more than
// kSweeps QL sweeps (non-finite intermediate values; a finite symmetric matrix needs a handful)
bool implicit_ql(std::vector<double> &zt, int n, std::vector<double> &d, std::vector<double> &e)
{
    constexpr int kSweeps = 64;
    for (int i = 1; i < n; ++i) e[i - 1] = e[i];
    e[n - 1] = 0.0;
    double f = 0.0, tst1 = 0.0;
    const double eps = std::ldexp(1.0, -52);
    for (int l = 0; l < n; ++l) {
        tst1 = std::max(tst1, std::fabs(d[l]) + std::fabs(e[l]));
        int m = l;
        while (m < n - 1 && !(std::fabs(e[m]) <= eps * tst1)) ++m;
        if (m > l) {
            int sweeps = 0;
            do {
                if (++sweeps > kSweeps) return false;
                double g = d[l];
                double p = (d[l + 1] - g) / (2.0 * e[l]);
                double r = std::hypot(p, 1.0);
                if (p < 0.0) r = -r;
                d[l] = e[l] / (p + r);
                d[l + 1] = e[l] * (p + r);
                const double dl1 = d[l + 1];
                double h = g - d[l];
                for (int i = l + 2; i < n; ++i) d[i] -= h;
                f += h;
                p = d[m];
                double c = 1.0, c2 = c, c3 = c;
                const double el1 = e[l + 1];
                double s = 0.0, s2 = 0.0;
                for (int i = m - 1; i >= l; --i) {
                    c3 = c2;
                    c2 = c;
                    s2 = s;
                    g = c * e[i];
                    h = c * p;
                    r = std::hypot(p, e[i]);
                    e[i + 1] = s * r;
                    s = e[i] / r;
                    c = p / r;
                    p = c * d[i] - s * g;
                    d[i + 1] = h + s * (c * g + s * d[i]);
                    double *z0 = zt.data() + (size_t)i * (size_t)n, *z1 = z0 + n;
                    for (int k = 0; k < n; ++k) {
                        const double hk = z1[k];
                        z1[k] = s * z0[k] + c * hk;
                        z0[k] = c * z0[k] - s * hk;
                    }
                }
                p = -s * s2 * c3 * el1 * e[l] / dl1;
                e[l] = s * p;
                d[l] = c * p;
            } while (std::fabs(e[l]) > eps * tst1);
        }
        d[l] += f;
        e[l] = 0.0;
    }
    return true;
}

}  // namespace

extern "C" int thz_host_pca_components(const double *gram, size_t L, uint64_t count, int K, float *components,
                                       double *eigenvalues, double *total_variance)
{
    if (!gram || !components || !eigenvalues || L < 1 || L > THZ_PCA_MAX_LEN || count < 2 || K < 1
        || K > THZ_PCA_MAX_COMPONENTS || (size_t)K > L)
        return THZ_ERR_INVALID;
    const int n = (int)L;
    const double div = (double)(count - 1);
    std::vector<double> a((size_t)n * (size_t)n);
    double biggest = 0.0, trace = 0.0;
    for (size_t i = 0; i < a.size(); ++i) {
        if (!std::isfinite(gram[i])) return THZ_ERR_INVALID;
        a[i] = gram[i] / div;
        biggest = std::max(biggest, std::fabs(a[i]));
    }
    for (int i = 0; i < n; ++i) trace += a[(size_t)i * (size_t)n + (size_t)i];
    if (total_variance) *total_variance = trace;
    // a power of two takes the matrix to O(1): exact, and the squares of the reduction cannot overflow
    int ex = 0;
    if (biggest > 0.0) (void)std::frexp(biggest, &ex);
    for (double &x : a) x = std::ldexp(x, -ex);
    // the upper triangle is what the caller computed; the reduction reads the lower one: one matrix either way when
    // the input is symmetric, the mean of the two otherwise
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < i; ++j) {
            const double m = 0.5 * (a[(size_t)i * n + j] + a[(size_t)j * n + i]);
            a[(size_t)i * n + j] = a[(size_t)j * n + i] = m;
        }
    std::vector<double> d((size_t)n), e((size_t)n), zt((size_t)n * (size_t)n);
    tridiagonalise(a, n, d, e);
    for (int r = 0; r < n; ++r)
        for (int c = 0; c < n; ++c) zt[(size_t)c * n + r] = a[(size_t)r * n + c];
    if (!implicit_ql(zt, n, d, e)) return THZ_ERR_INVALID;
    std::vector<int> order((size_t)n);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return d[x] > d[y]; });
    for (int c = 0; c < K; ++c) {
        const double *v = zt.data() + (size_t)order[(size_t)c] * (size_t)n;
        double norm = 0.0;
        for (int j = 0; j < n; ++j) norm += v[j] * v[j];
        norm = std::sqrt(norm);
        if (!(std::isfinite(d[order[(size_t)c]]) && std::isfinite(norm) && norm > 0.0)) return THZ_ERR_INVALID;
        // the sign: the entry of largest magnitude is positive, the lowest index winning a tie — magnitudes compared as
        // they round to f32, so that a tie in exact arithmetic is a tie here whatever the last bits of the f64 vector
        int top = 0;
        float top_mag = -1.0f;
        for (int j = 0; j < n; ++j) {
            const float mag = std::fabs((float)(v[j] / norm));
            if (mag > top_mag) {
                top_mag = mag;
                top = j;
            }
        }
        const double sign = v[top] < 0.0 ? -1.0 : 1.0;
        for (int j = 0; j < n; ++j) components[(size_t)c * L + (size_t)j] = (float)(sign * v[j] / norm);
        eigenvalues[c] = std::ldexp(d[order[(size_t)c]], ex);
    }
    return THZ_OK;
}
