// selftest.cpp -- native GPU self-test + micro-benchmarks for libgpk.so.
// Test infrastructure only (host references are plain C++ loops).  Built by the
// Makefile into gpk_selftest; run on the MI355X box:
//     ./gpk_selftest            correctness of every entry point vs host loops
//     ./gpk_selftest --perf     + timings (HIP events) of the hot kernels
//     ./gpk_selftest --rq       only the checks of the term kind with a shape parameter (rational quadratic)
//     ./gpk_selftest --delta    only the checks of the Delta term kind
//     ./gpk_selftest --scaled   only the checks of the kernel matrix with row and column factors (gpk_kmat_scaled), both kernels
//     ./gpk_selftest --diff     only the checks of the derivative blocks of the kernel matrix (gpk_kmat_diff)
//     ./gpk_selftest --potrf-vjp   only the checks of the VJP of the Cholesky factorisation (gpk_potrf_vjp)
//     ./gpk_selftest --nuclear-norm   only the checks of the nuclear norm by the polar iteration (gpk_nuclear_norm)
//     ./gpk_selftest --append   only the checks of the bordered Cholesky factorisation (gpk_potrf_border)
#include <hip/hip_runtime.h>
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <climits>
#include <cstring>
#include <random>
#include <string>
#include <limits>
#include <vector>
#include <atomic>
#include <functional>
#include <thread>
#include "../../include/gpk.h"

#define HIPCHK(x)                                                                       \
    do {                                                                                \
        hipError_t e = (x);                                                             \
        if (e != hipSuccess) {                                                          \
            printf("HIP error %s at %s:%d\n", hipGetErrorString(e), __FILE__, __LINE__); \
            exit(3);                                                                    \
        }                                                                               \
    } while (0)

static int g_fail = 0, g_pass = 0;
static void report(const std::string& name, double err, double tol) {
    const bool ok = (err <= tol) && std::isfinite(err);
    printf("%s %-58s err=%.3e tol=%.1e\n", ok ? "PASS" : "FAIL", name.c_str(), err, tol);
    fflush(stdout);
    if (ok) ++g_pass; else ++g_fail;
}

template <typename T> struct DT;
template <> struct DT<double> { static constexpr int v = GPK_F64; static constexpr double eps = 1e-12; static const char* name() { return "f64"; } };
template <> struct DT<float> { static constexpr int v = GPK_F32; static constexpr double eps = 2e-4; static const char* name() { return "f32"; } };

template <typename T>
struct Dev {
    T* p = nullptr;
    size_t n = 0;
    explicit Dev(size_t n_) : n(n_) { HIPCHK(hipMalloc(&p, std::max<size_t>(n, 1) * sizeof(T))); }
    ~Dev() { hipFree(p); }
    void up(const std::vector<T>& h) { HIPCHK(hipMemcpy(p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice)); }
    std::vector<T> down() const {
        std::vector<T> h(n);
        HIPCHK(hipMemcpy(h.data(), p, n * sizeof(T), hipMemcpyDeviceToHost));
        return h;
    }
    void zero() { HIPCHK(hipMemset(p, 0, n * sizeof(T))); }
};

// The host references are O(n^3) scalar loops; on one core they were 300 of the GPU suite's 510 seconds (round 6: 72 factorisations of
// order 2048 for ONE batched case).  They run on every host core now -- over the members of a batch, the rows of a column block, the
// rows under a matrix -- with every entry's summation order unchanged (same bits as the serial loops).
static void parallel_for(int n, const std::function<void(int)>& f, int grain = 1) {
    unsigned hw = std::thread::hardware_concurrency();
    const int nt = (int)std::min<unsigned>((unsigned)std::max((n + grain - 1) / grain, 1), std::min(hw ? hw : 1u, 64u));
    if (nt <= 1) {
        for (int i = 0; i < n; ++i) f(i);
        return;
    }
    std::atomic<int> next{0};
    std::vector<std::thread> th;
    th.reserve(nt);
    for (int t = 0; t < nt; ++t)
        th.emplace_back([&] {
            for (int i0 = next.fetch_add(grain); i0 < n; i0 = next.fetch_add(grain))
                for (int i = i0; i < std::min(n, i0 + grain); ++i) f(i);
        });
    for (auto& t : th) t.join();
}

static std::mt19937_64 rng(1234);
template <typename T>
static std::vector<T> randv(size_t n, double scale = 1.0) {
    std::normal_distribution<double> d(0.0, 1.0);
    std::vector<T> v(n);
    for (auto& x : v) x = (T)(scale * d(rng));
    return v;
}

template <typename T>
static double relerr(const std::vector<T>& got, const std::vector<double>& ref) {
    double num = 0, den = 0;
    for (size_t i = 0; i < ref.size(); ++i) {
        const double d = (double)got[i] - ref[i];
        if (!std::isfinite((double)got[i])) return INFINITY;
        num = std::max(num, std::fabs(d));
        den = std::max(den, std::fabs(ref[i]));
    }
    return num / std::max(den, 1e-300);
}

// ----------------------------------------------------------------------------
// MFMA layout probe (documents the lane maps the kernels rely on)
// ----------------------------------------------------------------------------
typedef double d4 __attribute__((ext_vector_type(4)));
typedef float f4 __attribute__((ext_vector_type(4)));
__global__ void probe64(const double* A, const double* B, double* C) {   // A 16x4, B 4x16 row-major
    const int l = threadIdx.x;
    d4 acc = {0, 0, 0, 0};
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(A[(l & 15) * 4 + (l >> 4)], B[(l >> 4) * 16 + (l & 15)], acc, 0, 0, 0);
    for (int i = 0; i < 4; ++i) C[((l >> 4) + 4 * i) * 16 + (l & 15)] = acc[i];
}
__global__ void probe32(const float* A, const float* B, float* C) {
    const int l = threadIdx.x;
    f4 acc = {0, 0, 0, 0};
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(A[(l & 15) * 4 + (l >> 4)], B[(l >> 4) * 16 + (l & 15)], acc, 0, 0, 0);
    for (int i = 0; i < 4; ++i) C[((l >> 4) * 4 + i) * 16 + (l & 15)] = acc[i];
}
template <typename T>
static void test_probe() {
    auto A = randv<T>(64), B = randv<T>(64);
    Dev<T> dA(64), dB(64), dC(256);
    dA.up(A); dB.up(B);
    if (sizeof(T) == 8) hipLaunchKernelGGL(probe64, dim3(1), dim3(64), 0, 0, (double*)dA.p, (double*)dB.p, (double*)dC.p);
    else hipLaunchKernelGGL(probe32, dim3(1), dim3(64), 0, 0, (float*)dA.p, (float*)dB.p, (float*)dC.p);
    HIPCHK(hipDeviceSynchronize());
    std::vector<double> ref(256, 0.0);
    for (int i = 0; i < 16; ++i) for (int j = 0; j < 16; ++j) for (int k = 0; k < 4; ++k) ref[i * 16 + j] += (double)A[i * 4 + k] * (double)B[k * 16 + j];
    report(std::string("mfma_layout_") + DT<T>::name(), relerr(dC.down(), ref), DT<T>::eps);
}

// ----------------------------------------------------------------------------
// GEMM
// ----------------------------------------------------------------------------
template <typename T>
static void test_gemm_case(bool ak, bool bk, int M, int N, int K, double alpha, double beta, int batch, bool lower, int pad) {
    const int64_t lda = (ak ? K : M) + pad, ldb = (bk ? K : N) + pad, ldc = N + pad;
    const int64_t ra = ak ? M : K, rb = bk ? N : K;
    const int64_t sA = ra * lda + 2 * pad, sB = rb * ldb + 2 * pad, sC = M * ldc + 2 * pad;
    auto A = randv<T>(sA * batch), B = randv<T>(sB * batch), C = randv<T>(sC * batch);
    Dev<T> dA(A.size()), dB(B.size()), dC(C.size());
    dA.up(A); dB.up(B); dC.up(C);
    int st = gpk_gemm(DT<T>::v, ak, bk, M, N, K, alpha, dA.p, lda, sA, dB.p, ldb, sB, beta, dC.p, ldc, sC, batch, lower, nullptr);
    HIPCHK(hipDeviceSynchronize());
    auto got = dC.down();
    std::vector<double> ref(C.begin(), C.end());
    parallel_for(batch * M, [&](int bm) {          // (one output row each)
        const int b = bm / M, m = bm % M;
        for (int n = 0; n < N; ++n) {
            if (lower && n > m) { ref[b * sC + m * ldc + n] = (double)got[b * sC + m * ldc + n]; continue; }   // above the diagonal: unspecified
            double s = 0;
            for (int k = 0; k < K; ++k) {
                const double a = ak ? A[b * sA + m * lda + k] : A[b * sA + k * lda + m];
                const double bb = bk ? B[b * sB + n * ldb + k] : B[b * sB + k * ldb + n];
                s += a * bb;
            }
            const double c0 = (beta != 0.0) ? beta * (double)C[b * sC + m * ldc + n] : 0.0;
            ref[b * sC + m * ldc + n] = alpha * s + c0;
        }
    }, 8);
    char nm[160];
    snprintf(nm, sizeof nm, "gemm_%s %c%c M%d N%d K%d a%.0f b%.0f batch%d low%d pad%d st%d", DT<T>::name(), ak ? 'k' : 'r', bk ? 'k' : 'r', M, N, K, alpha, beta, batch, (int)lower, pad, st);
    report(nm, st ? INFINITY : relerr(got, ref), DT<T>::eps * std::sqrt((double)K + 1));
}
// GPK_GEMM_TRI_K_LOWER: A (M x K, k-major) lower triangular -> same result as the full product
template <typename T>
static void test_gemm_trilow_case(bool bk, int M, int N) {
    const int K = M;
    auto A = randv<T>((size_t)M * K), B = randv<T>((size_t)(bk ? N : K) * (bk ? K : N));
    for (int m = 0; m < M; ++m) for (int k = m + 1; k < K; ++k) A[(size_t)m * K + k] = T(0);
    Dev<T> dA(A.size()), dB(B.size()), dC((size_t)M * N);
    dA.up(A); dB.up(B);
    int st = gpk_gemm(DT<T>::v, 1, bk, M, N, K, 1.0, dA.p, K, 0, dB.p, bk ? K : N, 0, 0.0, dC.p, N, 0, 1, GPK_GEMM_TRI_K_LOWER, nullptr);
    HIPCHK(hipDeviceSynchronize());
    std::vector<double> ref((size_t)M * N, 0.0);
    parallel_for(M, [&](int m) {
        for (int n = 0; n < N; ++n) {
            double s = 0;
            for (int k = 0; k <= m; ++k) s += (double)A[(size_t)m * K + k] * (double)(bk ? B[(size_t)n * K + k] : B[(size_t)k * N + n]);
            ref[(size_t)m * N + n] = s;
        }
    }, 4);
    char nm[160];
    snprintf(nm, sizeof nm, "gemm_trilow_%s k%c M%d N%d st%d", DT<T>::name(), bk ? 'k' : 'r', M, N, st);
    report(nm, st ? INFINITY : relerr(dC.down(), ref), DT<T>::eps * std::sqrt((double)K + 1));
}
// in-place use (C aliases A): P <- P W^T, the panel TRSM of the Cholesky; one workgroup per row tile
template <typename T>
static void test_gemm_inplace_case(int M, int64_t lda, int batch) {
    const int N = 128, K = 128;
    const int64_t sA = (int64_t)M * lda;
    auto A = randv<T>((size_t)sA * batch), W = randv<T>((size_t)N * K);
    Dev<T> dA(A.size()), dW(W.size());
    dA.up(A); dW.up(W);
    int st = gpk_gemm(DT<T>::v, 1, 1, M, N, K, 1.0, dA.p, lda, sA, dW.p, K, 0, 0.0, dA.p, lda, sA, batch, 0, nullptr);
    HIPCHK(hipDeviceSynchronize());
    auto got = dA.down();
    std::vector<double> ref(A.begin(), A.end());
    parallel_for(batch * M, [&](int bm) {
        const int b = bm / M, m = bm % M;
        for (int n = 0; n < N; ++n) {
            double s = 0;
            for (int k = 0; k < K; ++k) s += (double)A[b * sA + m * lda + k] * (double)W[(size_t)n * K + k];
            ref[b * sA + m * lda + n] = s;
        }
    }, 64);
    char nm[160];
    snprintf(nm, sizeof nm, "gemm_inplace_%s M%d lda%d batch%d st%d", DT<T>::name(), M, (int)lda, batch, st);
    report(nm, st ? INFINITY : relerr(got, ref), DT<T>::eps * 12);
}
template <typename T>
static void test_gemm() {
    test_gemm_inplace_case<T>(15360, 256, 1);       // 64 x 128 per workgroup (two column tiles)
    test_gemm_inplace_case<T>(3001, 131, 1);        // ragged, unaligned
    test_gemm_inplace_case<T>(1920, 130, 80);       // 128-tile path (>= 1024 tiles)
    test_gemm_trilow_case<T>(false, 512, 2048);     // 64x64 tiles
    test_gemm_trilow_case<T>(false, 300, 70);       // ragged
    test_gemm_trilow_case<T>(true, 1024, 256);
    test_gemm_trilow_case<T>(false, 1024, 8192 + 64);   // 128x128 tiles (>= 1024 of them), ragged edge
    for (int ak = 0; ak < 2; ++ak)
        for (int bk = 0; bk < 2; ++bk) {
            test_gemm_case<T>(ak, bk, 128, 128, 128, 1, 0, 1, false, 0);
            test_gemm_case<T>(ak, bk, 256, 384, 64, -1, 1, 2, false, 0);
            test_gemm_case<T>(ak, bk, 100, 70, 37, 1, 1, 1, false, 0);
            test_gemm_case<T>(ak, bk, 300, 200, 150, -1, 0, 3, false, 1);
        }
    // an empty contraction (K = 0): C = beta C, and no spinning k loop -- whole tiles on purpose (the kernels without
    // bounds checks run at least one chunk), lda = ldb = pad keeps the leading dimensions legal
    test_gemm_case<T>(true, true, 128, 128, 0, 1, 1, 1, false, 4);
    test_gemm_case<T>(true, false, 256, 128, 0, 1, 0, 2, false, 4);
    test_gemm_case<T>(true, true, 1024, 1024, 0, -1, 1, 1, false, 4);
    test_gemm_case<T>(true, true, 1024, 1024, 8, -1, 1, 1, false, 0);
    test_gemm_case<T>(true, true, 512, 512, 256, -1, 1, 1, true, 0);
    test_gemm_case<T>(true, true, 5 * 128 + 17, 5 * 128 + 17, 128, -1, 1, 2, true, 0);
    test_gemm_case<T>(true, true, 4352, 4352, 32, -1, 1, 1, true, 0);    // 34x34 tiles -> XCD super-tile path
    test_gemm_case<T>(true, false, 4224, 4224, 32, 1, 0, 1, false, 0);   // 33x33 tiles, rectangular super-tiles
    test_gemm_case<T>(true, false, 300, 3000, 40, 1, 1, 1, false, 1);    // many more tile columns than rows: column-major tile order
    test_gemm_case<T>(true, true, 260, 2100, 33, -1, 0, 2, false, 0);
    // more than one round of 128-tiles with a short last round: its tiles run as 64 x 64 quarters (ragged edges, both operand layouts)
    test_gemm_case<T>(true, true, 4100, 4100, 70, -1, 1, 1, true, 1);
    test_gemm_case<T>(false, false, 3000, 3100, 50, 1, 1, 1, false, 1);
    test_gemm_case<T>(true, false, 4100, 4100, 40, -1, 1, 1, true, 0);
    test_gemm_case<T>(false, true, 3072, 3328, 48, 1, 0, 1, false, 0);
    // ragged M, N AND K with aligned operands: the edge tiles take the pipelined loop on clamped rows, the partial last k-chunk goes
    // through the bounds-checked loads behind it (round 4); an operand stored K x M whose M is not a whole number of vectors does not
    test_gemm_case<T>(true, true, 1000, 900, 1000, -1, 1, 1, false, 0);
    test_gemm_case<T>(true, false, 1000, 904, 336, 1, 0, 1, false, 0);
    test_gemm_case<T>(false, true, 1000, 904, 336, -1, 1, 1, false, 0);
    test_gemm_case<T>(false, false, 1026, 1030, 200, 1, 1, 1, false, 2);
    test_gemm_case<T>(true, true, 777, 777, 1000, -1, 1, 1, true, 0);
}

// ----------------------------------------------------------------------------
// kernel matrix
// ----------------------------------------------------------------------------
static double kappa(int kind, double r2, double dot, double il) {
    const double q = r2 * il * il;
    switch (kind) {
        case GPK_K_EQ: return std::exp(-0.5 * q);
        case GPK_K_MATERN12: return std::exp(-std::sqrt(q));
        case GPK_K_MATERN32: { double s = std::sqrt(3 * q); return (1 + s) * std::exp(-s); }
        case GPK_K_MATERN52: { double s = std::sqrt(5 * q); return (1 + s + s * s / 3) * std::exp(-s); }
        case GPK_K_LINEAR: return dot * il * il;
        default: return 1.0;
    }
}
template <typename T>
static void test_kmat_case(std::vector<int> kinds, int n, int m, int d, int batch, bool sym, bool lower, bool acc, bool dvec) {
    const int nt = (int)kinds.size();
    std::vector<double> var(nt), il(nt);
    for (int t = 0; t < nt; ++t) { var[t] = 0.5 + 0.3 * t; il[t] = 1.0 / (0.7 + 0.2 * t); }
    if (sym) m = n;
    auto X = randv<T>((size_t)batch * n * d), Y = sym ? X : randv<T>((size_t)batch * m * d);
    const int64_t ld = m + 3;
    auto O = randv<T>((size_t)batch * n * ld);
    auto dv = randv<T>((size_t)batch * n);
    Dev<T> dX(X.size()), dY(Y.size()), dO(O.size()), dD(dv.size());
    dX.up(X); dY.up(Y); dO.up(O); dD.up(dv);
    int st = gpk_kmat(DT<T>::v, kinds.data(), var.data(), il.data(), nullptr, nt, dX.p, n, d, (int64_t)n * d, sym ? dX.p : dY.p, m, d, (int64_t)m * d, d,
                      dO.p, ld, (int64_t)n * ld, batch, lower, sym, sym ? 0.25 : 0.0, dvec ? dD.p : nullptr, n, acc, nullptr);
    HIPCHK(hipDeviceSynchronize());
    auto got = dO.down();
    std::vector<double> ref(O.begin(), O.end());
    const int TN = 64 * (16 / (int)sizeof(T));
    for (int b = 0; b < batch; ++b)
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < m; ++j) {
                if (lower && (j / TN) * TN > (i / 32) * 32 + 31) continue;
                double r2 = 0, dot = 0;
                for (int k = 0; k < d; ++k) {
                    const double a = X[((size_t)b * n + i) * d + k], c = Y[((size_t)b * m + j) * d + k];
                    r2 += (a - c) * (a - c);
                    dot += a * c;
                }
                double v = 0;
                for (int t = 0; t < nt; ++t) v += var[t] * kappa(kinds[t], r2, dot, il[t]);
                if (sym && i == j) v += 0.25 + (dvec ? (double)dv[(size_t)b * n + i] : 0.0);
                const size_t o = (size_t)b * n * ld + (size_t)i * ld + j;
                ref[o] = acc ? (double)O[o] + v : v;
            }
    char nm[160];
    snprintf(nm, sizeof nm, "kmat_%s k%d.. nt%d n%d m%d d%d b%d sym%d low%d acc%d dv%d st%d", DT<T>::name(), kinds[0], nt, n, m, d, batch, sym, lower, acc, dvec, st);
    report(nm, st ? INFINITY : relerr(got, ref), DT<T>::eps * 50);
}
// kernel values ELEMENT by element against an 80-bit reference, in units of eps * (1 + |argument of the exponential|): that
// factor is what the rounding of the squared distance (D terms, a few ulp) is amplified by; what is left measures the device's own
// exp / sqrt (a table-based exp and a shortened rsqrt iteration since round 5).  Scales from near-duplicates to e^-600.
template <typename T>
static void test_kmat_ulp(int kind, double scale, double ilv) {
    const int n = 192, m = 320, d = 8;
    auto X = randv<T>((size_t)n * d, scale), Y = randv<T>((size_t)m * d, scale);
    for (int k = 0; k < d; ++k) Y[k] = X[k] * (T)(1 + 64 * (double)std::numeric_limits<T>::epsilon());                 // one near-duplicate pair, one exact duplicate
    for (int k = 0; k < d; ++k) Y[d + k] = X[d + k];
    Dev<T> dX(X.size()), dY(Y.size()), dO((size_t)n * m);
    dX.up(X); dY.up(Y);
    double var = 1.3, il = ilv;
    int st = gpk_kmat(DT<T>::v, &kind, &var, &il, nullptr, 1, dX.p, n, d, 0, dY.p, m, d, 0, d, dO.p, m, 0, 1, 0, 0, 0.0, nullptr, 0, 0, nullptr);
    HIPCHK(hipDeviceSynchronize());
    auto got = dO.down();
    double worst = 0, amin = 0;
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < m; ++j) {
            long double r2 = 0;
            for (int k = 0; k < d; ++k) { const long double df = (long double)X[(size_t)i * d + k] - (long double)Y[(size_t)j * d + k]; r2 += df * df; }
            const long double q = r2 * (long double)il * (long double)il;
            long double a, v;
            if (kind == GPK_K_EQ) { a = -0.5L * q; v = expl(a); }
            else if (kind == GPK_K_MATERN12) { a = -sqrtl(q); v = expl(a); }
            else if (kind == GPK_K_MATERN32) { a = -sqrtl(3 * q); v = (1 - a) * expl(a); }
            else { a = -sqrtl(5 * q); v = (1 - a + a * a / 3) * expl(a); }
            v *= (long double)var;
            if (a < (sizeof(T) == 8 ? -700 : -85)) continue;      // (denormal results: absolute, not relative, accuracy there)
            const double e = (double)(fabsl((long double)got[(size_t)i * m + j] - v) / v) / ((double)std::numeric_limits<T>::epsilon() * (1.0 + (double)-a));
            worst = std::max(worst, e);
            amin = std::min(amin, (double)a);
        }
    char nm[160];
    snprintf(nm, sizeof nm, "kmat_%s kind%d elementwise, exp arguments down to %.0f: worst error / (eps (1 + |arg|)) st%d", DT<T>::name(), kind, amin, st);
    report(nm, st ? INFINITY : worst, 6.0);
}
template <typename T>
static void test_kmat() {
    for (int kind : {GPK_K_EQ, GPK_K_MATERN12, GPK_K_MATERN32, GPK_K_MATERN52}) {
        test_kmat_ulp<T>(kind, 1.0, 0.9);
        test_kmat_ulp<T>(kind, 1.0, (sizeof(T) == 8 ? 1.0 : 0.35) * (kind == GPK_K_EQ ? 6.0 : 60.0));
        test_kmat_ulp<T>(kind, 1e-3, 1.0);
    }
    for (int k = 0; k <= 5; ++k) test_kmat_case<T>({k}, 70, 45, 3, 1, false, false, false, false);
    test_kmat_case<T>({GPK_K_EQ}, 300, 300, 8, 2, true, false, false, true);
    test_kmat_case<T>({GPK_K_EQ}, 700, 700, 8, 1, true, true, false, false);
    test_kmat_case<T>({GPK_K_EQ, GPK_K_LINEAR}, 257, 129, 4, 1, false, false, true, false);
    test_kmat_case<T>({GPK_K_MATERN52, GPK_K_MATERN32, GPK_K_CONST}, 64, 512, 20, 1, false, false, false, false);
    test_kmat_case<T>({GPK_K_EQ}, 33, 33, 1, 3, true, false, false, false);
    // kdiag
    {
        const int n = 100, d = 5;
        std::vector<int> kinds = {GPK_K_EQ, GPK_K_LINEAR};
        std::vector<double> var = {0.7, 1.3}, il = {1.0, 0.5};
        auto X = randv<T>(n * d);
        Dev<T> dX(X.size()), dO(n);
        dX.up(X);
        int st = gpk_kdiag(DT<T>::v, kinds.data(), var.data(), il.data(), nullptr, 2, dX.p, n, d, n * d, d, dO.p, n, 1, nullptr);
        HIPCHK(hipDeviceSynchronize());
        std::vector<double> ref(n);
        for (int i = 0; i < n; ++i) { double nr = 0; for (int k = 0; k < d; ++k) nr += (double)X[i * d + k] * X[i * d + k]; ref[i] = 0.7 + 1.3 * 0.25 * nr; }
        report(std::string("kdiag_") + DT<T>::name(), st ? INFINITY : relerr(dO.down(), ref), DT<T>::eps * 50);
    }
}

// gpk_kmat_scaled (--scaled): the value contract of gpk.h.  K = gpk_kmat's output for the same arguments (itself held to the host loop
// above, at that loop's tolerance); an element of the scaled launch has the BITS of fl(fl(K rs_i) cs_j) -- a missing scale skips its
// multiplication, both missing: K's bits --, and an element that receives an addition a (the diagonal of a symmetric launch, every
// element of an accumulating one) lies within eps (|v| + |a|) of v + a.  `which`: 3 = both scales, 1 = rows, 2 = columns, 0 = neither;
// `shared`: one vector for the whole batch (stride 0).  Reported: the number of elements outside the contract (0 passes).
template <typename T>
static void test_scaled_case(std::vector<int> kinds, int n, int m, int d, int batch, bool sym, bool lower, bool acc, bool dvec, int which,
                             bool shared) {
    const int nt = (int)kinds.size();
    std::vector<double> var(nt), il(nt), shp(nt, 0.0);
    bool shaped = false;
    for (int t = 0; t < nt; ++t) {
        var[t] = 0.5 + 0.3 * t; il[t] = 1.0 / (0.7 + 0.2 * t);
        if (kinds[t] == GPK_K_RQ) { shp[t] = 1.5 + t; shaped = true; }
    }
    if (sym) m = n;
    auto X = randv<T>((size_t)batch * n * d), Y = sym ? X : randv<T>((size_t)batch * m * d);
    const int64_t ld = m + 3;
    auto O = randv<T>((size_t)batch * n * ld);
    auto dv = randv<T>((size_t)batch * n), rs = randv<T>((size_t)batch * n), cs = sym ? rs : randv<T>((size_t)batch * m);
    rs[n / 3] = T(0);
    if (sym) cs = rs; else cs[m / 3] = T(0);
    Dev<T> dX(X.size()), dY(Y.size()), dO(O.size()), dK(O.size()), dD(dv.size()), dR(rs.size()), dC(cs.size());
    dX.up(X); dY.up(Y); dO.up(O); dK.zero(); dD.up(dv); dR.up(rs); dC.up(cs);
    const double* shapes = shaped ? shp.data() : nullptr;
    const double dadd = sym ? 0.25 : 0.0;
    int st = gpk_kmat(DT<T>::v, kinds.data(), var.data(), il.data(), shapes, nt, dX.p, n, d, (int64_t)n * d, sym ? dX.p : dY.p, m, d, (int64_t)m * d, d,
                      dK.p, ld, (int64_t)n * ld, batch, 0, sym, 0.0, nullptr, 0, 0, nullptr);
    const int64_t srs = shared ? 0 : n, scs = shared ? 0 : m;
    st |= gpk_kmat_scaled(DT<T>::v, kinds.data(), var.data(), il.data(), shapes, nt, dX.p, n, d, (int64_t)n * d, sym ? dX.p : dY.p, m, d, (int64_t)m * d,
                          d, (which & 1) ? dR.p : nullptr, srs, (which & 2) ? dC.p : nullptr, scs, dO.p, ld, (int64_t)n * ld, batch, lower, sym, dadd,
                          dvec ? dD.p : nullptr, n, acc, nullptr);
    HIPCHK(hipDeviceSynchronize());
    auto got = dO.down(), K = dK.down();
    const int TN = 64 * (16 / (int)sizeof(T));
    const long double eps = std::numeric_limits<T>::epsilon();
    long bad = 0;
    for (int b = 0; b < batch; ++b)
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < m; ++j) {
                const size_t o = (size_t)b * n * ld + (size_t)i * ld + j;
                if (lower && (j / TN) * TN > (i / 32) * 32 + 31) { bad += got[o] != O[o]; continue; }      // untouched
                volatile T v = K[o];
                if (which & 1) v = v * rs[(shared ? 0 : (size_t)b * n) + i];
                if (which & 2) v = v * cs[(shared ? 0 : (size_t)b * m) + j];
                long double a = acc ? (long double)O[o] : 0.0L, aa = std::fabs(a);
                const bool diag = sym && i == j;
                if (diag) { a += dadd; aa += dadd; if (dvec) { a += dv[(size_t)b * n + i]; aa += std::fabs((long double)dv[(size_t)b * n + i]); } }
                if (!acc && !diag) bad += memcmp(&got[o], const_cast<T*>(&v), sizeof(T)) != 0;
                else bad += !(std::fabs((long double)got[o] - ((long double)v + a)) <= eps * (std::fabs((long double)v) + aa));
            }
    for (size_t b = 0; b < (size_t)batch * n; ++b)      // the padding behind every row stays what it was
        for (int64_t j = m; j < ld; ++j) bad += got[b * ld + j] != O[b * ld + j];
    char nm[200];
    snprintf(nm, sizeof nm, "kmat_scaled_%s k%d.. nt%d n%d m%d d%d b%d sym%d low%d acc%d dv%d sc%d sh%d st%d", DT<T>::name(), kinds[0], nt, n, m, d,
             batch, sym, lower, acc, dvec, which, shared, st);
    report(nm, st ? INFINITY : (double)bad, 0.5);
}
template <typename T>
static void test_scaled() {
    const int TN = 64 * (16 / (int)sizeof(T));
    // every program: the single-kind ones, EQ + Linear, the generic and the shaped term table, on the row-band walk (d <= 8) ...
    for (std::vector<int> kinds : {std::vector<int>{GPK_K_EQ}, {GPK_K_MATERN12}, {GPK_K_MATERN32}, {GPK_K_MATERN52}, {GPK_K_RQ}, {GPK_K_EQ, GPK_K_LINEAR},
                                   {GPK_K_MATERN52, GPK_K_MATERN32, GPK_K_CONST}, {GPK_K_RQ, GPK_K_EQ, GPK_K_LINEAR}}) {
        test_scaled_case<T>(kinds, 33, TN + 1, 8, 1, false, false, false, false, 3, false);
        test_scaled_case<T>(kinds, 65, 2 * TN + 3, 3, 2, false, false, false, false, 3, false);
    }
    // ... and on the one-tile kernel with two and three dimension chunks
    for (int d : {9, 17}) {
        test_scaled_case<T>({GPK_K_EQ}, 33, TN + 1, d, 1, false, false, false, false, 3, false);
        test_scaled_case<T>({GPK_K_RQ, GPK_K_EQ, GPK_K_LINEAR}, 33, TN + 1, d, 1, false, false, true, false, 3, false);
    }
    // a missing scale, both missing, a vector shared by the batch, the smallest launch
    for (int which : {0, 1, 2}) test_scaled_case<T>({GPK_K_EQ}, 31, TN - 1, 3, 2, false, false, false, false, which, false);
    test_scaled_case<T>({GPK_K_MATERN32}, 33, 2 * TN + 1, 2, 3, false, false, false, false, 3, true);
    test_scaled_case<T>({GPK_K_EQ}, 1, 1, 1, 1, false, false, false, false, 3, false);
    // accumulate; the symmetric launches: the diagonal additions stay unscaled, the compact lower-triangle grid leaves the upper tiles
    test_scaled_case<T>({GPK_K_EQ, GPK_K_LINEAR}, 65, 2 * TN + 3, 4, 1, false, false, true, false, 3, false);
    test_scaled_case<T>({GPK_K_EQ}, 300, 300, 8, 2, true, false, false, true, 3, false);
    test_scaled_case<T>({GPK_K_EQ}, 3 * TN + 5, 3 * TN + 5, 8, 1, true, true, false, true, 3, false);
    test_scaled_case<T>({GPK_K_MATERN52, GPK_K_MATERN32, GPK_K_CONST}, 3 * TN + 5, 3 * TN + 5, 2, 1, true, true, true, true, 3, false);
}

// ----------------------------------------------------------------------------
// Cholesky + solves
// ----------------------------------------------------------------------------
template <typename T>
static std::vector<T> make_spd(int n, int batch, int64_t ld) {
    // EQ kernel on random 3-d points + 0.5 I  (condition number modest)
    std::vector<T> A((size_t)batch * n * ld, (T)0);
    for (int b = 0; b < batch; ++b) {
        auto X = randv<double>((size_t)n * 3);
        auto fill_row = [&](int i) {
            for (int j = 0; j <= i; ++j) {
                double r2 = 0;
                for (int k = 0; k < 3; ++k) { double df = X[i * 3 + k] - X[j * 3 + k]; r2 += df * df; }
                double v = std::exp(-0.5 * r2) + (i == j ? 0.5 : 0.0);
                A[(size_t)b * n * ld + (size_t)i * ld + j] = (T)v;
                A[(size_t)b * n * ld + (size_t)j * ld + i] = (T)v;
            }
        };
        if (n >= 1024) parallel_for(n, fill_row);       // (row i writes the pairs (i, j <= i): no two rows share an element)
        else for (int i = 0; i < n; ++i) fill_row(i);
    }
    return A;
}
// L[i][j] = (A[i][j] - sum_{k<j} L[i][k] L[j][k]) / L[j][j], every sum over ascending k (the bits of the plain column-by-column loop,
// whatever the schedule).  Row i's entries in the columns [j0, min(j1, i + 1)) of a column block: eight sums at a time over the columns
// in front of the block -- independent chains for the core to overlap -- then each entry's few terms inside the block.
static void host_chol_row(double* A, int64_t ld, int i, int j0, int j1) {
    double* Li = A + (int64_t)i * ld;
    const int je = std::min(j1, i + 1);
    for (int jb = j0; jb < je; jb += 8) {
        const int nj = std::min(8, je - jb);
        double s[8];
        const double* Lj[8];
        for (int q = 0; q < 8; ++q) {
            const int j = jb + std::min(q, nj - 1);
            Lj[q] = A + (int64_t)j * ld;
            s[q] = Li[j];
        }
        for (int k = 0; k < j0; ++k) {
            const double a = Li[k];
            s[0] -= a * Lj[0][k]; s[1] -= a * Lj[1][k]; s[2] -= a * Lj[2][k]; s[3] -= a * Lj[3][k];
            s[4] -= a * Lj[4][k]; s[5] -= a * Lj[5][k]; s[6] -= a * Lj[6][k]; s[7] -= a * Lj[7][k];
        }
        for (int q = 0; q < nj; ++q) {
            const int j = jb + q;
            double t = s[q];
            for (int k = j0; k < j; ++k) t -= Li[k] * Lj[q][k];
            Li[j] = (i == j) ? std::sqrt(t) : t / Lj[q][j];
        }
    }
}
// column blocks of 32: the block's own rows (serial), then every row below it on its own (`par`: spread over the host's cores)
static void host_chol(double* A, int n, int64_t ld, bool par) {
    constexpr int W = 32;
    for (int j0 = 0; j0 < n; j0 += W) {
        const int j1 = std::min(n, j0 + W);
        for (int i = j0; i < j1; ++i) host_chol_row(A, ld, i, j0, j1);
        if (par && n - j1 >= 1024) parallel_for(n - j1, [&](int r) { host_chol_row(A, ld, j1 + r, j0, j1); }, 32);
        else for (int i = j1; i < n; ++i) host_chol_row(A, ld, i, j0, j1);
    }
}
template <typename T>
static void test_potrf_case(int n, int batch, int nbo, int nrhs_small, int nrhs_big, int sb) {
    const int64_t ld = n + (n % 2);   // keep rows 16-byte aligned for f64, exercise ld != n
    auto A = make_spd<T>(n, batch, ld);
    const int64_t sA = (int64_t)n * ld;
    const int64_t de = gpk_dinv_elems(n);
    Dev<T> dA(A.size()), dinv((size_t)de * batch);
    Dev<int> info(batch);
    dA.up(A); info.zero();
    int st = gpk_potrf(DT<T>::v, dA.p, n, ld, sA, batch, dinv.p, info.p, nbo, nullptr);
    HIPCHK(hipDeviceSynchronize());
    auto L = dA.down();
    auto inf = info.down();
    // host reference factor
    std::vector<double> Lref(A.begin(), A.end());
    if (batch == 1) host_chol(Lref.data(), n, ld, true);
    else parallel_for(batch, [&](int b) { host_chol(Lref.data() + b * sA, n, ld, false); });      // (the members of a batch are independent)
    double num = 0, den = 0;
    bool finite = true;
    for (int b = 0; b < batch; ++b)
        for (int i = 0; i < n; ++i)
            for (int j = 0; j <= i; ++j) {
                const double g = L[b * sA + i * ld + j], r = Lref[b * sA + i * ld + j];
                if (!std::isfinite(g)) finite = false;
                num = std::max(num, std::fabs(g - r));
                den = std::max(den, std::fabs(r));
            }
    char nm[160];
    snprintf(nm, sizeof nm, "potrf_%s n%d batch%d nbo%d st%d info%d", DT<T>::name(), n, batch, nbo, st, inf[0]);
    report(nm, (st || !finite || inf[0]) ? INFINITY : num / den, DT<T>::eps * 100);

    // dinv check: inv(L_cc) * L_cc = I on the first and last diagonal block of batch 0
    {
        auto W = dinv.down();
        const int nblk = (n + 127) / 128;
        double worst = 0;
        for (int blk : {0, nblk - 1}) {
            const int o = blk * 128, nv = std::min(128, n - o);
            for (int i = 0; i < nv; ++i)
                for (int j = 0; j < nv; ++j) {
                    double s = 0;
                    for (int k = 0; k < nv; ++k) s += (double)W[(size_t)blk * 16384 + i * 128 + k] * Lref[(o + k) * ld + o + j] * (k >= j ? 1.0 : 0.0);
                    worst = std::max(worst, std::fabs(s - (i == j ? 1.0 : 0.0)));
                }
        }
        snprintf(nm, sizeof nm, "dinv128_%s n%d", DT<T>::name(), n);
        report(nm, worst, DT<T>::eps * 1000);
    }

    // logdet
    {
        Dev<T> out(batch);
        int s2 = gpk_logdet_chol(DT<T>::v, dA.p, n, ld, sA, batch, out.p, nullptr);
        HIPCHK(hipDeviceSynchronize());
        std::vector<double> ref(batch, 0.0);
        for (int b = 0; b < batch; ++b) for (int i = 0; i < n; ++i) ref[b] += 2 * std::log(Lref[b * sA + i * ld + i]);
        snprintf(nm, sizeof nm, "logdet_%s n%d st%d", DT<T>::name(), n, s2);
        report(nm, s2 ? INFINITY : relerr(out.down(), ref), DT<T>::eps * 100);
    }

    // merged inverses + solves
    Dev<T> dsb((size_t)batch * ((n + sb - 1) / sb) * sb * sb), tmpm((size_t)((n + sb - 1) / sb) * sb * sb / 4 + 16);
    int s3 = gpk_trtri_merge(DT<T>::v, dA.p, n, ld, sA, batch, dinv.p, sb, dsb.p, tmpm.p, nullptr);
    HIPCHK(hipDeviceSynchronize());
    for (int pass = 0; pass < 2; ++pass) {
        const int nrhs = pass == 0 ? nrhs_small : nrhs_big;
        if (nrhs <= 0) continue;
        const int64_t ldb = nrhs + (pass == 0 ? 0 : 2);
        auto Bm = randv<T>((size_t)batch * n * ldb);
        Dev<T> dB(Bm.size()), tmp((size_t)batch * sb * nrhs + GPK_TRSV_CTRL_ELEMS);
        dB.up(Bm);
        int s4 = pass == 0 ? gpk_trsv_lower(DT<T>::v, dA.p, n, ld, sA, dsb.p, sb, dB.p, nrhs, ldb, (int64_t)n * ldb, tmp.p, batch, nullptr)
                           : gpk_trsm_lower(DT<T>::v, dA.p, n, ld, sA, dsb.p, sb, dB.p, nrhs, ldb, (int64_t)n * ldb, tmp.p, batch, nullptr);
        HIPCHK(hipDeviceSynchronize());
        std::vector<double> ref(Bm.begin(), Bm.end());
        parallel_for(batch * nrhs, [&](int bc) {          // (column c of member b touches only its own entries of `ref`)
            const int b = bc / nrhs, c = bc % nrhs;
            for (int i = 0; i < n; ++i) {
                double s = ref[((size_t)b * n + i) * ldb + c];
                for (int k = 0; k < i; ++k) s -= Lref[b * sA + i * ld + k] * ref[((size_t)b * n + k) * ldb + c];
                ref[((size_t)b * n + i) * ldb + c] = s / Lref[b * sA + i * ld + i];
            }
        });
        // compare only the nrhs columns
        auto got = dB.down();
        double nu = 0, de2 = 0;
        for (int b = 0; b < batch; ++b) for (int i = 0; i < n; ++i) for (int c = 0; c < nrhs; ++c) {
            const size_t o = ((size_t)b * n + i) * ldb + c;
            if (!std::isfinite((double)got[o])) nu = INFINITY;
            nu = std::max(nu, std::fabs((double)got[o] - ref[o]));
            de2 = std::max(de2, std::fabs(ref[o]));
        }
        snprintf(nm, sizeof nm, "%s_%s n%d nrhs%d sb%d batch%d st%d/%d", pass == 0 ? "trsv" : "trsm", DT<T>::name(), n, nrhs, sb, batch, s3, s4);
        report(nm, (s3 || s4) ? INFINITY : nu / de2, DT<T>::eps * 1000);
        if (pass == 1) {   // the same solve out of place: the solution goes to a second buffer (its own leading dimension), b is workspace
            const int64_t ldx = nrhs + 1;
            Dev<T> dX((size_t)batch * n * ldx);
            dX.up(std::vector<T>((size_t)batch * n * ldx, T(7)));
            dB.up(Bm);
            const int s5 = gpk_trsm_lower_to(DT<T>::v, dA.p, n, ld, sA, dsb.p, sb, dB.p, nrhs, ldb, (int64_t)n * ldb, dX.p, ldx, (int64_t)n * ldx, batch, nullptr);
            HIPCHK(hipDeviceSynchronize());
            auto gx = dX.down();
            double nu2 = 0;
            for (int b = 0; b < batch; ++b) for (int i = 0; i < n; ++i) {
                for (int c = 0; c < nrhs; ++c) {
                    const double g = (double)gx[((size_t)b * n + i) * ldx + c];
                    if (!std::isfinite(g)) nu2 = INFINITY;
                    nu2 = std::max(nu2, std::fabs(g - ref[((size_t)b * n + i) * ldb + c]));
                }
                if ((double)gx[((size_t)b * n + i) * ldx + nrhs] != 7.0) nu2 = INFINITY;      // the padding column of x is not touched
            }
            snprintf(nm, sizeof nm, "trsm_to_%s n%d nrhs%d sb%d batch%d st%d", DT<T>::name(), n, nrhs, sb, batch, s5);
            report(nm, s5 ? INFINITY : nu2 / de2, DT<T>::eps * 1000);
        }
    }
}
template <typename T>
static void test_potrf() {
    // the single-column sweep of one factor: ragged last blocks, every merged block width
    test_potrf_case<T>(2500, 1, 0, 1, 0, 512);
    test_potrf_case<T>(4500, 1, 0, 1, 0, 1024);
    test_potrf_case<T>(2304, 1, 0, 1, 0, 256);
    test_potrf_case<T>(4096, 1, 0, 1, 0, 2048);
    test_potrf_case<T>(700, 1, 0, 1, 0, 256);
    test_potrf_case<T>(1664, 1, 256, 1, 0, 512);
    test_potrf_case<T>(10, 1, 0, 1, 3, 128);
    test_potrf_case<T>(100, 3, 0, 2, 0, 128);
    test_potrf_case<T>(128, 1, 0, 1, 130, 128);
    test_potrf_case<T>(200, 2, 0, 3, 64, 128);
    test_potrf_case<T>(256, 1, 128, 1, 0, 256);
    test_potrf_case<T>(384, 1, 256, 8, 200, 256);
    test_potrf_case<T>(500, 2, 256, 1, 129, 512);
    test_potrf_case<T>(1024, 1, 256, 1, 256, 512);
    test_potrf_case<T>(1200, 1, 512, 4, 100, 512);
    test_potrf_case<T>(1664, 1, 256, 1, 300, 256);
    test_potrf_case<T>(700, 70, 256, 1, 0, 128);     // larger batch, ragged
    test_potrf_case<T>(512, 64, 128, 2, 0, 128);
    // the mixed-phase batched steps (fp32, batch >= 64, orders that are multiples of 128 from 512 on; fp64: the lockstep launches):
    // every halving level, a partial last outer panel, batches that do not divide by the 8 queues
    test_potrf_case<T>(1024, 64, 256, 1, 0, 128);
    test_potrf_case<T>(640, 67, 256, 1, 0, 128);
    test_potrf_case<T>(1536, 65, 512, 1, 0, 128);
    test_potrf_case<T>(2048, 72, 0, 1, 0, 128);
    test_potrf_case<T>(1152, 64, 1024, 1, 0, 128);
}


// ----------------------------------------------------------------------------
// persistent two-problem update + look-ahead Cholesky
// ----------------------------------------------------------------------------
template <typename T>
static void test_update2_case(int M0, int N0, int M1, int K, int reserve, int pad) {
    // segment 0: rectangular, OUT OF PLACE (cin != c); segment 1: square, lower tiles only, in place
    const int64_t lda0 = K + pad, ldb0 = K + pad, ldcin = N0 + pad, ldc0 = N0 + 2 * pad, lda1 = K + pad, ldc1 = M1 + pad;
    auto A0 = randv<T>((size_t)M0 * lda0), B0 = randv<T>((size_t)N0 * ldb0), Cin = randv<T>((size_t)M0 * ldcin);
    auto A1 = randv<T>((size_t)M1 * lda1), C1 = randv<T>((size_t)M1 * ldc1);
    std::vector<T> C0((size_t)M0 * ldc0, (T)7);
    Dev<T> dA0(A0.size()), dB0(B0.size()), dCin(Cin.size()), dC0(C0.size()), dA1(A1.size()), dC1(C1.size());
    Dev<unsigned> ctrl(64);
    dA0.up(A0); dB0.up(B0); dCin.up(Cin); dC0.up(C0); dA1.up(A1); dC1.up(C1);
    gpk_update_t u[2];
    u[0] = gpk_update_t{M0, N0, K, dA0.p, lda0, dB0.p, ldb0, dCin.p, ldcin, dC0.p, ldc0, 0};
    u[1] = gpk_update_t{M1, M1, K, dA1.p, lda1, dA1.p, lda1, dC1.p, ldc1, dC1.p, ldc1, 1};
    const int st = gpk_gemm_update2(DT<T>::v, u, 2, -1.0, ctrl.p, reserve, nullptr);
    HIPCHK(hipDeviceSynchronize());
    auto g0 = dC0.down(), g1 = dC1.down();
    double num = 0, den = 0;
    bool ok = true;
    for (int i = 0; i < M0; ++i)
        for (int j = 0; j < N0; ++j) {
            double r = Cin[(size_t)i * ldcin + j];
            for (int k = 0; k < K; ++k) r -= (double)A0[(size_t)i * lda0 + k] * (double)B0[(size_t)j * ldb0 + k];
            const double g = g0[(size_t)i * ldc0 + j];
            if (!std::isfinite(g)) ok = false;
            num = std::max(num, std::fabs(g - r)); den = std::max(den, std::fabs(r));
        }
    const int ts = 64;   // tiles strictly above the diagonal (at the finest tile size) must be untouched
    for (int i = 0; i < M1; ++i)
        for (int j = 0; j < M1; ++j) {
            double r = C1[(size_t)i * ldc1 + j];
            const double g = g1[(size_t)i * ldc1 + j];
            if (j <= i) {
                for (int k = 0; k < K; ++k) r -= (double)A1[(size_t)i * lda1 + k] * (double)A1[(size_t)j * lda1 + k];
            } else if (j / 128 > i / 128 || (j / ts > i / ts && g == r)) {
                // untouched (above the tile diagonal for whichever tile size ran)
            } else {
                for (int k = 0; k < K; ++k) r -= (double)A1[(size_t)i * lda1 + k] * (double)A1[(size_t)j * lda1 + k];
            }
            if (!std::isfinite(g)) ok = false;
            num = std::max(num, std::fabs(g - r)); den = std::max(den, std::fabs(r));
        }
    char nm[160];
    snprintf(nm, sizeof nm, "update2_%s %dx%d+%d^2 k%d reserve%d pad%d st%d", DT<T>::name(), M0, N0, M1, K, reserve, pad, st);
    report(nm, (st || !ok) ? INFINITY : num / den, DT<T>::eps * 100);
}

template <typename T>
static void test_potrf_la_case(int n, int nb, int mode, int64_t min_rows, int64_t tail_rows = 0, int sb = 0) {
    const int64_t ld = n + (n % 2);
    auto A = make_spd<T>(n, 1, ld);
    const int64_t de = gpk_dinv_elems(n);
    const int wb = sb > 0 ? sb : nb;           // width of the explicit inverses
    const int nblk = (n + wb - 1) / wb;
    Dev<T> dA(A.size()), dRef(A.size()), dinv((size_t)de), dinv2((size_t)de), dbig((size_t)nblk * wb * wb), ws((size_t)gpk_potrf_la_ws_elems(n, nb));
    Dev<int> info(1), info2(1);
    dA.up(A); dRef.up(A); info.zero(); info2.zero();
    gpk_tune(7, mode); gpk_tune(6, min_rows); gpk_tune(9, tail_rows);
    const int st = sb > 0 ? gpk_potrf_la_split(DT<T>::v, dA.p, n, ld, dinv.p, dbig.p, nb, sb, ws.p, info.p, nullptr)
                          : gpk_potrf_la(DT<T>::v, dA.p, n, ld, dinv.p, dbig.p, nb, ws.p, info.p, nullptr);
    gpk_tune(7, 1); gpk_tune(6, 2048); gpk_tune(9, 0);
    const int st2 = gpk_potrf(DT<T>::v, dRef.p, n, ld, 0, 1, dinv2.p, info2.p, 0, nullptr);
    HIPCHK(hipDeviceSynchronize());
    auto L = dA.down(), R = dRef.down();
    double num = 0, den = 0;
    bool finite = true;
    for (int i = 0; i < n; ++i)
        for (int j = 0; j <= i; ++j) {
            const double g = L[(size_t)i * ld + j], r = R[(size_t)i * ld + j];
            if (!std::isfinite(g)) finite = false;
            num = std::max(num, std::fabs(g - r)); den = std::max(den, std::fabs(r));
        }
    char nm[160];
    snprintf(nm, sizeof nm, "potrf_la_%s n%d nb%d sb%d mode%d minrows%lld tail%lld st%d/%d info%d", DT<T>::name(), n, nb, wb, mode, (long long)min_rows, (long long)tail_rows, st, st2, info.down()[0]);
    report(nm, (st || st2 || !finite || info.down()[0]) ? INFINITY : num / den, DT<T>::eps * 100);
    // upper triangle untouched
    {
        double worst = 0;
        for (int i = 0; i < n; ++i) for (int j = (i / 128 + 1) * 128; j < n; ++j) worst = std::max(worst, std::fabs((double)L[(size_t)i * ld + j] - (double)A[(size_t)i * ld + j]));
        snprintf(nm, sizeof nm, "potrf_la_%s n%d above the 128-block diagonal untouched", DT<T>::name(), n);
        report(nm, worst, 0.0);
    }
    // merged inverses: W_j L_jj = I on the first and the last block; 128-block inverses equal the plain path's
    {
        auto W = dbig.down();
        double worst = 0;
        for (int blk : {0, nblk / 2, nblk - 1}) {
            const int o = blk * wb, nv = std::min(wb, n - o);
            for (int i = 0; i < nv; i += 7)
                for (int j = 0; j < nv; ++j) {
                    double sacc = 0;
                    for (int k = j; k <= i; ++k) sacc += (double)W[(size_t)blk * wb * wb + (size_t)i * wb + k] * (double)R[(size_t)(o + k) * ld + o + j];
                    worst = std::max(worst, std::fabs(sacc - (i == j ? 1.0 : 0.0)));
                }
        }
        snprintf(nm, sizeof nm, "potrf_la_%s n%d nb%d dinv_nb", DT<T>::name(), n, nb);
        report(nm, worst, DT<T>::eps * 1000);
        auto d1 = dinv.down(), d2 = dinv2.down();
        double nu = 0, dn = 0;
        for (size_t i = 0; i < d1.size(); ++i) { nu = std::max(nu, std::fabs((double)d1[i] - (double)d2[i])); dn = std::max(dn, std::fabs((double)d2[i])); }
        snprintf(nm, sizeof nm, "potrf_la_%s n%d nb%d dinv128", DT<T>::name(), n, nb);
        report(nm, nu / dn, DT<T>::eps * 1000);
    }
}

// factorisation with rows under the matrix (gpk_potrf_rows): the factor against the plain path's, the extra rows against E L^{-T}
// by substitution on the host
template <typename T>
static void test_potrf_rows_case(int n, int extra, int nb, int sb, int64_t tail, int agg = 2, int flags = 0) {
    // flags & 1: the last 64 rows are the right-hand side's strip -- `extra` counts the rows in front of it plus the vector itself
    const int strip = (flags & 1) ? GPK_ROWS_RHS_STRIP : 0;
    const int64_t ld = n, rows = n + extra + (strip ? strip - 1 : 0);
    auto A = make_spd<T>(n, 1, ld);
    auto E = randv<T>((size_t)(rows - n) * ld);
    for (size_t i = (size_t)extra * ld; i < E.size(); ++i) E[i] = T(0);      // (the strip's padding)
    std::vector<T> full((size_t)rows * ld);
    std::copy(A.begin(), A.end(), full.begin());
    std::copy(E.begin(), E.end(), full.begin() + (size_t)n * ld);
    const int wb = sb > 0 ? sb : (nb > 0 ? nb : 128);
    const int nblk = (n + wb - 1) / wb;
    Dev<T> dA(full.size()), dRef(A.size()), dinv((size_t)gpk_dinv_elems(n) + 128 * 128), dinv2((size_t)gpk_dinv_elems(n)), dbig((size_t)nblk * wb * wb),
        ws((size_t)(nb > 0 ? gpk_potrf_la_ws_elems(rows, nb) : 16));
    Dev<int> info(1), info2(1);
    dA.up(full); dRef.up(A); info.zero(); info2.zero();
    gpk_tune(9, tail); gpk_tune(47, agg);
    // flags: the last row as a right-hand side (round 6) -- the same numbers are expected in it
    const int st = flags ? gpk_potrf_rows_rhs(DT<T>::v, dA.p, n, rows, ld, dinv.p, dbig.p, nb, sb, ws.p, info.p, flags, nullptr)
                         : gpk_potrf_rows(DT<T>::v, dA.p, n, rows, ld, dinv.p, dbig.p, nb, sb, ws.p, info.p, nullptr);
    gpk_tune(9, 0); gpk_tune(47, 2);
    const int st2 = gpk_potrf(DT<T>::v, dRef.p, n, ld, 0, 1, dinv2.p, info2.p, 0, nullptr);
    HIPCHK(hipDeviceSynchronize());
    auto G = dA.down(), R = dRef.down();
    double num = 0, den = 0, znum = 0, zden = 0;
    bool finite = true;
    for (int i = 0; i < n; ++i)
        for (int j = 0; j <= i; ++j) {
            const double g = G[(size_t)i * ld + j], r = R[(size_t)i * ld + j];
            if (!std::isfinite(g)) finite = false;
            num = std::max(num, std::fabs(g - r)); den = std::max(den, std::fabs(r));
        }
    std::vector<double> znum_e(extra, 0.0), zden_e(extra, 0.0);
    std::vector<char> bad_e(extra, 0);
    parallel_for(extra, [&](int e) {            // z L^T = E[e]:  z_j = (E[e][j] - sum_{k<j} z_k L[j][k]) / L[j][j]   (the rows are independent)
        std::vector<double> z(n);
        for (int j = 0; j < n; ++j) {
            double acc = E[(size_t)e * ld + j];
            for (int k = 0; k < j; ++k) acc -= z[k] * (double)R[(size_t)j * ld + k];
            z[j] = acc / (double)R[(size_t)j * ld + j];
        }
        double zn = 0, zd = 0;
        char bad = 0;
        for (int j = 0; j < n; ++j) {
            const double g = G[(size_t)(n + e) * ld + j];
            if (!std::isfinite(g)) bad = 1;
            zn = std::max(zn, std::fabs(g - z[j])); zd = std::max(zd, std::fabs(z[j]));
        }
        znum_e[e] = zn; zden_e[e] = zd; bad_e[e] = bad;
    });
    for (int e = 0; e < extra; ++e) {
        if (bad_e[e]) finite = false;
        znum = std::max(znum, znum_e[e]); zden = std::max(zden, zden_e[e]);
    }
    char nm[200];
    snprintf(nm, sizeof nm, "potrf_rows_%s n%d +%d rows nb%d sb%d tail%lld agg%d flags%d st%d/%d info%d: factor", DT<T>::name(), n, extra, nb, wb, (long long)tail, agg, flags, st, st2, info.down()[0]);
    report(nm, (st || st2 || !finite || info.down()[0]) ? INFINITY : num / den, DT<T>::eps);
    snprintf(nm, sizeof nm, "potrf_rows_%s n%d +%d rows nb%d sb%d tail%lld agg%d flags%d: rows = E L^-T", DT<T>::name(), n, extra, nb, wb, (long long)tail, agg, flags);
    report(nm, (st || !finite) ? INFINITY : znum / zden, DT<T>::eps * 2);
}

// batched factorisation with one right-hand side per matrix solved along (gpk_potrf_rhs): factors bit-identical to gpk_potrf's,
// the solved vectors against gpk_trsv_lower on those factors
template <typename T>
static void test_potrf_rhs_case(int n, int batch) {
    const int64_t ld = n, bs = (int64_t)n * ld;
    auto A = make_spd<T>(n, batch, ld);
    auto Bv = randv<T>((size_t)batch * n);
    Dev<T> dA(A.size()), dR(A.size()), dinv((size_t)batch * gpk_dinv_elems(n)), dinv2((size_t)batch * gpk_dinv_elems(n)), dB(Bv.size()), dB2(Bv.size()),
        tmp((size_t)batch * 128 + 16), tmp2((size_t)batch * 128 + 16);
    Dev<int> info(batch), info2(batch);
    dA.up(A); dR.up(A); dB.up(Bv); dB2.up(Bv); info.zero(); info2.zero();
    const int st = gpk_potrf_rhs(DT<T>::v, dA.p, n, ld, bs, batch, dinv.p, info.p, 0, dB.p, n, tmp.p, nullptr);
    const int st2 = gpk_potrf(DT<T>::v, dR.p, n, ld, bs, batch, dinv2.p, info2.p, 0, nullptr);
    const int st3 = gpk_trsv_lower(DT<T>::v, dR.p, n, ld, bs, dinv2.p, 128, dB2.p, 1, 1, n, tmp2.p, batch, nullptr);
    HIPCHK(hipDeviceSynchronize());
    auto G = dA.down(), R = dR.down();
    auto x = dB.down(), x2 = dB2.down();
    size_t diff = 0;
    for (int b = 0; b < batch; ++b)
        for (int i = 0; i < n; ++i)
            for (int j = 0; j <= i; ++j) diff += G[(size_t)b * bs + (size_t)i * ld + j] != R[(size_t)b * bs + (size_t)i * ld + j];
    double num = 0, den = 0;
    bool finite = true;
    for (size_t i = 0; i < x.size(); ++i) {
        if (!std::isfinite((double)x[i])) finite = false;
        num = std::max(num, std::fabs((double)x[i] - (double)x2[i])); den = std::max(den, std::fabs((double)x2[i]));
    }
    int bad = 0;
    for (int v : info.down()) bad += v != 0;
    char nm[200];
    snprintf(nm, sizeof nm, "potrf_rhs_%s n%d batch%d st%d/%d/%d bad_info%d: factors differ in %zu entries", DT<T>::name(), n, batch, st, st2, st3, bad, diff);
    report(nm, (st || st2 || st3 || bad || diff) ? INFINITY : 0.0, DT<T>::eps);
    snprintf(nm, sizeof nm, "potrf_rhs_%s n%d batch%d: L^-1 b against gpk_trsv_lower", DT<T>::name(), n, batch);
    report(nm, (st || !finite) ? INFINITY : num / den, DT<T>::eps * 200);
}

template <typename T>
static void test_potrf_rhs() {
    test_potrf_rhs_case<T>(512, 64);      // mixed-phase steps (fp32): the sweep's steps on the side stream
    test_potrf_rhs_case<T>(1024, 70);
    test_potrf_rhs_case<T>(2048, 64);
    test_potrf_rhs_case<T>(640, 9);       // lockstep launches: the sweep behind the factorisation
    test_potrf_rhs_case<T>(300, 5);       // ragged order
    test_potrf_rhs_case<T>(1024, 1);
}

template <typename T>
static void test_potrf_rows() {
    test_potrf_rows_case<T>(128, 64, 0, 0, 0);             // one diagonal block + rows
    test_potrf_rows_case<T>(640, 200, 0, 0, 0);            // one pipelined panel
    test_potrf_rows_case<T>(1024, 300, 0, 0, 0);
    test_potrf_rows_case<T>(2560, 333, 0, 0, 0);
    test_potrf_rows_case<T>(5120, 260, 0, 0, 0);           // several panels (1024 wide), fill tiles with rows under the square part
    test_potrf_rows_case<T>(3072, 300, 512, 0, 1024);      // look-ahead + plain tail
    test_potrf_rows_case<T>(3072, 300, 512, 256, 1024);    // ... explicit inverses narrower than the outer blocks
    test_potrf_rows_case<T>(4096, 520, 1024, 0, 2048, 1);
    test_potrf_rows_case<T>(4096, 130, 256, 0, 512, 3);
    test_potrf_rows_case<T>(3840, 1000, 256, 0, 100, 2);   // tail shorter than a block: raised to one block
    test_potrf_rows_case<T>(2048, 77, 256, 0, 0);          // n <= the default tail: all plain
    // orders that are whole 128-blocks but not whole panels: a last panel of one block, 17 / 33 blocks, the look-ahead's last outer
    // block 128 wide with a plain tail whose last panel is one block
    test_potrf_rows_case<T>(2176, 130, 0, 0, 0);
    test_potrf_rows_case<T>(4224, 64, 0, 0, 0);
    test_potrf_rows_case<T>(5248, 200, 0, 0, 0);
    test_potrf_rows_case<T>(4224, 96, 1024, 0, 2048);
    test_potrf_rows_case<T>(7296, 64, 1024, 512, 3072);
    // round 6: the last row as a right-hand side vector (side stream through the look-ahead steps, a row in the tail)
    test_potrf_rows_case<T>(640, 65, 0, 0, 0, 2, 1);               // pipelined panel: a row like the others
    test_potrf_rows_case<T>(3072, 301, 512, 0, 1024, 2, 1);
    test_potrf_rows_case<T>(3072, 65, 512, 256, 1024, 2, 3);       // inverses narrower than the outer blocks, no tail inverses
    test_potrf_rows_case<T>(4096, 1, 1024, 0, 2048, 1, 1);         // the right-hand side alone
    test_potrf_rows_case<T>(7296, 129, 1024, 512, 3072, 2, 3);
    test_potrf_rows_case<T>(2048, 78, 256, 0, 0, 2, 3);            // all plain
}

template <typename T>
static void test_lookahead() {
    for (int pass = 0; pass < 2; ++pass) {      // 128-tile kernels forced, then 64-tile kernels forced
        gpk_tune(1, pass == 0 ? 0 : ((int64_t)1 << 40));
        test_update2_case<T>(300, 200, 260, 70, 0, 0);
        test_update2_case<T>(384, 128, 512, 64, 1, 0);
        test_update2_case<T>(1000, 256, 1100, 128, 1, 2);
        test_update2_case<T>(129, 1, 5, 3, 1, 1);
    }
    gpk_tune(1, 512);
    test_potrf_la_case<T>(700, 256, 1, 0);
    test_potrf_la_case<T>(1024, 256, 1, 0);
    test_potrf_la_case<T>(1200, 512, 1, 0);
    test_potrf_la_case<T>(1664, 256, 0, 0);
    test_potrf_la_case<T>(3000, 512, 1, 0);
    test_potrf_la_case<T>(3000, 1024, 1, 1024);
    test_potrf_la_case<T>(4096, 1024, 1, 0);
    test_potrf_la_case<T>(5000, 512, 1, 2048);
    test_potrf_la_case<T>(4096, 1024, 1, 0, 0, 512);       // explicit inverses narrower than the outer blocks (gpk_potrf_la_split)
    test_potrf_la_case<T>(5000, 1024, 1, 1024, 1000, 256);
    test_potrf_la_case<T>(3000, 512, 1, 0, 700, 256);
    test_potrf_la_case<T>(2100, 1024, 0, 0, 300, 512);
    gpk_tune(40, 256); gpk_tune(41, 4096);              // the next diagonal block's update inside the trailing update, at these small orders and every block width
    test_potrf_la_case<T>(4096, 1024, 1, 0);
    test_potrf_la_case<T>(5000, 512, 1, 1024);
    test_potrf_la_case<T>(6000, 256, 1, 0, 700);
    gpk_tune(40, 9216); gpk_tune(41, 512);
    test_potrf_la_case<T>(10, 256, 1, 0, 5120);        // all plain + merge
    test_potrf_la_case<T>(1200, 512, 1, 0, 5120);
    test_potrf_la_case<T>(1664, 256, 1, 0, 700);       // look-ahead, then a plain tail
    test_potrf_la_case<T>(3000, 512, 1, 0, 1500);
    test_potrf_la_case<T>(4096, 1024, 1, 0, 2048);
    test_potrf_la_case<T>(5000, 1024, 1, 1024, 1000);
    // aggregated trailing updates (round 5): every depth m, ragged orders, with / without the fused diagonal-block segment, a change of
    // policy half-way (knob 48: several depths in one step), explicit inverses narrower than the outer blocks
    for (int m : {1, 2, 3, 4, 7}) {
        gpk_tune(47, m);
        test_potrf_la_case<T>(3000, 256, 1, 0, 300);
        test_potrf_la_case<T>(4100, 512, 1, 1024, 600);
        test_potrf_la_case<T>(2900, 256, 0, 0, 300, 128 * 2);
        gpk_tune(48, 1800);
        test_potrf_la_case<T>(3333, 256, 1, 0, 500);
        gpk_tune(48, 0);
        gpk_tune(40, 256); gpk_tune(41, 4096);
        test_potrf_la_case<T>(3000, 256, 1, 0, 300);
        gpk_tune(48, 1500);
        test_potrf_la_case<T>(3000, 256, 1, 0, 300);
        gpk_tune(48, 0);
        gpk_tune(40, 9216); gpk_tune(41, 512);
    }
    gpk_tune(47, 2);
    test_potrf_la_case<T>(16896, 256, 1, 0, 1024);       // 66 outer blocks: more than a column-group mask has bits (every block, every step)
    // a non-positive-definite matrix is reported with the global pivot order
    {
        const int n = 1500, nb = 512, bad = 1111;
        const int64_t ld = n;
        auto A = make_spd<T>(n, 1, ld);
        A[(size_t)bad * ld + bad] = (T)(-5);
        Dev<T> dA(A.size()), dinv((size_t)gpk_dinv_elems(n)), dbig((size_t)3 * nb * nb), ws((size_t)gpk_potrf_la_ws_elems(n, nb));
        Dev<int> info(1);
        dA.up(A); info.zero();
        for (int64_t tail : {0, 700}) {
            dA.up(A); info.zero();
            gpk_tune(6, 0); gpk_tune(9, tail);
            const int st = gpk_potrf_la(DT<T>::v, dA.p, n, ld, dinv.p, dbig.p, nb, ws.p, info.p, nullptr);
            gpk_tune(6, 2048); gpk_tune(9, 0);
            HIPCHK(hipDeviceSynchronize());
            char nm[160];
            snprintf(nm, sizeof nm, "potrf_la_%s not PD (tail %lld): info %d (expect %d) st%d", DT<T>::name(), (long long)tail, info.down()[0], bad + 1, st);
            report(nm, (st == 0 && info.down()[0] == bad + 1) ? 0.0 : INFINITY, 0.0);
        }
    }
}

// where do workgroups land?  (XCC id, SE/SH/CU fields of HW_ID) of a 2048-workgroup grid
__global__ void census_kernel(unsigned* out) {
    unsigned xcc, hw;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
    if (threadIdx.x == 0) { out[2 * blockIdx.x] = xcc; out[2 * blockIdx.x + 1] = hw; }
    // stay a little so that the grid spreads over every CU
    const long long t0 = wall_clock64();
    while (wall_clock64() - t0 < 2000) {}
}
static void census() {
    const int nb = 2048;
    Dev<unsigned> out(2 * nb);
    hipLaunchKernelGGL(census_kernel, dim3(nb), dim3(256), 0, 0, out.p);
    HIPCHK(hipDeviceSynchronize());
    auto h = out.down();
    std::vector<int> cnt(8 * 256, 0);
    int b2x = 0;
    for (int b = 0; b < nb; ++b) {
        const unsigned xcc = h[2 * b] & 0xf, key = (h[2 * b + 1] >> 8) & 0xff;
        if ((int)(xcc & 7) == b % 8) ++b2x;
        cnt[(xcc & 7) * 256 + key]++;
    }
    printf("CENSUS block b on XCC b%%8 for %d of %d blocks; raw xcc/hw_id of blocks 0..7:", b2x, nb);
    for (int b = 0; b < 8; ++b) printf(" %x/%08x", h[2 * b], h[2 * b + 1]);
    printf("\n");
    for (int x = 0; x < 8; ++x) {
        int cus = 0;
        printf("CENSUS xcc %d keys(se.sh.cu:count):", x);
        for (int k = 0; k < 256; ++k)
            if (cnt[x * 256 + k]) { ++cus; printf(" %d.%d.%d:%d", (k >> 5) & 7, (k >> 4) & 1, k & 15, cnt[x * 256 + k]); }
        printf("  => %d distinct CUs\n", cus);
    }
}

// ----------------------------------------------------------------------------
// reductions / misc
// ----------------------------------------------------------------------------
template <typename T>
static void test_misc() {
    const int rows = 1000, cols = 300, batch = 2;
    const int64_t ld = cols + 4;
    auto V = randv<T>((size_t)batch * rows * ld), w = randv<T>((size_t)batch * rows);
    Dev<T> dV(V.size()), dw(w.size()), od((size_t)batch * cols), os((size_t)batch * cols), ws(2 * (size_t)batch * gpk_colreduce_chunks(rows) * cols);
    dV.up(V); dw.up(w);
    int st = gpk_colreduce(DT<T>::v, dV.p, rows, cols, ld, (int64_t)rows * ld, dw.p, rows, od.p, os.p, ws.p, batch, nullptr);
    HIPCHK(hipDeviceSynchronize());
    std::vector<double> rd((size_t)batch * cols, 0), rs((size_t)batch * cols, 0);
    for (int b = 0; b < batch; ++b) for (int r = 0; r < rows; ++r) for (int c = 0; c < cols; ++c) {
        const double v = V[((size_t)b * rows + r) * ld + c];
        rd[b * cols + c] += v * w[b * rows + r];
        rs[b * cols + c] += v * v;
    }
    report(std::string("colreduce_dot_") + DT<T>::name(), st ? INFINITY : relerr(od.down(), rd), DT<T>::eps * 100);
    report(std::string("colreduce_ss_") + DT<T>::name(), st ? INFINITY : relerr(os.down(), rs), DT<T>::eps * 100);
    // tril + add_diag + copy2d
    const int n = 300;
    auto A = randv<T>((size_t)n * n), dv = randv<T>(n);
    Dev<T> dA(A.size()), dd(n), dC(A.size());
    dA.up(A); dd.up(dv);
    gpk_add_diag(DT<T>::v, dA.p, n, n, (int64_t)n * n, 0.5, dd.p, n, 1, nullptr);
    gpk_tril(DT<T>::v, dA.p, n, n, (int64_t)n * n, 1, nullptr);
    gpk_copy2d(DT<T>::v, dA.p, n, 0, dC.p, n, 0, n, n, 1, nullptr);
    HIPCHK(hipDeviceSynchronize());
    std::vector<double> ref((size_t)n * n);
    for (int i = 0; i < n; ++i) for (int j = 0; j < n; ++j) ref[i * n + j] = j > i ? 0.0 : (double)A[i * n + j] + (i == j ? 0.5 + (double)dv[i] : 0.0);
    report(std::string("add_diag_tril_copy_") + DT<T>::name(), relerr(dC.down(), ref), DT<T>::eps);
}

// ----------------------------------------------------------------------------
// kernel VJP with an explicit cotangent (gradient of the pseudo-point ELBO)
// ----------------------------------------------------------------------------
static void kappa_all_host(int kind, double q, double& k, double& dkq, double& dk) {
    switch (kind) {
        case GPK_K_EQ: k = std::exp(-0.5 * q); dk = -0.5 * k; dkq = dk * q; break;
        case GPK_K_MATERN12: { double r = std::sqrt(q); k = std::exp(-r); dkq = -0.5 * r * k; dk = r > 0 ? -0.5 * k / r : 0.0; break; }
        case GPK_K_MATERN32: { double s = std::sqrt(3 * q), e = std::exp(-s); k = (1 + s) * e; dk = -1.5 * e; dkq = dk * q; break; }
        case GPK_K_MATERN52: { double s = std::sqrt(5 * q), e = std::exp(-s); k = (1 + s + s * s / 3) * e; dk = -(5.0 / 6.0) * (1 + s) * e; dkq = dk * q; break; }
        case GPK_K_LINEAR: k = q; dkq = q; dk = 1; break;
        default: k = 1; dkq = 0; dk = 0;
    }
}
template <typename T>
static void test_vjp_dense_case(std::vector<int> kinds, int n, int m, int d, bool scale_rank1, bool want_gx) {
    const int nt = (int)kinds.size();
    std::vector<double> var(nt), il(nt);
    for (int t = 0; t < nt; ++t) { var[t] = 0.6 + 0.25 * t; il[t] = 1.0 / (0.8 + 0.3 * t); }
    const int64_t ldg = m + 5;
    auto X = randv<T>((size_t)n * d), Y = randv<T>((size_t)m * d), G = randv<T>((size_t)n * ldg);
    auto cs = randv<T>(m), w = randv<T>(n), b = randv<T>(m);
    int64_t rt = 0, nc = 0;
    gpk_kmat_vjp_dense_grid(n, m, &rt, &nc);
    const int W = 2 * GPK_MAX_TERMS + 1;
    Dev<T> dX(X.size()), dY(Y.size()), dG(G.size()), dcs(m), dw(n), db(m), dP((size_t)rt * nc * W), dC((size_t)rt * m), dGX((size_t)nc * n * d);
    dX.up(X); dY.up(Y); dG.up(G); dcs.up(cs); dw.up(w); db.up(b);
    int st = gpk_kmat_vjp_dense(DT<T>::v, kinds.data(), var.data(), il.data(), nullptr, nt, dX.p, n, d, dY.p, m, d, d, dG.p, ldg,
                                scale_rank1 ? dcs.p : nullptr, scale_rank1 ? dw.p : nullptr, scale_rank1 ? db.p : nullptr,
                                dP.p, dC.p, want_gx ? dGX.p : nullptr, nullptr);
    HIPCHK(hipDeviceSynchronize());
    auto P = dP.down(), C = dC.down(), GX = dGX.down();
    std::vector<double> rS(2 * nt, 0.0), rC(m, 0.0), rGX((size_t)n * d, 0.0);
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < m; ++j) {
            double ge = (double)G[(size_t)i * ldg + j];
            if (scale_rank1) ge = ge * (double)cs[j] + (double)w[i] * (double)b[j];
            double r2 = 0, dot = 0;
            for (int k = 0; k < d; ++k) { const double a = X[(size_t)i * d + k], c = Y[(size_t)j * d + k]; r2 += (a - c) * (a - c); dot += a * c; }
            double kfull = 0;
            for (int t = 0; t < nt; ++t) {
                const double q = (kinds[t] == GPK_K_LINEAR ? dot : r2) * il[t] * il[t];
                double k, dkq, dk;
                kappa_all_host(kinds[t], q, k, dkq, dk);
                rS[2 * t] += ge * k; rS[2 * t + 1] += ge * dkq; kfull += var[t] * k;
                for (int c = 0; c < d; ++c) {
                    const double a = X[(size_t)i * d + c], y = Y[(size_t)j * d + c];
                    rGX[(size_t)i * d + c] += kinds[t] == GPK_K_LINEAR ? ge * var[t] * il[t] * il[t] * y
                                                                       : ge * var[t] * dk * 2 * il[t] * il[t] * (a - y);
                }
            }
            rC[j] += ge * kfull;
        }
    std::vector<T> gS(2 * nt, T(0)), gC(m, T(0)), gGX((size_t)n * d, T(0));
    for (int64_t wg = 0; wg < rt * nc; ++wg) for (int t = 0; t < 2 * nt; ++t) gS[t] += P[(size_t)wg * W + t];
    for (int64_t r = 0; r < rt; ++r) for (int j = 0; j < m; ++j) gC[j] += C[(size_t)r * m + j];
    if (want_gx) for (int64_t c = 0; c < nc; ++c) for (size_t e = 0; e < (size_t)n * d; ++e) gGX[e] += GX[(size_t)c * n * d + e];
    char nm[160];
    snprintf(nm, sizeof nm, "vjp_dense_%s k%d nt%d n%d m%d d%d sr%d st%d", DT<T>::name(), kinds[0], nt, n, m, d, scale_rank1, st);
    report(std::string(nm) + " sums", st ? INFINITY : relerr(gS, rS), DT<T>::eps * 50);
    report(std::string(nm) + " colsum", st ? INFINITY : relerr(gC, rC), DT<T>::eps * 50);
    if (want_gx) report(std::string(nm) + " gradx", st ? INFINITY : relerr(gGX, rGX), DT<T>::eps * 50);
}
template <typename T>
static void test_vjp_dense() {
    for (int k = 0; k <= 5; ++k) test_vjp_dense_case<T>({k}, 70, 45, 3, false, true);
    test_vjp_dense_case<T>({GPK_K_EQ, GPK_K_LINEAR}, 130, 1000, 8, true, true);
    test_vjp_dense_case<T>({GPK_K_MATERN52, GPK_K_MATERN32, GPK_K_CONST}, 64, 513, 20, true, false);
    test_vjp_dense_case<T>({GPK_K_EQ}, 300, 9000, 2, true, true);
    {   // d/dX beyond 8 input dimensions is refused, not silently wrong
        Dev<T> z(64);
        std::vector<int> kinds = {GPK_K_EQ};
        std::vector<double> one = {1.0};
        int st = gpk_kmat_vjp_dense(DT<T>::v, kinds.data(), one.data(), one.data(), nullptr, 1, z.p, 2, 9, z.p, 2, 9, 9, z.p, 2, nullptr, nullptr, nullptr, z.p, nullptr, z.p, nullptr);
        report(std::string("vjp_dense_refuses_gradx_d9_") + DT<T>::name(), st < 0 ? 0.0 : INFINITY, 1.0);
    }
}


// ----------------------------------------------------------------------------
// rational quadratic: the kind with a shape parameter (`shapes` of gpk_kmat / gpk_kdiag / gpk_kmat_vjp / gpk_kmat_vjp_dense)   --rq
// ----------------------------------------------------------------------------
// RQ values element by element against the 80-bit reference, in units of eps (1 + alpha log1p(u)), u = q / (2 alpha): the rounding
// of the squared distance reaches the value multiplied by the exponent alpha log1p(u) (at most, for u >> 1), the rest is the device's
// log1p and exp.  `generic`: a second term of variance 0 sends the call through the term-table program instead of the dedicated one.
// Asserted at twice the worst figure measured on the MI355X (profiles/README.md), which leaves room for another compiler's log1p.
#define GPK_RQ_ULP_BOUND 4.9      /* measured: 2.41 (fp32), 2.26 (fp64) */
template <typename T>
static void test_rq_ulp(double alpha, double scale, double ilv, bool generic) {
    const int n = 192, m = 320, d = 8;
    auto X = randv<T>((size_t)n * d, scale), Y = randv<T>((size_t)m * d, scale);
    for (int k = 0; k < d; ++k) Y[k] = X[k] * (T)(1 + 64 * (double)std::numeric_limits<T>::epsilon());
    for (int k = 0; k < d; ++k) Y[d + k] = X[d + k];
    Dev<T> dX(X.size()), dY(Y.size()), dO((size_t)n * m);
    dX.up(X); dY.up(Y);
    int kinds[2] = {GPK_K_RQ, GPK_K_CONST};
    double var[2] = {1.3, 0.0}, il[2] = {ilv, 1.0}, sh[2] = {alpha, 0.0};
    int st = gpk_kmat(DT<T>::v, kinds, var, il, sh, generic ? 2 : 1, dX.p, n, d, 0, dY.p, m, d, 0, d, dO.p, m, 0, 1, 0, 0, 0.0, nullptr, 0, 0, nullptr);
    HIPCHK(hipDeviceSynchronize());
    auto got = dO.down();
    double worst = 0, amax = 0;
    bool dup_exact = (double)got[(size_t)1 * m + 1] == (double)(T)1.3;      // x_1 == y_1: exactly the variance
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < m; ++j) {
            long double r2 = 0;
            for (int k = 0; k < d; ++k) { const long double df = (long double)X[(size_t)i * d + k] - (long double)Y[(size_t)j * d + k]; r2 += df * df; }
            const long double u = r2 * (long double)ilv * (long double)ilv / (2 * (long double)alpha);
            const long double a = (long double)alpha * log1pl(u);
            const long double v = 1.3L * expl(-a);
            if (a > (sizeof(T) == 8 ? 700 : 85)) continue;
            const double e = (double)(fabsl((long double)got[(size_t)i * m + j] - v) / v) / ((double)std::numeric_limits<T>::epsilon() * (1.0 + (double)a));
            worst = std::max(worst, e);
            amax = std::max(amax, (double)a);
        }
    char nm[200];
    snprintf(nm, sizeof nm, "kmat_%s rq alpha=%g il=%g %s elementwise, exponents up to %.0f: worst error / (eps (1 + alpha log1p u)) st%d", DT<T>::name(), alpha, ilv,
             generic ? "term table" : "own program", amax, st);
    report(nm, st ? INFINITY : worst, GPK_RQ_ULP_BOUND);
    report(std::string("kmat_") + DT<T>::name() + " rq duplicate point gives the variance exactly", dup_exact ? 0.0 : INFINITY, 0.0);
}
static void kappa_rq_host(double q, double a, double& k, double& dkq, double& dk, double& da) {
    const double u = q / (2 * a), lg = std::log1p(u);
    k = std::exp(-a * lg); dk = -0.5 * k / (1 + u); dkq = dk * q; da = k * (u / (1 + u) - lg);
}
template <typename T>
static void test_rq() {
    for (int band = 1; band >= 0; --band) {
        gpk_tune(12, band);
        for (double alpha : {0.1, 1.0, 50.0})
            for (int generic = 0; generic < 2; ++generic) {
                test_rq_ulp<T>(alpha, 1.0, 0.9, generic);
                test_rq_ulp<T>(alpha, 1.0, 30.0, generic);
                test_rq_ulp<T>(alpha, 1e-3, 1.0, generic);
            }
    }
    gpk_tune(12, 1);
    {   // kinds without a shape parameter: a non-NULL junk `shapes` array gives the same bits as NULL; an RQ term without alpha is refused
        const int n = 130, d = 3;
        auto X = randv<T>((size_t)n * d);
        Dev<T> dX(X.size()), dA((size_t)n * n), dB((size_t)n * n);
        dX.up(X);
        int kind = GPK_K_EQ, rq = GPK_K_RQ; double var = 0.8, il = 1.1, sh = 7.0, bad = 0.0;
        int st = gpk_kmat(DT<T>::v, &kind, &var, &il, nullptr, 1, dX.p, n, d, 0, dX.p, n, d, 0, d, dA.p, n, 0, 1, 0, 1, 0.1, nullptr, 0, 0, nullptr);
        st |= gpk_kmat(DT<T>::v, &kind, &var, &il, &sh, 1, dX.p, n, d, 0, dX.p, n, d, 0, d, dB.p, n, 0, 1, 0, 1, 0.1, nullptr, 0, 0, nullptr);
        HIPCHK(hipDeviceSynchronize());
        auto a = dA.down(), b = dB.down();
        report(std::string("kmat without rq terms: junk shapes == NULL shapes, bit for bit ") + DT<T>::name(), (st == 0 && !memcmp(a.data(), b.data(), a.size() * sizeof(T))) ? 0.0 : INFINITY, 0.0);
        st = gpk_kmat(DT<T>::v, &rq, &var, &il, nullptr, 1, dX.p, n, d, 0, dX.p, n, d, 0, d, dA.p, n, 0, 1, 0, 1, 0.1, nullptr, 0, 0, nullptr);
        report(std::string("kmat refuses an rq term (no alpha) ") + DT<T>::name(), st < 0 ? 0.0 : INFINITY, 0.0);
        st = gpk_kmat(DT<T>::v, &rq, &var, &il, &bad, 1, dX.p, n, d, 0, dX.p, n, d, 0, d, dA.p, n, 0, 1, 0, 1, 0.1, nullptr, 0, 0, nullptr);
        report(std::string("kmat refuses alpha <= 0 ") + DT<T>::name(), st < 0 ? 0.0 : INFINITY, 0.0);
        Dev<T> dD(n);
        int k2[2] = {GPK_K_RQ, GPK_K_LINEAR}; double v2[2] = {0.7, 1.3}, l2[2] = {1.0, 0.5}, s2[2] = {0.3, 0.0};
        st = gpk_kdiag(DT<T>::v, k2, v2, l2, s2, 2, dX.p, n, d, 0, d, dD.p, n, 1, nullptr);
        HIPCHK(hipDeviceSynchronize());
        std::vector<double> ref(n);
        for (int i = 0; i < n; ++i) { double nr = 0; for (int k = 0; k < d; ++k) nr += (double)X[i * d + k] * X[i * d + k]; ref[i] = 0.7 + 1.3 * 0.25 * nr; }
        report(std::string("kdiag rq + linear ") + DT<T>::name(), st ? INFINITY : relerr(dD.down(), ref), DT<T>::eps * 50);
    }
    {   // explicit-cotangent VJP with RQ terms: three sums per term, column sums, d/dx
        const int n = 130, m = 257, d = 3, nt = 3;
        int kinds[nt] = {GPK_K_RQ, GPK_K_EQ, GPK_K_RQ};
        double var[nt] = {0.6, 0.85, 1.1}, il[nt] = {1.0 / 0.8, 1.0 / 1.1, 1.0 / 2.5}, sh[nt] = {0.4, 0.0, 9.0};
        const int64_t ldg = m + 5;
        auto X = randv<T>((size_t)n * d), Y = randv<T>((size_t)m * d), G = randv<T>((size_t)n * ldg);
        auto cs = randv<T>(m), w = randv<T>(n), b = randv<T>(m);
        int64_t rt = 0, nc = 0;
        gpk_kmat_vjp_dense_grid(n, m, &rt, &nc);
        const int W = 3 * GPK_MAX_TERMS + 1;
        Dev<T> dX(X.size()), dY(Y.size()), dG(G.size()), dcs(m), dw(n), db(m), dP((size_t)rt * nc * W), dC((size_t)rt * m), dGX((size_t)nc * n * d);
        dX.up(X); dY.up(Y); dG.up(G); dcs.up(cs); dw.up(w); db.up(b);
        int st = gpk_kmat_vjp_dense(DT<T>::v, kinds, var, il, sh, nt, dX.p, n, d, dY.p, m, d, d, dG.p, ldg, dcs.p, dw.p, db.p, dP.p, dC.p, dGX.p, nullptr);
        HIPCHK(hipDeviceSynchronize());
        auto P = dP.down(), C = dC.down(), GX = dGX.down();
        std::vector<double> rS(3 * nt, 0.0), rC(m, 0.0), rGX((size_t)n * d, 0.0);
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < m; ++j) {
                const double ge = (double)G[(size_t)i * ldg + j] * (double)cs[j] + (double)w[i] * (double)b[j];
                double r2 = 0;
                for (int k = 0; k < d; ++k) { const double a = X[(size_t)i * d + k], c = Y[(size_t)j * d + k]; r2 += (a - c) * (a - c); }
                double kfull = 0;
                for (int t = 0; t < nt; ++t) {
                    const double q = r2 * il[t] * il[t];
                    double k, dkq, dk, da = 0;
                    if (kinds[t] == GPK_K_RQ) kappa_rq_host(q, sh[t], k, dkq, dk, da); else kappa_all_host(kinds[t], q, k, dkq, dk);
                    rS[3 * t] += ge * k; rS[3 * t + 1] += ge * dkq; rS[3 * t + 2] += ge * da; kfull += var[t] * k;
                    for (int c = 0; c < d; ++c) rGX[(size_t)i * d + c] += ge * var[t] * dk * 2 * il[t] * il[t] * ((double)X[(size_t)i * d + c] - (double)Y[(size_t)j * d + c]);
                }
                rC[j] += ge * kfull;
            }
        std::vector<T> gS(3 * nt, T(0)), gC(m, T(0)), gGX((size_t)n * d, T(0));
        for (int64_t wg = 0; wg < rt * nc; ++wg) for (int t = 0; t < nt; ++t) for (int c = 0; c < 3; ++c) gS[3 * t + c] += P[(size_t)wg * W + 3 * t + c];
        for (int64_t r = 0; r < rt; ++r) for (int j = 0; j < m; ++j) gC[j] += C[(size_t)r * m + j];
        for (int64_t c = 0; c < nc; ++c) for (size_t e = 0; e < (size_t)n * d; ++e) gGX[e] += GX[(size_t)c * n * d + e];
        std::string nm = std::string("vjp_dense_") + DT<T>::name() + " rq+eq+rq n130 m257 d3";
        report(nm + " sums (S1, S2, S3)", st ? INFINITY : relerr(gS, rS), DT<T>::eps * 50);
        report(nm + " colsum", st ? INFINITY : relerr(gC, rC), DT<T>::eps * 50);
        report(nm + " gradx", st ? INFINITY : relerr(gGX, rGX), DT<T>::eps * 50);
        st = gpk_kmat_vjp_dense(DT<T>::v, kinds, var, il, nullptr, nt, dX.p, n, d, dY.p, m, d, d, dG.p, ldg, dcs.p, dw.p, db.p, dP.p, dC.p, dGX.p, nullptr);
        report(std::string("vjp_dense refuses an rq term (no alpha) ") + DT<T>::name(), st < 0 ? 0.0 : INFINITY, 0.0);

        // the log-density form (gpk_kmat_vjp): G = 1/2 (A diag(g) A^T - sum(g) Kinv) over the lower triangle of a symmetric Kinv
        const int C2 = 2;
        auto Kh = randv<T>((size_t)n * n), A = randv<T>((size_t)n * C2);
        for (int i = 0; i < n; ++i) for (int j = 0; j < i; ++j) Kh[(size_t)j * n + i] = Kh[(size_t)i * n + j];
        double g[C2] = {0.7, -0.2};
        const int64_t nb = gpk_kmat_vjp_blocks(n);
        Dev<T> dK(Kh.size()), dA(A.size()), dP2((size_t)nb * W), dDg(n);
        dK.up(Kh); dA.up(A);
        st = gpk_kmat_vjp(DT<T>::v, kinds, il, sh, nt, dX.p, n, d, d, dK.p, n, dA.p, C2, C2, g, dP2.p, dDg.p, nullptr);
        HIPCHK(hipDeviceSynchronize());
        auto P2 = dP2.down();
        std::vector<double> rS2(3 * nt + 1, 0.0);
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < n; ++j) {
                double aa = 0;
                for (int c = 0; c < C2; ++c) aa += g[c] * (double)A[(size_t)i * C2 + c] * (double)A[(size_t)j * C2 + c];
                const double Gij = 0.5 * (aa - (g[0] + g[1]) * (double)Kh[(size_t)std::max(i, j) * n + std::min(i, j)]);
                double r2 = 0;
                for (int k = 0; k < d; ++k) { const double a = X[(size_t)i * d + k], c = X[(size_t)j * d + k]; r2 += (a - c) * (a - c); }
                for (int t = 0; t < nt; ++t) {
                    const double q = r2 * il[t] * il[t];
                    double k, dkq, dk, da = 0;
                    if (kinds[t] == GPK_K_RQ) kappa_rq_host(q, sh[t], k, dkq, dk, da); else kappa_all_host(kinds[t], q, k, dkq, dk);
                    rS2[3 * t] += Gij * k; rS2[3 * t + 1] += Gij * dkq; rS2[3 * t + 2] += Gij * da;
                }
                if (i == j) rS2[3 * nt] += Gij;
            }
        std::vector<T> gS2(3 * nt + 1, T(0));
        for (int64_t bk = 0; bk < nb; ++bk) {
            for (int t = 0; t < 3 * nt; ++t) gS2[t] += P2[(size_t)bk * W + t];
            gS2[3 * nt] += P2[(size_t)bk * W + 3 * GPK_MAX_TERMS];
        }
        report(std::string("kmat_vjp_") + DT<T>::name() + " rq+eq+rq n130 d3 sums (S1, S2, S3, trace)", st ? INFINITY : relerr(gS2, rS2), DT<T>::eps * 50);
    }
}

// ----------------------------------------------------------------------------
// Derivative blocks of the kernel matrix (gpk_kmat_diff)   --diff
// ----------------------------------------------------------------------------
// Element by element against the closed forms of include/gpk.h in long double, on the inputs as the dtype holds them:
// |got - ref| <= DIFF_TOL eps absum, absum = sum_t |v_t| (|first addend| + |second addend|) (1 + |argument of the exponential|).
// DIFF_TOL = 8: ~2.5 eps (1 + |arg|) for an exponential (gpk_kmat's own figure), one rounding each for the scaled distance, the
// difference D_a, the products with c, v and the profile's constant, and the sum over terms.
static const double DIFF_TOL = 8.0;
struct DiffTable { const char* name; int nt; int kinds[8]; double var[8], scale[8], shape[8]; bool shaped; };
static const DiffTable DIFF_TABLES[] = {
    {"eq", 1, {GPK_K_EQ}, {1.5}, {0.75}, {0}, false},
    {"matern32", 1, {GPK_K_MATERN32}, {0.75}, {1.25}, {0}, false},
    {"rq0.7", 1, {GPK_K_RQ}, {1.25}, {1.5}, {0.7}, true},
    {"eq+linear+const", 3, {GPK_K_EQ, GPK_K_LINEAR, GPK_K_CONST}, {1.0, 0.5, 0.25}, {1.5, 2.0, 1.0}, {0, 0, 0}, false},
    {"all8", 8, {GPK_K_EQ, GPK_K_MATERN32, GPK_K_MATERN52, GPK_K_RQ, GPK_K_LINEAR, GPK_K_CONST, GPK_K_EQ, GPK_K_RQ},
     {1.0, 0.5, 0.75, 1.25, 0.25, 2.0, 0.5, 0.375}, {1.0, 2.0, 1.5, 0.75, 4.0, 1.0, 3.0, 2.5}, {0, 0, 0, 0.7, 0, 0, 0, 3.0}, true},
};
// value and absum of one element; mode 0: d/dx_a, 1: d/dy_b, 2: d2/dx_a dy_b
template <typename T>
static void diff_ref(const DiffTable& tb, const T* x, const T* y, int d, int a, int b, int mode, long double* val, long double* absum) {
    long double r2 = 0;
    for (int k = 0; k < d; ++k) { const long double df = (long double)x[k] - (long double)y[k]; r2 += df * df; }
    const long double da = a >= 0 ? (long double)x[a] - (long double)y[a] : 0, db = b >= 0 ? (long double)x[b] - (long double)y[b] : 0;
    long double v = 0, ab = 0;
    for (int t = 0; t < tb.nt; ++t) {
        const long double il = (long double)(1.0 / tb.scale[t]), c = il * il, var = tb.var[t], q = c * r2;
        long double k1 = 0, k2dd = 0, arg = 0;
        switch (tb.kinds[t]) {
            case GPK_K_CONST: continue;
            case GPK_K_LINEAR: {
                const long double term = mode == 0 ? c * var * (long double)y[a] : mode == 1 ? c * var * (long double)x[b] : (a == b ? c * var : 0);
                v += term; ab += fabsl(term);
                continue;
            }
            case GPK_K_EQ: { const long double e = expl(-q / 2); k1 = -e / 2; k2dd = e / 4 * da * db; arg = q / 2; break; }
            case GPK_K_RQ: {
                const long double al = tb.shape[t], l = log1pl(q / (2 * al));
                k1 = -expl(-(al + 1) * l) / 2; k2dd = (al + 1) / (4 * al) * expl(-(al + 2) * l) * da * db; arg = (al + 2) * l; break;
            }
            case GPK_K_MATERN52: { const long double sd = sqrtl(5 * q), e = expl(-sd); k1 = -5.0L / 6 * (1 + sd) * e; k2dd = 25.0L / 12 * e * da * db; arg = sd; break; }
            default: { const long double sd = sqrtl(3 * q), e = expl(-sd); k1 = -1.5L * e; k2dd = sd > 0 ? 2.25L * e * da * db / sd : 0; arg = sd; break; }
        }
        long double first, second = 0;
        if (mode == 0) first = 2 * c * var * k1 * da;
        else if (mode == 1) first = -2 * c * var * k1 * db;
        else { first = -4 * c * c * var * k2dd; second = a == b ? -2 * c * var * k1 : 0; }
        v += first + second;
        ab += (fabsl(first) + fabsl(second)) * (1 + arg);
    }
    *val = v; *absum = ab;
}
template <typename T>
static void test_diff() {
    const double eps = (double)std::numeric_limits<T>::epsilon();
    for (int band = 1; band >= 0; --band) {
        gpk_tune(12, band);
        const char* kn = band ? "row-band" : "tile";
        for (const DiffTable& tb : DIFF_TABLES) {
            double ils[8];
            for (int t = 0; t < tb.nt; ++t) ils[t] = 1.0 / tb.scale[t];
            for (int d : {1, 3, 8, 9}) {                   // (d = 9: past one staged chunk -- the tile kernel whatever the knob says)
                double worst[3] = {0, 0, 0};
                int status = 0;
                size_t nonzero_coincident = 0, nans = 0;
                for (int shape = 0; shape < 3; ++shape) {
                    const int n = shape == 0 ? 1 : shape == 1 ? 33 : 97, m = shape == 0 ? 1 : shape == 1 ? 65 : 259;
                    auto X = randv<T>((size_t)n * d, 1.0 / sqrt((double)d)), Y = randv<T>((size_t)m * d, 1.0 / sqrt((double)d));
                    for (int j = 0; j < m; j += 5) for (int k = 0; k < d; ++k) Y[(size_t)j * d + k] = X[(size_t)((j * 7) % n) * d + k];      // coincident points
                    Dev<T> dX(X.size()), dY(Y.size()), dO((size_t)n * m);
                    dX.up(X); dY.up(Y);
                    const int dimsets[4][2] = {{0, 0}, {d - 1, 0}, {0, d - 1}, {d - 1, d - 1}};
                    for (int ds = 0; ds < (d > 1 ? 4 : 1); ++ds)
                        for (int mode = 0; mode < 3; ++mode) {
                            const int a = mode == 1 ? -1 : dimsets[ds][0], b = mode == 0 ? -1 : dimsets[ds][1];
                            status |= gpk_kmat_diff(DT<T>::v, tb.kinds, tb.var, ils, tb.shaped ? tb.shape : nullptr, tb.nt, a, b, dX.p, n, d, 0, dY.p, m, d, 0, d,
                                                    dO.p, m, 0, 1, 0, 0, 0.0, nullptr, 0, 0, nullptr);
                            HIPCHK(hipDeviceSynchronize());
                            auto got = dO.down();
                            for (int i = 0; i < n; ++i)
                                for (int j = 0; j < m; ++j) {
                                    long double v, ab;
                                    diff_ref<T>(tb, &X[(size_t)i * d], &Y[(size_t)j * d], d, a, b, mode, &v, &ab);
                                    const long double g = got[(size_t)i * m + j];
                                    if (g != g) { ++nans; continue; }
                                    const double e = ab > 0 ? (double)(fabsl(g - v) / ab) / eps : (g == 0 ? 0.0 : INFINITY);
                                    worst[mode] = std::max(worst[mode], e);
                                    // one-sided blocks of a stationary table are exactly 0 at coincident points
                                    if (mode < 2 && j % 5 == 0 && i == (j * 7) % n && strcmp(tb.name, "eq+linear+const") && strcmp(tb.name, "all8")) nonzero_coincident += g != 0;
                                }
                        }
                }
                char nm[200];
                snprintf(nm, sizeof nm, "kmat_diff_%s %s %s d%d: worst |err| / (eps absum) dx %.2f dy %.2f dxy %.2f (%zu NaN, %zu nonzero coincident) st%d", DT<T>::name(), tb.name, kn,
                         d, worst[0], worst[1], worst[2], nans, nonzero_coincident, status);
                report(nm, (status || nans || nonzero_coincident) ? INFINITY : std::max(worst[0], std::max(worst[1], worst[2])), DIFF_TOL);
            }
        }
        // symmetric, lower-only, diag_add + diag_vec, n = 130: the lower triangle bit for bit the full launch's, skipped tiles untouched
        for (int d : {3, 9}) {
            const DiffTable& tb = DIFF_TABLES[4];
            double ils[8];
            for (int t = 0; t < tb.nt; ++t) ils[t] = 1.0 / tb.scale[t];
            const int n = 130, a = d - 1;
            auto X = randv<T>((size_t)n * d, 1.0 / sqrt((double)d));
            std::vector<T> dv(n);
            for (int i = 0; i < n; ++i) dv[i] = (T)((i % 16) / 8.0);
            Dev<T> dX(X.size()), dV(n), dF((size_t)n * n), dL((size_t)n * n);
            dX.up(X); dV.up(dv);
            std::vector<T> fill((size_t)n * n, (T)-7);
            dL.up(fill);
            int st = gpk_kmat_diff(DT<T>::v, tb.kinds, tb.var, ils, tb.shape, tb.nt, a, a, dX.p, n, d, 0, dX.p, n, d, 0, d, dF.p, n, 0, 1, 0, 1, 0.25, dV.p, 0, 0, nullptr);
            st |= gpk_kmat_diff(DT<T>::v, tb.kinds, tb.var, ils, tb.shape, tb.nt, a, a, dX.p, n, d, 0, dX.p, n, d, 0, d, dL.p, n, 0, 1, 1, 1, 0.25, dV.p, 0, 0, nullptr);
            HIPCHK(hipDeviceSynchronize());
            auto full = dF.down(), low = dL.down();
            size_t bad = 0;
            double worst = 0;
            const int TN = 64 * (16 / (int)sizeof(T));
            for (int i = 0; i < n; ++i)
                for (int j = 0; j < n; ++j) {
                    if (j <= i) bad += memcmp(&full[(size_t)i * n + j], &low[(size_t)i * n + j], sizeof(T)) != 0;
                    else if ((j / TN) * TN > (i / 32) * 32 + 31) bad += low[(size_t)i * n + j] != (T)-7;      // a skipped tile
                    long double v, ab;
                    diff_ref<T>(tb, &X[(size_t)i * d], &X[(size_t)j * d], d, a, a, 2, &v, &ab);
                    if (i == j) { v += 0.25L + (long double)dv[i]; ab += 0.25L + (long double)dv[i]; }
                    worst = std::max(worst, (double)(fabsl((long double)full[(size_t)i * n + j] - v) / ab) / eps);
                }
            char nm[200];
            snprintf(nm, sizeof nm, "kmat_diff_%s all8 %s d%d symmetric n130 + diag: %zu lower-only mismatches st%d", DT<T>::name(), kn, d, bad, st);
            report(nm, (st || bad) ? INFINITY : worst, DIFF_TOL);
        }
    }
    gpk_tune(12, 1);
    {   // the argument codes (include/gpk.h)
        int eq = GPK_K_EQ, m12 = GPK_K_MATERN12, rq = GPK_K_RQ;
        double one = 1.0, zero = 0.0;
        Dev<T> dX(8), dO(16);
        auto call = [&](const int* kind, const double* shapes, int nt, int a, int b, int d, int lower, int sym) {
            return gpk_kmat_diff(DT<T>::v, kind, &one, &one, shapes, nt, a, b, dX.p, 2, d, 0, dX.p, 2, d, 0, d, dO.p, 2, 0, 1, lower, sym, 0.0, nullptr, 0, 0, nullptr);
        };
        const int got[] = {call(&m12, nullptr, 1, 0, 0, 2, 0, 0), call(&rq, nullptr, 1, 0, 0, 2, 0, 0), call(&rq, &zero, 1, 0, 0, 2, 0, 0), call(&eq, nullptr, 9, 0, 0, 2, 0, 0),
                           call(&eq, nullptr, 1, 2, 0, 2, 0, 0), call(&eq, nullptr, 1, -1, -1, 2, 0, 0), call(&eq, nullptr, 1, 0, 2, 2, 0, 0),
                           call(&eq, nullptr, 1, 0, 1, 2, 0, 1), call(&eq, nullptr, 1, 0, -1, 2, 1, 0), call(&eq, nullptr, 1, 1, 1, 2, 1, 1)};
        const int want[] = {-2, -1, -5, -6, -7, -7, -8, -23, -23, 0};
        HIPCHK(hipDeviceSynchronize());
        int bad = 0;
        for (int i = 0; i < 10; ++i) bad += got[i] != want[i];
        report(std::string("kmat_diff_") + DT<T>::name() + " argument codes", (double)bad, 0.0);
    }
}

// ----------------------------------------------------------------------------
// Delta: 1 where the scaled squared distance is below epsilon, else 0 (epsilon in `shapes` of gpk_kmat / gpk_kdiag and the VJP entries)   --delta
// ----------------------------------------------------------------------------
// Inputs are small integers over 4 with rows of y copied from x: every squared distance is 0 or at least 1/16, computed without
// rounding in both dtypes, so the host evaluates the kernel EXACTLY and every element has to match bit for bit -- Delta alone, beside
// a constant term, lower-only (nothing above the diagonal tiles is written), accumulated into a filled buffer, through both kernels.
template <typename T>
static std::vector<T> quarters(size_t n, int span) {
    std::vector<T> v(n);
    for (auto& x : v) x = (T)((int)(rng() % (2 * span + 1)) - span) / (T)4;
    return v;
}
// gpk_kmat_batch_terms / gpk_kdiag_batch_terms (one term table per batch entry, on the device): entry b of ONE launch against gpk_kmat /
// gpk_kdiag on entry b alone with row b of the tables as host arrays -- the same element program on the same numbers, so bit for bit.
// Run under both values of knob 12: the one-tile kernel at d = 3 is a path the release library never takes.
template <typename T>
static void test_batch_terms() {
    const int B = 3, n = 130, m = 97, pad = 2;
    struct Case { const char* name; std::vector<int> kinds; };
    const std::vector<Case> cases = {{"eq", {GPK_K_EQ}}, {"matern52", {GPK_K_MATERN52}}, {"rq", {GPK_K_RQ}}, {"eq+linear", {GPK_K_EQ, GPK_K_LINEAR}},
                                     {"table3", {GPK_K_MATERN32, GPK_K_EQ, GPK_K_CONST}},
                                     {"all8", {GPK_K_EQ, GPK_K_MATERN12, GPK_K_MATERN32, GPK_K_MATERN52, GPK_K_LINEAR, GPK_K_CONST, GPK_K_RQ, GPK_K_DELTA}}};
    for (int d : {3, 9}) {
        auto hx = randv<T>((size_t)B * n * d), hy = randv<T>((size_t)B * m * d);
        for (int b = 0; b < B; ++b)
            for (int i = 0; i < 20 * d; ++i) hy[(size_t)b * m * d + i] = hx[(size_t)b * n * d + i];     // coincident points: the Delta term is 1 there
        Dev<T> dX(hx.size()), dY(hy.size()), dO((size_t)B * n * m), dR((size_t)B * n * m), dOd((size_t)B * n), dRd((size_t)B * n);
        dX.up(hx); dY.up(hy);
        for (const Case& c : cases) {
            const int nt = (int)c.kinds.size(), st_ = nt + pad;       // rows of the tables padded: the stride is not nterms
            std::vector<double> var((size_t)B * st_, NAN), ils((size_t)B * st_, NAN), shp((size_t)B * st_, NAN);
            for (int b = 0; b < B; ++b)
                for (int t = 0; t < nt; ++t) {
                    var[b * st_ + t] = 0.5 + 0.25 * ((b + t) % 5);
                    ils[b * st_ + t] = 1.0 / (0.7 + 0.6 * ((b + 2 * t) % 3));
                    shp[b * st_ + t] = c.kinds[t] == GPK_K_DELTA ? 1e-6 * (b + 1) : 0.8 + 1.1 * b;
                }
            Dev<double> dV(var.size()), dI(ils.size()), dS(shp.size());
            dV.up(var); dI.up(ils); dS.up(shp);
            int st = gpk_kmat_batch_terms(DT<T>::v, c.kinds.data(), dV.p, dI.p, dS.p, nt, st_, dX.p, n, d, (int64_t)n * d, dY.p, m, d, (int64_t)m * d, d,
                                          dO.p, m, (int64_t)n * m, B, 0, 0, 0.0, nullptr, 0, 0, nullptr);
            st |= gpk_kdiag_batch_terms(DT<T>::v, c.kinds.data(), dV.p, dI.p, dS.p, nt, st_, dX.p, n, d, (int64_t)n * d, d, dOd.p, n, B, nullptr);
            for (int b = 0; b < B; ++b) {
                st |= gpk_kmat(DT<T>::v, c.kinds.data(), &var[b * st_], &ils[b * st_], &shp[b * st_], nt, dX.p + (size_t)b * n * d, n, d, 0,
                               dY.p + (size_t)b * m * d, m, d, 0, d, dR.p + (size_t)b * n * m, m, 0, 1, 0, 0, 0.0, nullptr, 0, 0, nullptr);
                st |= gpk_kdiag(DT<T>::v, c.kinds.data(), &var[b * st_], &ils[b * st_], &shp[b * st_], nt, dX.p + (size_t)b * n * d, n, d, 0, d,
                                dRd.p + (size_t)b * n, 0, 1, nullptr);
            }
            HIPCHK(hipDeviceSynchronize());
            const auto got = dO.down(), ref = dR.down(), gotd = dOd.down(), refd = dRd.down();
            size_t bad = 0, nan = 0;
            for (size_t i = 0; i < got.size(); ++i) { bad += memcmp(&got[i], &ref[i], sizeof(T)) != 0; nan += !std::isfinite((double)got[i]); }
            for (size_t i = 0; i < gotd.size(); ++i) bad += memcmp(&gotd[i], &refd[i], sizeof(T)) != 0;
            report(std::string("batch_terms ") + DT<T>::name() + " " + c.name + " d=" + std::to_string(d) + " differing elements (status " + std::to_string(st) + ")",
                   (double)(bad + nan + (st != 0)), 0.0);
        }
    }
}

template <typename T>
static void test_delta() {
    const double eps = 1e-6;
    for (int band = 1; band >= 0; --band) {
        gpk_tune(12, band);
        const char* kn = band ? "row-band" : "tile";
        for (int d : {1, 3, 8, 9}) {                       // (d = 9: past one staged chunk -- the tile kernel whatever the knob says)
            const int n = 130, m = 259;
            auto X = quarters<T>((size_t)n * d, d == 1 ? 40 : 2), Y = quarters<T>((size_t)m * d, d == 1 ? 40 : 2);
            for (int j = 0; j < m; j += 3) for (int k = 0; k < d; ++k) Y[(size_t)j * d + k] = X[(size_t)((j * 7) % n) * d + k];
            Dev<T> dX(X.size()), dY(Y.size()), dO((size_t)n * m);
            dX.up(X); dY.up(Y);
            int kinds[2] = {GPK_K_DELTA, GPK_K_CONST};
            double var[2] = {1.5, 0.25}, sh[2] = {eps, 0.0};
            for (double il : {1.0, 0.5}) {                 // (power-of-two scales keep q exact: 0 or >= 1/64)
                double ils[2] = {il, 1.0};
                for (int nt = 1; nt <= 2; ++nt) {
                    for (int acc = 0; acc < 2; ++acc) {
                        std::vector<T> base((size_t)n * m);
                        for (size_t e = 0; e < base.size(); ++e) base[e] = (T)((int)(e % 7) - 3);
                        dO.up(base);
                        int st = gpk_kmat(DT<T>::v, kinds, var, ils, sh, nt, dX.p, n, d, 0, dY.p, m, d, 0, d, dO.p, m, 0, 1, 0, 0, 0.0, nullptr, 0, acc, nullptr);
                        HIPCHK(hipDeviceSynchronize());
                        auto got = dO.down();
                        size_t bad = 0, ones = 0;
                        for (int i = 0; i < n; ++i)
                            for (int j = 0; j < m; ++j) {
                                bool same = true;
                                for (int k = 0; k < d; ++k) same = same && X[(size_t)i * d + k] == Y[(size_t)j * d + k];
                                const T want = (T)((acc ? base[(size_t)i * m + j] : T(0)) + (T)(same ? 1.5 : 0.0) + (T)(nt == 2 ? 0.25 : 0.0));
                                ones += same;
                                bad += got[(size_t)i * m + j] != want;
                            }
                        char nm[200];
                        snprintf(nm, sizeof nm, "kmat_%s delta%s %s d%d il=%g%s: mismatching elements (%zu ones) st%d", DT<T>::name(), nt == 2 ? "+const" : "", kn, d, il,
                                 acc ? " accumulate" : "", ones, st);
                        report(nm, (st || ones < (size_t)m / 3) ? INFINITY : (double)bad, 0.0);
                    }
                }
            }
            // symmetric, lower-only, diag_add: tiles above the diagonal keep what was there, the diagonal is variance + diag_add
            {
                Dev<T> dS((size_t)n * n);
                std::vector<T> fill((size_t)n * n, (T)-7);
                dS.up(fill);
                for (int i = 100; i < n; ++i) for (int k = 0; k < d; ++k) X[(size_t)i * d + k] = X[(size_t)(i - 100) * d + k];
                dX.up(X);
                double one = 1.0;
                int st = gpk_kmat(DT<T>::v, kinds, var, &one, sh, 1, dX.p, n, d, 0, dX.p, n, d, 0, d, dS.p, n, 0, 1, 1, 1, 0.5, nullptr, 0, 0, nullptr);
                HIPCHK(hipDeviceSynchronize());
                auto got = dS.down();
                size_t bad = 0;
                const int TN = 64 * (16 / (int)sizeof(T));
                for (int i = 0; i < n; ++i)
                    for (int j = 0; j < n; ++j) {
                        bool same = true;
                        for (int k = 0; k < d; ++k) same = same && X[(size_t)i * d + k] == X[(size_t)j * d + k];
                        const T want = (T)((same ? 1.5 : 0.0) + (i == j ? 0.5 : 0.0));
                        if (j <= i) bad += got[(size_t)i * n + j] != want;
                        else if ((j / TN) * TN > (i / 32) * 32 + 31) bad += got[(size_t)i * n + j] != (T)-7;      // a skipped tile
                    }
                char nm[200];
                snprintf(nm, sizeof nm, "kmat_%s delta %s d%d symmetric lower-only + diag_add: mismatching elements st%d", DT<T>::name(), kn, d, st);
                report(nm, st ? INFINITY : (double)bad, 0.0);
            }
        }
    }
    gpk_tune(12, 1);
    {   // a NaN input row gives a NaN row; the two return codes; the diagonal
        const int n = 33, m = 65, d = 3;
        auto X = quarters<T>((size_t)n * d, 2), Y = quarters<T>((size_t)m * d, 2);
        X[5 * d + 1] = std::numeric_limits<T>::quiet_NaN();
        Dev<T> dX(X.size()), dY(Y.size()), dO((size_t)n * m), dD(n);
        dX.up(X); dY.up(Y);
        int kind = GPK_K_DELTA; double var = 1.5, il = 1.0, sh = eps, bad = 0.0;
        int st = gpk_kmat(DT<T>::v, &kind, &var, &il, &sh, 1, dX.p, n, d, 0, dY.p, m, d, 0, d, dO.p, m, 0, 1, 0, 0, 0.0, nullptr, 0, 0, nullptr);
        HIPCHK(hipDeviceSynchronize());
        auto got = dO.down();
        size_t wrong = 0;
        for (int i = 0; i < n; ++i) for (int j = 0; j < m; ++j) wrong += (i == 5) != (got[(size_t)i * m + j] != got[(size_t)i * m + j]);
        report(std::string("kmat delta: a NaN input row is a NaN row, no other ") + DT<T>::name(), st ? INFINITY : (double)wrong, 0.0);
        st = gpk_kmat(DT<T>::v, &kind, &var, &il, nullptr, 1, dX.p, n, d, 0, dY.p, m, d, 0, d, dO.p, m, 0, 1, 0, 0, 0.0, nullptr, 0, 0, nullptr);
        report(std::string("kmat refuses a delta term (no epsilon) with -1 ") + DT<T>::name(), st == -1 ? 0.0 : INFINITY, 0.0);
        st = gpk_kmat(DT<T>::v, &kind, &var, &il, &bad, 1, dX.p, n, d, 0, dY.p, m, d, 0, d, dO.p, m, 0, 1, 0, 0, 0.0, nullptr, 0, 0, nullptr);
        report(std::string("kmat refuses epsilon <= 0 with -5 ") + DT<T>::name(), st == -5 ? 0.0 : INFINITY, 0.0);
        st = gpk_kdiag(DT<T>::v, &kind, &var, &il, nullptr, 1, dX.p, n, d, 0, d, dD.p, n, 1, nullptr);
        report(std::string("kdiag refuses a delta term with -1 ") + DT<T>::name(), st == -1 ? 0.0 : INFINITY, 0.0);
        st = gpk_kdiag(DT<T>::v, &kind, &var, &il, &bad, 1, dX.p, n, d, 0, d, dD.p, n, 1, nullptr);
        report(std::string("kdiag refuses epsilon <= 0 with -5 ") + DT<T>::name(), st == -5 ? 0.0 : INFINITY, 0.0);
        int k2[2] = {GPK_K_DELTA, GPK_K_LINEAR}; double v2[2] = {0.75, 1.5}, l2[2] = {1.0, 0.5}, s2[2] = {eps, 0.0};
        X[5 * d + 1] = (T)0.25;
        dX.up(X);
        st = gpk_kdiag(DT<T>::v, k2, v2, l2, s2, 2, dX.p, n, d, 0, d, dD.p, n, 1, nullptr);
        HIPCHK(hipDeviceSynchronize());
        auto dg = dD.down();
        size_t wd = 0;
        for (int i = 0; i < n; ++i) { double nr = 0; for (int k = 0; k < d; ++k) nr += (double)X[i * d + k] * X[i * d + k]; wd += (double)dg[i] != 0.75 + 1.5 * 0.25 * nr; }
        report(std::string("kdiag delta + linear: mismatching elements ") + DT<T>::name(), st ? INFINITY : (double)wd, 0.0);
        // the VJP entries: -1 without shapes, -5 for a bad epsilon
        Dev<T> dG((size_t)n * m), dP((size_t)64 * (3 * GPK_MAX_TERMS + 1)), dK((size_t)n * n), dA(n), dDg(n);
        double g1 = 1.0;
        st = gpk_kmat_vjp_dense(DT<T>::v, &kind, &var, &il, nullptr, 1, dX.p, n, d, dY.p, m, d, d, dG.p, m, nullptr, nullptr, nullptr, dP.p, nullptr, nullptr, nullptr);
        report(std::string("vjp_dense refuses a delta term with -1 ") + DT<T>::name(), st == -1 ? 0.0 : INFINITY, 0.0);
        st = gpk_kmat_vjp_dense(DT<T>::v, &kind, &var, &il, &bad, 1, dX.p, n, d, dY.p, m, d, d, dG.p, m, nullptr, nullptr, nullptr, dP.p, nullptr, nullptr, nullptr);
        report(std::string("vjp_dense refuses epsilon <= 0 with -5 ") + DT<T>::name(), st == -5 ? 0.0 : INFINITY, 0.0);
        st = gpk_kmat_vjp(DT<T>::v, &kind, &il, nullptr, 1, dX.p, n, d, d, dK.p, n, dA.p, 1, 1, &g1, dP.p, dDg.p, nullptr);
        report(std::string("kmat_vjp refuses a delta term with -1 ") + DT<T>::name(), st == -1 ? 0.0 : INFINITY, 0.0);
        st = gpk_kmat_vjp(DT<T>::v, &kind, &il, &bad, 1, dX.p, n, d, d, dK.p, n, dA.p, 1, 1, &g1, dP.p, dDg.p, nullptr);
        report(std::string("kmat_vjp refuses epsilon <= 0 with -5 ") + DT<T>::name(), st == -5 ? 0.0 : INFINITY, 0.0);
    }
    {   // explicit-cotangent VJP, Delta beside EQ: S1 = sum Geff kappa, S2 = S3 = 0 exactly, kappa in colsum, nothing in gradx
        const int n = 130, m = 259, d = 3, nt = 2;
        int kinds[nt] = {GPK_K_EQ, GPK_K_DELTA};
        double var[nt] = {0.75, 1.5}, il[nt] = {1.0, 1.0}, sh[nt] = {0.0, eps};
        auto X = quarters<T>((size_t)n * d, 2), Y = quarters<T>((size_t)m * d, 2), G = randv<T>((size_t)n * m);
        int64_t rt = 0, nc = 0;
        gpk_kmat_vjp_dense_grid(n, m, &rt, &nc);
        const int W = 3 * GPK_MAX_TERMS + 1;
        Dev<T> dX(X.size()), dY(Y.size()), dG(G.size()), dP((size_t)rt * nc * W), dC((size_t)rt * m), dGX((size_t)nc * n * d);
        dX.up(X); dY.up(Y); dG.up(G);
        int st = gpk_kmat_vjp_dense(DT<T>::v, kinds, var, il, sh, nt, dX.p, n, d, dY.p, m, d, d, dG.p, m, nullptr, nullptr, nullptr, dP.p, dC.p, dGX.p, nullptr);
        HIPCHK(hipDeviceSynchronize());
        auto P = dP.down(), C = dC.down(), GX = dGX.down();
        std::vector<double> rS(2, 0.0), rC(m, 0.0), rGX((size_t)n * d, 0.0);
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < m; ++j) {
                double r2 = 0;
                for (int k = 0; k < d; ++k) { const double a = X[(size_t)i * d + k], c = Y[(size_t)j * d + k]; r2 += (a - c) * (a - c); }
                const double ge = G[(size_t)i * m + j], kd = r2 < eps ? 1.0 : 0.0;
                rS[0] += ge * std::exp(-0.5 * r2); rS[1] += ge * kd;
                rC[j] += ge * (0.75 * std::exp(-0.5 * r2) + 1.5 * kd);
                for (int c = 0; c < d; ++c) rGX[(size_t)i * d + c] += ge * 0.75 * -std::exp(-0.5 * r2) * ((double)X[(size_t)i * d + c] - (double)Y[(size_t)j * d + c]);
            }
        std::vector<T> gS(2, T(0)), gC(m, T(0)), gGX((size_t)n * d, T(0));
        for (int64_t c = 0; c < nc; ++c) for (size_t e = 0; e < (size_t)n * d; ++e) gGX[e] += GX[(size_t)c * n * d + e];
        bool zeros = true;
        for (int64_t wg = 0; wg < rt * nc; ++wg) {
            gS[0] += P[(size_t)wg * W]; gS[1] += P[(size_t)wg * W + 3];
            zeros = zeros && P[(size_t)wg * W + 4] == T(0) && P[(size_t)wg * W + 5] == T(0);
        }
        for (int64_t r = 0; r < rt; ++r) for (int j = 0; j < m; ++j) gC[j] += C[(size_t)r * m + j];
        std::string nm = std::string("vjp_dense_") + DT<T>::name() + " eq+delta n130 m259 d3";
        report(nm + " S1", st ? INFINITY : relerr(gS, rS), DT<T>::eps * 50);
        report(nm + " S2 = S3 = 0 for the delta term", zeros ? 0.0 : INFINITY, 0.0);
        report(nm + " colsum", st ? INFINITY : relerr(gC, rC), DT<T>::eps * 50);
        report(nm + " gradx (the eq term's alone)", st ? INFINITY : relerr(gGX, rGX), DT<T>::eps * 50);
    }
}

// ----------------------------------------------------------------------------
// perf
// ----------------------------------------------------------------------------
struct Timer {
    hipEvent_t a, b;
    Timer() { hipEventCreate(&a); hipEventCreate(&b); }
    void start() { hipEventRecord(a, 0); }
    float stop() { hipEventRecord(b, 0); hipEventSynchronize(b); float ms; hipEventElapsedTime(&ms, a, b); return ms; }
};
template <typename T>
static void perf() {
    Timer tm;
    const double peak = sizeof(T) == 8 ? 78.6 : 157.3;
    // GEMM NT
    for (int n : {4096, 8192}) {
        Dev<T> A((size_t)n * n), B((size_t)n * n), C((size_t)n * n);
        auto h = randv<T>((size_t)n * n);
        A.up(h); B.up(h); C.zero();
        for (int rep = 0; rep < 2; ++rep) {
            tm.start();
            gpk_gemm(DT<T>::v, 1, 1, n, n, n, -1.0, A.p, n, 0, B.p, n, 0, 1.0, C.p, n, 0, 1, 0, nullptr);
            const float ms = tm.stop();
            const double tf = 2.0 * n * n * (double)n / ms * 1e-9;
            printf("PERF gemm_nt_%s n=%d  %.3f ms  %.2f TFLOP/s  (%.1f%% of %.1f)\n", DT<T>::name(), n, ms, tf, 100 * tf / peak, peak);
        }
    }
    // SYRK-like trailing update: M=N=16384-ish, K=256, lower
    for (int k : {128, 256, 512}) {
        const int n = 12288;
        Dev<T> P((size_t)n * k), C((size_t)n * n);
        auto h = randv<T>((size_t)n * k);
        P.up(h); C.zero();
        for (int rep = 0; rep < 2; ++rep) {
            tm.start();
            gpk_gemm(DT<T>::v, 1, 1, n, n, k, -1.0, P.p, k, 0, P.p, k, 0, 1.0, C.p, n, 0, 1, 1, nullptr);
            const float ms = tm.stop();
            const double tf = 1.0 * n * (double)n * k / ms * 1e-9;
            printf("PERF syrk_lower_%s n=%d k=%d  %.3f ms  %.2f TFLOP/s (sym count) (%.1f%%)\n", DT<T>::name(), n, k, ms, tf, 100 * tf / peak);
        }
    }
    // kmat + potrf + trsv + trsm at growing N
    for (int n : {2048, 4096, 8192, 16384}) {
        const int d = 8;
        auto hx = randv<T>((size_t)n * d);
        Dev<T> X(hx.size()), K((size_t)n * n), dinv(gpk_dinv_elems(n));
        Dev<int> info(1);
        X.up(hx);
        int kind = GPK_K_EQ; double var = 1.0, il = 1.0;
        float ms_k = 0, ms_p = 0;
        for (int rep = 0; rep < 2; ++rep) {
            info.zero();
            tm.start();
            gpk_kmat(DT<T>::v, &kind, &var, &il, nullptr, 1, X.p, n, d, 0, X.p, n, d, 0, d, K.p, n, 0, 1, 1, 1, 0.1, nullptr, 0, 0, nullptr);
            ms_k = tm.stop();
            tm.start();
            gpk_potrf(DT<T>::v, K.p, n, n, 0, 1, dinv.p, info.p, 0, nullptr);
            ms_p = tm.stop();
        }
        const double tf = (double)n * n * n / 3.0 / ms_p * 1e-9;
        printf("PERF kmat_lower_%s n=%d d=%d  %.3f ms  %.1f GB/s (lower bytes)\n", DT<T>::name(), n, d, ms_k, 0.5 * n * (double)n * sizeof(T) / ms_k * 1e-6);
        printf("PERF potrf_%s n=%d  %.3f ms  %.2f TFLOP/s (%.1f%% of %.1f) info=%d\n", DT<T>::name(), n, ms_p, tf, 100 * tf / peak, peak, info.down()[0]);
        for (int nbo : {128, 512}) {
            info.zero();
            gpk_kmat(DT<T>::v, &kind, &var, &il, nullptr, 1, X.p, n, d, 0, X.p, n, d, 0, d, K.p, n, 0, 1, 1, 1, 0.1, nullptr, 0, 0, nullptr);
            tm.start();
            gpk_potrf(DT<T>::v, K.p, n, n, 0, 1, dinv.p, info.p, nbo, nullptr);
            const float ms = tm.stop();
            printf("PERF potrf_%s n=%d nbo=%d  %.3f ms  %.2f TFLOP/s\n", DT<T>::name(), n, nbo, ms, (double)n * n * n / 3.0 / ms * 1e-9);
        }
        // trsv (nrhs = 1), sb = 128
        {
            Dev<T> y(n), tmp(512 + GPK_TRSV_CTRL_ELEMS);
            auto hy = randv<T>(n);
            for (int rep = 0; rep < 2; ++rep) {
                y.up(hy);
                tm.start();
                gpk_trsv_lower(DT<T>::v, K.p, n, n, 0, dinv.p, 128, y.p, 1, 1, 0, tmp.p, 1, nullptr);
                const float ms = tm.stop();
                if (rep) printf("PERF trsv_%s n=%d sb=128  %.3f ms  %.1f GB/s\n", DT<T>::name(), n, ms, 0.5 * n * (double)n * sizeof(T) / ms * 1e-6);
            }
        }
        // merge + trsm (nrhs = 2048)
        for (int sb : {128, 512}) {
            const int nrhs = 2048;
            Dev<T> dsb((size_t)((n + sb - 1) / sb) * sb * sb), tmpm((size_t)((n + sb - 1) / sb) * sb * sb / 4 + 16), Bm((size_t)n * nrhs), tmp((size_t)sb * nrhs);
            auto hb = randv<T>((size_t)n * nrhs);
            Bm.up(hb);
            tm.start();
            gpk_trtri_merge(DT<T>::v, K.p, n, n, 0, 1, dinv.p, sb, dsb.p, tmpm.p, nullptr);
            const float ms_m = tm.stop();
            tm.start();
            gpk_trsm_lower(DT<T>::v, K.p, n, n, 0, dsb.p, sb, Bm.p, nrhs, nrhs, 0, tmp.p, 1, nullptr);
            const float ms = tm.stop();
            printf("PERF trsm_%s n=%d nrhs=%d sb=%d  merge %.3f ms  solve %.3f ms  %.2f TFLOP/s\n", DT<T>::name(), n, nrhs, sb, ms_m, ms, (double)n * n * nrhs / ms * 1e-9);
        }
    }
    // batched: 512 x 2048 (f32 config 4) -- only for float to bound memory/time
    if (sizeof(T) == 4) {
        const int n = 2048, d = 3, batch = 512;
        auto hx = randv<T>((size_t)batch * n * d);
        Dev<T> X(hx.size()), K((size_t)batch * n * n), dinv((size_t)batch * gpk_dinv_elems(n));
        Dev<int> info(batch);
        X.up(hx);
        int kind = GPK_K_EQ; double var = 1.0, il = 1.0;
        for (int rep = 0; rep < 2; ++rep) {
            info.zero();
            tm.start();
            gpk_kmat(DT<T>::v, &kind, &var, &il, nullptr, 1, X.p, n, d, (int64_t)n * d, X.p, n, d, (int64_t)n * d, d, K.p, n, (int64_t)n * n, batch, 1, 1, 0.1, nullptr, 0, 0, nullptr);
            const float ms_k = tm.stop();
            tm.start();
            gpk_potrf(DT<T>::v, K.p, n, n, (int64_t)n * n, batch, dinv.p, info.p, 0, nullptr);
            const float ms_p = tm.stop();
            printf("PERF batched_%s 512x2048: kmat %.3f ms, potrf %.3f ms  %.2f TFLOP/s\n", DT<T>::name(), ms_k, ms_p, batch * (double)n * n * n / 3.0 / ms_p * 1e-9);
        }
    }
}


// look-ahead Cholesky and persistent update, timed:  --perf-la
template <typename T>
static void perf_la(int nmax) {
    Timer tm;
    const double peak = sizeof(T) == 8 ? 78.6 : 157.3;
    // trailing-update shape of the first outer step at N = 16384, nbo = 1024
    {
        const int n = std::min(15360, nmax - 1024), k = 1024;
        Dev<T> P((size_t)(n + 1024) * k), C((size_t)n * n), Tn((size_t)n * 1024), Cs((size_t)n * 1024);
        Dev<unsigned> ctrl(64);
        P.up(randv<T>((size_t)(n + 1024) * k, 0.01)); C.zero(); Cs.zero();
        for (int rep = 0; rep < 2; ++rep) {
            tm.start();
            gpk_gemm(DT<T>::v, 1, 1, n, n, k, -1.0, P.p, k, 0, P.p, k, 0, 1.0, C.p, n, 0, 1, 1, nullptr);
            float ms = tm.stop();
            if (rep) printf("PERFLA trail_%s n=%d k=%d plain kernel        %.3f ms  %.2f TFLOP/s (%.1f%%)\n", DT<T>::name(), n, k, ms, 1.0 * n * (double)n * k / ms * 1e-9, 100.0 * n * (double)n * k / ms * 1e-9 / peak);
        }
        for (int reserve = 0; reserve < 2; ++reserve)
            for (int rep = 0; rep < 2; ++rep) {
                gpk_update_t u{n, n, k, P.p, k, P.p, k, C.p, n, C.p, n, 1};
                tm.start();
                gpk_gemm_update2(DT<T>::v, &u, 1, -1.0, ctrl.p, reserve, nullptr);
                float ms = tm.stop();
                if (rep) printf("PERFLA trail_%s n=%d k=%d persistent reserve=%d %.3f ms  %.2f TFLOP/s (%.1f%%)\n", DT<T>::name(), n, k, reserve, ms, 1.0 * n * (double)n * k / ms * 1e-9, 100.0 * n * (double)n * k / ms * 1e-9 / peak);
            }
        for (int rep = 0; rep < 2; ++rep) {   // strip (out of place) + triangle in one launch
            gpk_update_t u[2];
            u[0] = gpk_update_t{n, 1024, k, P.p + (size_t)1024 * k, k, P.p, k, Cs.p, 1024, Tn.p, 1024, 0};
            u[1] = gpk_update_t{n, n, k, P.p + (size_t)1024 * k, k, P.p + (size_t)1024 * k, k, C.p, n, C.p, n, 1};
            tm.start();
            gpk_gemm_update2(DT<T>::v, u, 2, -1.0, ctrl.p, 1, nullptr);
            float ms = tm.stop();
            const double fl = 1.0 * n * (double)n * k + 2.0 * n * 1024.0 * k;
            if (rep) printf("PERFLA trail_%s n=%d k=%d persistent strip+triangle reserve=1 %.3f ms  %.2f TFLOP/s (%.1f%%)\n", DT<T>::name(), n, k, ms, fl / ms * 1e-9, 100 * fl / ms * 1e-9 / peak);
        }
    }
    for (int n : {2048, 4096, 8192, 16384}) {
        if (n > nmax) continue;
        const int d = 8;
        auto hx = randv<T>((size_t)n * d);
        Dev<T> X(hx.size()), K((size_t)n * n), dinv(gpk_dinv_elems(n));
        Dev<int> info(1);
        X.up(hx);
        int kind = GPK_K_EQ; double var = 1.0, il = 1.0;
        for (int rep = 0; rep < 2; ++rep) {
            info.zero();
            gpk_kmat(DT<T>::v, &kind, &var, &il, nullptr, 1, X.p, n, d, 0, X.p, n, d, 0, d, K.p, n, 0, 1, 1, 1, 0.1, nullptr, 0, 0, nullptr);
            tm.start();
            gpk_potrf(DT<T>::v, K.p, n, n, 0, 1, dinv.p, info.p, 0, nullptr);
            const float ms = tm.stop();
            if (rep) printf("PERFLA potrf_%s n=%d plain            %.3f ms  %.2f TFLOP/s (%.1f%%)\n", DT<T>::name(), n, ms, (double)n * n * n / 3.0 / ms * 1e-9, 100 * (double)n * n * n / 3.0 / ms * 1e-9 / peak);
        }
        for (int nb : {512, 1024}) {
            Dev<T> dbig((size_t)((n + nb - 1) / nb) * nb * nb), ws((size_t)gpk_potrf_la_ws_elems(n, nb));
            for (int cfg = 0; cfg < 4; ++cfg) {
                const int mode = cfg == 0 ? 0 : 1;
                const int64_t minrows = cfg == 1 ? 0 : (cfg == 2 ? 2048 : 4096);
                gpk_tune(7, mode); gpk_tune(6, minrows);
                float best = 1e30f;
                for (int rep = 0; rep < 3; ++rep) {
                    info.zero();
                    gpk_kmat(DT<T>::v, &kind, &var, &il, nullptr, 1, X.p, n, d, 0, X.p, n, d, 0, d, K.p, n, 0, 1, 1, 1, 0.1, nullptr, 0, 0, nullptr);
                    tm.start();
                    gpk_potrf_la(DT<T>::v, K.p, n, n, dinv.p, dbig.p, nb, ws.p, info.p, nullptr);
                    const float ms = tm.stop();
                    if (rep) best = std::min(best, ms);
                }
                printf("PERFLA potrf_%s n=%d look-ahead nb=%d mode=%d minrows=%lld  %.3f ms  %.2f TFLOP/s (%.1f%%) info=%d\n", DT<T>::name(), n, nb, mode, (long long)minrows, best,
                       (double)n * n * n / 3.0 / best * 1e-9, 100 * (double)n * n * n / 3.0 / best * 1e-9 / peak, info.down()[0]);
            }
            gpk_tune(7, 1); gpk_tune(6, 2048);
        }
    }
}


// --perf-la-tail: plain (pipelined panels) against look-ahead at several orders, outer blocks and plain-tail lengths
template <typename T>
static void perf_la_tail(std::initializer_list<int> ns) {
    Timer tm;
    for (int n : ns) {
        const int d = 8;
        auto hx = randv<T>((size_t)n * d);
        Dev<T> X(hx.size()), K((size_t)n * n), dinv(gpk_dinv_elems(n));
        Dev<int> info(1);
        X.up(hx);
        int kind = GPK_K_EQ; double var = 1.0, il = 1.0;
        auto run = [&](auto&& call) {
            float best = 1e30f;
            for (int rep = 0; rep < 3; ++rep) {
                info.zero();
                gpk_kmat(DT<T>::v, &kind, &var, &il, nullptr, 1, X.p, n, d, 0, X.p, n, d, 0, d, K.p, n, 0, 1, 1, 1, 0.1, nullptr, 0, 0, nullptr);
                tm.start();
                call();
                const float ms = tm.stop();
                if (rep) best = std::min(best, ms);
            }
            return best;
        };
        for (int nbo : {512, 1024, 2048}) {
            const float ms = run([&] { gpk_potrf(DT<T>::v, K.p, n, n, 0, 1, dinv.p, info.p, nbo, nullptr); });
            printf("PERFTAIL potrf_%s n=%d plain nbo=%d  %.3f ms  %.2f TFLOP/s\n", DT<T>::name(), n, nbo, ms, (double)n * n * n / 3.0 / ms * 1e-9);
        }
        for (int nb : {512, 1024}) {
            Dev<T> dbig((size_t)((n + nb - 1) / nb) * nb * nb), ws((size_t)gpk_potrf_la_ws_elems(n, nb));
            for (int tail : {4096, 6144, 8192, 10240}) {
                if (tail >= n) continue;
                gpk_tune(9, tail);
                const float ms = run([&] { gpk_potrf_la(DT<T>::v, K.p, n, n, dinv.p, dbig.p, nb, ws.p, info.p, nullptr); });
                printf("PERFTAIL potrf_%s n=%d look-ahead nb=%d tail=%d  %.3f ms  %.2f TFLOP/s info=%d\n", DT<T>::name(), n, nb, tail, ms,
                       (double)n * n * n / 3.0 / ms * 1e-9, info.down()[0]);
            }
            gpk_tune(9, 0);
        }
        {   // 1024-column outer blocks with 512-wide explicit inverses (what fp32 runs)
            const int nb = 1024, sb = 512;
            Dev<T> dbig((size_t)((n + sb - 1) / sb) * sb * sb), ws((size_t)gpk_potrf_la_ws_elems(n, nb));
            const float ms = run([&] { gpk_potrf_la_split(DT<T>::v, K.p, n, n, dinv.p, dbig.p, nb, sb, ws.p, info.p, nullptr); });
            printf("PERFTAIL potrf_%s n=%d look-ahead nb=%d sb=%d tail=default  %.3f ms  %.2f TFLOP/s info=%d\n", DT<T>::name(), n, nb, sb, ms,
                   (double)n * n * n / 3.0 / ms * 1e-9, info.down()[0]);
        }
    }
}

// one look-ahead factorisation on an explicit stream, for rocprofv3 traces:  --la-one f64|f32 N NB MODE MINROWS
template <typename T>
static void la_one(int n, int nb, int mode, int64_t minrows, int reps, int ldpad = 0) {
    const int64_t ld = n + ldpad;
    const int d = 8;
    auto hx = randv<T>((size_t)n * d);
    Dev<T> X(hx.size()), K((size_t)n * ld), dinv(gpk_dinv_elems(n));
    Dev<T> dbig((size_t)((n + nb - 1) / nb) * nb * nb), ws((size_t)gpk_potrf_la_ws_elems(n, nb));
    Dev<int> info(1);
    X.up(hx);
    int kind = GPK_K_EQ; double var = 1.0, il = 1.0;
    hipStream_t st;
    HIPCHK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    hipEvent_t a, b;
    hipEventCreate(&a); hipEventCreate(&b);
    gpk_tune(7, mode); gpk_tune(6, minrows);
    for (int rep = 0; rep < reps; ++rep) {
        HIPCHK(hipMemsetAsync(info.p, 0, sizeof(int), st));
        gpk_kmat(DT<T>::v, &kind, &var, &il, nullptr, 1, X.p, n, d, 0, X.p, n, d, 0, d, K.p, ld, 0, 1, 1, 1, 0.1, nullptr, 0, 0, st);
        hipEventRecord(a, st);
        if (mode >= 0) gpk_potrf_la(DT<T>::v, K.p, n, ld, dinv.p, dbig.p, nb, ws.p, info.p, st);
        else gpk_potrf(DT<T>::v, K.p, n, ld, 0, 1, dinv.p, info.p, 0, st);
        hipEventRecord(b, st);
        HIPCHK(hipStreamSynchronize(st));
        float ms; hipEventElapsedTime(&ms, a, b);
        printf("LAONE ldpad=%d potrf_%s n=%d nb=%d mode=%d minrows=%lld  %.3f ms  %.2f TFLOP/s info=%d\n", ldpad, DT<T>::name(), n, nb, mode, (long long)minrows, ms, (double)n * n * n / 3.0 / ms * 1e-9, info.down()[0]);
    }
}


// aggregated trailing updates, A/B in one process:  --perf-agg f64|f32 N NB SB ROUNDS TAIL M1 M2 ...
template <typename T>
static void perf_agg(int n, int nb, int sb, int rounds, const std::vector<int>& ms_list, int64_t tail = 0) {
    const int d = 8;
    auto hx = randv<T>((size_t)n * d);
    const int wb = sb > 0 ? sb : nb;
    Dev<T> X(hx.size()), K((size_t)n * n), dinv(gpk_dinv_elems(n));
    Dev<T> dbig((size_t)((n + wb - 1) / wb) * wb * wb), ws((size_t)gpk_potrf_la_ws_elems(n, nb));
    Dev<int> info(1);
    X.up(hx);
    int kind = GPK_K_EQ; double var = 1.0, il = 1.0;
    hipStream_t st;
    HIPCHK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    hipEvent_t a, b;
    hipEventCreate(&a); hipEventCreate(&b);
    if (tail > 0) gpk_tune(9, tail);
    std::vector<double> sum(ms_list.size(), 0.0), best(ms_list.size(), 1e30);
    for (int r = 0; r <= rounds; ++r)          // round 0: warm-up
        for (size_t c = 0; c < ms_list.size(); ++c) {
            gpk_tune(47, ms_list[c]);
            HIPCHK(hipMemsetAsync(info.p, 0, sizeof(int), st));
            gpk_kmat(DT<T>::v, &kind, &var, &il, nullptr, 1, X.p, n, d, 0, X.p, n, d, 0, d, K.p, n, 0, 1, 1, 1, 0.1, nullptr, 0, 0, st);
            hipEventRecord(a, st);
            if (sb > 0 && sb < nb) gpk_potrf_la_split(DT<T>::v, K.p, n, n, dinv.p, dbig.p, nb, sb, ws.p, info.p, st);
            else gpk_potrf_la(DT<T>::v, K.p, n, n, dinv.p, dbig.p, nb, ws.p, info.p, st);
            hipEventRecord(b, st);
            HIPCHK(hipStreamSynchronize(st));
            float ms; hipEventElapsedTime(&ms, a, b);
            if (r > 0) { sum[c] += ms; best[c] = std::min(best[c], (double)ms); }
            printf("PERFAGG potrf_%s n=%d nb=%d sb=%d tail=%lld m=%d round %d  %.3f ms  info=%d\n", DT<T>::name(), n, nb, wb, (long long)tail, ms_list[c], r, ms, info.down()[0]);
        }
    for (size_t c = 0; c < ms_list.size(); ++c)
        printf("PERFAGG SUMMARY potrf_%s n=%d nb=%d sb=%d tail=%lld m=%d  mean %.3f ms  best %.3f ms  (%.2f TFLOP/s)\n", DT<T>::name(), n, nb, wb, (long long)tail, ms_list[c],
               sum[c] / rounds, best[c], (double)n * n * n / 3.0 / best[c] * 1e-9);
    gpk_tune(47, 2); gpk_tune(9, 0);
}

// factorisation with rows under the matrix, timed against the factorisation alone + the separate solve:  --perf-rows f64|f32 N EXTRA NB SB ROUNDS
template <typename T>
static void perf_rows(int n, int extra, int nb, int sb, int rounds) {
    const int d = 8;
    const int64_t rows = (int64_t)n + extra;
    auto hx = randv<T>((size_t)n * d);
    const int wb = sb > 0 ? sb : nb;
    Dev<T> X(hx.size()), K((size_t)rows * n), dinv((size_t)gpk_dinv_elems(n) + 128 * 128), E((size_t)extra * n);
    Dev<T> dbig((size_t)((n + wb - 1) / wb) * wb * wb), ws((size_t)gpk_potrf_la_ws_elems(rows, nb));
    Dev<int> info(1);
    X.up(hx);
    E.up(randv<T>((size_t)extra * n, 0.01));
    int kind = GPK_K_EQ; double var = 1.0, il = 1.0;
    hipStream_t st;
    HIPCHK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    hipEvent_t a, b;
    hipEventCreate(&a); hipEventCreate(&b);
    for (int r = 0; r <= rounds; ++r)
        for (int with_rows = 0; with_rows < 2; ++with_rows) {
            HIPCHK(hipMemsetAsync(info.p, 0, sizeof(int), st));
            gpk_kmat(DT<T>::v, &kind, &var, &il, nullptr, 1, X.p, n, d, 0, X.p, n, d, 0, d, K.p, n, 0, 1, 1, 1, 0.1, nullptr, 0, 0, st);
            HIPCHK(hipMemcpyAsync(K.p + (size_t)n * n, E.p, sizeof(T) * (size_t)extra * n, hipMemcpyDeviceToDevice, st));
            hipEventRecord(a, st);
            gpk_potrf_rows(DT<T>::v, K.p, n, with_rows ? rows : n, n, dinv.p, dbig.p, nb, (sb > 0 && sb < nb) ? sb : 0, ws.p, info.p, st);
            hipEventRecord(b, st);
            HIPCHK(hipStreamSynchronize(st));
            float ms; hipEventElapsedTime(&ms, a, b);
            if (r > 0) printf("PERFROWS potrf_%s n=%d +%d rows nb=%d sb=%d %s round %d  %.3f ms  info=%d\n", DT<T>::name(), n, extra, nb, wb,
                              with_rows ? "with the rows " : "matrix alone  ", r, ms, info.down()[0]);
        }
}

// shader clock and k-loop pace of chosen trailing updates INSIDE a look-ahead factorisation:  --la-clock f64|f32 N NB
template <typename T>
static void la_clock(int n, int nb, int warm = 0) {
    const int d = 8, grid = 512;
    // `warm` big updates enqueued right before every factorisation (no idle in between): what does the load history do to the clock?
    Dev<T> WP(warm ? (size_t)15360 * 1024 : 1), WC(warm ? (size_t)15360 * 15360 : 1);
    Dev<unsigned> wctrl(64);
    if (warm) { WP.up(randv<T>((size_t)15360 * 1024, 0.01)); WC.zero(); }
    hipEvent_t ea, eb;
    hipEventCreate(&ea); hipEventCreate(&eb);
    auto hx = randv<T>((size_t)n * d);
    Dev<T> X(hx.size()), K((size_t)n * n), dinv(gpk_dinv_elems(n));
    Dev<T> dbig((size_t)((n + nb - 1) / nb) * nb * nb), ws((size_t)gpk_potrf_la_ws_elems(n, nb));
    Dev<int> info(1);
    Dev<long long> prof((size_t)grid * 8 * 8);
    X.up(hx);
    int kind = GPK_K_EQ; double var = 1.0, il = 1.0;
    hipStream_t st;
    HIPCHK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    const int kchunks = nb / (int)(128 / sizeof(T));
    for (int which = -2; which < 10; ++which) {      // two warm-up factorisations, then one per stamped update
        HIPCHK(hipMemsetAsync(info.p, 0, sizeof(int), st));
        gpk_kmat(DT<T>::v, &kind, &var, &il, nullptr, 1, X.p, n, d, 0, X.p, n, d, 0, d, K.p, n, 0, 1, 1, 1, 0.1, nullptr, 0, 0, st);
        if (which >= 0) { prof.zero(); }
        for (int w = 0; w < warm; ++w) {
            gpk_update_t u{15360, 15360, 1024, WP.p, 1024, WP.p, 1024, WC.p, 15360, WC.p, 15360, 1};
            gpk_gemm_update2(DT<T>::v, &u, 1, -1.0, wctrl.p, 0, st);
        }
        if (which >= 0) { gpk_tune(20, which); gpk_tune_tile_prof(prof.p); }
        hipEventRecord(ea, st);
        gpk_potrf_la(DT<T>::v, K.p, n, n, dinv.p, dbig.p, nb, ws.p, info.p, st);
        hipEventRecord(eb, st);
        HIPCHK(hipStreamSynchronize(st));
        gpk_tune_tile_prof(nullptr);
        float pms = 0; hipEventElapsedTime(&pms, ea, eb);
        printf("LACLOCK potrf %.3f ms (%d updates enqueued right before it)\n", pms, warm);
        if (which < 0) continue;
        auto h = prof.down();
        for (int ti = 1; ti < 8; ti += 3) {
            double b = 0, cyc = 0; int cnt = 0;
            for (int w = 0; w < grid; ++w) {
                const long long* q = &h[((size_t)w * 8 + ti) * 8];
                if (q[3] == 0) continue;
                b += (q[2] - q[1]) * 0.01; cyc += (double)(q[5] - q[4]); ++cnt;
            }
            if (cnt) printf("LACLOCK %s n=%d update #%d, tile #%d of a workgroup (%d workgroups): k loop %.1f us = %.3f us per chunk = %.0f cycles per chunk at %.0f MHz\n",
                            DT<T>::name(), n, which, ti, cnt, b / cnt, b / cnt / kchunks, cyc / cnt / kchunks, cyc / b);
        }
    }
    gpk_tune(20, -1);
}

// kernel-matrix kernel alone, the shapes of the four GPU configs:  --perf-kmat
template <typename T>
static void perf_kmat_case(const char* nm, int nterms, const int* kinds, int64_t n, int64_t m, int d, int batch, int lower, int ldpad = 0, const double* shapes = nullptr) {
    const bool sym = (m == 0);
    if (sym) m = n;
    const int64_t ldk = m + ldpad;
    auto hx = randv<T>((size_t)batch * n * d);
    Dev<T> X(hx.size()), Y(sym ? 1 : (size_t)m * d), K((size_t)batch * n * ldk);
    X.up(hx);
    if (!sym) Y.up(randv<T>((size_t)m * d));
    double var[2] = {1.0, 1.0}, il[2] = {1.0, 1.0};
    Timer tm;
    for (int band = 1; band >= 0; --band) {
        gpk_tune(12, band);
        float best = 1e30f;
        for (int rep = 0; rep < 4; ++rep) {
            tm.start();
            gpk_kmat(DT<T>::v, kinds, var, il, shapes, nterms, X.p, n, d, n * d, sym ? X.p : Y.p, m, d, sym ? n * d : 0, d, K.p, ldk, n * ldk, batch, lower, sym ? 1 : 0, 0.1, nullptr, 0, 0, nullptr);
            const float ms = tm.stop();
            if (rep) best = std::min(best, ms);
        }
        const double bytes = (lower ? 0.5 : 1.0) * batch * (double)n * m * sizeof(T);
        printf("PERFKMAT %-28s %s %s  %.3f ms  %.2f TB/s (%s bytes)\n", nm, DT<T>::name(), band ? "row-band kernel" : "tile kernel    ", best, bytes / best * 1e-9, lower ? "lower" : "all");
    }
    gpk_tune(12, 1);
}
static void perf_kmat() {
    const int eq[1] = {GPK_K_EQ}, eql[2] = {GPK_K_EQ, GPK_K_LINEAR}, m52[1] = {GPK_K_MATERN52};
    perf_kmat_case<double>("cfg2 N=16384 D=8 EQ lower", 1, eq, 16384, 0, 8, 1, 1);
    perf_kmat_case<double>("cfg2, ld = N + 16", 1, eq, 16384, 0, 8, 1, 1, 16);
    perf_kmat_case<double>("cfg2, ld = N + 80", 1, eq, 16384, 0, 8, 1, 1, 80);
    perf_kmat_case<double>("cfg2 full matrix", 1, eq, 16384, 0, 8, 1, 0);
    perf_kmat_case<double>("N=16000 D=8 EQ lower", 1, eq, 16000, 0, 8, 1, 1);
    perf_kmat_case<float>("N=16384 D=8 EQ lower", 1, eq, 16384, 0, 8, 1, 1);
    perf_kmat_case<float>("cfg3 N=32768 D=4 EQ+Lin lower", 2, eql, 32768, 0, 4, 1, 1);
    perf_kmat_case<float>("cfg4 512xN=2048 D=3 EQ lower", 1, eq, 2048, 0, 3, 512, 1);
    perf_kmat_case<float>("cfg5 4096x200000 D=8 EQ", 1, eq, 4096, 200000, 8, 1, 0);
    const int m32[1] = {GPK_K_MATERN32}, m12[1] = {GPK_K_MATERN12};
    perf_kmat_case<double>("N=16384 D=8 Matern52 lower", 1, m52, 16384, 0, 8, 1, 1);
    perf_kmat_case<double>("N=16384 D=8 Matern32 lower", 1, m32, 16384, 0, 8, 1, 1);
    perf_kmat_case<double>("N=16384 D=8 Matern12 lower", 1, m12, 16384, 0, 8, 1, 1);
    perf_kmat_case<double>("N=16384 D=3 Matern52 lower", 1, m52, 16384, 0, 3, 1, 1);
    perf_kmat_case<float>("N=32768 D=4 Matern52 lower", 1, m52, 32768, 0, 4, 1, 1);
    perf_kmat_case<float>("N=16384x2048 D=8 EQ (K_x*)", 1, eq, 16384, 2048, 8, 1, 0);
    // the rational quadratic next to Matern-5/2 (closest instruction mix: one transcendental more than EQ)
    const int rq[1] = {GPK_K_RQ};
    const double rqa[1] = {1.5};
    perf_kmat_case<double>("N=16384 D=8 RQ lower", 1, rq, 16384, 0, 8, 1, 1, 0, rqa);
    perf_kmat_case<float>("N=16384 D=8 RQ lower", 1, rq, 16384, 0, 8, 1, 1, 0, rqa);
    perf_kmat_case<float>("N=16384 D=8 Matern52 lower", 1, m52, 16384, 0, 8, 1, 1);
    // noise as a process: EQ + v * Delta takes the term table of the launches with shapes; EQ with diag_add (the cases above) is its rival
    const int eqd[2] = {GPK_K_EQ, GPK_K_DELTA};
    const double eqds[2] = {0.0, 1e-6};
    perf_kmat_case<double>("N=16384 D=8 EQ+Delta lower", 2, eqd, 16384, 0, 8, 1, 1, 0, eqds);
    perf_kmat_case<float>("N=16384 D=8 EQ+Delta lower", 2, eqd, 16384, 0, 8, 1, 1, 0, eqds);
}

// the mixed-derivative launch beside the plain kernel-matrix launch of the same shape (both write the same bytes)   --perf-diff
template <typename T>
static void perf_diff_case(int64_t n, int d, int lower) {
    auto hx = randv<T>((size_t)n * d);
    Dev<T> X(hx.size()), K((size_t)n * n);
    X.up(hx);
    int kind = GPK_K_EQ; double var = 1.0, il = 1.0;
    Timer tm;
    for (int which = 0; which < 2; ++which) {
        float best = 1e30f;
        for (int rep = 0; rep < 5; ++rep) {
            tm.start();
            if (which) gpk_kmat_diff(DT<T>::v, &kind, &var, &il, nullptr, 1, 0, 0, X.p, n, d, 0, X.p, n, d, 0, d, K.p, n, 0, 1, lower, 1, 0.1, nullptr, 0, 0, nullptr);
            else gpk_kmat(DT<T>::v, &kind, &var, &il, nullptr, 1, X.p, n, d, 0, X.p, n, d, 0, d, K.p, n, 0, 1, lower, 1, 0.1, nullptr, 0, 0, nullptr);
            const float ms = tm.stop();
            if (rep) best = std::min(best, ms);
        }
        const double bytes = (lower ? 0.5 : 1.0) * (double)n * n * sizeof(T);
        printf("PERFDIFF N=%lld D=%d EQ %s %s %-34s %.3f ms  %.2f TB/s\n", (long long)n, d, lower ? "lower" : "full ", DT<T>::name(),
               which ? "gpk_kmat_diff d2/dx0 dy0" : "gpk_kmat (compile-time EQ program)", best, bytes / best * 1e-9);
    }
}

// one problem, for rocprofv3: kmat + potrf (+ trsv, merge, trsm) at order n
template <typename T>
static void profile_one(int n, int nbo, int reps) {
    const int d = 8, nrhs = 2048, sb = 512;
    auto hx = randv<T>((size_t)n * d);
    Dev<T> X(hx.size()), K((size_t)n * n), dinv(gpk_dinv_elems(n)), y(n), tmp((size_t)sb * nrhs + GPK_TRSV_CTRL_ELEMS);
    Dev<T> dsb((size_t)((n + sb - 1) / sb) * sb * sb), tmpm((size_t)((n + sb - 1) / sb) * sb * sb / 4 + 16), Bm((size_t)n * nrhs);
    Dev<int> info(1);
    X.up(hx);
    y.up(randv<T>(n));
    Bm.up(randv<T>((size_t)n * nrhs));
    int kind = GPK_K_EQ; double var = 1.0, il = 1.0;
    Timer tm;
    for (int rep = 0; rep < reps; ++rep) {
        info.zero();
        gpk_kmat(DT<T>::v, &kind, &var, &il, nullptr, 1, X.p, n, d, 0, X.p, n, d, 0, d, K.p, n, 0, 1, 1, 1, 0.1, nullptr, 0, 0, nullptr);
        tm.start();
        gpk_potrf(DT<T>::v, K.p, n, n, 0, 1, dinv.p, info.p, nbo, nullptr);
        const float ms = tm.stop();
        printf("PROFILE potrf_%s n=%d nbo=%d %.3f ms %.2f TFLOP/s\n", DT<T>::name(), n, nbo, ms, (double)n * n * n / 3.0 / ms * 1e-9);
        gpk_trsv_lower(DT<T>::v, K.p, n, n, 0, dinv.p, 128, y.p, 1, 1, 0, tmp.p, 1, nullptr);
        gpk_trtri_merge(DT<T>::v, K.p, n, n, 0, 1, dinv.p, sb, dsb.p, tmpm.p, nullptr);
        gpk_trsm_lower(DT<T>::v, K.p, n, n, 0, dsb.p, sb, Bm.p, nrhs, nrhs, 0, tmp.p, 1, nullptr);
        HIPCHK(hipDeviceSynchronize());
    }
}

// one GEMM shape, timed alone:  --gemm f64|f32 M N K [lower]   (k-major operands, C = C - A B^T)
template <typename T>
static void gemm_one(int M, int N, int K, int flags, int reps, int64_t lda = -1) {
    if (lda < 0) lda = K;
    Dev<T> A((size_t)M * K), B((size_t)N * K), C((size_t)M * N);
    A.up(randv<T>((size_t)M * K, 0.01)); B.up(randv<T>((size_t)N * K, 0.01)); C.zero();
    Timer tm;
    for (int rep = 0; rep < reps; ++rep) {
        tm.start();
        // flags: 1/2/4/8 as in gpk.h, 32: beta = 0, 64: B stored K x N (n contiguous)
        gpk_gemm(DT<T>::v, 1, (flags & 64) ? 0 : 1, M, N, K, -1.0, A.p, lda, 0, B.p, (flags & 64) ? N : K, 0, (flags & 32) ? 0.0 : 1.0, C.p, N, 0, 1, flags & 15, nullptr);
        const float ms = tm.stop();
        const double fl = ((flags & 13) ? 1.0 : 2.0) * M * (double)N * K;
        printf("GEMM %s M=%d N=%d K=%d flags=%d lda=%lld  %.3f ms  %.2f TFLOP/s\n", DT<T>::name(), M, N, K, flags, (long long)lda, ms, fl / ms * 1e-9);
    }
}

__global__ void rsq_probe(const double* x, double* y, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] = __builtin_amdgcn_rsq(x[i]);
}
static void rsq_precision() {
    const int n = 1 << 16;
    std::vector<double> x(n);
    std::uniform_real_distribution<double> u(0.01, 100.0);
    for (auto& v : x) v = u(rng);
    Dev<double> dx(n), dy(n);
    dx.up(x);
    hipLaunchKernelGGL(rsq_probe, dim3(n / 256), dim3(256), 0, 0, dx.p, dy.p, n);
    HIPCHK(hipDeviceSynchronize());
    auto y = dy.down();
    double worst = 0;
    for (int i = 0; i < n; ++i) worst = std::max(worst, std::fabs(y[i] * std::sqrt(x[i]) - 1.0));
    printf("RSQ_F64 max relative error of v_rsq_f64: %.3e (= 2^%.1f)\n", worst, std::log2(worst));
}


// pure-register MFMA ceiling: every wave runs `iters` x 16 independent v_mfma (no memory)
__global__ __launch_bounds__(256) void mfma_peak64(double* out, int iters, long long* clk) {
    d4 acc[16];
    for (int i = 0; i < 16; ++i) acc[i] = d4{0, 0, 0, 0};
    double a = threadIdx.x * 1e-3, b = 1.0 + threadIdx.x * 1e-4;
    const long long c0 = __builtin_readcyclecounter(), w0 = wall_clock64();
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int i = 0; i < 16; ++i) asm volatile("v_mfma_f64_16x16x4_f64 %0, %1, %2, %0" : "+v"(acc[i]) : "v"(a), "v"(b));
    }
    asm volatile("s_nop 15\n\ts_nop 15\n\ts_nop 15" ::: "memory");
    const long long c1 = __builtin_readcyclecounter(), w1 = wall_clock64();
    double s = 0;
    for (int i = 0; i < 16; ++i) s += acc[i][0] + acc[i][1] + acc[i][2] + acc[i][3];
    out[blockIdx.x * 256 + threadIdx.x] = s;
    if (threadIdx.x == 0 && blockIdx.x == 0) { clk[0] = c1 - c0; clk[1] = w1 - w0; }
}
__global__ __launch_bounds__(256) void mfma_peak32(float* out, int iters, long long* clk) {
    f4 acc[16];
    for (int i = 0; i < 16; ++i) acc[i] = f4{0, 0, 0, 0};
    float a = threadIdx.x * 1e-3f, b = 1.0f + threadIdx.x * 1e-4f;
    const long long c0 = __builtin_readcyclecounter(), w0 = wall_clock64();
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int i = 0; i < 16; ++i) asm volatile("v_mfma_f32_16x16x4_f32 %0, %1, %2, %0" : "+v"(acc[i]) : "v"(a), "v"(b));
    }
    asm volatile("s_nop 15\n\ts_nop 15\n\ts_nop 15" ::: "memory");
    const long long c1 = __builtin_readcyclecounter(), w1 = wall_clock64();
    float s = 0;
    for (int i = 0; i < 16; ++i) s += acc[i][0] + acc[i][1] + acc[i][2] + acc[i][3];
    out[blockIdx.x * 256 + threadIdx.x] = s;
    if (threadIdx.x == 0 && blockIdx.x == 0) { clk[0] = c1 - c0; clk[1] = w1 - w0; }
}
static void mfma_peak() {
    Timer tm;
    Dev<double> o64((size_t)512 * 256);
    Dev<float> o32((size_t)512 * 256);
    Dev<long long> clk(2);
    int wallrate = 0;
    hipDeviceGetAttribute(&wallrate, hipDeviceAttributeWallClockRate, 0);
    for (int blocks : {256, 512}) {
        for (int rep = 0; rep < 2; ++rep) {
            const int iters = 4000;
            tm.start();
            hipLaunchKernelGGL(mfma_peak64, dim3(blocks), dim3(256), 0, 0, o64.p, iters, clk.p);
            float ms = tm.stop();
            auto c = clk.down();
            double tf = (double)blocks * 4 * iters * 16 * 2048.0 / ms * 1e-9;
            if (rep) printf("MFMAPEAK f64 blocks=%d: %.3f ms  %.2f TFLOP/s  cycles=%lld wall_ticks=%lld (wall clock %d kHz) -> shader clock %.0f MHz, %.1f cycles/MFMA/SIMD\n", blocks, ms, tf,
                            c[0], c[1], wallrate, (double)c[0] / ((double)c[1] / wallrate) * 1e-3, (double)c[0] / (iters * 16.0 * (blocks / 256)));
            tm.start();
            hipLaunchKernelGGL(mfma_peak32, dim3(blocks), dim3(256), 0, 0, o32.p, iters, clk.p);
            ms = tm.stop();
            c = clk.down();
            tf = (double)blocks * 4 * iters * 16 * 2048.0 / ms * 1e-9;
            if (rep) printf("MFMAPEAK f32 blocks=%d: %.3f ms  %.2f TFLOP/s  shader clock %.0f MHz\n", blocks, ms, tf, (double)c[0] / ((double)c[1] / wallrate) * 1e-3);
        }
    }
}

template <int BYTES>
__global__ __launch_bounds__(256) void lds_hog(double* out, int iters) {
    __shared__ double buf[BYTES / 8];
    for (int i = threadIdx.x; i < BYTES / 8; i += 256) buf[i] = i;
    __syncthreads();
    double acc = 0;
    for (int it = 0; it < iters; ++it) acc += buf[(threadIdx.x * 17 + it * 31) % (BYTES / 8)];
    out[threadIdx.x] = acc;
}


// ---------------------------------------------------------------------------
// experiment: where and when does the dispatcher place a one-workgroup kernel of a second stream while a
// resident grid holds every CU but a few?   --dispatch
// ---------------------------------------------------------------------------
struct HogArgs { unsigned keys[8]; unsigned* ctrl; long long* t_start; long long spin_ticks; int mode; };   // mode 0: stay, 1: first arrival per XCC leaves, 2: static keys leave
__global__ __launch_bounds__(256, 2) void hog_kernel(HogArgs p) {
    __shared__ char pad[72 * 1024];
    __shared__ int leave;
    if (threadIdx.x == 0) {
        unsigned xcc, hw;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
        xcc &= 7u;
        const unsigned key = ((hw >> 8) & 0xffu) + 1u;
        int lv = 0;
        if (p.mode == 1) { const unsigned old = atomicCAS(&p.ctrl[1 + xcc], 0u, key); lv = (old == 0u || old == key); }
        if (p.mode == 2) lv = (p.keys[xcc] == key);
        if (lv) atomicAdd(&p.ctrl[9 + xcc], 1u);
        if (blockIdx.x == 0) *p.t_start = wall_clock64();
        leave = lv;
        pad[threadIdx.x] = (char)lv;
    }
    __syncthreads();
    if (leave) return;
    const long long t0 = wall_clock64();
    while (wall_clock64() - t0 < p.spin_ticks) {}
    if (pad[1] == 77) p.ctrl[31] = 1;
}
__global__ __launch_bounds__(256, 1) void probe_kernel(unsigned long long* out, int idx) {
    extern __shared__ char big[];
    if (threadIdx.x == 0) {
        unsigned xcc, hw;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
        out[2 * (idx * gridDim.x + blockIdx.x)] = ((unsigned long long)(xcc & 7u) << 32) | ((hw >> 8) & 0xffu);
        out[2 * (idx * gridDim.x + blockIdx.x) + 1] = (unsigned long long)wall_clock64();
        big[0] = 1;
    }
    const long long t0 = wall_clock64();
    while (wall_clock64() - t0 < 2000) {}    // 20 us
}
static void masked_census(const char* nm, const uint32_t* mask) {
    hipStream_t st;
    hipError_t e = hipExtStreamCreateWithCUMask(&st, 8, mask);
    if (e != hipSuccess) { printf("MASK %s: create failed: %s\n", nm, hipGetErrorString(e)); return; }
    const int nb = 256;
    Dev<unsigned> out(2 * nb);
    hipLaunchKernelGGL(census_kernel, dim3(nb), dim3(256), 0, st, out.p);
    HIPCHK(hipStreamSynchronize(st));
    auto h = out.down();
    std::vector<int> cnt(8 * 256, 0);
    for (int b = 0; b < nb; ++b) cnt[(h[2 * b] & 7) * 256 + ((h[2 * b + 1] >> 8) & 0xff)]++;
    printf("MASK %-28s ->", nm);
    for (int x = 0; x < 8; ++x) for (int k = 0; k < 256; ++k) if (cnt[x * 256 + k]) printf(" x%d:%d.%d(%d)", x, (k >> 5) & 7, k & 15, cnt[x * 256 + k]);
    printf("\n");
    hipStreamDestroy(st);
}
static void dispatch_experiment() {
    HIPCHK(hipFuncSetAttribute((const void*)probe_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 134144));
    // 1. which CUs does a CU-mask bit enable?
    { uint32_t m[8] = {1, 0, 0, 0, 0, 0, 0, 0}; masked_census("bit 0", m); }
    { uint32_t m[8] = {2, 0, 0, 0, 0, 0, 0, 0}; masked_census("bit 1", m); }
    { uint32_t m[8] = {0x100, 0, 0, 0, 0, 0, 0, 0}; masked_census("bit 8", m); }
    { uint32_t m[8] = {0, 1, 0, 0, 0, 0, 0, 0}; masked_census("bit 32", m); }
    { uint32_t m[8] = {0xff, 0, 0, 0, 0, 0, 0, 0}; masked_census("bits 0..7", m); }
    { uint32_t m[8] = {1, 1, 1, 1, 1, 1, 1, 1}; masked_census("bit 0 of every word", m); }
    { uint32_t m[8] = {0x01010101, 0x01010101, 0, 0, 0, 0, 0, 0}; masked_census("bits 0,8,..,56", m); }
    { uint32_t m[8] = {0x11111111, 0, 0, 0, 0, 0, 0, 0}; masked_census("bits 0,4,..,28", m); }
    // 2. probes beside a resident grid
    hipStream_t s_main, s_aux, s_mask;
    HIPCHK(hipStreamCreateWithFlags(&s_main, hipStreamNonBlocking));
    HIPCHK(hipStreamCreateWithFlags(&s_aux, hipStreamNonBlocking));
    uint32_t mk[8] = {0xff, 0, 0, 0, 0, 0, 0, 0};
    const bool have_mask = hipExtStreamCreateWithCUMask(&s_mask, 8, mk) == hipSuccess;
    // keys the masked stream can reach
    unsigned keys[8] = {0};
    if (have_mask) {
        Dev<unsigned> out(2 * 256);
        hipLaunchKernelGGL(census_kernel, dim3(256), dim3(256), 0, s_mask, out.p);
        HIPCHK(hipStreamSynchronize(s_mask));
        auto h = out.down();
        for (int b = 0; b < 256; ++b) keys[h[2 * b] & 7] = ((h[2 * b + 1] >> 8) & 0xff) + 1;
        printf("DISPATCH masked stream keys:");
        for (int x = 0; x < 8; ++x) printf(" x%d:%d.%d", x, ((keys[x] - 1) >> 5) & 7, (keys[x] - 1) & 15);
        printf("\n");
    }
    Dev<unsigned> ctrl(64);
    Dev<long long> tstart(1);
    const int nprobe = 12;
    for (int cfg = 0; cfg < 6; ++cfg) {
        // cfg 0: hog stays everywhere, probes unmasked; 1: first-arrival reserve, probes unmasked; 2: static keys, probes unmasked;
        // 3: static keys, probes on the masked stream; 4: static keys, 64-workgroup small probes (40 KB) unmasked; 5: the same, masked
        const int mode = cfg == 0 ? 0 : (cfg == 1 ? 1 : 2);
        hipStream_t sp = (cfg == 3 || cfg == 5) ? s_mask : s_aux;
        if ((cfg == 3 || cfg == 5) && !have_mask) continue;
        const int pgrid = cfg >= 4 ? 64 : 1;
        const size_t plds = cfg >= 4 ? 40960 : 134144;
        Dev<unsigned long long> out(2 * nprobe * pgrid);
        ctrl.zero();
        HogArgs ha;
        for (int x = 0; x < 8; ++x) ha.keys[x] = keys[x];
        ha.ctrl = ctrl.p; ha.t_start = tstart.p; ha.spin_ticks = 200000; ha.mode = mode;   // 2 ms
        HIPCHK(hipDeviceSynchronize());
        hipLaunchKernelGGL(hog_kernel, dim3(512), dim3(256), 0, s_main, ha);
        for (int i = 0; i < nprobe; ++i) hipLaunchKernelGGL(probe_kernel, dim3(pgrid), dim3(256), plds, sp, out.p, i);
        HIPCHK(hipDeviceSynchronize());
        auto h = out.down();
        auto c = ctrl.down();
        const long long t0 = tstart.down()[0];
        int left = 0; for (int x = 0; x < 8; ++x) left += c[9 + x];
        printf("DISPATCH cfg %d (hog mode %d, %d workgroups left; probes: grid %d, %zu B LDS, %s stream):", cfg, mode, left, pgrid, plds, (sp == s_mask) ? "masked" : "plain");
        for (int i = 0; i < nprobe; ++i) {
            long long tmin = (long long)h[2 * (i * pgrid) + 1], tmax = tmin;
            for (int b = 0; b < pgrid; ++b) { tmin = std::min(tmin, (long long)h[2 * (i * pgrid + b) + 1]); tmax = std::max(tmax, (long long)h[2 * (i * pgrid + b) + 1]); }
            const unsigned long long loc = h[2 * (i * pgrid)];
            printf(" [%lld..%lld us @x%llu:%llu.%llu]", (tmin - t0) / 100, (tmax - t0) / 100, loc >> 32, ((loc & 0xff) >> 5) & 7, loc & 15);
        }
        printf("\n");
    }
}


// where does a tile of the persistent trailing update spend its time?   --tileprof
static void tile_profile(int k = 1024, int lower = 1, int warm = 0) {
    const int n = 15360, grid = 512;
    Dev<double> P((size_t)n * k), C((size_t)n * n);
    Dev<unsigned> ctrl(64);
    Dev<long long> prof((size_t)grid * 8 * 8);
    P.up(randv<double>((size_t)n * k, 0.01)); C.zero();
    Timer tm;
    for (int rep = 0; rep < 2; ++rep) {
        prof.zero();
        gpk_update_t u{n, n, k, P.p, k, P.p, k, C.p, n, C.p, n, lower};
        // `warm` launches of the same update enqueued right before the measured one: the chip is busy (and clocked up) when it starts
        for (int w = 0; rep && w < warm; ++w) gpk_gemm_update2(GPK_F64, &u, 1, -1.0, ctrl.p, 0, nullptr);
        gpk_tune_tile_prof(rep ? prof.p : nullptr);
        tm.start();
        gpk_gemm_update2(GPK_F64, &u, 1, -1.0, ctrl.p, 0, nullptr);
        const float ms = tm.stop();
        printf("TILEPROF update 15360^2 %s k=%d %s, %d launches right before it: %.3f ms  %.1f TFLOP/s\n", lower ? "lower" : "full", k, rep ? "with stamps" : "plain (first launch)",
               rep ? warm : 0, ms, (lower ? 1.0 : 2.0) * n * (double)n * k / ms * 1e-9);
    }
    gpk_tune_tile_prof(nullptr);
    auto h = prof.down();
    for (int ti = 0; ti < 8; ++ti) {
        double a = 0, b = 0, c = 0, gap = 0, cyc = 0, arr = 0; int cnt = 0, cg = 0;
        for (int w = 0; w < grid; ++w) {
            const long long* q = &h[((size_t)w * 8 + ti) * 8];
            if (q[3] == 0) continue;
            a += (q[1] - q[0]) * 0.01; b += (q[2] - q[1]) * 0.01; c += (q[3] - q[2]) * 0.01; cyc += (double)(q[5] - q[4]); ++cnt;
            if (q[6]) arr += (q[6] - q[1]) * 0.01;
            if (ti > 0) { const long long* pq = &h[((size_t)w * 8 + ti - 1) * 8]; gap += (q[0] - pq[3]) * 0.01; ++cg; }
        }
        if (cnt) printf("TILEPROF tile #%d of a workgroup (%d workgroups): request C %.1f us | k loop (incl. C arrival, first chunk) %.1f us = %.3f us per chunk at %.0f MHz shader clock, of it C + first chunk arrived after %.1f us | stores retired %.1f us | gap to previous tile %.1f us\n",
                        ti, cnt, a / cnt, b / cnt, b / cnt / (k / 16), cyc / b, arr / cnt, c / cnt, cg ? gap / cg : 0.0);
    }
    // start-time spread of the first tiles and of the last stamps
    long long t0 = LLONG_MAX, t1 = 0, e0 = LLONG_MAX, e1 = 0;
    for (int w = 0; w < grid; ++w) { const long long* q = &h[(size_t)w * 8 * 8]; if (q[3]) { t0 = std::min(t0, q[0]); t1 = std::max(t1, q[0]); } }
    printf("TILEPROF first tiles start within %.1f us of each other\n", (t1 - t0) * 0.01);
}

// experiment: CU-masked streams (does a reserved CU let a small kernel overlap a big GEMM?)
static void cumask_experiment() {
    const int n = 8192;
    Dev<double> A((size_t)n * n), Bm((size_t)n * n), C((size_t)n * n), D((size_t)2048 * 2048), dinv(gpk_dinv_elems(2048));
    Dev<int> info(1);
    auto h = randv<double>((size_t)n * n);
    A.up(h); Bm.up(h); C.zero();
    auto spd = make_spd<double>(2048, 1, 2048);
    hipStream_t s_def, s_m8, s_half, s_small;
    HIPCHK(hipStreamCreate(&s_def));
    HIPCHK(hipStreamCreate(&s_small));
    uint32_t m8[8], mh[8];
    for (int i = 0; i < 8; ++i) { m8[i] = 0xFFFFFFFFu; mh[i] = 0x0000FFFFu; }
    m8[0] = 0xFFFFFF00u;   // bits 0..7: one CU per XCC if bit i <-> XCC i % 8
    hipError_t e1 = hipExtStreamCreateWithCUMask(&s_m8, 8, m8), e2 = hipExtStreamCreateWithCUMask(&s_half, 8, mh);
    printf("CUMASK create: %s %s\n", hipGetErrorString(e1), hipGetErrorString(e2));
    hipEvent_t a, b;
    hipEventCreate(&a); hipEventCreate(&b);
    auto time_gemm = [&](hipStream_t st, const char* nm) {
        for (int rep = 0; rep < 2; ++rep) {
            hipEventRecord(a, st);
            gpk_gemm(GPK_F64, 1, 1, n, n, n, -1.0, A.p, n, 0, Bm.p, n, 0, 1.0, C.p, n, 0, 1, 0, st);
            hipEventRecord(b, st);
            hipEventSynchronize(b);
            float ms; hipEventElapsedTime(&ms, a, b);
            if (rep) printf("CUMASK gemm 8192^3 on %-10s %.3f ms\n", nm, ms);
        }
    };
    time_gemm(s_def, "default");
    if (e1 == hipSuccess) time_gemm(s_m8, "mask-8");
    if (e2 == hipSuccess) time_gemm(s_half, "mask-half");
    // overlap: big GEMM on X, potrf(2048) chain on s_small; wall time of both
    auto overlap = [&](hipStream_t big, const char* nm) {
        for (int rep = 0; rep < 2; ++rep) {
            D.up(spd); info.zero();
            HIPCHK(hipDeviceSynchronize());
            auto t0 = std::chrono::high_resolution_clock::now();
            gpk_gemm(GPK_F64, 1, 1, n, n, n, -1.0, A.p, n, 0, Bm.p, n, 0, 1.0, C.p, n, 0, 1, 0, big);
            gpk_potrf(GPK_F64, D.p, 2048, 2048, 0, 1, dinv.p, info.p, 0, s_small);
            hipEventRecord(b, s_small);
            hipEventSynchronize(b);
            auto t1 = std::chrono::high_resolution_clock::now();
            HIPCHK(hipDeviceSynchronize());
            auto t2 = std::chrono::high_resolution_clock::now();
            if (rep) printf("CUMASK overlap big=%-10s potrf(2048) done after %.3f ms, everything after %.3f ms\n", nm,
                            std::chrono::duration<double, std::milli>(t1 - t0).count(), std::chrono::duration<double, std::milli>(t2 - t0).count());
        }
    };
    {   // mask-layout sweep: which bits cost the least?
        struct M { const char* nm; std::vector<int> clear; };
        std::vector<M> ms = {{"clr{0}", {0}}, {"clr{0,4..28}", {0, 4, 8, 12, 16, 20, 24, 28}}, {"clr{0..7}", {0, 1, 2, 3, 4, 5, 6, 7}},
                             {"clr{0,32..224}", {0, 32, 64, 96, 128, 160, 192, 224}}, {"clr{0,1,2,3}", {0, 1, 2, 3}},
                             {"clr{0,8..56}", {0, 8, 16, 24, 32, 40, 48, 56}}, {"clr{0..31}", {0,1,2,3,4,5,6,7,8,9,10,11,12,13,14,15,16,17,18,19,20,21,22,23,24,25,26,27,28,29,30,31}}};
        for (auto& m : ms) {
            uint32_t w[8];
            for (int i = 0; i < 8; ++i) w[i] = 0xFFFFFFFFu;
            for (int bit : m.clear) w[bit / 32] &= ~(1u << (bit % 32));
            hipStream_t st;
            if (hipExtStreamCreateWithCUMask(&st, 8, w) == hipSuccess) {
                time_gemm(st, m.nm);
                hipStreamDestroy(st);
            }
        }
    }
    overlap(s_def, "default");
    if (e1 == hipSuccess) overlap(s_m8, "mask-8");
    // diag-kernel-only chain (20 x potrf of one 128 block) beside the big GEMM
    auto overlap_diag = [&](hipStream_t big, const char* nm, bool with_big) {
        for (int rep = 0; rep < 2; ++rep) {
            D.up(spd); info.zero();
            HIPCHK(hipDeviceSynchronize());
            auto t0 = std::chrono::high_resolution_clock::now();
            if (with_big) gpk_gemm(GPK_F64, 1, 1, n, n, n, -1.0, A.p, n, 0, Bm.p, n, 0, 1.0, C.p, n, 0, 1, 0, big);
            for (int q = 0; q < 20; ++q) gpk_potrf(GPK_F64, D.p + (size_t)q * 128 * 2049 * 0, 128, 2048, 0, 1, dinv.p, info.p, 0, s_small);
            hipEventRecord(b, s_small);
            hipEventSynchronize(b);
            auto t1 = std::chrono::high_resolution_clock::now();
            HIPCHK(hipDeviceSynchronize());
            auto t2 = std::chrono::high_resolution_clock::now();
            if (rep) printf("CUMASK diag-chain big=%-10s 20 diag kernels done after %.3f ms, everything after %.3f ms\n", nm,
                            std::chrono::duration<double, std::milli>(t1 - t0).count(), std::chrono::duration<double, std::milli>(t2 - t0).count());
        }
    };
    {   // can an 80 KB / 20 KB workgroup on a HIGH-PRIORITY stream get in beside the big GEMM?
        int lo, hi;
        hipDeviceGetStreamPriorityRange(&lo, &hi);
        hipStream_t s_hi;
        HIPCHK(hipStreamCreateWithPriority(&s_hi, hipStreamNonBlocking, hi));
        Dev<double> o(256);
        auto hog = [&](int kb, bool with_big, hipStream_t st, const char* nm) {
            for (int rep = 0; rep < 2; ++rep) {
                HIPCHK(hipDeviceSynchronize());
                auto t0 = std::chrono::high_resolution_clock::now();
                if (with_big) gpk_gemm(GPK_F64, 1, 1, n, n, n, -1.0, A.p, n, 0, Bm.p, n, 0, 1.0, C.p, n, 0, 1, 0, s_def);
                for (int q = 0; q < 20; ++q) {
                    if (kb == 80) hipLaunchKernelGGL(lds_hog<81920>, dim3(1), dim3(256), 0, st, o.p, 20000);
                    else if (kb == 134) hipLaunchKernelGGL(lds_hog<137216>, dim3(1), dim3(256), 0, st, o.p, 20000);
                    else hipLaunchKernelGGL(lds_hog<20480>, dim3(1), dim3(256), 0, st, o.p, 20000);
                }
                hipEventRecord(b, st);
                hipEventSynchronize(b);
                auto t1 = std::chrono::high_resolution_clock::now();
                HIPCHK(hipDeviceSynchronize());
                if (rep) printf("PRIO hog %3d KB x20 on %-8s stream, big GEMM %s: done after %.3f ms\n", kb, nm, with_big ? "yes" : "no ",
                                std::chrono::duration<double, std::milli>(t1 - t0).count());
            }
        };
        printf("PRIO priority range lo=%d hi=%d\n", lo, hi);
        for (int kb : {20, 80, 134}) {
            hog(kb, false, s_hi, "hi-prio");
            hog(kb, true, s_hi, "hi-prio");
            hog(kb, true, s_small, "normal");
        }
    }
    overlap_diag(s_def, "none", false);
    overlap_diag(s_def, "default", true);
    if (e1 == hipSuccess) overlap_diag(s_m8, "mask-8", true);
}

template <typename T>
static void diag_phase_profile(int n, int ver, int pipe = 0) {
    const int nblk = (n + 127) / 128;
    Dev<long long> prof((size_t)nblk * 32);
    prof.zero();
    (void)ver;
    gpk_tune(37, pipe);
    gpk_tune_diag_prof(prof.p);
    profile_one<T>(n, 0, 1);
    gpk_tune_diag_prof(nullptr);
    auto h = prof.down();
    for (int blk : {0, nblk / 2 + 1, nblk - 1}) {
        if (ver == 0) {
            const long long* q = &h[(size_t)blk * 16];
            printf("DIAGPROF %s blk %d cycles: load %lld  factor %lld [trsm %lld  c1 %lld  chol(wave0) %lld]  storeL %lld  invert %lld [16x16 %lld]  storeW %lld  total %lld\n",
                   DT<T>::name(), blk, q[1] - q[0], q[2] - q[1], q[8], q[9], q[10], q[3] - q[2], q[4] - q[3], q[6] - q[3], q[5] - q[4], q[5] - q[0]);
        } else {
            const long long* q = &h[(size_t)blk * 32];
            printf("DIAGPROF3 %s blk %d cycles: load %lld | panel0 %lld | steps", DT<T>::name(), blk, q[1] - q[0], q[2] - q[1]);
            for (int s = 0; s < 7; ++s) printf(" %lld", q[3 + s] - q[2 + s]);
            printf(" | last two row blocks of the inverse %lld | total %lld\n", q[12] - q[10], q[13] - q[0]);
            printf("DIAGPROF3 %s blk %d   of which column update before the panel (U1):", DT<T>::name(), blk);
            for (int s = 0; s < 7; ++s) printf(" %lld", q[21 + s] - q[2 + s]);
            printf("\n");
            if (pipe && q[29] > q[16] && q[30] > q[16])
                printf("PIPEPROF %s blk %d critical path after the inverse is out (us): strip solve starts %.2f, computed %.2f, published %.2f | last tile update starts %.2f, computed %.2f, published %.2f | chain sees the block %.2f\n",
                       DT<T>::name(), blk, (q[17] - q[16]) * 0.01, (q[18] - q[16]) * 0.01, (q[19] - q[16]) * 0.01, (q[20] - q[16]) * 0.01, (q[28] - q[16]) * 0.01,
                       (q[29] - q[16]) * 0.01, (q[30] - q[16]) * 0.01);
            if (pipe && q[15] > q[13] && blk + 1 < nblk)      // the chain workgroup of the pipelined panel
                printf("PIPEPROF %s blk %d cycles: wait for the block's tiles %lld | publish the inverse %lld | step period %lld\n",
                       DT<T>::name(), blk, q[0] - q[14], q[15] - q[13], q[32 + 14] - q[14]);
        }
    }
    gpk_tune(37, 1);
}

// --perf-pipe: the factorisation of small / chain-bound matrices with and without the pipelined panel kernel, at several outer
// block widths (nbo = n: the whole matrix is ONE pipelined panel)
template <typename T>
static void perf_pipe() {
    Timer tm;
    for (int n : {1024, 2048, 4096, 8192}) {
        const int d = 8;
        auto hx = randv<T>((size_t)n * d);
        Dev<T> X(hx.size()), K((size_t)n * n), dinv(gpk_dinv_elems(n));
        Dev<int> info(1);
        X.up(hx);
        int kind = GPK_K_EQ; double var = 1.0, il = 1.0;
        for (int pipe = 0; pipe < 2; ++pipe) {
            gpk_tune(37, pipe);
            for (int nbo : {256, 512, 1024, 2048, 4096, 8192}) {
                if (nbo > n || (!pipe && nbo > 1024)) continue;
                float best = 1e30f;
                for (int rep = 0; rep < 4; ++rep) {
                    info.zero();
                    gpk_kmat(DT<T>::v, &kind, &var, &il, nullptr, 1, X.p, n, d, 0, X.p, n, d, 0, d, K.p, n, 0, 1, 1, 1, 0.1, nullptr, 0, 0, nullptr);
                    tm.start();
                    gpk_potrf(DT<T>::v, K.p, n, n, 0, 1, dinv.p, info.p, nbo, nullptr);
                    const float ms = tm.stop();
                    if (rep && ms < best) best = ms;
                }
                printf("PERFPIPE potrf_%s n=%d nbo=%d pipe=%d  %.3f ms  %.2f TFLOP/s info=%d\n", DT<T>::name(), n, nbo, pipe, best,
                       (double)n * n * n / 3.0 / best * 1e-9, info.down()[0]);
            }
        }
        gpk_tune(37, 1);
    }
}

// --perf-trsm: the 2048-column solve of the posterior path at N = 16384 (cfg2) / 32768 fp32 (cfg3), in place and out of place
template <typename T>
static void perf_trsm(int n, int nrhs) {
    auto hx = randv<T>((size_t)n * 8);
    Dev<T> X(hx.size()), K((size_t)n * n), dinv(gpk_dinv_elems(n)), Bm((size_t)n * nrhs), Xo((size_t)n * nrhs);
    Dev<int> info(1);
    X.up(hx);
    int kind = GPK_K_EQ; double var = 1.0, il = 1.0;
    info.zero();
    gpk_kmat(DT<T>::v, &kind, &var, &il, nullptr, 1, X.p, n, 8, 0, X.p, n, 8, 0, 8, K.p, n, 0, 1, 1, 1, 0.1, nullptr, 0, 0, nullptr);
    gpk_potrf(DT<T>::v, K.p, n, n, 0, 1, dinv.p, info.p, 0, nullptr);
    auto hb = randv<T>((size_t)n * nrhs);
    Timer tm;
    for (int sb : {512, 1024, 2048}) {
        Dev<T> dsb((size_t)((n + sb - 1) / sb) * sb * sb), tmpm((size_t)((n + sb - 1) / sb) * sb * sb / 4 + 16), tmp((size_t)sb * nrhs);
        gpk_trtri_merge(DT<T>::v, K.p, n, n, 0, 1, dinv.p, sb, dsb.p, tmpm.p, nullptr);
        for (int oop = 0; oop < 2; ++oop)
            for (int rep = 0; rep < 3; ++rep) {
                Bm.up(hb);
                tm.start();
                if (oop) gpk_trsm_lower_to(DT<T>::v, K.p, n, n, 0, dsb.p, sb, Bm.p, nrhs, nrhs, 0, Xo.p, nrhs, 0, 1, nullptr);
                else gpk_trsm_lower(DT<T>::v, K.p, n, n, 0, dsb.p, sb, Bm.p, nrhs, nrhs, 0, tmp.p, 1, nullptr);
                const float ms = tm.stop();
                if (rep) printf("PERFTRSM %s n=%d nrhs=%d sb=%d %s  %.3f ms  %.2f TFLOP/s\n", DT<T>::name(), n, nrhs, sb, oop ? "out-of-place" : "in-place    ", ms,
                                (double)n * n * nrhs / ms * 1e-9);
            }
    }
}

// one right-hand side: the per-block sweep (2 n / sb launches) against the single resident launch   --perf-trsv
template <typename T>
static void perf_trsv(int n, std::vector<int> sbs) {
    auto hx = randv<T>((size_t)n * 8);
    Dev<T> X(hx.size()), K((size_t)n * n), dinv(gpk_dinv_elems(n)), y(n);
    Dev<int> info(1);
    X.up(hx);
    int kind = GPK_K_EQ; double var = 1.0, il = 1.0;
    info.zero();
    gpk_kmat(DT<T>::v, &kind, &var, &il, nullptr, 1, X.p, n, 8, 0, X.p, n, 8, 0, 8, K.p, n, 0, 1, 1, 1, 0.1, nullptr, 0, 0, nullptr);
    gpk_potrf(DT<T>::v, K.p, n, n, 0, 1, dinv.p, info.p, 0, nullptr);
    auto hy = randv<T>((size_t)n);
    Timer tm;
    for (int sb : sbs) {
        Dev<T> dsb((size_t)((n + sb - 1) / sb) * sb * sb), tmpm((size_t)((n + sb - 1) / sb) * sb * sb / 4 + 16), tmp((size_t)sb + GPK_TRSV_CTRL_ELEMS);
        gpk_trtri_merge(DT<T>::v, K.p, n, n, 0, 1, dinv.p, sb, dsb.p, tmpm.p, nullptr);
        for (int rep = 0; rep < 4; ++rep) {
            y.up(hy);
            tm.start();
            gpk_trsv_lower(DT<T>::v, K.p, n, n, 0, dsb.p, sb, y.p, 1, 1, 0, tmp.p, 1, nullptr);
            const float ms = tm.stop();
            if (rep) printf("PERFTRSV %s n=%d sb=%d per-block   %.3f ms  %.2f TB/s\n", DT<T>::name(), n, sb, ms, 0.5 * n * (double)n * sizeof(T) / ms * 1e-9);
        }
    }
}

// XOR of every 32-bit word of the lower triangles of `batch` n x n fp32 matrices: an order-independent fingerprint of ALL factors of a
// batched factorisation (--batched-stress)
__global__ void xor_lower_kernel(const unsigned* a, int n, long long per, unsigned* out) {
    const long long b = blockIdx.y;
    const int row = blockIdx.x;
    unsigned v = 0;
    for (int c = threadIdx.x; c <= row; c += blockDim.x) v ^= a[b * per + (long long)row * n + c] * (unsigned)(2654435761u + row + 7 * c);
    for (int off = 32; off > 0; off >>= 1) v ^= __shfl_xor(v, off);
    if ((threadIdx.x & 63) == 0) atomicXor(out, v);
}

// The VJP of the Cholesky factorisation (gpk_potrf_vjp)   --potrf-vjp
// Against an 80-bit host evaluation of the formula of include/gpk.h on the factor as the device left it (so the error is the
// entry's own): abar = W^T Psym W, W = L^{-1}, Psym = (P + P^T) / 2, P = Phi(L^T tril(lbar)).  NaN is planted in the strict upper
// triangles of l and lbar (garbage by contract); padded leading dimensions; a second call must write the same bits.
template <typename T>
static void test_potrf_vjp() {
    const double tol = sizeof(T) == 8 ? 1e-9 : 2e-3;
    for (int n : {1, 127, 129, 300}) {
        for (int sb : {128, 256}) {
            if (sb == 256 && n != 300) continue;
            const int ld = n + 5, ldlb = n + 3, lda = n + 7;
            std::vector<double> a((size_t)n * (n + 8));
            { std::normal_distribution<double> d(0.0, 1.0); for (auto& v : a) v = d(rng) / std::sqrt((double)(n + 8)); }
            std::vector<T> hA((size_t)n * ld, (T)0), hB((size_t)n * ldlb, (T)0);
            for (int i = 0; i < n; ++i)
                for (int j = 0; j <= i; ++j) {
                    double acc = i == j ? 0.5 : 0.0;
                    for (int k = 0; k < n + 8; ++k) acc += a[(size_t)i * (n + 8) + k] * a[(size_t)j * (n + 8) + k];
                    hA[(size_t)i * ld + j] = (T)acc;
                }
            { std::normal_distribution<double> d(0.0, 1.0); for (int i = 0; i < n; ++i) for (int j = 0; j <= i; ++j) hB[(size_t)i * ldlb + j] = (T)d(rng); }
            Dev<T> dA(hA.size()), dB(hB.size()), dinv(gpk_dinv_elems(n)), dsb((size_t)((n + sb - 1) / sb) * sb * sb),
                tmpm((size_t)((n + sb - 1) / sb) * sb * sb / 4 + 16), out((size_t)n * lda), ws((size_t)gpk_potrf_vjp_ws_elems(n, sb));
            Dev<int> info(1);
            info.zero();
            dA.up(hA);
            int st = gpk_potrf(DT<T>::v, dA.p, n, ld, 0, 1, dinv.p, info.p, 0, nullptr);
            st |= gpk_trtri_merge(DT<T>::v, dA.p, n, ld, 0, 1, dinv.p, sb, dsb.p, tmpm.p, nullptr);
            HIPCHK(hipDeviceSynchronize());
            std::vector<T> hL = dA.down();
            const T nan = std::numeric_limits<T>::quiet_NaN();
            for (int i = 0; i < n; ++i) {
                for (int j = i + 1; j < ld; ++j) hL[(size_t)i * ld + j] = nan;
                for (int j = i + 1; j < ldlb; ++j) hB[(size_t)i * ldlb + j] = nan;
            }
            dA.up(hL);
            dB.up(hB);
            std::vector<T> sentinel(out.n, (T)-7);
            out.up(sentinel);
            st |= gpk_potrf_vjp(DT<T>::v, dA.p, n, ld, dsb.p, sb, dB.p, ldlb, out.p, lda, ws.p, nullptr);
            HIPCHK(hipDeviceSynchronize());
            const std::vector<T> got = out.down();
            st |= gpk_potrf_vjp(DT<T>::v, dA.p, n, ld, dsb.p, sb, dB.p, ldlb, out.p, lda, ws.p, nullptr);
            HIPCHK(hipDeviceSynchronize());
            const std::vector<T> again = out.down();
            // the 80-bit reference
            typedef long double R;
            std::vector<R> L((size_t)n * n, 0), W((size_t)n * n, 0), P((size_t)n * n, 0), Tm((size_t)n * n, 0), ref((size_t)n * n, 0);
            for (int i = 0; i < n; ++i) for (int j = 0; j <= i; ++j) L[(size_t)i * n + j] = (R)hL[(size_t)i * ld + j];
            parallel_for(n, [&](int j) {                       // column j of W = L^{-1} by forward substitution
                for (int i = j; i < n; ++i) {
                    R acc = i == j ? 1.0L : 0.0L;
                    for (int k = j; k < i; ++k) acc -= L[(size_t)i * n + k] * W[(size_t)k * n + j];
                    W[(size_t)i * n + j] = acc / L[(size_t)i * n + i];
                }
            });
            parallel_for(n, [&](int i) {                       // Psym from the lower triangle of L^T tril(lbar)
                for (int j = 0; j <= i; ++j) {
                    R acc = 0;
                    for (int k = i; k < n; ++k) acc += L[(size_t)k * n + i] * (R)hB[(size_t)k * ldlb + j];
                    P[(size_t)i * n + j] = 0.5L * acc;
                }
            });
            for (int i = 0; i < n; ++i) for (int j = i + 1; j < n; ++j) P[(size_t)i * n + j] = P[(size_t)j * n + i];
            parallel_for(n, [&](int i) {                       // Tm = Psym W
                for (int j = 0; j < n; ++j) {
                    R acc = 0;
                    for (int k = j; k < n; ++k) acc += P[(size_t)i * n + k] * W[(size_t)k * n + j];
                    Tm[(size_t)i * n + j] = acc;
                }
            });
            parallel_for(n, [&](int i) {                       // ref = W^T Tm
                for (int j = 0; j < n; ++j) {
                    R acc = 0;
                    for (int k = i; k < n; ++k) acc += W[(size_t)k * n + i] * Tm[(size_t)k * n + j];
                    ref[(size_t)i * n + j] = acc;
                }
            });
            double num = 0, den = 0;
            bool sym = true, same = true, kept = true;
            for (int i = 0; i < n; ++i) {
                for (int j = 0; j < n; ++j) {
                    const R r = 0.5L * (ref[(size_t)i * n + j] + ref[(size_t)j * n + i]);
                    const double g = (double)got[(size_t)i * lda + j];
                    if (!std::isfinite(g)) num = INFINITY;
                    num = std::max(num, (double)fabsl((R)g - r));
                    den = std::max(den, (double)fabsl(r));
                    sym = sym && memcmp(&got[(size_t)i * lda + j], &got[(size_t)j * lda + i], sizeof(T)) == 0;
                }
                for (int j = n; j < lda; ++j) kept = kept && got[(size_t)i * lda + j] == (T)-7;
            }
            same = memcmp(got.data(), again.data(), got.size() * sizeof(T)) == 0;
            char name[160];
            snprintf(name, sizeof name, "potrf_vjp %s n=%d sb=%d (NaN above the diagonals, padded ld)", DT<T>::name(), n, sb);
            report(name, st ? INFINITY : num / den, tol);
            snprintf(name, sizeof name, "potrf_vjp %s n=%d sb=%d symmetric / repeatable / in bounds", DT<T>::name(), n, sb);
            report(name, (sym && same && kept) ? 0.0 : 1.0, 0.0);
        }
    }
    // argument codes
    Dev<T> buf(4096);
    int bad = 0;
    bad += gpk_potrf_vjp(7, buf.p, 4, 4, buf.p, 128, buf.p, 4, buf.p, 4, buf.p, nullptr) != -1;
    bad += gpk_potrf_vjp(DT<T>::v, nullptr, 0, 0, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, nullptr) != 0;
    bad += gpk_potrf_vjp(DT<T>::v, nullptr, 4, 4, buf.p, 128, buf.p, 4, buf.p, 4, buf.p, nullptr) != -2;
    bad += gpk_potrf_vjp(DT<T>::v, buf.p, ((int64_t)1 << 20) + 1, (int64_t)1 << 21, buf.p, 128, buf.p, (int64_t)1 << 21, buf.p, (int64_t)1 << 21, buf.p, nullptr) != -3;
    bad += gpk_potrf_vjp(DT<T>::v, buf.p, 4, 3, buf.p, 128, buf.p, 4, buf.p, 4, buf.p, nullptr) != -4;
    bad += gpk_potrf_vjp(DT<T>::v, buf.p, 4, 4, nullptr, 128, buf.p, 4, buf.p, 4, buf.p, nullptr) != -5;
    bad += gpk_potrf_vjp(DT<T>::v, buf.p, 4, 4, buf.p, 100, buf.p, 4, buf.p, 4, buf.p, nullptr) != -6;
    bad += gpk_potrf_vjp(DT<T>::v, buf.p, 4, 4, buf.p, 128, nullptr, 4, buf.p, 4, buf.p, nullptr) != -7;
    bad += gpk_potrf_vjp(DT<T>::v, buf.p, 4, 4, buf.p, 128, buf.p, 3, buf.p, 4, buf.p, nullptr) != -8;
    bad += gpk_potrf_vjp(DT<T>::v, buf.p, 4, 4, buf.p, 128, buf.p, 4, nullptr, 4, buf.p, nullptr) != -9;
    bad += gpk_potrf_vjp(DT<T>::v, buf.p, 4, 4, buf.p, 128, buf.p, 4, buf.p, 3, buf.p, nullptr) != -10;
    bad += gpk_potrf_vjp(DT<T>::v, buf.p, 4, 4, buf.p, 128, buf.p, 4, buf.p, 4, nullptr, nullptr) != -11;
    report(std::string("potrf_vjp ") + DT<T>::name() + " argument codes", bad, 0.0);
}

// The nuclear norm by the Newton-Schulz polar iteration (gpk_nuclear_norm)   --nuclear-norm
// Against a host evaluation of the singular values: one-sided Jacobi (Hestenes) rotations in 80-bit arithmetic on the matrix as the
// device reads it, the sum of the column norms at convergence.  Batches of two with a padded leading dimension and a batch stride
// beyond n * ld, NaN planted in all padding and in the whole workspace; a second call must write the same bits, the input is read only.
static double host_nuclear_norm(std::vector<long double> a, int n) {      // a: n x n row-major, used up
    typedef long double R;
    for (int sweep = 0; sweep < 60; ++sweep) {
        R off = 0;
        for (int p = 0; p < n - 1; ++p)
            for (int q = p + 1; q < n; ++q) {
                R app = 0, aqq = 0, apq = 0;
                for (int i = 0; i < n; ++i) {
                    const R x = a[(size_t)i * n + p], y = a[(size_t)i * n + q];
                    app += x * x; aqq += y * y; apq += x * y;
                }
                if (apq == 0 || fabsl(apq) <= 1e-19L * sqrtl(app * aqq)) continue;
                off = std::max(off, fabsl(apq) / sqrtl(app * aqq));
                const R zeta = (aqq - app) / (2 * apq);
                const R t = (zeta >= 0 ? 1.0L : -1.0L) / (fabsl(zeta) + sqrtl(1 + zeta * zeta));
                const R c = 1 / sqrtl(1 + t * t), s = c * t;
                for (int i = 0; i < n; ++i) {
                    const R x = a[(size_t)i * n + p], y = a[(size_t)i * n + q];
                    a[(size_t)i * n + p] = c * x - s * y;
                    a[(size_t)i * n + q] = s * x + c * y;
                }
            }
        if (off < 1e-17L) break;
    }
    R sum = 0;
    for (int j = 0; j < n; ++j) {
        R ss = 0;
        for (int i = 0; i < n; ++i) ss += a[(size_t)i * n + j] * a[(size_t)i * n + j];
        sum += sqrtl(ss);
    }
    return (double)sum;
}

template <typename T>
static void test_nuclear_norm() {
    const double tol = sizeof(T) == 8 ? 1e-12 : 1e-5;
    const int iters = sizeof(T) == 8 ? 60 : 40;
    const T nan = std::numeric_limits<T>::quiet_NaN();
    for (int n : {1, 33, 129, 200}) {
        const int batch = 2, ld = n + 5;
        const size_t sm = (size_t)n * ld + 11;
        std::vector<T> hM(sm * batch, nan);
        std::normal_distribution<double> d(0.0, 1.0);
        for (int b = 0; b < batch; ++b)
            for (int i = 0; i < n; ++i)
                for (int j = 0; j < n; ++j) hM[b * sm + (size_t)i * ld + j] = (T)((b ? 3.0 : 0.25) * d(rng));
        const size_t wse = (size_t)gpk_nuclear_norm_ws_elems(n, batch);
        Dev<T> dM(hM.size()), out(batch + 2), ws(wse);
        dM.up(hM);
        ws.up(std::vector<T>(wse, nan));
        out.up(std::vector<T>(batch + 2, (T)-7));
        int st = gpk_nuclear_norm(DT<T>::v, dM.p, n, ld, (int64_t)sm, batch, iters, out.p, ws.p, nullptr);
        HIPCHK(hipDeviceSynchronize());
        const std::vector<T> got = out.down();
        st |= gpk_nuclear_norm(DT<T>::v, dM.p, n, ld, (int64_t)sm, batch, iters, out.p, ws.p, nullptr);
        HIPCHK(hipDeviceSynchronize());
        const std::vector<T> again = out.down(), after = dM.down();
        std::vector<double> ref(batch);
        parallel_for(batch, [&](int b) {
            std::vector<long double> a((size_t)n * n);
            for (int i = 0; i < n; ++i) for (int j = 0; j < n; ++j) a[(size_t)i * n + j] = (long double)hM[b * sm + (size_t)i * ld + j];
            ref[b] = host_nuclear_norm(a, n);
        });
        double err = 0;
        for (int b = 0; b < batch; ++b) err = std::max(err, std::isfinite((double)got[b]) ? std::fabs((double)got[b] - ref[b]) / ref[b] : INFINITY);
        char name[160];
        snprintf(name, sizeof name, "nuclear_norm %s n=%d batch=2 (NaN in padding and workspace)", DT<T>::name(), n);
        report(name, st ? INFINITY : err, tol);
        const bool ok = memcmp(got.data(), again.data(), got.size() * sizeof(T)) == 0 && got[batch] == (T)-7 && got[batch + 1] == (T)-7 &&
                        memcmp(after.data(), hM.data(), hM.size() * sizeof(T)) == 0;
        snprintf(name, sizeof name, "nuclear_norm %s n=%d repeatable / in bounds / input kept", DT<T>::name(), n);
        report(name, ok ? 0.0 : 1.0, 0.0);
    }
    {   // exact cases: the zero matrix gives 0 (no 0 / 0), the identity gives n
        const int n = 40;
        std::vector<T> hM((size_t)2 * n * n, (T)0);
        for (int i = 0; i < n; ++i) hM[(size_t)n * n + (size_t)i * n + i] = (T)1;
        Dev<T> dM(hM.size()), out(2), ws((size_t)gpk_nuclear_norm_ws_elems(n, 2));
        dM.up(hM);
        const int st = gpk_nuclear_norm(DT<T>::v, dM.p, n, n, (int64_t)n * n, 2, iters, out.p, ws.p, nullptr);
        HIPCHK(hipDeviceSynchronize());
        const std::vector<T> got = out.down();
        report(std::string("nuclear_norm ") + DT<T>::name() + " zero matrix = 0", st ? INFINITY : std::fabs((double)got[0]), 0.0);
        report(std::string("nuclear_norm ") + DT<T>::name() + " identity = n", st ? INFINITY : std::fabs((double)got[1] - n) / n, tol);
    }
    // workspace size and argument codes
    Dev<T> buf(4096);
    int bad = 0;
    bad += gpk_nuclear_norm_ws_elems(200, 3) != 3 * (3 * 200 * 208 + 7 + 1);
    bad += gpk_nuclear_norm_ws_elems(0, 3) != 0 || gpk_nuclear_norm_ws_elems(-1, 1) != 0 || gpk_nuclear_norm_ws_elems(5, 0) != 0;
    bad += gpk_nuclear_norm(7, buf.p, 4, 4, 16, 1, 5, buf.p, buf.p, nullptr) != -1;
    bad += gpk_nuclear_norm(DT<T>::v, nullptr, 0, 0, 0, 1, 0, nullptr, nullptr, nullptr) != 0;
    bad += gpk_nuclear_norm(DT<T>::v, nullptr, 4, 4, 16, 0, 0, nullptr, nullptr, nullptr) != 0;
    bad += gpk_nuclear_norm(DT<T>::v, nullptr, 4, 4, 16, 1, 5, buf.p, buf.p, nullptr) != -2;
    bad += gpk_nuclear_norm(DT<T>::v, buf.p, ((int64_t)1 << 20) + 1, (int64_t)1 << 21, 0, 1, 5, buf.p, buf.p, nullptr) != -3;
    bad += gpk_nuclear_norm(DT<T>::v, buf.p, 4, 3, 16, 1, 5, buf.p, buf.p, nullptr) != -4;
    bad += gpk_nuclear_norm(DT<T>::v, buf.p, 4, 4, -1, 2, 5, buf.p, buf.p, nullptr) != -5;
    bad += gpk_nuclear_norm(DT<T>::v, buf.p, 4, 4, 0, 65536, 5, buf.p, buf.p, nullptr) != -6;
    bad += gpk_nuclear_norm(DT<T>::v, buf.p, 4, 4, 16, 1, 0, buf.p, buf.p, nullptr) != -7;
    bad += gpk_nuclear_norm(DT<T>::v, buf.p, 4, 4, 16, 1, 5, nullptr, buf.p, nullptr) != -8;
    bad += gpk_nuclear_norm(DT<T>::v, buf.p, 4, 4, 16, 1, 5, buf.p, nullptr, nullptr) != -9;
    report(std::string("nuclear_norm ") + DT<T>::name() + " workspace size and argument codes", bad, 0.0);
}

// ----------------------------------------------------------------------------
// The bordered Cholesky factorisation (gpk_potrf_border)   --append
// The entry takes V = L11^{-1} K12 from its caller, so the contract is checked on operands made up here -- a random well-conditioned
// lower-triangular L11, a random V and K22 = V^T V + M M^T + I -- against 80-bit host loops, in units of eps and with the bounds any
// order of summation guarantees (Higham's gamma_k, k = the number of terms of the longest sum):
//   L21 is V^T bit for bit;   |K22 - V^T V - L22 L22^T| <= (n + q + 1) eps (|K22| + |V|^T |V| + |L22| |L22|^T);
//   |w2 - L22^{-1} (r2 - V^T w1)| <= (n + q + 1) eps |L22^{-1}| (|r2| + |V|^T |w1|), L22 as the device left it;
//   |D_g L_gg - I| <= 129 eps |D_g| |L_gg| for the touched 128-blocks of the grown factor, identity-padded;
//   nothing else is written (sentinels in the old rows, the padding columns, the rows behind the factor, the lower dinv blocks);
//   a second call writes the same bits;   info = n + j for a K22 whose j-th new pivot is not positive;   the argument codes.
// Shapes: those of tests/test_potrf_border_gpu.py, one with a padded leading dimension, one in a capacity buffer.
template <typename T>
static void test_append() {
    typedef long double R;
    const double eps = std::numeric_limits<T>::epsilon();
    const T sentinel = (T)777;
    struct Shape { int n, q, extra_ld, extra_rows; };
    const Shape shapes[] = {{1, 1, 0, 0}, {127, 1, 0, 0}, {128, 1, 0, 0}, {130, 126, 0, 0}, {130, 127, 0, 0}, {130, 127, 16, 0}, {200, 128, 0, 0},
                            {200, 128, 184, 184}, {384, 64, 0, 0}, {1000, 5, 0, 0}, {1000, 9, 0, 0}, {4133, 16, 0, 0}};
    for (const Shape& sh : shapes) {
        const int n = sh.n, q = sh.q, m = n + q, ld = m + sh.extra_ld, rows = m + sh.extra_rows;
        const int nblk = (m + 127) / 128, keep = n / 128;
        std::normal_distribution<double> d(0.0, 1.0);
        std::vector<T> hA((size_t)rows * ld, sentinel), hV((size_t)n * q), hM((size_t)q * q), hw1(n), hr2(q);
        for (int i = 0; i < n; ++i)
            for (int j = 0; j <= i; ++j) hA[(size_t)i * ld + j] = (T)(i == j ? 1.0 + std::fabs(d(rng)) : 0.5 * d(rng) / std::sqrt((double)n));
        for (auto& x : hV) x = (T)(d(rng) / std::sqrt((double)n));
        for (auto& x : hM) x = (T)(d(rng) / std::sqrt((double)q));
        for (auto& x : hw1) x = (T)d(rng);
        for (auto& x : hr2) x = (T)d(rng);
        std::vector<R> gram((size_t)q * q), agram((size_t)q * q);           // V^T V and |V|^T |V|, lower triangles
        parallel_for(q, [&](int i) {
            for (int j = 0; j <= i; ++j) {
                R s = 0, a = 0;
                for (int k = 0; k < n; ++k) { const R p = (R)hV[(size_t)k * q + i] * (R)hV[(size_t)k * q + j]; s += p; a += fabsl(p); }
                gram[(size_t)i * q + j] = s; agram[(size_t)i * q + j] = a;
            }
        });
        for (int i = 0; i < q; ++i)
            for (int j = 0; j <= i; ++j) {
                R s = gram[(size_t)i * q + j] + (i == j ? 1 : 0);
                for (int k = 0; k < q; ++k) s += (R)hM[(size_t)i * q + k] * (R)hM[(size_t)j * q + k];
                hA[(size_t)(n + i) * ld + n + j] = (T)s;
            }
        const size_t wse = (size_t)gpk_potrf_border_ws_elems(n, q);
        Dev<T> dA(hA.size()), dV(hV.size()), dinv((size_t)nblk * 128 * 128), w1(n), r2(q), ws(wse);
        Dev<int> info(1);
        const std::vector<T> hD((size_t)nblk * 128 * 128, sentinel);
        auto run = [&](const std::vector<T>& a0, bool rhs, std::vector<T>& a1, std::vector<T>& d1, std::vector<T>& w2) -> int {
            dA.up(a0); dV.up(hV); dinv.up(hD); w1.up(hw1); r2.up(hr2);
            ws.up(std::vector<T>(wse, std::numeric_limits<T>::quiet_NaN()));
            std::vector<int> one(1, -5);
            HIPCHK(hipMemcpy(info.p, one.data(), sizeof(int), hipMemcpyHostToDevice));
            const int st = gpk_potrf_border(DT<T>::v, dA.p, n, q, ld, dV.p, q, dinv.p, rhs ? w1.p : nullptr, rhs ? r2.p : nullptr, info.p, ws.p, nullptr);
            HIPCHK(hipDeviceSynchronize());
            a1 = dA.down(); d1 = dinv.down(); w2 = r2.down();
            HIPCHK(hipMemcpy(one.data(), info.p, sizeof(int), hipMemcpyDeviceToHost));
            return st ? -1000 + st : one[0];
        };
        std::vector<T> a1, d1, w2, a2, d2, w2b;
        const int inf = run(hA, true, a1, d1, w2);
        const int inf2 = run(hA, true, a2, d2, w2b);
        char name[200], tag[80];
        snprintf(tag, sizeof tag, "%s n=%d q=%d ld=%d rows=%d", DT<T>::name(), n, q, ld, rows);
        // untouched memory, L21 = V^T, repeatability
        bool same = inf == 0 && inf2 == 0;
        for (int i = 0; i < rows && same; ++i)
            for (int j = 0; j < ld; ++j) {
                const size_t at = (size_t)i * ld + j;
                const bool written = i >= n && i < m && j < m;      // (right of the diagonal the new rows are unspecified)
                if (!written && memcmp(&a1[at], &hA[at], sizeof(T)) != 0) { same = false; break; }
                if (i >= n && i < m && j < n && memcmp(&a1[at], &hV[(size_t)j * q + (i - n)], sizeof(T)) != 0) { same = false; break; }
            }
        for (size_t at = 0; at < (size_t)keep * 128 * 128 && same; ++at) same = d1[at] == sentinel;
        same = same && memcmp(a1.data(), a2.data(), a1.size() * sizeof(T)) == 0 && memcmp(d1.data(), d2.data(), d1.size() * sizeof(T)) == 0 &&
               memcmp(w2.data(), w2b.data(), w2.size() * sizeof(T)) == 0;
        snprintf(name, sizeof name, "append %s untouched / L21 = V^T / repeatable", tag);
        report(name, same ? 0.0 : 1.0, 0.0);
        // L22
        auto L = [&](int i, int j) -> R { return j <= i ? (R)a1[(size_t)(n + i) * ld + n + j] : (R)0; };
        double worst = 0;
        for (int i = 0; i < q; ++i)
            for (int j = 0; j <= i; ++j) {
                R s = 0, a = 0;
                for (int k = 0; k <= j; ++k) { s += L(i, k) * L(j, k); a += fabsl(L(i, k) * L(j, k)); }
                const R k22 = (R)hA[(size_t)(n + i) * ld + n + j];
                const R res = fabsl(k22 - gram[(size_t)i * q + j] - s), scale = fabsl(k22) + agram[(size_t)i * q + j] + a;
                worst = std::max(worst, std::isfinite((double)res) ? (double)(res / (eps * scale)) : INFINITY);
            }
        snprintf(name, sizeof name, "append %s |K22 - V^T V - L22 L22^T| (units of eps)", tag);
        report(name, worst, n + q + 1);
        // w2 against substitution in 80 bits with the device's L22; the tolerance needs |L22^{-1}|
        {
            std::vector<R> inv((size_t)q * q, 0), t(q), at(q);
            for (int c = 0; c < q; ++c)
                for (int i = c; i < q; ++i) {
                    R s = i == c ? 1 : 0;
                    for (int k = c; k < i; ++k) s -= L(i, k) * inv[(size_t)k * q + c];
                    inv[(size_t)i * q + c] = s / L(i, i);
                }
            for (int i = 0; i < q; ++i) {
                R s = hr2[i], a = fabsl((R)hr2[i]);
                for (int k = 0; k < n; ++k) { const R p = (R)hV[(size_t)k * q + i] * (R)hw1[k]; s -= p; a += fabsl(p); }
                t[i] = s; at[i] = a;
            }
            worst = 0;
            for (int i = 0; i < q; ++i) {
                R want = 0, tol = 0;
                for (int k = 0; k <= i; ++k) { want += inv[(size_t)i * q + k] * t[k]; tol += fabsl(inv[(size_t)i * q + k]) * at[k]; }
                const R err = fabsl((R)w2[i] - want);
                worst = std::max(worst, std::isfinite((double)err) ? (double)(err / (eps * tol)) : INFINITY);
            }
            snprintf(name, sizeof name, "append %s w2 = L22^{-1} (r2 - V^T w1) (units of eps)", tag);
            report(name, worst, n + q + 1);
        }
        // the touched diagonal-block inverses of the grown factor
        worst = 0;
        bool shape_ok = true;
        for (int g = keep; g < nblk; ++g) {
            const int nv = std::min(128, m - 128 * g);
            auto Lg = [&](int i, int j) -> R { return (i < nv && j <= i) ? (R)a1[(size_t)(128 * g + i) * ld + 128 * g + j] : (R)(i == j ? 1 : 0); };
            const T* D = d1.data() + (size_t)g * 128 * 128;
            for (int i = 0; i < 128; ++i)
                for (int j = 0; j < 128; ++j) {
                    if (j > i) { shape_ok = shape_ok && D[i * 128 + j] == (T)0; continue; }
                    if (i >= nv) { shape_ok = shape_ok && D[i * 128 + j] == (T)(i == j ? 1 : 0); continue; }
                    R s = 0, a = 0;
                    for (int k = j; k <= i; ++k) { s += (R)D[i * 128 + k] * Lg(k, j); a += fabsl((R)D[i * 128 + k] * Lg(k, j)); }
                    const R res = fabsl(s - (i == j ? 1 : 0));
                    worst = std::max(worst, std::isfinite((double)res) ? (double)(res / (eps * a)) : INFINITY);
                }
        }
        snprintf(name, sizeof name, "append %s |D L - I| of the touched 128-blocks (units of eps)", tag);
        report(name, shape_ok ? worst : INFINITY, 129);
        // without a residual: the same factor;   a non-positive pivot: info = n + its order
        std::vector<T> a3, d3, w3;
        const int inf3 = run(hA, false, a3, d3, w3);
        bool ok = inf3 == 0 && memcmp(a1.data(), a3.data(), a1.size() * sizeof(T)) == 0 && memcmp(d1.data(), d3.data(), d1.size() * sizeof(T)) == 0 &&
                  memcmp(w3.data(), hr2.data(), w3.size() * sizeof(T)) == 0;
        const int jbad = q / 2;
        std::vector<T> hB = hA;
        hB[(size_t)(n + jbad) * ld + n + jbad] = (T)(gram[(size_t)jbad * q + jbad] * 0.5L);      // below V^T V alone: the pivot is negative
        const int inf4 = run(hB, false, a3, d3, w3);
        ok = ok && inf4 == n + jbad + 1;
        for (int i = 0; i < n && ok; ++i) ok = memcmp(&a3[(size_t)i * ld], &hA[(size_t)i * ld], (size_t)ld * sizeof(T)) == 0;
        snprintf(name, sizeof name, "append %s no residual: same factor / info = n + j (got %d, want %d)", tag, inf4, n + jbad + 1);
        report(name, ok ? 0.0 : 1.0, 0.0);
    }
    // workspace size and argument codes (nothing is launched)
    Dev<T> buf(4096);
    Dev<int> info(1);
    int bad = 0;
    bad += gpk_version() < 112;
    bad += gpk_potrf_border_ws_elems(1000, 9) <= 0 || gpk_potrf_border_ws_elems(0, 9) != 0 || gpk_potrf_border_ws_elems(10, 0) != 0 ||
           gpk_potrf_border_ws_elems(10, GPK_BORDER_MAX + 1) != 0;
    bad += gpk_potrf_border(7, buf.p, 20, 4, 24, buf.p, 4, buf.p, buf.p, buf.p, info.p, buf.p, nullptr) != -1;
    bad += gpk_potrf_border(DT<T>::v, nullptr, 20, 4, 24, buf.p, 4, buf.p, buf.p, buf.p, info.p, buf.p, nullptr) != -2;
    bad += gpk_potrf_border(DT<T>::v, buf.p, 0, 4, 24, buf.p, 4, buf.p, buf.p, buf.p, info.p, buf.p, nullptr) != -3;
    bad += gpk_potrf_border(DT<T>::v, buf.p, 20, 0, 24, buf.p, 4, buf.p, buf.p, buf.p, info.p, buf.p, nullptr) != -4;
    bad += gpk_potrf_border(DT<T>::v, buf.p, 20, 129, 200, buf.p, 129, buf.p, buf.p, buf.p, info.p, buf.p, nullptr) != -4;
    bad += gpk_potrf_border(DT<T>::v, buf.p, 20, 4, 23, buf.p, 4, buf.p, buf.p, buf.p, info.p, buf.p, nullptr) != -5;
    bad += gpk_potrf_border(DT<T>::v, buf.p, 20, 4, 24, nullptr, 4, buf.p, buf.p, buf.p, info.p, buf.p, nullptr) != -6;
    bad += gpk_potrf_border(DT<T>::v, buf.p, 20, 4, 24, buf.p, 3, buf.p, buf.p, buf.p, info.p, buf.p, nullptr) != -7;
    bad += gpk_potrf_border(DT<T>::v, buf.p, 20, 4, 24, buf.p, 4, nullptr, buf.p, buf.p, info.p, buf.p, nullptr) != -8;
    bad += gpk_potrf_border(DT<T>::v, buf.p, 20, 4, 24, buf.p, 4, buf.p, nullptr, buf.p, info.p, buf.p, nullptr) != -9;
    bad += gpk_potrf_border(DT<T>::v, buf.p, 20, 4, 24, buf.p, 4, buf.p, buf.p, nullptr, info.p, buf.p, nullptr) != -10;
    bad += gpk_potrf_border(DT<T>::v, buf.p, 20, 4, 24, buf.p, 4, buf.p, buf.p, buf.p, nullptr, buf.p, nullptr) != -11;
    bad += gpk_potrf_border(DT<T>::v, buf.p, 20, 4, 24, buf.p, 4, buf.p, buf.p, buf.p, info.p, nullptr, nullptr) != -12;
    report(std::string("append ") + DT<T>::name() + " version, workspace size and argument codes", bad, 0.0);
}

int main(int argc, char** argv) {
    bool do_perf = false, only_perf = false;
    for (int i = 1; i + 2 < argc; ++i)     // --set KEY VALUE: tuning knobs (gpk_debug_set)
        if (!strcmp(argv[i], "--set")) gpk_tune(atoi(argv[i + 1]), atoll(argv[i + 2]));
    for (int i = 1; i < argc; ++i) {
        if (!strcmp(argv[i], "--batched-stress") && i + 1 < argc) {   // REPS runs of the mixed-phase batched factorisation against ONE lockstep run: every factor, bit for bit
            const int reps = atoi(argv[i + 1]);
            const int n = 2048, d = 3, batch = 512;
            auto hx = randv<float>((size_t)batch * n * d);
            Dev<float> X(hx.size()), K((size_t)batch * n * n), dinv((size_t)batch * gpk_dinv_elems(n));
            Dev<int> info(batch);
            Dev<unsigned> fp(1);
            X.up(hx);
            int kind = GPK_K_EQ; double var = 1.0, il = 1.0;
            auto run = [&](int mode) -> unsigned {
                gpk_tune(53, mode);
                info.zero();
                fp.zero();
                gpk_kmat(GPK_F32, &kind, &var, &il, nullptr, 1, X.p, n, d, (int64_t)n * d, X.p, n, d, (int64_t)n * d, d, K.p, n, (int64_t)n * n, batch, 1, 1, 0.1, nullptr, 0, 0, nullptr);
                gpk_potrf(GPK_F32, K.p, n, n, (int64_t)n * n, batch, dinv.p, info.p, 0, nullptr);
                hipLaunchKernelGGL(xor_lower_kernel, dim3(n, batch), dim3(256), 0, nullptr, reinterpret_cast<const unsigned*>(K.p), n, (long long)n * n, fp.p);
                unsigned h = 0;
                hipMemcpy(&h, fp.p, sizeof(h), hipMemcpyDeviceToHost);
                std::vector<int> inf(batch);
                hipMemcpy(inf.data(), info.p, sizeof(int) * batch, hipMemcpyDeviceToHost);
                for (int b = 0; b < batch; ++b) if (inf[b] != 0) { printf("info[%d] = %d\n", b, inf[b]); h ^= 0xdeadu; }
                return h;
            };
            const unsigned ref = run(0);
            int bad = 0;
            for (int r = 0; r < reps; ++r) bad += run(1) != ref;
            printf("BATCHED-STRESS %d mixed-phase factorisations of 512 x 2048^2 against the lockstep one (fingerprint %08x of every lower triangle): %d differ\n", reps, ref, bad);
            return bad ? 1 : 0;
        }
        if (!strcmp(argv[i], "--batched") && i + 1 < argc) {   // --batched NBO [BATCH]: BATCH (512) x 2048 f32 potrf with outer block NBO
            const int nbo = atoi(argv[i + 1]);
            const int n = 2048, d = 3, batch = (i + 2 < argc && atoi(argv[i + 2]) >= 8) ? atoi(argv[i + 2]) : 512;
            auto hx = randv<float>((size_t)batch * n * d);
            Dev<float> X(hx.size()), K((size_t)batch * n * n), dinv((size_t)batch * gpk_dinv_elems(n));
            Dev<int> info(batch);
            X.up(hx);
            int kind = GPK_K_EQ; double var = 1.0, il = 1.0;
            Timer tm;
            for (int rep = 0; rep < 3; ++rep) {
                info.zero();
                gpk_kmat(GPK_F32, &kind, &var, &il, nullptr, 1, X.p, n, d, (int64_t)n * d, X.p, n, d, (int64_t)n * d, d, K.p, n, (int64_t)n * n, batch, 1, 1, 0.1, nullptr, 0, 0, nullptr);
                tm.start();
                gpk_potrf(GPK_F32, K.p, n, n, (int64_t)n * n, batch, dinv.p, info.p, nbo, nullptr);
                const float ms = tm.stop();
                if (rep) printf("BATCHED potrf_f32 %dx2048 nbo=%d  %.3f ms  %.2f TFLOP/s\n", batch, nbo, ms, batch * (double)n * n * n / 3.0 / ms * 1e-9);
            }
            {   // the mixed-phase steps against the lockstep launches (dev build: knob 53): the same arithmetic in the same order per entry --
                // the factors of the first and the last 4 matrices, lower triangles, bit by bit
                std::vector<float> ref[2];
                for (int mode = 0; mode < 2; ++mode) {
                    gpk_tune(53, mode);
                    info.zero();
                    gpk_kmat(GPK_F32, &kind, &var, &il, nullptr, 1, X.p, n, d, (int64_t)n * d, X.p, n, d, (int64_t)n * d, d, K.p, n, (int64_t)n * n, batch, 1, 1, 0.1, nullptr, 0, 0, nullptr);
                    gpk_potrf(GPK_F32, K.p, n, n, (int64_t)n * n, batch, dinv.p, info.p, nbo, nullptr);
                    hipDeviceSynchronize();
                    ref[mode].resize((size_t)8 * n * n);
                    hipMemcpy(ref[mode].data(), K.p, (size_t)4 * n * n * sizeof(float), hipMemcpyDeviceToHost);
                    hipMemcpy(ref[mode].data() + (size_t)4 * n * n, K.p + (size_t)(batch - 4) * n * n, (size_t)4 * n * n * sizeof(float), hipMemcpyDeviceToHost);
                }
                size_t diff = 0;
                for (int b = 0; b < 8; ++b)
                    for (int i = 0; i < n; ++i)
                        for (int j = 0; j <= i; ++j) {
                            const size_t at = (size_t)b * n * n + (size_t)i * n + j;
                            if (memcmp(&ref[0][at], &ref[1][at], sizeof(float)) != 0) ++diff;
                        }
                printf("BATCHED mixed-phase steps vs lockstep launches: %zu differing entries in 8 factors (release library: both runs are the default path)\n", diff);
                gpk_tune(53, 1);
            }
            // the forward solve of one right-hand side per matrix (the quadratic form of the log-density)
            auto hy = randv<float>((size_t)batch * n);
            Dev<float> Y(hy.size());
            for (int rep = 0; rep < 4; ++rep) {
                Y.up(hy);
                tm.start();
                gpk_trsv_lower(GPK_F32, K.p, n, n, (int64_t)n * n, dinv.p, 128, Y.p, 1, 1, n, nullptr, batch, nullptr);
                const float ms = tm.stop();
                if (rep) printf("BATCHED trsv_f32 512x2048  %.3f ms  %.2f TB/s (lower triangle + inverted diagonal blocks)\n", ms,
                                batch * (0.5 * n * (double)(n - 128) + 128.0 * n) * sizeof(float) / ms * 1e-9);
            }
            return 0;
        }
        if (!strcmp(argv[i], "--cumask")) { cumask_experiment(); return 0; }
        if (!strcmp(argv[i], "--dispatch")) { dispatch_experiment(); return 0; }
        if (!strcmp(argv[i], "--tileprof")) {                  // --tileprof [K [LOWER [WARM]]]
            const int k = (i + 1 < argc && atoi(argv[i + 1]) > 0) ? atoi(argv[i + 1]) : 1024;
            tile_profile(k, (i + 2 < argc) ? atoi(argv[i + 2]) : 1, (i + 3 < argc) ? atoi(argv[i + 3]) : 0);
            return 0;
        }
        if (!strcmp(argv[i], "--mfmapeak")) { mfma_peak(); return 0; }
        if (!strcmp(argv[i], "--diagprof") && i + 1 < argc) {
            rsq_precision();
            for (int ver = 0; ver < 3; ++ver) {      // old kernel, 512-thread kernel, the same inside the pipelined panel
                diag_phase_profile<double>(atoi(argv[i + 1]), ver > 0, ver == 2);
                diag_phase_profile<float>(atoi(argv[i + 1]), ver > 0, ver == 2);
            }
            return 0;
        }
        if (!strcmp(argv[i], "--profile") && i + 3 < argc) {   // --profile f64|f32 N NBO
            const int n = atoi(argv[i + 2]), nbo = atoi(argv[i + 3]);
            if (!strcmp(argv[i + 1], "f64")) profile_one<double>(n, nbo, 2); else profile_one<float>(n, nbo, 2);
            return 0;
        }
        if (!strcmp(argv[i], "--gemm") && i + 4 < argc) {      // --gemm f64|f32 M N K [flags]
            const int M = atoi(argv[i + 2]), N = atoi(argv[i + 3]), K = atoi(argv[i + 4]);
            const int flags = (i + 5 < argc) ? atoi(argv[i + 5]) : 0;
            const int64_t lda = (i + 6 < argc) ? atoll(argv[i + 6]) : -1;
            if (!strcmp(argv[i + 1], "f64")) gemm_one<double>(M, N, K, flags, 4, lda); else gemm_one<float>(M, N, K, flags, 4, lda);
            return 0;
        }
        if (!strcmp(argv[i], "--census")) { census(); return 0; }
        if (!strcmp(argv[i], "--perf-kmat")) { perf_kmat(); return 0; }
        if (!strcmp(argv[i], "--perf-diff")) {                 // the derivative launch against the plain one, N = 16384, D = 8
            for (int lower = 1; lower >= 0; --lower) { perf_diff_case<double>(16384, 8, lower); perf_diff_case<float>(16384, 8, lower); }
            return 0;
        }
        if (!strcmp(argv[i], "--perf-fill") && i + 1 < argc) {      // --perf-fill N: plain POTRF at N for several splits of the workers between panel tasks and fill tiles
            const int n = atoi(argv[i + 1]);
            for (int wg : {-1, 16, 32, 48, 64, 85, 128, 170}) {
                gpk_tune(38, wg < 0 ? 0 : 1);
                gpk_tune(39, wg < 0 ? 0 : wg);
                printf("FILL panel workgroups %d (fill %s):\n", wg, wg < 0 ? "off" : "on");
                perf_la_tail<double>({n});
                perf_la_tail<float>({n});
            }
            gpk_tune(38, 1); gpk_tune(39, 0);
            return 0;
        }
        if (!strcmp(argv[i], "--perf-la-tail")) { perf_la_tail<double>({6144, 8192, 10240, 12288, 16384}); perf_la_tail<float>({8192, 12288, 16384, 32768}); return 0; }
        if (!strcmp(argv[i], "--perf-pipe")) { perf_pipe<double>(); perf_pipe<float>(); return 0; }
        if (!strcmp(argv[i], "--perf-trsv")) { perf_trsv<double>(16384, {512, 1024, 2048}); perf_trsv<float>(32768, {256, 512, 1024}); return 0; }
        if (!strcmp(argv[i], "--perf-trsm")) { perf_trsm<double>(16384, 2048); perf_trsm<float>(32768, 2048); return 0; }
        if (!strcmp(argv[i], "--kmat")) {                      // only the kernel-matrix checks, both kernels
            for (int band = 1; band >= 0; --band) { gpk_tune(12, band); test_kmat<double>(); test_kmat<float>(); }
            printf("SUMMARY pass=%d fail=%d\n", g_pass, g_fail);
            return g_fail ? 1 : 0;
        }
        if (!strcmp(argv[i], "--rq")) {                        // only the checks of the kind with a shape parameter (rational quadratic)
            test_rq<double>(); test_rq<float>();
            printf("SUMMARY pass=%d fail=%d\n", g_pass, g_fail);
            return g_fail ? 1 : 0;
        }
        if (!strcmp(argv[i], "--diff")) {                      // only the checks of the derivative blocks (gpk_kmat_diff), both kernels
            test_diff<double>(); test_diff<float>();
            printf("SUMMARY pass=%d fail=%d\n", g_pass, g_fail);
            return g_fail ? 1 : 0;
        }
        if (!strcmp(argv[i], "--batch-terms")) {               // only the checks of the per-batch term tables, both kernels
            for (int band = 1; band >= 0; --band) { gpk_tune(12, band); test_batch_terms<double>(); test_batch_terms<float>(); }
            printf("SUMMARY pass=%d fail=%d\n", g_pass, g_fail);
            return g_fail ? 1 : 0;
        }
        if (!strcmp(argv[i], "--scaled")) {                    // only the checks of gpk_kmat_scaled, both kernels
            for (int band = 1; band >= 0; --band) { gpk_tune(12, band); test_scaled<double>(); test_scaled<float>(); }
            printf("SUMMARY pass=%d fail=%d\n", g_pass, g_fail);
            return g_fail ? 1 : 0;
        }
        if (!strcmp(argv[i], "--delta")) {                     // only the checks of the Delta kind
            test_delta<double>(); test_delta<float>();
            printf("SUMMARY pass=%d fail=%d\n", g_pass, g_fail);
            return g_fail ? 1 : 0;
        }
        if (!strcmp(argv[i], "--potrf-vjp")) {                 // only the checks of the Cholesky VJP (gpk_potrf_vjp)
            test_potrf_vjp<double>(); test_potrf_vjp<float>();
            printf("SUMMARY pass=%d fail=%d\n", g_pass, g_fail);
            return g_fail ? 1 : 0;
        }
        if (!strcmp(argv[i], "--nuclear-norm")) {              // only the checks of the nuclear norm (gpk_nuclear_norm)
            test_nuclear_norm<double>(); test_nuclear_norm<float>();
            printf("SUMMARY pass=%d fail=%d\n", g_pass, g_fail);
            return g_fail ? 1 : 0;
        }
        if (!strcmp(argv[i], "--append")) {                    // only the checks of the bordered factorisation (gpk_potrf_border)
            test_append<double>(); test_append<float>();
            printf("SUMMARY pass=%d fail=%d\n", g_pass, g_fail);
            return g_fail ? 1 : 0;
        }
        if (!strcmp(argv[i], "--potrf")) {                     // only the factorisation checks (plain + look-ahead)
            test_potrf<double>(); test_potrf<float>();
            test_lookahead<double>(); test_lookahead<float>();
            printf("SUMMARY pass=%d fail=%d\n", g_pass, g_fail);
            return g_fail ? 1 : 0;
        }
        if (!strcmp(argv[i], "--rows")) {                      // only the factorisations with rows under the matrix
            test_potrf_rows<double>(); test_potrf_rows<float>();
        test_potrf_rhs<double>(); test_potrf_rhs<float>();
            test_potrf_rhs<double>(); test_potrf_rhs<float>();
            printf("SUMMARY pass=%d fail=%d\n", g_pass, g_fail);
            return g_fail ? 1 : 0;
        }
        if (!strcmp(argv[i], "--lookahead")) {                 // only the look-ahead / persistent-update checks
            test_lookahead<double>(); test_lookahead<float>();
            printf("SUMMARY pass=%d fail=%d\n", g_pass, g_fail);
            return g_fail ? 1 : 0;
        }
        if (!strcmp(argv[i], "--la-one") && i + 5 < argc) {      // --la-one f64|f32 N NB MODE(-1 = plain potrf) MINROWS [REPS]
            const int n = atoi(argv[i + 2]), nb = atoi(argv[i + 3]), mode = atoi(argv[i + 4]);
            const int64_t mr = atoll(argv[i + 5]);
            const int reps = (i + 6 < argc) ? atoi(argv[i + 6]) : 3;
            const int ldpad = (i + 7 < argc) ? atoi(argv[i + 7]) : 0;
            if (!strcmp(argv[i + 1], "f64")) la_one<double>(n, nb, mode, mr, reps, ldpad); else la_one<float>(n, nb, mode, mr, reps, ldpad);
            return 0;
        }
        if (!strcmp(argv[i], "--perf-agg") && i + 6 < argc) {    // --perf-agg f64|f32 N NB SB ROUNDS TAIL M1 [M2 ...]
            const int n = atoi(argv[i + 2]), nb = atoi(argv[i + 3]), sb = atoi(argv[i + 4]), rounds = atoi(argv[i + 5]);
            const int64_t tail = atoll(argv[i + 6]);
            std::vector<int> ml;
            for (int q = i + 7; q < argc && argv[q][0] != '-'; ++q) ml.push_back(atoi(argv[q]));
            if (ml.empty()) ml = {1, 2};
            if (!strcmp(argv[i + 1], "f64")) perf_agg<double>(n, nb, sb, rounds, ml, tail); else perf_agg<float>(n, nb, sb, rounds, ml, tail);
            return 0;
        }
        if (!strcmp(argv[i], "--perf-rows") && i + 6 < argc) {    // --perf-rows f64|f32 N EXTRA NB SB ROUNDS
            const int n = atoi(argv[i + 2]), extra = atoi(argv[i + 3]), nb = atoi(argv[i + 4]), sb = atoi(argv[i + 5]), rounds = atoi(argv[i + 6]);
            if (!strcmp(argv[i + 1], "f64")) perf_rows<double>(n, extra, nb, sb, rounds); else perf_rows<float>(n, extra, nb, sb, rounds);
            return 0;
        }
        if (!strcmp(argv[i], "--la-clock") && i + 3 < argc) {
            const int warm = (i + 4 < argc) ? atoi(argv[i + 4]) : 0;
            if (!strcmp(argv[i + 1], "f64")) la_clock<double>(atoi(argv[i + 2]), atoi(argv[i + 3]), warm); else la_clock<float>(atoi(argv[i + 2]), atoi(argv[i + 3]), warm);
            return 0;
        }
        if (!strcmp(argv[i], "--perf-la")) {                   // --perf-la [NMAX]
            const int nmax = (i + 1 < argc && atoi(argv[i + 1]) > 0) ? atoi(argv[i + 1]) : 16384;
            perf_la<double>(nmax); perf_la<float>(nmax);
            return 0;
        }
        if (!strcmp(argv[i], "--perf")) do_perf = true;
        if (!strcmp(argv[i], "--only-perf")) do_perf = only_perf = true;
    }
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, 0));
    printf("device: %s  arch=%s  CUs=%d  clock=%d MHz  gpk_version=%d\n", prop.name, prop.gcnArchName, prop.multiProcessorCount, prop.clockRate / 1000, gpk_version());
    if (!only_perf) {
        test_probe<double>(); test_probe<float>();
        gpk_tune(1, 0);                 // force the 128x128-tile kernels
        test_gemm<double>(); test_gemm<float>();
        gpk_tune(1, (int64_t)1 << 40);  // force the 64x64-tile kernels
        test_gemm<double>(); test_gemm<float>();
        gpk_tune(1, 512);               // library default
        test_kmat<double>(); test_kmat<float>();
        test_potrf<double>(); test_potrf<float>();
        test_lookahead<double>(); test_lookahead<float>();
        test_potrf_rows<double>(); test_potrf_rows<float>();
        test_potrf_rhs<double>(); test_potrf_rhs<float>();
        test_misc<double>(); test_misc<float>();
        test_vjp_dense<double>(); test_vjp_dense<float>();
        test_rq<double>(); test_rq<float>();
        test_delta<double>(); test_delta<float>();
        test_diff<double>(); test_diff<float>();
        test_scaled<double>(); test_scaled<float>();
        test_potrf_vjp<double>(); test_potrf_vjp<float>();
        test_nuclear_norm<double>(); test_nuclear_norm<float>();
        test_append<double>(); test_append<float>();
        printf("SUMMARY pass=%d fail=%d\n", g_pass, g_fail);
    }
    if (do_perf) { perf<double>(); perf<float>(); }
    return g_fail ? 1 : 0;
}
