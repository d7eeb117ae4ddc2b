// gpk_border.hip -- the bordered Cholesky factorisation (gpk_potrf_border in include/gpk.h): q <= 128 new rows under a factor of
// order n, O(n q^2 + q^3) behind the caller's O(n^2 q) solve V = L11^{-1} K12, instead of refactorising at n^3 / 3.
//   L21 = V^T,   L22 = chol(K22 - V^T V),   w2 = L22^{-1} (r2 - V^T w1)
// Four launches on the caller's stream:
//   (a) border_gram_kernel     one pass over V: V^T into the new rows of the matrix (tiles transposed through LDS), the partial Gram
//                              matrices V_c^T V_c of at most GRAM_MAX_CHUNKS row chunks (lower 32 x 32 tiles, one workgroup per chunk
//                              and tile) and the partial V_c^T w1 into the workspace;
//       border_sum_kernel      the partials added in chunk order, one thread per element (the second level of the reduction);
//   (b) border_factor_kernel   one workgroup: S = K22 - sum, factorised in LDS by the block routine of the factorisation
//                              (gpk_potrf.hip, diag3_block), w2 by substitution, info;
//   (c) border_inverse_kernel  one workgroup per 128-block of the GROWN factor that has a new row (at most two): the block's lower
//                              triangle from the matrix, inverted in place in LDS, into its slot of `dinv` (identity-padded).
// No atomics, every sum in a fixed order: a repeated call writes the same bits.  No allocation, no host synchronisation.
#include "gpk_common.hpp"

namespace {

constexpr int GT = 32;                  // Gram tile edge, and rows staged per step
constexpr int GRAM_MAX_CHUNKS = 64;     // partial sums per element, added up in chunk order by border_sum_kernel (one thread per element)
constexpr int IP = GPK_DB + 1;          // LDS row pitch of the block that is inverted
constexpr int INV_LANES = 8;            // border_inverse_kernel: lanes per row of the block
constexpr int INV_THREADS = INV_LANES * GPK_DB;

// rows of V per chunk: whole 128-row blocks, at most GRAM_MAX_CHUNKS chunks
static inline int64_t chunk_rows(int64_t n) { return gpk_cdiv(gpk_cdiv(n, GRAM_MAX_CHUNKS), GPK_DB) * GPK_DB; }
static inline int64_t chunk_count(int64_t n) { return gpk_cdiv(n, chunk_rows(n)); }

// Workgroup (c, t): row chunk c of V, lower Gram tile t = (ti, tj), tj <= ti.  256 threads as 8 x 32: thread (ty, tx) owns the sums
// G[32 ti + ty + 8 m][32 tj + tx], m < 4, over the chunk's rows in order.  The tiles with tj == 0 also write their 32 columns of V
// transposed (lanes along the rows of V: unit stride in the matrix) and add up their 32 entries of V_c^T w1.
template <typename T>
__global__ __launch_bounds__(256) void border_gram_kernel(const T* __restrict__ V, int64_t ldv, int64_t n, int q, int64_t chunk,
                                                          T* __restrict__ at, int64_t ld, const T* __restrict__ w1,
                                                          T* __restrict__ gram, T* __restrict__ dots) {
    __shared__ T Vi[GT][GT + 1], Vj[GT][GT + 1], wv[GT];
    int ti = 0, tj = (int)blockIdx.y;
    while (tj > ti) { tj -= ti + 1; ++ti; }
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int64_t r0 = (int64_t)blockIdx.x * chunk;
    const int64_t r1 = r0 + chunk < n ? r0 + chunk : n;
    const int ci = GT * ti + tx, cj = GT * tj + tx;
    T acc[4] = {T(0), T(0), T(0), T(0)};
    T dot = T(0);
    for (int64_t rb = r0; rb < r1; rb += GT) {
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const int64_t r = rb + ty + 8 * m;
            const bool in = r < r1;
            Vi[ty + 8 * m][tx] = (in && ci < q) ? V[r * ldv + ci] : T(0);
            Vj[ty + 8 * m][tx] = (in && cj < q) ? V[r * ldv + cj] : T(0);
        }
        if (ty == 0) wv[tx] = (w1 != nullptr && rb + tx < r1) ? w1[rb + tx] : T(0);
        __syncthreads();
#pragma unroll 8
        for (int k = 0; k < GT; ++k) {
            const T b = Vj[k][tx];
#pragma unroll
            for (int m = 0; m < 4; ++m) acc[m] += Vi[k][ty + 8 * m] * b;
        }
        if (tj == 0) {
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                const int col = GT * ti + ty + 8 * m;
                const int64_t r = rb + tx;
                if (col < q && r < r1) at[(int64_t)col * ld + r] = Vi[tx][ty + 8 * m];
            }
            if (ty == 0 && dots != nullptr) {
#pragma unroll 8
                for (int k = 0; k < GT; ++k) dot += Vi[k][tx] * wv[k];
            }
        }
        __syncthreads();
    }
    T* g = gram + (int64_t)blockIdx.x * q * q;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const int i = GT * ti + ty + 8 * m;
        if (i < q && cj < q) g[(int64_t)i * q + cj] = acc[m];
    }
    if (tj == 0 && ty == 0 && dots != nullptr && ci < q) dots[(int64_t)blockIdx.x * q + ci] = dot;
}

// Second level of the reduction: element e of the q * q + q sums (the Gram matrix, then V^T w1) = its `nparts` partials added in
// chunk order by one thread -- the one-workgroup launch behind it reads one matrix instead of `nparts`.  Entries above the diagonal
// of the Gram matrix are never written by border_gram_kernel and are skipped here.
template <typename T>
__global__ __launch_bounds__(256) void border_sum_kernel(const T* __restrict__ gram, const T* __restrict__ dots, int nparts, int q,
                                                         T* __restrict__ tot) {
    const int qq = q * q;
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= qq + (dots != nullptr ? q : 0)) return;
    T s = T(0);
    if (e < qq) {
        if (e % q > e / q) return;
        for (int k = 0; k < nparts; ++k) s += gram[(int64_t)k * qq + e];
    } else {
        for (int k = 0; k < nparts; ++k) s += dots[(int64_t)k * q + (e - qq)];
    }
    tot[e] = s;
}

// Block g = g0 + blockIdx.x of the factor of order ntot: X = inv(L_gg), identity-padded behind the factor's last row like the blocks
// gpk_potrf leaves.  Column by column from the right, row i:  X[i][j] = -(sum_{k = j+1}^{i} X[i][k] L[k][j]) / L[j][j],
// X[j][j] = 1 / L[j][j] -- row i of X against column j of L, so that X L = I holds row by row to a few rounding errors of
// |X| |L|.  In place: column j of L is overwritten once every thread has read it (the barrier), and the columns right of it, which
// hold X, are only read by the eight lanes of the row that wrote them (one wave: its LDS accesses are in order).
template <typename T>
__global__ __launch_bounds__(INV_THREADS) void border_inverse_kernel(const T* __restrict__ a, int64_t ld, int64_t ntot, int64_t g0,
                                                                     T* __restrict__ dinv) {
    __shared__ T S[GPK_DB * IP];
    const int64_t g = g0 + blockIdx.x, base = g * GPK_DB;
    const int nv = ntot - base < GPK_DB ? (int)(ntot - base) : GPK_DB;
    const T* A = a + base * ld + base;
    const int tid = threadIdx.x;
    for (int idx = tid; idx < GPK_DB * GPK_DB; idx += INV_THREADS) {
        const int r = idx >> 7, c = idx & 127;
        S[r * IP + c] = (r < nv && c <= r) ? A[(int64_t)r * ld + c] : ((r == c) ? T(1) : T(0));
    }
    __syncthreads();
    // eight neighbouring lanes per row: lane part p takes the terms k = j + 1 + p, j + 9 + p, ... of the row's sum (two partial sums,
    // alternating), the eight are added by a butterfly -- every lane of the eight ends up with the same bits, in the same order on every call
    const int i = tid / INV_LANES, part = tid % INV_LANES;
    for (int j = GPK_DB - 1; j >= 0; --j) {
        T x = T(0);
        if (i >= j) {
            T s0 = T(0), s1 = T(0);
            int k = j + 1 + part;
            for (; k + INV_LANES <= i; k += 2 * INV_LANES) {
                s0 += S[i * IP + k] * S[k * IP + j];
                s1 += S[i * IP + k + INV_LANES] * S[(k + INV_LANES) * IP + j];
            }
            if (k <= i) s0 += S[i * IP + k] * S[k * IP + j];
            T s = s0 + s1;
            s += __shfl_xor(s, 1, 64);
            s += __shfl_xor(s, 2, 64);
            s += __shfl_xor(s, 4, 64);
            const T d = S[j * IP + j];
            x = (i == j) ? T(1) / d : -s / d;
        }
        __syncthreads();                       // every thread has read column j of L: it becomes column j of X
        if (i >= j && part == 0) S[i * IP + j] = x;
    }
    __syncthreads();
    T* W = dinv + g * (int64_t)(GPK_DB * GPK_DB);
    for (int idx = tid; idx < GPK_DB * GPK_DB; idx += INV_THREADS) {
        const int r = idx >> 7, c = idx & 127;
        W[idx] = c <= r ? S[r * IP + c] : T(0);
    }
}

}  // namespace

int64_t gpk_potrf_border_ws_elems_impl(int64_t n, int q) {
    if (n < 1 || q < 1 || q > GPK_DB) return 0;
    return (chunk_count(n) + 1) * ((int64_t)q * q + q);      // the partial sums per chunk, and their totals
}

template <typename T>
int gpk_potrf_border_launch(T* a, int64_t n, int q, int64_t ld, const T* v, int64_t ldv, T* dinv, const T* w1, T* r2, int* info, T* ws,
                            hipStream_t stream) {
    if (a == nullptr) return GPK_ERR_ARG(2);
    if (n < 1 || n > (int64_t(1) << 30)) return GPK_ERR_ARG(3);
    if (q < 1 || q > GPK_DB) return GPK_ERR_ARG(4);
    if (ld < n + q) return GPK_ERR_ARG(5);
    if (v == nullptr) return GPK_ERR_ARG(6);
    if (ldv < q) return GPK_ERR_ARG(7);
    if (dinv == nullptr) return GPK_ERR_ARG(8);
    if (w1 == nullptr && r2 != nullptr) return GPK_ERR_ARG(9);
    if (w1 != nullptr && r2 == nullptr) return GPK_ERR_ARG(10);
    if (info == nullptr) return GPK_ERR_ARG(11);
    if (ws == nullptr) return GPK_ERR_ARG(12);
    const int64_t chunk = chunk_rows(n), nchunks = chunk_count(n);
    const int tiles = (q + GT - 1) / GT;
    T* gram = ws;
    T* dots = ws + nchunks * (int64_t)q * q;
    hipLaunchKernelGGL((border_gram_kernel<T>), dim3((unsigned)nchunks, (unsigned)(tiles * (tiles + 1) / 2)), dim3(256), 0, stream, v, ldv,
                       n, q, chunk, a + n * ld, ld, w1, gram, r2 != nullptr ? dots : (T*)nullptr);
    GPK_CHECK_LAUNCH();
    T* tot = dots + nchunks * (int64_t)q;
    hipLaunchKernelGGL((border_sum_kernel<T>), dim3((unsigned)((q * q + q + 255) / 256)), dim3(256), 0, stream, gram,
                       r2 != nullptr ? dots : (const T*)nullptr, (int)nchunks, q, tot);
    GPK_CHECK_LAUNCH();
    const int st = gpk_border_factor_launch<T>(a + n * ld + n, ld, q, tot, r2 != nullptr ? tot + (int64_t)q * q : (const T*)nullptr, 1, r2, info,
                                               (int)n, stream);
    if (st) return st;
    const int64_t g0 = n / GPK_DB, g1 = (n + q - 1) / GPK_DB;
    hipLaunchKernelGGL((border_inverse_kernel<T>), dim3((unsigned)(g1 - g0 + 1)), dim3(INV_THREADS), 0, stream, a, ld, n + q, g0, dinv);
    GPK_CHECK_LAUNCH();
    return GPK_OK;
}
template int gpk_potrf_border_launch<double>(double*, int64_t, int, int64_t, const double*, int64_t, double*, const double*, double*, int*,
                                             double*, hipStream_t);
template int gpk_potrf_border_launch<float>(float*, int64_t, int, int64_t, const float*, int64_t, float*, const float*, float*, int*, float*,
                                            hipStream_t);
