// gpk_nuclear.hip -- the nuclear norm (sum of the singular values) of a batch of square matrices (gpk_nuclear_norm in include/gpk.h):
//   |M|_* = tr(U^T M),   U = the orthogonal polar factor of M = the limit of the Newton-Schulz iteration
//   X_0 = M / |M|_F,     X <- X (3/2 I - 1/2 X^T X)
// Everything cubic runs on the MFMA GEMM with its batch strides -- S = lower(X^T X) (GPK_GEMM_LOWER) and X' = X T per step; the
// kernels here are the quadratic glue with the batch entry in blockIdx.z: the two fixed-order reductions (the Frobenius norm in front,
// sum_ij X_ij M_ij behind), the scaled copy X_0 and the full symmetric T = 3/2 I - 1/2 S from the lower triangle of S (one tiled
// transposed write through LDS).  No atomics, no host read, and a launch sequence that depends on (n, batch, iters) alone: the same
// bits on every call.
#include "gpk_common.hpp"

namespace {

constexpr int VT = 32;         // tile edge of the elementwise kernels and row band of the reductions: 256 threads as 32 x 8
constexpr int RED_MAX = 512;   // most partial sums (workgroups) per batch entry in a reduction

static inline int64_t ws_ld(int64_t n) { return gpk_cdiv(n, 16) * 16; }      // rows of the workspace matrices stay 16-byte aligned
static inline int64_t red_parts(int64_t n) { const int64_t b = gpk_cdiv(n, VT); return b < RED_MAX ? b : RED_MAX; }

// The 256 values of a workgroup added up in LDS, in a fixed tree order; the total is returned to every thread.
__device__ __forceinline__ double block_sum(double v, double* red) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    return red[0];
}

// Stage one of  sum_ij a_ij b_ij  over an n x n view (a == b: the sum of squares): workgroup p of entry z takes the 32-row bands
// p, p + gridDim.x, ...; a thread walks its columns c = tid, tid + 256, ... of every row of a band and keeps its sum in fp64 (both
// dtypes; the operands are exact in fp64, so are their products).  One partial sum per workgroup, rounded to T: part[z * gridDim.x + p].
// Nothing outside the n columns of a row is read.
template <typename T>
__global__ __launch_bounds__(256) void dot_partial_kernel(const T* __restrict__ a, int64_t lda, int64_t sa, const T* __restrict__ b,
                                                          int64_t ldb, int64_t sb, int64_t n, T* __restrict__ part) {
    __shared__ double red[256];
    a += (int64_t)blockIdx.z * sa;
    b += (int64_t)blockIdx.z * sb;
    const int64_t bands = (n + VT - 1) / VT;
    double acc = 0.0;
    for (int64_t band = blockIdx.x; band < bands; band += gridDim.x) {
        const int64_t r1 = (band + 1) * VT < n ? (band + 1) * VT : n;
        for (int64_t r = band * VT; r < r1; ++r) {
            const T* ar = a + r * lda;
            const T* br = b + r * ldb;
            for (int64_t c = threadIdx.x; c < n; c += 256) acc += (double)ar[c] * (double)br[c];
        }
    }
    const double tot = block_sum(acc, red);
    if (threadIdx.x == 0) part[(int64_t)blockIdx.z * gridDim.x + blockIdx.x] = (T)tot;
}

// Stage two: one workgroup per entry adds up its `parts` partial sums (thread t takes t, t + 256, ...; then the tree) and writes
// out[z] = the sum, or its square root (SQRT: the Frobenius norm).
template <typename T, bool SQRT>
__global__ __launch_bounds__(256) void dot_finish_kernel(const T* __restrict__ part, int parts, T* __restrict__ out) {
    __shared__ double red[256];
    const T* p = part + (int64_t)blockIdx.x * parts;
    double acc = 0.0;
    for (int i = threadIdx.x; i < parts; i += 256) acc += (double)p[i];
    const double tot = block_sum(acc, red);
    if (threadIdx.x == 0) out[blockIdx.x] = (T)(SQRT ? sqrt(tot) : tot);
}

// x = m / |m|_F per entry (the norm from device memory); a norm of zero (the zero matrix) gives x = 0, never 0 / 0.
template <typename T>
__global__ __launch_bounds__(256) void scale_copy_kernel(const T* __restrict__ m, int64_t ld, int64_t sm, const T* __restrict__ nrm,
                                                         T* __restrict__ x, int64_t ldx, int64_t sx, int64_t n) {
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int64_t c = (int64_t)blockIdx.x * VT + tx;
    if (c >= n) return;
    m += (int64_t)blockIdx.z * sm;
    x += (int64_t)blockIdx.z * sx;
    const T f = nrm[blockIdx.z];
    for (int i = ty; i < VT; i += 8) {
        const int64_t r = (int64_t)blockIdx.y * VT + i;
        if (r >= n) break;
        x[r * ldx + c] = f > T(0) ? m[r * ld + c] / f : T(0);
    }
}

// In place: s (n x n, what a lower-only GEMM wrote -- the entries above the diagonal are never read) becomes the FULL symmetric
// t = 3/2 I - 1/2 s.  One workgroup per tile on / below the diagonal: the tile is read by rows, kept in LDS with a pitch of 33
// elements (the transposed read walks a column; the padding breaks the power-of-two stride that would put a column on one bank), and
// written twice by rows -- where it was read and transposed into the mirrored tile.  In place is safe: a workgroup reads its own
// tile only, every read of a tile precedes the barrier, and the mirrored tile (strictly above the diagonal) is nobody's source.
template <typename T>
__global__ __launch_bounds__(256) void newton_sym_kernel(T* __restrict__ s, int64_t ld, int64_t ss, int64_t n) {
    __shared__ T tile[VT][VT + 1];
    const int bi = blockIdx.y, bj = blockIdx.x;      // source tile: rows bi, columns bj <= bi
    if (bj > bi) return;
    s += (int64_t)blockIdx.z * ss;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int i = ty; i < VT; i += 8) {
        const int64_t r = (int64_t)bi * VT + i, c = (int64_t)bj * VT + tx;
        const bool in = r < n && c <= r;
        const T v = in ? (r == c ? T(1.5) : T(0)) - T(0.5) * s[r * ld + c] : T(0);
        tile[i][tx] = v;
        if (in) s[r * ld + c] = v;
    }
    __syncthreads();
    for (int i = ty; i < VT; i += 8) {
        const int64_t r = (int64_t)bj * VT + i, c = (int64_t)bi * VT + tx;      // destination: the mirrored tile
        if (r < n && c < n && c > r) s[r * ld + c] = tile[tx][i];
    }
}

}  // namespace

// Largest order: the 32-tiles of the kernels here are grid dimensions y (<= 65535), the workspace pitch stays far below the GEMM's
// limit on the leading dimension of C (2^25), and n * ld of a workspace matrix far inside 2^63.  Largest batch: grid dimension z
// here, y in the GEMM.
#define GPK_NUCLEAR_NMAX ((int64_t)1 << 20)
#define GPK_NUCLEAR_BMAX ((int64_t)65535)

int64_t gpk_nuclear_norm_ws_elems_impl(int64_t n, int64_t batch) {
    if (n <= 0 || batch <= 0 || n > GPK_NUCLEAR_NMAX || batch > GPK_NUCLEAR_BMAX) return 0;
    return batch * (3 * n * ws_ld(n) + red_parts(n) + 1);
}

// ws: [Xa | Xb | S | part | nrm] -- three blocks of `batch` n x ldw matrices, batch * parts partial sums, batch norms.
//   nrm = |m|_F                                            (dot_partial_kernel on (m, m), dot_finish_kernel with the root)
//   Xa  = m / nrm                                          (scale_copy_kernel)
//   per step:  S = lower(X^T X)                            (GEMM, LOWER: both operands are X, stored K x M)
//              S = T = 3/2 I - 1/2 S, full                 (newton_sym_kernel)
//              X' = X T                                    (GEMM: X stored M x K; T, symmetric, read as N x K) into the other X buffer
//   out = sum_ij X_ij m_ij                                 (dot_partial_kernel on (X, m), dot_finish_kernel)
template <typename T>
int gpk_nuclear_norm_launch(const T* m, int64_t n, int64_t ld, int64_t sm, int64_t batch, int iters, T* out, T* ws, hipStream_t stream) {
    if (n <= 0 || batch <= 0) return GPK_OK;
    if (m == nullptr) return GPK_ERR_ARG(2);
    if (n > GPK_NUCLEAR_NMAX) return GPK_ERR_ARG(3);
    if (ld < n) return GPK_ERR_ARG(4);
    if (sm < 0) return GPK_ERR_ARG(5);
    if (batch > GPK_NUCLEAR_BMAX) return GPK_ERR_ARG(6);
    if (iters < 1) return GPK_ERR_ARG(7);
    if (out == nullptr) return GPK_ERR_ARG(8);
    if (ws == nullptr) return GPK_ERR_ARG(9);
    const int64_t ldw = ws_ld(n), sw = n * ldw;
    const int parts = (int)red_parts(n);
    T* X = ws;
    T* Y = ws + batch * sw;
    T* S = ws + 2 * batch * sw;
    T* part = ws + 3 * batch * sw;
    T* nrm = part + batch * parts;
    const unsigned t = (unsigned)gpk_cdiv(n, VT);
    const dim3 grid(t, t, (unsigned)batch), rgrid((unsigned)parts, 1, (unsigned)batch);
    hipLaunchKernelGGL((dot_partial_kernel<T>), rgrid, dim3(256), 0, stream, m, ld, sm, m, ld, sm, n, part);
    GPK_CHECK_LAUNCH();
    hipLaunchKernelGGL((dot_finish_kernel<T, true>), dim3((unsigned)batch), dim3(256), 0, stream, (const T*)part, parts, nrm);
    GPK_CHECK_LAUNCH();
    hipLaunchKernelGGL((scale_copy_kernel<T>), grid, dim3(256), 0, stream, m, ld, sm, (const T*)nrm, X, ldw, sw, n);
    GPK_CHECK_LAUNCH();
    for (int it = 0; it < iters; ++it) {
        int st = gpk_gemm_launch<T>(false, false, n, n, n, T(1), X, ldw, sw, X, ldw, sw, T(0), S, ldw, sw, batch, GPK_GEMM_LOWER, stream);
        if (st) return st == GPK_ERR_LAUNCH ? st : GPK_ERR_ARG(3);
        hipLaunchKernelGGL((newton_sym_kernel<T>), grid, dim3(256), 0, stream, S, ldw, sw, n);
        GPK_CHECK_LAUNCH();
        st = gpk_gemm_launch<T>(true, true, n, n, n, T(1), X, ldw, sw, S, ldw, sw, T(0), Y, ldw, sw, batch, 0, stream);
        if (st) return st == GPK_ERR_LAUNCH ? st : GPK_ERR_ARG(3);
        T* tmp = X; X = Y; Y = tmp;
    }
    hipLaunchKernelGGL((dot_partial_kernel<T>), rgrid, dim3(256), 0, stream, (const T*)X, ldw, sw, m, ld, sm, n, part);
    GPK_CHECK_LAUNCH();
    hipLaunchKernelGGL((dot_finish_kernel<T, false>), dim3((unsigned)batch), dim3(256), 0, stream, (const T*)part, parts, out);
    GPK_CHECK_LAUNCH();
    return GPK_OK;
}

#define GPK_INST(T) \
    template int gpk_nuclear_norm_launch<T>(const T*, int64_t, int64_t, int64_t, int64_t, int, T*, T*, hipStream_t);
GPK_INST(double)
GPK_INST(float)
#undef GPK_INST
