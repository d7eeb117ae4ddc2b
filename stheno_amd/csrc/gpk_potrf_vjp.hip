// gpk_potrf_vjp.hip -- the vector-Jacobian product of the Cholesky factorisation A = L L^T (gpk_potrf_vjp in include/gpk.h):
//   abar = W^T Psym W,   W = L^{-1},   Psym = 1/2 (P + P^T),   P = Phi(L^T tril(lbar)),   Phi = lower triangle, diagonal halved.
// Everything cubic runs on the MFMA GEMM with its triangular flags and on gpk_trtri_lower; the kernels here are the quadratic
// glue: clean lower-triangular copies of the two inputs (the GEMM's TRI_K flag skips whole k-chunks, so the diagonal tiles must read
// zeros above the diagonal -- the caller's strict upper triangles are garbage by contract), and Phi + the half-sum into a full
// symmetric matrix (one tiled transposed read through LDS).  The final mirror is gpk_symmetrize: a copy, so abar == abar^T bit
// for bit.  No atomics, fixed launch sequence: the same bits on every call.
#include "gpk_common.hpp"

namespace {

constexpr int VT = 32;     // tile edge of the two kernels: 32 x 32 elements, 256 threads as 32 x 8

// dst = tril(src): the lower triangle copied, the strict upper triangle ZEROED; nothing above the diagonal of src is read.
template <typename T>
__global__ __launch_bounds__(256) void tril_copy_kernel(const T* __restrict__ src, int64_t lds, T* __restrict__ dst, int64_t ldd, int64_t n) {
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int64_t c = (int64_t)blockIdx.x * VT + tx;
    if (c >= n) return;
    for (int i = ty; i < VT; i += 8) {
        const int64_t r = (int64_t)blockIdx.y * VT + i;
        if (r >= n) break;
        dst[r * ldd + c] = (c <= r) ? src[r * lds + c] : T(0);
    }
}

// out = 1/2 (Phi(p) + Phi(p)^T), full and symmetric, from the LOWER triangle of p (n x n; what a lower-only GEMM wrote -- the entries
// above the diagonal are never read):  out[r][c] = out[c][r] = p[r][c] / 2 for c <= r  (Phi halves the diagonal, the half-sum of the
// two triangles halves everything else).  One workgroup per tile on / below the diagonal: the tile is read by rows (coalesced), kept
// in LDS with a pitch of 33 elements (the transposed read walks a column: one access width of padding per row breaks the power-of-two
// stride that would put a column on one bank), and written twice, by rows both times -- as it is and transposed into the mirrored tile.
template <typename T>
__global__ __launch_bounds__(256) void phi_sym_kernel(const T* __restrict__ p, int64_t ldp, T* __restrict__ out, int64_t ldo, int64_t n) {
    __shared__ T tile[VT][VT + 1];
    const int bi = blockIdx.y, bj = blockIdx.x;      // source tile: rows bi, columns bj <= bi
    if (bj > bi) return;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int i = ty; i < VT; i += 8) {
        const int64_t r = (int64_t)bi * VT + i, c = (int64_t)bj * VT + tx;
        const T v = (r < n && c <= r) ? p[r * ldp + c] * T(0.5) : T(0);
        tile[i][tx] = v;
        if (r < n && c <= r) out[r * ldo + c] = v;
    }
    __syncthreads();
    for (int i = ty; i < VT; i += 8) {
        const int64_t r = (int64_t)bj * VT + i, c = (int64_t)bi * VT + tx;      // destination: the mirrored tile
        if (r < n && c < n && c > r) out[r * ldo + c] = tile[tx][i];
    }
}

static inline int64_t ws_ld(int64_t n) { return gpk_cdiv(n, 16) * 16; }      // rows of the workspace matrices stay 16-byte aligned

}  // namespace

// Largest order: the 32-tiles of the kernels here and of gpk_symmetrize are grid dimensions y (<= 65535), and n * ld of a
// workspace matrix stays far inside 2^63.
#define GPK_POTRF_VJP_NMAX ((int64_t)1 << 20)

int64_t gpk_potrf_vjp_ws_elems_impl(int64_t n, int sb) {
    if (n <= 0 || !gpk_valid_sb(sb)) return 0;
    return 3 * n * ws_ld(n) + (int64_t)sb * n;
}

// ws: [Lc | Bc | X | tmp], three n x ldw matrices and the sb * n elements of gpk_trtri_lower's scratch.
//   Lc = tril(l), Bc = tril(lbar)                          (two copies)
//   X  = lower(Lc^T Bc)                                    (GEMM, LOWER | TRI_K: both operands are stored K x M and vanish for k < row)
//   Lc = Psym = 1/2 (Phi(X) + Phi(X)^T)                    (phi_sym_kernel)
//   Bc = W = L^{-1}                                        (gpk_trtri_lower: reads l below its sb-blocks only, the blocks through dinv_sb)
//   X  = W^T Psym                                          (GEMM, TRI_K: A = W is stored K x M and vanishes for k < row)
//   abar = lower(W^T X^T) = lower(W^T Psym W)              (GEMM, LOWER | TRI_K)
//   abar's upper triangle = the mirror                     (gpk_symmetrize)
template <typename T>
int gpk_potrf_vjp_launch(const T* l, int64_t n, int64_t ld, const T* dinv_sb, int sb, const T* lbar, int64_t ldlb, T* abar, int64_t lda,
                         T* ws, hipStream_t stream) {
    if (n <= 0) return GPK_OK;
    if (l == nullptr) return GPK_ERR_ARG(2);
    if (n > GPK_POTRF_VJP_NMAX) return GPK_ERR_ARG(3);
    if (ld < n) return GPK_ERR_ARG(4);
    if (dinv_sb == nullptr) return GPK_ERR_ARG(5);
    if (!gpk_valid_sb(sb)) return GPK_ERR_ARG(6);
    if (lbar == nullptr) return GPK_ERR_ARG(7);
    if (ldlb < n) return GPK_ERR_ARG(8);
    if (abar == nullptr) return GPK_ERR_ARG(9);
    if (lda < n) return GPK_ERR_ARG(10);
    if (ws == nullptr) return GPK_ERR_ARG(11);
    const int64_t ldw = ws_ld(n);
    T* Lc = ws;
    T* Bc = ws + n * ldw;
    T* X = ws + 2 * n * ldw;
    T* tmp = ws + 3 * n * ldw;
    const unsigned t = (unsigned)gpk_cdiv(n, VT);
    const dim3 grid(t, t);
    hipLaunchKernelGGL((tril_copy_kernel<T>), grid, dim3(256), 0, stream, l, ld, Lc, ldw, n);
    GPK_CHECK_LAUNCH();
    hipLaunchKernelGGL((tril_copy_kernel<T>), grid, dim3(256), 0, stream, lbar, ldlb, Bc, ldw, n);
    GPK_CHECK_LAUNCH();
    int st = gpk_gemm_launch<T>(false, false, n, n, n, T(1), Lc, ldw, 0, Bc, ldw, 0, T(0), X, ldw, 0, 1, GPK_GEMM_LOWER | GPK_GEMM_TRI_K, stream);
    if (st) return st == GPK_ERR_LAUNCH ? st : GPK_ERR_ARG(3);
    hipLaunchKernelGGL((phi_sym_kernel<T>), grid, dim3(256), 0, stream, X, ldw, Lc, ldw, n);
    GPK_CHECK_LAUNCH();
    st = gpk_trtri_launch<T>(l, n, ld, dinv_sb, sb, Bc, ldw, tmp, stream);
    if (st) return st == GPK_ERR_LAUNCH ? st : GPK_ERR_ARG(3);
    st = gpk_gemm_launch<T>(false, true, n, n, n, T(1), Bc, ldw, 0, Lc, ldw, 0, T(0), X, ldw, 0, 1, GPK_GEMM_TRI_K, stream);
    if (st) return st == GPK_ERR_LAUNCH ? st : GPK_ERR_ARG(3);
    st = gpk_gemm_launch<T>(false, true, n, n, n, T(1), Bc, ldw, 0, X, ldw, 0, T(0), abar, lda, 0, 1, GPK_GEMM_LOWER | GPK_GEMM_TRI_K, stream);
    if (st) return st == GPK_ERR_LAUNCH ? st : GPK_ERR_ARG(10);      // (the GEMM's own limit on the leading dimension of C)
    st = gpk_symmetrize_launch<T>(abar, n, lda, 0, 1, stream);
    if (st) return st == GPK_ERR_LAUNCH ? st : GPK_ERR_ARG(3);
    return GPK_OK;
}

#define GPK_INST(T)                                                                                                            \
    template int gpk_potrf_vjp_launch<T>(const T*, int64_t, int64_t, const T*, int, const T*, int64_t, T*, int64_t, T*, hipStream_t);
GPK_INST(double)
GPK_INST(float)
#undef GPK_INST
