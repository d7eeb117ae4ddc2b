/* gpk.h -- C ABI of libgpk.so: the MI355X (gfx950) kernels behind the dense
 * Gaussian-process inference hot path of wesselb/stheno.
 *
 * The reference is pure Python; its arithmetic for this path lives in the
 * un-vendored packages `mlkernels` (kernel evaluation), `matrix` and `lab`
 * (Cholesky / triangular solves / reductions, dispatched to LAPACK).  Each
 * entry point below replaces the op named in its comment at the reference
 * call site given as file:line (paths relative to the reference repository).
 * INTEGRATION.md shows the ctypes binding a maintainer would add.
 *
 * Conventions
 *  - All matrices are ROW-MAJOR with a leading dimension `ld*` in ELEMENTS.
 *  - `batch` independent problems are laid out with a stride `s*` in ELEMENTS
 *    (stheno's batched computation: README.md:744-766, random.py:261,274).
 *  - Every pointer named x/y/a/b/l/out/... is a DEVICE pointer owned by the
 *    caller; term descriptors (`kinds`, `variances`, `inv_ls`, `shapes`) are HOST arrays of `nterms` entries.
 *  - `dtype`: GPK_F32 or GPK_F64; all device buffers of a call share it.
 *  - `stream` is a hipStream_t passed as void*.  Calls only ENQUEUE work: no
 *    device allocation, no free, no host synchronisation, no retained pointers.
 *    Process-wide state is limited to: one helper stream (CU-masked to one CU per XCD) +
 *    events per device that gpk_potrf_la / gpk_init create on first use (fork/join around
 *    the caller's stream, serialised by a mutex; that first use allocates 36 bytes for a
 *    moment and synchronises once), the cached CU count per device, the tuning knobs of gpk_tune and the
 *    opt-in measurement hooks gpk_prof_*.  Everything else is thread-safe for distinct
 *    streams/buffers.
 *  - Return value: 0 on success; -k if argument k (1-based) is invalid;
 *    GPK_ERR_LAUNCH if a kernel launch failed.  No C++ exception crosses the ABI.
 */
#ifndef GPK_H
#define GPK_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GPK_F32 0
#define GPK_F64 1

#define GPK_OK 0
#define GPK_ERR_LAUNCH (-100)

/* kernel term kinds; one term = variance * kappa(dist(x, y) * inv_ls)   (GPK_K_RQ, GPK_K_DELTA: kappa also takes a SHAPE parameter,
 * shapes[t]; a term table with such a kind is "shaped") */
#define GPK_K_EQ 0        /* exp(-r^2/2)                        mlkernels.EQ        */
#define GPK_K_MATERN12 1  /* exp(-r)                            mlkernels.Exp       */
#define GPK_K_MATERN32 2  /* (1+sqrt3 r) exp(-sqrt3 r)          mlkernels.Matern32  */
#define GPK_K_MATERN52 3  /* (1+sqrt5 r+5r^2/3) exp(-sqrt5 r)   mlkernels.Matern52  */
#define GPK_K_LINEAR 4    /* <x, y>                             mlkernels.Linear    */
#define GPK_K_CONST 5     /* 1                                  mlkernels.OneKernel */
#define GPK_K_RQ 6        /* (1 + r^2/(2 alpha))^(-alpha)       mlkernels.RQ(alpha): shape = alpha > 0, see gpk_kmat */
#define GPK_K_DELTA 7     /* 1 if r^2 < epsilon, else 0         mlkernels.Delta(epsilon): shape = epsilon > 0, see gpk_kmat */
#define GPK_MAX_TERMS 8

#define GPK_GEMM_LOWER 1
#define GPK_GEMM_TRI_K 2
#define GPK_GEMM_TRI_K_LOWER 4
#define GPK_GEMM_TRI_K_LOWER_B 8
/* bit 4 (16), no name: the in-place panel solve of gpk_potrf -- B (n <= 128 rows, k-major) is lower triangular from column 0 and the multiply-adds right of its diagonal are skipped per 16-column fragment */

#define GPK_DIAG_BLOCK 128 /* order of the diagonal blocks whose inverses gpk_potrf leaves in `dinv` */

/* 104: the four entries that take a term table take `shapes` behind `inv_ls`; their `_s` twins of versions 102-103 are retired in version 104.
 * 105: gpk_kmat_diff.  106: gpk_kmat_diff_vjp.  107: gpk_kmat_batch_terms, gpk_kdiag_batch_terms.
 * 108: gpk_kmat_vjp_dense_batch, gpk_kmat_vjp_dense_batch_grid.
 * 109: gpk_kmat_scaled.  110: gpk_potrf_vjp.  111: gpk_nuclear_norm.  112: gpk_potrf_border. */
int gpk_version(void);

/* Optional: create the per-device helper stream of gpk_potrf_la now (current device) instead of at its first
 * call -- it costs one stream creation, a 64-workgroup census kernel and ONE host synchronisation, which must
 * not happen inside a stream capture. */
int gpk_init(void);

/* Destroy the helper streams and events again (idempotent; they are re-created on demand).  Call it before the process
 * exits (the Python binding registers it with atexit): a CU-masked stream that is still alive at exit can crash the
 * teardown of the runtime / of a profiler wrapped around the process. */
void gpk_shutdown(void);

/* Kernel matrix  out[i][j] (+)= sum_t variances[t] * kappa_kinds[t](x_i, y_j; inv_ls[t], shapes[t])
 * and, if `symmetric` (x and y are the same points), + diag_add + diag_vec[i] on i == j.
 * Replaces mlkernels `pairwise` + `B.add(K, noise)`:  stheno/model/fdd.py:79,
 * stheno/model/observations.py:139 (K_x), :285-286 (K_zx, K_z).
 *   x: n x d (ldx), y: m x d (ldy), out: n x m (ld).  lower_only: skip tiles above the diagonal.
 *   diag_vec: nullable, n values per batch (stride s_diag).  accumulate: out += instead of out =.
 *   shapes: read for the kinds that have a shape parameter (GPK_K_RQ: alpha, GPK_K_DELTA: epsilon) and ignored for the others; may be
 *   NULL exactly when no term is GPK_K_RQ or GPK_K_DELTA.  A term table without such a kind writes the same bits whatever `shapes` holds.
 *   Returns -4 for nterms outside 0 .. GPK_MAX_TERMS, -1 for an unknown kind or a shaped kind with shapes == NULL, -5 for a shape <= 0.
 *   Numerics: squared distances from direct differences (no |x|^2 + |y|^2 - 2 x.y cancellation); exp and sqrt are the library's own
 *   branch-free device routines -- every value within ~2.5 eps (1 + |argument of the exponential|) of the exactly rounded one for the
 *   given inputs (measured element by element against an 80-bit reference: csrc/selftest.cpp, `kmat_* elementwise`); NaN inputs give
 *   NaN values; the distance of a point to itself is exactly 0 (sqrt(0) is evaluated as 1e-140 in fp64).
 *   GPK_K_RQ is evaluated as exp(-alpha log1p(q / (2 alpha))), q = r^2 / scale^2: a single RQ term has a row-band program of its own
 *   next to EQ / Matern; within ~2.5 eps (1 + alpha log1p(q / (2 alpha))) of the exactly rounded value (csrc/selftest.cpp, `--rq`).
 *   GPK_K_DELTA: with q = r^2 / scale^2 (direct differences) the value is 1 where q < epsilon and 0 elsewhere -- no transcendental, so
 *   coincident points give exactly the variance and every element is exact in both dtypes unless q lies within rounding of epsilon;
 *   NaN inputs give NaN.  A Delta term always takes the term-table program of the shaped launches (csrc/selftest.cpp, `--delta`):
 *   mlkernels `Delta(epsilon)`, the noise process e of `y = f + e`. */
int gpk_kmat(int dtype, const int* kinds, const double* variances, const double* inv_ls, const double* shapes, int nterms,
             const void* x, int64_t n, int64_t ldx, int64_t sx, const void* y, int64_t m, int64_t ldy,
             int64_t sy, int d, void* out, int64_t ld, int64_t so, int64_t batch, int lower_only,
             int symmetric, double diag_add, const void* diag_vec, int64_t s_diag, int accumulate,
             void* stream);

/* gpk_kmat with a ROW FACTOR and a COLUMN FACTOR applied at the store:
 *   out[b][i][j] (+)= row_scale[b * s_rs + i] * col_scale[b * s_cs + j] * sum_t variances[t] * kappa_kinds[t](x[b]_i, y[b]_j)
 * and, on i == j of a symmetric launch, + diag_add + diag_vec[i], UNSCALED, as in gpk_kmat.  The kernel of a process times a function,
 * fn(x) k(x, y) fn(y), and its one-sided cross-kernels: replaces mlkernels `k * TensorProductKernel(fn)` behind `GP.__mul__`,
 * stheno/model/measure.py:242-251.  A sum  fn k_a fn + k_b  is one gpk_kmat launch and one accumulating launch of this entry into the same
 * buffer: no n x m temporary for the scaled summand.
 *   row_scale: n values per batch entry, col_scale: m values; DEVICE pointers, unit stride, the launch's dtype.  s_rs, s_cs: batch strides in
 *   elements; 0 shares one vector among the entries.  Either pointer may be NULL: all ones, no multiplication.  With both NULL the entry
 *   IS gpk_kmat (the unscaled kernels: gpk_kmat's bits).
 *   Every other argument is gpk_kmat's, with gpk_kmat's meaning, checks and return codes.  gpk_kmat's codes (-1, -4, -5, -6, -13) stand
 *   for arguments in front of the four new ones, so none of them shifts; the scales have no code of their own (they cannot be checked
 *   on the host).  An empty problem (n, m or batch <= 0) returns 0.
 *   Value contract (csrc/selftest.cpp `--scaled`, tests/test_kmat_scaled_gpu.py):
 *    - the launch takes the program and the launch plan gpk_kmat takes for the same arguments -- the single-kind EQ / Matern / RQ
 *      programs, EQ + Linear, the generic and the shaped term table, the packed fp32 path, the fp64 table exponential, the row-band walk
 *      for d <= 8, the one-tile kernel beyond, the compact lower-triangle grid -- so with p the value gpk_kmat computes, an element is
 *      fl(fl(p * rs_i) * cs_j): the bits of the two multiplications applied to gpk_kmat's output.  A missing scale skips its multiplication;
 *    - the diagonal addition and the accumulate follow as in gpk_kmat; their add may fuse with the last multiplication (one rounding
 *      instead of two);
 *    - a NaN scale gives NaN in its row or column only; a zero scale gives exact zeros where p is finite.
 *   rs of a row is wave-uniform (the row-band kernel stages a band's 32 values in LDS beside its x rows, the one-tile kernel loads it as
 *   a uniform value), cs of a lane's columns is one small load per column tile, fetched with the next tile's y values.  There is no
 *   per-batch-term-table form. */
int gpk_kmat_scaled(int dtype, const int* kinds, const double* variances, const double* inv_ls, const double* shapes, int nterms,
                    const void* x, int64_t n, int64_t ldx, int64_t sx, const void* y, int64_t m, int64_t ldy, int64_t sy, int d,
                    const void* row_scale, int64_t s_rs, const void* col_scale, int64_t s_cs,
                    void* out, int64_t ld, int64_t so, int64_t batch, int lower_only, int symmetric,
                    double diag_add, const void* diag_vec, int64_t s_diag, int accumulate, void* stream);

/* Derivative blocks of the kernel matrix: dim_x >= 0 differentiates w.r.t. x[:, dim_x], dim_y >= 0 w.r.t. y[:, dim_y]; -1: not.
 * At least one of them is >= 0 (both -1: the argument error for dim_x -- gpk_kmat is the call for that).
 *   out[i][j] (+)= d/dx_i[a] k(x_i, y_j)   |   d/dy_j[b] k(x_i, y_j)   |   d^2/dx_i[a] dy_j[b] k(x_i, y_j),      k = sum_t variances[t] kappa_t
 * -- the covariance of a process with its derivative and of two derivatives.  Replaces mlkernels `DerivativeKernel` (autodiff through
 * `pairwise`) behind `GP.diff`: stheno/model/measure.py:343-360 (mean, kernel and left rule of the derivative process).
 * Everything from `x` on is gpk_kmat's argument list with gpk_kmat's meaning (leading dimensions, batch strides, lower_only,
 * diag_add / diag_vec on i == j of a symmetric launch, accumulate).
 *   Formulas.  A stationary term is v kappa(q), q = c |x - y|^2, c = inv_ls^2; with D_a = x[a] - y[a]:
 *     d/dx_a = 2 c v kappa'(q) D_a,    d/dy_b = -2 c v kappa'(q) D_b,    d^2/dx_a dy_b = v (-4 c^2 kappa''(q) D_a D_b - 2 c kappa'(q) [a == b])
 *     GPK_K_EQ         kappa' = -kappa / 2                        kappa'' = kappa / 4
 *     GPK_K_RQ         kappa' = -(1 + u)^(-alpha - 1) / 2         kappa'' = (alpha + 1) / (4 alpha) (1 + u)^(-alpha - 2),  u = q / (2 alpha)
 *     GPK_K_MATERN52   kappa' = -(5/6) (1 + s) e^(-s)             kappa'' = (25/12) e^(-s),                                 s = sqrt(5 q)
 *     GPK_K_MATERN32   kappa' = -(3/2) e^(-s)                     kappa'' = 9 / (4 s) e^(-s),                               s = sqrt(3 q)
 *     GPK_K_LINEAR (c v <x, y>):  d/dx_a = c v y[a],   d/dy_b = c v x[b],   d^2/dx_a dy_b = c v [a == b];      GPK_K_CONST: 0.
 *   RQ's powers are exp(-(alpha + 1) log1p(u)) and exp(-(alpha + 2) log1p(u)): every exponent on this path is <= 0, as in gpk_kmat.
 *   Matern32's kappa'' D_a D_b tends to 0 with the distance (|D_a D_b| <= |x - y|^2): at coincident points the second derivative is
 *   exactly -2 c v kappa'(0) [a == b] and the one-sided derivatives of every stationary table are exactly 0, in both dtypes; NaN inputs
 *   give NaN values in their row / column only.  GPK_K_MATERN12 and GPK_K_DELTA are not differentiable and are refused.
 *   Numerics: squared distances and D_a, D_b from direct differences; element by element within a few eps of
 *   sum_t |v_t| (|first addend| + |second addend|) (1 + |argument of the exponential|) (csrc/selftest.cpp, `--diff`; tests/test_diff_gpu.py).
 *   Two launch shapes like gpk_kmat: the row-band walk for d <= 8, the chunked one-tile kernel beyond; one term-table program.
 *   Every argument is checked before an empty problem (n, m or batch <= 0) returns 0.  Returns -k for argument k:
 *     -6  nterms outside 0 .. GPK_MAX_TERMS;      -2  a kind without a derivative (GPK_K_MATERN12, GPK_K_DELTA) or an unknown kind;
 *     `shapes` exactly as for gpk_kmat (it may be NULL exactly when no term is GPK_K_RQ): -1 for a GPK_K_RQ term with shapes == NULL -- the
 *         one code here that is no argument position, kept equal to the sibling entry's --, -5 for an alpha <= 0;
 *     -17 d < 0;      -7  dim_x outside [-1, d), or dim_x and dim_y both -1;      -8  dim_y outside [-1, d);
 *     -23 `symmetric` or `lower_only` set although dim_x != dim_y or one of them is -1 (the one-sided blocks are not symmetric, and the
 *         mixed block of two different dimensions is not either);
 *     -10 / -14 / -21  n (more than 2^31 - 1 rows, or more than 65535 row tiles of 32), m, batch (> 65535) too large. */
int gpk_kmat_diff(int dtype, const int* kinds, const double* variances, const double* inv_ls, const double* shapes, int nterms,
                  int dim_x, int dim_y, const void* x, int64_t n, int64_t ldx, int64_t sx, const void* y, int64_t m, int64_t ldy,
                  int64_t sy, int d, void* out, int64_t ld, int64_t so, int64_t batch, int lower_only,
                  int symmetric, double diag_add, const void* diag_vec, int64_t s_diag, int accumulate,
                  void* stream);

/* Kernel diagonal  out[i] = k(x_i, x_i).  Replaces mlkernels `elwise`:
 * stheno/model/fdd.py:66, stheno/model/observations.py:304.
 * `shapes` as for gpk_kmat, with the same return codes (-4, -1 for a shaped kind with shapes == NULL, -5 for a shape <= 0; kinds are
 * not range-checked): an RQ or Delta term contributes its variance on the diagonal, whatever its shape. */
int gpk_kdiag(int dtype, const int* kinds, const double* variances, const double* inv_ls, const double* shapes, int nterms,
              const void* x, int64_t n, int64_t ldx, int64_t sx, int d, void* out, int64_t so,
              int64_t batch, void* stream);

/* gpk_kmat with ONE TERM TABLE PER BATCH ENTRY: entry b is gpk_kmat's result for x[b], y[b] with the parameters of row b,
 *   out[b][i][j] (+)= sum_t variances[b * s_terms + t] * kappa_kinds[t](x[b]_i, y[b]_j; inv_ls[b * s_terms + t], shapes[b * s_terms + t]).
 * `kinds` stays a HOST array of nterms entries: the structure of the kernel is shared by the batch.  `variances`, `inv_ls` and `shapes`
 * are DEVICE pointers to fp64 tables of `batch` rows of nterms values, s_terms (>= nterms, in elements) apart; `shapes` may be NULL
 * exactly when no term is GPK_K_RQ or GPK_K_DELTA, and is read for those kinds alone.  Nothing is read back and nothing synchronises.
 * Every other argument is gpk_kmat's, with gpk_kmat's meaning.
 *   The workgroups of entry b load row b with uniform loads and derive what gpk_kmat derives on the host, in the same precision and
 *   order (inv_ls^2 and 1 / (2 alpha) in fp64, then rounded to the dtype), once per workgroup; then they run the program gpk_kmat
 *   selects for the same kinds (the single-kind EQ / Matern / RQ programs, EQ + Linear, the generic and the shaped term table) on the
 *   same launch shape.  Entry b therefore holds the bits gpk_kmat writes for x[b], y[b] and row b's parameters (tests/test_batch_terms_gpu.py).
 *   The values in device memory cannot be checked on the host: an inverse scale that is NaN, an RQ alpha <= 0 (its logarithm's argument
 *   is negative or its exponent positive) or a NaN anywhere in a row gives NaN or Inf values in THAT BATCH ENTRY only; a Delta
 *   epsilon <= 0 gives a term that is 0 everywhere.  gpk_kmat's -5 (a shape <= 0) is therefore never returned.
 *   Returns, checked in this order behind the empty problem (n, m or batch <= 0: 0): -4 for nterms outside 0 .. GPK_MAX_TERMS,
 *   -6 for n, m (more than 2^31 - 1, or more than 65535 row tiles of 32) or batch (> 65535) too large, -13 for d < 0, -1 for an unknown kind
 *   or a shaped kind with shapes == NULL, -3 for variances == NULL or inv_ls == NULL with nterms > 0, -7 for s_terms < nterms. */
int gpk_kmat_batch_terms(int dtype, const int* kinds, const double* variances, const double* inv_ls, const double* shapes, int nterms,
                         int64_t s_terms, const void* x, int64_t n, int64_t ldx, int64_t sx, const void* y, int64_t m, int64_t ldy,
                         int64_t sy, int d, void* out, int64_t ld, int64_t so, int64_t batch, int lower_only,
                         int symmetric, double diag_add, const void* diag_vec, int64_t s_diag, int accumulate,
                         void* stream);

/* gpk_kdiag with one term table per batch entry (tables as for gpk_kmat_batch_terms):
 *   out[b][i] = sum_t variances[b * s_terms + t] * (kinds[t] == GPK_K_LINEAR ? |x[b]_i|^2 inv_ls[b * s_terms + t]^2 : 1).
 * Returns -4, -1 (a shaped kind with shapes == NULL; kinds are not range-checked, as in gpk_kdiag), -3 and -7 as above, -6 for
 * batch > 65535. */
int gpk_kdiag_batch_terms(int dtype, const int* kinds, const double* variances, const double* inv_ls, const double* shapes, int nterms,
                          int64_t s_terms, const void* x, int64_t n, int64_t ldx, int64_t sx, int d, void* out, int64_t so,
                          int64_t batch, void* stream);

/* Number of elements of the `dinv` workspace gpk_potrf needs per batch entry. */
int64_t gpk_dinv_elems(int64_t n);

/* In-place lower Cholesky  A = L L^T  (only the lower triangle is read and written; the
 * strict upper triangle is left untouched: use gpk_tril for a clean factor).  `dinv` receives inv(L_cc) of every 128x128
 * diagonal block ([batch][ceil(n/128)][128][128], identity-padded); `info`
 * (int per batch entry, MUST be zeroed by the caller) receives the LAPACK-style
 * order of the first non-positive pivot, 0 if none.  nbo: outer block of the right-looking
 * sweep (128 * 2^k; <= 0 selects the default -- one matrix: the whole matrix up to n = 4096, else 1024; batches: 1024 for
 * n >= 8192, 512 for n >= 2048, else 256).
 * ONE matrix (batch == 1) is factorised panel by panel with ONE launch per panel of nbo columns (+ a memset of its control words,
 * which live in a `dinv` slot the panel does not write): a chain workgroup factorises and inverts the diagonal blocks, the other
 * workgroups take the solves and updates of the panel as tasks and wait for each other through flag words in device memory
 * (gpk_potrf.hip, potrf_pipe_kernel; the task list is deadlock-free whatever part of the grid is resident).  A workgroup that
 * waited for seconds gives up and makes all others leave: `info` = -1 then (never observed; the factor is unusable).
 * BATCHES of at least 64 fp32 matrices whose order is a multiple of 128 (from 512 on; 16-byte aligned, on a stream without a CU
 * mask) take one launch for the diagonal blocks and ONE mixed-phase launch for everything below them per 128-column step
 * (gpk_potrf.hip, batch_mix_kernel: panel solves and update tiles of different matrices share the CUs; per-matrix counters in the
 * next `dinv` slot order them, without fences -- every task of a matrix runs on the XCD the matrix is pinned to).  That placement is
 * checked on the device: a violation is reported as `info` = -2 for one of the batch's matrices (never observed; the factors are
 * unusable).  Same arithmetic in the same order per entry as the lockstep launches other batches take: bit-identical factors.
 * Replaces `B.cholesky(B.reg(K))` (LAPACK potrf): implicit under B.logdet / B.iqf_diag at
 * stheno/random.py:274-276, explicit at stheno/model/observations.py:300. */
int gpk_potrf(int dtype, void* a, int64_t n, int64_t ld, int64_t sa, int64_t batch, void* dinv,
              int* info, int nbo, void* stream);

/* The same factorisation for ONE large matrix with LOOK-AHEAD: outer blocks of `nb` columns (256 ... 4096,
 * a power of two); the serial panel chain of outer step j+1 (diagonal-block factorisations) runs on a helper
 * stream, on CUs the persistent trailing-update kernel of step j leaves empty, and the rows below each diagonal
 * block are solved by ONE GEMM with the explicit inverse of the nb x nb diagonal block.  Results as gpk_potrf, plus
 * `dinv_nb` = [ceil(n/nb)][nb][nb], the inverses of the nb x nb diagonal blocks of L -- exactly what
 * gpk_trtri_merge(sb = nb) would produce, so the solves below can take them as they are.
 * `ws`: gpk_potrf_la_ws_elems(n, nb) elements of scratch.  `info` as for gpk_potrf (one int, zeroed by the caller).
 * The helper stream is forked from / joined to `stream` with events; under stream capture it joins the capture. */
/* gpk_potrf with ONE right-hand side per matrix solved along (round 6): `b` holds batch vectors of n entries (unit stride, sb elements
 * apart), overwritten by L^{-1} b -- what gpk_trsv_lower(l, ..., sb = 128, nrhs = 1) would compute behind the factorisation.
 * Batches that take the mixed-phase steps (fp32, >= 64 aligned matrices) do the sweep inside those steps: the diagonal-block launch
 * of each 128-column step turns that block of b into inv(L_jj) b_j, and every solve tile of the step subtracts its 128 x 128 tile of
 * L times that block from its own 128 entries of b, reading back the tile it has just stored -- no separate pass over the factor.
 * Every other shape factorises, then sweeps with gpk_trsv_lower (sb = 128) on `stream`.
 * `tmp`: batch * 128 + GPK_TRSV_CTRL_ELEMS elements; dinv as for gpk_potrf (required).
 * Replaces `B.cholesky` + the solve inside `B.iqf_diag(K, y - m)`: stheno/random.py:272-279 (batched: tests/model/test_cases.py:134-176). */
int gpk_potrf_rhs(int dtype, void* a, int64_t n, int64_t ld, int64_t sa, int64_t batch, void* dinv, int* info, int nbo, void* b, int64_t sb,
                  void* tmp, void* stream);

int64_t gpk_potrf_la_ws_elems(int64_t n, int nb);
int gpk_potrf_la(int dtype, void* a, int64_t n, int64_t ld, void* dinv, void* dinv_nb, int nb, void* ws, int* info,
                 void* stream);
/* The same with explicit inverses NARROWER than the outer blocks: `sb` (256 ... nb, a power of two) wide.  The rows below an nb-block
 * are then solved by block substitution over its nb / sb column blocks (same flops, 2 nb / sb - 1 GEMMs instead of one) and `dinv_sb` =
 * [ceil(n/sb)][sb][sb] is what gpk_trtri_merge(sb) would produce.  For fp32: the error of everything solved against an explicit inverse
 * grows with its width (posterior mean of configs[2] at N = 32768 against fp64: 1.0e-3 with 1024-wide inverses, 7e-4 with 512), while
 * the factorisation is fastest with 1024-column outer blocks. */
int gpk_potrf_la_split(int dtype, void* a, int64_t n, int64_t ld, void* dinv, void* dinv_sb, int nb, int sb, void* ws, int* info,
                       void* stream);

/* Factorisation WITH ROWS UNDER THE MATRIX (round 5): `a` holds `rows` >= n rows of n columns -- the symmetric matrix (lower
 * triangle read) in the first n, anything else below, typically K(x*, x) of the posterior.  The extra rows are carried through
 * the factorisation like the rows below a diagonal block: every panel solve and every trailing update includes them, and they
 * come out as  a[n:, :] L^{-T}  -- the TRANSPOSE of the whitened cross-covariance L^{-1} K(x, x*) that `gpk_trsm_lower` would
 * have to compute afterwards.  Their flops ride in the factorisation's own GEMM launches and, in its chain-bound tail, on
 * workgroups that would otherwise wait: the separate many-column solve (and its ~30 launches) disappears from the posterior path.
 * nb = 0: pipelined panels (any n up to the look-ahead threshold; dinv_sb / ws unused);  nb > 0: look-ahead as gpk_potrf_la /
 * gpk_potrf_la_split (sb = 0: sb = nb), `ws`: gpk_potrf_la_ws_elems(rows, nb).
 * n must be a multiple of 128 when rows > n; `dinv`: gpk_dinv_elems(n) + 128 * 128 elements (one slot more: control words).
 * Replaces `B.cholesky` + the `B.solve(L, K_zx)` of mlkernels' PosteriorKernel / PosteriorMean (observations.py:148-168) in one call. */
int gpk_potrf_rows(int dtype, void* a, int64_t n, int64_t rows, int64_t ld, void* dinv, void* dinv_sb, int nb, int sb, void* ws, int* info,
                   void* stream);

/* The same with flags (round 6):
 *   GPK_ROWS_RHS               the last GPK_ROWS_RHS_STRIP (64) rows are a strip whose FIRST row, a[rows - 64][0 .. n), is one right-hand
 *                              side b (contiguous); the other 63 are padding (initialise them -- zeros; unspecified on return): whole
 *                              64-row strips keep the plain tail on its fast kernels.  b comes out as L^{-1} b like every
 *                              other row does, but through the look-ahead steps it is treated as the vector it is -- the two matrix-vector
 *                              products per diagonal block of gpk_trsv_lower, enqueued as soon as a panel is final on a third stream (CU mask of the helper stream), so
 *                              that they run beside the trailing updates instead of as ~30 dependent launches behind the factorisation;
 *                              the plain tail (and the pipelined panels, nb = 0) carry it as a row.  The observations y - m(x) of the
 *                              posterior mean / log-density: the single-column solve disappears from the step.
 *   GPK_ROWS_NO_TAIL_INVERSES  the sb-wide explicit inverses of the plain tail's diagonal blocks (the last <= 6144 columns) are NOT
 *                              written to dinv_sb (nobody is going to solve against this factor with them; gpk_trtri_merge computes
 *                              them from `dinv` on demand).  The look-ahead panels' own inverses are always there.
 * Replaces `B.cholesky` + `B.solve(L, K_zx)` + the solve inside `B.iqf_diag(K, y - m)`: stheno/model/observations.py:148-168,
 * stheno/random.py:272-279. */
#define GPK_ROWS_RHS 1
#define GPK_ROWS_NO_TAIL_INVERSES 2
#define GPK_ROWS_RHS_STRIP 64
int gpk_potrf_rows_rhs(int dtype, void* a, int64_t n, int64_t rows, int64_t ld, void* dinv, void* dinv_sb, int nb, int sb, void* ws, int* info,
                       int flags, void* stream);

/* Merge the 128-block inverses into inverses of sb x sb diagonal blocks
 * (sb = 128 * 2^k <= 4096); dinv_sb: [batch][ceil(n/sb)][sb][sb];
 * tmp: >= ceil(n/sb) * sb * sb / 4 elements.  Part of the blocked TRSM below. */
int gpk_trtri_merge(int dtype, const void* l, int64_t n, int64_t ld, int64_t sl, int64_t batch,
                    const void* dinv128, int sb, void* dinv_sb, void* tmp, void* stream);

/* B <- L^{-1} B, many right-hand sides: recursive blocked solve on the MFMA GEMM (half of the flops in ONE GEMM with K = n/2, a
 * quarter in two with K = n/4, ...; the sb x sb diagonal blocks by their merged inverses).  tmp: batch * sb * nrhs elements.
 * Replaces `B.solve(L, .)` / the solves inside `B.iqf` (LAPACK trsm):
 * stheno/model/observations.py:301,322,327,329; mlkernels.PosteriorMean/PosteriorKernel
 * constructed at observations.py:148-168. */
int gpk_trsm_lower(int dtype, const void* l, int64_t n, int64_t ld, int64_t sl, const void* dinv_sb,
                   int sb, void* b, int64_t nrhs, int64_t ldb, int64_t sb_stride, void* tmp,
                   int64_t batch, void* stream);

/* The same solve OUT OF PLACE: x = L^{-1} b into a second n x nrhs buffer (ldx >= nrhs), `b` is used up as workspace.  Saves the
 * copy of every solved block (the in-place form builds it in `tmp` first): the form the posterior path uses for its
 * 2048-column solve.  Replaces the same reference call sites as gpk_trsm_lower. */
int gpk_trsm_lower_to(int dtype, const void* l, int64_t n, int64_t ld, int64_t sl, const void* dinv_sb,
                      int sb, void* b, int64_t nrhs, int64_t ldb, int64_t sb_stride, void* x, int64_t ldx,
                      int64_t sx_stride, int64_t batch, void* stream);

/* B <- L^{-1} B, nrhs <= 8 (GEMV sweep, HBM-bound).  tmp: batch * sb * nrhs + GPK_TRSV_CTRL_ELEMS elements (16-byte aligned;
 * the extra elements are reserved: they held the control words of a single-launch sweep that has been removed).
 * Replaces the solve inside `B.iqf_diag(var, y - mean)`: stheno/random.py:276,
 * stheno/model/observations.py:335. */
#define GPK_TRSV_CTRL_ELEMS 16
int gpk_trsv_lower(int dtype, const void* l, int64_t n, int64_t ld, int64_t sl, const void* dinv_sb,
                   int sb, void* b, int nrhs, int64_t ldb, int64_t sb_stride, void* tmp, int64_t batch,
                   void* stream);

/* X = L^{-T} B, many right-hand sides, OUT OF PLACE like gpk_trsm_lower_to (`b` is used up as workspace, x: ldx >= nrhs): the same
 * recursive blocked solve run bottom-up -- X2 = L22^{-T} B2, B1 -= L21^T X2 (ONE GEMM reading L21 where it is, K x M), X1 = L11^{-T} B1;
 * the leaves multiply by the transposes of the same merged sb x sb inverses (dinv_sb as for gpk_trsm_lower).
 * Replaces the `B.solve(L^T, .)` (LAPACK trsm, transposed) inside the reference's autograd through mlkernels.PosteriorMean /
 * PosteriorKernel (observations.py:148-168): the backward of the posterior mean and marginal variances. */
int gpk_trsm_lower_t(int dtype, const void* l, int64_t n, int64_t ld, int64_t sl, const void* dinv_sb,
                     int sb, void* b, int64_t nrhs, int64_t ldb, int64_t sb_stride, void* x, int64_t ldx,
                     int64_t sx_stride, int64_t batch, void* stream);

/* B <- L^{-T} B, nrhs <= 8: bottom-up sweep over the sb-blocks, two launches per block (transposed GEMVs: L read by block rows,
 * HBM-bound like gpk_trsv_lower).  tmp: batch * sb * nrhs elements.  Replaces the single-column transposed solves of the same
 * backward (`K^{-1} (y - m)` and `L^{-T} (V g)`). */
int gpk_trsv_lower_t(int dtype, const void* l, int64_t n, int64_t ld, int64_t sl, const void* dinv_sb,
                     int sb, void* b, int nrhs, int64_t ldb, int64_t sb_stride, void* tmp, int64_t batch,
                     void* stream);

/* C = alpha * op(A) op(B)^T-style contraction + beta * C on MFMA:
 *   C[m][n] = alpha * sum_k a(m,k) b(n,k) + beta * C[m][n]
 * a_kmajor != 0: A stored M x K (k contiguous); else stored K x M.  Same for B (N x K / K x N).
 * flags: GPK_GEMM_LOWER = only tiles on/below the diagonal (SYRK); GPK_GEMM_TRI_K = both operands
 * vanish for k < their row index (lower-triangular factors stored K x M, e.g. W^T W with W = L^{-1}):
 * all-zero k-chunks are skipped; GPK_GEMM_TRI_K_LOWER = A (M x K) is lower triangular (a(m,k) = 0 for
 * k > m, e.g. an inverted diagonal block times right-hand sides): the k loop stops at the tile's last row;
 * GPK_GEMM_TRI_K_LOWER_B = the same for B (b(n,k) = 0 for k > n: right-hand sides times an inverted block, transposed).
 * Replaces the dense products
 * `B.mm` / `B.matmul` / `B.iqf` outer products: stheno/model/observations.py:322-323,
 * mlkernels.PosteriorKernel (full covariance), `B.sample` (L xi): stheno/random.py:351. */
int gpk_gemm(int dtype, int a_kmajor, int b_kmajor, int64_t m, int64_t n, int64_t k, double alpha,
             const void* a, int64_t lda, int64_t sa, const void* b, int64_t ldb, int64_t sb, double beta,
             void* c, int64_t ldc, int64_t sc, int64_t batch, int flags, void* stream);

/* The same contraction with a column scaling and column statistics folded into the store (unbatched, beta = 0, no GPK_GEMM_LOWER):
 *   c[m][n] = alpha * sum_k a(m,k) b(n,k) * colscale[n]          (colscale NULL: no scaling)
 *   colss[r][n] = sum over the 64 rows of slab r of (alpha * sum_k a(m,k) b(n,k))^2      (colss NULL: not computed)
 * colss: gpk_gemm_colss_rows(m) rows of ldss >= n elements; the column sums of squares of the UNSCALED product are the sums of its
 * rows.  What SURVEY 8(b) proposed as `gpk_syrk_scaled`, cut where the pseudo-point path needs it: V = L_z^{-1} K_zx leaves the
 * kernel as V K_n^{-1/2}, and Q_x_diag = column sums of squares of V (`B.matmul_diag`) is a by-product -- the stand-alone scaling
 * and reduction passes over the M x N matrix are gone.  Replaces `B.solve` + `B.matmul_diag` + the K_n^{-1/2} scalings at
 * stheno/model/observations.py:301, 305, 322, 327. */
int64_t gpk_gemm_colss_rows(int64_t m);
int gpk_gemm_colscale(int dtype, int a_kmajor, int b_kmajor, int64_t m, int64_t n, int64_t k, double alpha,
                      const void* a, int64_t lda, const void* b, int64_t ldb, void* c, int64_t ldc, int flags,
                      const void* colscale, void* colss, int64_t ldss, void* stream);

/* Up to two rank-k updates in ONE persistent launch (a resident set of workgroups pulls 128x128 tiles of
 * both problems from a device-side counter: one ramp, one tail):
 *   c[m][n] = cin[m][n] + alpha * sum_k a[m][k] b[n][k]        a: m x k, b: n x k, both row-major
 * `cin` may differ from `c` (out-of-place update).  lower_only: tiles on/below the diagonal only.
 * ctrl: 256 bytes of device scratch (zeroed by the call).  reserve_cus != 0: the kernel leaves one CU per XCD
 * empty while it runs, for work enqueued on another stream (what gpk_potrf_la does for its panel chain).
 * This is the trailing update of gpk_potrf_la, exposed for measurement and reuse. */
typedef struct {
    int64_t m, n, k;
    const void* a; int64_t lda;
    const void* b; int64_t ldb;
    const void* cin; int64_t ldcin;
    void* c; int64_t ldc;
    int lower_only;
} gpk_update_t;
int gpk_gemm_update2(int dtype, const gpk_update_t* upd, int nupd, double alpha, void* ctrl, int reserve_cus,
                     void* stream);

/* out[b] = 2 * sum_i log L[i][i].  Replaces `B.logdet`: stheno/random.py:274,
 * stheno/model/observations.py:334. */
int gpk_logdet_chol(int dtype, const void* l, int64_t n, int64_t ld, int64_t sl, int64_t batch,
                    void* out, void* stream);

/* Number of row chunks (workspace sizing) used by gpk_colreduce for `rows` rows. */
int64_t gpk_colreduce_chunks(int64_t rows);

/* Row reductions of Z (rows x n, row-major, ld >= n):  out_dot[i] = sum_k Z[i][k] w[k]  (skipped if out_dot is NULL),
 * out_ss[i] = sum_k Z[i][k]^2  (skipped if out_ss is NULL), one pass.  The posterior mean and marginal variance from the rows
 * gpk_potrf_rows leaves under the factor (Z = K(x*, x) L^{-T}): the same quantities as gpk_colreduce on L^{-1} K(x, x*).
 * Replaces the reductions inside mlkernels' PosteriorMean / PosteriorKernel.elwise (observations.py:148-168). */
int gpk_rowreduce(int dtype, const void* z, int64_t rows, int64_t n, int64_t ld, const void* w, void* out_dot, void* out_ss, void* stream);

/* Fused column reductions of V (rows x cols):
 *   out_dot[j] = sum_i V[i][j] w[i]   (skipped if out_dot or w is NULL)
 *   out_ss[j]  = sum_i V[i][j]^2      (skipped if out_ss is NULL)
 * ws: 2 * batch * gpk_colreduce_chunks(rows) * cols elements.  Deterministic (two-stage).
 * Replaces `B.iqf_diag` / `B.matmul_diag(V, V, tr_a=True)` (random.py:276, observations.py:305)
 * and the mean contraction of mlkernels.PosteriorMean. */
int gpk_colreduce(int dtype, const void* v, int64_t rows, int64_t cols, int64_t ld, int64_t sv,
                  const void* w, int64_t sw, void* out_dot, void* out_ss, void* ws, int64_t batch,
                  void* stream);

/* out[i][j] = sum_s parts[s][i][j] for j <= i: the partial products of a SPLIT-K symmetric update (`nparts` n x n matrices, `sp`
 * elements apart, of which only the lower tiles were written -- gpk_gemm with GPK_GEMM_LOWER over a batch of k-slices) added up in a
 * fixed order, lower triangle only (entries above the diagonal of `out` are unspecified).  The pseudo-point path's
 * `V K_n^{-1} V^T` (observations.py:322) with its 200 000-long contraction cut into 25 slices: replaces a zero fill of the 25 partial
 * matrices and a torch reduction over all of them. */
int gpk_sum_lower(int dtype, const void* parts, int64_t nparts, int64_t n, int64_t ldp, int64_t sp, void* out, int64_t ldo, void* stream);

/* Zero the strict upper triangle (clean Cholesky factor for `B.cholesky` consumers). */
int gpk_tril(int dtype, void* a, int64_t n, int64_t ld, int64_t sa, int64_t batch, void* stream);

/* A[i][i] += s + (v ? v[i] : 0):  `B.add(var, Diagonal)` / `B.reg`: stheno/model/fdd.py:79. */
int gpk_add_diag(int dtype, void* a, int64_t n, int64_t ld, int64_t sa, double s, const void* v,
                 int64_t sv, int64_t batch, void* stream);

/* V[i][j] *= s[j]  (column scaling by K_n^{-1/2} in the pseudo-point ELBO: the
 * `B.iqf(K_n, .)` with diagonal K_n of stheno/model/observations.py:322,327). */
int gpk_scale_cols(int dtype, void* v, int64_t rows, int64_t cols, int64_t ld, int64_t sv, const void* s,
                   int64_t ss, int64_t batch, void* stream);

/* Mirror the lower triangle into the upper one (full symmetric matrix after a lower-only SYRK/kmat). */
int gpk_symmetrize(int dtype, void* a, int64_t n, int64_t ld, int64_t sa, int64_t batch, void* stream);

/* y[m x nrhs] = alpha * A[m x k] x[k x nrhs] + beta * y, nrhs <= 8, A row-major; trans must be 0.
 * HBM-bound matrix-vector products of the path (e.g. `B.iqf(K_n, V^T, y)`: observations.py:327). */
int gpk_gemv(int dtype, int trans, int64_t m, int64_t k, int nrhs, double alpha, const void* a, int64_t lda,
             int64_t sa, const void* x, int64_t ldx, int64_t sx, double beta, void* y, int64_t ldy, int64_t sy,
             int64_t batch, void* stream);

/* W <- L^{-1}: the full lower-triangular inverse (n x n, ldw), N^3/3 flops on the MFMA GEMM.
 * dinv_sb as for gpk_trsm_lower (unbatched); tmp: sb * n elements.  With gpk_gemm(K x M storage,
 * GPK_GEMM_LOWER | GPK_GEMM_TRI_K) it gives K^{-1} = W^T W for the log-density gradient. */
int gpk_trtri_lower(int dtype, const void* l, int64_t n, int64_t ld, const void* dinv_sb, int sb, void* w,
                    int64_t ldw, void* tmp, void* stream);

/* The two kernel VJPs below leave per-workgroup PARTIAL ROWS of NS * GPK_MAX_TERMS + 1 elements, to be summed over the rows by the
 * caller: NS = 3 if any term's kind has a shape parameter (GPK_K_RQ, GPK_K_DELTA), NS = 2 otherwise --
 *   row[NS t] = S1_t = sum G kappa_t,   row[NS t + 1] = S2_t = sum G kappa_t'(q) q,   row[NS t + 2] = S3_t = sum G d kappa_t / d shape_t
 *   (NS = 3 only; 0 for kinds without a shape),   row[NS * GPK_MAX_TERMS]: the trace slot.
 * d/d variance_t = S1_t;  d/d scale_t = -2 v_t S2_t / l_t;  d/d alpha_t = v_t S3_t.
 * RQ, with u = q / (2 alpha): kappa' q = -(q / 2) kappa / (1 + u),  d kappa / d alpha = kappa (u / (1 + u) - log1p(u)).
 * Delta (piecewise constant): S2_t = S3_t = 0 -- its variance is learnable, its scale and epsilon are not.
 * `shapes` as for gpk_kmat: may be NULL exactly when no term is shaped; a shaped kind with shapes == NULL returns -1. */

/* Kernel-hyperparameter VJP of the GP log-density (hyper-parameter learning through
 * `f(x, noise).logpdf(y)`: readme_example13_optimisation_torch.py:47-53).  With
 *   G = d logpdf / dK = 1/2 (A diag(g) A^T - sum(g) K^{-1}),  A = K^{-1} (y - m)  (n x ncols <= 8),
 * one pass over the LOWER triangle of `kinv` accumulates one partial row per workgroup (gpk_kmat_vjp_blocks(n) of them; the trace
 * slot holds trace(G)) and writes diag_g[i] = G_ii = d logpdf / d noise_i.  `g` (host): upstream gradient per column.
 * Returns -3 for nterms outside 0 .. GPK_MAX_TERMS, -1 for an unknown kind or missing `shapes`, -3 for an RQ alpha <= 0, -5 for a
 * Delta epsilon <= 0. */
int64_t gpk_kmat_vjp_blocks(int64_t n);
int gpk_kmat_vjp(int dtype, const int* kinds, const double* inv_ls, const double* shapes, int nterms, const void* x, int64_t n,
                 int64_t ldx, int d, const void* kinv, int64_t ldk, const void* alpha, int ncols, int64_t lda,
                 const double* g, void* partial, void* diag_g, void* stream);

/* Kernel VJP with an explicit cotangent (gradient of the pseudo-point ELBO w.r.t. kernel
 * hyper-parameters, observation noise and inducing inputs: the learning loop that
 * readme_example10_sparse.py:8-29 / stheno/model/observations.py:279-336 feed when `stheno.torch`
 * tensors carry gradients).  For K = k(x, y) (n x m, never formed) and
 *   Geff_ij = g[i][j] * colscale[j] + w[i] * b[j]      (colscale and the pair (w, b) may be NULL),
 * one pass over g writes, per workgroup (rowtiles x nchunks of them, see gpk_kmat_vjp_dense_grid),
 *   one partial row of sums over Geff (the trace slot is unused: 0),
 *   colsum[rowtile][j] = sum_{i in tile} Geff_ij K_ij        (NULL to skip; sum over row tiles),
 *   gradx[chunk][i][0..d) = sum_{j in chunk} Geff_ij dK_ij/dx_i   (NULL to skip; needs d <= 8; sum over chunks;
 *   RQ: through kappa' = -kappa / (2 (1 + u)); a Delta term counts in colsum, nothing in gradx).
 * Deterministic (no atomics).  Returns -5 for nterms outside 0 .. GPK_MAX_TERMS, -1 for an unknown kind or missing `shapes`, -4 for an
 * RQ alpha <= 0, -5 for a Delta epsilon <= 0. */
int gpk_kmat_vjp_dense_grid(int64_t n, int64_t m, int64_t* rowtiles, int64_t* nchunks);
int gpk_kmat_vjp_dense(int dtype, const int* kinds, const double* variances, const double* inv_ls, const double* shapes, int nterms,
                       const void* x, int64_t n, int64_t ldx, const void* y, int64_t m, int64_t ldy, int d,
                       const void* g, int64_t ldg, const void* colscale, const void* w, const void* b,
                       void* partial, void* colsum, void* gradx, void* stream);

/* The same reduction for a BATCH of independent problems under ONE term table (gradients through batched posterior means and marginal
 * variances under shared hyper-parameters): entry e reads x + e sx, y + e sy, g + e sg, colscale + e s_cs, w + e s_w, b + e s_b
 * (batch strides in elements, offsets in 64 bits) and is reduced by the kernel of gpk_kmat_vjp_dense, the batch being the third grid
 * dimension -- gpk_kmat_vjp_dense is the batch = 1 call of this entry and writes the same bits.  A batch stride of 0 is legal for every
 * input: sx = 0 shares one data set among the entries, sg = 0 with ldg = 0 is an all-zero cotangent operand of one row (a loss that
 * reaches the kernel matrix through w b^T only).  Outputs are packed per entry, to be summed by the caller as for the unbatched entry:
 *   partial [batch][rowtiles * nchunks][NS * GPK_MAX_TERMS + 1],   colsum [batch][rowtiles][m]  (nullable),
 *   gradx   [batch][nchunks][n][d]  (nullable; d <= 8),
 * rowtiles and nchunks from gpk_kmat_vjp_dense_batch_grid: row tiles as for the unbatched entry, and
 *   nchunks = clamp(cdiv(2048, rowtiles * batch), 1, column tiles)      (evened out over the column tiles),
 * so the launch aims at the ~2048 workgroups the unbatched grid aims at; with many entries a workgroup walks a whole row of column
 * tiles, its gradx accumulators in registers, and nchunks = 1.  Deterministic (no atomics).
 * Returns the codes of gpk_kmat_vjp_dense for the arguments the two share -- 0 at once for n or m <= 0; -5 nterms outside
 * 0 .. GPK_MAX_TERMS; -1 an unknown kind or missing `shapes`; -4 an RQ alpha <= 0; -5 a Delta epsilon <= 0; -7 n or m above 2^31 - 1;
 * -17 exactly one of w, b given; -12 gradx != NULL with d > 8; -9 more than 65535 column chunks -- and -28 for batch > 65535 (the
 * grid's limit).  batch <= 0 is an empty problem: 0, behind those checks.  gpk_kmat_vjp_dense_batch_grid: -4 for a NULL output. */
int gpk_kmat_vjp_dense_batch_grid(int64_t n, int64_t m, int64_t batch, int64_t* rowtiles, int64_t* nchunks);
int gpk_kmat_vjp_dense_batch(int dtype, const int* kinds, const double* variances, const double* inv_ls, const double* shapes, int nterms,
                             const void* x, int64_t n, int64_t ldx, int64_t sx, const void* y, int64_t m, int64_t ldy, int64_t sy, int d,
                             const void* g, int64_t ldg, int64_t sg, const void* colscale, int64_t s_cs,
                             const void* w, int64_t s_w, const void* b, int64_t s_b,
                             void* partial, void* colsum, void* gradx, int64_t batch, void* stream);

/* VJP of a derivative block: `g` (n x m, ldg, unit inner stride) is the explicit cotangent of the block gpk_kmat_diff writes for the
 * same (dim_x, dim_y) -- gradients of a posterior through the covariance of a process with its derivative and of two derivatives.
 * The block is never formed.  Grid, partial rows and their summation as for gpk_kmat_vjp_dense (rowtiles x nchunks workgroups from
 * gpk_kmat_vjp_dense_grid, rows of NS * GPK_MAX_TERMS + 1 elements, NS = 3 exactly when a term is GPK_K_RQ, the trace slot 0);
 * deterministic (no atomics), `g` is read once and nothing outside its n x m view; any d (input dimensions in chunks of 8).
 *   A block element is sum_t v_t beta_t.  Stationary term, c = inv_ls^2, q = c |x - y|^2, D_a = x[a] - y[a], kappa', kappa'' as above:
 *     d/dx_a         beta = 2 c kappa' D_a                                   c dbeta/dc = 2 c D_a (kappa' + q kappa'')
 *     d/dy_b         the same with -D_b
 *     d^2/dx_a dy_b  beta = -4 c^2 kappa'' D_a D_b - 2 c kappa' [a == b]
 *                    c dbeta/dc = -4 c^2 D_a D_b (2 kappa'' + q kappa''') - 2 c [a == b] (kappa' + q kappa'')
 *     GPK_K_EQ        q kappa''' = -q kappa / 8
 *     GPK_K_RQ        q kappa''' = -(alpha + 1)(alpha + 2) / (8 alpha^2) q (1 + u)^(-alpha - 3)
 *     GPK_K_MATERN52  q kappa''' = -(25/24) s e^(-s)
 *     GPK_K_MATERN32  q kappa''' = -(9/8) (1 + s) / s e^(-s),  so  2 kappa'' + q kappa''' = (9/8) (3 - s) / s e^(-s)
 *   GPK_K_LINEAR: beta = c y[a] | c x[b] | c [a == b] and c dbeta/dc = beta;  GPK_K_CONST: 0.
 *     row[NS t]     = S1_t = sum g beta_t                    d/d variance_t = S1_t
 *     row[NS t + 1] = S2_t = sum g c dbeta_t/dc              d/d scale_t = -2 v_t S2_t / l_t
 *     row[NS t + 2] = S3_t = sum g dbeta_t/dalpha_t          d/d alpha_t = v_t S3_t      (GPK_K_RQ only; 0 for every other kind)
 *   RQ's shape derivative, P_k = (1 + u)^(-alpha - k):  dP_k/dalpha = P_k ((alpha + k) u / (alpha (1 + u)) - log1p(u)),
 *   kappa' = -P_1 / 2, kappa'' = (alpha + 1) / (4 alpha) P_2; every exponent stays <= 0.  Matern32's 1 / s is taken as 0 where s is not
 *   positive, as in gpk_kmat_diff: coincident points add exactly 0 to its sums in both dtypes.
 *   gradx (nullable): [nchunks][n][d], the gradient with respect to the row input, summed over chunks by the caller; the two one-sided
 *   modes and d <= 8 only:
 *     d/dx_a:  dbeta/dx_e = 4 c^2 kappa'' D_a D_e + 2 c kappa' [e == a];     d/dy_b: -(4 c^2 kappa'' D_b D_e + 2 c kappa' [e == b]);
 *     GPK_K_LINEAR: 0 for d/dx_a, c [e == b] for d/dy_b.  (The mixed block's input gradient needs kappa''' alone, which Matern32 does
 *     not have at coincident points: not provided.)
 *   Numerics: element by element within 1.2 eps (the sums) / 3.5 eps (gradx) of the sum of the absolute values of everything added
 *   up for an output, in both dtypes (measured on an MI355X against an 80-bit reference: tests/diff_vjp_reference.py,
 *   tests/test_diff_vjp_gpu.py, profiles/README.md "Derivative-block gradient kernel, element by element").
 *   Every argument is checked before an empty problem (n or m <= 0) returns 0.  Returns -k for argument k:
 *     -6  nterms outside 0 .. GPK_MAX_TERMS;      -2  GPK_K_MATERN12, GPK_K_DELTA or an unknown kind;
 *     `shapes` as for gpk_kmat_diff: -1 for a GPK_K_RQ term with shapes == NULL, -5 for an alpha <= 0;
 *     -15 d < 0;      -7  dim_x outside [-1, d), or dim_x and dim_y both -1;      -8  dim_y outside [-1, d);
 *     -10 / -13  n / m too large (more than 2^31 - 1, or more than 65535 column chunks);
 *     -19 gradx != NULL in the mixed mode or with d > 8. */
int gpk_kmat_diff_vjp(int dtype, const int* kinds, const double* variances, const double* inv_ls, const double* shapes, int nterms,
                      int dim_x, int dim_y, const void* x, int64_t n, int64_t ldx, const void* y, int64_t m, int64_t ldy, int d,
                      const void* g, int64_t ldg, void* partial, void* gradx, void* stream);

/* VJP of the Cholesky factorisation A = L L^T (gradients through `B.cholesky`: joint posterior samples `mean + chol(Sigma) xi`,
 * stheno/random.py:351, under a learnable kernel).
 *   l: the factor gpk_potrf left (n x n, ld; ONLY its lower triangle is read -- the strict upper triangle holds whatever gpk_potrf
 *   left there).  lbar: the cotangent of L (n x n, ldlb; only its lower triangle is read).  abar (n x n, lda, written FULL and exactly
 *   symmetric, abar[i][j] == abar[j][i] bit for bit):
 *     abar = W^T Psym W,   W = L^{-1},   Psym = 1/2 (P + P^T),   P = Phi(L^T tril(lbar)),   Phi = lower triangle with the diagonal halved
 *   so that <abar, E> = d/dt sum(lbar * chol(A + t E)) for every symmetric E.  dinv_sb / sb as for gpk_trsm_lower (unbatched).
 *   ws: gpk_potrf_vjp_ws_elems(n, sb) elements of scratch = three n x ceil16(n) matrices + the sb * n of gpk_trtri_lower (0 for n <= 0 or
 *   an invalid sb); 16-byte aligned for the GEMM's vector loads.
 *   Launches, all on `stream`: two clean lower-triangular copies of l and lbar into ws (the GEMM's GPK_GEMM_TRI_K skips whole
 *   k-chunks, not elements, so its diagonal tiles must read zeros above the diagonal; NaN or Inf in the callers' strict upper
 *   triangles never reaches the result), lower(L^T lbar) by one GEMM (GPK_GEMM_LOWER | GPK_GEMM_TRI_K), Phi and the half-sum into a
 *   full symmetric matrix by one tiled transposing kernel, W by gpk_trtri_lower, W^T Psym (GPK_GEMM_TRI_K) and lower(W^T Psym W)
 *   (GPK_GEMM_LOWER | GPK_GEMM_TRI_K) by two GEMMs, the mirror by gpk_symmetrize (a copy).  About (1/3 + 1/3 + 1 + 1/3) 2 n^3 / 2
 *   multiply-adds.  No allocation, no host synchronisation, no atomics: a repeated call writes the same bits.  Nothing outside the
 *   n x n view of abar is written; l, lbar and dinv_sb are not modified.  n is any order (the 128-block inverses are identity-padded).
 *   Returns -k for argument k, checked in this order: -1 an unknown dtype; then n <= 0 returns 0 (an empty problem); -2 l == NULL;
 *   -3 n above 2^20; -4 ld < n; -5 dinv_sb == NULL; -6 sb not 128 * 2^k <= 4096; -7 lbar == NULL; -8 ldlb < n; -9 abar == NULL;
 *   -10 lda < n (or beyond the GEMM's limit on the leading dimension of C); -11 ws == NULL.  GPK_ERR_LAUNCH if a launch failed. */
int64_t gpk_potrf_vjp_ws_elems(int64_t n, int sb);
int gpk_potrf_vjp(int dtype, const void* l, int64_t n, int64_t ld, const void* dinv_sb, int sb, const void* lbar, int64_t ldlb,
                  void* abar, int64_t lda, void* ws, void* stream);

/* Nuclear norm (sum of the singular values) of a batch of square matrices:  out[b] = |M_b|_* = tr(U_b^T M_b),  U the orthogonal
 * polar factor of M, taken as the limit of the Newton-Schulz iteration
 *     X_0 = M / |M|_F,      X <- X (3/2 I - 1/2 X^T X)                      (`iters` steps, two GEMMs each: 3 n^3 flops per step)
 * With V1 = L1 L1^T, V2 = L2 L2^T and M = L2^T L1 it is tr (V1^(1/2) V2 V1^(1/2))^(1/2), the cross term of the 2-Wasserstein distance
 * between two normal distributions -- V1^(1/2) V2 V1^(1/2), V2 V1 and M^T M share their non-zero eigenvalues.  Replaces the two dense
 * eigendecompositions `B.root(B.matmul(B.root(V1), V2, B.root(V1)))` of `Normal.w2`: stheno/random.py:313-329.
 *   m: `batch` matrices of n x n, row stride ld >= n, batch stride sm >= 0 (0 shares one matrix); READ ONLY, and only inside its n
 *   columns: the padding of a row may hold NaN.  out: batch values.  ws: gpk_nuclear_norm_ws_elems(n, batch) elements of scratch =
 *   batch * (3 n ceil16(n) + min(ceil(n / 32), 512) + 1): three n x ceil16(n) matrices per entry (X, X', S), the per-workgroup partial
 *   sums of the reductions and the norm (0 for n <= 0, batch <= 0 or a size the entry refuses); 16-byte aligned for the GEMM's vector
 *   loads; its contents on entry do not matter (NaN included).
 *   Launches, all on `stream`: the Frobenius norm of every entry as a two-stage reduction (per-workgroup partial sums over 32-row
 *   bands, accumulated in fp64 in both dtypes, then one finishing workgroup per entry; fixed order); X_0 = M / |M|_F with the norm read
 *   from device memory (a zero matrix gives X_0 = 0 and out = 0, never NaN); per step S = lower(X^T X) by one GEMM (GPK_GEMM_LOWER),
 *   the full symmetric T = 3/2 I - 1/2 S from the lower triangle of S by one tiled transposing kernel, X' = X T by one GEMM into the
 *   second X buffer; at the end out[b] = sum_ij X_ij M_ij by the same two-stage reduction, reading the caller's m with its strides.
 *   The batch is the third grid dimension of the kernels and the batch of the GEMMs: one launch sequence for all entries, which
 *   depends on (n, batch, iters) alone.  No allocation, no host read, no atomics: a repeated call writes the same bits.
 *   Step count: a singular value that has not reached 1 after k steps was below about 1.5^-(k - 8) |M|_F to begin with and contributes
 *   at most its own size to the error; 60 steps (fp64) / 40 (fp32) leave that below the rounding of the sum.
 *   There is no convergence read.  Entries far outside 1e-150 .. 1e150 in magnitude overflow or underflow the sum of squares.
 *   Returns -k for argument k, checked in this order: -1 an unknown dtype; then n <= 0 or batch <= 0 returns 0 (an empty problem,
 *   nothing launched); -2 m == NULL; -3 n above 2^20 (the 32-tiles of the kernels are a grid dimension); -4 ld < n; -5 sm < 0;
 *   -6 batch above 65535 (a grid dimension); -7 iters < 1; -8 out == NULL; -9 ws == NULL.  GPK_ERR_LAUNCH if a launch failed. */
int64_t gpk_nuclear_norm_ws_elems(int64_t n, int64_t batch);
int gpk_nuclear_norm(int dtype, const void* m, int64_t n, int64_t ld, int64_t sm, int64_t batch, int iters, void* out, void* ws,
                     void* stream);

/* BORDERED Cholesky: grow the factor of an n x n matrix by q new rows and columns without refactorising (a data set that grows by a
 * few points per step: sequential conditioning, Bayesian optimisation).  With K11 = L11 L11^T factored and the bordered matrix
 * [[K11, K12], [K12^T, K22]]:   L21 = (L11^{-1} K12)^T,   L22 = chol(K22 - L21 L21^T),   w2 = L22^{-1} (r2 - L21 w1).
 * The O(n^2 q) part, V = L11^{-1} K12, is the caller's (gpk_trsm_lower_to / gpk_trsv_lower); this entry is the O(n q^2 + q^3) rest.
 * On entry:  a (leading dimension ld >= n + q): rows [0, n) hold L11 (strict upper triangle unspecified, as after gpk_potrf);
 *   a[n + i][n + j], j <= i < q, holds the lower triangle of K22 WITH its diagonal additions (noise, jitter);
 *   v: V, n x q, unit inner stride, leading dimension ldv >= q;
 *   dinv: ceil((n + q) / 128) blocks of 128 x 128, the first ceil(n / 128) as gpk_potrf left them for L11;
 *   w1 (n values: L11^{-1} r1) and r2 (q values): both given or both NULL;
 *   ws: gpk_potrf_border_ws_elems(n, q) elements of scratch (0 for an n or q the entry refuses); info: one int (need not be zeroed).
 * On return: a[n + i][0 .. n) = row i of V^T (L21); a[n + i][n .. n + i] = L22 (entries right of the diagonal in the new rows are
 *   unspecified); rows < n of `a` are not written.  dinv blocks g >= n / 128 (integer division) hold the inverse of the 128 x 128
 *   diagonal block of the GROWN factor -- the block L11 filled only partly (n % 128 != 0) is REWRITTEN -- padded as gpk_potrf pads
 *   a partial last block: the block is taken as diag(L_gg, I), so its inverse has the identity behind row n + q and zeros above the
 *   diagonal.  Blocks below n / 128 are not written.  r2 is overwritten by w2.  info[0] = 0, or n + j when the leading minor of order
 *   n + j of the bordered matrix is not positive definite (gpk_potrf's convention; the new rows, dinv and r2 are then unspecified).
 * Four launches on `stream` (gpk_border.hip): V^T + partial Gram matrices of at most 64 row chunks of V + partial V^T w1 in one pass
 * over V; the partials added in chunk order, one thread per element; ONE workgroup that forms S = K22 - sum and factorises it in LDS
 * with the block routine of gpk_potrf, w2 by forward substitution; one workgroup per touched 128-block (at most two) that inverts the
 * block of the grown factor by substitution (X L = I row by row).  No atomics, fixed summation order: a repeated call writes the same bits.  No
 * allocation, no host synchronisation.
 * Returns -k for argument k, all checked before anything is launched: -1 an unknown dtype; -2 a == NULL; -3 n < 1 (or above 2^30);
 * -4 q outside 1 .. GPK_BORDER_MAX; -5 ld < n + q; -6 v == NULL; -7 ldv < q; -8 dinv == NULL; -9 r2 given without w1; -10 w1 given
 * without r2; -11 info == NULL; -12 ws == NULL.  GPK_ERR_LAUNCH if a launch failed. */
#define GPK_BORDER_MAX 128
int64_t gpk_potrf_border_ws_elems(int64_t n, int q);
int gpk_potrf_border(int dtype, void* a, int64_t n, int q, int64_t ld, const void* v, int64_t ldv, void* dinv, const void* w1, void* r2,
                     int* info, void* ws, void* stream);

/* Measurement hooks (bench.py's live roofline figure).  Between gpk_prof_start and
 * gpk_prof_stop every MFMA GEMM launch of this process is bracketed by HIP events on its
 * launch stream; gpk_prof_stop synchronises those events and returns the summed duration,
 * launch count and ALGORITHMIC flops (2mnk; mnk for a lower-only symmetric update) of the
 * launches of one kernel variant: 16*(64x64-tile kernel) + 8*(f64) + 4*(a_kmajor) + 2*(b_kmajor)
 * + 1*(bounds-checked kernel); + 32 = the persistent update (gemm_persist_kernel), 64 + ... = panel_step_kernel,
 * 96 + ... = gemm_trilo_pair_kernel, 128 + ... = gemm_trib_kernel, 160 (+ 8: f64) = batch_mix_kernel (one mixed-phase step of a batched
 * factorisation: its panel solves at the TRSM count + its update tiles at the symmetric count); or -1 for all.  Not thread-safe; off by default; not used
 * by the product path. */
int gpk_prof_start(void);
int gpk_prof_stop(int variant, double* total_ms, int64_t* launches, double* useful_flops);

/* The SUSTAINED rate of the matrix pipes, measured on the device the call runs on ("re-derive on the box from a measured
 * MFMA micro-benchmark and print the value used"): one workgroup per CU, `waves_per_simd` (1 or 2) register-resident waves per SIMD
 * streaming v_mfma_f64_16x16x4_f64 / v_mfma_f32_16x16x4_f32 (the instructions every GEMM of this library issues) on pseudo-random
 * operands into 8 independent accumulators, launches repeated until `min_ms` of device time have passed.  Out: *tflops = flops / HIP-event
 * time; *ms = that time; *clock_mhz = the shader clock the stream ran at (s_memtime cycles over the 100 MHz wall clock, last launch,
 * mean over CUs); *issue_eff = tflops / (CUs x clock x 128 (f64) / 256 (f32) flops per CU and cycle) -- the last three may be NULL.
 * A measurement hook like gpk_prof_*: allocates its own 4 KiB of scratch, SYNCHRONISES the stream, not on the product path. */
int gpk_mfma_peak(int dtype, double min_ms, int waves_per_simd, double* tflops, double* ms, double* clock_mhz, double* issue_eff, void* stream);

/* Development aids.  The RELEASE library (stheno_amd/csrc/libgpk.so) has no tuning knobs: every one of them is a compile-time
 * constant at its measured optimum and gpk_tune() does nothing.  The dev build (stheno_amd/csrc/dev/libgpk.so, -DGPK_DEV_KNOBS;
 * what the native self-test links against and what GPK_DEV=1 makes the Python binding load) keeps them mutable for A/B runs
 * (`gpk_selftest --set KEY VALUE`).  key 1: use 64x64 GEMM tiles below this many 128-tiles; 6: look-ahead overlaps while the
 * trailing matrix has at least this many rows; 7: 0 = look-ahead algorithm on one stream, 1 = with the helper stream; 8: the
 * persistent update takes 64x64 tiles below this many 128-tiles; 9: gpk_potrf_la finishes the last this-many rows with the plain
 * algorithm (0 = 6144); 12: 1 = row-band kernel-matrix kernel, 0 = one tile per workgroup (gpk_kmat and gpk_kmat_diff); 17: 1 = one-workgroup-per-matrix TRSV
 * for batches of small factors; 20: gpk_tune_tile_prof stamps only the v-th persistent launch since this knob was set (-1 = every launch); 31: quarter tiles for
 * the last partial round of a 128-tile GEMM launch; 32: fused panel-step kernel (batched / fallback path); 34: compact 1-D grid for
 * lower-triangle kernel matrices; 36: triangular-operand fragment skipping in panel solves; 37: 1 = one pipelined launch per panel
 * for single matrices, 0 = diagonal-block kernel + panel-step kernel per 128 columns (the batched path's steps); 38: the rest of a
 * panel's trailing update rides in the next panel's launch; 39: workgroups that take panel tasks first in such a launch (0 = a
 * third of the CUs); 40 / 41: the look-ahead's update of the next diagonal block is the first segment of the trailing update while
 * that has at least (40) rows and the outer block is at most (41) wide; 42: small products with a lower-triangular A (the leaves of
 * the recursive solve) as pairs of 32-row tiles with equal K per workgroup; 45: batched 128-tile GEMM launches as a 1-D grid with all
 * tiles of a matrix on one XCD; 47: gpk_potrf_la aggregates its trailing updates -- a column block is brought up to date every
 * this-many outer steps (1 = every step); 48: ... only while the trailing matrix has at least this many rows; 51: fp64 kernel
 * matrices with a square root (Matern) take the row-band kernel too; 52: panel width of the pipelined plain factorisation of one
 * matrix above n = 4096; 53: batched fp32 factorisations take the mixed-phase steps (0 = lockstep launches, 1 = mixed-phase; fp64
 * always takes the lockstep launches); 54: ... from this many matrices on; 55: tasks between a matrix's solves and its update tiles
 * in the queue order; 57: fp32 batches of more matrices than CUs take the diagonal-block kernel compiled for two workgroups per CU.
 * (Removed in round 4 with the code they selected: 2 / 4 / 13 -- XCD super-tile, row-pair and column-major tile orders -- and 30,
 * the 256-thread diagonal-block kernel of rounds 1-2.  Removed after rounds 5 and 6, measured slower or flat: 10 / 11 / 18 -- the
 * persistent panel GEMM of gpk_potrf_la, the strip's place in the trailing update, the reserved CUs' rejoin switch -- 49 / 50, the
 * single-launch sweep of gpk_trsv_lower, 56 and 60, development switches and the left-looking update of the mixed-phase steps, and
 * 58 / 59, chunked task claims of the persistent update; 53 lost its fp64 value 2.)
 * gpk_tune_diag_prof: device buffer (32 int64 per diagonal block, or NULL) for cycle / wall-clock stamps of the diagonal-block
 * kernel and of the pipelined panel's chain and critical tasks (read by `gpk_selftest --diagprof`). */
void gpk_tune(int key, int64_t value);
void gpk_tune_diag_prof(long long* dev_buf);
/* device buffer (grid x 8 tiles x 8 int64, or NULL): stamps of the persistent update's first 8 tiles per workgroup:
 * [0..3] wall clock (10 ns ticks) at entry / C tile requested / k loop done / stores retired, [4], [5] shader-cycle
 * counter at the start and the end of the k loop (so the clock the loop ran at can be read off), [6] wall clock when the C values
 * and the first operand chunk have arrived (pipelined 128-tile), [7] unused. */
void gpk_tune_tile_prof(long long* dev_buf);

/* Strided 2-D copy (rows x cols). */
int gpk_copy2d(int dtype, const void* src, int64_t lds, int64_t ss, void* dst, int64_t ldd, int64_t sd,
               int64_t rows, int64_t cols, int64_t batch, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GPK_H */
