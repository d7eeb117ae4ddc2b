// gpk_kdiff.hip -- derivative blocks of the kernel matrix: fused pairwise distance + derivative of the kernel.
//
//   out[i][j] (+)= d/dx_i[a] k(x_i, y_j)                 (dim_x = a >= 0, dim_y = -1)
//                  d/dy_j[b] k(x_i, y_j)                 (dim_x = -1, dim_y = b >= 0)
//                  d^2/dx_i[a] dy_j[b] k(x_i, y_j)       (both >= 0)          k = sum_t variance_t kappa_t
//
// Replaces: mlkernels `DerivativeKernel` (autodiff of `pairwise`) behind `GP.diff` -- stheno/model/measure.py:343-360: the
// covariance blocks of a process with its derivative and of two derivatives.  Formulas in include/gpk.h (gpk_kmat_diff).
//
// Same memory profile as gpk_kmat.hip -- N x M values written once, HBM-write-bound -- and the same two launch shapes on the same
// launch geometry (gpk_kmat_plan.hpp) and tile helpers (gpk_kmat_tile.hpp): the row-band walk (d <= 8: Y tiles staged through LDS,
// 8 KiB contiguous per row and workgroup, non-temporal stores) and the chunked one-tile kernel (d > 8); X rows in LDS, squared
// distances from direct differences.  On top of r^2 an element keeps the differences in the selected dimensions,
// x[a] - y[a] and x[b] - y[b] (for Linear terms: y[a] or x[b] themselves).  One term-table program; the mode and "some term has a
// shape parameter" are template parameters (the one-sided modes never evaluate kappa'', tables without RQ never the logarithm).
#include "gpk_common.hpp"
#include "gpk_kmat_tile.hpp"

GPK_KNOB(int, g_kdiff_band, 1);      // tuning knob (gpk_tune(12, v), shared with gpk_kmat): 1 = row-band kernel, 0 = the one-tile-per-workgroup kernel
GPK_KNOB(int, g_kdiff_compact, 1);   // tuning knob (gpk_tune(34, v), shared with gpk_kmat): 1-D compact grid for the lower triangle of a square matrix
void gpk_tune_kdiff(int key, int64_t value) {
    if (key == 12) GPK_KNOB_SET(g_kdiff_band = (int)value;);
    if (key == 34) GPK_KNOB_SET(g_kdiff_compact = (int)value;);
}

namespace {

enum { MODE_DX = 0, MODE_DY = 1, MODE_DXY = 2 };

template <typename T>
struct KdiffArgs {
    const T* X;
    const T* Y;
    T* out;
    const T* diag_vec;
    int64_t ldx, ldy, sX, sY, ld, sO, sDiag;
    int n, m, d;
    int dim_x, dim_y;
    int nterms;
    KTermT<T> terms[GPK_MAX_TERMS];
    T diag_add;
    int symmetric, lower_only, accumulate, vec_ok;
    int ct, nbands, compact;     // row-band kernel: as in gpk_kmat.hip
    // GPK_K_RQ: 1 / (2 alpha), alpha + 1, alpha + 2 and (alpha + 1) / (4 alpha)
    T hshape[GPK_MAX_TERMS];
    T shape1[GPK_MAX_TERMS];
    T shape2[GPK_MAX_TERMS];
    T rq2[GPK_MAX_TERMS];
};

// The chosen derivative of the term table at one pair of points.  With q = c r^2, c = ils2:
//   s1 = sum_t v c kappa'(q),   s2 = sum_t v c^2 kappa''(q)   (stationary terms),   lin = sum_t v c   (Linear terms)
//   d/dx_a = 2 s1 da + lin y_a,   d/dy_b = -2 s1 db + lin x_b,   d2/dx_a dy_b = -4 s2 da db + [a == b] (lin - 2 s1)
// da = x_a - y_a, db = x_b - y_b; `other`: y_a (MODE_DX) / x_b (MODE_DY); `same`: a == b (MODE_DXY).
// Matern32's kappa'' = 9 / (4 s) e^{-s} is singular at s = 0 while kappa'' da db -> 0 (|da db| <= r^2 = s^2 / (3 c)): its 1 / s is taken
// as 0 where s is not positive, and da db = 0 there, so coincident points give exactly 0 in both dtypes.
template <typename T, int MODE, bool SH>
__device__ __forceinline__ T diff_terms(const KdiffArgs<T>& p, T r2, T da, T db, T other, bool same) {
    T s1 = T(0), s2 = T(0), lin = T(0);
    for (int t = 0; t < p.nterms; ++t) {
        const int kind = p.terms[t].kind;
        const T c = p.terms[t].ils2;
        const T vc = p.terms[t].variance * c;
        const T q = r2 * c;
        if (kind == GPK_K_EQ) {
            const T e = gpk_exp<T>(T(-0.5) * q);
            s1 += vc * T(-0.5) * e;
            if (MODE == MODE_DXY) s2 += vc * c * T(0.25) * e;
        } else if (kind == GPK_K_MATERN32) {
            const T s = gpk_sqrtk<T>(T(3) * q);
            const T e = gpk_exp<T>(-s);
            s1 += vc * T(-1.5) * e;
            if (MODE == MODE_DXY) s2 += vc * c * T(2.25) * e * (s > T(0) ? T(1) / s : T(0));
        } else if (kind == GPK_K_MATERN52) {
            const T s = gpk_sqrtk<T>(T(5) * q);
            const T e = gpk_exp<T>(-s);
            s1 += vc * T(-5.0 / 6.0) * (T(1) + s) * e;
            if (MODE == MODE_DXY) s2 += vc * c * T(25.0 / 12.0) * e;
        } else if (kind == GPK_K_LINEAR) {
            lin += vc;
        } else if (SH && kind == GPK_K_RQ) {
            // (1 + u)^(-alpha - 1) and (1 + u)^(-alpha - 2), u = q / (2 alpha), through exp and log1p: exponents <= 0 like every other here
            const T l = gpk_log1p<T>(q * p.hshape[t]);
            s1 += vc * T(-0.5) * gpk_exp<T>(-p.shape1[t] * l);
            if (MODE == MODE_DXY) s2 += vc * c * p.rq2[t] * gpk_exp<T>(-p.shape2[t] * l);
        }
        // (GPK_K_CONST: nothing; the kinds without a derivative never get here -- the launcher refuses them)
    }
    if (MODE == MODE_DX) return T(2) * s1 * da + lin * other;
    if (MODE == MODE_DY) return T(-2) * s1 * db + lin * other;
    const T val = T(-4) * s2 * (da * db);
    return same ? val + (lin - T(2) * s1) : val;
}

// One tile per workgroup, the input dimensions in chunks of DC (any d); the selected coordinates are fetched beside the chunks.
template <typename T, int MODE, bool SH, int DC>
__global__ __launch_bounds__(256) void kdiff_kernel(KdiffArgs<T> p) {
    typedef typename Traits<T>::vec_t vec_t;
    constexpr int VEC = Traits<T>::VEC;
    constexpr int TN = 64 * VEC;
    __shared__ T xs[TM * DC];
    __shared__ T xsel[2][TM];       // x[row][dim_x], x[row][dim_y] of the tile's rows

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int row0 = blockIdx.y * TM;
    const int col0 = blockIdx.x * TN;
    if (p.lower_only && col0 > row0 + TM - 1) return;

    const int64_t b = blockIdx.z;
    const T* __restrict__ X = p.X + b * p.sX;
    const T* __restrict__ Y = p.Y + b * p.sY;
    T* __restrict__ out = p.out + b * p.sO;

    const int colb = col0 + lane * VEC;   // first of this lane's VEC columns

    if (tid < 2 * TM) {      // (published by the first barrier of the chunk loop; d >= 1: a selected dimension exists)
        const int which = tid / TM, r = tid % TM, row = row0 + r;
        const int dim = which ? p.dim_y : p.dim_x;
        xsel[which][r] = (row < p.n && dim >= 0) ? X[(int64_t)row * p.ldx + dim] : T(0);
    }
    T ya[VEC], yb[VEC];      // y[col][dim_x], y[col][dim_y] of this lane's columns
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
        const int col = colb + v;
        ya[v] = (MODE != MODE_DY && col < p.m) ? Y[(int64_t)col * p.ldy + p.dim_x] : T(0);
        yb[v] = (MODE != MODE_DX && col < p.m) ? Y[(int64_t)col * p.ldy + p.dim_y] : T(0);
    }

    T r2[RW][VEC];
#pragma unroll
    for (int r = 0; r < RW; ++r)
#pragma unroll
        for (int v = 0; v < VEC; ++v) r2[r][v] = T(0);

    for (int dc = 0; dc < p.d; dc += DC) {
        __syncthreads();
        if (tid < TM * DC) {   // stage X chunk: TM*DC <= 256 elements, one per thread
            const int r = tid / DC, j = tid % DC;
            const int row = row0 + r;
            xs[tid] = (row < p.n && dc + j < p.d) ? X[(int64_t)row * p.ldx + dc + j] : T(0);
        }
        T yv[VEC][DC];
#pragma unroll
        for (int v = 0; v < VEC; ++v)
#pragma unroll
            for (int j = 0; j < DC; ++j) {
                const int col = colb + v;
                yv[v][j] = (col < p.m && dc + j < p.d) ? Y[(int64_t)col * p.ldy + dc + j] : T(0);
            }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < RW; ++r) {
            const int rl = wave * RW + r;
#pragma unroll
            for (int j = 0; j < DC; ++j) {
                const T xv = xs[rl * DC + j];
#pragma unroll
                for (int v = 0; v < VEC; ++v) {
                    const T df = xv - yv[v][j];
                    r2[r][v] += df * df;
                }
            }
        }
    }

    const bool same = p.dim_x == p.dim_y;
#pragma unroll
    for (int r = 0; r < RW; ++r) {
        const int rl = wave * RW + r;
        const int row = row0 + rl;
        if (row >= p.n) continue;
        const T xa = xsel[0][rl], xb = xsel[1][rl];
        T vals[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
            const int col = colb + v;
            T val = diff_terms<T, MODE, SH>(p, r2[r][v], xa - ya[v], xb - yb[v], MODE == MODE_DX ? ya[v] : xb, same);
            if (p.symmetric && col == row) kmat_add_diag(p, b, row, val);
            vals[v] = val;
        }
        T* o = out + (int64_t)row * p.ld + colb;
        if (p.vec_ok && colb + VEC <= p.m) {
            vec_t w;
            if (p.accumulate) {
                w = *reinterpret_cast<const vec_t*>(o);
#pragma unroll
                for (int v = 0; v < VEC; ++v) w[v] += vals[v];
            } else {
#pragma unroll
                for (int v = 0; v < VEC; ++v) w[v] = vals[v];
            }
            *reinterpret_cast<vec_t*>(o) = w;
        } else {
#pragma unroll
            for (int v = 0; v < VEC; ++v)
                if (colb + v < p.m) o[v] = p.accumulate ? o[v] + vals[v] : vals[v];
        }
    }
}

// Row-band kernel (d <= DC <= 8), the walk of kmat_band_kernel: the band's X rows staged once, Y tiles double-buffered through
// LDS (dimension-major), the next tile's Y in flight under this tile's arithmetic, CT back-to-back wave-stores per row.  The selected
// coordinates are already there: x[a], x[b] in the staged rows, y[a], y[b] as two more vector reads of the staged Y tile.
template <typename T, int MODE, bool SH, int DC>
__global__ __launch_bounds__(256) void kdiff_band_kernel(KdiffArgs<T> p) {
    typedef typename Traits<T>::vec_t vec_t;
    constexpr int VEC = Traits<T>::VEC;
    constexpr int TN = 64 * VEC;
    constexpr int TNP = TN + 4;                 // LDS row pitch of the transposed Y tile (bank spread of the staging writes)
    constexpr int YL = (TN * DC + 255) / 256;   // Y elements each thread stages per column tile
    __shared__ T xs[TM * DC];
    __shared__ __attribute__((aligned(16))) T ys[2][DC * TNP];   // Y tile, dimension-major: ys[j][c]

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int by = blockIdx.y, bx = blockIdx.x;
    if (p.compact) {
        gpk_kmat_compact_decode((int)blockIdx.x, p.nbands, p.compact, by, bx);
        if (by >= p.nbands) return;
    }
    const int row0 = by * TM;
    const int CT = p.ct;
    const int ct0 = bx * CT;
    if (p.lower_only && ct0 * TN > row0 + TM - 1) return;

    const int64_t b = blockIdx.z;
    const T* __restrict__ X = p.X + b * p.sX;
    const T* __restrict__ Y = p.Y + b * p.sY;
    T* __restrict__ out = p.out + b * p.sO;

    kmat_stage_band_x<T, DC>(p, X, tid, row0, xs);
    T stage[YL];
    auto fetch_y = [&](int col0) {      // consecutive lanes fetch consecutive elements of the (contiguous) Y tile
#pragma unroll
        for (int k = 0; k < YL; ++k) {
            const int idx = tid + 256 * k;
            const int c = idx / DC, j = idx % DC;
            const int col = col0 + c;
            stage[k] = (idx < TN * DC && col < p.m && j < p.d) ? Y[(int64_t)col * p.ldy + j] : T(0);
        }
    };
    auto commit_y = [&](int buf) {
#pragma unroll
        for (int k = 0; k < YL; ++k) {
            const int idx = tid + 256 * k;
            if (idx < TN * DC) ys[buf][(idx % DC) * TNP + idx / DC] = stage[k];
        }
    };
    fetch_y(ct0 * TN);
    commit_y(0);
    __syncthreads();

    // (uniform; a dimension that is not differentiated reads dimension 0 and the mode never uses the value)
    const int ja = MODE != MODE_DY ? p.dim_x : 0, jb = MODE != MODE_DX ? p.dim_y : 0;
    const bool same = p.dim_x == p.dim_y;

    for (int c = 0; c < CT; ++c) {
        const int col0 = (ct0 + c) * TN;
        if (col0 >= p.m || (p.lower_only && col0 > row0 + TM - 1)) break;       // (uniform over the workgroup)
        const bool more = (c + 1 < CT) && (col0 + TN < p.m) && !(p.lower_only && col0 + TN > row0 + TM - 1);
        if (more) fetch_y(col0 + TN);                 // next tile's Y: in flight under this tile's arithmetic
        T yv[DC][VEC];
#pragma unroll
        for (int j = 0; j < DC; ++j) {
            const vec_t w = *reinterpret_cast<const vec_t*>(&ys[c & 1][j * TNP + lane * VEC]);
#pragma unroll
            for (int v = 0; v < VEC; ++v) yv[j][v] = w[v];
        }
        T ya[VEC], yb[VEC];
        {
            const vec_t wa = *reinterpret_cast<const vec_t*>(&ys[c & 1][ja * TNP + lane * VEC]);
            const vec_t wb = *reinterpret_cast<const vec_t*>(&ys[c & 1][jb * TNP + lane * VEC]);
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                ya[v] = wa[v];
                yb[v] = wb[v];
            }
        }
        const int colb = col0 + lane * VEC;
        const bool has_diag = p.symmetric && col0 <= row0 + TM - 1 && col0 + TN > row0;   // (uniform) only such tiles touch the diagonal
#pragma unroll
        for (int r = 0; r < RW; ++r) {
            const int rl = wave * RW + r;
            const int row = row0 + rl;
            if (row >= p.n) continue;      // (wave-uniform; no barrier inside the row loop)
            T xr[DC];              // this row of the band: wave-uniform LDS broadcast reads
#pragma unroll
            for (int j = 0; j < DC; ++j) xr[j] = xs[rl * DC + j];
            const T xa = xs[rl * DC + ja], xb = xs[rl * DC + jb];
            T vals[VEC];
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                T r2 = T(0);
#pragma unroll
                for (int j = 0; j < DC; ++j) {
                    const T df = xr[j] - yv[j][v];
                    r2 += df * df;
                }
                T val = diff_terms<T, MODE, SH>(p, r2, xa - ya[v], xb - yb[v], MODE == MODE_DX ? ya[v] : xb, same);
                if (has_diag && colb + v == row) kmat_add_diag(p, b, row, val);
                vals[v] = val;
            }
            T* o = out + (int64_t)row * p.ld + colb;
            if (p.vec_ok && colb + VEC <= p.m) {
                vec_t w;
                if (p.accumulate) {
                    w = *reinterpret_cast<const vec_t*>(o);
#pragma unroll
                    for (int v = 0; v < VEC; ++v) w[v] += vals[v];
                    *reinterpret_cast<vec_t*>(o) = w;
                } else {
#pragma unroll
                    for (int v = 0; v < VEC; ++v) w[v] = vals[v];
                    __builtin_nontemporal_store(w, reinterpret_cast<vec_t*>(o));     // written once, read by a later kernel
                }
            } else {
#pragma unroll
                for (int v = 0; v < VEC; ++v)
                    if (colb + v < p.m) o[v] = p.accumulate ? o[v] + vals[v] : vals[v];
            }
        }
        if (more) commit_y((c + 1) & 1);     // the other buffer: nobody reads it during this iteration
        __syncthreads();
    }
}

template <typename T, int MODE, bool SH>
void launch_mode(const KdiffArgs<T>& a, bool band, dim3 grid, hipStream_t stream) {
#define GPK_KDIFF(KERNEL, DCV) hipLaunchKernelGGL((KERNEL<T, MODE, SH, DCV>), grid, dim3(256), 0, stream, a)
    if (band) GPK_KMAT_DC(a.d, GPK_KDIFF, kdiff_band_kernel);
    else GPK_KMAT_DC(a.d, GPK_KDIFF, kdiff_kernel);
#undef GPK_KDIFF
}

}  // namespace

// terms: host arrays of length nterms.  Error codes: the argument positions of gpk_kmat_diff (include/gpk.h); every argument is
// checked before an empty problem returns GPK_OK.
template <typename T>
int gpk_kmat_diff_launch(const int* kinds, const double* variances, const double* inv_ls, const double* shapes, int nterms,
                         int dim_x, int dim_y, const T* X, int64_t n, int64_t ldx, int64_t sX, const T* Y, int64_t m, int64_t ldy,
                         int64_t sY, int d, T* out, int64_t ld, int64_t sO, int64_t batch, int lower_only,
                         int symmetric, double diag_add, const T* diag_vec, int64_t sDiag, int accumulate,
                         hipStream_t stream) {
    if (nterms < 0 || nterms > GPK_MAX_TERMS) return GPK_ERR_ARG(6);
    bool shaped = false;
    for (int t = 0; t < nterms; ++t) {
        const int k = kinds[t];
        if (k != GPK_K_EQ && k != GPK_K_MATERN32 && k != GPK_K_MATERN52 && k != GPK_K_LINEAR && k != GPK_K_CONST && k != GPK_K_RQ)
            return GPK_ERR_ARG(2);      // Matern12 and Delta have no derivative; unknown kinds
        if (k == GPK_K_RQ) {
            shaped = true;
            if (shapes == nullptr) return GPK_ERR_ARG(1);       // (gpk_kmat's rules for `shapes`: -1 without the array, -5 for alpha <= 0)
            if (!(shapes[t] > 0)) return GPK_ERR_ARG(5);
        }
    }
    if (d < 0) return GPK_ERR_ARG(17);
    if (dim_x < -1 || dim_x >= d || (dim_x < 0 && dim_y < 0)) return GPK_ERR_ARG(7);
    if (dim_y < -1 || dim_y >= d) return GPK_ERR_ARG(8);
    if ((symmetric || lower_only) && !(dim_x == dim_y && dim_x >= 0)) return GPK_ERR_ARG(23);      // the one-sided blocks are not symmetric
    if (n > INT32_MAX) return GPK_ERR_ARG(10);
    if (m > INT32_MAX) return GPK_ERR_ARG(14);
    if (batch > 65535) return GPK_ERR_ARG(21);
    const int64_t gy = gpk_cdiv(n > 0 ? n : 1, TM);
    if (gy > 65535) return GPK_ERR_ARG(10);
    if (n <= 0 || m <= 0 || batch <= 0) return GPK_OK;
    constexpr int VEC = Traits<T>::VEC;
    KdiffArgs<T> a;
    a.X = X; a.Y = Y; a.out = out; a.diag_vec = diag_vec;
    a.ldx = ldx; a.ldy = ldy; a.sX = sX; a.sY = sY; a.ld = ld; a.sO = sO; a.sDiag = sDiag;
    a.n = (int)n; a.m = (int)m; a.d = d;
    a.dim_x = dim_x; a.dim_y = dim_y;
    a.nterms = nterms;
    gpk_pack_terms(a.terms, kinds, variances, inv_ls, nterms, true);
    for (int t = 0; t < GPK_MAX_TERMS; ++t) {
        const bool rq = t < nterms && kinds[t] == GPK_K_RQ;
        a.hshape[t] = rq ? (T)(0.5 / shapes[t]) : T(0);
        a.shape1[t] = rq ? (T)(shapes[t] + 1.0) : T(0);
        a.shape2[t] = rq ? (T)(shapes[t] + 2.0) : T(0);
        a.rq2[t] = rq ? (T)((shapes[t] + 1.0) / (4.0 * shapes[t])) : T(0);
    }
    a.diag_add = (T)diag_add;
    a.symmetric = symmetric; a.lower_only = lower_only; a.accumulate = accumulate;
    a.vec_ok = ((uintptr_t)out % 16 == 0) && (ld % VEC == 0) && (sO % VEC == 0);
    const bool band = d <= 8 && g_kdiff_band;
    const KmatPlan plan = gpk_kmat_plan(n, m, batch, VEC, lower_only, symmetric, band, g_kdiff_compact);
    a.ct = plan.ct; a.nbands = plan.nbands; a.compact = plan.compact;
    const dim3 grid(plan.gx, plan.gy, plan.gz);
    const int mode = dim_y < 0 ? MODE_DX : dim_x < 0 ? MODE_DY : MODE_DXY;
    if (shaped) {
        if (mode == MODE_DX) launch_mode<T, MODE_DX, true>(a, band, grid, stream);
        else if (mode == MODE_DY) launch_mode<T, MODE_DY, true>(a, band, grid, stream);
        else launch_mode<T, MODE_DXY, true>(a, band, grid, stream);
    } else {
        if (mode == MODE_DX) launch_mode<T, MODE_DX, false>(a, band, grid, stream);
        else if (mode == MODE_DY) launch_mode<T, MODE_DY, false>(a, band, grid, stream);
        else launch_mode<T, MODE_DXY, false>(a, band, grid, stream);
    }
    GPK_CHECK_LAUNCH();
    return GPK_OK;
}

#define GPK_INST(T)                                                                                                          \
    template int gpk_kmat_diff_launch<T>(const int*, const double*, const double*, const double*, int, int, int, const T*, \
                                         int64_t, int64_t, int64_t, const T*, int64_t, int64_t, int64_t, int, T*, int64_t,  \
                                         int64_t, int64_t, int, int, double, const T*, int64_t, int, hipStream_t);
GPK_INST(double)
GPK_INST(float)
