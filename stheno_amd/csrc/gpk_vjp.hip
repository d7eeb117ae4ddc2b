// gpk_vjp.hip -- kernel-hyperparameter VJP of the GP log-density ("next" row 8(f)-1:
// hyper-parameter learning, reference usage readme_example13_optimisation_torch.py:47-53).
//
// With  G = d logpdf / dK = 1/2 (A diag(g) A^T - s K^{-1})   (A = K^{-1} r, N x C;
// g = upstream gradients per column, s = sum(g)),  the gradient w.r.t. the parameters of
//   K_ij = sum_t v_t kappa_t(q_t),  q_t = |x_i - x_j|^2 / l_t^2   (or <x_i, x_j> / l_t^2)
// is  d/dv_t = sum_ij G_ij kappa_t,   d/dl_t = -2 v_t / l_t * sum_ij G_ij kappa_t'(q) q,
// d/dnoise_i = G_ii.  One pass over the LOWER triangle of K^{-1} (symmetry: off-diagonal
// entries count twice): pairwise distances are recomputed from x, G is never stored.
// HBM-bound: reads N^2/2 elements once.  Output: per-workgroup partial sums
// [nblocks][2 T + 1] (S1_t, S2_t, trace(G)) -- summed by the caller -- and diag(G).
//
// A term table with a kind that has a SHAPE parameter (rational quadratic: alpha) launches the same kernels instantiated with SH = true,
// which know GPK_K_RQ and carry a third sum per term, S3_t = sum_ij G_ij d kappa_t / d alpha_t, in partial rows of 3 T + 1 elements.
// GPK_K_DELTA (1 where q < epsilon, else 0; epsilon in `shape`) lives there too: piecewise constant, so S2_t = S3_t = 0 and no d/dx.
// The SH = false instantiations are what every other term table launches: the code they have always been.
#include "gpk_common.hpp"

namespace {

constexpr int VT = 64;    // tile edge
constexpr int VDC = 8;    // input dims per staged chunk
constexpr int VMAXC = 8;  // max columns of A

template <typename T>
struct VjpArgs {
    const T* X;
    const T* Kinv;
    const T* A;
    T* partial;
    T* diagG;
    int64_t ldx, ldk, lda;
    int n, d, C, nterms, ntile;
    int kind[GPK_MAX_TERMS];
    T ils2[GPK_MAX_TERMS];
    T g[VMAXC];
    T s;
    T shape[GPK_MAX_TERMS];    // (SH only; behind everything else)
};

template <typename T>
__device__ __forceinline__ T vexp(T x);
template <>
__device__ __forceinline__ double vexp<double>(double x) { return exp(x); }
template <>
__device__ __forceinline__ float vexp<float>(float x) { return expf(x); }
template <typename T>
__device__ __forceinline__ T vsqrt(T x);
template <>
__device__ __forceinline__ double vsqrt<double>(double x) { return sqrt(x); }
template <>
__device__ __forceinline__ float vsqrt<float>(float x) { return sqrtf(x); }

// kappa(q) and kappa'(q) * q
template <typename T>
__device__ __forceinline__ void kappa_and_dq(int kind, T q, T& k, T& dkq) {
    if (kind == GPK_K_EQ) {
        k = vexp<T>(T(-0.5) * q);
        dkq = T(-0.5) * q * k;
    } else if (kind == GPK_K_MATERN12) {
        const T r = vsqrt<T>(q);
        k = vexp<T>(-r);
        dkq = T(-0.5) * r * k;
    } else if (kind == GPK_K_MATERN32) {
        const T s = vsqrt<T>(T(3) * q), e = vexp<T>(-s);
        k = (T(1) + s) * e;
        dkq = T(-0.5) * s * s * e;
    } else if (kind == GPK_K_MATERN52) {
        const T s = vsqrt<T>(T(5) * q), e = vexp<T>(-s);
        k = (T(1) + s + s * s * T(1.0 / 3.0)) * e;
        dkq = -(s * s * T(1.0 / 6.0)) * (T(1) + s) * e;
    } else if (kind == GPK_K_LINEAR) {
        k = q;
        dkq = q;
    } else {
        k = T(1);
        dkq = T(0);
    }
}

template <typename T>
__device__ __forceinline__ T vlog1p(T x);
template <>
__device__ __forceinline__ double vlog1p<double>(double x) { return log1p(x); }
template <>
__device__ __forceinline__ float vlog1p<float>(float x) { return log1pf(x); }

// rational quadratic kappa = (1 + u)^(-alpha), u = q / (2 alpha):  kappa' = -kappa / (2 (1 + u)),  kappa' q,
// d kappa / d alpha = kappa (u / (1 + u) - log1p(u))
template <typename T>
__device__ __forceinline__ void kappa_rq(T q, T a, T& k, T& dkq, T& dk, T& da) {
    const T u = q * (T(0.5) / a);
    const T lg = vlog1p<T>(u), ri = T(1) / (T(1) + u);
    k = vexp<T>(-a * lg);
    dk = T(-0.5) * k * ri;
    dkq = dk * q;
    da = k * (u * ri - lg);
}

// Delta: 1 within epsilon (in q), else 0; NaN stays NaN.  Piecewise constant: no derivative in q, x or epsilon.
template <typename T>
__device__ __forceinline__ T kappa_delta(T q, T eps) {
    return q != q ? q : (q < eps ? T(1) : T(0));
}

template <typename T, bool SH>
__global__ __launch_bounds__(256) void kmat_vjp_kernel(VjpArgs<T> p) {
    constexpr int NS = SH ? 3 : 2;      // sums per term
    __shared__ T xi[VT * VDC], xj[VT * VDC], ai[VT * VMAXC], aj[VT * VMAXC];
    __shared__ T red[4 * (2 * GPK_MAX_TERMS + 1)];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // lower-triangular tile enumeration
    const int bid = blockIdx.x;
    int ti = (int)((sqrtf(8.f * (float)bid + 1.f) - 1.f) * 0.5f);
    while ((ti + 1) * (ti + 2) / 2 <= bid) ++ti;
    while (ti * (ti + 1) / 2 > bid) --ti;
    const int tj = bid - ti * (ti + 1) / 2;
    const int i0 = ti * VT, j0 = tj * VT;
    const int ty = tid >> 4, tx = tid & 15;     // 16 x 16 threads, 4 x 4 elements each

    T r2[4][4], dt[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) r2[a][b] = dt[a][b] = T(0);

    for (int dc = 0; dc < p.d; dc += VDC) {
        __syncthreads();
        for (int idx = tid; idx < VT * VDC; idx += 256) {
            const int r = idx / VDC, c = idx % VDC;
            xi[idx] = (i0 + r < p.n && dc + c < p.d) ? p.X[(int64_t)(i0 + r) * p.ldx + dc + c] : T(0);
            xj[idx] = (j0 + r < p.n && dc + c < p.d) ? p.X[(int64_t)(j0 + r) * p.ldx + dc + c] : T(0);
        }
        __syncthreads();
#pragma unroll
        for (int c = 0; c < VDC; ++c) {
            T a[4], b[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                a[q] = xi[(ty * 4 + q) * VDC + c];
                b[q] = xj[(tx * 4 + q) * VDC + c];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const T df = a[u] - b[v];
                    r2[u][v] += df * df;
                    dt[u][v] += a[u] * b[v];
                }
        }
    }
    // alphas of the tile rows / columns
    for (int idx = tid; idx < VT * VMAXC; idx += 256) {
        const int r = idx / VMAXC, c = idx % VMAXC;
        ai[idx] = (i0 + r < p.n && c < p.C) ? p.A[(int64_t)(i0 + r) * p.lda + c] : T(0);
        aj[idx] = (j0 + r < p.n && c < p.C) ? p.A[(int64_t)(j0 + r) * p.lda + c] : T(0);
    }
    __syncthreads();

    // G for this thread's 4 x 4 elements (weighted for the symmetric double count)
    T Gw[4][4];
    T tr = T(0);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int i = i0 + ty * 4 + u;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int j = j0 + tx * 4 + v;
            Gw[u][v] = T(0);
            if (i < p.n && j < p.n && j <= i) {
                T aa = T(0);
                for (int c = 0; c < p.C; ++c) aa += p.g[c] * ai[(ty * 4 + u) * VMAXC + c] * aj[(tx * 4 + v) * VMAXC + c];
                const T G = T(0.5) * (aa - p.s * p.Kinv[(int64_t)i * p.ldk + j]);
                Gw[u][v] = (i == j) ? G : T(2) * G;
                if (i == j) {
                    tr += G;
                    p.diagG[i] = G;
                }
            }
        }
    }
    // per term: two block-wide sums (no per-thread accumulator array -> no scratch)
    T* out = p.partial + (int64_t)bid * (NS * GPK_MAX_TERMS + 1);
    for (int t = 0; t <= p.nterms; ++t) {
        T s1 = T(0), s2 = T(0), s3 = T(0);
        if (t < p.nterms) {
            const int kind = p.kind[t];
            const T ils2 = p.ils2[t];
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const T q = (kind == GPK_K_LINEAR ? dt[u][v] : r2[u][v]) * ils2;
                    T k, dkq;
                    if (SH && kind == GPK_K_RQ) {
                        T dk, da;
                        kappa_rq<T>(q, p.shape[t], k, dkq, dk, da);
                        s3 += Gw[u][v] * da;
                    } else if (SH && kind == GPK_K_DELTA) {
                        k = kappa_delta<T>(q, p.shape[t]);
                        dkq = T(0);
                    } else {
                        kappa_and_dq<T>(kind, q, k, dkq);
                    }
                    s1 += Gw[u][v] * k;
                    s2 += Gw[u][v] * dkq;
                }
        } else {
            s1 = tr;     // last round carries the trace
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            s1 += __shfl_xor(s1, o, 64);
            s2 += __shfl_xor(s2, o, 64);
            if (SH) s3 += __shfl_xor(s3, o, 64);
        }
        __syncthreads();
        if (lane == 0) {
            red[wave * 2] = s1;
            red[wave * 2 + 1] = s2;
            if (SH) red[8 + wave] = s3;
        }
        __syncthreads();
        if (tid == 0) {
            const T a1 = red[0] + red[2] + red[4] + red[6], a2 = red[1] + red[3] + red[5] + red[7];
            if (t < p.nterms) {
                out[NS * t] = a1;
                out[NS * t + 1] = a2;
                if (SH) out[NS * t + 2] = red[8] + red[9] + red[10] + red[11];
            } else {
                out[NS * GPK_MAX_TERMS] = a1;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Dense-G variant (gradient of the pseudo-point ELBO, row 8(f)-1): the cotangent of a RECTANGULAR
// kernel matrix K(X, Y) (n x m) is given explicitly,
//     Geff_ij = G_ij * colscale_j + w_i * b_j        (colscale / (w, b) optional),
// and one pass produces
//   * per-term sums   S1_t = sum Geff kappa_t,  S2_t = sum Geff kappa_t'(q) q      (-> d/dv_t, d/dl_t),
//   * column sums     colsum_j = sum_i Geff_ij K_ij                                (-> d/d noise_j),
//   * d/dX            gradx_i = sum_j Geff_ij dK_ij/dx_i   (first argument; input dim <= 8).
// A workgroup owns a 64-row tile and a CHUNK of 64-column tiles: the d/dX accumulators stay in
// registers across the chunk, column sums leave per row tile; partial results are summed by the
// caller (deterministic, no atomics).  HBM-bound: G is read exactly once.
// A BATCH of independent problems under one term table is the third grid dimension: entry e = blockIdx.z reads its inputs at
// e * (batch stride) elements (64-bit offsets; a stride of 0 shares one operand among the entries) and writes its own packed block of
// every output.  The column chunks shrink in number as the batch grows (gpk_kmat_vjp_dense_grid_impl), so with many entries a
// workgroup walks a whole row of column tiles with its d/dX accumulators in registers.  batch = 1 is the unbatched launch: entry 0,
// offsets 0, the grid and every summation order it has always had.
constexpr int DT = 64;

template <typename T>
struct VjpDenseArgs {
    const T *X, *Y, *G, *cs, *w, *b;
    T *partial, *colsum, *gradx;
    int64_t ldx, ldy, ldg;
    int64_t sx, sy, sg, scs, sw, sb;      // batch strides of the inputs, in elements (0: shared by the entries)
    int n, m, d, nterms, tiles_per_chunk, ctiles, nchunks;
    int kind[GPK_MAX_TERMS];
    T ils2[GPK_MAX_TERMS], var[GPK_MAX_TERMS];
    T shape[GPK_MAX_TERMS];    // (SH only; behind everything else)
};

// kappa(q), kappa'(q) q and kappa'(q)   (kappa' of exp(-sqrt(q)) is singular at 0: reported as 0)
template <typename T>
__device__ __forceinline__ void kappa_all(int kind, T q, T& k, T& dkq, T& dk) {
    if (kind == GPK_K_EQ) {
        k = vexp<T>(T(-0.5) * q);
        dk = T(-0.5) * k;
        dkq = dk * q;
    } else if (kind == GPK_K_MATERN12) {
        const T r = vsqrt<T>(q);
        k = vexp<T>(-r);
        dkq = T(-0.5) * r * k;
        dk = r > T(0) ? T(-0.5) * k / r : T(0);
    } else if (kind == GPK_K_MATERN32) {
        const T s = vsqrt<T>(T(3) * q), e = vexp<T>(-s);
        k = (T(1) + s) * e;
        dk = T(-1.5) * e;
        dkq = dk * q;
    } else if (kind == GPK_K_MATERN52) {
        const T s = vsqrt<T>(T(5) * q), e = vexp<T>(-s);
        k = (T(1) + s + s * s * T(1.0 / 3.0)) * e;
        dk = T(-5.0 / 6.0) * (T(1) + s) * e;
        dkq = dk * q;
    } else if (kind == GPK_K_LINEAR) {
        k = q;
        dkq = q;
        dk = T(1);
    } else {
        k = T(1);
        dkq = T(0);
        dk = T(0);
    }
}

template <typename T, bool SH>
__global__ __launch_bounds__(256) void kmat_vjp_dense_kernel(VjpDenseArgs<T> p) {
    constexpr int NS = SH ? 3 : 2;      // sums per term
    __shared__ T xi[DT * VDC], yj[DT * VDC];
    __shared__ T csred[16 * DT];
    __shared__ T red[4 * NS * GPK_MAX_TERMS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ty = tid >> 4, tx = tid & 15;     // 16 x 16 threads, 4 x 4 elements each
    const int rt = blockIdx.x, chunk = blockIdx.y;
    const int i0 = rt * DT;
    const bool want_gx = p.gradx != nullptr;     // launcher guarantees d <= VDC then
    // this batch entry's operands (uniform: scalar registers); its outputs are packed [entry][...] with the unbatched shapes
    const int64_t e = blockIdx.z;
    const T* const X = p.X + e * p.sx;
    const T* const Y = p.Y + e * p.sy;
    const T* const G = p.G + e * p.sg;
    const T* const cs = p.cs != nullptr ? p.cs + e * p.scs : nullptr;
    const T* const w = p.w != nullptr ? p.w + e * p.sw : nullptr;
    const T* const b = p.b != nullptr ? p.b + e * p.sb : nullptr;
    T* const colsum = p.colsum != nullptr ? p.colsum + e * gridDim.x * p.m : nullptr;
    T* const gradx = want_gx ? p.gradx + e * p.nchunks * p.n * p.d : nullptr;

    T s1[GPK_MAX_TERMS], s2[GPK_MAX_TERMS], s3[SH ? GPK_MAX_TERMS : 1];
#pragma unroll
    for (int t = 0; t < GPK_MAX_TERMS; ++t) s1[t] = s2[t] = T(0);
    if (SH) {
#pragma unroll
        for (int t = 0; t < GPK_MAX_TERMS; ++t) s3[SH ? t : 0] = T(0);
    }
    T gx[4][VDC];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int c = 0; c < VDC; ++c) gx[u][c] = T(0);
    T wi[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int i = i0 + ty * 4 + u;
        wi[u] = (w != nullptr && i < p.n) ? w[i] : T(0);
    }

    const int ct_end = min((chunk + 1) * p.tiles_per_chunk, p.ctiles);
    for (int ct = chunk * p.tiles_per_chunk; ct < ct_end; ++ct) {
        const int j0 = ct * DT;
        T r2[4][4], dt[4][4];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) r2[a][b] = dt[a][b] = T(0);
        for (int dc = 0; dc < p.d; dc += VDC) {
            __syncthreads();
            for (int idx = tid; idx < DT * VDC; idx += 256) {
                const int r = idx / VDC, c = idx % VDC;
                xi[idx] = (i0 + r < p.n && dc + c < p.d) ? X[(int64_t)(i0 + r) * p.ldx + dc + c] : T(0);
                yj[idx] = (j0 + r < p.m && dc + c < p.d) ? Y[(int64_t)(j0 + r) * p.ldy + dc + c] : T(0);
            }
            __syncthreads();
#pragma unroll
            for (int c = 0; c < VDC; ++c) {
                T a[4], b[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    a[q] = xi[(ty * 4 + q) * VDC + c];
                    b[q] = yj[(tx * 4 + q) * VDC + c];
                }
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int v = 0; v < 4; ++v) {
                        const T df = a[u] - b[v];
                        r2[u][v] += df * df;
                        dt[u][v] += a[u] * b[v];
                    }
            }
        }
        // effective cotangent of this thread's 4 x 4 elements
        T Ge[4][4];
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int j = j0 + tx * 4 + v;
            const T csj = (cs != nullptr && j < p.m) ? cs[j] : T(1);
            const T bj = (b != nullptr && j < p.m) ? b[j] : T(0);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int i = i0 + ty * 4 + u;
                T g = T(0);
                if (i < p.n && j < p.m) g = G[(int64_t)i * p.ldg + j] * csj + wi[u] * bj;
                Ge[u][v] = g;
            }
        }
        T kfull[4][4], cS[4][4], cL[4][4];
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int v = 0; v < 4; ++v) kfull[u][v] = cS[u][v] = cL[u][v] = T(0);
#pragma unroll
        for (int t = 0; t < GPK_MAX_TERMS; ++t) {
            if (t < p.nterms) {
                const int kind = p.kind[t];
                const T ils2 = p.ils2[t], var = p.var[t];
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int v = 0; v < 4; ++v) {
                        const T q = (kind == GPK_K_LINEAR ? dt[u][v] : r2[u][v]) * ils2;
                        T k, dkq, dk;
                        if (SH && kind == GPK_K_RQ) {
                            T da;
                            kappa_rq<T>(q, p.shape[t], k, dkq, dk, da);
                            s3[SH ? t : 0] += Ge[u][v] * da;
                        } else if (SH && kind == GPK_K_DELTA) {
                            k = kappa_delta<T>(q, p.shape[t]);
                            dkq = dk = T(0);
                        } else {
                            kappa_all<T>(kind, q, k, dkq, dk);
                        }
                        s1[t] += Ge[u][v] * k;
                        s2[t] += Ge[u][v] * dkq;
                        kfull[u][v] += var * k;
                        if (kind == GPK_K_LINEAR)
                            cL[u][v] += var * ils2;
                        else
                            cS[u][v] += T(2) * var * ils2 * dk;
                    }
            }
        }
        // column sums over this row tile: 4 rows per thread, then the 16 ty-groups through LDS
        if (colsum != nullptr) {
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                T acc = T(0);
#pragma unroll
                for (int u = 0; u < 4; ++u) acc += Ge[u][v] * kfull[u][v];
                csred[ty * DT + tx * 4 + v] = acc;
            }
            __syncthreads();
            if (tid < DT) {
                T acc = T(0);
#pragma unroll
                for (int g = 0; g < 16; ++g) acc += csred[g * DT + tid];
                if (j0 + tid < p.m) colsum[(int64_t)rt * p.m + j0 + tid] = acc;
            }
        }
        // d/dx_i: sum_j Ge [ cS (x_i - y_j) + cL y_j ]     (xi / yj still hold the only d-chunk)
        if (want_gx) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                T sumS = T(0);
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    cS[u][v] *= Ge[u][v];
                    cL[u][v] = cL[u][v] * Ge[u][v] - cS[u][v];
                    sumS += cS[u][v];
                }
#pragma unroll
                for (int c = 0; c < VDC; ++c) {
                    T acc = sumS * xi[(ty * 4 + u) * VDC + c];
#pragma unroll
                    for (int v = 0; v < 4; ++v) acc += cL[u][v] * yj[(tx * 4 + v) * VDC + c];
                    gx[u][c] += acc;
                }
            }
        }
    }

    // per-term sums of the whole workgroup
    T* out = p.partial + ((e * gridDim.x + rt) * p.nchunks + chunk) * (NS * GPK_MAX_TERMS + 1);
#pragma unroll
    for (int t = 0; t < GPK_MAX_TERMS; ++t) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            s1[t] += __shfl_xor(s1[t], o, 64);
            s2[t] += __shfl_xor(s2[t], o, 64);
            if (SH) s3[SH ? t : 0] += __shfl_xor(s3[SH ? t : 0], o, 64);
        }
    }
    __syncthreads();
    if (lane == 0) {
#pragma unroll
        for (int t = 0; t < GPK_MAX_TERMS; ++t) {
            red[(wave * GPK_MAX_TERMS + t) * NS] = s1[t];
            red[(wave * GPK_MAX_TERMS + t) * NS + 1] = s2[t];
            if (SH) red[(wave * GPK_MAX_TERMS + t) * NS + 2] = s3[SH ? t : 0];
        }
    }
    __syncthreads();
    if (tid < NS * GPK_MAX_TERMS) {
        out[tid] = red[tid] + red[NS * GPK_MAX_TERMS + tid] + red[2 * NS * GPK_MAX_TERMS + tid] + red[3 * NS * GPK_MAX_TERMS + tid];
    } else if (tid == NS * GPK_MAX_TERMS) {
        out[tid] = T(0);
    }
    // d/dX: reduce over the 16 tx lanes of each row group, one partial per column chunk
    if (want_gx) {
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int c = 0; c < VDC; ++c) {
                T v = gx[u][c];
#pragma unroll
                for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
                const int i = i0 + ty * 4 + u;
                if (tx == 0 && i < p.n && c < p.d) gradx[((int64_t)chunk * p.n + i) * p.d + c] = v;
            }
    }
}

// The term table of either launch from the host arrays of the entry points, padded to GPK_MAX_TERMS with constant terms (`var`: dense variant only)
template <typename T>
void vjp_pack_terms(const int* kinds, const double* variances, const double* inv_ls, const double* shapes, int nterms, int* kind, T* ils2, T* var, T* shape) {
    for (int t = 0; t < GPK_MAX_TERMS; ++t) {
        kind[t] = t < nterms ? kinds[t] : GPK_K_CONST;
        ils2[t] = t < nterms ? (T)(inv_ls[t] * inv_ls[t]) : T(0);
        if (var != nullptr) var[t] = t < nterms ? (T)variances[t] : T(0);
        shape[t] = (t < nterms && (kinds[t] == GPK_K_RQ || kinds[t] == GPK_K_DELTA)) ? (T)shapes[t] : T(1);
    }
}

}  // namespace

// Row tiles, column chunks and column tiles per chunk of a launch over `batch` entries: the chunks aim at ~2048 workgroups in all,
// nchunks = clamp(cdiv(2048, rowtiles * batch), 1, column tiles), evened out over the column tiles.  batch = 1: the unbatched rule.
void gpk_kmat_vjp_dense_grid_impl(int64_t n, int64_t m, int64_t batch, int64_t* rowtiles, int64_t* nchunks, int64_t* tiles_per_chunk) {
    const int64_t rt = gpk_cdiv(n > 0 ? n : 1, DT), ct = gpk_cdiv(m > 0 ? m : 1, DT);
    int64_t nc = gpk_cdiv(2048, rt * (batch > 0 ? batch : 1));
    if (nc > ct) nc = ct;
    if (nc < 1) nc = 1;
    const int64_t tpc = gpk_cdiv(ct, nc);
    *rowtiles = rt;
    *nchunks = gpk_cdiv(ct, tpc);
    if (tiles_per_chunk) *tiles_per_chunk = tpc;
}

// SH = some term is RQ or Delta: the instantiation that reads `shapes` for them and writes the 3-wide partial rows.  The one launcher
// of kmat_vjp_dense_kernel: gpk_kmat_vjp_dense is its batch = 1 call (batch strides 0).  Status codes: include/gpk.h.
template <typename T>
int gpk_kmat_vjp_dense_batch_launch(const int* kinds, const double* variances, const double* inv_ls, const double* shapes, int nterms,
                                    const T* X, int64_t n, int64_t ldx, int64_t sx, const T* Y, int64_t m, int64_t ldy, int64_t sy, int d,
                                    const T* G, int64_t ldg, int64_t sg, const T* colscale, int64_t s_cs, const T* w, int64_t s_w,
                                    const T* b, int64_t s_b, T* partial, T* colsum, T* gradx, int64_t batch, hipStream_t stream) {
    if (n <= 0 || m <= 0) return GPK_OK;
    if (nterms < 0 || nterms > GPK_MAX_TERMS) return GPK_ERR_ARG(5);
    bool shaped;
    if (const int st = gpk_check_terms(kinds, shapes, nterms, true, GPK_ERR_ARG(4), &shaped)) return st;
    if (n > INT32_MAX || m > INT32_MAX) return GPK_ERR_ARG(7);
    if ((w == nullptr) != (b == nullptr)) return GPK_ERR_ARG(17);
    if (gradx != nullptr && d > VDC) return GPK_ERR_ARG(12);     // d/dX is implemented for d <= 8
    if (batch > 65535) return GPK_ERR_ARG(28);                   // (the grid's third dimension)
    if (batch <= 0) return GPK_OK;
    VjpDenseArgs<T> a;
    a.X = X; a.Y = Y; a.G = G; a.cs = colscale; a.w = w; a.b = b;
    a.partial = partial; a.colsum = colsum; a.gradx = gradx;
    a.ldx = ldx; a.ldy = ldy; a.ldg = ldg;
    a.sx = sx; a.sy = sy; a.sg = sg; a.scs = s_cs; a.sw = s_w; a.sb = s_b;
    a.n = (int)n; a.m = (int)m; a.d = d; a.nterms = nterms;
    int64_t rt, nc, tpc;
    gpk_kmat_vjp_dense_grid_impl(n, m, batch, &rt, &nc, &tpc);
    a.tiles_per_chunk = (int)tpc; a.nchunks = (int)nc; a.ctiles = (int)gpk_cdiv(m, DT);
    vjp_pack_terms<T>(kinds, variances, inv_ls, shapes, nterms, a.kind, a.ils2, a.var, a.shape);
    if (nc > 65535) return GPK_ERR_ARG(9);
    const dim3 grid((unsigned)rt, (unsigned)nc, (unsigned)batch);
    if (shaped)
        hipLaunchKernelGGL((kmat_vjp_dense_kernel<T, true>), grid, dim3(256), 0, stream, a);
    else
        hipLaunchKernelGGL((kmat_vjp_dense_kernel<T, false>), grid, dim3(256), 0, stream, a);
    GPK_CHECK_LAUNCH();
    return GPK_OK;
}
template int gpk_kmat_vjp_dense_batch_launch<double>(const int*, const double*, const double*, const double*, int, const double*, int64_t,
                                                     int64_t, int64_t, const double*, int64_t, int64_t, int64_t, int, const double*,
                                                     int64_t, int64_t, const double*, int64_t, const double*, int64_t, const double*,
                                                     int64_t, double*, double*, double*, int64_t, hipStream_t);
template int gpk_kmat_vjp_dense_batch_launch<float>(const int*, const double*, const double*, const double*, int, const float*, int64_t,
                                                    int64_t, int64_t, const float*, int64_t, int64_t, int64_t, int, const float*, int64_t,
                                                    int64_t, const float*, int64_t, const float*, int64_t, const float*, int64_t, float*,
                                                    float*, float*, int64_t, hipStream_t);

// ---------------------------------------------------------------------------------------------
// VJP of a DERIVATIVE block (gpk_kmat_diff_vjp in gpk.h): the explicit cotangent g (n x m) of the block gpk_kmat_diff writes for the
// same (dim_x, dim_y) -- never formed here -- reduced to the per-term sums of the block's derivatives with respect to the variances,
// the scales and RQ's alpha, and (one-sided modes, d <= 8) to the gradient with respect to the row input.  The walk of
// kmat_vjp_dense_kernel: a workgroup owns a 64-row tile and a chunk of 64-column tiles, 4 x 4 elements per thread, the input
// dimensions staged in chunks of 8; the selected coordinates x[a], x[b] / y[a], y[b] are fetched beside the chunks.  With
// q = c r^2, D_a = x[a] - y[a], a block element is sum_t v_t beta_t:
//   d/dx_a:          beta = 2 c kappa' D_a                      c dbeta/dc = 2 c D_a (kappa' + q kappa'')
//   d/dy_b:          the same with -D_b
//   d2/dx_a dy_b:    beta = -4 c^2 kappa'' D_a D_b - 2 c kappa' [a == b]
//                    c dbeta/dc = -4 c^2 D_a D_b (2 kappa'' + q kappa''') - 2 c [a == b] (kappa' + q kappa'')
// and d beta / d alpha the same expressions on d kappa' / d alpha, d kappa'' / d alpha (RQ).  Linear: beta = c y[a] | c x[b] | c [a == b]
// and c dbeta/dc = beta; Const: nothing.  The mode, "some term is RQ" and "gradx is wanted" are template parameters: a one-sided launch
// without gradx never evaluates kappa'', a table without RQ never the logarithm.  gradx is summed in LDS by each row's owner thread, not
// in 32 more registers per thread: with eight terms x three sums in fp64 those spilled 200 to 340 bytes per lane to scratch memory in
// every fp64 gradx instantiation; this way one of them (RQ table, d/dy) is left with 32 bytes, the others with none.  The term table
// is walked term by term, as in kmat_vjp_dense_kernel: with the elements outermost the unrolled body of the RQ instantiations is past
// the compiler's size limit, the loop over this thread's rows stays rolled and its register arrays are indexed dynamically.
namespace {

enum { DMODE_DX = 0, DMODE_DY = 1, DMODE_DXY = 2 };

template <typename T>
struct VjpDiffArgs {
    const T *X, *Y, *G;
    T *partial, *gradx;
    int64_t ldx, ldy, ldg;
    int n, m, d, nterms, tiles_per_chunk, ctiles, nchunks;
    int dim_x, dim_y;
    int kind[GPK_MAX_TERMS];
    T ils2[GPK_MAX_TERMS], var[GPK_MAX_TERMS];
    T shape[GPK_MAX_TERMS];    // (SH only) RQ's alpha
};

// The profile of a stationary kind at q: k1 = kappa', k2 = kappa'', qk2 = q kappa'', m3 = 2 kappa'' + q kappa''' and (RQ) the
// derivatives of kappa' and kappa'' with respect to alpha.
//   eq         kappa''' = -kappa / 8
//   matern52   q kappa''' = -(25/24) s e^(-s)
//   matern32   q kappa'' = (3/4) s e^(-s),  2 kappa'' + q kappa''' = (9/8) (3 - s) / s e^(-s);  1 / s is taken as 0 where s is not
//              positive, as the forward kernel does (whatever multiplies it tends to 0 with the distance)
//   rq         P_k = (1 + u)^(-alpha - k) from exp(-(alpha + 1) log1p(u)) and 1 / (1 + u): every exponent <= 0;
//              q kappa''' = -kappa'' q (alpha + 2) / (2 alpha (1 + u)),  dP_k / dalpha = P_k ((alpha + k) u / (alpha (1 + u)) - log1p(u))
template <typename T, bool SH>
__device__ __forceinline__ void diff_profile(int kind, T q, T al, T& k1, T& k2, T& qk2, T& m3, T& k1a, T& k2a) {
    k1a = k2a = T(0);
    if (kind == GPK_K_EQ) {
        const T e = vexp<T>(T(-0.5) * q);
        k1 = T(-0.5) * e;
        k2 = T(0.25) * e;
        qk2 = q * k2;
        m3 = e * (T(0.5) - T(0.125) * q);
    } else if (kind == GPK_K_MATERN32) {
        const T s = vsqrt<T>(T(3) * q), e = vexp<T>(-s);
        const T is = s > T(0) ? T(1) / s : T(0);
        k1 = T(-1.5) * e;
        k2 = T(2.25) * e * is;
        qk2 = T(0.75) * s * e;
        m3 = T(1.125) * (T(3) - s) * e * is;
    } else if (kind == GPK_K_MATERN52) {
        const T s = vsqrt<T>(T(5) * q), e = vexp<T>(-s);
        k1 = T(-5.0 / 6.0) * (T(1) + s) * e;
        k2 = T(25.0 / 12.0) * e;
        qk2 = T(5.0 / 12.0) * s * s * e;
        m3 = e * (T(25.0 / 6.0) - T(25.0 / 24.0) * s);
    } else if (SH && kind == GPK_K_RQ) {
        const T h = T(0.5) / al, u = q * h;
        const T lg = vlog1p<T>(u), ri = T(1) / (T(1) + u);
        const T p1 = vexp<T>(-(al + T(1)) * lg), p2 = p1 * ri;
        const T w = T(2) * h * u * ri;                 // u / (alpha (1 + u))
        k1 = T(-0.5) * p1;
        k2 = (al + T(1)) * T(0.5) * h * p2;            // (alpha + 1) / (4 alpha) P_2
        qk2 = q * k2;
        m3 = k2 * (T(2) - q * ri * (al + T(2)) * h);
        k1a = T(-0.5) * p1 * ((al + T(1)) * w - lg);
        k2a = (al + T(1)) * T(0.5) * h * p2 * ((al + T(2)) * w - lg) - h * h * p2;
    } else {
        k1 = k2 = qk2 = m3 = T(0);
    }
}

template <typename T, int MODE, bool SH, bool GX>
__global__ __launch_bounds__(256) void kmat_diff_vjp_kernel(VjpDiffArgs<T> p) {
    constexpr int NS = SH ? 3 : 2;      // sums per term
    __shared__ T xi[DT * VDC], yj[DT * VDC];
    __shared__ T red[4 * NS * GPK_MAX_TERMS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ty = tid >> 4, tx = tid & 15;     // 16 x 16 threads, 4 x 4 elements each
    const int rt = blockIdx.x, chunk = blockIdx.y;
    const int i0 = rt * DT;
    const bool same = p.dim_x == p.dim_y;
    const int sel = MODE == DMODE_DY ? p.dim_y : p.dim_x;      // (GX: the one-sided modes) the differentiated dimension

    T s1[GPK_MAX_TERMS], s2[GPK_MAX_TERMS], s3[SH ? GPK_MAX_TERMS : 1];
#pragma unroll
    for (int t = 0; t < GPK_MAX_TERMS; ++t) s1[t] = s2[t] = T(0);
    if (SH) {
#pragma unroll
        for (int t = 0; t < GPK_MAX_TERMS; ++t) s3[SH ? t : 0] = T(0);
    }
    // (GX) d/dX of the tile's rows over this workgroup's chunk.  Row r belongs to the thread tx == 0 of its row group alone (it zeroes,
    // adds to and writes out its own 4 x VDC entries: no barrier), so no thread carries 32 more accumulators through the term table.
    __shared__ T gxs[GX ? DT * VDC : 1];
    if (GX && tx == 0) {
#pragma unroll
        for (int k = 0; k < 4 * VDC; ++k) gxs[GX ? ty * 4 * VDC + k : 0] = T(0);
    }
    T xa[4], xb[4];      // x[row][dim_x], x[row][dim_y] of this thread's rows
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int i = i0 + ty * 4 + u;
        xa[u] = (MODE != DMODE_DY && i < p.n) ? p.X[(int64_t)i * p.ldx + p.dim_x] : T(0);
        xb[u] = (MODE != DMODE_DX && i < p.n) ? p.X[(int64_t)i * p.ldx + p.dim_y] : T(0);
    }

    const int ct_end = min((chunk + 1) * p.tiles_per_chunk, p.ctiles);
    for (int ct = chunk * p.tiles_per_chunk; ct < ct_end; ++ct) {
        const int j0 = ct * DT;
        T ya[4], yb[4];      // y[col][dim_x], y[col][dim_y] of this thread's columns
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int j = j0 + tx * 4 + v;
            ya[v] = (MODE != DMODE_DY && j < p.m) ? p.Y[(int64_t)j * p.ldy + p.dim_x] : T(0);
            yb[v] = (MODE != DMODE_DX && j < p.m) ? p.Y[(int64_t)j * p.ldy + p.dim_y] : T(0);
        }
        T r2[4][4];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) r2[a][b] = T(0);
        for (int dc = 0; dc < p.d; dc += VDC) {
            __syncthreads();
            for (int idx = tid; idx < DT * VDC; idx += 256) {
                const int r = idx / VDC, c = idx % VDC;
                xi[idx] = (i0 + r < p.n && dc + c < p.d) ? p.X[(int64_t)(i0 + r) * p.ldx + dc + c] : T(0);
                yj[idx] = (j0 + r < p.m && dc + c < p.d) ? p.Y[(int64_t)(j0 + r) * p.ldy + dc + c] : T(0);
            }
            __syncthreads();
#pragma unroll
            for (int c = 0; c < VDC; ++c) {
                T a[4], b[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    a[q] = xi[(ty * 4 + q) * VDC + c];
                    b[q] = yj[(tx * 4 + q) * VDC + c];
                }
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int v = 0; v < 4; ++v) {
                        const T df = a[u] - b[v];
                        r2[u][v] += df * df;
                    }
            }
        }
        // the cotangent of this thread's 4 x 4 elements (nothing outside the n x m view is read)
        T Ge[4][4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = i0 + ty * 4 + u;
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int j = j0 + tx * 4 + v;
                Ge[u][v] = (i < p.n && j < p.m) ? p.G[(int64_t)i * p.ldg + j] : T(0);
            }
        }
        // term by term (the kind is uniform: one branch per term and tile); (GX) d block / dx_e = cD (x_e - y_e) + cS [e == sel],
        // cD and cS summed over the terms
        T cD[GX ? 4 : 1][GX ? 4 : 1], cS[GX ? 4 : 1][GX ? 4 : 1];
        if (GX) {
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int v = 0; v < 4; ++v) cD[GX ? u : 0][GX ? v : 0] = cS[GX ? u : 0][GX ? v : 0] = T(0);
        }
#pragma unroll
        for (int t = 0; t < GPK_MAX_TERMS; ++t) {
            if (t < p.nterms) {
                const int kind = p.kind[t];
                const T c = p.ils2[t], var = p.var[t];
                const T al = SH ? p.shape[t] : T(1);
                if (kind == GPK_K_LINEAR) {
#pragma unroll
                    for (int u = 0; u < 4; ++u)
#pragma unroll
                        for (int v = 0; v < 4; ++v) {
                            const T be = MODE == DMODE_DX ? c * ya[v] : MODE == DMODE_DY ? c * xb[u] : (same ? c : T(0));
                            s1[t] += Ge[u][v] * be;
                            s2[t] += Ge[u][v] * be;
                            if (GX && MODE == DMODE_DY) cS[GX ? u : 0][GX ? v : 0] += var * c;
                        }
                } else if (kind != GPK_K_CONST) {
#pragma unroll
                    for (int u = 0; u < 4; ++u)
#pragma unroll
                        for (int v = 0; v < 4; ++v) {
                            T k1, k2, qk2, m3, k1a, k2a;
                            diff_profile<T, SH>(kind, r2[u][v] * c, al, k1, k2, qk2, m3, k1a, k2a);
                            T be, bc, ba;
                            if (MODE == DMODE_DXY) {
                                const T f = T(-4) * c * c * ((xa[u] - ya[v]) * (xb[u] - yb[v]));
                                const T h = same ? T(-2) * c : T(0);
                                be = f * k2 + h * k1;
                                bc = f * m3 + h * (k1 + qk2);
                                ba = f * k2a + h * k1a;
                            } else {
                                const T sd = MODE == DMODE_DX ? xa[u] - ya[v] : yb[v] - xb[u];      // D_a, or -D_b
                                const T f = T(2) * c * sd;
                                be = f * k1;
                                bc = f * (k1 + qk2);
                                ba = f * k1a;
                                if (GX) {
                                    cD[GX ? u : 0][GX ? v : 0] += var * (T(2) * c) * f * k2;
                                    cS[GX ? u : 0][GX ? v : 0] += (MODE == DMODE_DX ? T(2) : T(-2)) * var * c * k1;
                                }
                            }
                            s1[t] += Ge[u][v] * be;
                            s2[t] += Ge[u][v] * bc;
                            if (SH) s3[SH ? t : 0] += Ge[u][v] * ba;
                        }
                }
            }
        }
        // d/dx_i[e] += (sum_j Ge cD) x_i[e] - sum_j Ge cD y_j[e] + [e == sel] sum_j Ge cS   (xi / yj still hold the only d-chunk): this
        // row's share of the tile over the 16 tx lanes of the row group, then into the owner's entries
        if (GX) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                T sumD = T(0), sumS = T(0);
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    cD[GX ? u : 0][GX ? v : 0] *= Ge[u][v];
                    sumD += cD[GX ? u : 0][GX ? v : 0];
                    sumS += cS[GX ? u : 0][GX ? v : 0] * Ge[u][v];
                }
#pragma unroll
                for (int c = 0; c < VDC; ++c) {
                    T a = sumD * xi[(ty * 4 + u) * VDC + c] + (c == sel ? sumS : T(0));
#pragma unroll
                    for (int v = 0; v < 4; ++v) a -= cD[GX ? u : 0][GX ? v : 0] * yj[(tx * 4 + v) * VDC + c];
#pragma unroll
                    for (int o = 8; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
                    if (tx == 0) gxs[GX ? (ty * 4 + u) * VDC + c : 0] += a;
                }
            }
        }
    }

    // per-term sums of the whole workgroup
    T* out = p.partial + ((int64_t)rt * p.nchunks + chunk) * (NS * GPK_MAX_TERMS + 1);
#pragma unroll
    for (int t = 0; t < GPK_MAX_TERMS; ++t) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            s1[t] += __shfl_xor(s1[t], o, 64);
            s2[t] += __shfl_xor(s2[t], o, 64);
            if (SH) s3[SH ? t : 0] += __shfl_xor(s3[SH ? t : 0], o, 64);
        }
    }
    __syncthreads();
    if (lane == 0) {
#pragma unroll
        for (int t = 0; t < GPK_MAX_TERMS; ++t) {
            red[(wave * GPK_MAX_TERMS + t) * NS] = s1[t];
            red[(wave * GPK_MAX_TERMS + t) * NS + 1] = s2[t];
            if (SH) red[(wave * GPK_MAX_TERMS + t) * NS + 2] = s3[SH ? t : 0];
        }
    }
    __syncthreads();
    if (tid < NS * GPK_MAX_TERMS) {
        out[tid] = red[tid] + red[NS * GPK_MAX_TERMS + tid] + red[2 * NS * GPK_MAX_TERMS + tid] + red[3 * NS * GPK_MAX_TERMS + tid];
    } else if (tid == NS * GPK_MAX_TERMS) {
        out[tid] = T(0);      // the trace slot
    }
    // d/dX: one partial per column chunk, written by the rows' owners
    if (GX && tx == 0) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = i0 + ty * 4 + u;
            for (int c = 0; c < p.d; ++c)
                if (i < p.n) p.gradx[((int64_t)chunk * p.n + i) * p.d + c] = gxs[GX ? (ty * 4 + u) * VDC + c : 0];
        }
    }
}

template <typename T, int MODE, bool SH>
void diff_vjp_launch_mode(const VjpDiffArgs<T>& a, dim3 grid, hipStream_t stream) {
    if constexpr (MODE != DMODE_DXY) {
        if (a.gradx != nullptr) {
            hipLaunchKernelGGL((kmat_diff_vjp_kernel<T, MODE, SH, true>), grid, dim3(256), 0, stream, a);
            return;
        }
    }
    hipLaunchKernelGGL((kmat_diff_vjp_kernel<T, MODE, SH, false>), grid, dim3(256), 0, stream, a);
}

}  // namespace

// Status codes: the argument positions of gpk_kmat_diff_vjp (include/gpk.h); every argument is checked before an empty problem returns GPK_OK.
template <typename T>
int gpk_kmat_diff_vjp_launch(const int* kinds, const double* variances, const double* inv_ls, const double* shapes, int nterms,
                             int dim_x, int dim_y, const T* X, int64_t n, int64_t ldx, const T* Y, int64_t m, int64_t ldy, int d,
                             const T* G, int64_t ldg, T* partial, T* gradx, hipStream_t stream) {
    if (nterms < 0 || nterms > GPK_MAX_TERMS) return GPK_ERR_ARG(6);
    bool shaped = false;
    for (int t = 0; t < nterms; ++t) {
        const int k = kinds[t];
        if (k != GPK_K_EQ && k != GPK_K_MATERN32 && k != GPK_K_MATERN52 && k != GPK_K_LINEAR && k != GPK_K_CONST && k != GPK_K_RQ)
            return GPK_ERR_ARG(2);      // Matern12 and Delta have no derivative; unknown kinds
        if (k == GPK_K_RQ) {
            shaped = true;
            if (shapes == nullptr) return GPK_ERR_ARG(1);       // (`shapes` as for gpk_kmat_diff: -1 without the array, -5 for alpha <= 0)
            if (!(shapes[t] > 0)) return GPK_ERR_ARG(5);
        }
    }
    if (d < 0) return GPK_ERR_ARG(15);
    if (dim_x < -1 || dim_x >= d || (dim_x < 0 && dim_y < 0)) return GPK_ERR_ARG(7);
    if (dim_y < -1 || dim_y >= d) return GPK_ERR_ARG(8);
    if (n > INT32_MAX) return GPK_ERR_ARG(10);
    if (m > INT32_MAX) return GPK_ERR_ARG(13);
    const int mode = dim_y < 0 ? DMODE_DX : dim_x < 0 ? DMODE_DY : DMODE_DXY;
    if (gradx != nullptr && (mode == DMODE_DXY || d > VDC)) return GPK_ERR_ARG(19);     // d/dX: the one-sided modes, d <= 8
    int64_t rt, nc, tpc;
    gpk_kmat_vjp_dense_grid_impl(n, m, 1, &rt, &nc, &tpc);
    if (nc > 65535) return GPK_ERR_ARG(13);
    if (n <= 0 || m <= 0) return GPK_OK;
    VjpDiffArgs<T> a;
    a.X = X; a.Y = Y; a.G = G; a.partial = partial; a.gradx = gradx;
    a.ldx = ldx; a.ldy = ldy; a.ldg = ldg;
    a.n = (int)n; a.m = (int)m; a.d = d; a.nterms = nterms;
    a.dim_x = dim_x; a.dim_y = dim_y;
    a.tiles_per_chunk = (int)tpc; a.nchunks = (int)nc; a.ctiles = (int)gpk_cdiv(m, DT);
    for (int t = 0; t < GPK_MAX_TERMS; ++t) {
        a.kind[t] = t < nterms ? kinds[t] : GPK_K_CONST;
        a.ils2[t] = t < nterms ? (T)(inv_ls[t] * inv_ls[t]) : T(0);
        a.var[t] = t < nterms ? (T)variances[t] : T(0);
        a.shape[t] = (t < nterms && kinds[t] == GPK_K_RQ) ? (T)shapes[t] : T(1);
    }
    const dim3 grid((unsigned)rt, (unsigned)nc);
    if (shaped) {
        if (mode == DMODE_DX) diff_vjp_launch_mode<T, DMODE_DX, true>(a, grid, stream);
        else if (mode == DMODE_DY) diff_vjp_launch_mode<T, DMODE_DY, true>(a, grid, stream);
        else diff_vjp_launch_mode<T, DMODE_DXY, true>(a, grid, stream);
    } else {
        if (mode == DMODE_DX) diff_vjp_launch_mode<T, DMODE_DX, false>(a, grid, stream);
        else if (mode == DMODE_DY) diff_vjp_launch_mode<T, DMODE_DY, false>(a, grid, stream);
        else diff_vjp_launch_mode<T, DMODE_DXY, false>(a, grid, stream);
    }
    GPK_CHECK_LAUNCH();
    return GPK_OK;
}
template int gpk_kmat_diff_vjp_launch<double>(const int*, const double*, const double*, const double*, int, int, int, const double*,
                                              int64_t, int64_t, const double*, int64_t, int64_t, int, const double*, int64_t, double*,
                                              double*, hipStream_t);
template int gpk_kmat_diff_vjp_launch<float>(const int*, const double*, const double*, const double*, int, int, int, const float*,
                                             int64_t, int64_t, const float*, int64_t, int64_t, int, const float*, int64_t, float*, float*,
                                             hipStream_t);

int64_t gpk_kmat_vjp_blocks_impl(int64_t n) {
    const int64_t nt = gpk_cdiv(n > 0 ? n : 1, VT);
    return nt * (nt + 1) / 2;
}

// partial: gpk_kmat_vjp_blocks(n) * (NS * GPK_MAX_TERMS + 1) elements, NS = 3 if some term is RQ or Delta (SH), else 2; diag_g: n elements
template <typename T>
int gpk_kmat_vjp_launch(const int* kinds, const double* inv_ls, const double* shapes, int nterms, const T* X, int64_t n, int64_t ldx,
                        int d, const T* Kinv, int64_t ldk, const T* A, int C, int64_t lda, const double* g,
                        T* partial, T* diag_g, hipStream_t stream) {
    if (n <= 0) return GPK_OK;
    if (nterms < 0 || nterms > GPK_MAX_TERMS) return GPK_ERR_ARG(3);
    bool shaped;
    if (const int st = gpk_check_terms(kinds, shapes, nterms, true, GPK_ERR_ARG(3), &shaped)) return st;
    if (C < 1 || C > VMAXC) return GPK_ERR_ARG(11);
    if (n > INT32_MAX) return GPK_ERR_ARG(5);
    VjpArgs<T> a;
    a.X = X; a.Kinv = Kinv; a.A = A; a.partial = partial; a.diagG = diag_g;
    a.ldx = ldx; a.ldk = ldk; a.lda = lda;
    a.n = (int)n; a.d = d; a.C = C; a.nterms = nterms;
    a.ntile = (int)gpk_cdiv(n, VT);
    double s = 0;
    for (int c = 0; c < VMAXC; ++c) {
        a.g[c] = c < C ? (T)g[c] : T(0);
        if (c < C) s += g[c];
    }
    a.s = (T)s;
    vjp_pack_terms<T>(kinds, nullptr, inv_ls, shapes, nterms, a.kind, a.ils2, nullptr, a.shape);
    const int64_t nb = gpk_kmat_vjp_blocks_impl(n);
    if (shaped)
        hipLaunchKernelGGL((kmat_vjp_kernel<T, true>), dim3((unsigned)nb), dim3(256), 0, stream, a);
    else
        hipLaunchKernelGGL((kmat_vjp_kernel<T, false>), dim3((unsigned)nb), dim3(256), 0, stream, a);
    GPK_CHECK_LAUNCH();
    return GPK_OK;
}
template int gpk_kmat_vjp_launch<double>(const int*, const double*, const double*, int, const double*, int64_t, int64_t, int,
                                         const double*, int64_t, const double*, int, int64_t, const double*,
                                         double*, double*, hipStream_t);
template int gpk_kmat_vjp_launch<float>(const int*, const double*, const double*, int, const float*, int64_t, int64_t, int,
                                        const float*, int64_t, const float*, int, int64_t, const double*, float*,
                                        float*, hipStream_t);
