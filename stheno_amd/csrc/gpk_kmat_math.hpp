// gpk_kmat_math.hpp -- what the kernel-matrix kernels (gpk_kmat.hip) and their derivative kernels (gpk_kdiff.hip) share: the term
// descriptor and the branch-free device routines behind every kernel value (exp of a non-positive argument, the square root of a
// scaled squared distance, log1p).  Internal linkage: each translation unit compiles its own copy.
#pragma once
#include "gpk_common.hpp"

namespace {

template <typename T>
struct KTermT {
    int kind;
    T variance;
    T ils2;   // squared inverse length scale
};

__device__ __forceinline__ double gpk_exp_neg(double a);     // (below) branch-free fp64 exp of a non-positive argument
template <typename T>
__device__ __forceinline__ T gpk_exp(T x);
template <>
__device__ __forceinline__ double gpk_exp<double>(double x) { return gpk_exp_neg(x); }   // every argument on this path is <= 0
template <>
__device__ __forceinline__ float gpk_exp<float>(float x) { return expf(x); }
template <typename T>
__device__ __forceinline__ T gpk_sqrtk(T x);
// sqrt of a squared distance times a positive constant (x >= 0, often exactly 0 on the diagonal): the hardware rsq estimate
// (~2^-23 relative), ONE coupled Goldschmidt step (-> ~2^-45 on both the root and the half reciprocal root) and one residual
// correction, which is a Newton step of its own (-> rounding level; the second Goldschmidt step of sqrt_rsqrt in gpk_potrf.hip
// bought nothing measurable here) -- 8 FMA-class operations, no range scaling, no branch, no select -- instead of the library
// sqrt.  The argument is shifted by 1e-280 (rsq(0) would overflow): invisible from 1e-264 up, and sqrt(0) comes out as 1e-140,
// which moves a kernel value by < 1e-140.  NaN stays NaN.
template <>
__device__ __forceinline__ double gpk_sqrtk<double>(double x) {
    const double xc = x + 1e-280;
    const double y = __builtin_amdgcn_rsq(xc);
    double g = xc * y, h = 0.5 * y;
    double e = fma(-h, g, 0.5);
    g = fma(g, e, g);
    h = fma(h, e, h);
    return fma(fma(-g, g, xc), h, g);
}
template <>
__device__ __forceinline__ float gpk_sqrtk<float>(float x) { return sqrtf(x); }

// log(1 + u), u >= 0 (rational quadratic: u = q / (2 alpha)); the library routines keep full relative accuracy for small u
template <typename T>
__device__ __forceinline__ T gpk_log1p(T u);
template <>
__device__ __forceinline__ double gpk_log1p<double>(double u) { return log1p(u); }
template <>
__device__ __forceinline__ float gpk_log1p<float>(float u) { return log1pf(u); }

// fp64: Cody-Waite reduction a = n ln2 + r (|r| <= ln2 / 2, two-part ln2, one FMA each), the Taylor polynomial of degree 13 in
// Horner form (truncation 4e-18 relative on that interval) and v_ldexp_f64: 13 + 4 FMA-class operations and no branch, against
// ~3x that with branches for the library exp, which was what bounded the fp64 EQ build (2.3 of 8 TB/s).  Measured against
// expl() on 2e7 arguments in [-700, 0]: <= 0.87 ulp.  Arguments below -750 (the result is 0 from -745.2 on) are clamped so that
// -inf gives 0 rather than inf - inf; NaN stays NaN.
__device__ __forceinline__ double gpk_exp_neg(double a) {
    a = (a < -750.0) ? -750.0 : a;
    const double n = rint(a * 1.4426950408889634);
    double r = fma(-n, 6.93147180369123816490e-01, a);
    r = fma(-n, 1.90821492927058770002e-10, r);
    double p = 1.6059043836821613e-10;          // 1/13!
    p = fma(p, r, 2.08767569878681e-09);        // 1/12!
    p = fma(p, r, 2.505210838544172e-08);       // 1/11!
    p = fma(p, r, 2.755731922398589e-07);       // 1/10!
    p = fma(p, r, 2.7557319223985893e-06);      // 1/9!
    p = fma(p, r, 2.48015873015873e-05);        // 1/8!
    p = fma(p, r, 1.984126984126984e-04);       // 1/7!
    p = fma(p, r, 1.388888888888889e-03);       // 1/6!
    p = fma(p, r, 8.333333333333333e-03);       // 1/5!
    p = fma(p, r, 4.1666666666666664e-02);      // 1/4!
    p = fma(p, r, 1.6666666666666666e-01);      // 1/3!
    p = fma(p, r, 0.5);
    p = fma(p, r, 1.0);
    p = fma(p, r, 1.0);
    return ldexp(p, (int)n);
}

}  // namespace
