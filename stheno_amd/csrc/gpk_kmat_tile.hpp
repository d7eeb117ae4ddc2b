// gpk_kmat_tile.hpp -- what the kernel-matrix kernels (gpk_kmat.hip) and their derivative kernels (gpk_kdiff.hip) share beside the
// math of gpk_kmat_math.hpp and the launch geometry of gpk_kmat_plan.hpp: the staging of a band's X rows and the diagonal additions
// on the device (templates over the argument struct, KmatArgs / KdiffArgs), the dispatch over the staged dimensions and the packing of
// the term table in the launchers.  The Y-tile staging, the one-tile chunk loop and the row store are NOT here: out of a helper they
// compile to other instructions than written in the kernel (profiles/README.md, "Shared tile helpers").  Internal linkage.
#pragma once
#include "gpk_common.hpp"
#include "gpk_kmat_math.hpp"
#include "gpk_kmat_plan.hpp"

namespace {

// Row-band kernels: the band's X rows, TM * DC <= 256 elements, one per thread; d <= DC (launcher).
template <typename T, int DC, typename P>
__device__ __forceinline__ void kmat_stage_band_x(const P& p, const T* X, int tid, int row0, T* xs) {
    if (tid < TM * DC) {
        const int r = tid / DC, j = tid % DC;
        const int row = row0 + r;
        xs[tid] = (row < p.n && j < p.d) ? X[(int64_t)row * p.ldx + j] : T(0);
    }
}

// diag_add + diag_vec[row] of batch entry b onto a diagonal element
template <typename T, typename P>
__device__ __forceinline__ void kmat_add_diag(const P& p, int64_t b, int row, T& val) {
    val += p.diag_add;
    if (p.diag_vec != nullptr) val += p.diag_vec[b * p.sDiag + row];
}

// LAUNCH(args..., DC) with the smallest DC in {1, 2, 4, 8} that holds d (d <= 8 for the row-band kernels, any d for the one-tile ones)
#define GPK_KMAT_DC(d, LAUNCH, ...)                 \
    do {                                            \
        if ((d) <= 1) LAUNCH(__VA_ARGS__, 1);       \
        else if ((d) <= 2) LAUNCH(__VA_ARGS__, 2);  \
        else if ((d) <= 4) LAUNCH(__VA_ARGS__, 4);  \
        else LAUNCH(__VA_ARGS__, 8);                \
    } while (0)

// The term table of a launch from the host arrays of the entry points; `pad`: the unused entries are set too (constant terms of
// variance 0).  Returns "some term is Linear" (its value needs the dot product).
template <typename T>
inline bool gpk_pack_terms(KTermT<T>* terms, const int* kinds, const double* variances, const double* inv_ls, int nterms, bool pad) {
    bool linear = false;
    for (int t = 0; t < (pad ? GPK_MAX_TERMS : nterms); ++t) {
        const bool on = t < nterms;
        terms[t].kind = on ? kinds[t] : GPK_K_CONST;
        terms[t].variance = on ? (T)variances[t] : T(0);
        terms[t].ils2 = on ? (T)(inv_ls[t] * inv_ls[t]) : T(0);
        if (on && kinds[t] == GPK_K_LINEAR) linear = true;
    }
    return linear;
}

}  // namespace
