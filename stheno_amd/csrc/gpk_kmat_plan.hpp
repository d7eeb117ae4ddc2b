// gpk_kmat_plan.hpp -- the launch geometry of the kernel-matrix kernels (gpk_kmat.hip) and their derivative kernels (gpk_kdiff.hip):
// tile constants, the grid plan of a launch and the decode of the compact 1-D grid.  Plain C++ (no HIP header): the same text is
// compiled into both launchers and both row-band kernels and, by a host compiler alone, into kmat_plan_check.cpp, which walks the
// plan and the decode over a few thousand shapes (tests/test_kmat_plan.py).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define GPK_PLAN_HD __host__ __device__ __forceinline__
#else
#define GPK_PLAN_HD inline
#endif

namespace {

#if !defined(__HIPCC__)
inline int min(int a, int b) { return a < b ? a : b; }      // (a HIP compile has it for both sides)
#endif

constexpr int TM = 32;       // tile rows
constexpr int RW = 8;        // rows per wave
constexpr int CT_MAX = 8;    // row-band kernel: column tiles per workgroup (fewer when the grid would not fill the chip a few times over)

struct KmatPlan {
    int ct;           // row-band kernel: column tiles per workgroup
    int nbands;       // number of row bands (TM rows each)
    int compact;      // row-band kernel, lower triangle of one square matrix: a 1-D grid of exactly the (row band, column chunk) pairs on or
                      // below the diagonal -- `compact` = row bands per column chunk; 0 = the plain 2-D grid
    unsigned gx, gy, gz;
};

// vec: elements per 16-byte store (a tile is 64 * vec columns); band: the row-band kernel (else one tile per workgroup, ct = 1);
// compact_knob: tuning knob 34.  The caller has checked n, m, batch > 0 and that the row bands and the batch fit a grid dimension.
inline KmatPlan gpk_kmat_plan(int64_t n, int64_t m, int64_t batch, int vec, int lower_only, int symmetric, bool band, int compact_knob) {
    const int64_t tn = 64 * vec, gy = (n + TM - 1) / TM, tiles_x = (m + tn - 1) / tn;
    KmatPlan p = {1, (int)gy, 0, (unsigned)tiles_x, (unsigned)gy, (unsigned)batch};
    if (!band) return p;
    int ct = CT_MAX;
    while (ct > 1 && (tiles_x + ct - 1) / ct * gy * batch / (lower_only ? 2 : 1) < 6144) ct >>= 1;
    p.ct = ct;
    p.gx = (unsigned)((tiles_x + ct - 1) / ct);
    // Lower triangle of a square matrix with several column chunks per row band: half of the 2-D grid would be workgroups
    // that exit at once, and the dispatcher works through them in index order in front of the real ones (measured at
    // N = 16384: the lower triangle took 0.46 ms against 0.52 ms for the FULL matrix).  A 1-D grid of exactly the pairs needed.
    const int64_t chunk_cols = ct * tn;
    if (compact_knob && lower_only && symmetric && n == m && p.gx > 1 && chunk_cols % TM == 0) {
        const int64_t G = chunk_cols / TM;
        int64_t total = 0;
        for (int64_t g = 0; g * G < gy; ++g) total += ((gy - g * G < G) ? gy - g * G : G) * (g + 1);
        p.compact = (int)G;
        p.gx = (unsigned)total;
        p.gy = 1u;
    }
    return p;
}

// Compact 1-D grid over the (row band, column chunk) pairs on or below the diagonal: the bands of chunk-group g (G = `compact`
// consecutive row bands) have g + 1 chunks each.  Groups are laid out from the bottom of the matrix up (full chunks first).
GPK_PLAN_HD void gpk_kmat_compact_decode(int bid, int nbands, int G, int& by, int& bx) {
    int g = (nbands + G - 1) / G - 1;
    for (; g > 0; --g) {
        const int cnt = min(G, nbands - g * G) * (g + 1);
        if (bid < cnt) break;
        bid -= cnt;
    }
    by = g * G + bid / (g + 1);
    bx = bid % (g + 1);
}

}  // namespace
