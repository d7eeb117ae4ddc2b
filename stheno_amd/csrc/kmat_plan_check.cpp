// kmat_plan_check.cpp -- host-side check of the launch geometry of the kernel-matrix and derivative kernels (gpk_kmat_plan.hpp):
// for both vector widths, square sizes from 1 to 3000 and two large ones, and a few batch sizes,
//   * whenever the plan chooses the compact 1-D grid, decoding every workgroup index of it gives exactly the (row band, column
//     chunk) pairs on or below the diagonal -- ct0 * TN <= row0 + TM - 1 -- each once, and no row band outside the matrix;
//   * a plain 2-D grid covers every column tile: gx * ct >= tiles_x.
// Then prints the plans of the shapes that tests/test_diff_gpu.py relies on for its walk and compact-grid cases.
// Plain C++ (g++ kmat_plan_check.cpp && ./a.out); run by tests/test_kmat_plan.py.  Test infrastructure, not part of libgpk.so.
#include <cstdio>
#include <vector>
#include "gpk_kmat_plan.hpp"

static int check(int64_t n, int64_t batch, int vec, int lower) {
    const KmatPlan p = gpk_kmat_plan(n, n, batch, vec, lower, lower, true, 1);
    const int64_t tn = 64 * vec, tiles_x = (n + tn - 1) / tn;
    if (!p.compact) {
        if ((int64_t)p.gx * p.ct >= tiles_x && p.gy == (unsigned)p.nbands) return 0;
        std::printf("FAIL 2-D grid: n=%lld batch=%lld vec=%d lower=%d  ct=%d gx=%u gy=%u\n", (long long)n, (long long)batch, vec, lower, p.ct, p.gx, p.gy);
        return 1;
    }
    const int64_t chunks = (tiles_x + p.ct - 1) / p.ct;
    std::vector<int> seen((size_t)(p.nbands * chunks), 0);
    for (unsigned bid = 0; bid < p.gx; ++bid) {
        int by = -1, bx = -1;
        gpk_kmat_compact_decode((int)bid, p.nbands, p.compact, by, bx);
        const bool inside = by >= 0 && by < p.nbands && bx >= 0 && bx < chunks;
        if (!inside || (int64_t)bx * p.ct * tn > (int64_t)by * TM + TM - 1 || seen[(size_t)(by * chunks + bx)]++) {
            std::printf("FAIL decode: n=%lld batch=%lld vec=%d  ct=%d compact=%d  bid=%u -> by=%d bx=%d\n", (long long)n, (long long)batch, vec, p.ct,
                        p.compact, bid, by, bx);
            return 1;
        }
    }
    for (int by = 0; by < p.nbands; ++by)
        for (int64_t bx = 0; bx < chunks; ++bx)
            if ((bx * p.ct * tn <= (int64_t)by * TM + TM - 1) != (seen[(size_t)(by * chunks + bx)] == 1)) {
                std::printf("FAIL cover: n=%lld batch=%lld vec=%d  ct=%d compact=%d  by=%d bx=%lld\n", (long long)n, (long long)batch, vec, p.ct, p.compact,
                            by, (long long)bx);
                return 1;
            }
    return p.gy == 1u ? 0 : 1;
}

static void show(const char* name, int64_t n, int64_t m, int64_t batch, int vec, int lower) {
    const KmatPlan p = gpk_kmat_plan(n, m, batch, vec, lower, lower, true, 1);
    std::printf("plan %s: ct=%d compact=%d gx=%u gy=%u gz=%u\n", name, p.ct, p.compact, p.gx, p.gy, p.gz);
}

int main() {
    const int64_t batches[] = {1, 3, 96, 640};
    int shapes = 0, compact = 0;
    for (int vec = 2; vec <= 4; vec += 2)
        for (const int64_t batch : batches)
            for (int64_t n = 1; n <= 32768; n = n < 2997 ? n + 7 : n < 16384 ? 16384 : 2 * n)
                for (int lower = 0; lower < 2; ++lower) {
                    if (check(n, batch, vec, lower)) return 1;
                    ++shapes;
                    compact += gpk_kmat_plan(n, n, batch, vec, lower, lower, true, 1).compact != 0;
                }
    std::printf("%d shapes OK, %d of them on the compact grid\n", shapes, compact);
    show("walk f64", 97, 259, 1536, 2, 0);
    show("walk f32", 97, 600, 1536, 4, 0);
    show("compact f64", 300, 300, 640, 2, 1);
    show("compact f32", 600, 600, 640, 4, 1);
    return 0;
}
