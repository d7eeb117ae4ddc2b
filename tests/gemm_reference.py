"""Cases, references, a launch-plan model and runners for the MFMA GEMM entry points of ``stheno_amd/csrc/gpk_gemm.hip`` and
``gpk_gemm_tile.hpp``: ``gpk_gemm``, ``gpk_gemm_colscale`` and ``gpk_gemm_update2``.

``tests/test_gemm_kernels_gpu.py`` runs every case over ``HipBackend`` on the GPU, ``tests/test_gemm_reference_host.py`` runs the same
runners over a NumPy backend, shows that the bounds admit a correct implementation, that each of a list of single defects is caught and
that the case tables reach every branch of the launchers.  Nothing here touches a GPU: the runners take the backend and the device.

**Rounded data** (``linalg_reference.draw``: magnitudes log-uniform in [0.25, 1], random signs, fp32 numbers, so one reference serves both
dtypes).  The reference is computed in ``np.longdouble`` from the rounded inputs; every output gets its value and
``absum = |alpha| sum_k |a b| + |beta c|``.  Acceptance: ``|got - ref| <= (K_eff + 2) * eps * absum`` with ``K_eff`` the number of NON-ZERO
terms of that output (the k a flag leaves in the sum, less the exact zeros of sparse data: adding an exact zero rounds nothing).  The
kernel starts the accumulator at ``c * (beta / alpha)``, adds one product per k and multiplies by ``alpha`` at the end: at most
``K_eff + 3`` roundings of half an ``eps`` each on any term's way, whatever the order of the additions -- ``(K_eff + 3) / 2 <= K_eff + 2``.

**Grid data.**  Multiples of 2^-8 in [0.25, 1] with random signs, ``c`` on the 2^-16 grid in [-1, 1], ``alpha`` in {1, -1, -0.5}, ``beta`` in
{0, 1} and ``K + |beta / alpha| <= 256``: every product, every partial sum in any order, ``c * (beta / alpha)`` and the final scaling are exact
in fp32 and in fp64, so the reference is one fp64 ``matmul`` and the result has to EQUAL it (compared as numbers: the sign of a zero is
not looked at).  Any lost, doubled or misplaced term changes the value.  The two triangular cases on the 128-tiles need K = 256
(``data="grid128"``): A is zero at every k that is no multiple of 3, so at most 86 terms of at most 1 meet in an output and the sums stay
exact.

**Detection condition** (``detection_margin``): every non-zero term of every output of a rounded case is at least
``4 * (K_eff + 2) * eps * absum``.  Dense fp32 data meets it up to K = 360; longer contractions are zero outside at most 64 k positions
(``_support``) that include the first and last position of the first, second and last chunk of both dtypes and, for triangular operands,
the first and last position of every 32-row tile.

**Layouts.**  Operands sit in NaN-filled storage: leading dimension ``cols + pad``, optionally behind an element offset that breaks the
16-byte alignment, batch members one after the other.  ``C`` has ``SENT`` in every padding element and between batch members, which must
come back unchanged.  Under ``lower_only`` an entry above the diagonal inside a 128-tile strictly above the diagonal tile must be
untouched; elsewhere above the diagonal it is either untouched or the full product to the same bound.  Triangular flags get exact zeros
in the region they skip.

**colss** (``gpk_gemm_colscale``): per 64-row slab r and column n, ``ss = sum_m v_m^2`` with ``v = alpha * sum_k a b`` (unscaled), accepted
within ``eps * (2 (K_eff + 2) sum_m |v_m| absum_m + (d + 1) ss)``.  ``d = COLSS_DEPTH = 18``: in the epilogue of ``gemm_tile`` a lane adds the
squares of its 4 fragments x 4 accumulator registers one after the other (16 additions, the ``fi`` and ``i`` loops), then two shuffle
steps (``__shfl_xor`` 16 and 32) add the four lane groups: a chain of 18 additions; the ``+ 1`` is the rounding of the square."""
import zlib

import numpy as np
import torch

from .linalg_reference import DTYPES, EPS, LD, NP, SENT, TORCH, VEC, case_id, draw, host, support, sync  # noqa: F401

BK = {"float64": 16, "float32": 32}              # Traits<T>::BK: elements of k per 128-byte chunk
SMALL_TILE_BELOW = 512                           # g_small_tile_below: fewer 128-tiles than this take the 64-tile kernels
PERSIST_SMALL_BELOW = 512                        # g_persist_small_below
TILE = 128                                       # GPK_TILE
COLSS_DEPTH = 18
DENSE_K_MAX = 360                                # longest dense contraction that meets the detection condition in fp32
ALPHA, BETA = -0.75, 0.5
NAN = float("nan")
GARBAGE = 0x5A5A5A5A                             # what the ctrl words of gpk_gemm_update2 hold on entry


def cdiv(a, b):
    return -(-a // b)


# -- cases ------------------------------------------------------------------------------------------------------------------------------
def G(name, M, N, K, **kw):
    """One ``gpk_gemm`` / ``gpk_gemm_colscale`` case.  ``ak`` / ``bk``: operand stored (rows, K); ``aoff`` / ``boff``: element offset of the view;
    ``b_bcast``: one B for every batch member (batch stride 0); ``cgap``: rows of sentinels between the members of C; ``mode``: what
    ``gpk_gemm_colscale`` is asked for ("" | "scale" | "ss" | "both")."""
    c = dict(entry="gemm", id=name, M=M, N=N, K=K, batch=1, ak=True, bk=True, alpha=1.0, beta=0.0, lower=False, tri_k=False, tri_lo=False,
             tri_lo_b=False, panel=False, data="rounded", apad=0, bpad=0, cpad=1, aoff=0, boff=0, b_bcast=False, cgap=0, inplace=False,
             mode="", sspad=0, want=())
    assert set(kw) <= set(c), set(kw) - set(c)
    c.update(kw)
    c["seed"] = zlib.crc32(name.encode())
    return c


LAYOUTS = [(True, True), (True, False), (False, True), (False, False)]


def _lay(ak, bk):
    return ("MK" if ak else "KM") + ("NK" if bk else "KN")


def gemm_cases(dtype):
    b, V = BK[dtype], VEC[dtype]
    cs = []
    # 64-tile kernels without bounds checks
    for ak, bk in LAYOUTS:
        cs.append(G(f"k64-64x64x{b}-{_lay(ak, bk)}", 64, 64, b, ak=ak, bk=bk, cpad=0, want=("k64",)))
        cs.append(G(f"k64-128x192x{2 * b}-{_lay(ak, bk)}", 128, 192, 2 * b, ak=ak, bk=bk, alpha=ALPHA, beta=BETA, cpad=V, want=("k64",)))
    # 64-tile kernels with bounds checks
    cs.append(G("e64-1x1x1", 1, 1, 1, want=("k64e",)))
    for ak, bk in LAYOUTS:
        cs.append(G(f"e64-65x63x33-{_lay(ak, bk)}", 65, 63, 33, ak=ak, bk=bk, alpha=ALPHA, beta=BETA, want=("k64e",)))
        cs.append(G(f"e64-100x70x37-oddld-{_lay(ak, bk)}", 100, 70, 37, ak=ak, bk=bk, apad=(0 if ak else 1), bpad=(0 if bk else 1), want=("k64e", "pipe0")))
        cs.append(G(f"e64-100x72x{2 * b}-offset-{_lay(ak, bk)}", 100, 72, 2 * b, ak=ak, bk=bk, aoff=1, apad=V - 1, boff=1, bpad=V - 1, alpha=ALPHA,
                    beta=BETA, want=("k64e", "pipe0")))
    cs.append(G(f"e64-70x66x{b - 1}-K-below-BK", 70, 66, b - 1, want=("k64e",)))
    cs.append(G("e64-K0-beta1", 70, 66, 0, beta=1.0, want=("k64e",)))
    cs.append(G("e64-K0-beta0", 70, 66, 0, want=("k64e",)))
    cs.append(G(f"e64-KxM-{64 + V + 1}", 64 + V + 1, 64, 2 * b, ak=False, apad=V - 1, want=("k64e",)))          # aligned ld, M no multiple of VEC
    cs.append(G("e64-70x50x1003-sparse", 70, 50, 1003, alpha=ALPHA, beta=BETA, want=("k64e",)))
    cs.append(G("e64-130x70x997-sparse-KMNK", 130, 70, 997, ak=False, apad=V - 130 % V, want=("k64e",)))
    # 128-tile kernels on the 3-D grid (grid data), and the last 64-tile launch below the threshold
    cs.append(G("k128-b32-512x512x32", 512, 512, 32, batch=32, data="grid", alpha=-1.0, beta=1.0, cpad=0, want=("k128",)))
    cs.append(G("e128-b32-500x510x40", 500, 510, 40, batch=32, data="grid", bk=False, bpad=2, cpad=2, want=("k128e",)))
    cs.append(G("k64-b31-512x512x32", 512, 512, 32, batch=31, data="grid", alpha=-0.5, beta=1.0, cpad=0, want=("k64",)))
    # one XCD per matrix
    cs.append(G("xcd-b64-256x512x32", 256, 512, 32, batch=64, data="grid", b_bcast=True, cpad=0, want=("xcd",)))
    cs.append(G("xcd-b67-300x384x40", 300, 384, 40, batch=67, data="grid", alpha=-1.0, beta=1.0, cgap=3, cpad=4, want=("xcd", "xcd-ragged-batch")))
    # the last, partial round as quarter tiles (grid data)
    cs.append(G("split-2944x2944x32-KMKN", 2944, 2944, 32, data="grid", ak=False, bk=False, cpad=0, want=("split",)))
    cs.append(G("split-3072x4096x32", 3072, 4096, 32, data="grid", alpha=-0.5, beta=1.0, cpad=0, want=("split", "split-half-round")))
    cs.append(G("split-lower-4000x4000x40", 4000, 4000, 40, data="grid", lower=True, alpha=-1.0, beta=1.0, cpad=0, want=("split", "tri_decode")))
    cs.append(G("nosplit-3072x4224x32", 3072, 4224, 32, data="grid", cpad=0, want=("nosplit",)))
    # lower_only, other shapes
    cs.append(G("lower-384x256x32", 384, 256, 32, lower=True, alpha=-1.0, beta=1.0, want=("lower-filter",)))
    cs.append(G("lower-700x300x50", 700, 300, 50, lower=True, alpha=-1.0, beta=1.0, want=("lower-filter",)))
    cs.append(G("lower-657x657x24", 5 * 128 + 17, 5 * 128 + 17, 24, lower=True, alpha=ALPHA, beta=BETA, want=("tri_decode",)))
    cs.append(G("lower-b2-200x200x40", 200, 200, 40, batch=2, lower=True, alpha=-1.0, beta=1.0, want=("tri_decode",)))
    # GPK_GEMM_TRI_K: both operands stored K x M
    for n in (64, 192, 300):
        cs.append(G(f"trik-{n}", n, n, n, ak=False, bk=False, tri_k=True, apad=(n % V and V - n % V), bpad=(n % V and V - n % V), want=("tri_k",)))
        cs.append(G(f"trik-lower-{n}", n, n, n, ak=False, bk=False, tri_k=True, lower=True, beta=1.0, want=("tri_k", "tri_decode")))
    cs.append(G("trik-200x200x100", 200, 200, 100, ak=False, bk=False, tri_k=True, want=("tri_k", "tri_k-clamp")))
    cs.append(G("trik-b3-192", 192, 192, 192, batch=3, ak=False, bk=False, tri_k=True, lower=True, beta=1.0, want=("tri_k",)))
    # GPK_GEMM_TRI_K_LOWER: A (M x K) lower triangular
    for n in (64, 192, 300):
        for bk in (True, False):
            cs.append(G(f"trilo-{n}-{_lay(True, bk)}", n, 100, n, bk=bk, tri_lo=True, beta=(BETA if bk else 0.0), alpha=ALPHA, want=("tri_lo",)))
    cs.append(G("trilo-K<M", 200, 70, 100, tri_lo=True, want=("tri_lo",)))
    cs.append(G("trilo-K>M", 100, 70, 200, tri_lo=True, bk=False, want=("tri_lo",)))
    cs.append(G("trilo-b3-192x64x192", 192, 64, 192, batch=3, tri_lo=True, bk=False, want=("tri_lo",)))
    cs.append(G("trilo-k128-b32-256x1024x256", 256, 1024, 256, batch=32, tri_lo=True, data="grid128", b_bcast=True, cpad=0, want=("tri_lo-128",)))
    # ... on gemm_trilo_pair_kernel
    for bk in (True, False):
        cs.append(G(f"pair-256x64x256-{_lay(True, bk)}", 256, 64, 256, bk=bk, tri_lo=True, cpad=0, want=("pair",)))
        cs.append(G(f"pair-512x100x512-{_lay(True, bk)}", 512, 100, 512, bk=bk, tri_lo=True, alpha=ALPHA, beta=BETA, want=("pair", "pair-e2")))
    cs.append(G("pair-320x64x320", 320, 64, 320, tri_lo=True, cpad=0, want=("pair", "pair-odd-half")))
    # GPK_GEMM_TRI_K_LOWER_B: B (N x K) lower triangular
    for n in (64, 256, 300):
        for m in (64, 200):
            cs.append(G(f"trilob-{m}x{n}x{n}", m, n, n, tri_lo_b=True, alpha=ALPHA, beta=(BETA if m == 200 else 0.0), want=("tri_lo_b",)))
    cs.append(G("trilob-k128-b32-1024x256x256", 1024, 256, 256, batch=32, tri_lo_b=True, data="grid128", b_bcast=True, cpad=0, want=("tri_lo_b-128",)))
    # in place: C aliases A
    for panel in (False, True):
        p = "-panel" if panel else ""
        w = ("trib",) if panel else ("inplace",)
        cs.append(G(f"inplace-64x128{p}", 64, 128, 128, inplace=True, panel=panel, cpad=0, want=w))
        cs.append(G(f"inplace-3001x128-ld131{p}", 3001, 128, 128, inplace=True, panel=panel, cpad=3, want=w))
        cs.append(G(f"inplace-b3-200x128{p}", 200, 128, 128, batch=3, inplace=True, panel=panel, cpad=0, cgap=2, want=w))
        cs.append(G(f"inplace-300x100-ld128{p}", 300, 100, 100, inplace=True, panel=panel, cpad=28, want=w))
        cs.append(G(f"inplace-300x128-KN{p}", 300, 128, 128, inplace=True, panel=panel, bk=False, cpad=0, want=("inplace-128",)))
    ids = [c["id"] for c in cs]
    assert len(set(ids)) == len(ids)
    return cs


def colscale_cases(dtype):
    b = BK[dtype]
    Ms, Ns, Ks = (1, 63, 64, 65, 128, 129, 200), (1, 15, 128, 130, 300), (1, b - 1, b, 3 * b + 5)
    modes, flags = ("both", "ss", "scale", ""), ("", "", "tri_k", "tri_lo", "tri_lo_b")
    cs = []
    i = 0
    for im, M in enumerate(Ms):
        for jn, N in enumerate(Ns):
            K = Ks[(im + jn) % 4]
            ak, bk = LAYOUTS[(im + 2 * jn) % 4]
            mode, fl = modes[(im + jn // 2) % 4], flags[(2 * im + jn) % 5]
            kw = {fl: True} if fl else {}
            cs.append(G(f"cs-{M}x{N}x{K}-{_lay(ak, bk)}-{mode or 'plain'}{'-' + fl if fl else ''}", M, N, K, ak=ak, bk=bk, mode=mode, cpad=i % 3, sspad=(i % 2) * 3,
                        alpha=(ALPHA if i % 2 else 1.0), apad=(i % 4 == 1) * 1, bpad=(i % 4 == 2) * 1, **kw))
            i += 1
    # every M with every mode that writes colss, every K at a ragged M
    for im, M in enumerate(Ms):
        cs.append(G(f"cs-{M}x130x{Ks[im % 4]}-ss", M, 130, Ks[im % 4], mode="ss", sspad=2))
        cs.append(G(f"cs-{M}x15x{Ks[(im + 2) % 4]}-both-KMKN", M, 15, Ks[(im + 2) % 4], ak=False, bk=False, mode="both", alpha=ALPHA))
    for ak, bk in LAYOUTS:
        for fl in ("", "tri_k", "tri_lo", "tri_lo_b"):
            kw = {fl: True} if fl else {}
            cs.append(G(f"cs-200x130x{3 * b + 5}-{_lay(ak, bk)}-both{'-' + fl if fl else ''}", 200, 130, 3 * b + 5, ak=ak, bk=bk, mode="both", sspad=1, **kw))
    # contractions longer than a tile, so that the k ranges of the flags bind on the 128-tiles
    for fl in ("tri_k", "tri_lo", "tri_lo_b"):
        cs.append(G(f"cs-200x200x200-both-{fl}", 200, 200, 200, mode="both", ak=(fl != "tri_k"), bk=(fl != "tri_k"), sspad=1, **{fl: True}))
    for M, N, K in ((128, 128, 2 * b), (256, 128, b)):
        cs.append(G(f"cs-{M}x{N}x{K}-both-aligned", M, N, K, mode="both", cpad=0))
    for c in cs:
        c["entry"] = "colscale"
        if c["mode"] in ("ss", "both"):
            c["data"] = "positive"
    ids = [c["id"] for c in cs]
    assert len(set(ids)) == len(ids)
    return cs


def U(name, segs, **kw):
    """One ``gpk_gemm_update2`` case; ``segs``: dicts with M, N, K, ``lower`` and ``oop`` (``cin`` is a buffer of its own with another
    leading dimension and ``c`` starts full of sentinels)."""
    c = dict(entry="update2", id=name, segs=[dict(dict(lower=False, oop=False, pad=0), **s) for s in segs], alpha=-1.0, data="rounded", want=(),
             both_reserves=False)
    c.update(kw)
    c["seed"] = zlib.crc32(name.encode())
    return c


def update2_cases(dtype):
    rect, sq = dict(M=300, N=200, K=40, oop=True, pad=1), dict(M=260, N=260, K=40, lower=True, pad=1)
    return [
        U("u2-300x200+260sq-K40", [rect, sq], alpha=ALPHA, want=("p64",)),
        U("u2-one-segment-300x200", [rect], alpha=ALPHA, want=("p64",)),
        U("u2-one-segment-260sq-lower", [sq], want=("p64",)),
        U("u2-empty-first-segment", [dict(M=0, N=200, K=40, oop=True), sq], want=("p64",)),
        U("u2-2560sq+256x128-K32", [dict(M=256, N=128, K=32, oop=True), dict(M=2560, N=2560, K=32, lower=True)], data="grid", both_reserves=True,
          want=("p64",)),
        # (45 x 46 / 2 + 8 = 1043 64-tiles: more than the 1024 slots of 256 CUs)
        U("u2-2880sq+256x128-K32", [dict(M=256, N=128, K=32, oop=True), dict(M=2880, N=2880, K=32, lower=True)], data="grid", both_reserves=True,
          want=("p64-loop",)),
        U("u2-4096sq+128x256-K32", [dict(M=128, N=256, K=32, oop=True), dict(M=4096, N=4096, K=32, lower=True)], data="grid", alpha=-0.5,
          both_reserves=True, want=("p128-split",)),
    ]


CASES = {"gemm": gemm_cases, "colscale": colscale_cases, "update2": update2_cases}


def all_cases(entry):
    return [(c, dt) for dt in DTYPES for c in CASES[entry](dt)]


# -- the launch plan: which kernel body a case runs on -------------------------------------------------------------------------------------
def layout(case, dtype):
    """Leading dimensions, batch strides and alignment of the operands as the runner lays them out and ``HipBackend.gemm`` passes them."""
    V, B = VEC[dtype], case["batch"]
    M, N, K = case["M"], case["N"], case["K"]
    out = {}
    for x, kmaj, R, off, pad, bc in (("a", case["ak"], M, case["aoff"], case["apad"], False), ("b", case["bk"], N, case["boff"], case["bpad"], case["b_bcast"])):
        rows, cols = (R, K) if kmaj else (K, R)
        if x == "a" and case["inplace"]:
            off, pad = 0, case["cpad"]
        ld = off + cols + pad
        out[x] = dict(rows=rows, cols=cols, off=off, pad=pad, ld=(ld if rows > 1 else max(cols, 1)),
                      stride=(0 if (B == 1 or bc) else (rows + (case["cgap"] if x == "a" and case["inplace"] else 0)) * ld))
    size = 8 if dtype == "float64" else 4
    out["aligned"] = all((o["off"] * size) % 16 == 0 and o["ld"] % V == 0 and o["stride"] % V == 0 for o in (out["a"], out["b"]))
    return out


def plan(case, dtype, cus=256):
    """The branch selection of ``gpk_gemm_launch2`` (cases of ``gpk_gemm`` and ``gpk_gemm_colscale``) and of ``gpk_gemm_persist_launch``
    (``gpk_gemm_update2``) in pure Python."""
    if case["entry"] == "update2":
        return _plan_update2(case, dtype, cus)
    b = BK[dtype]
    M, N, K, batch = case["M"], case["N"], case["K"], case["batch"]
    lower, inplace = case["lower"], case["inplace"]
    fused = case["entry"] == "colscale" and case["mode"] != ""
    flags = int(lower) | 2 * case["tri_k"] | 4 * case["tri_lo"] | 8 * case["tri_lo_b"] | 16 * case["panel"]
    tm, tn = cdiv(M, TILE), cdiv(N, TILE)
    t128 = (tm * (tm + 1) // 2 if lower and tm == tn else tm * tn) * batch
    ts, nct = (64 if t128 < SMALL_TILE_BELOW and not fused else 128), 1
    if inplace:
        assert N <= 128
        if ts == 64 and case["ak"] and case["bk"]:
            nct = 2
        else:
            ts = 128
    tiles_m, tiles_n = cdiv(M, ts), cdiv(N, ts * nct)
    tri = lower and tiles_m == tiles_n
    total = tiles_m * (tiles_m + 1) // 2 if tri else tiles_m * tiles_n
    aligned = layout(case, dtype)["aligned"]
    edge = bool(not aligned or M % ts or N % (ts * nct) or K % b or K < b)
    p = dict(ts=ts, nct=nct, edge=edge, aligned=aligned, tiles=total, split=False, split_from=None, rem=0, xcd=False, pair=False, trib=False,
             pipe0=False, persist=False, loops=False, kernel="gemm_kernel",
             order=("tri_decode" if tri else "reversed-columns" if case["tri_lo_b"] else "reversed-rows" if case["tri_lo"] else "row-major"),
             lower_filter=bool(lower and not tri))
    gridx = total
    if not fused and ts == 128 and nct == 1 and batch == 1 and not flags & 14 and not inplace:
        slots = 2 * cus
        p["rem"] = rem = total % slots
        if total > slots and rem > 0 and 2 * rem <= slots:
            p.update(split=True, split_from=total - rem)
            gridx = total + 3 * rem
    if not flags & 16 and ts == 128 and nct == 1 and batch >= 64 and not p["split"]:
        p["xcd"] = True
    if flags == 4 and case["ak"] and ts == 64 and nct == 1 and batch == 1 and M % 64 == 0 and M >= 256 and not inplace and cdiv(M, 64) * cdiv(N, 64) <= 2 * cus:
        p.update(pair=True, kernel="gemm_trilo_pair_kernel", ts=32, edge=bool(not aligned or N % 64 or K % b), tiles=(M // 32 // 2) * cdiv(N, 64))
        return p
    p["trib"] = trib = bool(flags & 16 and case["ak"] and case["bk"] and tiles_n == 1 and N <= 128 and not p["split"])
    if trib and (nct == 2 or ts == 128):
        p["kernel"] = "gemm_trib_kernel"
    elif nct == 1 and dtype == "float64" and not aligned:
        p["pipe0"] = True
    p["grid"] = gridx
    return p


def _plan_update2(case, dtype, cus):
    b, V = BK[dtype], VEC[dtype]
    live = [s for s in case["segs"] if s["M"] > 0 and s["N"] > 0]

    def tiles(s, ts):
        tm, tn = cdiv(s["M"], ts), cdiv(s["N"], ts)
        return tm * (tm + 1) // 2 if s["lower"] and tm == tn else tm * tn
    t128 = sum(tiles(s, 128) for s in live)
    ts = 64 if t128 < PERSIST_SMALL_BELOW else 128
    total = sum(tiles(s, ts) for s in live)
    per_cu = 2 if ts == 128 else 4
    slots = cus * per_cu
    gridx = min(total, slots)
    edge = any((s["K"] + s["pad"]) % V or s["M"] % ts or s["N"] % ts or s["K"] % b for s in live)
    out = {}
    for reserve in (0, 1):
        max_leave = per_cu * 8 if (reserve and total >= slots) else 0
        p = dict(ts=ts, edge=bool(edge), tiles=total, grid=gridx, persist=True, loops=total > slots, split=False, split_from=None, kernel="gemm_persist_kernel")
        if ts == 128 and total > gridx:
            workers = gridx - max_leave
            rem = total % workers
            if rem > 0 and 2 * rem <= workers:
                p.update(split=True, split_from=total - rem)
        out[reserve] = p
    return dict(out[0], with_reserve=out[1])


def branches(case, dtype, cus=256):
    """The names of the launcher branches a case reaches (what ``want`` of a case is checked against)."""
    p = plan(case, dtype, cus)
    out = set()
    if case["entry"] == "update2":
        out.add("p64-loop" if p["ts"] == 64 and p["loops"] else "p64" if p["ts"] == 64 else "p128-split" if p["split"] and p["with_reserve"]["split"] else "p128")
        return out
    if p["pair"]:
        out.add("pair")
        if p["edge"]:
            out.add("pair-e2")
        if (case["M"] // 32 // 2) % 2:
            out.add("pair-odd-half")
        return out
    if case["inplace"]:
        out.add("trib" if p["kernel"] == "gemm_trib_kernel" and p["nct"] == 2 else "inplace" if p["nct"] == 2 else "inplace-128")
        return out
    out.add(f"k{p['ts']}" + ("e" if p["edge"] else ""))
    if p["pipe0"]:
        out.add("pipe0")
    if p["xcd"]:
        out.add("xcd")
        if case["batch"] % 8:
            out.add("xcd-ragged-batch")
    if p["split"]:
        out.add("split")
        if 2 * p["rem"] == 2 * cus:
            out.add("split-half-round")
    elif p["ts"] == 128 and case["batch"] == 1 and 2 * p["rem"] > 2 * cus:
        out.add("nosplit")
    if p["order"] == "tri_decode":
        out.add("tri_decode")
    if p["lower_filter"]:
        out.add("lower-filter")
    if case["tri_k"]:
        out.add("tri_k")
        if case["M"] > case["K"]:
            out.add("tri_k-clamp")
    if case["tri_lo"]:
        out.add("tri_lo" if p["ts"] == 64 else "tri_lo-128")
    if case["tri_lo_b"]:
        out.add("tri_lo_b" if p["ts"] == 64 else "tri_lo_b-128")
    return out


#: every branch the tables have to reach at 256 CUs ("pipe0" exists in fp64 only)
REQUIRED = {"gemm": ["k64", "k64e", "k128", "k128e", "xcd", "xcd-ragged-batch", "split", "split-half-round", "nosplit", "tri_decode", "lower-filter",
                     "tri_k", "tri_k-clamp", "tri_lo", "tri_lo-128", "pair", "pair-e2", "pair-odd-half", "tri_lo_b", "tri_lo_b-128", "inplace",
                     "inplace-128", "trib"],
            "gemm/float64": ["pipe0"],
            "colscale": ["k128", "k128e"],
            "update2": ["p64", "p64-loop", "p128-split"]}


# -- inputs and references -------------------------------------------------------------------------------------------------------------
_CACHE = {}


def _grid(rng, shape):
    return rng.integers(64, 257, shape) / 256.0 * np.where(rng.random(shape) < 0.5, -1.0, 1.0)


def _support(rng, K, tri):
    """At most 64 positions of [0, K): the first and last position of the first, second and last chunk of both dtypes and, for
    triangular operands, the first and last position of every 32-row tile."""
    must = set()
    for b in (16, 32):
        last = (K - 1) // b * b
        must |= {0, b - 1, b, 2 * b - 1, last, K - 1}
    if tri:
        must |= {k for k in range(0, K, 32)} | {k - 1 for k in range(32, K + 1, 32)}
    assert len(must) <= 64
    return support(rng, K, must, count=64)


def _draw(rng, shape, data):
    if data.startswith("grid"):
        return _grid(rng, shape)
    d = draw(rng, shape)
    return np.abs(d) if data == "positive" else d


def _operands(rng, case, M, N, K, B, Bb):
    data = case["data"]
    a, b = _draw(rng, (B, M, K), data), _draw(rng, (Bb, N, K), data)
    m, n, k = np.arange(M)[:, None], np.arange(N)[:, None], np.arange(K)[None, :]
    if case.get("tri_k"):
        a[:, k < m] = 0.0
        b[:, k < n] = 0.0
    if case.get("tri_lo"):
        a[:, k > m] = 0.0
    if case.get("tri_lo_b") or case.get("panel"):
        b[:, k > n] = 0.0
    if data == "grid128":
        # a long triangular contraction on grid data: every third k only, so that at most 86 terms meet in an output
        a[:, :, np.arange(K) % 3 != 0] = 0.0
    elif K > DENSE_K_MAX and not data.startswith("grid"):
        keep = np.zeros(K, dtype=bool)
        keep[_support(rng, K, any(case.get(f) for f in ("tri_k", "tri_lo", "tri_lo_b", "panel")))] = True
        a[:, :, ~keep] = 0.0
    return a, b


def gemm_inputs(case):
    """``(a, b, c)``: logical (B, M, K), (B or 1, N, K) and (B, M, N) fp64 arrays of fp32 numbers; in place ``c`` is ``a``."""
    key = ("in", case["id"])
    if key in _CACHE:
        return _CACHE[key]
    rng = np.random.default_rng(case["seed"])
    M, N, K, B = case["M"], case["N"], case["K"], case["batch"]
    a, b = _operands(rng, case, M, N, K, B, 1 if case["b_bcast"] else B)
    if case["inplace"]:
        c = a
    elif case["data"].startswith("grid"):
        c = rng.integers(-65536, 65537, (B, M, N)) / 65536.0
    else:
        c = draw(rng, (B, M, N))
    if case["data"].startswith("grid"):
        assert K + abs(case["beta"] / case["alpha"]) <= 256 and case["alpha"] in (1.0, -1.0, -0.5) and case["beta"] in (0.0, 1.0)
    if not case["data"].startswith("grid"):           # (the large grid cases are cheap to draw again and too large to keep)
        _CACHE[key] = (a, b, c)
    return a, b, c


def bmm_t(a, b):
    """``a @ b^T`` of (B, M, K) and (B or 1, N, K) arrays; one B for every member as ONE product (NumPy's broadcast matmul is slow)."""
    if b.shape[0] == 1 and a.shape[0] > 1:
        return (a.reshape(-1, a.shape[2]) @ b[0].T).reshape(a.shape[0], a.shape[1], b.shape[1])
    return np.matmul(a, np.transpose(b, (0, 2, 1)))


def _reference(a, b, cin, alpha, beta, exact):
    """``(value, absum, K_eff, smallest term)``; ``exact`` (grid data): the value alone, in fp64."""
    bt = np.transpose(b, (0, 2, 1))
    if exact:
        v = alpha * bmm_t(a, b)
        return (v + beta * cin if beta else v), None, None, None
    al, bl = a.astype(LD), bt.astype(LD)
    p = np.matmul(al, bl) if a.shape[-1] else np.zeros(a.shape[:2] + (b.shape[1],), dtype=LD)
    ab = np.matmul(np.abs(al), np.abs(bl)) if a.shape[-1] else np.zeros_like(p)
    keff = np.matmul((a != 0).astype(np.float64), (bt != 0).astype(np.float64))
    val, absum = LD(alpha) * p, abs(LD(alpha)) * ab
    big = np.float64(np.inf)
    mina = np.min(np.where(a != 0, np.abs(a), big), axis=-1) if a.shape[-1] else np.full(a.shape[:2], big)
    minb = np.min(np.where(b != 0, np.abs(b), big), axis=-1) if a.shape[-1] else np.full(b.shape[:2], big)
    mt = abs(alpha) * mina[:, :, None] * minb[:, None, :]                   # a lower bound of the smallest non-zero term
    if beta:
        val, absum = val + LD(beta) * cin.astype(LD), absum + np.abs(LD(beta) * cin.astype(LD))
        mt = np.minimum(mt, np.abs(beta * cin))
    return val, absum, keff, np.where(keff > 0, mt, (np.abs(beta * cin) if beta else big))


def gemm_reference(case):
    key = ("ref", case["id"])
    if key in _CACHE:
        return _CACHE[key]
    a, b, c = gemm_inputs(case)
    ref = _reference(a, b, c, case["alpha"], case["beta"], case["data"].startswith("grid"))
    if not case["data"].startswith("grid"):
        _CACHE[key] = ref
    return ref


def detection_margin(case, dtype):
    """Smallest ``|term| / (4 (K_eff + 2) eps absum)`` over the outputs of a rounded case: at least 1 when the detection condition holds."""
    worst = np.inf
    refs = [gemm_reference(case)] if case["entry"] != "update2" else [update2_reference(case, i) for i in range(len(case["segs"]))]
    for val, absum, keff, mt in refs:
        if absum is None or not absum.size:
            continue
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(absum > 0, mt.astype(LD) / (4 * (keff + 2) * EPS[dtype] * np.where(absum > 0, absum, 1)), np.inf)
        worst = min(worst, float(r.min()))
    return worst


# -- checking ---------------------------------------------------------------------------------------------------------------------------
def _k_range(case, m, n):
    """The k range the flags leave to output (m, n), for failure messages."""
    lo, hi = 0, case["K"]
    if case.get("tri_k"):
        lo = max(m, n)
    if case.get("tri_lo"):
        hi = min(hi, m + 1)
    if case.get("tri_lo_b") or case.get("panel"):
        hi = min(hi, n + 1)
    return lo, hi


def check_product(case, dtype, got, ref, start, lower, what, path):
    """``got`` (B, M, N) against ``ref = (value, absum, K_eff, _)``; ``start``: what C held before the call (bits), looked at under
    ``lower`` only.  Returns the worst ratio to the bound (0 for grid data)."""
    val, absum, keff, _ = ref
    g64 = got.astype(np.float64)
    if absum is None:
        bad = ~(g64 == val)
        ratio = None
    else:
        err = np.abs(g64.astype(LD) - val)
        bound = (keff + 2) * EPS[dtype] * absum
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err == 0, LD(0), LD(np.inf)))
        ratio = np.where(np.isfinite(g64), ratio, LD(np.inf))
        bad = ratio > 1
    must = np.ones(got.shape[1:], dtype=bool)
    if lower:
        m, n = np.arange(got.shape[1])[:, None], np.arange(got.shape[2])[None, :]
        must = n <= m
        same = got.view(np.uint64 if got.dtype == np.float64 else np.uint32) == start.view(np.uint64 if got.dtype == np.float64 else np.uint32)
        far = (n // TILE) > (m // TILE)
        touched = far[None] & ~same
        assert not touched.any(), (f"{what} {case['id']} {dtype} [{path}]: element {tuple(int(i) for i in np.argwhere(touched)[0])} of a 128-tile strictly above "
                                   "the diagonal was written")
        bad = bad & ~(same & ~must[None])
    if bad.any():
        idx = np.argwhere(bad)
        w = idx[0] if ratio is None else idx[np.argmax(ratio[bad])]
        bi, m, n = (int(i) for i in w)
        raise AssertionError(f"{what} {case['id']} {dtype} [{path}]: {len(idx)} wrong elements, worst at (batch {bi}, m {m}, n {n}), k range {_k_range(case, m, n)}: "
                             f"got {g64[bi, m, n]!r}, reference {float(val[bi, m, n])!r}"
                             + ("" if ratio is None else f", {float(ratio[bi, m, n]):.3g} times the bound of {float(keff[bi, m, n]) + 2:.0f} eps absum"))
    if ratio is None or not ratio.size:
        return 0.0
    return float(ratio[:, must].max())


def _path(p):
    keys = ("kernel", "ts", "nct", "edge", "aligned", "pipe0", "split", "split_from", "xcd", "trib", "order")
    return " ".join(f"{k}={p[k]}" for k in keys if k in p)


def _store(arr, kmaj, dtype, device, off, pad, fill=NAN, gap=0):
    """``arr`` (B, R, K) stored (B, R + gap, off + K + pad) or, ``kmaj`` false, transposed: ``(buffer, view of the stored matrix)``."""
    s = arr if kmaj else np.transpose(arr, (0, 2, 1))
    B, R, C = s.shape
    buf = torch.full((B, R + gap, off + C + pad), fill, dtype=TORCH[dtype], device=device)
    view = buf[:, :R, off:off + C]
    view.copy_(torch.as_tensor(np.ascontiguousarray(s).astype(NP[dtype]), device=device))
    return buf, view


def _outside_is(buf, view_shape, off, fill):
    """Whether everything of ``buf`` (B, R', C') outside ``[:, :R, off:off + C]`` still holds ``fill``."""
    b = host(buf)
    mask = np.ones(b.shape, dtype=bool)
    mask[:, :view_shape[1], off:off + view_shape[2]] = False
    rest = b[mask]
    return bool(np.isnan(rest).all()) if fill != fill else bool((rest == fill).all())


def _sq(t, B):
    return t[0] if B == 1 else t


def _flags_kw(case):
    return dict(lower_only=case["lower"], tri_k=case["tri_k"], tri_k_lower=case["tri_lo"], tri_k_lower_b=case["tri_lo_b"], panel_solve=case["panel"])


def run_gemm(be, case, dtype, device):
    a, b, c = gemm_inputs(case)
    B, M, N = case["batch"], case["M"], case["N"]
    lay, p = layout(case, dtype), plan(case, dtype)
    bbuf, bv = _store(b, case["bk"], dtype, device, case["boff"], case["bpad"])
    if case["inplace"]:
        assert case["ak"] and N == case["K"]
        cbuf, ov = _store(a, True, dtype, device, 0, case["cpad"], fill=SENT, gap=case["cgap"])
        abuf, av = cbuf, ov
    else:
        abuf, av = _store(a, case["ak"], dtype, device, case["aoff"], case["apad"])
        # beta = 0 and every element written: C holds NaN on entry, it must not be read
        c0 = c if (case["beta"] or case["lower"]) else np.full(c.shape, np.nan)
        cbuf, ov = _store(c0, True, dtype, device, 0, case["cpad"], fill=SENT, gap=case["cgap"])
    start = host(ov).copy()
    a_before, b_before = host(abuf).copy(), host(bbuf).copy()
    if case["b_bcast"]:
        bv = bv.expand((B,) + tuple(bv.shape[1:]))
    av, bv, ovv = _sq(av, B), _sq(bv, B), _sq(ov, B)
    actual = all(t.data_ptr() % 16 == 0 and (t.shape[-2] == 1 or t.stride(-2) % VEC[dtype] == 0) and (t.dim() == 2 or t.stride(0) % VEC[dtype] == 0)
                 for t in (av, bv))
    assert actual == lay["aligned"] or min(av.shape[-2], bv.shape[-2]) <= 1 or case["K"] == 0, ("the layout model and the tensors disagree", case["id"])
    res = be.gemm(av, bv, a_kmajor=case["ak"], b_kmajor=case["bk"], alpha=case["alpha"], beta=case["beta"], out=ovv, **_flags_kw(case))
    sync(device)
    assert res is ovv
    r = check_product(case, dtype, host(ov), gemm_reference(case), start, case["lower"], "gemm", _path(p))
    assert _outside_is(cbuf, (B, M, N), 0, SENT), f"gemm {case['id']} {dtype} [{_path(p)}]: a sentinel in the padding of C changed"
    if not case["inplace"]:
        assert np.array_equal(host(abuf), a_before, equal_nan=True), "A changed"
    assert np.array_equal(host(bbuf), b_before, equal_nan=True), "B changed"
    return {"c": r}


# -- gpk_gemm_colscale ----------------------------------------------------------------------------------------------------------------------
def colss_rows(M):
    return 2 * cdiv(M, TILE)


def colscale_scale(case):
    return draw(np.random.default_rng(case["seed"] + 1), (case["N"],))


def colss_reference(case):
    """``(ss, bound / eps)`` per slab row and column, from the unscaled product."""
    key = ("ss", case["id"])
    if key not in _CACHE:
        a, b, _ = gemm_inputs(case)
        bt = np.transpose(b, (0, 2, 1))
        al, bl = a.astype(LD), bt.astype(LD)
        v = (LD(case["alpha"]) * np.matmul(al, bl))[0]
        absum = (abs(LD(case["alpha"])) * np.matmul(np.abs(al), np.abs(bl)))[0]
        keff = np.matmul((a != 0).astype(np.float64), (bt != 0).astype(np.float64))[0]
        R, M = colss_rows(case["M"]), case["M"]
        ss, bound = np.zeros((R, case["N"]), dtype=LD), np.zeros((R, case["N"]), dtype=LD)
        for r in range(R):
            sl = slice(64 * r, min(64 * r + 64, M))
            ss[r] = (v[sl] ** 2).sum(0)
            bound[r] = (2 * (keff[sl] + 2) * np.abs(v[sl]) * absum[sl]).sum(0) + (COLSS_DEPTH + 1) * ss[r]
        _CACHE[key] = (ss, bound, v)
    return _CACHE[key]


def colss_detection_margin(case, dtype):
    """Smallest ``v_m^2 / (4 bound)`` over the slab sums: a lost or doubled row moves a sum by at least four times its bound."""
    ss, bound, v = colss_reference(case)
    worst = np.inf
    for r in range(ss.shape[0]):
        sl = v[64 * r:64 * r + 64]
        if sl.shape[0]:
            assert (sl != 0).all()
            worst = min(worst, float(((sl ** 2).min(0) / (4 * EPS[dtype] * bound[r])).min()))
    return worst


def run_colscale(be, case, dtype, device):
    a, b, _ = gemm_inputs(case)
    M, N, mode = case["M"], case["N"], case["mode"]
    p = plan(case, dtype)
    assert p["ts"] == 128 or mode == ""
    abuf, av = _store(a, case["ak"], dtype, device, case["aoff"], case["apad"])
    bbuf, bv = _store(b, case["bk"], dtype, device, case["boff"], case["bpad"])
    cbuf, ov = _store(np.full((1, M, N), np.nan), True, dtype, device, 0, case["cpad"], fill=SENT)
    scale = colscale_scale(case) if mode in ("scale", "both") else None
    st = None if scale is None else torch.as_tensor(scale.astype(NP[dtype]), device=device)
    R = colss_rows(M)
    ssbuf = ssv = None
    if mode in ("ss", "both"):
        ssbuf = torch.full((R, N + case["sspad"]), SENT, dtype=TORCH[dtype], device=device)
        ssv = ssbuf[:, :N]
        ssv.fill_(NAN)
    flags = 2 * case["tri_k"] | 8 * case["tri_lo_b"]
    out, ss = be.gemm_colscale(av[0], bv[0], st, want_colss=ssv is not None, a_kmajor=case["ak"], b_kmajor=case["bk"], tri_k_lower=case["tri_lo"],
                               alpha=case["alpha"], flags=flags, out=ov[0], colss_rows=ssv)
    sync(device)
    val, absum, keff, mt = gemm_reference(case)
    if scale is not None:
        sl = scale.astype(LD)[None, None, :]
        ref = (val * sl, absum * np.abs(sl), keff, mt)
    else:
        ref = (val, absum, keff, mt)
    path = _path(p)
    worst = {"c": check_product(case, dtype, host(ov), ref, None, False, "gemm_colscale", path)}
    assert _outside_is(cbuf, (1, M, N), 0, SENT), f"gemm_colscale {case['id']} {dtype}: a sentinel in the padding of C changed"
    if ssv is not None:
        got = host(ssbuf)
        assert bool((got[:, N:] == SENT).all()), f"gemm_colscale {case['id']} {dtype}: the padding of colss changed"
        got = got[:, :N].astype(np.float64)
        assert np.isfinite(got).all(), (f"gemm_colscale {case['id']} {dtype} [{path}]: colss entry {tuple(int(i) for i in np.argwhere(~np.isfinite(got))[0])} "
                                        f"of {R} x {N} was left unwritten")
        ref_ss, bound, _ = colss_reference(case)
        for r in range(R):
            if 64 * r >= M:
                assert bool((got[r] == 0).all()), f"gemm_colscale {case['id']} {dtype} [{path}]: slab row {r} holds no valid row and is not exactly 0"
        err = np.abs(got.astype(LD) - ref_ss)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(bound > 0, err / (EPS[dtype] * np.where(bound > 0, bound, 1)), np.where(err == 0, 0, np.inf))
        w = np.unravel_index(np.argmax(ratio), ratio.shape)
        assert ratio[w] <= 1, (f"gemm_colscale {case['id']} {dtype} [{path}]: colss slab {int(w[0])} (rows {64 * int(w[0])}..{min(64 * int(w[0]) + 64, M) - 1}) "
                               f"column {int(w[1])}: got {got[w]!r}, reference {float(ref_ss[w])!r}, {float(ratio[w]):.3g} times the bound")
        worst["colss"] = float(ratio[w])
    if mode == "":
        # neither: the same launch as gpk_gemm with these operands -- the same bits
        c2buf, o2 = _store(np.full((1, M, N), np.nan), True, dtype, device, 0, case["cpad"], fill=SENT)
        be.gemm(av[0], bv[0], a_kmajor=case["ak"], b_kmajor=case["bk"], alpha=case["alpha"], out=o2[0], tri_k=case["tri_k"], tri_k_lower=case["tri_lo"],
                tri_k_lower_b=case["tri_lo_b"])
        sync(device)
        assert np.array_equal(host(cbuf), host(c2buf), equal_nan=True), f"gemm_colscale {case['id']} {dtype}: not the bits of gpk_gemm"
    return worst


# -- gpk_gemm_update2 -----------------------------------------------------------------------------------------------------------------------
def update2_inputs(case, i):
    key = ("u2in", case["id"], i)
    if key in _CACHE:
        return _CACHE[key]
    s = case["segs"][i]
    rng = np.random.default_rng(case["seed"] + i)
    a, b = _operands(rng, dict(data=case["data"]), s["M"], s["N"], s["K"], 1, 1)
    cin = rng.integers(-65536, 65537, (1, s["M"], s["N"])) / 65536.0 if case["data"] == "grid" else draw(rng, (1, s["M"], s["N"]))
    if case["data"] == "grid":
        assert s["K"] + abs(1 / case["alpha"]) <= 256 and case["alpha"] in (1.0, -1.0, -0.5)
    if case["data"] != "grid":
        _CACHE[key] = (a, b, cin)
    return a, b, cin


def update2_reference(case, i):
    key = ("u2ref", case["id"], i)
    if key in _CACHE:
        return _CACHE[key]
    a, b, cin = update2_inputs(case, i)
    ref = _reference(a, b, cin, case["alpha"], 1.0, case["data"] == "grid")
    if case["data"] != "grid":
        _CACHE[key] = ref
    return ref


def run_update2(be, case, dtype, device):
    p = plan(case, dtype)
    worst = {}
    results = []
    for reserve in ((0, 1) if case["both_reserves"] else (0,)):
        ups, keep = [], []
        for i, s in enumerate(case["segs"]):
            a, b, cin = update2_inputs(case, i)
            _, av = _store(a, True, dtype, device, 0, s["pad"])
            _, bv = _store(b, True, dtype, device, 0, s["pad"])
            if s["oop"]:
                _, cinv = _store(cin, True, dtype, device, 0, s["pad"] + 2)
                cbuf, cv = _store(np.full(cin.shape, SENT), True, dtype, device, 0, s["pad"], fill=SENT)
                ups.append(dict(a=av[0], b=bv[0], c=cv[0], cin=cinv[0], lower_only=s["lower"]))
            else:
                cbuf, cv = _store(cin, True, dtype, device, 0, s["pad"], fill=SENT)
                ups.append(dict(a=av[0], b=bv[0], c=cv[0], lower_only=s["lower"]))
            keep.append((cbuf, cv, host(cv).copy()))
        ctrl = torch.full((64,), GARBAGE, dtype=torch.int32, device=device)
        be.gemm_update2(ups, case["alpha"], reserve_cus=bool(reserve), ctrl=ctrl)
        sync(device)
        outs = []
        for i, (s, (cbuf, cv, start)) in enumerate(zip(case["segs"], keep)):
            got = host(cv)
            sub = dict(id=f"{case['id']} segment {i} reserve {reserve}", K=s["K"])
            r = check_product(sub, dtype, got, update2_reference(case, i), start, s["lower"], "gemm_update2", _path(p))
            worst[f"seg{i}"] = max(worst.get(f"seg{i}", 0.0), r)
            assert _outside_is(cbuf, got.shape, 0, SENT), f"gemm_update2 {sub['id']} {dtype}: a sentinel in the padding of C changed"
            outs.append(got.copy())
        results.append(outs)
    if len(results) == 2:
        for i, (x, y) in enumerate(zip(*results)):
            if case["segs"][i]["lower"]:
                # above the diagonal a diagonal tile is written as a whole or, cut into quarters, not at all -- and which tiles are cut
                # depends on the workgroups that leave
                x, y = np.tril(x), np.tril(y)
            assert np.array_equal(x, y), f"gemm_update2 {case['id']} {dtype}: segment {i} differs between reserve_cus = 0 and 1"
    return worst


RUNNERS = {"gemm": run_gemm, "colscale": run_colscale, "update2": run_update2}


def run(be, case, dtype, device):
    """Run one case (a rounded one only after its detection condition has been checked); prints and returns the worst ratios."""
    if not case["data"].startswith("grid"):
        m = detection_margin(case, dtype)
        assert m >= 1.0, ("a term is smaller than four times the bound", case["id"], dtype, m)
    worst = RUNNERS[case["entry"]](be, case, dtype, device)
    for k, v in worst.items():
        print(f"RATIO {case['entry']} {dtype} {k} {v:.3f} {case['id']}")
    return worst


def drop_cache():
    _CACHE.clear()


# -- refusals ---------------------------------------------------------------------------------------------------------------------------------
def _refused(fn, code, what):
    try:
        fn()
    except RuntimeError as e:
        assert f"status {code}" in str(e) and what in str(e), (str(e), code)
    else:
        raise AssertionError(f"{what} accepted what it should refuse with status {code}")


def _bits(t):
    return host(t).copy().view(np.uint8)


def run_gemm_refusals(be, dtype, device):
    T = TORCH[dtype]
    rng = np.random.default_rng(5)
    mk = lambda *s: torch.as_tensor(draw(rng, s).astype(NP[dtype]), device=device)      # noqa: E731
    a, b = mk(70, 40), mk(50, 40)
    cbuf = torch.full((70, 53), SENT, dtype=T, device=device)
    c = cbuf[:, :50]
    before = _bits(cbuf)
    _refused(lambda: be.gemm(a, b, alpha=0.0, beta=1.0, out=c), -6, "gpk_gemm")
    # ldc >= 2^25 (two rows that far apart)
    wide = torch.full((2 ** 25 + 64,), SENT, dtype=T, device=device)
    cw = torch.as_strided(wide, (2, 50), (2 ** 25, 1))
    _refused(lambda: be.gemm(a[:2], b, out=cw), -15, "gpk_gemm")
    sync(device)
    assert bool((wide[:64] == SENT).all()) and bool((wide[2 ** 25:] == SENT).all())
    del wide, cw
    # batch > 65535
    ab, bb, cb = mk(65536, 1, 1), mk(1, 1, 1), torch.full((65536, 1, 1), SENT, dtype=T, device=device)
    _refused(lambda: be.gemm(ab, bb, out=cb), -3, "gpk_gemm")
    sync(device)
    assert bool((cb == SENT).all())
    # in place with N > 128, and C aliasing B
    p = mk(70, 192)
    w = mk(192, 192)
    pb = _bits(p)
    _refused(lambda: be.gemm(p, w, out=p), -16, "gpk_gemm")
    sq = mk(64, 64)
    sb = _bits(sq)
    _refused(lambda: be.gemm(mk(64, 64), sq, out=sq), -16, "gpk_gemm")
    sync(device)
    assert np.array_equal(_bits(p), pb) and np.array_equal(_bits(sq), sb)
    # nothing to do: M, N or the batch empty -- status 0, C untouched
    be.gemm(a[:0], b, out=cbuf[:0, :50])
    be.gemm(a, b[:0], out=cbuf[:, :0])
    be.gemm(a.reshape(1, 70, 40)[:0], b.reshape(1, 50, 40)[:0], out=cbuf.reshape(1, 70, 53)[:0, :, :50])
    sync(device)
    assert np.array_equal(_bits(cbuf), before), "a refused or empty gpk_gemm wrote to C"


def run_colscale_refusals(be, dtype, device):
    T = TORCH[dtype]
    rng = np.random.default_rng(6)
    mk = lambda *s: torch.as_tensor(draw(rng, s).astype(NP[dtype]), device=device)      # noqa: E731
    a, b, s = mk(70, 40), mk(50, 40), mk(50)
    cbuf = torch.full((70, 53), SENT, dtype=T, device=device)
    c = cbuf[:, :50]
    ssb = torch.full((2, 50), SENT, dtype=T, device=device)
    before, ss_before = _bits(cbuf), _bits(ssb)
    _refused(lambda: be.gemm_colscale(a, b, s, out=c, flags=1), -13, "gpk_gemm_colscale")
    _refused(lambda: be.gemm_colscale(a, b, s, out=c, flags=16), -13, "gpk_gemm_colscale")
    short = torch.as_strided(ssb, (2, 50), (49, 1))
    _refused(lambda: be.gemm_colscale(a, b, None, want_colss=True, out=c, colss_rows=short), -17, "gpk_gemm_colscale")
    sq = mk(40, 40)
    sqb = _bits(sq)
    _refused(lambda: be.gemm_colscale(sq, mk(40, 40), mk(40), out=sq), -17, "gpk_gemm_colscale")
    _refused(lambda: be.gemm_colscale(mk(40, 40), sq, mk(40), out=sq), -17, "gpk_gemm_colscale")
    sync(device)
    assert np.array_equal(_bits(cbuf), before) and np.array_equal(_bits(ssb), ss_before) and np.array_equal(_bits(sq), sqb)


def run_update2_refusals(be, dtype, device):
    T = TORCH[dtype]
    rng = np.random.default_rng(7)
    mk = lambda *s: torch.as_tensor(draw(rng, s).astype(NP[dtype]), device=device)      # noqa: E731
    a, b = mk(70, 40), mk(50, 40)
    cbuf = torch.full((70, 53), SENT, dtype=T, device=device)
    u = dict(a=a, b=b, c=cbuf[:, :50])
    ctrl = torch.full((64,), GARBAGE, dtype=torch.int32, device=device)
    before = _bits(cbuf)
    _refused(lambda: be.gemm_update2([u, u, u], -1.0, ctrl=ctrl), -2, "gpk_gemm_update2")
    _refused(lambda: be.gemm_update2([dict(a=a[:, :0], b=b[:, :0], c=cbuf[:, :50])], -1.0, ctrl=ctrl), -1, "gpk_gemm_update2")
    _refused(lambda: be.gemm_update2([u], 0.0, ctrl=ctrl), -3, "gpk_gemm_update2")
    _refused(lambda: be.gemm_update2([u], -1.0, ctrl=0), -4, "gpk_gemm_update2")
    sync(device)
    assert np.array_equal(_bits(cbuf), before), "a refused gpk_gemm_update2 wrote to C"
