"""Cases, extended-precision references and runners for the kernels that consume the Cholesky factor: the reductions and the clean-up
kernels of ``stheno_amd/csrc/gpk_reduce.hip`` and the GEMV, the triangular solves and the triangular inverse of ``gpk_solve.hip``.

``tests/test_linalg_kernels_gpu.py`` runs every case over ``HipBackend`` on the GPU, ``tests/test_linalg_reference_host.py`` runs the same
runners over the test-only CPU backend, shows that the bounds admit a correct implementation and that each of a list of single defects
is caught.  Nothing here touches a GPU: the runners take the backend and the device.

**Inputs.**  Magnitudes are log-uniform in [0.25, 1] with random signs and are fp32 numbers, so one reference serves both dtypes.

**Summing kernels** (rowreduce, colreduce, gemv, logdet_chol, sum_lower).  The reference is computed in ``np.longdouble`` from the
rounded inputs; every output element gets its value and ``absum``, the sum of the absolute values of the terms that make it up
(``|beta y|`` included for gemv).  Acceptance: ``|got - ref| <= (depth + 2) * eps * absum``, ``depth`` being the length of the longest
addition chain of the kernel's fixed summation order (``depth_*`` below, derived from the code, not fitted) and the two extra units the
roundings of ``alpha * s`` and ``+ beta * y`` (or of the final ``2 * s``); logdet gets 4 more for the device ``log``.

**Detection condition** (``detection_margin``, asserted for every summing case by the host test): every non-zero term of every output is
at least ``4 * (depth + 2) * eps * absum`` in magnitude, so losing any one element, row, column, chunk or right-hand side moves an
output by four times the bound or more.  Dense fp32 data meets it up to n of about 4600 (``DENSE_MAX``); the longer cases (colreduce
over 131073 rows, gemv over two 4096-column staging chunks) are zero outside 64 positions that include the first and last position of
the first, second and last chunk, and the condition is about those.

**Element-wise kernels** (tril, symmetrize, add_diag, scale_cols, copy): the same bits as NumPy in the working dtype, sentinels in the
padding and between batch members unchanged.

**Solves** (tri_solve_ over its three paths, trtri): per column ``max|x - ref| <= 1000 eps max|ref|`` against SciPy in fp64 on the rounded
factor, the figure the native self-test applies block-wise."""
import math

import numpy as np
import scipy.linalg as sla
import torch

LD = np.longdouble
EPS = {"float64": LD(2.0) ** -52, "float32": LD(2.0) ** -23}
VEC = {"float64": 2, "float32": 4}            # elements per 16-byte vector
NP = {"float64": np.float64, "float32": np.float32}
TORCH = {"float64": torch.float64, "float32": torch.float32}
BITS = {"float64": np.uint64, "float32": np.uint32}
DTYPES = ("float64", "float32")
SENT = 7.0                                    # sentinel in padding that must stay as it is
DENSE_MAX = 4600                              # longest dense sum that meets the detection condition in fp32
SOLVE_UNITS = 1000                            # selftest.cpp's figure for trsv / trsm, here per column
ALPHA, BETA = -0.75, 0.5


def gemv_chunk(nrhs):
    """Columns of x staged per pass (``GemvChunk<NR>``; NR = 1, 2, 4, 8 for 1, 2, 3-4, 5-8 right-hand sides)."""
    return 4096 if nrhs == 1 else (2048 if nrhs == 2 else 512)


# -- summation depths (longest addition chain of each kernel's fixed order) -------------------------------------------------------------
def depth_rowreduce(n, dtype):
    """One wave per row: a lane adds up at most ``ceil(n / 64) + VEC`` products, then six shuffle steps."""
    return -(-n // 64) + VEC[dtype] + 6


def depth_gemv(k, dtype):
    """As rowreduce: the staging chunks split a lane's run, they do not reorder it."""
    return -(-k // 64) + VEC[dtype] + 6


def colreduce_chunks(rows):
    """``(rch, nchunk)`` of ``gpk_colreduce_launch``: 128-row chunks doubled until there are at most 1024 (``gpk_colreduce_nchunks_impl``),
    then the rows spread evenly over that many chunks."""
    rch = 128
    while -(-rows // rch) > 1024:
        rch *= 2
    nchunk = -(-max(rows, 1) // rch)
    return -(-max(rows, 1) // nchunk), nchunk


def depth_colreduce(rows):
    """A thread runs down its chunk of ``rch`` rows, the second kernel adds the ``nchunk`` partial sums in order."""
    rch, nchunk = colreduce_chunks(rows)
    return rch + nchunk


def logdet_threads(n, batch):
    return 1024 if (batch <= 16 and n >= 4096) else 256


def depth_logdet(n, batch):
    """``ceil(n / NT)`` logs per thread, six shuffle steps, ``NT / 64`` wave sums added in order."""
    nt = logdet_threads(n, batch)
    return -(-n // nt) + 6 + nt // 64


def depth_sum_lower(S):
    return S


def units(kernel, case, dtype):
    """The acceptance bound of a summing case in units of ``eps * absum``."""
    if kernel == "rowreduce":
        return depth_rowreduce(case["n"], dtype) + 2
    if kernel == "gemv":
        return depth_gemv(case["K"], dtype) + 2
    if kernel == "colreduce":
        return depth_colreduce(case["rows"]) + 2
    if kernel == "logdet":
        return depth_logdet(case["n"], case["batch"]) + 2 + 4
    if kernel == "sum_lower":
        return depth_sum_lower(case["S"]) + 2
    raise KeyError(kernel)


SUMMING = ("rowreduce", "colreduce", "gemv", "logdet", "sum_lower")


def ratios(got, ref, absum, dtype):
    """``|got - ref| / (eps * absum)`` element by element; an element nothing is added up for (absum = 0) has to be exactly 0: +inf if
    not, and so is anything that is not finite."""
    got = np.asarray(got, dtype=np.float64).astype(LD)
    ref, absum = np.asarray(ref, dtype=LD), np.asarray(absum, dtype=LD)
    assert got.shape == ref.shape == absum.shape, (got.shape, ref.shape, absum.shape)
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(absum > 0, err / (EPS[dtype] * np.where(absum > 0, absum, 1)), np.where(err == 0, LD(0), LD(np.inf)))
    return np.where(np.isfinite(got), r, LD(np.inf))


# -- inputs -----------------------------------------------------------------------------------------------------------------------------
def draw(rng, shape):
    """Log-uniform magnitudes in [0.25, 1], random signs, rounded to fp32 (held in fp64)."""
    m = 0.25 * 4.0 ** rng.random(shape)
    s = np.where(rng.random(shape) < 0.5, -1.0, 1.0)
    return np.clip((m * s).astype(np.float32).astype(np.float64), -1.0, 1.0)


def support(rng, n, must, count=64):
    """``count`` sorted positions in [0, n) that include ``must``."""
    must = sorted({int(i) for i in must if 0 <= i < n})
    rest = np.setdiff1d(np.arange(n), must)
    extra = rng.choice(rest, size=max(0, min(count, n) - len(must)), replace=False)
    return np.sort(np.concatenate([must, extra]).astype(np.int64))


def place(arr, dtype, device, pad=0, fill=float("nan"), off=0):
    """``arr`` (..., R, C) in a buffer (..., R, off + C + pad) filled with ``fill``: ``(buffer, view)``, the view holds ``arr``."""
    arr = np.asarray(arr)
    C = arr.shape[-1]
    buf = torch.full(arr.shape[:-1] + (off + C + pad,), fill, dtype=TORCH[dtype], device=device)
    view = buf[..., off:off + C]
    view.copy_(torch.as_tensor(arr.astype(NP[dtype]), device=device))
    return buf, view


def padding_is(buf, off, C, fill):
    """Whether everything of ``buf`` outside the columns [off, off + C) still holds ``fill``."""
    b = buf.detach().cpu().numpy()
    rest = np.concatenate([b[..., :off], b[..., off + C:]], axis=-1)
    return bool(np.isnan(rest).all()) if isinstance(fill, float) and math.isnan(fill) else bool((rest == fill).all())


def dev(a, dtype, device):
    return torch.as_tensor(np.ascontiguousarray(np.asarray(a).astype(NP[dtype])), device=device)


def host(t):
    return t.detach().cpu().numpy()


def same_bits(got, ref, dtype):
    got, ref = np.ascontiguousarray(got), np.ascontiguousarray(np.asarray(ref, dtype=NP[dtype]))
    return got.dtype == ref.dtype and got.shape == ref.shape and bool((got.view(BITS[dtype]) == ref.view(BITS[dtype])).all())


def sync(device):
    if str(device).startswith("cuda"):
        torch.cuda.synchronize()


# -- case tables ------------------------------------------------------------------------------------------------------------------------
def _case(kernel, seed, edges, **kw):
    name = f"{kernel}{seed}-" + "-".join(f"{k}{v}" for k, v in kw.items() if not isinstance(v, (tuple, list)))
    return dict(kernel=kernel, id=name, seed=seed, edges=tuple(edges), **kw)


def rowreduce_cases(dtype):
    V = VEC[dtype]
    U = 64 * V * 4                                      # one unrolled step of the vector path
    ns = [(1, "1"), (63, "63"), (64, "64"), (65, "65"), (U - V, "64*VEC*4-VEC"), (U, "64*VEC*4"), (U + V, "64*VEC*4+VEC"), (1025, "1025"),
          (4100, "4100")]
    rows = [1, 3, 4, 5, 9]
    want = ["both", "dot", "ss"]
    cs = []
    for i, (n, lab) in enumerate(ns):
        r, wt = rows[i % 5], want[i % 3]
        cs.append(_case("rowreduce", 100 + i, [f"n={lab}", f"rows={r}", f"want={wt}"], rows=r, n=n, pad=0, off=0, want=wt))
    cs.append(_case("rowreduce", 120, ["ld=n+VEC with NaN padding", "rows=5", "want=both"], rows=5, n=U, pad=V, off=0, want="both"))
    cs.append(_case("rowreduce", 121, ["ld=n+VEC with NaN padding", "n=64*VEC*4-VEC"], rows=9, n=U - V, pad=V, off=0, want="both"))
    cs.append(_case("rowreduce", 122, ["odd ld (scalar path)"], rows=5, n=U, pad=1, off=0, want="both"))
    cs.append(_case("rowreduce", 123, ["view z[:, 1:] (scalar path)"], rows=3, n=U, pad=V - 1, off=1, want="both"))
    cs.append(_case("rowreduce", 124, ["w=None with ss"], rows=4, n=U + V, pad=0, off=0, want="ss_no_w"))
    cs.append(_case("rowreduce", 125, ["w=None with ss", "odd ld (scalar path)"], rows=9, n=65, pad=0, off=0, want="ss_no_w"))
    return cs


def colreduce_cases(dtype):
    rows = [1, 127, 128, 129, 257, 1000]
    cols = [1, 255, 256, 257, 300]
    want = ["both", "dot", "ss"]
    cs = []
    for i in range(10):
        r, c = rows[i % 6], cols[i % 5]
        b, pad, wt = (3 if i % 2 else 1), (5 if i % 3 == 1 else 0), want[i % 3]
        e = [f"rows={r}", f"cols={c}", f"batch={b}", f"want={wt}"] + (["padded ld"] if pad else [])
        cs.append(_case("colreduce", 200 + i, e, rows=r, cols=c, batch=b, pad=pad, want=wt))
    cs.append(_case("colreduce", 220, ["131073 x 2 sparse: chunk 256, 513 chunks"], rows=131073, cols=2, batch=1, pad=0, want="both", sparse=1))
    return cs


def gemv_cases(dtype):
    V = VEC[dtype]
    Ms = [1, 15, 16, 17, 33]
    cs = []
    for j, nrhs in enumerate((1, 2, 3, 4, 5, 8)):
        ch = gemv_chunk(nrhs)
        for i, (K, lab) in enumerate([(1, "1"), (65, "65"), (ch - 1, "chunk-1"), (ch, "chunk"), (ch + V, "chunk+VEC"), (2 * ch + 3, "2*chunk+3")]):
            M, beta = Ms[(i + j) % 5], (BETA if (i + j) % 2 else 0.0)
            e = [f"nrhs={nrhs}", f"K={lab}", f"M={M}", f"nrhs={nrhs} K={lab}", "alpha=-0.75",
                 "beta=0.5" if beta else "beta=0 into NaN output"]
            cs.append(_case("gemv", 300 + 10 * j + i, e, M=M, K=K, nrhs=nrhs, batch=1, pad=0, off=0, beta=beta, sparse=int(K > DENSE_MAX)))
    for i, beta in enumerate((0.0, BETA)):
        cs.append(_case("gemv", 380 + i, ["batch=3 padded lda/ldx/ldy", "beta=0.5" if beta else "beta=0 into NaN output"],
                        M=17, K=65 + V - 65 % V, nrhs=3, batch=3, pad=V, off=0, beta=beta, sparse=0))
    cs.append(_case("gemv", 390, ["view a[:, 1:] (scalar path)"], M=17, K=64, nrhs=2, batch=1, pad=V - 1, off=1, beta=BETA, sparse=0))
    cs.append(_case("gemv", 391, ["view a[:, 1:] (scalar path)", "batch=3 padded lda/ldx/ldy"], M=33, K=512 + V, nrhs=8, batch=3, pad=2 * V - 1, off=1,
                    beta=0.0, sparse=0))
    return cs


def logdet_cases(dtype):
    cs = []
    i = 0
    for n in (1, 255, 256, 257, 2047, 2048, 2049):
        for b in (1, 3):
            pad = 3 if (i % 3 == 0 and n > 1) else 0
            cs.append(_case("logdet", 400 + i, [f"n={n}", f"batch={b}", "NaN off the diagonal"] + (["padded ld"] if pad else []), n=n, batch=b, pad=pad))
            i += 1
    for n in (4096, 8191, 8192, 8193):
        pad = 3 if n == 8191 else 0
        cs.append(_case("logdet", 400 + i, [f"n={n}", "batch=1", "1024 threads", "NaN off the diagonal"] + (["padded ld"] if pad else []), n=n, batch=1, pad=pad))
        i += 1
    if dtype == "float32":
        cs.append(_case("logdet", 430, ["n=4096 batch=16 (1024 threads)"], n=4096, batch=16, pad=0))
        cs.append(_case("logdet", 431, ["n=4096 batch=17 (256 threads)"], n=4096, batch=17, pad=0))
    return cs


def _tri_cases(kernel, base):
    cs = []
    for i, n in enumerate((1, 15, 16, 17, 31, 32, 33, 255, 256, 257, 513)):
        b, pad = (3 if i % 2 else 1), (3 if i % 3 != 2 else 0)
        cs.append(_case(kernel, base + i, [f"n={n}", f"batch={b}"] + (["padded ld with sentinels"] if pad else []), n=n, batch=b, pad=pad))
    cs.append(_case(kernel, base + 20, ["n=257", "batch=3", "padded ld with sentinels"], n=257, batch=3, pad=1))
    cs.append(_case(kernel, base + 21, ["n=33", "batch=1"], n=33, batch=1, pad=0))
    return cs


def tril_cases(dtype):
    return _tri_cases("tril", 500)


def symmetrize_cases(dtype):
    return _tri_cases("symmetrize", 540)


def add_diag_cases(dtype):
    cs = []
    modes = ["s", "v", "both"]
    i = 0
    for n in (1, 255, 256, 257):
        for k in range(2):
            mode = modes[(i + k) % 3]
            b, pad = (3 if k else 1), (3 if (i + k) % 2 else 0)
            e = [f"n={n}", f"mode={mode}"] + (["batched v"] if b > 1 and mode != "s" else []) + (["padded"] if pad else [])
            cs.append(_case("add_diag", 600 + 2 * i + k, e, n=n, batch=b, pad=pad, mode=mode))
        i += 1
    cs.append(_case("add_diag", 620, ["n=257", "mode=both", "batched v", "padded"], n=257, batch=3, pad=3, mode="both"))
    cs.append(_case("add_diag", 621, ["n=256", "mode=s"], n=256, batch=1, pad=0, mode="s"))
    return cs


def _rect_cases(kernel, base):
    rows = [1, 7, 8, 9, 100]
    cs = []
    for i, c in enumerate((1, 63, 64, 65, 255, 256, 257)):
        r, b = rows[i % 5], (3 if i % 2 else 1)
        pad, off = (3 if i % 3 else 0), (1 if i % 3 == 2 else 0)
        e = [f"rows={r}", f"cols={c}", f"batch={b}"] + (["padded"] if pad else []) + (["offset"] if off else [])
        cs.append(_case(kernel, base + i, e, rows=r, cols=c, batch=b, pad=pad, off=off))
    cs.append(_case(kernel, base + 10, ["rows=9", "cols=257", "batch=3", "padded", "offset"], rows=9, cols=257, batch=3, pad=2, off=1))
    cs.append(_case(kernel, base + 11, ["rows=100", "cols=256", "batch=3", "padded"], rows=100, cols=256, batch=3, pad=4, off=0))
    return cs


def scale_cols_cases(dtype):
    return _rect_cases("scale_cols", 700)


def copy_cases(dtype):
    return _rect_cases("copy", 740)


def sum_lower_cases(dtype):
    ns = (511, 512, 513) if dtype == "float64" else (1023, 1024, 1025, 1030)
    cs = []
    for i, n in enumerate(ns):
        S = (1, 2, 7)[i % 3]
        cs.append(_case("sum_lower", 800 + i, [f"n={256 * VEC[dtype]}{n - 256 * VEC[dtype]:+d}", f"S={S}", "second column block"], n=n, S=S, ppad=0, poff=0,
                        opad=0))
    n = ns[-1]
    cs.append(_case("sum_lower", 810, ["misaligned parts view (scalar loads)", "S=7"], n=n, S=7, ppad=VEC[dtype] - 1, poff=1, opad=0))
    cs.append(_case("sum_lower", 811, ["odd ldo (scalar stores)", "S=2"], n=ns[1], S=2, ppad=0, poff=0, opad=1))
    cs.append(_case("sum_lower", 812, ["misaligned parts view (scalar loads)", "odd ldo (scalar stores)", "S=1"], n=ns[0], S=1, ppad=VEC[dtype] - 1, poff=1,
                    opad=1 + ns[0] % 2))
    return cs


def tri_solve_cases(dtype):
    cs = []
    ns = (1, 127, 128, 129, 300)
    # the sweep: a launch pair per diagonal block
    k = 0
    for i, n in enumerate(ns):
        for j, nrhs in enumerate((1, 2, 3, 4, 5, 8)):
            b, sb = (1, 3, 63)[(i + j) % 3], (128, 256)[(i + j // 3) % 2]
            cs.append(_case("tri_solve", 900 + k, ["sweep", f"batch={b}", f"nrhs={nrhs}", f"n={n}", f"sb={sb}", "padded ldb", "padded factor ld"],
                            path="sweep", n=n, nrhs=nrhs, batch=b, sb=sb, lpad=(8, 3)[k % 2], bpad=1 + k % 3))
            k += 1
    # one workgroup per matrix (batch >= 64, sb = 128; nrhs <= 2 in fp64, <= 4 in fp32 -- fp64 with 3 or 4 columns falls back to the sweep)
    k = 0
    for i, n in enumerate(ns):
        for j, nrhs in enumerate((1, 2, 3, 4)):
            b = (64, 67)[(i + j) % 2]
            e = ["one workgroup per matrix", f"batch={b}", f"nrhs={nrhs}", f"n={n}", "padded ldb", "padded factor ld"]
            if nrhs == 3 and b == 64:
                e.append("fp64 nrhs=3 batch=64 falls back to the sweep")
            cs.append(_case("tri_solve", 950 + k, e, path="batched", n=n, nrhs=nrhs, batch=b, sb=128, lpad=(8, 3)[k % 2], bpad=1 + k % 3))
            k += 1
    if dtype == "float32":
        cs.append(_case("tri_solve", 980, ["LDS boundary: n=4096 nrhs=4 (64 KB, one workgroup)", "batch stride 0"], path="batched", n=4096, nrhs=4, batch=64,
                        sb=128, lpad=8, bpad=4, expand=1))
        cs.append(_case("tri_solve", 981, ["LDS boundary: n=4097 nrhs=4 (sweep)", "batch stride 0"], path="batched", n=4097, nrhs=4, batch=64, sb=128, lpad=7,
                        bpad=4, expand=1))
    # blocked out-of-place solve (more than 8 right-hand sides)
    k = 0
    for nrhs in (9, 130):
        for n in (129, 300, 700):
            for b in (1, 3):
                cs.append(_case("tri_solve", 990 + k, ["blocked", f"nrhs={nrhs}", f"n={n}", f"batch={b}", "padded ldb", "padded factor ld"], path="blocked", n=n,
                                nrhs=nrhs, batch=b, sb=(128, 256)[k % 2], lpad=(8, 3)[k % 2], bpad=1 + k % 3))
                k += 1
    return cs


def trtri_cases(dtype):
    cs = []
    k = 0
    for n in (1, 127, 128, 129, 300, 700):
        for sb in (128, 256):
            cs.append(_case("trtri", 1100 + k, [f"n={n}", f"sb={sb}"], n=n, sb=sb, lpad=(0, 8, 3)[k % 3]))
            k += 1
    return cs


CASES = {"rowreduce": rowreduce_cases, "colreduce": colreduce_cases, "gemv": gemv_cases, "logdet": logdet_cases, "tril": tril_cases,
         "symmetrize": symmetrize_cases, "add_diag": add_diag_cases, "scale_cols": scale_cols_cases, "copy": copy_cases,
         "sum_lower": sum_lower_cases, "tri_solve": tri_solve_cases, "trtri": trtri_cases}


def all_cases(kernel):
    """``[(case, dtype)]`` of a kernel, for parametrising."""
    return [(c, dt) for dt in DTYPES for c in CASES[kernel](dt)]


def case_id(p):
    return p["id"] if isinstance(p, dict) else str(p)


#: the edges every table has to hold, by their strings (checked by the host test for both dtypes unless a dtype is named)
REQUIRED_EDGES = {
    "rowreduce": [f"rows={r}" for r in (1, 3, 4, 5, 9)] + [f"n={n}" for n in ("1", "63", "64", "65", "64*VEC*4-VEC", "64*VEC*4", "64*VEC*4+VEC", "1025", "4100")]
    + ["ld=n+VEC with NaN padding", "odd ld (scalar path)", "view z[:, 1:] (scalar path)", "want=dot", "want=ss", "want=both", "w=None with ss"],
    "colreduce": [f"rows={r}" for r in (1, 127, 128, 129, 257, 1000)] + [f"cols={c}" for c in (1, 255, 256, 257, 300)]
    + ["batch=1", "batch=3", "padded ld", "want=dot", "want=ss", "want=both", "131073 x 2 sparse: chunk 256, 513 chunks"],
    "gemv": [f"nrhs={r} K={k}" for r in (1, 2, 3, 4, 5, 8) for k in ("1", "65", "chunk-1", "chunk", "chunk+VEC", "2*chunk+3")]
    + [f"M={m}" for m in (1, 15, 16, 17, 33)] + ["alpha=-0.75", "beta=0 into NaN output", "beta=0.5", "batch=3 padded lda/ldx/ldy", "view a[:, 1:] (scalar path)"],
    "logdet": [f"n={n}" for n in (1, 255, 256, 257, 2047, 2048, 2049, 4096, 8191, 8192, 8193)] + ["batch=1", "batch=3", "NaN off the diagonal", "padded ld"],
    "logdet/float32": ["n=4096 batch=16 (1024 threads)", "n=4096 batch=17 (256 threads)"],
    "tril": [f"n={n}" for n in (1, 15, 16, 17, 31, 32, 33, 255, 256, 257, 513)] + ["batch=1", "batch=3", "padded ld with sentinels"],
    "symmetrize": [f"n={n}" for n in (1, 15, 16, 17, 31, 32, 33, 255, 256, 257, 513)] + ["batch=1", "batch=3", "padded ld with sentinels"],
    "add_diag": [f"n={n}" for n in (1, 255, 256, 257)] + ["mode=s", "mode=v", "mode=both", "batched v", "padded"],
    "scale_cols": [f"rows={r}" for r in (1, 7, 8, 9, 100)] + [f"cols={c}" for c in (1, 63, 64, 65, 255, 256, 257)] + ["batch=3", "padded", "offset"],
    "copy": [f"rows={r}" for r in (1, 7, 8, 9, 100)] + [f"cols={c}" for c in (1, 63, 64, 65, 255, 256, 257)] + ["batch=3", "padded", "offset"],
    "sum_lower": ["S=1", "S=2", "S=7", "second column block", "misaligned parts view (scalar loads)", "odd ldo (scalar stores)"],
    "sum_lower/float64": ["n=512-1", "n=512+0", "n=512+1"],
    "sum_lower/float32": ["n=1024-1", "n=1024+0", "n=1024+1", "n=1024+6"],
    "tri_solve": ["sweep", "one workgroup per matrix", "blocked", "padded ldb", "padded factor ld", "fp64 nrhs=3 batch=64 falls back to the sweep"]
    + [f"batch={b}" for b in (1, 3, 63, 64, 67)] + [f"nrhs={r}" for r in (1, 2, 3, 4, 5, 8, 9, 130)] + [f"n={n}" for n in (1, 127, 128, 129, 300, 700)]
    + ["sb=128", "sb=256"],
    "tri_solve/float32": ["LDS boundary: n=4096 nrhs=4 (64 KB, one workgroup)", "LDS boundary: n=4097 nrhs=4 (sweep)", "batch stride 0"],
    "trtri": [f"n={n}" for n in (1, 127, 128, 129, 300, 700)] + ["sb=128", "sb=256"],
}


# -- references of the summing kernels: {output: (value, absum, smallest non-zero |term|)} in longdouble ----------------------------------
_CACHE = {}


def _minnz(a, axis):
    a = np.abs(np.asarray(a, dtype=np.float64))
    return np.min(np.where(a > 0, a, np.inf), axis=axis)


def rowreduce_inputs(case):
    rng = np.random.default_rng(case["seed"])
    return draw(rng, (case["rows"], case["n"])), draw(rng, (case["n"],))


def rowreduce_reference(case):
    key = ("rowreduce", case["id"])
    if key not in _CACHE:
        z, w = rowreduce_inputs(case)
        zl, wl = z.astype(LD), w.astype(LD)
        t = zl * wl[None, :]
        _CACHE[key] = {"dot": (t.sum(-1), np.abs(t).sum(-1), _minnz(t, -1)), "ss": ((zl * zl).sum(-1), (zl * zl).sum(-1), _minnz(zl * zl, -1))}
    return _CACHE[key]


def colreduce_inputs(case):
    rng = np.random.default_rng(case["seed"])
    B, R, C = case["batch"], case["rows"], case["cols"]
    v, w = draw(rng, (B, R, C)), draw(rng, (B, R))
    if case.get("sparse"):
        rch, nchunk = colreduce_chunks(R)
        keep = support(rng, R, [0, rch - 1, rch, 2 * rch - 1, (nchunk - 1) * rch, R - 1])
        mask = np.zeros(R, dtype=bool)
        mask[keep] = True
        v[:, ~mask, :] = 0.0
    return v, w


def colreduce_reference(case):
    key = ("colreduce", case["id"])
    if key not in _CACHE:
        v, w = colreduce_inputs(case)
        vl, wl = v.astype(LD), w.astype(LD)
        t = vl * wl[:, :, None]
        _CACHE[key] = {"dot": (t.sum(1), np.abs(t).sum(1), _minnz(t, 1)), "ss": ((vl * vl).sum(1), (vl * vl).sum(1), _minnz(vl * vl, 1))}
    return _CACHE[key]


def gemv_inputs(case):
    rng = np.random.default_rng(case["seed"])
    B, M, K, R = case["batch"], case["M"], case["K"], case["nrhs"]
    a, x, y = draw(rng, (B, M, K)), draw(rng, (B, K, R)), draw(rng, (B, M, R))
    if case["sparse"]:
        ch = gemv_chunk(R)
        keep = support(rng, K, [0, ch - 1, ch, 2 * ch - 1, 2 * ch, K - 2, K - 1])
        mask = np.zeros(K, dtype=bool)
        mask[keep] = True
        a[:, :, ~mask] = 0.0
    return a, x, y


def gemv_reference(case):
    key = ("gemv", case["id"])
    if key not in _CACHE:
        a, x, y = gemv_inputs(case)
        al, xl, yl = a.astype(LD), x.astype(LD), y.astype(LD)
        s = np.einsum("bmk,bkr->bmr", al, xl)
        ab = np.einsum("bmk,bkr->bmr", np.abs(al), np.abs(xl))
        beta = LD(case["beta"])
        val = LD(ALPHA) * s + beta * yl
        absum = abs(LD(ALPHA)) * ab + np.abs(beta * yl)
        # (a lower bound of the smallest term: the smallest entry of the row times the smallest entry of the column)
        mt = abs(ALPHA) * _minnz(a, -1)[:, :, None] * _minnz(x, 1)[:, None, :]
        if case["beta"]:
            mt = np.minimum(mt, np.abs(case["beta"] * y))
        _CACHE[key] = {"y": (val, absum, mt)}
    return _CACHE[key]


def logdet_inputs(case):
    rng = np.random.default_rng(case["seed"])
    return (2.0 + 2.0 * rng.random((case["batch"], case["n"]))).astype(np.float32).astype(np.float64)


def logdet_reference(case):
    key = ("logdet", case["id"])
    if key not in _CACHE:
        t = 2 * np.log(logdet_inputs(case).astype(LD))
        _CACHE[key] = {"logdet": (t.sum(-1), np.abs(t).sum(-1), _minnz(t, -1))}
    return _CACHE[key]


def sum_lower_inputs(case):
    rng = np.random.default_rng(case["seed"])
    return draw(rng, (case["S"], case["n"], case["n"]))


def sum_lower_reference(case):
    key = ("sum_lower", case["id"])
    if key not in _CACHE:
        p = sum_lower_inputs(case).astype(LD)
        _CACHE[key] = {"out": (p.sum(0), np.abs(p).sum(0), _minnz(p, 0))}
    return _CACHE[key]


REFERENCES = {"rowreduce": rowreduce_reference, "colreduce": colreduce_reference, "gemv": gemv_reference, "logdet": logdet_reference,
              "sum_lower": sum_lower_reference}


def detection_margin(kernel, case, dtype):
    """Smallest ``|term| / (4 * units * eps * absum)`` over the outputs of a summing case: at least 1 when the detection condition holds."""
    u = units(kernel, case, dtype)
    worst = np.inf
    for val, absum, mt in REFERENCES[kernel](case).values():
        worst = min(worst, float(np.min(np.asarray(mt, dtype=LD) / (4 * u * EPS[dtype] * np.asarray(absum, dtype=LD)))))
    return worst


def _accept(kernel, case, dtype, name, got, worst):
    """Check one output of a summing case against the a-priori bound; records the worst ratio in ``worst``."""
    val, absum, _ = REFERENCES[kernel](case)[name]
    r = float(np.max(ratios(got, val, absum, dtype))) if np.size(val) else 0.0
    worst[name] = max(worst.get(name, 0.0), r)
    assert r <= units(kernel, case, dtype), (kernel, case["id"], dtype, name, r, units(kernel, case, dtype))


# -- runners: run one case over a backend, assert, return {output: worst ratio} -----------------------------------------------------------
def run_rowreduce(be, case, dtype, device):
    z, w = rowreduce_inputs(case)
    rows, n = z.shape
    buf, zv = place(z, dtype, device, pad=case["pad"], off=case["off"])
    assert "odd ld (scalar path)" not in case["edges"] or zv.stride(0) % 2 == 1
    assert "view z[:, 1:] (scalar path)" not in case["edges"] or (zv.data_ptr() % 16 != 0 and zv.stride(0) % VEC[dtype] == 0)
    wt = case["want"]
    wv = None if wt == "ss_no_w" else dev(w, dtype, device)
    dot, ss = be.rowreduce(zv, wv, want_dot=wt in ("dot", "both", "ss_no_w"), want_ss=wt in ("ss", "both", "ss_no_w"))
    sync(device)
    assert (dot is not None) == (wt in ("dot", "both")) and (ss is not None) == (wt != "dot")
    worst = {}
    for name, got in (("dot", dot), ("ss", ss)):
        if got is not None:
            assert tuple(got.shape) == (rows,)
            _accept("rowreduce", case, dtype, name, host(got), worst)
    assert padding_is(buf, case["off"], n, float("nan"))
    return worst


def run_colreduce(be, case, dtype, device):
    v, w = colreduce_inputs(case)
    B, R, C = v.shape
    buf, vv = place(v, dtype, device, pad=case["pad"])
    wv = dev(w, dtype, device)
    if B == 1:
        vv, wv = vv[0], wv[0]
    wt = case["want"]
    dot, ss = be.colreduce(vv, wv if wt != "ss" else None, want_dot=wt != "ss", want_ss=wt != "dot")
    sync(device)
    assert (dot is not None) == (wt != "ss") and (ss is not None) == (wt != "dot")
    worst = {}
    for name, got in (("dot", dot), ("ss", ss)):
        if got is not None:
            _accept("colreduce", case, dtype, name, host(got).reshape(B, C), worst)
    return worst


def run_gemv(be, case, dtype, device):
    a, x, y = gemv_inputs(case)
    B, M, K = a.shape
    R, pad, beta = case["nrhs"], case["pad"], case["beta"]
    _, av = place(a, dtype, device, pad=pad, off=case["off"])
    _, xv = place(x, dtype, device, pad=pad)
    obuf, ov = place(y if beta else np.full(y.shape, np.nan), dtype, device, pad=pad, fill=SENT)
    assert "view a[:, 1:] (scalar path)" not in case["edges"] or (av.data_ptr() % 16 != 0 and av.stride(-2) % VEC[dtype] == 0 and K % VEC[dtype] == 0)
    if B == 1:
        av, xv, ov = av[0], xv[0], ov[0]
    res = be.gemv(av, xv, alpha=ALPHA, beta=beta, out=ov)
    sync(device)
    assert res is ov
    worst = {}
    _accept("gemv", case, dtype, "y", host(ov).reshape(B, M, R), worst)
    assert padding_is(obuf, 0, R, SENT)
    return worst


def run_gemv_refuses_nine_columns(be, dtype, device):
    """nrhs = 9 is refused and the output stays as it was."""
    rng = np.random.default_rng(9)
    a, x = dev(draw(rng, (17, 65)), dtype, device), dev(draw(rng, (65, 9)), dtype, device)
    out = torch.full((17, 9), SENT, dtype=TORCH[dtype], device=device)
    try:
        be.gemv(a, x, alpha=ALPHA, beta=0.0, out=out)
    except RuntimeError as e:
        assert "gemv" in str(e)
    else:
        raise AssertionError("gemv accepted nine right-hand sides")
    sync(device)
    assert bool((host(out) == SENT).all())


def run_logdet(be, case, dtype, device):
    d = logdet_inputs(case)
    B, n = d.shape
    buf = torch.full((B, n, n + case["pad"]), float("nan"), dtype=TORCH[dtype], device=device)
    lv = buf[..., :n]
    torch.diagonal(lv, dim1=-2, dim2=-1).copy_(dev(d, dtype, device))
    got = be.logdet_chol(lv[0] if B == 1 else lv)
    sync(device)
    worst = {}
    _accept("logdet", case, dtype, "logdet", host(got).reshape(B), worst)
    return worst


def _square_inputs(case):
    rng = np.random.default_rng(case["seed"])
    return draw(rng, (case["batch"], case["n"], case["n"]))


def run_tril(be, case, dtype, device):
    a = _square_inputs(case)
    B, n, _ = a.shape
    buf, av = place(a, dtype, device, pad=case["pad"], fill=SENT)
    res = be.tril_(av[0] if B == 1 else av)
    sync(device)
    assert res.data_ptr() == av.data_ptr()
    assert same_bits(host(av), np.tril(a.astype(NP[dtype])), dtype)
    assert padding_is(buf, 0, n, SENT)
    return {}


def run_symmetrize(be, case, dtype, device):
    a = _square_inputs(case)
    B, n, _ = a.shape
    low = np.tril(a).astype(NP[dtype])
    start = low.copy()
    iu = np.triu_indices(n, 1)
    start[:, iu[0], iu[1]] = np.nan                      # what is mirrored over is never read
    buf, av = place(start, dtype, device, pad=case["pad"], fill=SENT)
    be.symmetrize_(av[0] if B == 1 else av)
    sync(device)
    got = host(av)
    assert same_bits(np.tril(got), low, dtype), "the lower triangle changed"
    assert same_bits(got, low + np.transpose(np.tril(low, -1), (0, 2, 1)), dtype)
    assert padding_is(buf, 0, n, SENT)
    return {}


def run_add_diag(be, case, dtype, device):
    a = _square_inputs(case)
    B, n, _ = a.shape
    rng = np.random.default_rng(case["seed"] + 1)
    v = draw(rng, (B, n)) if case["mode"] != "s" else None
    s = 0.3 if case["mode"] != "v" else 0.0              # (0.3 is no fp32 number: the kernel adds T(s))
    buf, av = place(a, dtype, device, pad=case["pad"], fill=SENT)
    vt = None if v is None else dev(v, dtype, device)
    be.add_diag_(av[0] if B == 1 else av, s, vt[0] if (B == 1 and vt is not None) else vt)
    sync(device)
    T = NP[dtype]
    ref = a.astype(T)
    idx = np.arange(n)
    add = np.full((B, n), T(s), dtype=T)
    if v is not None:
        add = add + v.astype(T)
    ref[:, idx, idx] = ref[:, idx, idx] + add            # a + (T(s) + v): one rounding per addition
    assert same_bits(host(av), ref, dtype)
    assert padding_is(buf, 0, n, SENT)
    return {}


def _rect_inputs(case):
    rng = np.random.default_rng(case["seed"])
    return draw(rng, (case["batch"], case["rows"], case["cols"])), draw(rng, (case["batch"], case["cols"]))


def run_scale_cols(be, case, dtype, device):
    v, s = _rect_inputs(case)
    B, R, C = v.shape
    buf, vv = place(v, dtype, device, pad=case["pad"], off=case["off"], fill=SENT)
    st = dev(s, dtype, device)
    be.scale_cols_(vv[0] if B == 1 else vv, st[0] if B == 1 else st)
    sync(device)
    T = NP[dtype]
    assert same_bits(host(vv), v.astype(T) * s.astype(T)[:, None, :], dtype)
    assert padding_is(buf, case["off"], C, SENT)
    return {}


def run_copy(be, case, dtype, device):
    v, _ = _rect_inputs(case)
    B, R, C = v.shape
    buf, vv = place(v, dtype, device, pad=case["pad"], off=case["off"])
    src = vv[0] if B == 1 else vv
    out = be.copy(src)
    sync(device)
    assert tuple(out.shape) == tuple(src.shape) and (out.stride(-1) == 1 or C == 1) and out.data_ptr() != src.data_ptr()
    assert same_bits(host(out).reshape(B, R, C), v.astype(NP[dtype]), dtype)
    assert same_bits(host(vv), v.astype(NP[dtype]), dtype) and padding_is(buf, case["off"], C, float("nan"))
    return {}


def run_sum_lower(be, case, dtype, device):
    p = sum_lower_inputs(case)
    S, n, _ = p.shape
    start = p.copy()
    iu = np.triu_indices(n, 1)
    start[:, iu[0], iu[1]] = np.nan                      # strictly above the diagonal of a part: never part of a sum
    _, pv = place(start, dtype, device, pad=case["ppad"], off=case["poff"])
    obuf = torch.full((n, n + case["opad"]), SENT, dtype=TORCH[dtype], device=device)
    ov = obuf[:, :n]
    assert "misaligned parts view (scalar loads)" not in case["edges"] or pv.data_ptr() % 16 != 0
    assert "odd ldo (scalar stores)" not in case["edges"] or ov.stride(0) % 2 == 1
    res = be.sum_lower(pv, ov)
    sync(device)
    assert res is ov
    got = host(obuf)
    upper = np.triu(np.ones((n, n + case["opad"]), dtype=bool), 1)
    assert bool((got[upper] == SENT).all()), "something strictly above the diagonal of `out` (or in its padding) was written"
    val, absum, _ = sum_lower_reference(case)["out"]
    il = np.tril_indices(n)
    r = float(np.max(ratios(got[:, :n][il], val[il], absum[il], dtype)))
    assert r <= units("sum_lower", case, dtype), (case["id"], dtype, r)
    return {"out": r}


# -- solves -------------------------------------------------------------------------------------------------------------------------------
_FACTORS = {}


def _spd(n, batch, seed):
    """Well conditioned SPD matrices (as ``_factor`` of tests/test_posterior_grad_gpu.py): eigenvalues in [0.5, about 4.5]."""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((batch, n, n + 8)) / math.sqrt(n + 8)
    return a @ np.transpose(a, (0, 2, 1)) + 0.5 * np.eye(n)


def factor(be, n, batch, sb, lpad, seed, dtype, device):
    """``(l, dinv_sb, L64)``: the factor by the backend's own ``potrf_`` in a buffer with leading dimension n + lpad, NaN strictly above its
    diagonal, the inverted ``sb`` diagonal blocks (``None`` over the CPU stand-in), and the rounded factor in fp64 (lower triangle)."""
    key = (n, batch, sb, lpad, seed, dtype)
    if be.name != "hip" and key in _FACTORS:
        L64 = _FACTORS[key]
        _, lv = place(L64, dtype, device, pad=lpad, fill=0.0)
        dsb = None
    else:
        _, lv = place(_spd(n, batch, seed), dtype, device, pad=lpad, fill=0.0)
        dinv, info = be.potrf_(lv)[:2]
        assert int(info.abs().max()) == 0
        dsb = dinv if (sb == 128 or dinv is None) else be.trtri_merge(lv, dinv, sb)
        L64 = np.tril(host(lv).astype(np.float64))
        if be.name != "hip":
            _FACTORS[key] = L64
    iu = torch.triu_indices(n, n, 1, device=lv.device)
    lv[:, iu[0], iu[1]] = float("nan")
    return lv, dsb, L64


def solve_rhs(case):
    rng = np.random.default_rng(case["seed"] + 7)
    b = draw(rng, (case["batch"], case["n"], case["nrhs"])) * np.array([1.0, 1e3, 1e-3])[np.arange(case["nrhs"]) % 3]
    return b.astype(np.float32).astype(np.float64)


def column_ratios(x, ref, dtype):
    """``max_i |x - ref| / (eps * max_i |ref|)`` per column of (..., n, nrhs) arrays."""
    x, ref = np.asarray(x, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert x.shape == ref.shape
    r = np.abs(x - ref).max(-2) / (float(EPS[dtype]) * np.abs(ref).max(-2))
    return np.where(np.isfinite(x).all(-2), r, np.inf)


def run_tri_solve(be, case, dtype, device):
    n, B, R, sb = case["n"], case["batch"], case["nrhs"], case["sb"]
    b = solve_rhs(case)
    if case.get("expand"):
        # one factor for every member (batch stride 0: the ABI adds b * sl), the block inverses contiguous per member, the right-hand sides differ
        lv, dsb, L64 = factor(be, n, 1, sb, case["lpad"], case["seed"], dtype, device)
        lv = lv.expand(B, n, n)
        dsb = None if dsb is None else dsb.expand((B,) + tuple(dsb.shape[1:])).contiguous()
        assert lv.stride(0) == 0
        ref = sla.solve_triangular(L64[0], np.concatenate(list(b), axis=1), lower=True, check_finite=False)
        ref = np.stack(np.split(ref, B, axis=1))
    else:
        lv, dsb, L64 = factor(be, n, B, sb, case["lpad"], case["seed"], dtype, device)
        ref = np.stack([sla.solve_triangular(L64[i], b[i], lower=True, check_finite=False) for i in range(B)])
    bbuf, bv = place(b, dtype, device, pad=case["bpad"], fill=SENT)
    if B == 1:
        lv, bv = lv[0], bv[0]
    x = be.tri_solve_(lv, dsb, sb, bv)
    sync(device)
    assert (x is bv) == (R <= 8) or be.name != "hip"
    r = column_ratios(host(x).reshape(B, n, R), ref, dtype)
    assert float(r.max()) <= SOLVE_UNITS, (case["id"], dtype, r.max(), np.unravel_index(np.argmax(r), r.shape))
    assert padding_is(bbuf, 0, R, SENT)
    return {"x": float(r.max())}


def run_trtri(be, case, dtype, device):
    n, sb = case["n"], case["sb"]
    lv, dsb, L64 = factor(be, n, 1, sb, case["lpad"], case["seed"], dtype, device)
    w = be.trtri(lv[0], None if dsb is None else dsb[0], sb)
    sync(device)
    W = host(w).astype(np.float64)
    assert W.shape == (n, n) and bool((np.triu(W, 1) == 0).all()), "the strict upper triangle of the inverse is not exactly zero"
    r = column_ratios(W, sla.solve_triangular(L64[0], np.eye(n), lower=True, check_finite=False), dtype)
    assert float(r.max()) <= SOLVE_UNITS, (case["id"], dtype, r.max())
    res = np.abs(W @ L64[0] - np.eye(n)).max(-1) / float(EPS[dtype])          # row-wise residual, against the rows of I (max 1)
    assert float(res.max()) <= SOLVE_UNITS, (case["id"], dtype, res.max())
    return {"w": float(r.max()), "residual": float(res.max())}


RUNNERS = {"rowreduce": run_rowreduce, "colreduce": run_colreduce, "gemv": run_gemv, "logdet": run_logdet, "tril": run_tril,
           "symmetrize": run_symmetrize, "add_diag": run_add_diag, "scale_cols": run_scale_cols, "copy": run_copy, "sum_lower": run_sum_lower,
           "tri_solve": run_tri_solve, "trtri": run_trtri}


def run(be, case, dtype, device):
    """Run one case (a summing case only after its detection condition has been checked); prints the worst ratio per output (``-s`` shows
    them) and returns them."""
    if case["kernel"] in SUMMING:
        m = detection_margin(case["kernel"], case, dtype)
        assert m >= 1.0, ("a term is smaller than four times the bound", case["id"], dtype, m)
    worst = RUNNERS[case["kernel"]](be, case, dtype, device)
    for k, v in worst.items():
        print(f"RATIO {case['kernel']} {dtype} {k} {v:.3f} {case['id']}")
    return worst
