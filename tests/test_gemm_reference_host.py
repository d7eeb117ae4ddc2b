"""The cases, references, bounds and launch-plan model of ``tests/gemm_reference.py`` on the CPU: the runners of
``tests/test_gemm_kernels_gpu.py`` over a NumPy backend, so that

* every case passes for a correct implementation in both dtypes (the bounds are a-priori ones: this shows that they are not too tight);
* the detection condition holds for every rounded case and every ``colss`` case;
* each of a list of single defects makes at least one case fail in both dtypes;
* the case tables reach every branch of ``gpk_gemm_launch2`` and ``gpk_gemm_persist_launch`` at 256 CUs, and the constants of the plan
  model are the ones in the sources.

``HostBackend`` is ``OracleBackend`` with NumPy versions of ``gemm``, ``gemm_colscale`` and ``gemm_update2`` that honour the flags (the k loop
runs over the chunks the flags leave to a 64-row tile), the layouts, ``lower_only`` (whole 64-tiles on or below the diagonal) and in-place
use, round once per output and refuse what the library refuses."""
import os
import re

import numpy as np
import pytest
import torch

from . import gemm_reference as R
from .conftest import OracleBackend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _refuse(what, code):
    raise RuntimeError(f"libgpk {what} failed with status {code}")


def _np64(t):
    return np.array(t.detach().numpy(), dtype=np.float64, order="C")


class HostBackend(OracleBackend):
    #: the one defect of a ``Defective`` backend
    defect = None

    def _product(self, A, Bm, dtype, ts, tri_k=False, tri_lo=False, tri_lo_b=False):
        """``sum_k a b`` of (B, M, K) and (B or 1, N, K) arrays over the k chunks the flags leave to every ``ts``-row tile."""
        d = self.defect
        bk = 16 if dtype == torch.float64 else 32
        M, K, N = A.shape[1], A.shape[2], Bm.shape[1]
        m, n, k = np.arange(M)[:, None], np.arange(N)[:, None], np.arange(K)[None, :]
        ma, mb = np.ones((M, K), dtype=bool), np.ones((N, K), dtype=bool)
        if tri_k:
            ma &= k >= (m // ts * ts) // bk * bk + (bk if d == "tri_k_first_chunk" else 0)
        if tri_lo:
            ma &= k < R.cdiv((m // ts + 1) * ts, bk) * bk - (bk if d == "tri_lo_stops_early" else 0)
        if tri_lo_b:
            mb &= k < R.cdiv((n // ts + 1) * ts, bk) * bk - (bk if d == "tri_lo_stops_early" else 0)
        if d == "last_k" and K % bk:
            ma &= k < K - 1
        if d == "neighbour" and A.shape[0] > 1:
            A = np.concatenate([A[:1], A[:1], A[2:]])
        return R.bmm_t(A * ma, Bm * mb)

    def gemm(self, a, b, *, a_kmajor=True, b_kmajor=True, alpha=1.0, beta=0.0, out=None, lower_only=False, tri_k=False, tri_k_lower=False,
             tri_k_lower_b=False, panel_solve=False, _cin=None):
        d = self.defect
        if d == "layouts_swapped":
            if a.shape[-1] == a.shape[-2]:
                a_kmajor = not a_kmajor
            elif b.shape[-1] == b.shape[-2]:
                b_kmajor = not b_kmajor
        A = a if a_kmajor else a.transpose(-1, -2)
        Bm = b if b_kmajor else b.transpose(-1, -2)
        A3, B3, O3 = (t if t.dim() == 3 else t.unsqueeze(0) for t in (A, Bm, out))
        batch, M, N = max(A3.shape[0], B3.shape[0]), A3.shape[1], B3.shape[1]
        if M <= 0 or N <= 0 or batch <= 0:
            return out
        inplace = out.data_ptr() == a.data_ptr()
        if batch > 65535:
            _refuse("gpk_gemm", -3)
        if alpha == 0.0:
            _refuse("gpk_gemm", -6)
        if M > 1 and O3.stride(1) >= 2 ** 25:
            _refuse("gpk_gemm", -15)
        if (inplace and N > 128) or out.data_ptr() == b.data_ptr():
            _refuse("gpk_gemm", -16)
        if d == "no_beta":
            beta = 0.0
        C0 = _np64(O3)
        P = self._product(_np64(A3), _np64(B3), out.dtype, 64, tri_k, tri_k_lower, tri_k_lower_b)
        res = alpha * P + (beta * (C0 if _cin is None else _np64(_cin).reshape(C0.shape)) if beta != 0.0 else 0.0)
        m, n = np.arange(M)[:, None], np.arange(N)[None, :]
        W = np.ones((M, N), dtype=bool)
        if lower_only:
            W = (n // 64) <= (m // 64)
            if d == "upper_tile" and N > 128:
                W = W | ((m < 128) & (n >= 128) & (n < 256))
        if d == "last_row" and M % 64:
            W[M - 1, :] = False
        if d == "last_col" and N % 64:
            W[:, N - 1] = False
        if d == "quarter" and M > 2048 and N > 2048 and batch == 1:
            W[(M - 1) // 64 * 64:, (N - 1) // 64 * 64:] = False
        if d == "inplace_race" and inplace and N > 64:
            # the columns from 64 on are computed after the first 64 have been written over the operand
            A2 = _np64(A3).copy()
            A2[:, :, :64] = res[:, :, :64]
            res[:, :, 64:] = (alpha * self._product(A2, _np64(B3), out.dtype, 64, tri_k, tri_k_lower, tri_k_lower_b))[:, :, 64:]
        new = torch.as_tensor(np.where(W[None], res, C0), dtype=torch.float64).to(out.dtype)
        O3.copy_(torch.where(torch.as_tensor(W)[None], new, O3))
        return out

    def gemm_colscale(self, a, b, colscale=None, *, want_colss=False, a_kmajor=True, b_kmajor=True, tri_k_lower=False, alpha=1.0, flags=0, out=None,
                      colss_rows=None):
        d = self.defect
        A = (a if a_kmajor else a.transpose(-1, -2)).unsqueeze(0)
        Bm = (b if b_kmajor else b.transpose(-1, -2)).unsqueeze(0)
        M, N = A.shape[1], Bm.shape[1]
        flags = int(flags) | (4 if tri_k_lower else 0)
        if colss_rows is not None and colss_rows.stride(0) < N:
            _refuse("gpk_gemm_colscale", -17)
        if flags & ~(2 | 4 | 8):
            _refuse("gpk_gemm_colscale", -13)
        fused = colscale is not None or want_colss or colss_rows is not None
        if fused and out is not None and out.data_ptr() in (a.data_ptr(), b.data_ptr()):
            _refuse("gpk_gemm_colscale", -17)
        v = alpha * self._product(_np64(A), _np64(Bm), a.dtype, 128 if fused else 64, bool(flags & 2), bool(flags & 4), bool(flags & 8))[0]
        s = None if colscale is None else _np64(colscale).reshape(1, -1)
        res = torch.as_tensor(v if s is None else v * s, dtype=torch.float64).to(a.dtype)
        if out is None:
            out = res
        else:
            out.copy_(res)
        if not (want_colss or colss_rows is not None):
            return out, None
        rows = R.colss_rows(M)
        vv = v * s if (d == "colss_scaled" and s is not None) else v
        part = np.zeros((rows, N))
        for r in range(rows):
            sl = vv[64 * r:min(64 * r + 64, M)]
            part[r] = (sl ** 2).sum(0)
            if d == "colss_clamped":
                part[r] += (64 - sl.shape[0]) * vv[M - 1] ** 2
        part = torch.as_tensor(part, dtype=torch.float64).to(a.dtype)
        if colss_rows is None:
            return out, part.sum(0)
        for r in range(rows):
            if not (d == "colss_unwritten" and 64 * r >= M):
                colss_rows[r].copy_(part[r])
        return out, colss_rows

    def gemm_update2(self, updates, alpha, reserve_cus=False, ctrl=None):
        d = self.defect
        if not 1 <= len(updates) <= 2:
            _refuse("gpk_gemm_update2", -2)
        if isinstance(ctrl, int) and ctrl == 0:
            _refuse("gpk_gemm_update2", -4)
        if alpha == 0.0:
            _refuse("gpk_gemm_update2", -3)
        if any(u["a"].shape[1] <= 0 for u in updates):
            _refuse("gpk_gemm_update2", -1)
        for i, u in enumerate(updates):
            if d == "second_segment" and i == 1:
                continue
            c = u["c"]
            if c.shape[0] == 0 or c.shape[1] == 0:
                continue
            cin = u.get("cin")
            if cin is None or cin.data_ptr() == c.data_ptr() or d == "cin_ignored":
                cin = None
            self.gemm(u["a"], u["b"], alpha=alpha, beta=1.0, out=c, lower_only=bool(u.get("lower_only")), _cin=cin)
        if ctrl is not None:
            ctrl.zero_()
        return [u["c"] for u in updates]


class Defective(HostBackend):
    """``HostBackend`` with ONE defect, named by ``self.defect``."""

    def __init__(self, defect):
        self.defect = defect


#: defect -> (what it is, the entry points of which at least one case has to fail)
DEFECTS = {
    "last_k": ("loses the last k of a ragged chunk", ["gemm", "colscale"]),
    "tri_k_first_chunk": ("loses the first chunk under tri_k", ["gemm", "colscale"]),
    "tri_lo_stops_early": ("stops the k loop of tri_k_lo / tri_k_lo_b one chunk early", ["gemm", "colscale"]),
    "layouts_swapped": ("reads a square operand in the other layout", ["gemm"]),
    "no_beta": ("ignores beta", ["gemm", "update2"]),
    "cin_ignored": ("reads c where it should read cin", ["update2"]),
    "last_row": ("loses the last row of a ragged tile", ["gemm", "update2"]),
    "last_col": ("loses the last column of a ragged tile", ["gemm", "update2"]),
    "quarter": ("loses one quarter tile", ["gemm"]),
    "neighbour": ("computes one batch member from its neighbour's operand", ["gemm"]),
    "upper_tile": ("writes a 128-tile strictly above the diagonal under lower_only", ["gemm", "update2"]),
    "inplace_race": ("computes the columns from 64 on from rows it has already overwritten", ["gemm"]),
    "colss_unwritten": ("leaves a colss slab row without valid rows unwritten", ["colscale"]),
    "colss_clamped": ("adds a clamped copy of row M - 1 to colss for every row past M", ["colscale"]),
    "colss_scaled": ("takes colss from the scaled product", ["colscale"]),
    "second_segment": ("drops the second segment of update2", ["update2"]),
}

ALL = [(c, dt) for e in R.CASES for c, dt in R.all_cases(e)]


@pytest.fixture(autouse=True, scope="module")
def _references_are_dropped_afterwards():
    yield
    R.drop_cache()


@pytest.mark.parametrize("case,dtype", ALL, ids=R.case_id)
def test_every_case_passes_over_the_host_backend(case, dtype):
    R.run(HostBackend(), case, dtype, "cpu")


@pytest.mark.parametrize("dtype", R.DTYPES)
def test_refusals_of_the_host_backend(dtype):
    be = HostBackend()
    R.run_gemm_refusals(be, dtype, "cpu")
    R.run_colscale_refusals(be, dtype, "cpu")
    R.run_update2_refusals(be, dtype, "cpu")


@pytest.mark.parametrize("case,dtype", [p for p in ALL if not p[0]["data"].startswith("grid")], ids=R.case_id)
def test_detection_condition(case, dtype):
    """Every non-zero term of every output is at least four times the acceptance bound; every row of a colss slab moves its sum by
    four times the bound of the sum."""
    m = R.detection_margin(case, dtype)
    assert m >= 1.0, (case["id"], dtype, m)
    if case["entry"] == "colscale" and case["mode"] in ("ss", "both"):
        assert case["data"] == "positive"
        a, b, _ = R.gemm_inputs(case)
        assert (a >= 0).all() and (b >= 0).all()
        if not (case["tri_k"] or case["tri_lo"] or case["tri_lo_b"]):
            m = R.colss_detection_margin(case, dtype)
            assert m >= 1.0, (case["id"], dtype, m)


def test_dense_data_meets_the_detection_condition_up_to_360():
    eps = 2.0 ** -23
    assert 1 / 16 >= 4 * (360 + 2) * 360 * eps and not 1 / 16 >= 4 * (368 + 2) * 368 * eps
    assert R.DENSE_K_MAX == 360 and R.COLSS_DEPTH == 16 + 2


def test_grid_data_is_exact_in_fp32_in_any_order():
    """A permuted fp32 accumulation at K = 255 reproduces the fp64 product bit for bit."""
    rng = np.random.default_rng(0)
    a, b = R._grid(rng, (16, 255)), R._grid(rng, (12, 255))
    ref = a @ b.T
    perm = rng.permutation(255)
    acc = np.zeros((16, 12), dtype=np.float32)
    for k in perm:
        acc = acc + a[:, k].astype(np.float32)[:, None] * b[:, k].astype(np.float32)[None, :]
    assert acc.dtype == np.float32 and np.array_equal(acc.astype(np.float64), ref)


def _fails(be, case, dtype):
    try:
        R.RUNNERS[case["entry"]](be, case, dtype, "cpu")
    except AssertionError:
        return True
    return False


def _cost(c):
    if c["entry"] == "update2":
        return sum(s["M"] * s["N"] for s in c["segs"])
    return c["M"] * c["N"] * c["batch"]


@pytest.mark.parametrize("dtype", R.DTYPES)
@pytest.mark.parametrize("defect,entry", [(d, e) for d, (_, es) in DEFECTS.items() for e in es])
def test_a_single_defect_is_caught(defect, entry, dtype):
    be = Defective(defect)
    cases = sorted(R.CASES[entry](dtype), key=_cost)
    assert any(_fails(be, c, dtype) for c in cases), f"no {entry} case notices a backend that {DEFECTS[defect][0]}"


@pytest.mark.parametrize("dtype", R.DTYPES)
@pytest.mark.parametrize("entry", list(R.CASES))
def test_the_tables_reach_every_branch_at_256_cus(entry, dtype):
    have = set()
    for c in R.CASES[entry](dtype):
        got = R.branches(c, dtype, 256)
        missing = [w for w in c["want"] if w not in got and not (w == "pipe0" and dtype == "float32")]
        assert not missing, (c["id"], dtype, missing, got, R.plan(c, dtype))
        have |= got
    want = R.REQUIRED[entry] + R.REQUIRED.get(f"{entry}/{dtype}", [])
    assert not [w for w in want if w not in have], [w for w in want if w not in have]


def test_the_plan_names_the_kernels():
    for dtype in R.DTYPES:
        by_id = {c["id"]: c for c in R.gemm_cases(dtype)}
        for name in ("pair-256x64x256-MKNK", "pair-512x100x512-MKKN", "pair-320x64x320"):
            assert R.plan(by_id[name], dtype)["kernel"] == "gemm_trilo_pair_kernel"
        assert R.plan(by_id["pair-512x100x512-MKNK"], dtype)["edge"] and not R.plan(by_id["pair-256x64x256-MKNK"], dtype)["edge"]
        for name in ("inplace-64x128-panel", "inplace-3001x128-ld131-panel", "inplace-b3-200x128-panel", "inplace-300x100-ld128-panel"):
            p = R.plan(by_id[name], dtype)
            assert p["kernel"] == "gemm_trib_kernel" and (p["ts"], p["nct"]) == (64, 2), (name, p)
        p = R.plan(by_id["inplace-300x128-KN-panel"], dtype)
        assert p["kernel"] == "gemm_kernel" and (p["ts"], p["nct"]) == (128, 1)
        assert R.plan(by_id["inplace-64x128"], dtype)["kernel"] == "gemm_kernel"
        for c in by_id.values():
            p = R.plan(c, dtype)
            assert p["pipe0"] == (dtype == "float64" and not p["aligned"] and not c["inplace"] and not p["pair"]), (c["id"], p)
        assert R.plan(by_id["split-2944x2944x32-KMKN"], dtype)["split_from"] == 512 and R.plan(by_id["split-2944x2944x32-KMKN"], dtype)["rem"] == 17
        assert R.plan(by_id["split-3072x4096x32"], dtype)["rem"] == 256 and R.plan(by_id["split-lower-4000x4000x40"], dtype)["tiles"] == 528
        assert R.plan(by_id["nosplit-3072x4224x32"], dtype)["rem"] == 280 and not R.plan(by_id["nosplit-3072x4224x32"], dtype)["split"]
        assert R.plan(by_id["k128-b32-512x512x32"], dtype)["tiles"] * 32 == 512 and R.plan(by_id["k64-b31-512x512x32"], dtype)["ts"] == 64
        u = {c["id"]: R.plan(c, dtype) for c in R.update2_cases(dtype)}
        assert u["u2-2560sq+256x128-K32"]["tiles"] == 828 and not u["u2-2560sq+256x128-K32"]["loops"]
        assert u["u2-2880sq+256x128-K32"]["tiles"] == 1043 and u["u2-2880sq+256x128-K32"]["loops"]
        assert u["u2-4096sq+128x256-K32"]["tiles"] == 530 and u["u2-4096sq+128x256-K32"]["split_from"] == 512
        assert u["u2-4096sq+128x256-K32"]["with_reserve"]["split_from"] == 496


def test_the_constants_of_the_plan_are_the_ones_in_the_sources():
    def src(name):
        with open(os.path.join(ROOT, "stheno_amd", "csrc", name)) as f:
            return f.read()
    gemm, common, capi = src("gpk_gemm.hip"), src("gpk_common.hpp"), src("gpk_capi.hip")
    assert int(re.search(r"GPK_KNOB\(int64_t, g_small_tile_below, (\d+)\)", gemm).group(1)) == R.SMALL_TILE_BELOW
    assert int(re.search(r"GPK_KNOB\(int64_t, g_persist_small_below, (\d+)\)", gemm).group(1)) == R.PERSIST_SMALL_BELOW
    for knob in ("g_trib", "g_xcd_batch", "g_trilo_pairs", "g_split_tail"):
        assert re.search(r"GPK_KNOB\(int, %s, 1\)" % knob, gemm), knob
    assert int(re.search(r"#define GPK_TILE (\d+)", common).group(1)) == R.TILE
    assert [int(v) for v in re.findall(r"static constexpr int VEC = (\d+);", common)] == [R.VEC["float64"], R.VEC["float32"]]
    assert [int(v) for v in re.findall(r"static constexpr int BK = (\d+);", common)] == [R.BK["float64"], R.BK["float32"]]
    assert "const int64_t slots = (int64_t)device_cus() * 2;" in gemm and "const int per_cu = (ts == 128) ? 2 : 4;" in gemm
    assert "batch >= 64" in gemm and "M % 64 == 0 && M >= 256" in gemm
    assert re.search(r"gpk_gemm_colss_rows\(int64_t m\) \{ return 2 \* gpk_cdiv\(m, GPK_TILE\); \}", capi)
    assert float(np.finfo(np.longdouble).eps) < 2e-19, "the references need an extended-precision long double"
