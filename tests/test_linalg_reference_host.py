"""The cases, references, depths and bounds of ``tests/linalg_reference.py`` on the CPU: the runners of ``tests/test_linalg_kernels_gpu.py``
over the test-only backend of ``tests/conftest.py``, so that

* every case passes for a correct implementation in both dtypes (the bounds are a-priori ones: this shows that they are not too tight);
* the detection condition holds for every summing case;
* each of a list of single defects makes at least one case of every kernel it touches fail;
* the case tables hold every edge they were written for.

``HostBackend`` is ``OracleBackend`` with the three places restated where the stand-in is looser than ``HipBackend``'s contract and no
host logic depends on it: ``sum_lower`` writes nothing above the diagonal, ``add_diag_`` adds ``T(s) + v`` in one go, ``gemv`` refuses
more than eight right-hand sides.  A factor shared by every batch member (batch stride 0) is solved in one call."""
import numpy as np
import pytest
import torch

from . import linalg_reference as R
from .conftest import OracleBackend


class HostBackend(OracleBackend):
    def sum_lower(self, parts, out):
        n = out.shape[0]
        il = torch.tril_indices(n, n)
        out[il[0], il[1]] = parts[:, il[0], il[1]].sum(0)
        return out

    def add_diag_(self, a, s=0.0, v=None):
        d = torch.diagonal(a, dim1=-2, dim2=-1)
        add = torch.full(d.shape, float(s), dtype=a.dtype)
        if v is not None:
            add = add + v.reshape(d.shape)
        d += add
        return a

    def gemv(self, a, x, *, alpha=1.0, beta=0.0, out=None):
        if x.shape[-1] > 8:
            raise RuntimeError("gemv: at most eight right-hand sides")
        return super().gemv(a, x, alpha=alpha, beta=beta, out=out)

    def tri_solve_(self, l, dinv_sb, sb, b):
        if l.dim() == 3 and l.shape[0] > 1 and l.stride(0) == 0:         # one factor for every member: one solve over all the columns
            B, n, r = b.shape
            wide = b.permute(1, 0, 2).reshape(n, B * r).clone()
            super().tri_solve_(l[0], dinv_sb, sb, wide)
            b.copy_(wide.reshape(n, B, r).permute(1, 0, 2))
            return b
        return super().tri_solve_(l, dinv_sb, sb, b)


def _vec(t):
    return 2 if t.dtype == torch.float64 else 4


class Defective(HostBackend):
    """``HostBackend`` with ONE defect, named by ``self.defect``; every method applies the defects that make sense for it."""

    def __init__(self, defect):
        self.defect = defect

    # -- reductions
    def rowreduce(self, z, w=None, *, want_dot=True, want_ss=False):
        d, n = self.defect, z.shape[1]
        keep = n
        if d == "last_k":
            keep = n - 1
        elif d == "vec_tail":
            keep = n // _vec(z) * _vec(z)
        if d == "pad_col" and z.shape[0] > 1 and z.stride(0) > n:
            z = torch.as_strided(z, (z.shape[0], n + 1), z.stride(), z.storage_offset())
            w = None if w is None else torch.cat([w.reshape(-1), torch.ones(1, dtype=w.dtype)])
        elif keep < n:
            z, w = z[:, :keep], (None if w is None else w.reshape(-1)[:keep])
        dot, ss = super().rowreduce(z, w, want_dot=want_dot, want_ss=want_ss)
        if d == "last_row":
            for o in (dot, ss):
                if o is not None:
                    o[-1] = 0
        return dot, ss

    def colreduce(self, v, w=None, *, want_dot=False, want_ss=True):
        d = self.defect
        if d == "last_row":
            v, w = v[..., :-1, :], (None if w is None else w[..., :-1])
        if d == "member0" and v.dim() == 3:
            v, w = v[:1].expand_as(v), (None if w is None else w[:1].expand_as(w))
        if d == "pad_col" and v.stride(-2) > v.shape[-1] and v.shape[-2] > 1:
            v = torch.as_strided(v, v.shape[:-1] + (v.shape[-1] + 1,), v.stride(), v.storage_offset())
            dot, ss = super().colreduce(v, w, want_dot=want_dot, want_ss=want_ss)
            # (the padding column lands in the last real one)
            return tuple(None if o is None else torch.cat([o[..., :-2], o[..., -2:-1] + o[..., -1:]], dim=-1) for o in (dot, ss))
        dot, ss = super().colreduce(v, w, want_dot=want_dot, want_ss=want_ss)
        if d == "last_col":
            for o in (dot, ss):
                if o is not None:
                    o[..., -1] = 0
        return dot, ss

    def gemv(self, a, x, *, alpha=1.0, beta=0.0, out=None):
        d, K, r = self.defect, a.shape[-1], x.shape[-1]
        keep = K
        if d == "last_k":
            keep = K - 1
        elif d == "vec_tail":
            keep = K // _vec(a) * _vec(a)
        elif d == "first_chunk":
            keep = min(K, R.gemv_chunk(r))
        if keep < K:
            a, x = a[..., :keep], x[..., :keep, :]
        if d == "pad_col" and a.stride(-2) > K and a.shape[-2] > 1:
            a = torch.as_strided(a, a.shape[:-1] + (K + 1,), a.stride(), a.storage_offset())
            x = torch.cat([x, torch.ones(x.shape[:-2] + (1, r), dtype=x.dtype)], dim=-2)
        if d == "member0" and a.dim() == 3:
            a, x = a[:1].expand_as(a), x[:1].expand_as(x)
        if d == "no_alpha":
            alpha = 1.0
        if d == "no_beta":
            beta = 0.0
        before = out.clone()
        if d == "reads_out" and beta == 0.0:
            res = alpha * (a @ x) + 0.0 * out
        else:
            res = alpha * (a @ x) + (beta * out if beta != 0.0 else 0.0)
        if d == "swap_rhs" and r > 1:
            res = torch.cat([res[..., 1:2], res[..., 0:1], res[..., 2:]], dim=-1)
        out.copy_(res)
        if d == "last_row":
            out[..., -1, :] = before[..., -1, :]
        if d == "last_col":
            out[..., -1] = before[..., -1]
        return out

    def logdet_chol(self, l):
        d = self.defect
        if d == "member0" and l.dim() == 3:
            l = l[:1].expand_as(l)
        if d == "last_k":
            l = l[..., :-1, :-1]
        return super().logdet_chol(l)

    # -- element-wise
    def tril_(self, a):
        d = self.defect
        before = a.clone()
        a.copy_(torch.tril(a, -1) if d == "diag_upper" else torch.tril(a))
        if d == "last_col":
            a[..., -1] = before[..., -1]
        if d == "pad_col" and a.stride(-2) > a.shape[-1]:
            torch.as_strided(a, a.shape, a.stride(), a.storage_offset() + 1)[..., -1] = 0
        return a

    def symmetrize_(self, a):
        d = self.defect
        before = a.clone()
        low = torch.tril(a, -1) if d == "diag_upper" else torch.tril(a)
        a.copy_(low + torch.tril(a, -1).transpose(-1, -2))
        if d == "last_col":
            a[..., -1] = before[..., -1]
        if d == "member0" and a.dim() == 3:
            a.copy_(a[:1].expand_as(a).clone())
        return a

    def sum_lower(self, parts, out):
        d = self.defect
        n = out.shape[0]
        il = torch.tril_indices(n, n, -1 if d == "diag_upper" else 0)
        if d == "last_row":
            il = il[:, il[0] < n - 1]
        if d == "last_col":
            il = il[:, il[1] < n - 1]
        if d == "last_k":
            parts = parts[:-1] if parts.shape[0] > 1 else parts * 0
        out[il[0], il[1]] = parts[:, il[0], il[1]].sum(0)
        if d == "pad_col" and out.stride(0) > n:
            torch.as_strided(out, out.shape, out.stride(), out.storage_offset() + 1)[:, -1] = 0
        return out

    def add_diag_(self, a, s=0.0, v=None):
        d = self.defect
        if d == "member0" and v is not None and v.dim() == 2:
            v = v[:1].expand_as(v)
        before = a.clone()
        super().add_diag_(a, s, v)
        if d == "last_row":
            a[..., -1, -1] = before[..., -1, -1]
        return a

    def scale_cols_(self, v, s):
        d = self.defect
        if d == "member0" and s.dim() == 2:
            s = s[:1].expand_as(s)
        before = v.clone()
        super().scale_cols_(v, s)
        if d == "last_row":
            v[..., -1, :] = before[..., -1, :]
        if d == "last_col":
            v[..., -1] = before[..., -1]
        return v

    def copy(self, src):
        d = self.defect
        out = super().copy(src)
        if d == "last_row":
            out[..., -1, :] = 0
        if d == "last_col":
            out[..., -1] = 0
        if d == "member0" and out.dim() == 3:
            out = out[:1].expand_as(out).clone()
        if d == "pad_col" and src.stride(-2) > src.shape[-1] and src.storage_offset() > 0:
            out = torch.as_strided(src, src.shape, src.stride(), src.storage_offset() - 1).clone()
        return out

    # -- solves
    def tri_solve_(self, l, dinv_sb, sb, b):
        d = self.defect
        before = b.clone()
        if d == "member0" and l.dim() == 3 and l.stride(0) != 0:
            l = l[:1].expand_as(l).clone()
        x = super().tri_solve_(l, dinv_sb, sb, b)
        n, r = b.shape[-2], b.shape[-1]
        if d == "last_block":
            r0 = (n - 1) // sb * sb
            x[..., r0:, :] = before[..., r0:, :]
        if d == "last_col":
            x[..., -1] = before[..., -1]
        if d == "swap_rhs" and r > 1:
            x.copy_(torch.cat([x[..., 1:2], x[..., 0:1], x[..., 2:]], dim=-1))
        if d == "pad_col" and b.stride(-2) > r and n > 1:
            torch.as_strided(b, b.shape, b.stride(), b.storage_offset() + 1)[..., -1] = 0
        return x

    def trtri(self, l, dinv_sb, sb):
        d = self.defect
        w = super().trtri(l, dinv_sb, sb)
        n = w.shape[-1]
        if d == "last_block":
            r0 = (n - 1) // sb * sb
            w[r0:] = torch.eye(n, dtype=w.dtype)[r0:]
        if d == "diag_upper":
            w = w + torch.triu(torch.full_like(w, 1e-30), 1)
        return w


#: defect -> what it is and the kernels for which at least one case has to fail
DEFECTS = {
    "last_row": ("drops the last row", ["rowreduce", "colreduce", "gemv", "add_diag", "scale_cols", "copy", "sum_lower"]),
    "last_col": ("drops the last column", ["colreduce", "gemv", "tril", "symmetrize", "scale_cols", "copy", "sum_lower", "tri_solve"]),
    "last_k": ("drops the last element of K", ["rowreduce", "gemv", "logdet", "sum_lower"]),
    "vec_tail": ("drops the part of a row past the last whole 16-byte vector", ["rowreduce", "gemv"]),
    "first_chunk": ("drops everything past the first staging chunk", ["gemv"]),
    "pad_col": ("reads (or writes) a padding column", ["rowreduce", "colreduce", "gemv", "tril", "sum_lower", "copy", "tri_solve"]),
    "no_alpha": ("ignores alpha", ["gemv"]),
    "no_beta": ("ignores beta", ["gemv"]),
    "reads_out": ("reads `out` when beta = 0", ["gemv"]),
    "swap_rhs": ("swaps two right-hand-side columns", ["gemv", "tri_solve"]),
    "member0": ("uses member 0 for every batch member", ["colreduce", "gemv", "logdet", "symmetrize", "add_diag", "scale_cols", "copy", "tri_solve"]),
    "diag_upper": ("treats the diagonal as strictly above", ["tril", "symmetrize", "sum_lower", "trtri"]),
    "last_block": ("leaves the last diagonal block of a solve unsolved", ["tri_solve", "trtri"]),
}

ALL = [(k, c, dt) for k in R.CASES for c, dt in R.all_cases(k)]


@pytest.mark.parametrize("kernel,case,dtype", ALL, ids=R.case_id)
def test_every_case_passes_over_the_host_backend(kernel, case, dtype):
    R.run(HostBackend(), case, dtype, "cpu")


@pytest.mark.parametrize("dtype", R.DTYPES)
def test_nine_right_hand_sides_are_refused(dtype):
    R.run_gemv_refuses_nine_columns(HostBackend(), dtype, "cpu")


@pytest.mark.parametrize("kernel,case,dtype", [p for p in ALL if p[0] in R.SUMMING], ids=R.case_id)
def test_detection_condition(kernel, case, dtype):
    """Every non-zero term of every output is at least four times the acceptance bound."""
    m = R.detection_margin(kernel, case, dtype)
    assert m >= 1.0, (case["id"], dtype, m)


def test_the_bounds_are_the_documented_ones():
    assert R.units("rowreduce", {"n": 4100}, "float32") == 65 + 4 + 6 + 2
    assert R.units("gemv", {"K": 1}, "float64") == 1 + 2 + 6 + 2 == 11            # the smallest bound of all
    assert R.colreduce_chunks(131073) == (256, 513) and R.colreduce_chunks(129) == (65, 2) and R.colreduce_chunks(128) == (128, 1)
    assert R.units("colreduce", {"rows": 131073}, "float32") == 256 + 513 + 2
    assert R.units("logdet", {"n": 8193, "batch": 1}, "float64") == 9 + 6 + 16 + 6
    assert R.units("logdet", {"n": 4096, "batch": 17}, "float32") == 16 + 6 + 4 + 6
    assert R.units("sum_lower", {"S": 7}, "float64") == 9
    assert float(np.finfo(np.longdouble).eps) < 2e-19, "the references need an extended-precision long double"


def _fails(be, case, dtype):
    try:
        R.RUNNERS[case["kernel"]](be, case, dtype, "cpu")
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("dtype", R.DTYPES)
@pytest.mark.parametrize("kernel", list(R.CASES))
def test_the_defective_backend_without_a_defect_passes(kernel, dtype):
    """What the defects are built on is itself correct: a case that fails below fails because of the defect."""
    be = Defective("none")
    for c in R.CASES[kernel](dtype):
        R.RUNNERS[kernel](be, c, dtype, "cpu")


@pytest.mark.parametrize("dtype", R.DTYPES)
@pytest.mark.parametrize("defect,kernel", [(d, k) for d, (_, ks) in DEFECTS.items() for k in ks])
def test_a_single_defect_is_caught(defect, kernel, dtype):
    be = Defective(defect)
    cases = sorted(R.CASES[kernel](dtype), key=lambda c: c.get("n", 0) * c.get("batch", 1) + c.get("K", 0) + c.get("rows", 0))
    assert any(_fails(be, c, dtype) for c in cases), f"no {kernel} case notices a backend that {DEFECTS[defect][0]}"


@pytest.mark.parametrize("dtype", R.DTYPES)
@pytest.mark.parametrize("kernel", list(R.CASES))
def test_case_tables_hold_every_edge(kernel, dtype):
    have = {e for c in R.CASES[kernel](dtype) for e in c["edges"]}
    want = R.REQUIRED_EDGES[kernel] + R.REQUIRED_EDGES.get(f"{kernel}/{dtype}", [])
    missing = [e for e in want if e not in have]
    assert not missing, missing
    ids = [c["id"] for c in R.CASES[kernel](dtype)]
    assert len(set(ids)) == len(ids)
