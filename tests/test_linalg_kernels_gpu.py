"""The kernels that consume the Cholesky factor, called directly through ``HipBackend`` and checked element by element at the edges of
their launch geometry, in fp64 and fp32: ``gpk_rowreduce``, ``gpk_colreduce``, ``gpk_logdet_chol``, ``gpk_sum_lower``, ``gpk_tril``,
``gpk_symmetrize``, ``gpk_add_diag``, ``gpk_scale_cols``, ``gpk_copy2d`` (``stheno_amd/csrc/gpk_reduce.hip``) and ``gpk_gemv``, the three
paths of ``tri_solve_`` (the GEMV sweep, one workgroup per matrix, the blocked out-of-place solve) and ``gpk_trtri_lower``
(``gpk_solve.hip``).

Cases, references and acceptance are those of ``tests/linalg_reference.py``: the summing kernels against an 80-bit reference within
``(depth + 2) * eps * absum`` per element, an a-priori bound from each kernel's summation order; the element-wise kernels bit for bit
against NumPy, with sentinels in every padding; the solves per column within ``1000 * eps * max|ref|`` against SciPy in fp64 on the
rounded factor.  ``tests/test_linalg_reference_host.py`` shows on the CPU that a correct implementation passes every case and that a
lost row, column, tail, chunk, right-hand side or batch member does not.  The worst ratios measured on an MI355X are in
``profiles/README.md`` ("Solve, GEMV and reduction kernels, element by element"); they are for the record and set no bound."""
import pytest

from . import linalg_reference as R

pytestmark = pytest.mark.gpu


def _params(kernel):
    return pytest.mark.parametrize("case,dtype", R.all_cases(kernel), ids=R.case_id)


@_params("rowreduce")
def test_rowreduce(hip_backend, case, dtype):
    R.run(hip_backend, case, dtype, "cuda")


@_params("colreduce")
def test_colreduce(hip_backend, case, dtype):
    R.run(hip_backend, case, dtype, "cuda")


@_params("gemv")
def test_gemv(hip_backend, case, dtype):
    R.run(hip_backend, case, dtype, "cuda")


@pytest.mark.parametrize("dtype", R.DTYPES)
def test_gemv_refuses_nine_right_hand_sides(hip_backend, dtype):
    R.run_gemv_refuses_nine_columns(hip_backend, dtype, "cuda")


@_params("logdet")
def test_logdet_chol(hip_backend, case, dtype):
    R.run(hip_backend, case, dtype, "cuda")


@_params("tril")
def test_tril(hip_backend, case, dtype):
    R.run(hip_backend, case, dtype, "cuda")


@_params("symmetrize")
def test_symmetrize(hip_backend, case, dtype):
    R.run(hip_backend, case, dtype, "cuda")


@_params("add_diag")
def test_add_diag(hip_backend, case, dtype):
    R.run(hip_backend, case, dtype, "cuda")


@_params("scale_cols")
def test_scale_cols(hip_backend, case, dtype):
    R.run(hip_backend, case, dtype, "cuda")


@_params("copy")
def test_copy(hip_backend, case, dtype):
    R.run(hip_backend, case, dtype, "cuda")


@_params("sum_lower")
def test_sum_lower(hip_backend, case, dtype):
    R.run(hip_backend, case, dtype, "cuda")


@_params("tri_solve")
def test_tri_solve(hip_backend, case, dtype):
    R.run(hip_backend, case, dtype, "cuda")


@_params("trtri")
def test_trtri(hip_backend, case, dtype):
    R.run(hip_backend, case, dtype, "cuda")
