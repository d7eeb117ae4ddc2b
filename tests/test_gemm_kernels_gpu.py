"""The MFMA GEMM entry points of ``stheno_amd/csrc/gpk_gemm.hip``, called directly through ``HipBackend`` and checked element by element
on every launch path, in fp64 and fp32: ``gpk_gemm`` (64- and 128-tiles with and without bounds checks, the kernels for unaligned fp64,
the XCD-batched grid, the quarter-tile tail, ``lower_only``, the three triangular flags, ``gemm_trilo_pair_kernel``, in-place use with
and without the panel-solve bit), ``gpk_gemm_colscale`` (column scaling and per-slab column sums of squares at ragged M, N and K) and
``gpk_gemm_update2`` (the persistent kernel with one and two segments, looping workgroups and the quarter-tile tail).

Cases, references and acceptance are those of ``tests/gemm_reference.py``: rounded data against an 80-bit reference within
``(K_eff + 2) * eps * absum`` per element, grid data equal to one fp64 product, sentinels in every padding, untouched tiles above the
diagonal under ``lower_only``, every ``colss`` slab row written.  ``tests/test_gemm_reference_host.py`` shows on the CPU that a correct
implementation passes every case, that a list of single defects does not, and which launcher branch every case reaches.  The worst
ratios measured on an MI355X are in ``profiles/README.md`` ("GEMM kernels, element by element"); they are for the record and set no
bound."""
import pytest

from . import gemm_reference as R

pytestmark = pytest.mark.gpu


def _params(entry):
    return pytest.mark.parametrize("case,dtype", R.all_cases(entry), ids=R.case_id)


@pytest.fixture(autouse=True, scope="module")
def _references_are_dropped_afterwards():
    yield
    R.drop_cache()


@_params("gemm")
def test_gemm(hip_backend, case, dtype):
    R.run(hip_backend, case, dtype, "cuda")


@_params("colscale")
def test_gemm_colscale(hip_backend, case, dtype):
    R.run(hip_backend, case, dtype, "cuda")


@_params("update2")
def test_gemm_update2(hip_backend, case, dtype):
    R.run(hip_backend, case, dtype, "cuda")


@pytest.mark.parametrize("dtype", R.DTYPES)
def test_gemm_refusals(hip_backend, dtype):
    R.run_gemm_refusals(hip_backend, dtype, "cuda")


@pytest.mark.parametrize("dtype", R.DTYPES)
def test_gemm_colscale_refusals(hip_backend, dtype):
    R.run_colscale_refusals(hip_backend, dtype, "cuda")


@pytest.mark.parametrize("dtype", R.DTYPES)
def test_gemm_update2_refusals(hip_backend, dtype):
    R.run_update2_refusals(hip_backend, dtype, "cuda")
