"""The launch geometry of the kernel-matrix and derivative kernels (``stheno_amd/csrc/gpk_kmat_plan.hpp``) on the host:
``stheno_amd/csrc/kmat_plan_check.cpp`` walks the plan and the decode of the compact 1-D grid over a few thousand shapes and fails on
a (row band, column chunk) pair that is missing, doubled or outside the matrix, and on a 2-D grid that does not cover every column
tile.  It also prints the plans of the shapes with which ``tests/test_diff_gpu.py`` reaches the walk over several column tiles and the
compact grid: were they different, those tests would pass without running the code they are there for.  Plain C++, no GPU."""
import os
import re
import shutil
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "stheno_amd", "csrc")

#: (ct, compact) of the shapes of test_diff_gpu.py: test_walk_of_several_column_tiles / test_compact_grid_with_two_tiles_per_workgroup
PLANS = {"walk f64": (8, 0), "walk f32": (8, 0), "compact f64": (2, 8), "compact f32": (2, 16)}


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs a host C++ compiler")
def test_plan_covers_the_matrix_and_the_compact_grid_decodes_to_the_lower_pairs(tmp_path):
    exe = tmp_path / "kmat_plan_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-o", str(exe), os.path.join(CSRC, "kmat_plan_check.cpp")], check=True, cwd=CSRC)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:]
    assert "shapes OK" in out.stdout
    plans = {m[0]: (int(m[1]), int(m[2])) for m in re.findall(r"^plan (.+): ct=(\d+) compact=(\d+) ", out.stdout, re.M)}
    assert plans == PLANS
