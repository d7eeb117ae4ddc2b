"""The admission layer (``stheno_amd/learnable.py``) in front of the autograd functions issues the backend calls it issued before it
was gathered into one module: every scenario of ``scripts/dump_learnable.py`` is replayed on the test-only host backends under the
script's recording wrapper and its trace -- the backend methods in order, the shapes of their tensor arguments, the optional arguments
given, the exception type of a refusal -- is held, entry by entry, against ``tests/golden/learnable_backend_trace.json``, which was
recorded with the same script from the commit before the move.  The entries of the scenarios added since (``LATER_SCENARIOS``:
function-scaled and per-batch log-densities, batched posteriors, the joint covariance) were recorded from the commit before the autograd
functions came to share their stages, and do not list an optional argument given at its default; the older entries are as they were.
A difference means the host code changed what runs: the code is wrong, not the fixture.  No GPU."""
import importlib.util
import json
import os

import pytest

from .conftest import ROOT


def _load_script():
    spec = importlib.util.spec_from_file_location("dump_learnable", os.path.join(ROOT, "scripts", "dump_learnable.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


DUMP = _load_script()
with open(os.path.join(ROOT, "tests", "golden", "learnable_backend_trace.json")) as fh:
    GOLDEN = json.load(fh)
ALL = DUMP.SCENARIOS + DUMP.LATER_SCENARIOS


def test_the_fixture_holds_the_scenarios_of_the_script():
    assert sorted(GOLDEN) == sorted(name for name, _, _ in ALL)


@pytest.mark.parametrize("name,host,fn", ALL, ids=[name for name, _, _ in ALL])
def test_backend_trace_is_the_recorded_one(name, host, fn):
    trace, _ = DUMP.run_scenario(name, host, fn)
    want = GOLDEN[name]
    assert trace["raises"] == want["raises"]
    for i, (got, ref) in enumerate(zip(trace["calls"], want["calls"])):
        assert got == ref, f"call {i} of {name}"
    assert len(trace["calls"]) == len(want["calls"])
