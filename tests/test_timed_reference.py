"""tests/timed_reference.py held to tests/golden/timed_reference.npz: the numbers the five helper modules it replaced gave on the small
cases of the host tests (tests/golden/make_timed_reference.py names the commit and rebuilds the inputs).  Integer outputs exactly -- the
generator refuses a case with a decision near its threshold --, float rows to the tolerance the GPU is held to on the same rows: 1e-8,
float32 I/O 2e-6, so that another machine's libm cannot fail the test while a changed loop still does."""
import importlib.util
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
TOL = {"float64": 1e-8, "float32": 2e-6}


def _generator(golden_dir):
    spec = importlib.util.spec_from_file_location("make_timed_reference", os.path.join(golden_dir, "make_timed_reference.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def fixture(golden_dir):
    gen = _generator(golden_dir)
    with np.load(gen.FIXTURE) as z:
        return gen, {k: z[k] for k in z.files}


@pytest.mark.parametrize("io", ["float64", "float32"])
@pytest.mark.parametrize("name", ["goto", "goto_stall", "follow", "goto_js", "follow_js", "script"])
def test_numbers_are_the_replaced_modules(oracle_c, fixture, name, io):
    import timed_reference as tr
    gen, gold = fixture
    assert gen.REV in str(gold["readme"]) and set(gen.CASES) == {k.split("/")[0] for k in gold if "/" in k}
    r = gen.CASES[name](tr, oracle_c, np.dtype(io))
    keys = [k.split("/")[2] for k in gold if k.startswith("%s/%s/" % (name, io))]
    joint = name in gen.JOINT_SPACE          # a joint-space move reports no distances
    assert set(keys) == {k for k in gen.INTS + gen.FLOATS if k in r} - ({"dist_traj"} if joint else set())
    assert {"next", "pending", "q_traj", "diff"} <= set(keys) and ("dist_traj" in keys) == (not joint)
    assert ("stalled" in keys) == (name == "goto_stall") and ("arrived" in keys) == name.startswith("goto")
    for k in keys:
        want, got = gold["%s/%s/%s" % (name, io, k)], r[k]
        assert got.shape == want.shape, k
        if k in gen.INTS:
            assert got.dtype == np.int32 and np.array_equal(got, want), (k, got, want)
        else:
            assert np.array_equal(np.isnan(got), np.isnan(want)), k
            err = np.nanmax(np.abs(got - want.astype(np.float64)), initial=0.0)
            assert err < TOL[io], (k, err)
