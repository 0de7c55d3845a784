"""The host's float64 forms of the whole-arm avoidance command against the 50-digit form of tests/hp_avoid.py, without a GPU: that the
bar of tests/test_gpu_link_avoid.py -- K_MARGIN units beyond the output's half ulp -- is attainable in float64, by the law as written
(host_avoid) and by the kernel's one-pass algebra (walk_avoid); and the Jacobian-transpose algebra itself against central differences of
the sphere positions."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hp_avoid as ha  # noqa: E402
import hp_links as hl  # noqa: E402


def _hold(got, ref, io_dtype, what):
    """got (unrounded float64) within K_MARGIN units of the reference; exactly zero where the unit is 0"""
    err, lim = ha.error(got, ref), ha.K_MARGIN * ref["unit"]
    assert np.all(got[ref["unit"] == 0] == 0), what
    assert np.all(err <= lim), (what, float((err / np.where(lim > 0, lim, 1.0)).max()))


@pytest.mark.parametrize("robot", hl.ROBOTS)
@pytest.mark.parametrize("io_dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_host_forms_within_the_bar(robot, io_dtype):
    for case in ha.CASES:
        c, ref, host = ha.host_case(robot, io_dtype, case)
        walk = ha.walk_avoid(c["chain"], c["spheres"], c["q"], c["pts"], **ha.call_args(c))
        B = c["q"].shape[0]
        assert 3 * ref["active"].sum() >= B and (B == 1 or not ref["active"].all())     # the case is not vacuous in 50 digits either
        moves = any(link > 0 for link, _c, _r in c["spheres"])      # (the list `one` holds a sphere on link 0: pushed, it moves no joint)
        assert np.all(ref["hi"][~ref["active"]] == 0) and np.any(ref["hi"][ref["active"]] != 0) == moves
        print("%-10s %-7s %-30s d0 = %.4f  %3d of %3d arms active; host %.3f, one-pass %.3f units" % (
            robot, np.dtype(io_dtype).name, case, c["d0"], ref["active"].sum(), B,
            ha.worst_units(host, ref, np.float64), ha.worst_units(walk, ref, np.float64)))
        _hold(host, ref, io_dtype, (case, "host"))
        _hold(walk, ref, io_dtype, (case, "one-pass"))


@pytest.mark.parametrize("io_dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_edges(io_dtype):
    c = ha.edge_case(io_dtype)
    ref = ha.avoid(c["chain"], c["spheres"], c["q"], c["pts"], **ha.call_args(c))
    arm = ha.EDGE_ARMS.index
    for form in (ha.host_avoid, ha.walk_avoid):
        got = form(c["chain"], c["spheres"], c["q"], c["pts"], **ha.call_args(c))
        assert np.isfinite(got).all()
        _hold(got, ref, io_dtype, form.__name__)
        for name in ("nan_q", "scale_zero", "no_rows"):
            assert np.all(got[arm(name)] == 0), name
    for name in ("at_d0", "penetrating", "coincident", "prismatic_tail", "general"):
        assert np.any(ref["hi"][arm(name)] != 0), name
    # the pair at d0 adds nothing: with sphere 1 alone (the other spheres meet that row too), the command is the same without the row
    only1 = dict(c, mask=np.array([0, 7, 0], dtype=np.uint32))
    without = dict(only1, pts=c["pts"].copy())
    without["pts"][arm("at_d0"), 0] = np.nan
    ref1 = ha.avoid(c["chain"], c["spheres"], c["q"], c["pts"], **ha.call_args(only1))
    ref2 = ha.avoid(c["chain"], c["spheres"], c["q"], without["pts"], **ha.call_args(only1))
    assert np.any(ref1["hi"][arm("at_d0")] != 0)
    assert np.array_equal(ref1["hi"][arm("at_d0")], ref2["hi"][arm("at_d0")]) and np.array_equal(ref1["lo"][arm("at_d0")], ref2["lo"][arm("at_d0")])
    # the sphere behind the all-prismatic tail pushes the two prismatic joints, and no sphere on link 0 pushes anything
    assert np.all(ref["hi"][arm("prismatic_tail"), 4:] != 0)
    only0 = dict(c, mask=np.array([7, 0, 0], dtype=np.uint32))
    assert np.all(ha.avoid(c["chain"], c["spheres"], c["q"], c["pts"], **ha.call_args(only0))["hi"] == 0)


@pytest.mark.parametrize("robot", hl.ROBOTS)
def test_jacobian_transpose_against_central_differences(robot):
    """tau_k = sum_i F_i . dP_i / dq_k: the sphere positions of hp_links.host_points at q +- h e_k, the forces held fixed"""
    case = ha.CASES[0]
    c, _ref, _host = ha.host_case(robot, np.float64, case)
    tau, p = ha.host_avoid(c["chain"], c["spheres"], c["q"], c["pts"], detail=True, **ha.call_args(c))
    h = 1e-6
    fd = np.zeros_like(tau)
    for k in range(c["chain"].n):
        e = np.zeros(c["chain"].n)
        e[k] = h
        dP = (hl.host_points(c["chain"], c["spheres"], p["q"] + e)[:, :, :3] - hl.host_points(c["chain"], c["spheres"], p["q"] - e)[:, :, :3]) / (2 * h)
        fd[:, k] = (p["F"] * dP).sum(axis=(1, 2))
    fd[~p["on"].any(axis=(1, 2))] = 0.0
    assert np.any(tau != 0)
    assert np.abs(tau - fd).max() <= 1e-6 * max(1.0, np.abs(tau).max()), np.abs(tau - fd).max()
    walk = ha.walk_avoid(c["chain"], c["spheres"], c["q"], c["pts"], **ha.call_args(c))
    assert np.abs(walk - fd).max() <= 1e-6 * max(1.0, np.abs(tau).max())
