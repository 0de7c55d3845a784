"""The C oracle against the high-precision reference (tests/hp_reference.py) as the solve's conditioning worsens.

Every other test runs the damped-least-squares solve at lambda = 0.1 on poses drawn from 0.8 of the joint range, where the normal matrix
A = Jw Jw^T + lambda^2 I has a condition number of a few hundred.  Here lambda goes down to 1e-3 (and to 0 on regular poses) with arms on
and next to the shoulder, elbow and wrist singularities, the zero pose and the nodes of the kernels' sin / cos table: cond reaches 4e6, and
an error of the factorisation that stays under 1e-9 at the default is amplified ten thousand times.  A fixed bar against the oracle cannot
be used there -- plain double arithmetic is itself off by 1e-8 rad/s and more -- so the oracle is held to the reference first, with a bar
that scales with the conditioning, and the GPU tests (tests/test_gpu_conditioning.py) hold the kernels to the same reference.

Bars.  pose: 1e-14 (a product of up to 15 frames of entries <= 1.2 in double: a few u).  qdot_vf, per arm:
    err_b <= 8 cond_b u max_i |qdot_b,i|,  u = 2^-53,
the forward error bound of a backward stable solve with a modest constant (the textbook bound carries a factor of the dimension, 6).

Measured on these cases (B = 192 per case, this file's own print, 64 cases with the two I/O types): the oracle's worst ratio
err / (cond u |qdot|) is 4.79 (lwr_wide, float64, lambda 0.1, the sweep's weights, an arm of cond 18) and 4.14 (lwr, float64, lambda 1e-2,
the sweep's weights); with unit weights it stays below 1.5.  48 of the 64 cases are below 1.  The worst pose error is 7.1e-16.  The largest
cond at lambda = 1e-3: powercube6 3.5e6, lwr 4.0e6, lwr_dual14 1.4e7 with unit weights; 5.7e5, 8.6e5, 3.8e6 with the sweep's weights
(wy's smallest entry is 0.1: sigma_1 falls).  The reference's own residual |A y - Wy tw| / |Wy tw| stays below 2.1e-44."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hp_reference as hp  # noqa: E402

IO = [np.float32, np.float64]
POSE_BAR = 1e-14
K_ORACLE = 8.0


@pytest.mark.parametrize("io_dtype", IO, ids=["f32", "f64"])
@pytest.mark.parametrize("case", hp.cases(), ids=hp.case_id)
def test_oracle_against_the_reference(oracle_c, case, io_dtype):
    robot, lam, wname, poses = case
    chain, params, w, kinds, eps, orc, ref, R = hp.oracle_case(oracle_c, robot, io_dtype, lam, wname, poses)
    assert params.flags == 0 and np.all(orc["status"] == 0)
    assert np.array_equal(orc["qdot_out"], orc["qdot_vf"])
    rat, err = hp.ratio(orc["qdot_vf"], ref)
    perr = hp.error(orc["pose"], ref, "pose").max()
    b = int(np.argmax(rat))
    print("%-11s %s lambda %-6g %-8s %-7s oracle ratio %.3f (arm %d kind %d eps %g, err %.2e, cond %.2e), max cond %.3e, pose err %.2e, residual %.1e"
          % (robot, np.dtype(io_dtype).name, lam, wname, poses, R, b, kinds[b], eps[b], err[b], ref["cond"][b], ref["cond"].max(), perr,
             ref["resid"].max()))
    assert ref["resid"].max() < hp.RESIDUAL_BAR      # the reference solves its own system
    assert np.all(np.isfinite(orc["qdot_vf"])) and np.abs(ref["qdot"]).max() > 0.1
    assert perr < POSE_BAR
    assert np.all(rat <= K_ORACLE), (R, b, kinds[b], eps[b])


@pytest.mark.parametrize("io_dtype", IO, ids=["f32", "f64"])
def test_the_sweep_reaches_the_conditioning_it_claims(oracle_c, io_dtype):
    """From the reference alone: at lambda = 1e-3 the largest cond is above 1e6 with unit weights (powercube6, lwr, lwr_dual14), above 1e5
    with the sweep's weights (1e6 for lwr_dual14); at the default lambda = 0.1 it stays where the rest of the suite works."""
    for robot in ("powercube6", "lwr", "lwr_dual14"):
        for wname, floor in (("unit", 1e6), ("weighted", 1e6 if robot == "lwr_dual14" else 1e5)):
            ref = hp.oracle_case(oracle_c, robot, io_dtype, 1e-3, wname, "mixed")[6]
            assert ref["cond"].max() > floor, (robot, wname, ref["cond"].max())
        ref = hp.oracle_case(oracle_c, robot, io_dtype, 0.1, "unit", "mixed")[6]
        assert ref["cond"].max() < 2e3, (robot, ref["cond"].max())


def test_every_wave_and_every_group_of_eight_mixes_the_kinds():
    kinds, ie = hp.pattern()
    assert len(kinds) == hp.B_ARMS == 192
    for g in kinds.reshape(-1, 8):
        assert set(g) == set(range(hp.N_KINDS))
    for wv, we in zip(kinds.reshape(-1, 64), ie.reshape(-1, 64)):
        assert {(k, e) for k, e in zip(wv, we)} == {(k, e) for k in range(hp.N_KINDS) for e in range(len(hp.EPS))}


@pytest.mark.parametrize("io_dtype", IO, ids=["f32", "f64"])
def test_the_poses_are_what_their_kind_says(io_dtype):
    for robot in ("powercube6", "lwr", "lwr_dual14"):
        chain, w, kinds, eps = hp.make_case(robot, io_dtype)
        q, n = w["q"], chain.n
        assert np.array_equal(q, q.astype(io_dtype).astype(np.float64))
        assert np.all(q > chain.q_lo) and np.all(q < chain.q_hi)
        e = eps.astype(io_dtype).astype(np.float64)[:, None]
        for k, cols in ((0, np.arange(1, n, 2)), (1, [3]), (2, [n - 2]), (3, np.arange(n))):
            m = kinds == k
            assert np.array_equal(np.abs(q[m][:, cols]), np.broadcast_to(e[m], q[m][:, cols].shape))
        m = kinds == 4
        t = q[m] * (32 / np.pi) - 0.5 * (np.arange(len(q))[m] % 2)[:, None]
        inner = np.abs(q[m]) < 0.94 * chain.q_hi     # (not clipped)
        assert inner.mean() > 0.8 and np.abs(t - np.rint(t))[inner].max() < (1e-5 if io_dtype == np.float32 else 1e-13)
    chain, w, kinds, _ = hp.make_case("lwr_wide", io_dtype, "regular")
    assert np.all(kinds == 5) and np.abs(w["q"]).max() > 45.0 and w["q"].min() < -45.0   # up to eight turns, both signs
