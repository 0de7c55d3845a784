"""The C oracle's nullspace module against the high-precision reference (tests/hp_nullspace.py) as J loses rank.

Every other test of qdot_null compares a kernel with this oracle at 1e-9 / 1e-6 on poses drawn from 0.8 of the joint range, where
sigma_1 / sigma_6 of J is a few tens.  Here the arms sit on and next to the shoulder, elbow and wrist singularities and the zero pose
(hp_reference's mixed poses; the kind-4 arms moved off the singular nodes of the sin / cos table, hp_nullspace.make_case), and the oracle
-- a one-sided Jacobi SVD with pinv's rcond of 1e-15, then an eigen-decomposition with the reference's 1e-8 threshold; for chains of 8 and
more joints the stated row rule of VFIK_PROJ_ROW_MIN -- is held to a 50-digit restatement: restrict (through Pz), the null vector,
qdot_null of a whole cycle and the status, at both I/O roundings of q.

Bar per arm outside the zone: max(S, 8 u (sigma_1 / sigma_6) scale) (hp_nullspace.bar), times null_gain for qdot_null; scale = 1 for v,
max|z| for Pz, their sum for a cycle with both.  The zone, the ambiguous sets and the caps on them are hp_nullspace's, computed from the
reference alone and asserted before the oracle's numbers are looked at.

Measured (this file's print; the oracle's worst ratio R = err / (u sigma_1 / sigma_6 scale) per case, float32 / float64 rounding of q):
    powercube6   restrict Pz 0.22 / 0.26                            cycle `Pz` and `both` 0.22 / 0.26 (`v`: nothing to move along)
    lwr          restrict Pz 0.47 / 0.44   null vector 0.39 / 0.37  cycle `v` 0.39 / 0.37   `Pz` 0.46 / 0.44   `both` 0.39 / 0.31
    lwr_dual14   restrict Pz 1.41 / 1.38 (the row rule)             cycle `Pz` and `both` 1.30 / 1.23
    sequence A   0.39, 0.39, 0.49, 0.60 / 0.37, 0.37, 0.33, 0.35 at its four steps
Zone: powercube6 19 of 192 arms (kind 2 at eps 0 and 1e-9, kind 3 at eps 0), lwr 55 (kinds 0, 1, 3 at eps 0 and 1e-9, kind 0 at eps 1e-6;
arm 7, the stretched elbow moved to 3e-8 rad, is held at sigma_6 / sigma_1 = 3.8e-10), lwr_dual14 5 (kind 3 at eps 1e-3: a pivot within a
factor of 4 of the rule's threshold).  Sign-ambiguous: lwr 9, none elsewhere; stop-ambiguous: none.  Stops: lwr 8 of the 16 regular arms put
0.02 rad from a limit of the chain (sets `v` and `both`); under narrow per-arm limits lwr 14, lwr_dual14 21, smallest margin 3.3e-3.
The oracle's null vector has |J v| / sigma_1 <= 4.8 u.  The reference's residuals: solve below 1e-41, |J v| / sigma_1 below 3e-45."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hp_nullspace as hn  # noqa: E402
import hp_reference as hp  # noqa: E402

IO = [np.float32, np.float64]
K_ORACLE = 8.0
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _jac(oc, chain, q):
    return np.array([oc.jacobian(chain, row)[0] for row in q])


def _check(err, ref, io_dtype, scale, held, what, kinds, eps):
    barv = hn.bar(ref, io_dtype, K_ORACLE, scale)
    rat = np.where(held, err / (hp.U / np.maximum(ref["gap"], 1e-300) * np.maximum(scale, 1e-300)), 0.0)
    b = int(np.argmax(rat))
    print("    %-22s R %7.3f (arm %3d kind %d eps %-5g gap %.2e, err %.2e)  worst err / bar %.3f"
          % (what, rat[b], b, kinds[b], eps[b], ref["gap"][b], err[b], np.where(held, err / barv, 0.0).max()))
    bad = held & ~(err <= barv)
    assert not bad.any(), "%s: arms %s over the bar (kinds %s, eps %s, gaps %s, err %s)" % (
        what, np.nonzero(bad)[0][:8], kinds[bad][:8], eps[bad][:8], ref["gap"][bad][:8], err[bad][:8])
    return float(rat.max())


def test_the_rule_constant_is_the_header_s():
    with open(os.path.join(ROOT, "include", "vfik_types.h")) as f:
        m = re.search(r"#define\s+VFIK_PROJ_ROW_MIN\s+(\S+)", f.read())
    assert m and float(m.group(1)) == hn.PROJ_ROW_MIN


@pytest.mark.parametrize("io_dtype", IO, ids=["f32", "f64"])
@pytest.mark.parametrize("robot", hn.NS_ROBOTS)
def test_restrict_and_the_null_vector_against_the_reference(oracle_c, robot, io_dtype):
    oc = oracle_c
    case = hn.oracle_case(oc, robot, io_dtype, "both")
    chain, ref, cyc, kinds, eps, w = case["chain"], case["ref"], case["cyc"], case["kinds"], case["eps"], case["w"]
    n = chain.n
    hn.assert_caps(ref, cyc, kinds, robot)
    held = ~ref["zone"]
    print("\n%s %s: zone %d of %d %s, sign-ambiguous %d, stop-ambiguous %d; residuals: solve %.1e, |J v| / sigma_1 %.1e"
          % (robot, np.dtype(io_dtype).name, (~held).sum(), len(held), sorted(set(zip(kinds[~held].tolist(), eps[~held].tolist()))),
             (cyc["sign_amb"] & held).sum(), (cyc["stop_amb"] & held).sum(), ref["resid"][held].max(), ref["vres"][held].max()))
    assert ref["resid"][held].max() < hp.RESIDUAL_BAR and ref["vres"][held].max() < hp.RESIDUAL_BAR
    J = _jac(oc, chain, w["q"])
    proj = oc.restrict_rows if n >= 8 else oc.restrict
    Pz = np.array([proj(J[b]) @ ref["z"][b] for b in range(len(J))])
    zmax = np.abs(ref["z"]).max(axis=1)
    assert zmax.max() > 0.1
    _check(hn.error(Pz, ref, "Pz").max(axis=1), ref, io_dtype, zmax, held, "restrict Pz", kinds, eps)
    if n == 6:   # no nullspace: the projection of anything is zero within the bar (asserted above against the reference's 1e-40)
        assert np.abs(ref["Pz"][held]).max() < 1e-30
    if n == 7:
        v = np.zeros((len(J), n))
        for b in np.nonzero(held)[0]:
            basis = oc.NullspaceC(n).basis(J[b])
            assert len(basis) == 1, (b, kinds[b], eps[b], len(basis))
            v[b] = basis[0]
        err = hn.error(v, ref, "v").max(axis=1)
        flip = np.abs(v + ref["v"] + ref["v_lo"]).max(axis=1)
        amb = hn.raw_sign_ambiguous(ref)
        err = np.where(amb, np.minimum(err, flip), err)
        _check(err, ref, io_dtype, np.ones(len(J)), held, "null vector", kinds, eps)


@pytest.mark.parametrize("io_dtype", IO, ids=["f32", "f64"])
@pytest.mark.parametrize("pset", hn.PSETS)
@pytest.mark.parametrize("robot", hn.NS_ROBOTS)
def test_a_cycle_s_qdot_null_and_status_against_the_reference(oracle_c, robot, pset, io_dtype):
    case = hn.oracle_case(oracle_c, robot, io_dtype, pset)
    chain, ref, cyc, kinds, eps, orc, params = (case[k] for k in ("chain", "ref", "cyc", "kinds", "eps", "orc", "params"))
    hn.assert_caps(ref, cyc, kinds, "%s %s" % (robot, pset))
    print("\n%s %s %s: oracle R %.3f (arm %d kind %d eps %g)" % (robot, np.dtype(io_dtype).name, pset, case["R"], case["R_arm"],
                                                                 kinds[case["R_arm"]], eps[case["R_arm"]]))
    failures = []
    allowed = hn.ST_LIMIT_STOP | hn.ST_NULL_AMBIGUOUS
    hn.check_zone(orc["qdot_null"], orc["status"], ref, case["ctrl"][:, 0], case["jl"], params.null_gain, allowed, "oracle", failures)
    hn.check_null(orc["qdot_null"], orc["status"], ref, cyc, np.float64, K_ORACLE, case["scale"], params.null_gain,
                  hn.expected_status(chain.n), "oracle qdot_null", kinds, eps, failures)
    if pset != "Pz" and chain.n == 7:
        # the stop decision is exercised both ways: regular arms sit NEAR_LIMIT from a limit of the chain, and c0 v decides
        hn.assert_stops(ref, cyc, "%s %s" % (robot, pset), 4)
        # the null vector's own residual, which sees what the bar of qdot_null cannot (hp_nullspace.check_residual)
        res = hn.check_residual(orc["qdot_null"], orc["status"], case["ctrl"][:, 0], params.null_gain, (robot, np.dtype(io_dtype).name, hn.POSES),
                                chain, case["w"]["q"], ref, cyc, np.float64, K_ORACLE, "oracle", kinds, eps, failures) if pset == "v" else 0.0
        assert res <= K_ORACLE
    # the mixer: qdot_out = 1 qdot_vf + 0.7 qdot_null, unfused, in the oracle's own doubles
    assert np.array_equal(orc["qdot_out"], orc["qdot_vf"] * hn.MIX_W[0] + orc["qdot_null"] * hn.MIX_W[1])
    assert not failures, "\n".join(failures)


def test_every_wave_and_every_group_of_eight_mixes_the_kinds():
    kinds, ie = hp.pattern()
    for g in kinds.reshape(-1, 8):
        assert set(g) == set(range(hp.N_KINDS))
    for wv, we in zip(kinds.reshape(-1, 64), ie.reshape(-1, 64)):
        assert {(k, e) for k, e in zip(wv, we)} == {(k, e) for k in range(hp.N_KINDS) for e in range(len(hp.EPS))}
    # ... and c0 takes both signs in every group of eight of the sets that use it
    ctrl, _ = hn.pset_inputs("v", hp.B_ARMS)
    assert set(np.unique(ctrl[:, 0])) == {-1.0, 1.0}
    assert all(len(set(g)) == 2 for g in ctrl[:, 0].reshape(-1, 8))


@pytest.mark.parametrize("io_dtype", IO, ids=["f32", "f64"])
def test_the_kind_4_arms_stay_on_the_table_and_off_the_singularities(io_dtype):
    for robot in hn.NS_ROBOTS:
        chain, w, kinds, _ = hn.make_case(robot, io_dtype)
        m = kinds == 4
        q = w["q"]
        assert np.all(q > chain.q_lo) and np.all(q < chain.q_hi)
        t = q[m] * (32 / np.pi) - 0.5 * (np.arange(len(q))[m] % 2)[:, None]
        inner = np.abs(q[m]) < 0.94 * chain.q_hi
        assert inner.mean() > 0.8 and np.abs(t - np.rint(t))[inner].max() < (1e-5 if io_dtype == np.float32 else 1e-13)
        assert min(hn._gap_of(chain, row) for row in q[m]) >= hn.NODE_GAP


@pytest.mark.parametrize("io_dtype", IO, ids=["f32", "f64"])
def test_sequence_a_builds_its_branches_and_the_oracle_follows_it(oracle_c, io_dtype):
    """Cycle sequence A (hp_nullspace.sequence_a): every wave and every group of eight arms holds lanes BUILT for the step's branch of
    the warm path (the condition cleared by a factor of 4, recomputed from the reference vectors) next to lanes that are not; the zone's caps hold
    at every step, and a cap on the lanes held up to sign that were never in the zone; and the oracle, with its own double state, is within its bar at every step."""
    seq = hn.sequence_a(io_dtype)
    kinds, eps = seq["kinds"], seq["eps"]
    outs, Rs = hn.sequence_oracle(oracle_c, seq)
    for k in range(4):
        ref, cyc = seq["refs"][k], seq["cycs"][k]
        assert ref["zone"].sum() * 3 <= len(kinds) and not np.any(ref["zone"] & (kinds >= 4))
        clean = ~np.any([seq["refs"][i]["zone"] for i in range(k + 1)], axis=0)       # never in the zone so far
        # of those, held up to sign only: 5 % as everywhere while the pose stands still; after a turn or a jump the lanes whose warm / cold
        # decision is not cleared by the factor of 4 join them, and at most one lane in six may be such
        cap = len(kinds) // 20 if k < 2 else len(kinds) // 6
        assert (cyc["sign_amb"] & clean).sum() <= cap, (hn.SEQ_STEPS[k], (cyc["sign_amb"] & clean).sum())
        if k:
            b = seq["built"][k]
            print("%s: %d lanes built (keep %.3f .. %.3f, rho %.2e .. %.2e), %d held up to sign, oracle R %.3f"
                  % (hn.SEQ_STEPS[k], b.sum(), np.nanmin(seq["keep"][k][b]), np.nanmax(seq["keep"][k][b]), np.nanmin(seq["rho"][k][b]),
                     np.nanmax(seq["rho"][k][b]), (cyc["sign_amb"] & ~ref["zone"]).sum(), Rs[k]))
            assert all(grp.any() for grp in b.reshape(-1, 8)), hn.SEQ_STEPS[k]           # a built lane in every group of eight ...
            assert all(not wv.all() for wv in b.reshape(-1, 64)), hn.SEQ_STEPS[k]         # ... beside lanes of another kind in every wave
        failures = []
        hn.check_null(outs[k]["qdot_null"], outs[k]["status"], ref, cyc, np.float64, K_ORACLE, 1.0, seq["params"].null_gain, 0,
                      "oracle " + hn.SEQ_STEPS[k], kinds, eps, failures)
        assert not failures, "\n".join(failures)


@pytest.mark.parametrize("io_dtype", IO, ids=["f32", "f64"])
@pytest.mark.parametrize("robot", hn.NS_ROBOTS)
def test_narrow_per_arm_limits_make_arms_stop(oracle_c, robot, io_dtype):
    """Set `both` under hp_nullspace.narrow_limits: on the chains that have a nullspace, arms outside the zone clearly stop and others
    with limits of the same kind clearly do not (asserted on the reference), and the oracle takes the reference's decision on each.
    (powercube6 has no nullspace: outside the zone its qn is zero and it never stops -- asserted as such.)"""
    case = hn.limits_case(oracle_c, robot, io_dtype)
    chain, ref, cyc, kinds, eps, orc, params = (case[k] for k in ("chain", "ref", "cyc", "kinds", "eps", "orc", "params"))
    hn.assert_caps(ref, cyc, kinds, robot)
    if chain.n == 6:
        assert not cyc["stop"].any()
    else:
        hn.assert_stops(ref, cyc, robot, 8)
    print("\n%s %s: %d arms stop, %d stop-ambiguous, smallest margin %.1e, oracle R %.3f"
          % (robot, np.dtype(io_dtype).name, cyc["stop"].sum(), cyc["stop_amb"].sum(), cyc["margin"][~ref["zone"]].min(), case["R"]))
    failures = []
    hn.check_null(orc["qdot_null"], orc["status"], ref, cyc, np.float64, K_ORACLE, case["scale"], params.null_gain,
                  hn.expected_status(chain.n), "oracle qdot_null", kinds, eps, failures)
    assert not failures, "\n".join(failures)
