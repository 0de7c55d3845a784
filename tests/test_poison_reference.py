"""tests/poison_reference.py on the CPU: the helper's own pieces on hand-made cases, and the C oracle's side of everything the GPU tests
(tests/test_gpu_poison_isolation.py, tests/test_gpu_poison_moves.py) take for granted -- on the very inputs they use: the handles of
tests/test_gpu_variants.py built without a device.

For every family of cycle kernels, both I/O types and every poison kind the family's launch takes, on the oracle alone:
  * the kind matters: every arm of P gets VFIK_ST_NAN and a command row that is not finite -- or the kind is in poison_reference.SWALLOWED,
    and then the oracle's rows of P are all finite, ST_NAN is not set, and the rows differ from the clean run's (the poison did arrive);
  * the oracle's neighbours -- the arms next to P -- are untouched, rows, status and nullspace state bit for bit;
  * the oracle recovers in ONE cycle: the clean cycle behind the poisoned one has finite rows on every arm of P, with no reset in between
    (a NaN in lastvec fails nullspace:101-103's compare, the sign stays and the vector is overwritten).
For every configuration a built variant runs under: the four q kinds matter on its chain (the 6-, 7-, 10- and 14-joint chains, on and off
their DH pattern, with and without tool and IK weights), and a rollout keeps the poison for all its cycles with the clamp on and off."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_variants as kv  # noqa: E402
import poison_reference as pr  # noqa: E402
import test_gpu_variants as tv  # noqa: E402


@pytest.fixture(scope="module")
def env():
    import __graft_entry__ as g
    g.build()
    return pr.host_env()


# ---- the helper's own pieces ----------------------------------------------------------------------------------------------------------
def _inputs(B=141, n=7, K=3, seed=0):
    rng = np.random.default_rng(seed)
    return pr.Inputs(rng.normal(size=(B, n)), null_control=rng.normal(size=(B, 4)), q_ref=rng.normal(size=(B, n)), q_lo=-2 + rng.normal(size=(B, n)),
                     q_hi=2 + rng.normal(size=(B, n)), ext=rng.normal(size=(B, n)), goal=rng.normal(size=(B, 16)), rep=rng.normal(size=(B, K, 4)))


@pytest.mark.parametrize("kind", pr.KINDS)
def test_a_kind_spoils_its_member_on_P_and_nothing_else(kind):
    x = _inputs()
    P = pr.arms(141)
    y = pr.poison(kind, x, P)
    rest = np.setdiff1d(np.arange(141), P)
    for name in pr.Inputs.NAMES:
        a, b = getattr(x, name), getattr(y, name)
        assert pr.same_bits(a[rest], b[rest]), name
        if name == pr.needs(kind):
            bad = ~np.isfinite(b[P].reshape(len(P), -1))
            assert np.all(bad.sum(axis=1) == 1), name            # one element per arm
            assert np.isfinite(b[P].reshape(len(P), -1)[:, 0]).all() or kind == "q_nan_first" or kind == "null_control_nan"
        else:
            assert pr.same_bits(a, b), name
    # a reference, a goal row and a repeller row keep a finite FIRST element: a NaN there is the "leave alone" convention, not poison
    assert np.isfinite(y.q_ref[:, 0]).all() and np.isfinite(y.goal[:, 0]).all() and np.isfinite(y.rep[:, :, 0]).all()


def test_arms_of_P():
    assert list(pr.arms(205)) == [0, 63, 64, 204]
    assert list(pr.arms(205, "eight-lanes")) == [0, 7, 8, 63, 64, 204]
    assert list(pr.arms(65701, "two-waves")) == [0, 63, 65536, 65700]
    with pytest.raises(AssertionError):
        pr.arms(256)          # no partial last wave


def test_the_contract_sentences_on_hand_made_rows():
    nan, inf = np.nan, np.inf
    ref = np.array([[1.0, nan, 3.0], [inf, 2.0, 3.0]])
    assert pr.laundered(ref, ref, 1e-9) == (0, 0, 0.0)
    assert pr.laundered(np.array([[1.0, 5.0, 3.0], [inf, 2.0, 3.0]]), ref, 1e-9)[0] == 1          # a finite value where the oracle has NaN
    assert pr.laundered(np.array([[1.0, -inf, 3.0], [nan, 2.0, 3.0]]), ref, 1e-9)[:2] == (0, 0)    # not finite is not finite
    assert pr.laundered(np.array([[1.0, nan, 3.5], [inf, 2.0, 3.0]]), ref, 1e-9)[1:] == (1, 0.5)
    assert pr.laundered(np.array([[nan, nan, 3.0], [inf, 2.0, 3.0]]), ref, 1e-9)[:2] == (0, 0)     # (C2 allows more NaN inside the arm)
    assert pr.unrecovered(ref, ref, 1e-9) == (0, 0.0)                                              # no finite row: nothing to hold
    fin = np.array([[1.0, 2.0], [3.0, 4.0]])
    assert pr.unrecovered(fin, fin, 1e-9) == (0, 0.0)
    assert pr.unrecovered(np.array([[1.0, nan], [3.0, 4.0]]), fin, 1e-9)[0] == 1                   # C3 allows none
    assert pr.unrecovered(np.array([[1.0, 2.0], [3.0, 4.25]]), fin, 1e-9) == (1, 0.25)
    assert pr.unrecovered(np.array([[1.0, 2.0], [3.0, 4.25]]), np.array([[1.0, 2.0], [3.0, nan]]), 1e-9) == (0, 0.0)
    a = np.array([1.0, nan])
    assert pr.same_bits(a, a.copy()) and not pr.same_bits(a, np.array([1.0, -nan]))
    assert not pr.same_bits(np.array([0.0]), np.array([-0.0]))


def test_np_clip_keeps_a_nan_and_clamps_an_infinity():
    lo, hi = np.array([-1.0, -1.0, -1.0]), np.array([1.0, 1.0, 1.0])
    out = np.clip(np.array([np.nan, np.inf, -np.inf]), lo, hi)
    assert np.isnan(out[0]) and out[1] == 1.0 and out[2] == -1.0


def test_moved_fields_is_the_move_rule(env):
    chain = env.robots.lwr()
    w = env.synth.make_workload(chain, 3, 3, seed=5, io_dtype=np.float32)
    F, nf = w["fields"], w["nfields"]
    goal = np.tile(np.arange(16.0) + 0.1, (3, 1))
    rep = np.tile(np.arange(8.0).reshape(2, 4) + 0.3, (3, 1, 1))
    goal[1, 0] = np.nan          # leaves the goal alone
    goal[2, 3] = np.nan          # goes in
    rep[1, 0, 0] = np.nan        # leaves repeller 0 alone
    rep[2, 1, 1] = np.inf        # goes in
    M = pr.moved_fields(F, nf, goal, rep, np.float32)
    r32 = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)  # noqa: E731
    assert np.array_equal(M["p"][0, 0, :12], r32(goal[0, :12])) and np.array_equal(M["p"][0, 0, 12:], F["p"][0, 0, 12:])
    assert np.array_equal(M["p"][1, 0], F["p"][1, 0])
    assert np.isnan(M["p"][2, 0, 3]) and np.array_equal(M["p"][2, 0, :3], r32(goal[2, :3]))
    assert np.array_equal(M["p"][0, 1, :4], r32(rep[0, 0])) and np.array_equal(M["p"][0, 2, :4], r32(rep[0, 1]))
    assert np.array_equal(M["p"][0, 3], F["p"][0, 3]) and np.array_equal(M["p"][:, :, 4:6][:, 1:], F["p"][:, :, 4:6][:, 1:])
    assert np.array_equal(M["p"][1, 1], F["p"][1, 1]) and np.isinf(M["p"][2, 2, 1])
    for k in ("id", "type", "force"):
        assert np.array_equal(M[k], F[k])


# ---- the oracle's side, family by family ----------------------------------------------------------------------------------------------
def _near(P, B):
    """P and the arms next to it"""
    return np.unique(np.clip(np.concatenate([P - 1, P, P + 1]), 0, B - 1))


CASES = [(f, io) for f in pr.FAMILIES for io in (32, 64) if (f, io) not in pr.NOT_BUILT]


@pytest.mark.parametrize("family,io", CASES, ids=["%s-f%d" % c for c in CASES])
def test_oracle_by_family_and_kind(env, family, io):
    r = pr.pick(kv.by_group(), family, io)
    h = pr.host_handle(env, r, seed=pr.SEED)
    pr.family_setup(h, family)
    P = pr.arms(r.B, family)
    idx = _near(P, r.B)
    inP = np.isin(idx, P)
    clean = pr.family_inputs(h, r, family)
    nxt = pr.family_inputs(h, r, family, second=True)
    want = pr.COMMAND_ROWS + ("pose", "pose_nt", "v6", "qdist", "status")

    def run(first):
        st = env.oc.new_states(len(idx), r.nj) if r.ns else None
        a = pr.oracle_cycle(env.oc, h.chain, h.params, h.w["fields"], h.w["nfields"], h.tool, first, idx, r.t, states=st, want=want)
        a = {k: np.array(v, copy=True) for k, v in a.items() if k != "states"}
        b = pr.oracle_cycle(env.oc, h.chain, h.params, h.w["fields"], h.w["nfields"], h.tool, nxt, idx, r.t, states=st, want=want)
        return a, b, st
    a0, b0, st0 = run(clean)
    assert all(np.isfinite(a0[k]).all() and np.isfinite(b0[k]).all() for k in want if k != "status")
    assert not pr.nan_bit(a0["status"]).any()
    kinds = pr.kinds_of(family, r)
    assert set(pr.Q_KINDS) | set(pr.SCENE_KINDS) <= set(kinds)
    for kind in kinds:
        a, b, st = run(pr.poison(kind, clean, P))
        # the neighbours: rows, status and state bit for bit
        for k in want:
            assert pr.same_bits(a[k][~inP], a0[k][~inP]) and pr.same_bits(b[k][~inP], b0[k][~inP]), (kind, k)
        if r.ns:
            for i in np.flatnonzero(~inP):
                assert bytes(st[i]) == bytes(st0[i]), (kind, idx[i])
        cmd = a["qdot_out"][inP]
        if kind in pr.SWALLOWED:
            assert np.isfinite(cmd).all() and not pr.nan_bit(a["status"][inP]).any(), kind
            assert np.all(np.abs(cmd - a0["qdot_out"][inP]).max(axis=1) > 1e-6), kind       # ... and yet it arrived
        else:
            assert np.all(pr.nan_bit(a["status"][inP])), (kind, a["status"][inP])
            assert np.all((~np.isfinite(cmd)).any(axis=1)), kind
        # recovery: one cycle
        assert all(np.isfinite(b[k][inP]).all() for k in want if k != "status"), kind
        assert not pr.nan_bit(b["status"][inP]).any(), kind
        assert pr.RECOVERY_CYCLES == 1


GROUPS = tv.GROUPS


@pytest.mark.parametrize("nj,io,ns", GROUPS, ids=["nj%d-f%d-%s" % (n, t, "ns" if ns else "plain") for n, t, ns in GROUPS])
def test_q_kinds_matter_under_every_configuration_the_variants_run(env, nj, io, ns):
    variants = kv.by_group().get((nj, io, ns), [])
    assert variants
    seen = {}
    for v in variants:
        r = tv.Recipe(v)
        cfg = r.key + (r.roll, r.limits)
        if cfg in seen:
            continue
        seen[cfg] = True
        h = pr.host_handle(env, r, seed=pr.SEED)
        family = "two-waves" if r.big else "eight-lanes" if r.cap else None
        P = pr.arms(r.B, family)
        q = pr.mixed_q(h.w["q"], P)
        assert pr.same_bits(np.delete(q, P, axis=0), np.delete(h.w["q"], P, axis=0)) and not np.isfinite(q[P]).all(axis=1).any()
        x = pr.Inputs(q, q_lo=h.q_lo if r.limits else None, q_hi=h.q_hi if r.limits else None)
        st = env.oc.new_states(len(P), r.nj) if r.ns else None
        a = pr.oracle_cycle(env.oc, h.chain, h.params, h.w["fields"], h.w["nfields"], h.tool, x, P, r.t, states=st)
        assert np.all(pr.nan_bit(a["status"])), (cfg, a["status"])
        assert np.all((~np.isfinite(a["qdot_out"])).any(axis=1)), cfg
        if r.roll:
            for clamp in (False, True):
                qe, last = pr.oracle_rollout(env.oc, h.chain, h.params, h.w["fields"], h.w["nfields"], h.tool, q, P, r.t, tv.ROLL_K, tv.ROLL_DT, clamp,
                                             states=env.oc.new_states(len(P), r.nj) if r.ns else None)
                assert np.all((~np.isfinite(qe)).any(axis=1)) and np.all((~np.isfinite(last["qdot_out"])).any(axis=1)), (cfg, clamp)
    assert len(seen) >= 1


# ---- the timed moves: the reference's side of tests/test_gpu_poison_moves.py -----------------------------------------------------------
MOVE_CASES = [(m, io) for m in pr.MOVES for io in (32, 64)]


@pytest.mark.parametrize("move,io", MOVE_CASES, ids=["%s-f%d" % c for c in MOVE_CASES])
def test_a_poisoned_arm_in_the_reference_of_a_timed_move(env, move, io):
    """In tests/timed_reference.py's run of poison_reference.move_case: the arms of P have a NaN path from the first check on and VFIK_ST_NAN,
    never arrive and are never at a waypoint; without a stall rule they are under way at every check -- so pending never reaches 0 and a poll
    never ends the move early --, with the rule they stall at the check where the count reaches patience and leave pending; every other arm's
    rows are those of the clean run; and in the clean run arms do arrive, at more than one check (or there would be nothing to isolate)."""
    dt = np.dtype(np.float32 if io == 32 else np.float64)
    n_checks = pr.MOVE_CYCLES // pr.MOVE_STRIDE
    clean, pois = pr.move_case(dt, False), pr.move_case(dt, True)
    P = pois["P"]
    out = np.ones(pr.MOVE_B, dtype=bool)
    out[P] = False
    assert pr.same_bits(clean["q0"][out], pois["q0"][out]) and np.isnan(pois["q0"][P]).sum() == len(P)
    for rule in (False, True):
        for clamp, hold in ((True, True), (True, False), (False, True), (False, False)):
            r0 = pr.move_reference(env.oc, clean, move, clamp, hold, rule)
            r1 = pr.move_reference(env.oc, pois, move, clamp, hold, rule)
            assert np.isnan(r1["q_traj"][:, P]).all() and np.isnan(r1["q"][P]).all() and np.isnan(r1["qdot_out"][P]).all()
            assert pr.nan_bit(r1["status"][P]).all() and not pr.nan_bit(r1["status"][out]).any()
            assert np.all(r1["reached"][P] == -1) and np.all(r1["next"][P] == 0)
            for k in ("q_traj", "dist_traj", "way_traj"):
                assert np.array_equal(r1[k][:, out], r0[k][:, out], equal_nan=True), k
            for k in ("reached", "next", "q", "diff", "qdot_out", "status") + (("stalled",) if rule else ()):
                assert np.array_equal(r1[k][out], r0[k][out], equal_nan=True), k
            uw0, uw1 = pr.under_way(r0, n_checks, pr.MOVE_STRIDE), pr.under_way(r1, n_checks, pr.MOVE_STRIDE)
            assert np.array_equal(uw0.sum(axis=1), r0["pending"]) and np.array_equal(uw1.sum(axis=1), r1["pending"])
            assert np.array_equal(r1["pending"] - r0["pending"], uw1[:, P].sum(axis=1) - uw0[:, P].sum(axis=1))
            # no arm is within the margin of a threshold in the poisoned run: tests/test_gpu_poison_moves.py compares pending and checks_run
            # with this reference only then, so the comparison must not be able to stop running unnoticed
            near = np.minimum.reduce([r1[k] for k in ("closest_c", "closest_j", "closest_s", "closest_sj") if k in r1]) < pr.MOVE_MARGIN[dt]
            assert not near.any(), (move, io, rule, clamp, hold, np.flatnonzero(near))
            takes_part = r1["length"][P] > 0
            if rule:
                at = pr.MOVE_RULE["patience"] * pr.MOVE_STRIDE - 1
                assert np.all(r1["stalled"][P][takes_part] == at) and np.all(r1["stalled"][P][~takes_part] == -1)
                assert not uw1[pr.MOVE_RULE["patience"] - 1:, P].any()
            else:
                assert np.all(uw1[:, P] == takes_part[None, :]) and takes_part.any()
                assert pr.poll_prediction(r1["pending"], 2) == n_checks          # a poisoned arm keeps the move running
            arrived = r0["reached"][np.arange(pr.MOVE_B), np.maximum(r0["length"] - 1, 0)]
            assert len(set(arrived[arrived >= 0])) >= 2 and np.count_nonzero(arrived >= 0) >= pr.MOVE_B // 2
    assert list(pr.poll_prediction(np.array(p), 2) for p in ([3, 2, 0, 0, 0, 0], [3, 0, 1, 0, 0, 0], [1, 1, 1, 1, 1, 0], [0, 1, 1, 1, 1, 1])) == [4, 2, 6, 6]
