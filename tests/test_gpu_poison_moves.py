"""The five timed moves with a poisoned start: vfik_goto, vfik_follow, vfik_goto_js, vfik_follow_js and vfik_script on 130 LWR arms, 24
cycles at stride 4, with the clamp on and off, hold on and off, both I/O types, each once without and once with the stall rule -- and the
arms P (poison_reference.arms: 0, 63, 64, 129) starting from a q with a NaN.  The scene is poison_reference.move_case; coupling, wait rule
and avoid rule stay off (under them an arm's NaN reaches its partner through their documented NaN-row rules, which their own tests cover).

Every combination runs twice on one handle, clean and poisoned, and is held to the contract of include/vfik.h:

  C1  arms outside P: arrived / reached / next, q, q_traj, dist_traj, diff, way_traj, stalled and the rows of the last cycle are the same
      BITS in both runs; pending[k] is the clean run's plus the change in the number of arms of P under way (a poisoned arm never arrives,
      so without a stall rule it stays under way where the clean arm may have arrived; with the rule it is declared stalled and leaves);
      one clean cycle on the same handle behind each move, with no reset, is the same bits outside P too (the per-arm device state).
  C2  arms of P, against tests/timed_reference.py stepped with the same poisoned start (np.clip where the run clamps, which keeps a NaN):
      wherever its q_traj, q, diff or qdot_out is not finite the GPU's is not finite, where both are finite they agree within the suite's
      bars (tests/test_gpu_goto_js.py: 1e-8 / 2e-6 for the path, 1e-7 / 2e-5 for the rows); VFIK_ST_NAN exactly as the reference; a
      poisoned arm never arrives, is never reported at a waypoint, is under way at every check until the stall rule takes it out, and is
      stalled exactly when the reference says.
  C3  the clean cycle behind the move equals the oracle's on P, run on the reference's state and scene as the move left them (the four
      forms whose mixer the handle owns).
  The early exit: checks_run under poll=2 is what the GPU's own pending predicts and -- no arm being within the margin of a threshold in
  the reference's run -- what the reference's pending predicts: a poisoned arm keeps a move without a stall rule running to its end.

What is taken for granted of the reference's side here is asserted in tests/test_poison_reference.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import poison_reference as pr  # noqa: E402
import test_gpu_variants as tv  # noqa: E402

pytestmark = pytest.mark.gpu

N, STRIDE, DT = pr.MOVE_CYCLES, pr.MOVE_STRIDE, pr.MOVE_DT
N_CHECKS = N // STRIDE


@pytest.fixture(scope="module")
def env():
    import __graft_entry__ as g
    g.build()
    from oracle import oracle_c
    from vfclik_amd import _abi, engine
    oracle_c.build()

    class E:
        pass

    e = E()
    e.oc, e.abi, e.engine = oracle_c, _abi, engine
    return e


def _move(eng, c, move, clamp, hold, poll=0):
    io = c["io_dtype"]
    q = c["q0"].astype(io)
    prec, via = pr.move_js_prec(c["chain"].n)
    common = dict(stride=STRIDE, hold=hold, clamp=clamp, trajectory=True, want=pr.MOVE_WANT, poll=poll)
    eng.set_fields(c["w"]["fields"], c["w"]["nfields"])
    eng.reset_state()
    if move == "goto":
        return eng.goto_host(q, N, DT, pr.MOVE_PREC, **common)
    if move == "follow":
        return eng.follow_host(q, c["way"], N, DT, pr.MOVE_PREC, via_precision=pr.MOVE_VIA, **common)
    if move == "goto_js":
        return eng.goto_js_host(q, c["q_ref"].astype(io), N, DT, prec, **common)
    if move == "follow_js":
        return eng.follow_js_host(q, c["wayq"], N, DT, prec, via_precision=via, **common)
    return eng.script_host(q, c["kind"], c["way_s"], c["wayq_s"], N, DT, pr.MOVE_PREC, prec, via_precision=pr.MOVE_VIA, js_via_precision=via,
                           **common)


PER_ARM = ("arrived", "reached", "next", "q", "diff", "stalled", "qdot_out", "status")
PER_CHECK = ("q_traj", "dist_traj", "way_traj")


def _sub_states(st, P):
    sub = (type(st[0]) * len(P))()
    for i, b in enumerate(P):
        sub[i] = st[int(b)]
    return sub


CASES = [(m, io) for m in pr.MOVES for io in (32, 64)]


@pytest.mark.parametrize("move,io", CASES, ids=["%s-f%d" % c for c in CASES])
def test_a_poisoned_start_stays_in_its_arm(env, move, io):
    dt = np.dtype(np.float32 if io == 32 else np.float64)
    tol_q, tol_v = pr.MOVE_TOL[dt]
    clean, pois = pr.move_case(dt, False), pr.move_case(dt, True)
    P = pois["P"]
    B, n = clean["q0"].shape
    out = np.ones(B, dtype=bool)
    out[P] = False
    q_next = clean["q_ref"]
    failures = []
    for rule in (False, True):
        eng = env.engine.Engine(clean["chain"], B, io_dtype=dt, max_slots=8, params=clean["params"])
        if rule:
            eng.set_stall_rule(**pr.MOVE_RULE)
        try:
            for clamp in (True, False):
                for hold in (True, False):
                    what = "%s float%d rule %s clamp %s hold %s" % (move, io, rule, clamp, hold)
                    bad = []
                    ref = pr.move_reference(env.oc, pois, move, clamp, hold, rule)
                    g0 = _move(eng, clean, move, clamp, hold)
                    s0 = eng.step_host(q_next, want=tv.ROWS)
                    g1 = _move(eng, pois, move, clamp, hold)
                    s1 = eng.step_host(q_next, want=tv.ROWS)
                    assert g0["checks_run"] == N_CHECKS and g1["checks_run"] == N_CHECKS
                    assert set(g0) == set(g1) and ("stalled" in g1) == rule
                    # ---- C1
                    for k in PER_ARM:
                        if k in g1 and not pr.same_bits(g1[k][out], g0[k][out]):
                            bad.append("C1 %s differs outside P" % k)
                    for k in PER_CHECK:
                        if k in g1 and not pr.same_bits(g1[k][:, out], g0[k][:, out]):
                            bad.append("C1 %s differs outside P" % k)
                    for k in tv.ROWS:
                        if not pr.same_bits(s1[k][out], s0[k][out]):
                            bad.append("C1 the clean cycle behind the move: %s differs outside P" % k)
                    for g in (g0, g1):
                        g["length"] = ref["length"]
                    uw0, uw1 = pr.under_way(g0, N_CHECKS, STRIDE), pr.under_way(g1, N_CHECKS, STRIDE)
                    if not np.array_equal(uw0.sum(axis=1), g0["pending"]) or not np.array_equal(uw1.sum(axis=1), g1["pending"]):
                        bad.append("pending is not the count of arms under way: %s / %s, %s / %s" % (g0["pending"], uw0.sum(axis=1), g1["pending"], uw1.sum(axis=1)))
                    delta = uw1[:, P].sum(axis=1).astype(np.int64) - uw0[:, P].sum(axis=1)
                    if not np.array_equal(g1["pending"].astype(np.int64) - g0["pending"], delta):
                        bad.append("C1 pending %s, the clean run's %s, the arms of P account for %s" % (g1["pending"], g0["pending"], delta))
                    # ---- C2
                    for k, tol in (("q_traj", tol_q), ("q", tol_q), ("diff", 2 * tol_q), ("qdot_out", tol_v)):
                        if k not in g1:
                            continue
                        a, b = (g1[k][:, P], ref[k][:, P]) if k == "q_traj" else (g1[k][P], ref[k][P])
                        laund, nbad, e = pr.laundered(a, b, tol)
                        if laund or nbad:
                            bad.append("C2 %s on P: finite in %d elements where the reference is not, %d beyond the bar (worst %.2e, bar %.0e)" % (k, laund, nbad, e, tol))
                    if not np.isnan(ref["q_traj"][:, P]).all():
                        bad.append("the reference's path of P is not NaN throughout")
                    if not np.array_equal(pr.nan_bit(g1["status"][P]), pr.nan_bit(ref["status"][P])) or not pr.nan_bit(g1["status"][P]).all():
                        bad.append("C2 ST_NAN on P %s, the reference's %s" % (g1["status"][P], ref["status"][P]))
                    if "arrived" in g1:
                        if not np.all(g1["arrived"][P] == -1):
                            bad.append("C2 a poisoned arm arrived: %s" % g1["arrived"][P])
                    else:
                        if not (np.all(g1["reached"][P] == -1) and np.all(g1["next"][P] == 0)):
                            bad.append("C2 a poisoned arm was reported at a waypoint: %s next %s" % (g1["reached"][P], g1["next"][P]))
                        if not np.array_equal(g1["way_traj"][:, P], ref["way_traj"][:, P]):
                            bad.append("C2 way_traj of P differs from the reference's")
                    if rule and not np.array_equal(g1["stalled"][P], ref["stalled"][P]):
                        bad.append("C2 stalled on P %s, the reference's %s" % (g1["stalled"][P], ref["stalled"][P]))
                    if not np.array_equal(uw1[:, P], pr.under_way(ref, N_CHECKS, STRIDE)[:, P]):
                        bad.append("C2 the arms of P under way differ from the reference's")
                    # ---- C3: the clean cycle behind the move, on the reference's state and scene
                    if move != "script":
                        st = _sub_states(ref["states"], P)
                        o = pr.oracle_cycle(env.oc, clean["chain"], clean["params"], ref["fields"], clean["w"]["nfields"], None, pr.Inputs(q_next), P, dt,
                                            states=st)
                        for k in tv.ROWS:
                            if k == "status":
                                if not np.array_equal(s1[k][P], o[k]):
                                    bad.append("C3 status of P behind the move %s, the oracle's %s" % (s1[k][P], o[k]))
                                continue
                            nun, e = pr.unrecovered(s1[k][P], o[k], 1e-6 if io == 32 else 1e-9)
                            if nun:
                                bad.append("C3 %s of %d arms of P behind the move (worst %.2e)" % (k, nun, e))
                    # ---- the early exit
                    early = _move(eng, pois, move, clamp, hold, poll=2)
                    own = pr.poll_prediction(g1["pending"], 2)
                    if early["checks_run"] != own:
                        bad.append("checks_run under poll=2 is %d, the run's own pending %s says %d" % (early["checks_run"], g1["pending"], own))
                    near = np.minimum.reduce([ref[k] for k in ("closest_c", "closest_j", "closest_s", "closest_sj") if k in ref]) < pr.MOVE_MARGIN[dt]
                    if not near.any():
                        if not np.array_equal(g1["pending"], ref["pending"]):
                            bad.append("pending %s, the reference's %s" % (g1["pending"], ref["pending"]))
                        if early["checks_run"] != pr.poll_prediction(ref["pending"], 2):
                            bad.append("checks_run under poll=2 is %d, the reference's pending %s says %d" % (early["checks_run"], ref["pending"], pr.poll_prediction(ref["pending"], 2)))
                    if not rule and early["checks_run"] != N_CHECKS:
                        bad.append("a move with a poisoned arm and no stall rule ended early, at check %d" % early["checks_run"])
                    failures += ["%s: %s" % (what, b) for b in bad]
        finally:
            eng.close()
    assert not failures, "\n".join(failures)
