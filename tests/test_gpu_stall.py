"""The stall rule of the timed moves (include/vfik.h: vfik_set_stall_rule) on the GPU against its restatement with the oracle
(tests/timed_reference.py): which arm stalls at which check, beside which arm arrives, in vfik_goto (float64 and float32), vfik_goto_js and
vfik_script; the state machine replayed on the GPU's own rows; arms without a goal block and the two values of `stop`; the early exit of
the host form; the rule switched off again; the errors, the device-pointer form and the sharded form.

Inputs are those of tests/test_gpu_goto.py, tests/test_gpu_goto_js.py and tests/test_gpu_script.py (their `_case`, restated here), with
some arms sent where they cannot arrive: a goal position three times as far from the base, a posture 0.3 rad beyond a joint limit.

A stall is a threshold decision like an arrival: an arm any of whose progress compares m < best - eps comes, in the ORACLE's run, within
the margin of its threshold is left out of the exact comparison with the oracle, with the arms near an arrival threshold -- frame
decisions 1e-6 (float32 I/O: 1e-4), posture decisions 1e-7 (4e-6), at most 5 % (15 %) of the arms that take part, asserted on the
oracle's numbers before the GPU's are read.  EVERY arm, left out or not, is held to the helper's machine replayed on the GPU's own
q_traj and dist_traj rows: stalled, arrived / reached, next and pending exact.

The helper on the CPU: goto float64 (200 arms, `3::8` out of reach, stride 4, patience 5, eps (1e-3, 1e-2)): 3 arms left out, all 175
reachable arms arrive and none stalls, all 25 others stall, the last at cycle 231.  goto float32 (203 arms, `3::16`, stride 8, patience
3, eps (4e-3, 4e-2)): 12 left out, 189 arrive, the 13 out of reach stall by cycle 103 (and one reachable arm that creeps)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import timed_reference as st  # noqa: E402

pytestmark = pytest.mark.gpu

DT, PREC, KP = 0.01, (0.01, 0.05), 8.0
# frame decisions, posture decisions, the share of arms that may be left out (tests/test_gpu_script.py)
MARGIN = {np.dtype(np.float64): (1e-6, 1e-7, 0.05), np.dtype(np.float32): (1e-4, 4e-6, 0.15)}
TOL_Q = {np.dtype(np.float64): 1e-8, np.dtype(np.float32): 2e-6}
F, P = st.FRAME, st.POSTURE
PATTERNS = np.array([[P, F, F, P], [F, P, F, 0], [P, P, F, F], [F, F, P, P]], dtype=np.int32)
MIX_JOINT = [0.0, 0.0, 1.0, 0.0, 0.0, 0.0]


def _prec(n):
    return 0.004 + 0.002 * np.arange(n)


@pytest.fixture(scope="module")
def env():
    import __graft_entry__ as g
    g.build()
    from oracle import oracle_c
    from vfclik_amd import _abi, engine, robots, sharding, synth

    class E:
        pass

    e = E()
    e.oc, e.abi, e.engine, e.robots, e.synth, e.sharding = oracle_c, _abi, engine, robots, synth, sharding
    e.cache = {}
    return e


def _frozen(ref):
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ref


def _engine(env, chain, B, io_dtype, params, w):
    eng = env.engine.Engine(chain, B, io_dtype=io_dtype, max_slots=8, params=params)
    eng.set_fields(w["fields"], w["nfields"])
    return eng


def _left_out(ref, part, io_dtype):
    """The arms within a margin of an arrival or a stall threshold in the oracle's run -- frame decisions and posture decisions each with
    their own margin; the cap holds on the oracle's numbers alone."""
    mc, mj, cap = MARGIN[np.dtype(io_dtype)]
    near_stall = (ref["closest_s"] < mc) | (ref["closest_sj"] < mj)
    out = (ref["closest_c"] < mc) | (ref["closest_j"] < mj) | near_stall
    share = np.count_nonzero(out & part) / max(np.count_nonzero(part), 1)
    print("left out: %d of %d arms (%.1f %%, cap %.0f %%), %d of them near a stall threshold; %d stall, the last at cycle %d"
          % (np.count_nonzero(out & part), np.count_nonzero(part), 100 * share, 100 * cap, np.count_nonzero(near_stall & part),
             np.count_nonzero(ref["stalled"] >= 0), ref["stalled"].max()))
    assert share <= cap, share
    return out


def _own_pending(done_at, part, n_checks, stride):
    """pending[k] as the arms' own outcomes imply it: done_at (B,) the cycle at which the arm finished or stalled, -1: neither"""
    cyc = (np.arange(n_checks) + 1) * stride - 1
    return np.array([np.count_nonzero(part & ((done_at < 0) | (done_at > c))) for c in cyc], dtype=np.int32)


def _stopped_rows_repeat(got, stride, keys):
    """stop = 1: a stalled arm's rows after its stall check are that check's, bit for bit"""
    for b in np.flatnonzero(got["stalled"] >= 0):
        k = (got["stalled"][b] + 1) // stride - 1
        for key in keys:
            assert np.all(got[key][k:, b] == got[key][k, b]), (key, b)


# ---- 1, 2, 3: goto ------------------------------------------------------------------------------------------------------------------
GOTO = {np.dtype(np.float64): dict(B=200, far=slice(3, None, 8), flags=5, stride=4, rule=dict(patience=5, eps=(1e-3, 1e-2))),
        np.dtype(np.float32): dict(B=203, far=slice(3, None, 16), flags=0, stride=8, rule=dict(patience=3, eps=(4e-3, 4e-2)))}
GOTO_CYCLES = 400


def _goto_case(env, io_dtype):
    """tests/test_gpu_goto.py's inputs; the arms `far` get their goal position times 3"""
    c = GOTO[np.dtype(io_dtype)]
    B = c["B"]
    chain = env.robots.lwr()
    w = env.synth.make_workload(chain, B, 3, seed=53, io_dtype=np.dtype(io_dtype).type)
    rng = np.random.default_rng(7)
    qg = rng.uniform(0.7 * chain.q_lo, 0.7 * chain.q_hi, size=(B, chain.n))
    s = rng.uniform(0.02, 0.25, size=(B, 1))
    q0 = (qg + s * rng.uniform(-1.0, 1.0, size=(B, chain.n))).astype(io_dtype).astype(np.float64)
    goal = chain.fk(qg).reshape(B, 16)
    goal[c["far"], 3::4] *= [3.0, 3.0, 3.0, 1.0]
    w["fields"]["p"][:, 0, :16] = goal.astype(io_dtype).astype(np.float64)
    far = np.zeros(B, dtype=bool)
    far[c["far"]] = True
    return chain, w, q0, far, env.abi.default_params(flags=c["flags"], max_vel=0.7)


def _goto_reference(env, io_dtype):
    key = ("goto", np.dtype(io_dtype).name)
    if key not in env.cache:
        c = GOTO[np.dtype(io_dtype)]
        chain, w, q0, far, params = _goto_case(env, io_dtype)
        ref = st.goto(env.oc, chain, params, q0, w["fields"], w["nfields"], GOTO_CYCLES, c["stride"], DT, PREC, rule=st.Rule(**c["rule"]),
                      hold=True, clamp=True, io_dtype=io_dtype, want=("qdot_out",))
        env.cache[key] = (chain, w, q0, far, params, _frozen(ref))
    return env.cache[key]


@pytest.mark.parametrize("io_dtype", [np.float64, np.float32])
def test_goto_stalls(env, io_dtype):
    """vfik_goto with arms out of reach: hold, stop, 400 cycles.  Against the oracle outside the margins, and every arm against the
    machine replayed on the GPU's own rows."""
    io_dtype = np.dtype(io_dtype)
    c = GOTO[io_dtype]
    chain, w, q0, far, params, ref = _goto_reference(env, io_dtype)
    B, stride, n_checks = c["B"], c["stride"], GOTO_CYCLES // c["stride"]
    part = np.ones(B, dtype=bool)
    out = _left_out(ref, part, io_dtype)
    inc = ~out
    # what the oracle shows: every arm out of reach stalls, (nearly) every other arrives, nobody does both
    assert np.all(ref["stalled"][far] >= 0) and np.all(ref["arrived"][far] == -1)
    assert np.count_nonzero(ref["arrived"][~far] >= 0) >= np.count_nonzero(~far) - 1 and not np.any((ref["arrived"] >= 0) & (ref["stalled"] >= 0))
    eng = _engine(env, chain, B, io_dtype, params, w)
    eng.set_stall_rule(c["rule"]["patience"], eps=c["rule"]["eps"], stop=True)
    got = eng.goto_host(q0.astype(io_dtype), GOTO_CYCLES, DT, PREC, stride=stride, hold=True, clamp=True, trajectory=True, want=("qdot_out",))
    eng.close()
    assert got["checks_run"] == n_checks and got["stalled"].dtype == np.int32
    print("stalled: %d, arrived: %d" % (np.count_nonzero(got["stalled"] >= 0), np.count_nonzero(got["arrived"] >= 0)))
    for k in ("stalled", "arrived"):
        assert np.array_equal(got[k][inc], ref[k][inc]), (k, np.flatnonzero(inc & (got[k] != ref[k])))
    assert np.abs(got["pending"].astype(np.int64) - ref["pending"]).max() <= np.count_nonzero(out)
    if not out.any():
        assert np.array_equal(got["pending"], ref["pending"])
    eq = np.abs(got["q_traj"][:, inc].astype(np.float64) - ref["q_traj"][:, inc]).max()
    print("q_traj max error %.3e (tolerance %.1e)" % (eq, TOL_Q[io_dtype]))
    assert eq < TOL_Q[io_dtype]
    # every arm: the machine on the GPU's own rows
    m = st.replay(np.full((B, 1), F, dtype=np.int32), np.zeros((B, 1, chain.n)), ref["present"], got["q_traj"], got["dist_traj"], GOTO_CYCLES,
                  stride, PREC, np.zeros(chain.n), hold=True, io_dtype=io_dtype, rule=st.Rule(**c["rule"]))
    assert np.array_equal(got["stalled"], m.stalled), np.flatnonzero(got["stalled"] != m.stalled)
    assert np.array_equal(got["arrived"], m.reached[:, 0]) and np.array_equal(got["pending"], m.pending)
    done_at = np.maximum(got["arrived"], got["stalled"])
    assert np.array_equal(got["pending"], _own_pending(done_at, part, n_checks, stride))
    _stopped_rows_repeat(got, stride, ("q_traj", "dist_traj"))
    assert np.array_equal(got["q"], got["q_traj"][-1])


def test_goto_stop_without_hold(env):
    """hold off, no caller's gate, one goal: the rule's `stop` is then the ONLY reason the blocks run under the handle's gate.  The
    stalled arms' rows repeat from their stall check on, the arms that arrived keep tracking their goal, and all of it is the oracle's."""
    io_dtype = np.dtype(np.float64)
    c = GOTO[io_dtype]
    chain, w, q0, far, params = _goto_case(env, io_dtype)
    B, stride, n_checks = c["B"], c["stride"], GOTO_CYCLES // c["stride"]
    rule = st.Rule(**c["rule"])
    ref = st.goto(env.oc, chain, params, q0, w["fields"], w["nfields"], GOTO_CYCLES, stride, DT, PREC, rule=rule, hold=False, clamp=True,
                  want=("qdot_out",))
    part = np.ones(B, dtype=bool)
    inc = ~_left_out(ref, part, io_dtype)
    assert np.all(ref["stalled"][far] >= 0) and np.count_nonzero(ref["arrived"] >= 0) >= np.count_nonzero(~far) - 1
    eng = _engine(env, chain, B, io_dtype, params, w)
    eng.set_stall_rule(rule.patience, eps=rule.eps, stop=True)
    got = eng.goto_host(q0, GOTO_CYCLES, DT, PREC, stride=stride, hold=False, clamp=True, trajectory=True, want=("qdot_out",))
    eng.close()
    assert got["checks_run"] == n_checks
    for k in ("stalled", "arrived"):
        assert np.array_equal(got[k][inc], ref[k][inc]), (k, np.flatnonzero(inc & (got[k] != ref[k])))
    # The path, up to the check that decided the arm (a stalled arm's rows repeat from there: the whole path).  Beyond its arrival an arm
    # without hold hovers on its goal, where the cycle normalises a vanishing twist; that part of the path is no decision of this rule
    # and is not held to 1e-8 here.  (Seen: one arm of 200, arrived at cycle 15, leaves the oracle's path at cycle 211 by up to 4e-3 rad
    # and is back within 6e-5 at cycle 399 -- the same with the rule off and without the nullspace module.)
    done_at = np.maximum(got["arrived"], got["stalled"])
    upto = np.where(got["arrived"] >= 0, (done_at + 1) // stride, n_checks)
    live = np.arange(n_checks)[:, None] < upto[None, :]
    err = np.abs(got["q_traj"] - ref["q_traj"]).max(axis=2)
    eq = err[live & inc[None, :]].max()
    print("q_traj max error %.3e up to every arm's arrival (tolerance %.1e); %.3e beyond" % (eq, TOL_Q[io_dtype], err[:, inc].max()))
    assert eq < TOL_Q[io_dtype]
    m = st.replay(np.full((B, 1), F, dtype=np.int32), np.zeros((B, 1, chain.n)), ref["present"], got["q_traj"], got["dist_traj"], GOTO_CYCLES,
                  stride, PREC, np.zeros(chain.n), hold=False, rule=rule)
    assert np.array_equal(got["stalled"], m.stalled) and np.array_equal(got["arrived"], m.reached[:, 0]) and np.array_equal(got["pending"], m.pending)
    assert np.count_nonzero(got["stalled"] >= 0) >= np.count_nonzero(far)
    _stopped_rows_repeat(got, stride, ("q_traj", "dist_traj"))                       # stop: a stalled arm takes no further cycle
    for b in np.flatnonzero((got["arrived"] >= 0) & (got["arrived"] < GOTO_CYCLES - stride)):
        k = (got["arrived"][b] + 1) // stride - 1
        assert np.any(got["q_traj"][k + 1, b] != got["q_traj"][k, b]), b             # no hold: an arm that arrived keeps running


# ---- 4: goto_js ---------------------------------------------------------------------------------------------------------------------
JS = dict(B=130, stride=4, n_cycles=160, rule=dict(patience=4, eps_js=1e-3))


def _js_case(env, io_dtype=np.float64):
    """tests/test_gpu_goto_js.py's inputs; arms ::6 are sent 0.3 rad beyond the upper limit of joint 1"""
    B = JS["B"]
    chain = env.robots.lwr()
    w = env.synth.make_workload(chain, B, 3, seed=53, io_dtype=np.dtype(io_dtype).type)
    rng = np.random.default_rng(7)
    ref = rng.uniform(0.7 * chain.q_lo, 0.7 * chain.q_hi, size=(B, chain.n))
    s = rng.uniform(0.02, 0.25, size=(B, 1))
    q0 = (ref + s * rng.uniform(-1.0, 1.0, size=(B, chain.n))).astype(io_dtype).astype(np.float64)
    ref[::6, 1] = chain.q_hi[1] + 0.3
    ref = ref.astype(io_dtype).astype(np.float64)
    return chain, w, q0, ref, env.abi.default_params(flags=env.abi.F_MIXER, mix_w=MIX_JOINT, jp_kp=KP)


def test_goto_js_beyond_a_limit(env):
    """vfik_goto_js with clamp: a posture 0.3 rad beyond a limit never arrives -- the arm creeps up to the limit and stalls; the others
    arrive.  diff is (T)(ref - q) of the last check the arm ran, bit for bit: its arrival check, or the check that stalled it."""
    B, stride, n_cycles = JS["B"], JS["stride"], JS["n_cycles"]
    n_checks = n_cycles // stride
    chain, w, q0, q_ref, params = _js_case(env)
    rule = st.Rule(**JS["rule"])
    ref = st.goto_js(env.oc, chain, params, q0, w["fields"], w["nfields"], q_ref, n_cycles, stride, DT, _prec(chain.n), rule=rule, hold=True,
                     clamp=True, want=("qdot_out",))
    part = np.ones(B, dtype=bool)
    out = _left_out(ref, part, np.float64)
    inc = ~out
    beyond = np.zeros(B, dtype=bool)
    beyond[::6] = True
    assert np.all(ref["stalled"][beyond] >= 0) and np.all(ref["arrived"][beyond] == -1)
    assert np.all(ref["arrived"][~beyond] >= 0) and np.all(ref["stalled"][~beyond] == -1)
    eng = _engine(env, chain, B, np.float64, params, w)
    eng.set_stall_rule(rule.patience, eps_js=rule.eps_js, stop=True)
    got = eng.goto_js_host(q0, q_ref, n_cycles, DT, _prec(chain.n), stride=stride, hold=True, clamp=True, trajectory=True, want=("qdot_out",))
    eng.close()
    assert got["checks_run"] == n_checks
    for k in ("stalled", "arrived"):
        assert np.array_equal(got[k][inc], ref[k][inc]), (k, np.flatnonzero(inc & (got[k] != ref[k])))
    eq = np.abs(got["q_traj"][:, inc] - ref["q_traj"][:, inc]).max()
    print("q_traj max error %.3e" % eq)
    assert eq < 1e-8
    m = st.replay(np.full((B, 1), P, dtype=np.int32), q_ref[:, None, :], np.ones(B, dtype=bool), got["q_traj"], None, n_cycles, stride,
                  (0.0, 0.0), _prec(chain.n), hold=True, rule=rule)
    assert np.array_equal(got["stalled"], m.stalled) and np.array_equal(got["arrived"], m.reached[:, 0]) and np.array_equal(got["pending"], m.pending)
    done_at = np.maximum(got["arrived"], got["stalled"])
    assert np.all(done_at >= 0) and got["pending"][-1] == 0
    last = (done_at + 1) // stride - 1
    want = q_ref - got["q_traj"][last, np.arange(B)]
    assert np.array_equal(got["diff"], want) and np.array_equal(got["diff"], m.diff)
    _stopped_rows_repeat(got, stride, ("q_traj",))
    # they stopped just under the limit: the controller closes 1 - 0.92^4 = 0.28 of what is left per check, less than eps_js from 3.5e-3 on
    left = chain.q_hi[1] - got["q_traj"][-1, beyond, 1]
    assert np.all(left >= 0) and np.all(left < 1e-3 / (1.0 - (1.0 - KP * DT) ** stride))


# ---- 5: scripts ---------------------------------------------------------------------------------------------------------------------
W, SCRIPT_CYCLES = 4, 320   # (the 14-joint arms sent out of reach stall by cycle 291)
SCRIPT = {("lwr_dual14", 130): dict(io_dtype=np.float64, stride=4, rule=dict(patience=5, eps=(1e-3, 1e-2), eps_js=1e-3)),
          ("lwr", 203): dict(io_dtype=np.float32, stride=8, rule=dict(patience=3, eps=(4e-3, 4e-2), eps_js=1e-3))}
# (float32: the frame margin 1e-4 is 2.5 % of eps_pos, so an arm whose gain per check passes through eps on its way is likely left out.  With
# stride 8 an arm 0.01 m from its goal still gains 0.49 * 0.01 m a check, more than eps: it arrives before its gain gets there.  Stride 4
# and eps 4e-3 leave 72 of 202 arms out.)


def _script_case(env, robot, B, io_dtype=np.float64, kinds=None, far=True):
    """tests/test_gpu_script.py's inputs; far: step 2 of the arms ::5 cannot be reached -- a frame three times as far from the base, a
    posture 0.3 rad beyond the upper limit of joint 1"""
    chain = env.robots.by_name(robot)
    n = chain.n
    w = env.synth.make_workload(chain, B, 3, seed=53, io_dtype=np.dtype(io_dtype).type)
    rng = np.random.default_rng(21)
    qg = np.zeros((B, W, n))
    qg[:, 0] = rng.uniform(0.6 * chain.q_lo, 0.6 * chain.q_hi, size=(B, n))
    for i in range(1, W):
        qg[:, i] = qg[:, i - 1] + 0.12 * rng.uniform(-1.0, 1.0, size=(B, n))
    s = rng.uniform(0.02, 0.12, size=(B, 1))
    q0 = (qg[:, 0] + s * rng.uniform(-1.0, 1.0, size=(B, n))).astype(io_dtype).astype(np.float64)
    way = chain.fk(qg.reshape(B * W, n)).reshape(B, W, 16)
    if far:
        way[::5, 2, 3::4] *= [3.0, 3.0, 3.0, 1.0]
        qg[::5, 2, 1] = chain.q_hi[1] + 0.3
    way = way.astype(io_dtype).astype(np.float64)
    wayq = qg.astype(io_dtype).astype(np.float64)
    kind = PATTERNS[np.arange(B) % 4].copy() if kinds is None else np.full((B, W), kinds, dtype=np.int32)
    kind[7::10, 1:] = 0
    kind[5] = 0
    return chain, w, q0, kind, way, wayq, env.abi.default_params(flags=env.abi.F_MIXER, max_vel=0.7, jp_kp=KP)


@pytest.mark.parametrize("robot,B", list(SCRIPT))
def test_script_stalls(env, robot, B):
    """vfik_script with step 2 of every fifth arm out of reach: those arms reach steps 0 and 1 and stall at step 2; the others finish,
    although they take more than `patience` checks in total: the advance resets an arm's state."""
    c = SCRIPT[(robot, B)]
    io_dtype, stride = np.dtype(c["io_dtype"]), c["stride"]
    n_checks = SCRIPT_CYCLES // stride
    chain, w, q0, kind, way, wayq, params = _script_case(env, robot, B, io_dtype)
    p = _prec(chain.n)
    rule = st.Rule(**c["rule"])
    ref = _frozen(st.script(env.oc, chain, params, q0, w["fields"], w["nfields"], kind, way, wayq, SCRIPT_CYCLES, stride, DT, PREC, p,
                            js_via_precision=3 * p, hold=True, clamp=True, io_dtype=io_dtype, want=("qdot_out",), stepped=chain.n > 7, rule=rule))
    L = st.lengths(kind)
    part = L > 0
    out = _left_out(ref, part, io_dtype)
    done = part & (ref["next"] == L)
    fin = ref["reached"][np.arange(B), np.maximum(L - 1, 0)]
    print("%d arms finish" % np.count_nonzero(done))
    inc = ~out
    far = np.zeros(B, dtype=bool)
    far[::5] = True
    far &= L > 2
    # what the oracle shows: the arms sent out of reach stall at step 2, nearly every other arm finishes, and those that finish needed
    # more checks than the patience
    assert np.all(ref["stalled"][far] >= 0) and np.all(ref["next"][far] == 2)
    assert np.count_nonzero(done) >= 0.9 * np.count_nonzero(part & ~far) and not np.any(done & (ref["stalled"] >= 0))
    assert np.all((fin[done & (L > 1)] + 1) // stride > rule.patience)
    eng = _engine(env, chain, B, io_dtype, params, w)
    eng.set_stall_rule(rule.patience, eps=rule.eps, eps_js=rule.eps_js, stop=True)
    got = eng.script_host(q0.astype(io_dtype), kind, way, wayq, SCRIPT_CYCLES, DT, PREC, p, js_via_precision=3 * p, stride=stride, hold=True,
                          clamp=True, trajectory=True, want=("qdot_out",))
    eng.close()
    assert got["checks_run"] == n_checks
    for k in ("reached", "next", "stalled"):
        assert np.array_equal(got[k][inc], ref[k][inc]), (k, np.flatnonzero(inc & np.any(np.atleast_2d(got[k].T != ref[k].T), axis=0)))
    assert np.array_equal(got["way_traj"][:, inc], ref["way_traj"][:, inc])
    eq = np.abs(got["q_traj"][:, inc].astype(np.float64) - ref["q_traj"][:, inc]).max()
    print("q_traj max error %.3e (tolerance %.1e)" % (eq, TOL_Q[io_dtype]))
    assert eq < TOL_Q[io_dtype]
    m = st.replay(kind, wayq, ref["present"], got["q_traj"], got["dist_traj"], SCRIPT_CYCLES, stride, PREC, p, js_via_precision=3 * p, hold=True,
                  io_dtype=io_dtype, rule=rule)
    assert np.array_equal(got["stalled"], m.stalled), np.flatnonzero(got["stalled"] != m.stalled)
    assert np.array_equal(got["reached"], m.reached) and np.array_equal(got["next"], m.next)
    assert np.array_equal(got["way_traj"], m.way_traj) and np.array_equal(got["pending"], m.pending) and np.array_equal(got["diff"], m.diff)
    _stopped_rows_repeat(got, stride, ("q_traj", "dist_traj", "way_traj"))


def test_pure_scripts_equal_follow_and_follow_js_with_the_rule(env):
    """With the rule set a frames-only script is vfik_follow and a postures-only script vfik_follow_js on a handle whose mixer holds the
    kind's weights, bit for bit, `stalled` included: 70 arms, step 2 of every fifth out of reach."""
    B = 70
    for kinds, mix_w in ((F, [1, 1, 0, 0, 0, 0]), (P, MIX_JOINT)):
        chain, w, q0, kind, way, wayq, _ = _script_case(env, "lwr", B, kinds=kinds)
        params = env.abi.default_params(flags=env.abi.F_MIXER, max_vel=0.7, jp_kp=KP, mix_w=mix_w)
        eng = _engine(env, chain, B, np.float64, params, w)
        eng.set_stall_rule(5, eps=(1e-3, 1e-2), eps_js=1e-3, stop=True)
        p = _prec(7)
        kw = dict(stride=4, hold=True, clamp=True, trajectory=True, want=("qdot_out", "status"))
        if kinds == F:
            way_nan = way.copy()
            way_nan[kind == 0] = np.nan
            a = eng.follow_host(q0, way_nan, SCRIPT_CYCLES, DT, PREC, **kw)
            keys = ("q", "reached", "next", "pending", "q_traj", "dist_traj", "way_traj", "qdot_out", "status", "stalled")
        else:
            wayq_nan = wayq.copy()
            wayq_nan[kind == 0] = np.nan
            a = eng.follow_js_host(q0, wayq_nan, SCRIPT_CYCLES, DT, p, via_precision=3 * p, **kw)
            keys = ("q", "reached", "next", "pending", "q_traj", "way_traj", "diff", "qdot_out", "status", "stalled")
        eng.reset_state()
        b = eng.script_host(q0, kind, way, wayq, SCRIPT_CYCLES, DT, PREC, p, js_via_precision=3 * p, **kw)
        eng.close()
        far = np.arange(B) % 5 == 0
        far &= st.lengths(kind) > 2
        print("kind %d: %d arms stall, %d finish" % (kinds, np.count_nonzero(a["stalled"] >= 0), np.count_nonzero(a["next"] == 4)))
        assert np.all(a["stalled"][far] >= 0) and np.all(a["next"][far] == 2) and np.count_nonzero(a["next"] == 4) >= 40
        assert a["checks_run"] == b["checks_run"]
        for k in keys:
            assert np.array_equal(a[k], b[k]), (kinds, k)


# ---- 6: arms without a goal block, stop = 0 against stop = 1 ---------------------------------------------------------------------------
def test_no_goal_block_and_stop(env):
    """2 * 256 + 37 arms (two full blocks of the check kernel and a partial one).  The odd arms have no field at all: their measure is
    NaN, never progress, so they stall at check patience - 1 exactly.  They are driven by an external command on mixer channel 3 alone:
    with stop = 0 they keep moving after the stall, with stop = 1 they stay where the stall check found them.  The rows of every arm
    that does not stall are the same in both runs, bit for bit."""
    B, stride, patience, n_cycles = 2 * 256 + 37, 4, 3, 80
    chain = env.robots.lwr()
    w = env.synth.make_workload(chain, B, 3, seed=53, io_dtype=np.float64)
    rng = np.random.default_rng(7)
    qg = rng.uniform(0.7 * chain.q_lo, 0.7 * chain.q_hi, size=(B, chain.n))
    q0 = qg + rng.uniform(0.02, 0.25, size=(B, 1)) * rng.uniform(-1.0, 1.0, size=(B, chain.n))
    w["fields"]["p"][:, 0, :16] = chain.fk(qg).reshape(B, 16)
    odd = np.arange(B) % 2 == 1
    w["nfields"][odd] = 0
    params = env.abi.default_params(flags=env.abi.F_MIXER, max_vel=0.7, mix_w=[1, 1, 0, 1, 0, 0])
    push = np.where(odd[:, None], 0.05, 0.0) * np.ones((B, chain.n))
    runs = {}
    for stop in (0, 1):
        eng = _engine(env, chain, B, np.float64, params, w)
        eng.set_ext_cmd(3, push)
        eng.set_stall_rule(patience, eps=(1e-4, 1e-3), stop=bool(stop))
        runs[stop] = eng.goto_host(q0, n_cycles, DT, PREC, stride=stride, hold=True, trajectory=True, want=("qdot_out",))
        eng.close()
    a, b = runs[0], runs[1]
    k = patience - 1
    for r in (a, b):
        assert np.all(r["stalled"][odd] == patience * stride - 1) and np.all(r["arrived"][odd] == -1)
        assert np.count_nonzero(r["arrived"][~odd] >= 0) >= 0.9 * np.count_nonzero(~odd)
        done_at = np.maximum(r["arrived"], r["stalled"])
        assert np.array_equal(r["pending"], _own_pending(done_at, np.ones(B, dtype=bool), n_cycles // stride, stride))
    assert np.array_equal(a["stalled"], b["stalled"]) and np.array_equal(a["arrived"], b["arrived"]) and np.array_equal(a["pending"], b["pending"])
    free = a["stalled"] < 0            # (an even arm may creep and stall too: it is no "other arm")
    assert not free[odd].any() and np.count_nonzero(free) >= 0.9 * np.count_nonzero(~odd)
    for key in ("q_traj", "dist_traj"):
        assert np.array_equal(a[key][:, free], b[key][:, free]), key
        assert np.array_equal(a[key][:k + 1, odd], b[key][:k + 1, odd], equal_nan=True), key
    assert np.array_equal(a["qdot_out"][free], b["qdot_out"][free])
    assert np.all(b["q_traj"][k:, odd] == b["q_traj"][k, odd])                                  # stop = 1: they stay
    moved = np.abs(a["q_traj"][-1, odd] - a["q_traj"][k, odd]).min(axis=1)
    assert np.all(moved > 0.5 * 0.05 * DT * (n_cycles - patience * stride))                     # stop = 0: they go on


# ---- 7: early exit ------------------------------------------------------------------------------------------------------------------
def test_early_exit(env):
    """Test 1's scene with a time-out of 4000 cycles and poll = 8: with the rule the call ends at the first poll after the last stall or
    arrival; without it the arms out of reach keep it running to the time-out."""
    c = GOTO[np.dtype(np.float64)]
    chain, w, q0, far, params, ref = _goto_reference(env, np.float64)
    eng = _engine(env, chain, c["B"], np.float64, params, w)
    kw = dict(stride=4, hold=True, clamp=True, poll=8, want=("qdot_out",))
    a = eng.goto_host(q0, 4000, DT, PREC, **kw)
    assert a["checks_run"] == 1000 and "stalled" not in a and a["pending"][-1] == np.count_nonzero(a["arrived"] < 0) >= np.count_nonzero(far)
    eng.reset_state()
    eng.set_stall_rule(c["rule"]["patience"], eps=c["rule"]["eps"], stop=True)
    b = eng.goto_host(q0, 4000, DT, PREC, **kw)
    eng.close()
    done_at = np.maximum(b["arrived"], b["stalled"])
    assert np.all(done_at >= 0)
    last = int((done_at.max() + 1) // 4 - 1)          # the check of the last stall or arrival
    print("checks_run %d with the rule (last stall or arrival at check %d), %d without" % (b["checks_run"], last, a["checks_run"]))
    assert b["checks_run"] == (last + 1 + 7) // 8 * 8 and b["pending"].shape == (b["checks_run"],) and b["pending"][-1] == 0
    assert b["pending"][last] == 0 and (last == 0 or b["pending"][last - 1] > 0)


# ---- 8: the rule switched off again ---------------------------------------------------------------------------------------------------
def test_rule_off_again(env):
    """After set_stall_rule(None) a handle gives what a handle that never had a rule gives, bit for bit, and launches the same kernels."""
    c = GOTO[np.dtype(np.float64)]
    chain, w, q0, far, params, ref = _goto_reference(env, np.float64)
    kw = dict(stride=4, hold=True, clamp=True, trajectory=True, want=("qdot_out", "status"))
    fresh = _engine(env, chain, c["B"], np.float64, params, w)
    fresh.launched_kernels()
    a = fresh.goto_host(q0, 80, DT, PREC, **kw)
    names = fresh.launched_kernels()
    fresh.close()
    eng = _engine(env, chain, c["B"], np.float64, params, w)
    epoch, nbytes = eng.launch_epoch, eng.device_bytes
    eng.set_stall_rule(2, eps=(1e-3, 1e-2), stop=True)
    assert eng.launch_epoch == epoch and eng.device_bytes == nbytes + c["B"] * (16 + 4 + 4)
    s = eng.goto_host(q0, 80, DT, PREC, **kw)
    assert "stalled" in s and np.any(s["stalled"] >= 0)
    eng.set_stall_rule(None)
    eng.reset_state()
    eng.launched_kernels()
    b = eng.goto_host(q0, 80, DT, PREC, **kw)
    assert eng.launched_kernels() == names and names and "stalled" not in b
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    with pytest.raises(env.engine.VfikError):
        eng.stalled()
    eng.close()


# ---- 9: errors, the device-pointer form, the sharded form ------------------------------------------------------------------------------
def test_errors_device_pointer_and_sharded(env):
    import torch
    c = GOTO[np.dtype(np.float64)]
    chain, w, q0, far, params, ref = _goto_reference(env, np.float64)
    B = c["B"]
    eng = _engine(env, chain, B, np.float64, params, w)
    with pytest.raises(env.engine.VfikError):
        eng.stalled()                                   # VFIK_E_STATE: no rule
    out = np.zeros(B, dtype=np.int32)
    assert eng.lib.vfik_stalled_host(eng.h, out.ctypes.data) == -4      # VFIK_E_STATE
    host = np.zeros(B, dtype=np.int32)
    bad = [dict(patience=0), dict(patience=-3), dict(stop=2), dict(stop=-1), dict(eps_pos=-1e-3), dict(eps_rot=float("nan")),
           dict(eps_js=float("inf")), dict(eps_pos=float("inf")), dict(stalled=host.ctypes.data)]
    for kw in bad:
        r = env.abi.StallRule()
        r.patience, r.stop, r.eps_pos, r.eps_rot, r.eps_js = 3, 1, 1e-3, 1e-2, 1e-3
        for k, v in kw.items():
            setattr(r, k, v)
        assert eng.lib.vfik_set_stall_rule(eng.h, C.byref(r)) == -1, kw      # VFIK_E_ARG
        assert eng.lib.vfik_stalled_host(eng.h, out.ctypes.data) == -4       # and no rule was set
    with pytest.raises(ValueError):
        eng.set_stall_rule(3, stalled=torch.zeros(B, dtype=torch.int64, device="cuda:0"))
    # while the handle's stream is being captured both entry points refuse with VFIK_E_STATE and enqueue nothing: the capture goes on, and
    # its replay gives the captured step (tests/test_gpu_pipeline.py captures vfik_step the same way)
    cap = _engine(env, chain, B, np.float64, params, w)
    cap.set_stall_rule(3, eps=(1e-3, 1e-2))             # a rule in force: vfik_stalled_host has no other reason to refuse
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        cap.use_stream(s.cuda_stream)
        q = torch.from_numpy(q0).cuda()
        qd = torch.zeros(B, chain.n, dtype=torch.float64, device="cuda")
        io = cap.make_io(q, qdot_out=qd)
        cap.step(io)
        torch.cuda.synchronize()
        direct = qd.clone()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            cap.step(io)
            r = env.abi.StallRule()
            r.patience, r.stop, r.eps_pos, r.eps_rot, r.eps_js = 4, 1, 1e-3, 1e-2, 1e-3
            rc_set, msg_set = cap.lib.vfik_set_stall_rule(cap.h, C.byref(r)), cap.lib.vfik_last_error()
            rc_get, msg_get = cap.lib.vfik_stalled_host(cap.h, out.ctypes.data), cap.lib.vfik_last_error()
        assert rc_set == -4 and b"captur" in msg_set, (rc_set, msg_set)
        assert rc_get == -4 and b"captur" in msg_get, (rc_get, msg_get)
        qd.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(qd, direct)
        assert np.all(cap.stalled() == -1)                # outside the capture it answers again: no timed move yet
    cap.close()
    # the device-pointer form: the caller's array gets what the handle's own gets, and vfik_stalled_host reads it
    kw = dict(stride=4, hold=True, clamp=True, trajectory=True, want=("qdot_out",))
    rule = c["rule"]
    eng.set_stall_rule(rule["patience"], eps=rule["eps"], stop=True)
    a = eng.goto_host(q0, 240, DT, PREC, **kw)
    eng.reset_state()
    mine = torch.full((B,), 7, dtype=torch.int32, device="cuda:0")
    eng.set_stall_rule(rule["patience"], eps=rule["eps"], stop=True, stalled=mine)
    b = eng.goto_host(q0, 240, DT, PREC, **kw)
    assert np.array_equal(mine.cpu().numpy(), a["stalled"]) and np.any(a["stalled"] >= 0)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    eng.close()
    # the sharded form: two handles of 100 arms give the single engine's result
    sh = env.sharding.ShardedEngine(chain, B, rank=0, world=1, devices=(0, 0), io_dtype=np.float64, max_slots=8, params=params)
    sh.set_fields(w["fields"], w["nfields"])
    sh.set_stall_rule(rule["patience"], eps=rule["eps"], stop=True)
    two = sh.goto_host(q0, 240, DT, PREC, **kw)
    assert np.array_equal(sh.stalled(), a["stalled"])
    sh.set_stall_rule(None)
    off = sh.goto_host(q0, 16, DT, PREC, stride=4)
    sh.close()
    assert "stalled" not in off
    for k in a:
        assert np.array_equal(a[k], two[k]), k
