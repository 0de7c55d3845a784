"""Motion scripts (include/vfik.h: vfik_script / vfik_script_host: set_ref_js, a list of gotoFrame calls, set_ref_js, with the bridge's
controller switched around each change of kind, handlers.py:189-211, 346-387, 481-497, 544-576) on the GPU against their restatement with
the oracle (tests/timed_reference.py: script): which arm reaches which step at which check, the step every check was made against, the joint
path, the distance trace, `diff`, the count of arms under way, scripts of different lengths and shapes, the caller's gate, an arm
without a goal block, the hold, the early exit, the two pure forms against vfik_follow and vfik_follow_js, what the call leaves of
the handle, the kernels it launches, its argument errors, the device form and the sharded form.

Inputs: synth.make_workload(chain, B, 3, seed=53), W = 4, default_rng(21) drawn in the order of tests/test_gpu_follow.py's case:
qg[:, 0] = U(0.6 q_lo, 0.6 q_hi), qg[:, w] = qg[:, w - 1] + 0.12 U(-1, 1), s = U(0.02, 0.12) per arm, the start qg[:, 0] + s U(-1, 1).
Frame steps are chain.fk(qg), posture steps qg.  The kinds of arm b are pattern b % 4 of  P F F P | F P F end | P P F F | F F P P;
arms 7, 17, ... end after their first step, arm 5 has no script.  240 cycles, dt 0.01, clamp on, F_MIXER, max_vel 0.7, jp_kp 8;
Cartesian precision (0.01 m, 0.05 rad) at every step, joint precision 0.004 + 0.002 i at an arm's last step, 3 x that before it.

Margins and tolerances are the project's own (tests/test_gpu_follow.py, tests/test_gpu_follow_js.py): an arm any of whose frame
decisions comes, in the ORACLE's run, within 1e-6 (float32 I/O: 1e-4) of its threshold, or any of whose posture decisions within 1e-7
(4e-6), is left out of the exact comparison of reached, next and way_traj with the oracle -- at most 5 % (15 %) of the arms that take
part, asserted on the oracle's numbers before the GPU's are read; at least 90 % of them finish.  EVERY arm, left out or not, is held
to the state machine replayed with the helper's rules on the GPU's own q_traj and dist_traj rows: reached, next, way_traj and pending
exact, diff bit for bit.

The helper on the CPU (seed 21): lwr 200 arms float64 stride 1: 0 of 199 arms left out, 198 finish, the last step reached at cycle
159; lwr 203 arms float32 stride 4: 24 of 202 left out, 201 finish, last at cycle 167; lwr_dual14 130 arms float64 stride 4: 0 of
129 left out, all finish, last at cycle 187; lwr 70 arms float64 stride 4: 0 of 69 left out, all but arm 42 finish."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import timed_reference as sr  # noqa: E402

pytestmark = pytest.mark.gpu

N_CYCLES, DT, KP, W, PREC = 240, 0.01, 8.0, 4, (0.01, 0.05)
# frame decisions, posture decisions, the share of arms that may be left out
MARGIN = {np.dtype(np.float64): (1e-6, 1e-7, 0.05), np.dtype(np.float32): (1e-4, 4e-6, 0.15)}
TOL = {np.dtype(np.float64): (1e-8, 1e-7), np.dtype(np.float32): (2e-6, 2e-5)}   # q_traj, qdot_out
F, P = sr.FRAME, sr.POSTURE
PATTERNS = np.array([[P, F, F, P], [F, P, F, 0], [P, P, F, F], [F, F, P, P]], dtype=np.int32)
TRACES = ("q", "reached", "next", "pending", "q_traj", "dist_traj", "way_traj", "qdot_out", "status")


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


def _case(env, robot, B, io_dtype=np.float64, kinds=None, no_goal=None):
    """The inputs of the module's docstring; kinds: this kind at every step of every arm instead of the patterns (the ragged ends and the
    arm without a script stay); no_goal: this arm has no field at all."""
    chain = env.robots.by_name(robot)
    n = chain.n
    w = env.synth.make_workload(chain, B, 3, seed=53, io_dtype=io_dtype)
    rng = np.random.default_rng(21)
    qg = np.zeros((B, W, n))
    qg[:, 0] = rng.uniform(0.6 * chain.q_lo, 0.6 * chain.q_hi, size=(B, n))
    for i in range(1, W):
        qg[:, i] = qg[:, i - 1] + 0.12 * rng.uniform(-1.0, 1.0, size=(B, n))
    s = rng.uniform(0.02, 0.12, size=(B, 1))
    q0 = (qg[:, 0] + s * rng.uniform(-1.0, 1.0, size=(B, n))).astype(io_dtype).astype(np.float64)
    way = chain.fk(qg.reshape(B * W, n)).reshape(B, W, 16).astype(io_dtype).astype(np.float64)
    wayq = qg.astype(io_dtype).astype(np.float64)
    kind = PATTERNS[np.arange(B) % 4].copy() if kinds is None else np.full((B, W), kinds, dtype=np.int32)
    kind[7::10, 1:] = 0
    kind[5] = 0
    if no_goal is not None:
        w["nfields"][no_goal] = 0
    return chain, w, q0, kind, way, wayq


def _params(env, **kw):
    kw.setdefault("flags", env.abi.F_MIXER)
    return env.abi.default_params(max_vel=0.7, jp_kp=KP, **kw)


def _reference(env, robot, B, stride, hold, io_dtype=np.float64, gate=False, no_goal=None, n_cycles=N_CYCLES):
    """The oracle's run of a case, computed once per module and never modified."""
    key = (robot, B, stride, hold, np.dtype(io_dtype).name, gate, no_goal, n_cycles)
    if key not in env.cache:
        chain, w, q0, kind, way, wayq = _case(env, robot, B, io_dtype, no_goal=no_goal)
        params = _params(env)
        active = None
        if gate:
            active = np.ones(B, dtype=np.int32)
            active[::3] = 0
        p = _prec(chain.n)
        ref = sr.script(env.oc, chain, params, q0, w["fields"], w["nfields"], kind, way, wayq, n_cycles, stride, DT, PREC, p,
                        js_via_precision=3 * p, hold=hold, clamp=True, active=active, io_dtype=io_dtype, want=("qdot_out",), stepped=chain.n > 7)
        for v in ref.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        env.cache[key] = (chain, w, q0, kind, way, wayq, active, params, ref)
    return env.cache[key]


def _engine(env, chain, B, io_dtype, params, w):
    eng = env.engine.Engine(chain, B, io_dtype=io_dtype, max_slots=8, params=params)
    eng.set_fields(w["fields"], w["nfields"])
    return eng


def _script(eng, q0, kind, way, wayq, stride, hold, n_cycles=N_CYCLES, **kw):
    p = _prec(q0.shape[1])
    q_in = q0.astype(eng.io_dtype)
    keep = q_in.copy()
    got = eng.script_host(q_in, kind, way, wayq, n_cycles, DT, PREC, p, js_via_precision=3 * p, stride=stride, hold=hold, clamp=True,
                          trajectory=True, want=("qdot_out", "status"), **kw)
    assert np.array_equal(q_in, keep)   # io->q is never written
    return got


def _left_out(ref, part, io_dtype):
    """The arms within a margin of a threshold in the oracle's run; the cap and the share that finishes hold on the oracle's numbers alone."""
    mc, mj, cap = MARGIN[np.dtype(io_dtype)]
    out = (ref["closest_c"] < mc) | (ref["closest_j"] < mj)
    n_part = max(np.count_nonzero(part), 1)
    share = np.count_nonzero(out & part) / n_part
    done = part & (ref["next"] == ref["length"])
    fin = ref["reached"][np.arange(len(part)), np.maximum(ref["length"] - 1, 0)]
    print("left out: %d of %d arms (%.1f %%, cap %.0f %%); %d finish, the last step reached at cycle %d"
          % (np.count_nonzero(out & part), n_part, 100 * share, 100 * cap, np.count_nonzero(done), fin[done].max() if done.any() else -1))
    assert share <= cap, share
    return out, done


def _check(got, ref, q0, kind, wayq, stride, hold, io_dtype, active=None, n_checks=None, stuck=None, n_cycles=N_CYCLES):
    """stuck: an arm without a goal block, which never passes a frame step; n_checks: the checks the call is to have run (None: all)."""
    io_dtype = np.dtype(io_dtype)
    B, n = q0.shape
    p = _prec(n)
    n_checks = n_cycles // stride if n_checks is None else n_checks
    L = sr.lengths(kind)
    assert np.array_equal(L, ref["length"]) and set(L) == {0, 1, 3, 4}
    ua = np.ones(B, dtype=bool) if active is None else active != 0
    part = ua & (L > 0)
    out, done = _left_out(ref, part, io_dtype)
    if stuck is None:
        assert np.count_nonzero(done) >= 0.9 * np.count_nonzero(part)
    inc = ~out
    tol_q, tol_v = TOL[io_dtype]
    assert got["checks_run"] == n_checks
    # against the oracle outside the margins
    for k in ("reached", "next"):
        assert np.array_equal(got[k][inc], ref[k][inc]), (k, np.flatnonzero(inc & np.any(np.atleast_2d(got[k].T != ref[k].T), axis=0)))
    assert np.array_equal(got["way_traj"][:, inc], ref["way_traj"][:n_checks, inc])
    # every arm against the state machine on the GPU's own rows
    m = sr.replay(kind, wayq, ref["present"], got["q_traj"], got["dist_traj"], n_cycles, stride, PREC, p, js_via_precision=3 * p, hold=hold,
                  active=active, io_dtype=io_dtype)
    assert np.array_equal(got["reached"], m.reached), np.flatnonzero(np.any(got["reached"] != m.reached, axis=1))
    assert np.array_equal(got["next"], m.next) and np.array_equal(got["way_traj"], m.way_traj) and np.array_equal(got["pending"], m.pending)
    assert got["diff"].dtype == io_dtype and np.array_equal(got["diff"], m.diff), np.flatnonzero(np.any(got["diff"] != m.diff, axis=1))
    posture_checked = np.any((m.way_traj >= 0) & (kind[np.arange(B)[None, :], np.maximum(m.way_traj, 0)] == P), axis=0)
    assert np.all(got["diff"][~posture_checked] == 0) and np.any(got["diff"][posture_checked] != 0)   # a row is kept where no posture check was made
    rows = inc   # (an arm that advances at another check than the oracle's goes another way from there, with or without hold)
    eq = np.abs(got["q_traj"][:, rows].astype(np.float64) - ref["q_traj"][:n_checks, rows]).max()
    print("q_traj max error %.3e (tolerance %.1e)" % (eq, tol_q))
    assert eq < tol_q
    assert np.array_equal(got["q"], got["q_traj"][-1])
    # arms that take no part: their rows carry their start, nothing is stored for them
    assert np.all(got["q_traj"][:, ~part] == q0[~part].astype(io_dtype)) and np.all(got["way_traj"][:, ~part] == -1)
    assert np.all(got["reached"][~part] == -1) and np.all(got["next"][~part] == 0)
    assert np.all(got["status"][~part] == 0) and np.all(got["qdot_out"][~part] == 0) and np.all(got["diff"][~part] == 0)
    if stuck is not None:
        first_frame = int(np.argmax(kind[stuck] == F))
        assert got["next"][stuck] == first_frame and np.all(got["reached"][stuck, first_frame:] == -1) and got["pending"][-1] >= 1
    if hold:   # an arm at its last step repeats its rows, bit for bit
        fin = got["reached"][np.arange(B), np.maximum(L - 1, 0)]
        for b in np.flatnonzero(part & (got["next"] == L)):
            k = (fin[b] + 1) // stride - 1
            assert np.all(got["q_traj"][k:, b] == got["q_traj"][k, b]) and np.all(got["dist_traj"][k:, b] == got["dist_traj"][k, b]), b
            assert np.all(got["way_traj"][k:, b] == L[b] - 1), b
    if n_checks == n_cycles // stride:
        ev = np.abs(got["qdot_out"][rows].astype(np.float64) - ref["qdot_out"][rows]).max()
        print("qdot_out max error %.3e (tolerance %.1e)" % (ev, tol_v))
        assert ev < tol_v
    return inc


@pytest.mark.parametrize("robot,B,stride,hold,io_dtype", [("lwr", 200, 1, False, np.float64), ("lwr", 203, 4, True, np.float32),
                                                          ("lwr_dual14", 130, 4, True, np.float64)])
def test_script(env, robot, B, stride, hold, io_dtype):
    """lwr float64 with a check after every cycle; lwr float32 with 203 arms (rows that are not 16-byte aligned), stride 4 and hold;
    lwr_dual14 (stepped blocks) with stride 4 and hold."""
    chain, w, q0, kind, way, wayq, active, params, ref = _reference(env, robot, B, stride, hold, io_dtype)
    eng = _engine(env, chain, B, io_dtype, params, w)
    got = _script(eng, q0, kind, way, wayq, stride, hold)
    _check(got, ref, q0, kind, wayq, stride, hold, io_dtype)
    eng.close()


def test_frames_only_equals_follow(env):
    """A script of frames only, under the reference's cartesian bottle [1, 1, 0, 0], is vfik_follow on a handle whose mixer holds those
    weights, bit for bit: 70 arms, one full wave and a partial one."""
    B = 70
    chain, w, q0, kind, way, wayq = _case(env, "lwr", B, kinds=F)
    params = _params(env, mix_w=[1, 1, 0, 0, 0, 0])
    eng = _engine(env, chain, B, np.float64, params, w)
    way_nan = way.copy()
    way_nan[kind == 0] = np.nan
    kw = dict(stride=4, hold=True, clamp=True, trajectory=True, want=("qdot_out", "status"))
    a = eng.follow_host(q0, way_nan, N_CYCLES, DT, PREC, **kw)
    eng.reset_state()
    b = _script(eng, q0, kind, way, wayq, 4, True)
    assert np.count_nonzero(a["next"] == 4) >= 55 and a["checks_run"] == b["checks_run"]
    for k in TRACES:
        assert np.array_equal(a[k], b[k]), k
    assert np.all(b["diff"] == 0)
    eng.close()


def test_postures_only_equals_follow_js(env):
    """A script of postures only, under the joint bottle [0, 0, 1, 0], is vfik_follow_js on a handle whose mixer holds those weights."""
    B = 70
    chain, w, q0, kind, way, wayq = _case(env, "lwr", B, kinds=P)
    params = _params(env, mix_w=[0, 0, 1, 0, 0, 0])
    eng = _engine(env, chain, B, np.float64, params, w)
    wayq_nan = wayq.copy()
    wayq_nan[kind == 0] = np.nan
    p = _prec(7)
    a = eng.follow_js_host(q0, wayq_nan, N_CYCLES, DT, p, via_precision=3 * p, stride=4, hold=True, clamp=True, trajectory=True,
                           want=("qdot_out", "status"))
    b = _script(eng, q0, kind, way, wayq, 4, True)
    assert np.count_nonzero(a["next"] == 4) >= 55 and a["checks_run"] == b["checks_run"]
    for k in ("q", "reached", "next", "pending", "q_traj", "way_traj", "diff", "qdot_out", "status"):
        assert np.array_equal(a[k], b[k]), k
    eng.close()


def test_gate_and_missing_goal(env):
    """The caller gates every third arm: never run, nowhere reached, not counted.  Arm 1 (F P F end) has no field at all: it runs, stays
    at its first frame step and stays counted; nothing is written where its goal block would be."""
    B = 70
    chain, w, q0, kind, way, wayq, active, params, ref = _reference(env, "lwr", B, 4, True, gate=True, no_goal=1)
    eng = _engine(env, chain, B, np.float64, params, w)
    got = _script(eng, q0, kind, way, wayq, 4, True, active=active)
    _check(got, ref, q0, kind, wayq, 4, True, np.float64, active=active, stuck=1)
    assert np.all(got["reached"][::3] == -1) and got["pending"][0] <= np.count_nonzero(active)
    out = eng.step_host(q0, want=("qdot_out",))
    assert np.all(out["qdot_out"][1] == 0)        # still no goal: zero command
    eng.close()


def test_early_exit(env):
    """A run of 4000 cycles that polls every 8 checks ends a poll after the last arm is at its last step, and gives what the un-polled
    run of as many checks gives, bit for bit.  Under the caller's gate, which here keeps out the one arm that does not finish (arm 42):
    an early end comes only once no arm that takes part is under way."""
    B = 70
    chain, w, q0, kind, way, wayq, active, params, ref = _reference(env, "lwr", B, 4, True, gate=True)
    L = ref["length"]
    part = (L > 0) & (active != 0)
    out, done = _left_out(ref, part, np.float64)
    assert np.array_equal(done, part)
    last = int((ref["reached"][np.arange(B), np.maximum(L - 1, 0)][part].max() + 1) // 4 - 1)
    bound = (last + 8 + 7) // 8 * 8 + (8 if out.any() else 0)
    eng = _engine(env, chain, B, np.float64, params, w)
    a = _script(eng, q0, kind, way, wayq, 4, True, n_cycles=4000, poll=8, active=active)
    print("checks_run %d (oracle's last arrival at check %d, bound %d)" % (a["checks_run"], last, bound))
    assert 0 < a["checks_run"] <= bound and a["checks_run"] % 8 == 0
    assert a["pending"].shape == (a["checks_run"],) and a["pending"][-1] == 0 and np.array_equal(a["next"], np.where(part, L, 0))
    assert a["q_traj"].shape[0] == a["checks_run"] == a["dist_traj"].shape[0] == a["way_traj"].shape[0]
    eng.reset_state()
    # (the goal blocks hold the last frames sent now, and an arm that starts with a posture is measured against its goal as it stands)
    eng.set_fields(w["fields"], w["nfields"])
    b = _script(eng, q0, kind, way, wayq, 4, True, n_cycles=a["checks_run"] * 4, active=active)
    for k in TRACES + ("diff",):
        assert np.array_equal(a[k], b[k]), k
    eng.close()


def _goal_left(w, kind, way, got):
    """The field array with every arm's goal as the script left it: the last frame it was sent (rows 0..2), for arms with a goal block"""
    fields = np.array(w["fields"], copy=True)
    L = sr.lengths(kind)
    slot = sr.goal_slot(fields, w["nfields"])
    for b in range(kind.shape[0]):
        sent = [i for i in range(min(got["next"][b], L[b] - 1) + 1) if kind[b, i] == F] if L[b] > 0 else []
        if sent and slot[b] >= 0:
            fields["p"][b, slot[b], :12] = way[b, sent[-1], :12]
    return fields


@pytest.mark.parametrize("per_arm", [False, True])
def test_the_handle_is_left_as_it_was(env, per_arm):
    """Across a script the launch epoch does not move and a step afterwards equals the same step on a fresh handle that was given the
    goals the script left, bit for bit -- with the batch-wide bridge state, and with per-arm mixer weights and two different per-arm
    limiter speeds under F_LIMITER set beforehand.  There the script's arms were limited by their OWN max_vel: the oracle's run with
    those speeds, and no cycle of an arm faster than its speed allows while the slow arms do run into it."""
    B = 70
    abi = env.abi
    chain, w, q0, kind, way, wayq = _case(env, "lwr", B)
    params = _params(env, flags=abi.F_MIXER | (abi.F_LIMITER if per_arm else 0))
    rng = np.random.default_rng(5)
    mixw = np.tile([1.0, 1.0, 0.0, 0.0, 0.0, 0.0], (B, 1))
    mixw[:, :2] = rng.uniform(0.5, 1.0, (B, 2))
    max_vel = np.where(np.arange(B) % 2 == 0, 0.05, 0.7)

    def handle(fields):
        eng = env.engine.Engine(chain, B, io_dtype=np.float64, max_slots=8, params=params)
        eng.set_fields(fields, w["nfields"])
        if per_arm:
            eng.set_mixer_weights(mixw)
            eng.set_max_vel(max_vel)
        return eng
    eng = handle(w["fields"])
    own_ref = rng.uniform(0.5 * chain.q_lo, 0.5 * chain.q_hi, q0.shape)
    want = ("qdot_out", "goal_dist", "status")
    epoch, path, slots = eng.launch_epoch, eng.field_path, eng.slots_in_use
    got = _script(eng, q0, kind, way, wayq, 1, False)
    assert got["next"].sum() > B
    assert (eng.launch_epoch, eng.field_path, eng.slots_in_use) == (epoch, path, slots)
    after = eng.step_host(q0, want=want)
    after_ref = eng.step_host(q0, q_ref=own_ref, want=want + ("q_ref_out",))
    eng.close()
    fresh = handle(_goal_left(w, kind, way, got))
    first = fresh.step_host(q0, want=want)
    first_ref = fresh.step_host(q0, q_ref=own_ref, want=want + ("q_ref_out",))
    fresh.close()
    for k in want:
        assert np.array_equal(after[k], first[k]), k
        assert np.array_equal(after_ref[k], first_ref[k]), k
    assert np.array_equal(after_ref["q_ref_out"], first_ref["q_ref_out"])
    if per_arm:
        p = _prec(7)
        ref = sr.script(env.oc, chain, params, q0, w["fields"], w["nfields"], kind, way, wayq, N_CYCLES, 1, DT, PREC, p, js_via_precision=3 * p,
                        hold=False, clamp=True, want=("qdot_out",), bridge_arm=np.column_stack([mixw[:, 4], mixw[:, 5], max_vel]))
        part = ref["length"] > 0
        out, _ = _left_out(ref, part, np.float64)
        inc = ~out
        assert np.array_equal(got["reached"][inc], ref["reached"][inc])
        eq = np.abs(got["q_traj"][:, inc] - ref["q_traj"][:, inc]).max()
        print("q_traj max error against the oracle with per-arm limiter speeds %.3e" % eq)
        assert eq < TOL[np.dtype(np.float64)][0]
        speed = np.abs(np.diff(np.concatenate([q0[None], got["q_traj"]]), axis=0)).max(axis=(0, 2)) / DT    # stride 1: every cycle's
        assert np.all(speed[part] <= max_vel[part] * (1 + 1e-9))
        slow = part & (max_vel < 0.1)
        assert np.all(speed[slow] >= 0.05 * (1 - 1e-9)) and np.any(speed[part & ~slow] > 0.05)
        assert np.all(got["status"][slow] & abi.ST_LIMITED)


def test_only_a_rollouts_kernels(env):
    """A script lists the cycle kernels a rollout with q_ref under a gate lists on the same handle once it has per-arm mixer rows."""
    import kernel_variants as kv
    for robot in ("lwr", "lwr_dual14"):
        B = 70
        chain, w, q0, kind, way, wayq = _case(env, robot, B)
        eng = _engine(env, chain, B, np.float64, _params(env), w)
        eng.launched_kernels()
        got = _script(eng, q0, kind, way, wayq, 4, True, n_cycles=16)
        assert got["checks_run"] == 4
        of_script = eng.launched_kernels()
        mixw = np.tile([1.0, 1.0, 0.0, 0.0, 0.0, 0.0], (B, 1))
        mixw[::2, 0] = 0.5
        eng.set_mixer_weights(mixw)
        eng.rollout_host(q0, 4, DT, clamp=True, want=("qdot_out", "status", "goal_dist"), q_ref=wayq[:, 0], active=np.ones(B, dtype=np.int32))
        of_rollout = eng.launched_kernels()
        built = {v.name for v in kv.library_variants()}
        assert of_script and of_script == of_rollout, (of_script, of_rollout)
        for nm in of_script:
            assert kv.parse(nm).kernel.startswith("cycle_") and nm in built, nm
        eng.close()


def test_argument_errors_and_device_form(env):
    """What vfik_script refuses, with nothing enqueued; then Engine.script on torch tensors equals the host form."""
    import torch
    chain, w, q0, kind, way, wayq, active, params, ref = _reference(env, "lwr", 70, 4, True)
    B, n = q0.shape
    eng = _engine(env, chain, B, np.float64, params, w)
    reached = np.full((B, W), 77, dtype=np.int32)
    nxt = np.full(B, 77, dtype=np.int32)
    good = _prec(n)
    dummy = np.zeros((B, 16))
    assert way.ctypes.data % 16 == 0
    nan, inf = float("nan"), float("inf")

    def call(prec=good, via=None, null_opts=False, mix_frame=(1, 1, 0, 0), mix_posture=(0, 0, 1, 0), handle=None, **kw):
        io = env.engine.IO()
        io.q = q0.ctypes.data
        o = env.abi.ScriptOpts()
        o.n_cycles, o.stride, o.dt, o.n_way = 16, 4, DT, W
        o.pos_prec, o.rot_prec, o.via_pos_prec, o.via_rot_prec = PREC[0], PREC[1], PREC[0], PREC[1]
        o.kind, o.way16, o.wayq, o.reached, o.next = kind.ctypes.data, way.ctypes.data, wayq.ctypes.data, reached.ctypes.data, nxt.ctypes.data
        keep = [None if a is None else np.ascontiguousarray(a, dtype=np.float64) for a in (prec, via)]
        o.prec, o.via_prec = (None if a is None else a.ctypes.data for a in keep)
        for i in range(4):
            o.mix_frame[i], o.mix_posture[i] = mix_frame[i], mix_posture[i]
        for k, v in kw.items():
            setattr(io if hasattr(io, k) else o, k, v)
        h = eng if handle is None else handle
        return h.lib.vfik_script_host(h.h, C.byref(io), None if null_opts else C.byref(o), 0, None)

    def with_prec(i, v):
        p = good.copy()
        p[i] = v
        return p

    epoch = eng.launch_epoch
    bad = [dict(null_opts=True), dict(kind=None), dict(way16=None), dict(wayq=None), dict(reached=None), dict(next=None), dict(n_way=0),
           dict(n_way=-3), dict(way16=way.ctypes.data + 8), dict(wayq=wayq.ctypes.data + 4), dict(mix_frame=(1, nan, 0, 0)),
           dict(mix_frame=(inf, 1, 0, 0)), dict(mix_posture=(0, 0, nan, 0)), dict(mix_posture=(0, 0, 1, -inf)), dict(pos_prec=-1e-3),
           dict(rot_prec=nan), dict(via_pos_prec=nan), dict(via_rot_prec=-1e-3), dict(prec=None), dict(prec=with_prec(1, -1.0)),
           dict(prec=with_prec(6, nan)), dict(via=with_prec(0, -1.0)), dict(via=with_prec(2, nan)), dict(q_ref=q0.ctypes.data),
           dict(stride=0), dict(stride=-4), dict(n_cycles=0), dict(n_cycles=1000004), dict(n_cycles=10), dict(dt=nan), dict(dt=inf),
           dict(q_cmded=dummy.ctypes.data), dict(track_error=dummy.ctypes.data), dict(obj_dist=dummy.ctypes.data)]
    for kw in bad:
        rc = call(**kw)
        assert rc == -1, (kw, rc, eng.lib.vfik_last_error())   # VFIK_E_ARG
        with pytest.raises(env.engine.VfikError):
            eng._chk(rc)
    # a handle without the mixer: a script has nothing to switch controllers with
    plain = _engine(env, chain, B, np.float64, _params(env, flags=0), w)
    assert call(handle=plain) == -4, plain.lib.vfik_last_error()   # VFIK_E_STATE
    plain.close()
    eng.sync()
    assert eng.launch_epoch == epoch and np.all(reached == 77) and np.all(nxt == 77)
    with pytest.raises(ValueError):
        eng.script_host(q0, kind[:, :3], way, wayq, 16, DT, PREC, good)
    with pytest.raises(ValueError):
        eng.script_host(q0, kind, way, wayq, 16, DT, PREC, good, mix_frame=(1, 1, 0))
    assert call() == 0 and np.all(nxt <= W) and nxt[5] == 0 and np.all(reached < 16)
    p = good
    eng.set_fields(w["fields"], w["nfields"])   # (a script leaves the last frames sent in the goal blocks, which the next one's distances see)
    host = eng.script_host(q0, kind, way, wayq, 96, DT, PREC, p, js_via_precision=3 * p, stride=4, hold=True, clamp=True, trajectory=True,
                           want=("qdot_out",))
    dev = torch.device("cuda", 0)
    f64 = dict(dtype=torch.float64, device=dev)
    q = torch.from_numpy(q0).to(dev)
    t = dict(reached=torch.full((B, W), 7, dtype=torch.int32, device=dev), next=torch.full((B,), 7, dtype=torch.int32, device=dev),
             pending=torch.full((24,), 7, dtype=torch.int32, device=dev), q_out=torch.zeros(B, n, **f64), q_traj=torch.zeros(24, B, n, **f64),
             dist_traj=torch.zeros(24, B, 2, **f64), diff=torch.zeros(B, n, **f64), way_traj=torch.full((24, B), -1, dtype=torch.int32, device=dev))
    qd = torch.zeros(B, n, **f64)
    kt, wt, wqt = torch.from_numpy(kind).to(dev), torch.from_numpy(way).to(dev), torch.from_numpy(wayq).to(dev)
    eng.set_fields(w["fields"], w["nfields"])
    torch.cuda.synchronize()
    eng.script(eng.make_io(q, qdot_out=qd), kt, wt, wqt, 96, DT, PREC, p, js_via_precision=3 * p, stride=4, hold=True, clamp=True, **t)
    eng.sync()
    assert host["next"].sum() > B
    for k, hk in (("reached", "reached"), ("next", "next"), ("pending", "pending"), ("q_out", "q"), ("q_traj", "q_traj"),
                  ("dist_traj", "dist_traj"), ("diff", "diff"), ("way_traj", "way_traj")):
        assert np.array_equal(t[k].cpu().numpy(), host[hk]), k
    assert np.array_equal(qd.cpu().numpy(), host["qdot_out"]) and np.array_equal(q.cpu().numpy(), q0)
    eng.close()


def test_sharded_script_equals_single_engine(env):
    """ShardedEngine over devices (0, 0): two handles, 35 arms each, give the single engine's result on the whole batch."""
    chain, w, q0, kind, way, wayq, active, params, ref = _reference(env, "lwr", 70, 4, True)
    eng = _engine(env, chain, 70, np.float64, params, w)
    one = _script(eng, q0, kind, way, wayq, 4, True)
    eng.close()
    sh = env.sharding.ShardedEngine(chain, 70, rank=0, world=1, devices=(0, 0), io_dtype=np.float64, max_slots=8, params=params)
    sh.set_fields(w["fields"], w["nfields"])
    p = _prec(7)
    two = sh.script_host(q0, kind, way, wayq, N_CYCLES, DT, PREC, p, js_via_precision=3 * p, stride=4, hold=True, clamp=True, trajectory=True,
                         want=("qdot_out", "status"))
    sh.close()
    assert two["checks_run"] == one["checks_run"]
    for k in TRACES + ("diff",):
        assert np.array_equal(one[k], two[k]), k
