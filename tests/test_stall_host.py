"""CPU-side checks of the stall rule of the timed moves (include/vfik.h: vfik_set_stall_rule): the rule struct and its ctypes mirror, the
exported symbols, the Python methods, and the host restatement (tests/timed_reference.py) -- the rule on hand-made traces, and the
oracle-stepped loop with a rule against the same move without one, which it must reproduce bit for bit while the patience is larger
than the number of checks; a goto against a script of one frame step, a joint-space goto against one of one posture step."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from vfclik_amd import engine
    return engine.load_library()


def test_stall_rule_size_matches_the_mirror(lib):
    from vfclik_amd import _abi
    r = _abi.StallRule
    assert lib.vfik_stall_rule_size() == ctypes.sizeof(r) == 4 + 4 + 3 * 8 + 8
    assert (r.patience.offset, r.stop.offset, r.eps_pos.offset, r.eps_rot.offset, r.eps_js.offset, r.stalled.offset) == (0, 4, 8, 16, 24, 32)
    assert lib.vfik_abi_version() == 6 == _abi.ABI_VERSION   # entry points only


def test_stall_symbols_are_declared_and_exported(lib):
    hdr = open(os.path.join(ROOT, "include", "vfik.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    raw = ctypes.CDLL(os.path.join(ROOT, "vfclik_amd", "csrc", "libvfik_hip.so"))
    for name in ("vfik_stall_rule_size", "vfik_set_stall_rule", "vfik_stalled_host"):
        assert re.search(r"\b%s\s*\(" % name, code), name + " is not declared in include/vfik.h"
        assert hasattr(raw, name), "libvfik_hip.so does not export " + name
    assert "typedef struct vfik_stall_rule" in code


def test_engine_and_sharded_engine_have_the_methods(lib):
    from vfclik_amd import engine, sharding
    for cls in (engine.Engine, sharding.ShardedEngine):
        assert callable(cls.set_stall_rule) and callable(cls.stalled)


# ---- the rule on hand-made traces.  eps = (1/8, 1/4) and measures that are sums of powers of two: best - eps is exact ----
def _state(B, patience):
    import timed_reference as st
    return st.StallState(B, st.Rule(patience, eps=(0.125, 0.25), eps_js=0.125))


def test_progress_in_either_component_resets_count():
    s = _state(1, 3)
    sel, cart = np.array([True]), np.array([False])

    def step(d, a, cycle=0):
        return bool(s.step(sel, cart, np.array([d]), np.array([a]), cycle)[0])
    assert not step(1.0, 1.0) and s.count[0] == 0 and list(s.best[0]) == [1.0, 1.0]     # against best = +inf: progress
    assert not step(0.9, 0.8) and s.count[0] == 1 and list(s.best[0]) == [1.0, 1.0]     # neither gains its eps: best stays
    assert not step(0.9, 0.8) and s.count[0] == 2
    assert not step(1.5, 0.5) and s.count[0] == 0 and list(s.best[0]) == [1.0, 0.5]     # the angle alone: componentwise minimum
    assert not step(0.75, 2.0) and s.count[0] == 0 and list(s.best[0]) == [0.75, 0.5]   # the distance alone
    assert s.stalled[0] == -1


def test_equality_is_not_progress_and_the_stall_lands_at_the_patience_th_miss():
    s = _state(1, 3)
    sel, cart = np.array([True]), np.array([False])
    s.step(sel, cart, np.array([1.0]), np.array([1.0]), 3)
    assert not s.step(sel, cart, np.array([0.875]), np.array([0.75]), 7)[0] and s.count[0] == 1   # m == best - eps, both: a miss
    assert s.closest[0] == 0.0
    assert not s.step(sel, cart, np.array([0.875]), np.array([0.75]), 11)[0] and s.count[0] == 2
    assert s.stalled[0] == -1
    assert s.step(sel, cart, np.array([0.875]), np.array([0.75]), 15)[0] and s.stalled[0] == 15 and s.count[0] == 3
    t = _state(1, 3)
    t.step(sel, cart, np.array([1.0]), np.array([1.0]), 3)
    assert not t.step(sel, cart, np.array([0.875 - 2.0 ** -50]), np.array([0.75]), 7)[0] and t.count[0] == 0   # one bit under: progress


def test_nan_is_never_progress_and_the_joint_measure():
    import timed_reference as st
    s = _state(2, 2)
    sel = np.array([True, True])
    nan = np.nan
    assert list(s.step(sel, np.array([False, True]), np.array([nan, nan]), np.array([nan, 0.0]), 3)) == [False, False]
    assert list(s.step(sel, np.array([False, True]), np.array([nan, nan]), np.array([nan, 0.0]), 7)) == [True, True]   # check patience - 1
    assert list(s.stalled) == [7, 7] and np.all(np.isinf(s.best))
    inf = np.inf
    ref = np.array([[1.0, 2.0, 3.0]] * 4)
    q = np.array([[0.5, 2.25, 3.0], [0.5, 2.25, 3.0], [nan, 2.0, 3.0], [nan, 2.0, 3.0]])
    prec = np.array([[0.1, 0.1, 0.1], [inf, 0.1, 0.1], [0.1, 0.1, 0.1], [inf, inf, inf]])
    e = st.joint_measure(ref, q, prec)
    assert e[0] == 0.5 and e[1] == 0.25 and np.isnan(e[2]) and e[3] == 0.0   # all joints; finite precisions only; NaN stays; none: 0


STRIDE = 4


def _frames_machine(dist, patience, n_way=2, present=None, stop=True, hold=True):
    """replay of a frames-only script on hand-made distance rows dist (checks, B) in metres, angle 0 (NaN beside a NaN distance)"""
    import timed_reference as st
    n_checks, B = dist.shape
    kind = np.full((B, n_way), st.FRAME, dtype=np.int32)
    d2 = np.stack([dist, np.where(np.isnan(dist), np.nan, 0.0)], axis=2)
    present = np.ones(B, dtype=bool) if present is None else present
    return st.replay(kind, np.zeros((B, n_way, 2)), present, np.zeros((n_checks, B, 2)), d2, n_checks * STRIDE, STRIDE, (0.01, 0.05),
                     np.zeros(2), hold=hold, rule=st.Rule(patience, eps=(0.125, 0.25), stop=stop))


def test_machine_arrival_first_advance_resets_nan_rows_and_pending():
    """Arm 0: a miss, then it ARRIVES at the check where its count would reach 2; its second step starts from a reset state (1.0 is
    progress again, then two misses: stalled at check 5 -- without the reset it would stall at check 3).  Arm 1: NaN rows.  Arm 2: no
    goal block.  Arm 3 halves its distance: 1/8 == 1/4 - eps is one miss, the next check is progress again, and it arrives at both steps."""
    nan = np.nan
    dist = np.array([[1.0, 1.0, 0.005, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0],
                     [nan] * 10,
                     [0.5 ** i for i in range(10)],
                     [1.0, 0.5, 0.25, 0.125, 0.0625, 0.005, 1.0, 0.005, 1.0, 1.0]]).T
    m = _frames_machine(dist, 2, present=np.array([True, True, False, True]))

    def cyc(k):
        return (k + 1) * STRIDE - 1
    assert list(m.reached[0]) == [cyc(2), -1] and m.next[0] == 1 and m.stalled[0] == cyc(5)
    assert m.stalled[1] == cyc(1) == 2 * STRIDE - 1 and m.stalled[2] == cyc(1) and m.next[1] == 0 and m.next[2] == 0
    assert m.stalled[3] == -1 and list(m.reached[3]) == [cyc(5), cyc(7)]
    #                  check:   0  1  2  3  4  5  6  7  8  9
    assert list(m.pending) == [4, 2, 2, 2, 2, 1, 1, 0, 0, 0]
    assert list(m.way_traj[:, 0]) == [0, 0, 0, 1, 1, 1, 1, 1, 1, 1] and list(m.way_traj[:, 1]) == [0] * 10   # stopped: rows repeat
    assert not m.gate.any()


def test_machine_stop_off_keeps_the_arm_running_unchecked():
    """stop = 0: the stalled arm stays in the gate, leaves pending and is never checked again -- a distance under the precision later
    does not make it arrive."""
    dist = np.array([[1.0, 1.0, 1.0, 0.001, 0.001]]).T
    m = _frames_machine(dist, 2, n_way=1, stop=False)
    assert m.stalled[0] == 3 * STRIDE - 1 and m.reached[0, 0] == -1 and m.gate[0] and list(m.pending) == [1, 1, 0, 0, 0]
    m = _frames_machine(dist, 3, n_way=1, stop=False)
    assert m.stalled[0] == -1 and m.reached[0, 0] == 4 * STRIDE - 1          # arrival at the check where count would reach 3


def test_machine_posture_steps():
    """The joint rule.  Arm 0's reference starts with NaN; arm 1 creeps by 1/16 per check under eps_js = 1/8; arm 2's first joint is
    far off and never moves, its second gains 1/2 per check."""
    import timed_reference as st
    nan, inf = np.nan, np.inf
    n_checks = 8
    wayq = np.array([[[nan, 0.0]], [[0.0, 0.0]], [[0.0, 0.0]]])
    q = np.zeros((n_checks, 3, 2))
    q[:, 1, 0] = 4.0 - np.arange(n_checks) / 16.0
    q[:, 2, 0] = 9.0
    q[:, 2, 1] = 4.0 - np.arange(n_checks) / 2.0
    kind = np.full((3, 1), st.POSTURE, dtype=np.int32)

    def run(patience, prec):
        return st.replay(kind, wayq, np.ones(3, dtype=bool), q, None, n_checks * STRIDE, STRIDE, (0.0, 0.0), np.asarray(prec), hold=True,
                         rule=st.Rule(patience, eps_js=0.125))
    # joint 0 has no finite precision: it neither decides nor counts.  Arm 0: e = 0 at every check, progress against +inf once, then three
    # misses; its NaN never passes the arrival rule.  Arm 1 arrives at once.  Arm 2: e = 4 - k / 2, progress at every check.
    m = run(3, [inf, 0.25])
    assert list(m.stalled) == [4 * STRIDE - 1, -1, -1] and list(m.reached[:, 0]) == [-1, STRIDE - 1, -1] and list(m.pending[-2:]) == [1, 1]
    # Arm 0: e is NaN, stalled at check patience - 1.  Arm 1: 4, 63/16 (miss), 62/16 == 4 - 1/8 (equality: miss 2).  Arm 2: e = 9, 9, 9.
    m = run(2, [0.25, 0.25])
    assert list(m.stalled) == [2 * STRIDE - 1, 3 * STRIDE - 1, 3 * STRIDE - 1] and list(m.pending) == [3, 2, 0, 0, 0, 0, 0, 0]
    # patience 3: arm 1's fourth value 61/16 is under 4 - 1/8 (a miss moves no best): progress, and so on -- it never stalls
    m = run(3, [0.25, 0.25])
    assert list(m.stalled) == [3 * STRIDE - 1, -1, 4 * STRIDE - 1]


# ---- the oracle-stepped loop: with a patience above n_checks it is the move without a rule, bit for bit ----
N_CYCLES, DT, PREC = 160, 0.01, (0.01, 0.05)
JS_PREC = 0.01 * np.ones(7)


def _same(a, b, keys):
    for k in keys:
        assert np.array_equal(a[k], b[k], equal_nan=True), k


def _never():
    import timed_reference as st
    return st.Rule(N_CYCLES // STRIDE + 1, eps=(1e-3, 1e-2), eps_js=1e-3)


def test_patient_rule_is_goto_reference(lib):
    """goto with a patient rule = goto without one = a script of one frame step -- the arm's own goal, sent, under the handle's weights
    as the call's quad"""
    import timed_reference as st
    from oracle import oracle_c
    from vfclik_amd import _abi
    chain, w, qg, way, q0, params = st.three_lwr_arms(_abi.F_NULLSPACE | _abi.F_MIXER | _abi.F_LIMITER)
    w["fields"]["p"][:, 0, :16] = way[:, 1]          # the goal: one step of 0.1 rad per joint away
    w["nfields"][2] = 0                              # arm 2: no goal block
    kw = dict(hold=True, clamp=True, active=[1, 1, 1], want=("qdot_out",))
    a = st.goto(oracle_c, chain, params, q0, w["fields"], w["nfields"], N_CYCLES, STRIDE, DT, PREC, **kw)
    b = st.goto(oracle_c, chain, params, q0, w["fields"], w["nfields"], N_CYCLES, STRIDE, DT, PREC, rule=_never(), **kw)
    assert np.all(a["arrived"][:2] >= 0) and a["arrived"][2] == -1
    _same(a, b, ("arrived", "pending", "q_traj", "dist_traj", "q", "qdot_out", "status"))
    assert np.array_equal(a["closest"], b["closest_c"]) and np.all(b["stalled"] == -1)
    goal = np.where((w["nfields"] > 0)[:, None], w["fields"]["p"][:, 0, :16], 0.0)
    c = st.script(oracle_c, chain, params, q0, w["fields"], w["nfields"], np.full((3, 1), st.FRAME, dtype=np.int32), goal[:, None, :],
                  np.zeros((3, 1, 7)), N_CYCLES, STRIDE, DT, PREC, np.zeros(7), mix_frame=list(params.mix_w)[:4], **kw)
    c["arrived"] = c["reached"][:, 0]
    _same(b, c, ("arrived", "pending", "q_traj", "dist_traj", "q", "qdot_out", "status"))
    # and with patience 3 the arm without a goal block stalls at check 2, stops there, and the others are untouched
    d = st.goto(oracle_c, chain, params, q0, w["fields"], w["nfields"], N_CYCLES, STRIDE, DT, PREC, rule=st.Rule(3, eps=(1e-3, 1e-2)), **kw)
    assert list(d["stalled"]) == [-1, -1, 3 * STRIDE - 1] and np.array_equal(d["arrived"], a["arrived"])
    assert np.array_equal(d["q_traj"][:, :2], a["q_traj"][:, :2]) and np.all(d["q_traj"][2:, 2] == a["q_traj"][2, 2])
    assert np.array_equal(d["pending"], a["pending"] - (np.arange(N_CYCLES // STRIDE) >= 2))


def test_patient_rule_is_goto_js_reference(lib):
    """goto_js with a patient rule = goto_js without one = a script of one posture step under the handle's weights as the call's quad"""
    import timed_reference as st
    from oracle import oracle_c
    from vfclik_amd import _abi
    chain, w, qg, way, q0, params = st.three_lwr_arms(_abi.F_MIXER, mix_w=[0, 0, 1, 0, 0, 0], jp_kp=8.0)
    q_ref = qg[:, 0].copy()
    q_ref[2, 0] = np.nan                             # arm 2: no controller
    kw = dict(hold=True, clamp=True, want=("qdot_out",))
    a = st.goto_js(oracle_c, chain, params, q0, w["fields"], w["nfields"], q_ref, N_CYCLES, STRIDE, DT, JS_PREC, **kw)
    b = st.goto_js(oracle_c, chain, params, q0, w["fields"], w["nfields"], q_ref, N_CYCLES, STRIDE, DT, JS_PREC, rule=_never(), **kw)
    assert np.all(a["arrived"][:2] >= 0) and a["arrived"][2] == -1
    _same(a, b, ("arrived", "pending", "q_traj", "q", "diff", "qdot_out", "status"))
    assert np.array_equal(a["closest"], b["closest_j"]) and np.all(b["stalled"] == -1)
    c = st.script(oracle_c, chain, params, q0, w["fields"], w["nfields"], np.full((3, 1), st.POSTURE, dtype=np.int32), np.zeros((3, 1, 16)),
                  q_ref[:, None, :], N_CYCLES, STRIDE, DT, (0.0, 0.0), JS_PREC, mix_posture=list(params.mix_w)[:4], **kw)
    _same(b, c, ("reached", "pending", "q_traj", "q", "diff", "qdot_out", "status", "closest_j"))
    d = st.goto_js(oracle_c, chain, params, q0, w["fields"], w["nfields"], q_ref, N_CYCLES, STRIDE, DT, JS_PREC, rule=st.Rule(2, eps_js=1e-3), **kw)
    assert list(d["stalled"]) == [-1, -1, 2 * STRIDE - 1] and np.array_equal(d["arrived"], a["arrived"])


def test_patient_rule_is_script_reference(lib):
    import timed_reference as st
    from oracle import oracle_c
    from vfclik_amd import _abi
    chain, w, qg, way, q0, params = st.three_lwr_arms(_abi.F_MIXER, jp_kp=8.0)
    F, P = _abi.STEP_FRAME, _abi.STEP_POSTURE
    kind = np.array([[P, F, 0], [F, P, 0], [0, F, P]], dtype=np.int32)
    sign = np.array([1, -1, 1, -1, 1, -1, 1.0])
    q0 = np.array([qg[0, 0] + 0.02 * sign, qg[1, 0] + 0.03 * sign, qg[2, 0]])
    args = (oracle_c, chain, params, q0, w["fields"], w["nfields"], kind, way, qg, 240, STRIDE, DT, PREC, JS_PREC)
    kw = dict(hold=True, clamp=True, want=("qdot_out",))
    a = st.script(*args, **kw)
    b = st.script(*args, rule=st.Rule(61, eps=(1e-3, 1e-2), eps_js=1e-3), **kw)
    assert list(a["next"]) == [2, 2, 0]
    _same(a, b, ("reached", "next", "length", "pending", "q_traj", "dist_traj", "way_traj", "q", "diff", "qdot_out", "status", "q_ref",
                 "closest_c", "closest_j"))
    assert np.array_equal(a["fields"]["p"], b["fields"]["p"]) and np.all(b["stalled"] == -1)
    # both arms took more checks in total than a patience of 8, yet finish: the advance resets the state
    c = st.script(*args, rule=st.Rule(8, eps=(1e-4, 1e-3), eps_js=1e-4), **kw)
    checks = (a["reached"][:2, 1] + 1) // STRIDE
    assert np.all(checks > 8) and np.all(c["stalled"] == -1)
    _same(a, c, ("reached", "next", "q_traj"))
