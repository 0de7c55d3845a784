"""The timed moves under a coupling (include/vfik.h: vfik_set_coupling) on the GPU against tests/coupled_reference.py, the oracle-stepped
move with the other arm's link spheres in its loop.

The moves (coupled_reference.MOVES; arms in pairs b <-> b ^ 1 that end next to each other's spheres, three spheres per arm -- four on the
14-joint chain --, first_rep = 1 beside one static obstacle, the last arm of the odd batch without a partner):
    goto64   goto_host, lwr, 203 arms, float64, stride 1, nullspace module and mixer
    goto32   goto_host, lwr, 203 arms, float32, stride 4, hold
    stall64  goto_host, lwr, 203 arms, float64, stride 4, hold: the move of the stall-rule test
    follow   follow_host, lwr_dual14, 130 arms, float64, stride 4, hold, W = 3; arm 5's list is shorter, arm 8 has none

Against the reference: arrived / reached / next exact outside the suite's margin around the thresholds (1e-6; float32 1e-4), the joint
path within the suite's bars (1e-8; 2e-6).  Who is left out of the exact comparison: the arms within the margin IN THE REFERENCE'S RUN and,
under `hold`, the arms they are the source of -- an arm that stops at another check than the reference's is another obstacle for its
partner from there on.  The share is capped at 5 % (15 %) and asserted on the reference's numbers before the GPU's are read
(tests/test_coupled_reference.py checks the seeds on the CPU).

On the GPU's own rows: link_traj[k] is link_points of q_traj[k - 1] (k = 0: of io->q) bit for bit; with `hold` an arrived arm's spheres
stop moving in link_traj while its partner still runs; afterwards the repellers stand where the last block put them and the static obstacle
where it was (the next cycle equals that of an engine handed those rows through set_fields).
set_coupling(None) restores bit-equality with a handle that never had a coupling; a coupling whose every source is -1 equals the
uncoupled move bit for bit; a coupled move under set_stall_rule returns `stalled` as the reference has it."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import coupled_reference as cr  # noqa: E402
import timed_reference as tr  # noqa: E402

pytestmark = pytest.mark.gpu

N_CYCLES, DT, PREC = cr.N_CYCLES, cr.DT, cr.PREC
RULE = dict(patience=5, eps=(1e-3, 1e-2))   # tests/test_gpu_stall.py: its float64 goto


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


def _engine(env, name, c, params, coupled=True, trace=True, src=None):
    m = cr.MOVES[name]
    eng = env.engine.Engine(c["chain"], m["B"], io_dtype=m["io_dtype"], max_slots=8, params=params)
    eng.set_fields(c["w"]["fields"], c["w"]["nfields"])
    if coupled:
        eng.set_link_spheres(c["spheres"])
        eng.set_coupling(src_arm=c["src_arm"] if src is None else src, xform=c["xform"], first_rep=c["first_rep"],
                         trace_checks=N_CYCLES // m["stride"] if trace else None)
    return eng


def _move(eng, name, c, **kw):
    m = cr.MOVES[name]
    q_in = c["q0"].astype(eng.io_dtype)
    common = dict(stride=m["stride"], hold=m["hold"], clamp=True, trajectory=True, want=("qdot_out", "status"))
    common.update(kw)
    if c["way"] is None:
        return eng.goto_host(q_in, N_CYCLES, DT, PREC, **common)
    return eng.follow_host(q_in, c["way"], N_CYCLES, DT, PREC, **common)


def _left_out(name, c, ref, extra=None):
    """near a threshold in the reference's run, plus (hold) the arms such an arm is the source of; the cap on that, before the GPU is read"""
    m = cr.MOVES[name]
    part = ref["length"] > 0
    out, near, share, cap = cr.left_out(ref, part, m["io_dtype"], c["src_arm"], m["hold"], extra)
    print("%s: left out %d of %d arms (%d near a threshold; %.1f %%, cap %.0f %%)" % (name, np.count_nonzero(out & part), np.count_nonzero(part),
                                                                                     np.count_nonzero(near & part), 100 * share, 100 * cap))
    assert share <= cap, share
    return out, part


def _check(name, c, ref, got, out, part):
    m = cr.MOVES[name]
    io = np.dtype(m["io_dtype"])
    inc = ~out
    n_checks = N_CYCLES // m["stride"]
    assert got["checks_run"] == n_checks and got["q_traj"].shape == ref["q_traj"].shape
    if c["way"] is None:
        assert np.array_equal(got["arrived"][inc], ref["arrived"][inc]), np.flatnonzero(inc & (got["arrived"] != ref["arrived"]))
    else:
        assert np.array_equal(got["reached"][inc], ref["reached"][inc]) and np.array_equal(got["next"][inc], ref["next"][inc])
        assert np.all(got["next"][~part] == 0)
    rows = inc if m["hold"] else np.ones(m["B"], dtype=bool)
    eq = np.abs(got["q_traj"][:, rows].astype(np.float64) - ref["q_traj"][:, rows])
    print("%s: q_traj max error %.3e (bar %.1e)" % (name, eq.max(), cr.PATH_BAR[io]))
    per_arm = eq.max(axis=(0, 2))
    over = np.flatnonzero(per_arm >= cr.PATH_BAR[io])
    for b in np.flatnonzero(rows)[over][:8]:   # (what a failure is read from: the arm, the first check over the bar, its error there and at the end)
        e = np.abs(got["q_traj"][:, b].astype(np.float64) - ref["q_traj"][:, b]).max(axis=1)
        k = int(np.argmax(e >= cr.PATH_BAR[io]))
        print("  arm %d (source %d): over the bar from check %d (%.2e; the check before %.2e), at the end %.2e" % (b, c["src_arm"][b], k, e[k], e[max(k - 1, 0)], e[-1]))
    print("  arms over the bar: %d of %d" % (len(over), np.count_nonzero(rows)))
    assert eq.max() < cr.PATH_BAR[io]
    assert np.all(got["q_traj"][:, ~part] == c["q0"][~part].astype(io))


def _check_link_traj(eng, name, c, got, traj):
    """link_traj[k] = link_points of q_traj[k - 1] (k = 0: io->q), bit for bit, on the GPU's own rows"""
    m = cr.MOVES[name]
    n_checks = got["q_traj"].shape[0]
    assert traj.shape == (n_checks, m["B"], len(c["spheres"]), 4) and traj.dtype == np.dtype(m["io_dtype"])
    x = c["xform"]
    for k in range(n_checks):
        q = c["q0"] if k == 0 else got["q_traj"][k - 1].astype(np.float64)
        want = eng.link_points_host(q, c["src_arm"], x)
        assert np.array_equal(traj[k].astype(np.float64), want, equal_nan=True), k
    alone = c["src_arm"] < 0
    assert np.isnan(traj[:, alone]).all() and not np.isnan(traj[:, ~alone]).any()


def _check_scene_afterwards(env, eng, name, c, params, got, traj):
    """the partner's repellers stand where the last block put them, the static obstacle and everything else where it was: the next cycle is
    that of an engine that got those rows through set_fields"""
    m = cr.MOVES[name]
    f2 = np.array(c["w"]["fields"], copy=True)
    slots = cr.repeller_slots(f2, c["w"]["nfields"])
    last = traj[-1].astype(np.float64)
    for b in range(m["B"]):
        for j in range(len(c["spheres"])):
            if not np.isnan(last[b, j, 0]):
                f2["p"][b, slots[b][c["first_rep"] + j], 0:4] = last[b, j]
    if c["way"] is not None:   # a follow leaves the goal block at the waypoint the arm is under way to
        io = m["io_dtype"]
        for b in range(m["B"]):
            L = int(np.argmax(np.isnan(np.append(c["way"][b, :, 0], np.nan))))
            if L > 0:
                f2["p"][b, 0, :12] = c["way"][b, min(int(got["next"][b]), L - 1), :12].astype(io)
    ref = env.engine.Engine(c["chain"], m["B"], io_dtype=m["io_dtype"], max_slots=8, params=env.abi.default_params(flags=0, max_vel=0.7))
    ref.set_fields(f2, c["w"]["nfields"])
    eng.set_params(flags=0)
    q = got["q"].astype(np.float64)
    a, b = eng.step_host(q, want=("qdot_out", "pose")), ref.step_host(q, want=("qdot_out", "pose"))
    assert np.array_equal(a["qdot_out"], b["qdot_out"]) and np.array_equal(a["pose"], b["pose"])
    ref.close()


@pytest.mark.parametrize("name", ["goto64", "goto32", "follow"])
def test_against_the_coupled_reference(env, name):
    c, params, ref = cr.reference(env.oc, name)
    out, part = _left_out(name, c, ref)
    eng = _engine(env, name, c, params)
    got = _move(eng, name, c)
    traj = eng.link_traj()
    _check(name, c, ref, got, out, part)
    _check_link_traj(eng, name, c, got, traj)
    # the reference's own rows: the same positions up to the path's error times the arm's reach
    inc = ~out
    d = np.abs(traj[:, inc].astype(np.float64) - ref["link_traj"][:, inc])
    assert np.nanmax(d) < 1e3 * cr.PATH_BAR[np.dtype(cr.MOVES[name]["io_dtype"])]
    _check_scene_afterwards(env, eng, name, c, params, got, traj)
    eng.close()


def test_hold_freezes_an_arrived_arms_spheres(env):
    """goto32 (hold): once arm b arrived, the rows of b's spheres in its partner's link_traj repeat, while the partner still moves"""
    name = "goto32"
    c, params, _ref = cr.reference(env.oc, name)
    eng = _engine(env, name, c, params)
    got = _move(eng, name, c)
    traj = eng.link_traj()
    stride, arr, B = cr.MOVES[name]["stride"], got["arrived"], cr.MOVES[name]["B"]
    seen = 0
    for b in range(B - 1):
        p = b ^ 1
        if arr[b] < 0 or 0 <= arr[p] <= arr[b]:
            continue
        k = (arr[b] + 1) // stride
        if k >= traj.shape[0] - 1:
            continue
        assert np.all(traj[k:, p] == traj[k, p]), (b, p)
        assert np.any(traj[:k, p] != traj[k, p])                             # ... they moved until then
        assert np.any(got["q_traj"][k:, p] != got["q_traj"][k - 1, p])       # ... and the partner still runs
        seen += 1
    print("held arms whose partner still runs: %d" % seen)
    assert seen >= 10
    eng.close()


@pytest.mark.parametrize("name", ["goto64", "goto32"])
def test_off_and_no_source_equal_the_uncoupled_move(env, name):
    c, params, _ref = cr.reference(env.oc, name)
    keys = ("q_traj", "dist_traj", "arrived", "pending", "q", "qdot_out", "status")
    plain = _engine(env, name, c, params, coupled=False)
    want = _move(plain, name, c)
    # every source -1: the coupling's launches run and write nothing
    none = _engine(env, name, c, params, src=np.full(cr.MOVES[name]["B"], -1, dtype=np.int32))
    got = _move(none, name, c)
    assert all(np.array_equal(got[k], want[k]) for k in keys)
    assert np.isnan(none.link_traj()).all()
    # a coupled move, then the scene as it was and the coupling off: a handle that never had one
    eng = _engine(env, name, c, params, trace=False)
    moved = _move(eng, name, c)
    assert not np.array_equal(moved["q_traj"], want["q_traj"])
    eng.set_coupling(None)
    eng.set_fields(c["w"]["fields"], c["w"]["nfields"])
    eng.reset_state()
    again = _move(eng, name, c)
    assert all(np.array_equal(again[k], want[k]) for k in keys)
    with pytest.raises(env.engine.VfikError):
        eng.link_traj()
    for e in (plain, none, eng):
        e.close()


def test_coupled_move_under_the_stall_rule(env):
    """stall64 (lwr, 203 arms, float64, stride 4, hold) with a stall rule (stop): arms that a sphere of their partner keeps away from their
    goals stall instead of holding the move up.  (float64: an arm that cannot reach its goal creeps, and at float32 I/O with this
    rule 49 of the 203 arms have an arrival or progress compare within the suite's 1e-4 of its threshold in the reference's run -- 86 with
    the arms they are the source of, 42 % against a cap of 15 %; at float64 it is none.)"""
    name = "stall64"
    rule = tr.Rule(**RULE)
    c, params, ref = cr.reference(env.oc, name, rule=rule)
    m = cr.MOVES[name]
    near_stall = ref["closest_s"] < cr.MARGIN[np.dtype(m["io_dtype"])][0]
    out, part = _left_out(name, c, ref, extra=near_stall)
    print("reference: %d arrive, %d stall" % (np.count_nonzero(ref["arrived"] >= 0), np.count_nonzero(ref["stalled"] >= 0)))
    assert np.count_nonzero(ref["stalled"] >= 0) >= 10
    eng = _engine(env, name, c, params)
    eng.set_stall_rule(**RULE)
    got = _move(eng, name, c)
    inc = ~out
    assert np.array_equal(got["stalled"][inc], ref["stalled"][inc]), np.flatnonzero(inc & (got["stalled"] != ref["stalled"]))
    assert np.array_equal(got["arrived"][inc], ref["arrived"][inc])
    eq = np.abs(got["q_traj"][:, inc].astype(np.float64) - ref["q_traj"][:, inc])
    assert eq.max() < cr.PATH_BAR[np.dtype(m["io_dtype"])]
    # every arm, on the GPU's own rows: the machine replayed
    B, n = c["q0"].shape
    rep = tr.replay(np.full((B, 1), tr.FRAME, dtype=np.int32), np.zeros((B, 1, n)), ref["present"], got["q_traj"], got["dist_traj"], N_CYCLES,
                    m["stride"], PREC, np.zeros(n), hold=m["hold"], io_dtype=m["io_dtype"], rule=rule)
    assert np.array_equal(got["stalled"], rep.stalled) and np.array_equal(got["arrived"], rep.reached[:, 0])
    eng.close()
