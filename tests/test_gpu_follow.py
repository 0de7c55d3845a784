"""Waypoint lists (include/vfik.h: vfik_follow / vfik_follow_host) on the GPU against their restatement with the oracle
(tests/timed_reference.py: follow): which arm reaches which waypoint at which check, the joint path, the distance trace and the waypoint it
was measured against, the count of arms still under way, the hold, ragged paths, the caller's gate, the goal block afterwards, the
early exit of the host form, its argument errors, the kernels it launches and the sharded form.

Inputs: synth.make_workload(chain, B, 3, seed=53), W = 3, default_rng(12) drawn in this order: qg[:, 0] = U(0.6 q_lo, 0.6 q_hi),
qg[:, w] = qg[:, w - 1] + 0.12 U(-1, 1) for w = 1, 2, s = U(0.02, 0.12) per arm, the start qg[:, 0] + s U(-1, 1); waypoints
chain.fk(qg); 240 cycles, dt 0.01, clamp on, precision (0.01 m, 0.05 rad) at every waypoint, max_vel 0.7, hold on.

Reaching a waypoint is a threshold decision, and one that changes the arm's path from then on: an arm any of whose decisions comes, in
the ORACLE's run, within MARGIN of the threshold in force is left out of the exact comparison (float64 I/O: 1e-6, at most 5 % of the
arms; float32: 1e-4, at most 15 %); the cap is asserted on the oracle's numbers before the GPU's are looked at.  Of a left-out arm
only this is asserted: its `reached` row is ascending check cycles followed by -1, and `next` counts them."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import timed_reference as fr  # noqa: E402
import kernel_variants as kv  # noqa: E402

pytestmark = pytest.mark.gpu

N_CYCLES, DT, PREC, W = 240, 0.01, (0.01, 0.05), 3
MARGIN = {np.dtype(np.float64): (1e-6, 0.05), np.dtype(np.float32): (1e-4, 0.15)}
# float32 I/O: the figures of tests/test_gpu_goto.py:test_float32_hold_stride_4 (q, distances, velocities)
TOL32 = dict(tol_q=2e-6, tol_d=(2e-5, 1e-3), tol_v=2e-5)


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


def _case(env, robot, B, io_dtype=np.float64, gate=False, no_goal=None, ragged=False):
    """The inputs of the module's docstring; gate: the caller gates every third arm; no_goal: this arm has no field at all; ragged: arm b's
    path has (b + 3) % 4 rows -- 3, 0, 1, 2, 3, ... -- the rows behind it start with NaN."""
    chain = env.robots.by_name(robot)
    w = env.synth.make_workload(chain, B, 3, seed=53, io_dtype=io_dtype)
    rng = np.random.default_rng(12)
    qg = np.zeros((B, W, chain.n))
    qg[:, 0] = rng.uniform(0.6 * chain.q_lo, 0.6 * chain.q_hi, size=(B, chain.n))
    for i in range(1, W):
        qg[:, i] = qg[:, i - 1] + 0.12 * rng.uniform(-1.0, 1.0, size=(B, chain.n))
    s = rng.uniform(0.02, 0.12, size=(B, 1))
    q0 = (qg[:, 0] + s * rng.uniform(-1.0, 1.0, size=(B, chain.n))).astype(io_dtype).astype(np.float64)
    way = chain.fk(qg.reshape(B * W, chain.n)).reshape(B, W, 16).astype(io_dtype).astype(np.float64)
    if ragged:
        for b in range(B):
            way[b, (b + 3) % 4:, 0] = np.nan
    if no_goal is not None:
        w["nfields"][no_goal] = 0
    active = None
    if gate:
        active = np.ones(B, dtype=np.int32)
        active[::3] = 0
    return chain, w, q0, way, active


def _reference(env, robot, B, flags, stride, hold=True, io_dtype=np.float64, gate=False, no_goal=None, ragged=False, via=None, n_way=W):
    """The oracle's run of a case, computed once per module and never modified."""
    key = (robot, B, flags, stride, hold, np.dtype(io_dtype).name, gate, no_goal, ragged, via, n_way)
    if key not in env.cache:
        chain, w, q0, way, active = _case(env, robot, B, io_dtype, gate, no_goal, ragged)
        way = np.ascontiguousarray(way[:, :n_way])
        params = env.abi.default_params(flags=flags, max_vel=0.7)
        ref = fr.follow(env.oc, chain, params, q0, w["fields"], w["nfields"], way, N_CYCLES, stride, DT, PREC, via_precision=via, hold=hold,
                        clamp=True, active=active, io_dtype=io_dtype, want=("qdot_out",))
        for v in ref.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        env.cache[key] = (chain, w, q0, way, active, params, ref)
    return env.cache[key]


def _engine(env, chain, B, io_dtype, params, w):
    eng = env.engine.Engine(chain, B, io_dtype=io_dtype, max_slots=8, params=params)
    eng.set_fields(w["fields"], w["nfields"])
    return eng


def _left_out(ref, part, io_dtype):
    """The arms within the margin of a threshold in the oracle's run; the cap holds on the oracle's numbers alone."""
    margin, cap = MARGIN[np.dtype(io_dtype)]
    out = ref["closest"] < margin
    share = np.count_nonzero(out & part) / max(np.count_nonzero(part), 1)
    print("left out: %d of %d arms (%.1f %%, cap %.0f %%); nearest decision outside the margin %.2e"
          % (np.count_nonzero(out & part), np.count_nonzero(part), 100 * share, 100 * cap, ref["closest"][~out].min()))
    assert share <= cap, share
    return out


def _implied(reached, length, part, n_checks, stride):
    """pending[k] and way_traj[k] as an arm's own `reached` row implies them (way: -1 where the arm takes no part)."""
    cyc = (np.arange(n_checks) + 1) * stride - 1
    B = reached.shape[0]
    last = reached[np.arange(B), np.maximum(length - 1, 0)]
    pending = np.array([np.count_nonzero(part & ((last < 0) | (last > c))) for c in cyc])
    before = np.array([np.count_nonzero((reached >= 0) & (reached < c), axis=1) for c in cyc])   # waypoints reached at earlier checks
    way = np.where(part[None, :], np.minimum(before, np.maximum(length - 1, 0)[None, :]), -1)
    return pending, way


def _check(got, ref, q0, stride, io_dtype, active=None, no_goal=None, tol_q=1e-8, tol_d=(1e-8, 1e-6), tol_v=1e-7):
    B = q0.shape[0]
    ua = np.ones(B, dtype=bool) if active is None else active != 0
    length = ref["length"]
    part = ua & (length > 0)
    n_checks = N_CYCLES // stride
    out = _left_out(ref, part, io_dtype)
    inc = ~out
    r, nx = got["reached"], got["next"]
    assert got["checks_run"] == n_checks and got["q_traj"].shape == ref["q_traj"].shape
    print("waypoints reached: %d of %d, at %d distinct checks; arms at their last waypoint: %d of %d"
          % (np.count_nonzero(r >= 0), length[part].sum(), len(set(r[r >= 0])), np.count_nonzero(nx[part] == length[part]), np.count_nonzero(part)))
    # reached and next: exact outside the margin; inside it ascending check cycles, then -1
    assert np.array_equal(r[inc], ref["reached"][inc]), np.flatnonzero(inc & np.any(r != ref["reached"], axis=1))
    assert np.array_equal(nx[inc], ref["next"][inc])
    for b in range(B):
        assert 0 <= nx[b] <= length[b] and np.all(r[b, nx[b]:] == -1), b
        row = r[b, : nx[b]]
        assert np.all((row + 1) % stride == 0) and np.all(row >= 0) and np.all(row < N_CYCLES) and np.all(np.diff(row) > 0), (b, row)
    assert np.all(nx[~part] == 0)
    # the path and the distances: a left-out arm that advances at another check than the oracle's goes another way from there
    eq = np.abs(got["q_traj"][:, inc].astype(np.float64) - ref["q_traj"][:, inc])
    print("q_traj max error %.3e (tolerance %.1e)" % (eq.max(), tol_q))
    assert eq.max() < tol_q
    has = inc & part
    if no_goal is not None:
        has[no_goal] = False   # measured against an empty goal block: nothing the reference defines
    ed = np.abs(got["dist_traj"][:, has].astype(np.float64) - ref["dist_traj"][:, has])
    print("dist_traj max error %.3e m (tolerance %.1e), %.3e deg (tolerance %.1e)" % (ed[..., 0].max(), tol_d[0], ed[..., 1].max(), tol_d[1]))
    assert ed[..., 0].max() < tol_d[0] and ed[..., 1].max() < tol_d[1]
    # pending and way_traj: exactly what its own reached[] implies, and the oracle's up to the left-out arms
    own_p, own_w = _implied(r, length, part, n_checks, stride)
    assert np.array_equal(got["pending"], own_p)
    assert np.array_equal(got["way_traj"], own_w), np.argwhere(got["way_traj"] != own_w)[:5]
    assert np.abs(got["pending"].astype(np.int64) - ref["pending"]).max() <= np.count_nonzero(out & part)
    assert np.array_equal(got["way_traj"][:, inc], ref["way_traj"][:, inc])
    assert np.array_equal(got["q"], got["q_traj"][-1])
    # arms that take no part: every row carries their start
    assert np.all(got["q_traj"][:, ~part] == q0[~part].astype(io_dtype))
    ev = np.abs(got["qdot_out"][inc].astype(np.float64) - ref["qdot_out"][inc]).max()
    print("qdot_out max error %.3e (tolerance %.1e)" % (ev, tol_v))
    assert ev < tol_v
    return inc


def _held_rows_repeat(got, length, part, stride):
    """hold: from the check of its last waypoint on an arm's rows are that check's, bit for bit"""
    for b in np.flatnonzero(part & (got["next"] == length)):
        k = (got["reached"][b, length[b] - 1] + 1) // stride - 1
        assert np.all(got["q_traj"][k:, b] == got["q_traj"][k, b]) and np.all(got["dist_traj"][k:, b] == got["dist_traj"][k, b]), b


def _follow(eng, q0, way, stride, hold=True, active=None, **kw):
    q_in = q0.astype(eng.io_dtype)
    keep = q_in.copy()
    got = eng.follow_host(q_in, way, N_CYCLES, DT, PREC, stride=stride, hold=hold, clamp=True, trajectory=True, want=("qdot_out", "status"),
                          active=active, **kw)
    assert np.array_equal(q_in, keep)   # io->q is never written
    return got


def _run(env, robot, B, flags, stride, io_dtype=np.float64, **kw):
    chain, w, q0, way, active, params, ref = _reference(env, robot, B, flags, stride, io_dtype=io_dtype, **kw)
    eng = _engine(env, chain, B, io_dtype, params, w)
    got = _follow(eng, q0, way, stride, hold=kw.get("hold", True), active=active, via_precision=kw.get("via"))
    return chain, w, q0, way, active, params, ref, eng, got


def test_lwr_two_blocks(env):
    """lwr with the nullspace module and the mixer (flags 5), float64, 330 arms: two blocks of 256 threads, a partial last wave."""
    chain, w, q0, way, active, params, ref, eng, got = _run(env, "lwr", 330, 5, 4)
    assert np.count_nonzero(ref["next"] == 3) >= 0.99 * 330 and len(set(ref["reached"].ravel())) >= 15   # all the way, at many distinct checks
    inc = _check(got, ref, q0, 4, np.float64)
    _held_rows_repeat(got, ref["length"], np.ones(330, dtype=bool), 4)
    assert np.array_equal(got["status"][inc], ref["status"][inc])   # status ORs over the blocks
    # the goal block afterwards, and the held arms' sign memory
    nxt = env.oc.cycle_batch(chain, params, ref["q"], ref["fields"], w["nfields"], states=ref["states"], want=("qdot_out", "qdot_null"))
    out = eng.step_host(np.array(ref["q"]), want=("qdot_out", "qdot_null"))
    for k in ("qdot_out", "qdot_null"):
        err = np.abs(out[k][inc] - nxt[k][inc]).max()
        print("following cycle, %s max error %.3e" % (k, err))
        assert err < 1e-6, (k, err)
    eng.close()


@pytest.mark.parametrize("robot,flags", [("lwr_dual14", 7), ("powercube6", 12)])
def test_stepped_path(env, robot, flags):
    """lwr_dual14 with the joint-limit task too and powercube6 with mixer and limiter: the blocks are stepped launches."""
    chain, w, q0, way, active, params, ref, eng, got = _run(env, robot, 96, flags, 4)
    inc = _check(got, ref, q0, 4, np.float64)
    _held_rows_repeat(got, ref["length"], np.ones(96, dtype=bool), 4)
    assert np.array_equal(got["status"][inc], ref["status"][inc])
    eng.close()


def test_float32_device_form_odd_rows(env):
    """float32 I/O, stride 8, 96 arms, through the device form with q_traj, dist_traj and the start one element into their allocations: no
    row of the traces is 16-byte aligned (every block's q goes through the staging buffer).  The goto test's float32 tolerances."""
    import torch
    B, stride = 96, 8
    chain, w, q0, way, active, params, ref = _reference(env, "lwr", B, 0, stride, io_dtype=np.float32)
    eng = _engine(env, chain, B, np.float32, params, w)
    dev = torch.device("cuda", 0)
    n_checks = N_CYCLES // stride

    def odd(shape):
        t = torch.zeros(int(np.prod(shape)) + 1, device=dev)[1:].view(*shape)
        assert t.data_ptr() % 16 == 4 and t.is_contiguous()
        return t
    q = odd((B, 7))
    q.copy_(torch.from_numpy(q0.astype(np.float32)))
    t = dict(reached=torch.full((B, W), 7, dtype=torch.int32, device=dev), next=torch.full((B,), 7, dtype=torch.int32, device=dev),
             pending=torch.full((n_checks,), 7, dtype=torch.int32, device=dev), q_out=torch.zeros(B, 7, device=dev),
             q_traj=odd((n_checks, B, 7)), dist_traj=odd((n_checks, B, 2)), way_traj=torch.full((n_checks, B), -1, dtype=torch.int32, device=dev))
    qd = torch.zeros(B, 7, device=dev)
    wt = torch.from_numpy(way.astype(np.float32)).to(dev)
    torch.cuda.synchronize()
    eng.follow(eng.make_io(q, qdot_out=qd), wt, N_CYCLES, DT, PREC, stride=stride, hold=True, clamp=True, **t)
    eng.sync()
    got = {k: v.cpu().numpy() for k, v in t.items()}
    got["q"], got["qdot_out"], got["checks_run"] = got.pop("q_out"), qd.cpu().numpy(), n_checks
    _check(got, ref, q0, stride, np.float32, **TOL32)
    _held_rows_repeat(got, ref["length"], np.ones(B, dtype=bool), stride)
    eng.close()


def test_hold_off_keeps_tracking(env):
    """Without hold an arm at its last waypoint keeps tracking it: it runs every block, its rows go on changing, `next` stays L."""
    chain, w, q0, way, active, params, ref, eng, got = _run(env, "lwr", 96, 5, 4, hold=False)
    _check(got, ref, q0, 4, np.float64)
    done = np.flatnonzero(got["next"] == 3)
    assert len(done) >= 90
    moved = 0
    for b in done:
        k = (got["reached"][b, 2] + 1) // 4 - 1
        moved += k + 1 < N_CYCLES // 4 and np.any(got["q_traj"][k + 1:, b] != got["q_traj"][k, b])
        assert np.all(got["way_traj"][k:, b] == 2)
    assert moved >= 0.9 * len(done), moved
    eng.close()


def test_ragged_paths(env):
    """Paths of 3, 0, 1, 2, 3, ... rows.  An arm without a row is kept out like a gated one: never run (nothing stored for it), not
    counted, its q rows its start, its goal block what set_fields put there."""
    B = 96
    chain, w, q0, way, active, params, ref, eng, got = _run(env, "lwr", B, 5, 4, ragged=True)
    assert sorted(set(ref["length"])) == [0, 1, 2, 3]
    inc = _check(got, ref, q0, 4, np.float64)
    none = ref["length"] == 0
    assert np.all(got["status"][none] == 0) and np.all(got["qdot_out"][none] == 0) and np.all(got["way_traj"][:, none] == -1)
    assert got["pending"][0] <= np.count_nonzero(~none) and got["pending"][-1] == 0
    _held_rows_repeat(got, ref["length"], ~none, 4)
    # the goal blocks afterwards: waypoint min(next, L - 1) where the arm has a path, the set_fields goal where it has none
    assert np.array_equal(ref["fields"]["p"][none], w["fields"]["p"][none])
    nxt = env.oc.cycle_batch(chain, params, ref["q"], ref["fields"], w["nfields"], states=ref["states"], want=("qdot_out", "pose"))
    out = eng.step_host(np.array(ref["q"]), want=("qdot_out", "goal_dist"))
    err = np.abs(out["qdot_out"][inc] - nxt["qdot_out"][inc]).max()
    ed = np.abs(out["goal_dist"][inc] - fr.goal_distance(nxt["pose"], fr.goal_frames(ref["fields"], w["nfields"]))[inc]).max(axis=0)
    print("following cycle: qdot_out max error %.3e, goal_dist %.3e m %.3e deg" % (err, ed[0], ed[1]))
    assert err < 1e-6 and ed[0] < 1e-8 and ed[1] < 1e-6
    eng.close()


def test_gate_and_missing_goal(env):
    """The caller gates every third arm: never run, nowhere reached, not counted.  Arm 1 has no field at all: it runs, reaches nothing,
    stays counted, and nothing is written where its goal block would be (the following cycle still sees no goal: zero command)."""
    B = 96
    chain, w, q0, way, active, params, ref, eng, got = _run(env, "lwr", B, 0, 4, gate=True, no_goal=1)
    inc = _check(got, ref, q0, 4, np.float64, active=active, no_goal=1)
    assert np.all(got["reached"][1] == -1) and got["next"][1] == 0 and np.all(got["reached"][::3] == -1)
    assert got["pending"][-1] >= 1 and got["pending"][0] <= np.count_nonzero(active)
    assert np.all(got["status"][::3] == 0) and np.all(got["qdot_out"][::3] == 0)   # nothing was ever stored for a gated arm
    out = eng.step_host(q0, want=("qdot_out",))   # a gated arm's goal and the missing one stay, the others hold their last waypoint
    ref1 = env.oc.cycle_batch(chain, params, q0, ref["fields"], w["nfields"], want=("qdot_out",))
    assert np.abs(out["qdot_out"][inc] - ref1["qdot_out"][inc]).max() < 1e-6 and np.all(out["qdot_out"][1] == 0)
    eng.close()


def test_via_precision(env):
    """Via waypoints five times looser than the last one: they are reached no later than with the tight pair, `reached` is exact."""
    via = (5 * PREC[0], 5 * PREC[1])
    chain, w, q0, way, active, params, ref, eng, got = _run(env, "lwr", 96, 5, 4, via=via)
    tight = _reference(env, "lwr", 96, 5, 4)[6]
    assert np.all(ref["reached"][:, 0] <= tight["reached"][:, 0]) and np.any(ref["reached"][:, 0] < tight["reached"][:, 0])
    inc = _check(got, ref, q0, 4, np.float64)
    out_t = tight["closest"] < MARGIN[np.dtype(np.float64)][0]
    both = inc & ~out_t
    assert np.all(got["reached"][both, :2] <= tight["reached"][both, :2])
    eng.close()


def test_one_waypoint_equals_goto(env):
    """W = 1 with the goal set_fields holds is a goto: arrived == reached[:, 0], the same path, bit for bit."""
    B = 96
    chain, w, q0, way, active = _case(env, "lwr", B)
    params = env.abi.default_params(flags=5, max_vel=0.7)
    w["fields"]["p"][:, 0, :16] = way[:, 0]
    eng = _engine(env, chain, B, np.float64, params, w)
    kw = dict(stride=4, hold=True, clamp=True, trajectory=True, want=("qdot_out", "status"))
    a = eng.goto_host(q0, N_CYCLES, DT, PREC, **kw)
    eng.reset_state()
    b = eng.follow_host(q0, way[:, :1], N_CYCLES, DT, PREC, **kw)
    assert np.count_nonzero(a["arrived"] >= 0) >= 90
    assert np.array_equal(a["arrived"], b["reached"][:, 0]) and np.array_equal(b["next"], (a["arrived"] >= 0).astype(np.int32))
    for k in ("q", "pending", "q_traj", "dist_traj", "qdot_out", "status"):
        assert np.array_equal(a[k], b[k]), k
    eng.close()


def test_early_exit(env):
    """A run of 4000 cycles that polls every 8 checks ends a poll after the last arm is at its last waypoint, and gives what the
    un-polled run of as many checks gives, bit for bit."""
    chain, w, q0, way, active, params, ref = _reference(env, "lwr", 96, 5, 4)
    out = _left_out(ref, np.ones(96, dtype=bool), np.float64)
    assert np.all(ref["next"] == 3)
    last = int((ref["reached"][:, 2].max() + 1) // 4 - 1)
    bound = (last + 8 + 7) // 8 * 8 + (8 if out.any() else 0)
    eng = _engine(env, chain, 96, np.float64, params, w)
    kw = dict(stride=4, hold=True, clamp=True, trajectory=True, want=("qdot_out", "status"))
    a = eng.follow_host(q0, way, 4000, DT, PREC, poll=8, **kw)
    print("checks_run %d (oracle's last arrival at check %d, bound %d)" % (a["checks_run"], last, bound))
    assert 0 < a["checks_run"] <= bound and a["checks_run"] % 8 == 0
    assert a["pending"].shape == (a["checks_run"],) and a["pending"][-1] == 0 and np.all(a["next"] == 3)
    assert a["q_traj"].shape[0] == a["checks_run"] == a["dist_traj"].shape[0] == a["way_traj"].shape[0]
    eng.reset_state()   # (the goal blocks hold waypoint 2 now: the pass in front of block 0 puts waypoint 0 back)
    b = eng.follow_host(q0, way, a["checks_run"] * 4, DT, PREC, poll=0, **kw)
    assert b["checks_run"] == a["checks_run"]
    for k in ("q", "reached", "next", "pending", "q_traj", "dist_traj", "way_traj", "qdot_out", "status"):
        assert np.array_equal(a[k], b[k]), k
    eng.close()


def test_device_form_equals_host_form(env):
    """Engine.follow on torch tensors gives the host form's arrays (float64, ragged paths, the caller's gate)."""
    import torch
    B = 96
    chain, w, q0, way, active = _case(env, "lwr", B, gate=True, ragged=True)
    params = env.abi.default_params(flags=5, max_vel=0.7)
    eng = _engine(env, chain, B, np.float64, params, w)
    host = eng.follow_host(q0, way, 96, DT, PREC, stride=4, hold=True, clamp=True, trajectory=True, want=("qdot_out",), active=active)
    eng.reset_state()
    dev = torch.device("cuda", 0)
    f64 = dict(dtype=torch.float64, device=dev)
    q = torch.from_numpy(q0).to(dev)
    t = dict(reached=torch.full((B, W), 7, dtype=torch.int32, device=dev), next=torch.full((B,), 7, dtype=torch.int32, device=dev),
             pending=torch.full((24,), 7, dtype=torch.int32, device=dev), q_out=torch.zeros(B, 7, **f64), q_traj=torch.zeros(24, B, 7, **f64),
             dist_traj=torch.zeros(24, B, 2, **f64), way_traj=torch.full((24, B), -1, dtype=torch.int32, device=dev))
    qd = torch.zeros(B, 7, **f64)
    act = torch.from_numpy(active).to(dev)
    wt = torch.from_numpy(way).to(dev)
    torch.cuda.synchronize()
    eng.follow(eng.make_io(q, qdot_out=qd, active=act), wt, 96, DT, PREC, stride=4, hold=True, clamp=True, **t)
    eng.sync()
    assert host["next"].sum() > 0
    for k, hk in (("reached", "reached"), ("next", "next"), ("pending", "pending"), ("q_out", "q"), ("q_traj", "q_traj"),
                  ("dist_traj", "dist_traj"), ("way_traj", "way_traj")):
        assert np.array_equal(t[k].cpu().numpy(), host[hk]), k
    assert np.array_equal(qd.cpu().numpy(), host["qdot_out"]) and np.array_equal(q.cpu().numpy(), q0)
    eng.close()


def test_argument_errors(env):
    """Every refused call returns VFIK_E_ARG and enqueues nothing: reached and next keep their sentinel, and the engine still gives the
    two-block case's result."""
    chain, w, q0, way, active, params, ref = _reference(env, "lwr", 330, 5, 4)
    B = 330
    eng = _engine(env, chain, B, np.float64, params, w)
    reached = np.full((B, W), 77, dtype=np.int32)
    nxt = np.full(B, 77, dtype=np.int32)
    dummy = np.zeros((B, 16))
    assert way.ctypes.data % 16 == 0

    def call(null_opts=False, **kw):
        io = env.engine.IO()
        io.q = q0.ctypes.data
        o = env.abi.FollowOpts()
        o.n_cycles, o.stride, o.dt, o.pos_prec, o.rot_prec, o.via_pos_prec, o.via_rot_prec = 240, 4, DT, PREC[0], PREC[1], PREC[0], PREC[1]
        o.n_way, o.way16, o.reached, o.next = W, way.ctypes.data, reached.ctypes.data, nxt.ctypes.data
        for k, v in kw.items():
            setattr(io if hasattr(io, k) else o, k, v)
        return eng.lib.vfik_follow_host(eng.h, C.byref(io), None if null_opts else C.byref(o), 0, None)

    nan = float("nan")
    bad = [dict(null_opts=True), dict(way16=None), dict(reached=None), dict(next=None), dict(n_way=0), dict(n_way=-3),
           dict(way16=way.ctypes.data + 8), dict(via_pos_prec=-1e-3), dict(via_rot_prec=-1e-3), dict(via_pos_prec=nan), dict(via_rot_prec=nan),
           dict(stride=0), dict(stride=-4), dict(n_cycles=0), dict(n_cycles=1000004), dict(n_cycles=10), dict(dt=nan), dict(dt=float("inf")),
           dict(pos_prec=-1e-3), dict(rot_prec=-1e-3), dict(pos_prec=nan), dict(rot_prec=nan), dict(q_cmded=dummy.ctypes.data),
           dict(track_error=dummy.ctypes.data), dict(obj_dist=dummy.ctypes.data)]
    for kw in bad:
        rc = call(**kw)
        assert rc == -1, (kw, rc, eng.lib.vfik_last_error())   # VFIK_E_ARG
        with pytest.raises(env.engine.VfikError):
            eng._chk(rc)
    eng.sync()
    assert np.all(reached == 77) and np.all(nxt == 77)
    with pytest.raises(env.engine.VfikError):
        eng.follow_host(q0, way, 10, DT, PREC, stride=4)
    with pytest.raises(env.engine.VfikError):
        eng.follow_host(q0, way, 240, DT, PREC, via_precision=(0.01, -0.05))
    with pytest.raises(ValueError):
        eng.follow_host(q0, way[:, :, :12], 240, DT, PREC)
    got = _follow(eng, q0, way, 4)
    _check(got, ref, q0, 4, np.float64)
    assert call() == 0 and np.all(nxt <= 3) and np.all(reached < 240)
    eng.close()


@pytest.mark.parametrize("robot,flags", [("lwr", 5), ("lwr_dual14", 7)])
def test_only_a_gotos_kernels(env, robot, flags):
    """A follow lists no cycle kernel that a goto under the gate does not list, and moves nothing a captured launch depends on."""
    chain, w, q0, way, active = _case(env, robot, 96)
    params = env.abi.default_params(flags=flags, max_vel=0.7)
    eng = _engine(env, chain, 96, np.float64, params, w)
    eng.launched_kernels()
    eng.goto_host(q0, 16, DT, PREC, stride=4, hold=True, clamp=True)
    of_goto = eng.launched_kernels()
    epoch, path, slots = eng.launch_epoch, eng.field_path, eng.slots_in_use
    got = eng.follow_host(q0, way, 16, DT, PREC, stride=4, hold=True, clamp=True)
    assert got["checks_run"] == 4
    names = eng.launched_kernels()
    built = {v.name for v in kv.library_variants()}
    assert names and names <= of_goto, names - of_goto
    for nm in names:
        assert kv.parse(nm).kernel.startswith("cycle_") and nm in built, nm
    assert (eng.launch_epoch, eng.field_path, eng.slots_in_use) == (epoch, path, slots)
    eng.close()


def test_sharded_follow_equals_single_engine(env):
    """ShardedEngine over devices (0, 0): two handles, 48 arms each, give the single engine's result on the whole batch."""
    chain, w, q0, way, active, params, ref = _reference(env, "lwr", 96, 5, 4, ragged=True)
    eng = _engine(env, chain, 96, np.float64, params, w)
    one = _follow(eng, q0, way, 4)
    eng.close()
    sh = env.sharding.ShardedEngine(chain, 96, rank=0, world=1, devices=(0, 0), io_dtype=np.float64, max_slots=8, params=params)
    sh.set_fields(w["fields"], w["nfields"])
    two = sh.follow_host(q0, way, N_CYCLES, DT, PREC, stride=4, hold=True, clamp=True, trajectory=True, want=("qdot_out", "status"))
    sh.close()
    assert two["checks_run"] == one["checks_run"]
    for k in ("q", "reached", "next", "pending", "q_traj", "dist_traj", "way_traj", "qdot_out", "status"):
        assert np.array_equal(one[k], two[k]), k
