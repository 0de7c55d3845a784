"""The batched goto (include/vfik.h: vfik_goto / vfik_goto_host; handlers.py:346-440 for the batch) on the GPU against its
restatement with the oracle (tests/timed_reference.py: goto): which arm arrives at which check, the joint path, the distance trace, the count
of arms still under way, the hold, the caller's gate, the early exit of the host form, its argument errors, the kernels it launches
and the sharded form.

Inputs: synth.make_workload(chain, B, 3, seed=53) with its goal replaced by chain.fk(qg), qg = U(0.7 q_lo, 0.7 q_hi), and the start at
qg + s U(-1, 1), s = U(0.02, 0.25) per arm, default_rng(7); dt 0.01, 160 cycles, clamp on, precision (0.01 m, 0.05 rad), max_vel 0.7.

Arrival is a threshold decision: an arm whose distance or angle comes, in the ORACLE's run, within MARGIN of its threshold at any
check is left out of the exact comparison (float64 I/O: 1e-6, at most 5 % of the arms; float32: 1e-4, at most 15 %); the cap is
asserted on the oracle's numbers before the GPU's are looked at.  Of a left-out arm only this is asserted: `arrived` is -1 or a
check's cycle index, and the GPU's own distance row at that check is under both thresholds."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import timed_reference as gr  # noqa: E402
import kernel_variants as kv  # noqa: E402

pytestmark = pytest.mark.gpu

N_CYCLES, DT, PREC = 160, 0.01, (0.01, 0.05)
THR = np.array([PREC[0], PREC[1] * 180.0 / np.pi])   # the thresholds in the units of a distance row (metres, degrees)
MARGIN = {np.dtype(np.float64): (1e-6, 0.05), np.dtype(np.float32): (1e-4, 0.15)}


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


def _case(env, robot, B, io_dtype=np.float64, gate=False, no_goal=None):
    """The inputs of the module's docstring; gate: the caller gates every third arm; no_goal: this arm has no field at all."""
    chain = env.robots.by_name(robot)
    w = env.synth.make_workload(chain, B, 3, seed=53, io_dtype=io_dtype)
    rng = np.random.default_rng(7)
    qg = rng.uniform(0.7 * chain.q_lo, 0.7 * chain.q_hi, size=(B, chain.n))
    s = rng.uniform(0.02, 0.25, size=(B, 1))
    q0 = (qg + s * rng.uniform(-1.0, 1.0, size=(B, chain.n))).astype(io_dtype).astype(np.float64)
    w["fields"]["p"][:, 0, :16] = chain.fk(qg).reshape(B, 16).astype(io_dtype).astype(np.float64)
    if no_goal is not None:
        w["nfields"][no_goal] = 0
    active = None
    if gate:
        active = np.ones(B, dtype=np.int32)
        active[::3] = 0
    return chain, w, q0, active


def _reference(env, robot, B, flags, stride, hold, io_dtype=np.float64, gate=False, no_goal=None):
    """The oracle's goto of a case, computed once per module and never modified."""
    key = (robot, B, flags, stride, hold, np.dtype(io_dtype).name, gate, no_goal)
    if key not in env.cache:
        chain, w, q0, active = _case(env, robot, B, io_dtype, gate, no_goal)
        params = env.abi.default_params(flags=flags, max_vel=0.7)
        ref = gr.goto(env.oc, chain, params, q0, w["fields"], w["nfields"], N_CYCLES, stride, DT, PREC, hold=hold, clamp=True, active=active,
                      io_dtype=io_dtype, want=("qdot_out",))
        for v in ref.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        env.cache[key] = (chain, w, q0, active, params, ref)
    return env.cache[key]


def _engine(env, chain, B, io_dtype, params, w):
    eng = env.engine.Engine(chain, B, io_dtype=io_dtype, max_slots=8, params=params)
    eng.set_fields(w["fields"], w["nfields"])
    return eng


def _left_out(ref, ua, io_dtype):
    """The arms within the margin of a threshold in the oracle's run; the cap holds on the oracle's numbers alone."""
    margin, cap = MARGIN[np.dtype(io_dtype)]
    out = ref["closest"] < margin
    share = np.count_nonzero(out & ua) / max(np.count_nonzero(ua), 1)
    print("left out: %d of %d arms (%.1f %%, cap %.0f %%)" % (np.count_nonzero(out & ua), np.count_nonzero(ua), 100 * share, 100 * cap))
    assert share <= cap, share
    return out


def _check(got, ref, q0, stride, hold, io_dtype, active=None, no_goal=None, tol_q=1e-8, tol_d=(1e-8, 1e-6), tol_v=1e-7):
    B = q0.shape[0]
    ua = np.ones(B, dtype=bool) if active is None else active != 0
    n_checks = N_CYCLES // stride
    out = _left_out(ref, ua, io_dtype)
    inc = ~out
    arr = got["arrived"]
    assert got["checks_run"] == n_checks and got["q_traj"].shape == ref["q_traj"].shape
    print("arrived: %d of %d, first arrivals at %d distinct checks (cycles %d..%d)" % (np.count_nonzero(arr >= 0), np.count_nonzero(ua),
          len(set(arr[arr >= 0])), arr[arr >= 0].min(), arr.max()))
    # arrival: exact outside the margin; inside it a valid check whose own distances are under both thresholds
    assert np.array_equal(arr[inc], ref["arrived"][inc]), np.flatnonzero(inc & (arr != ref["arrived"]))
    for b in np.flatnonzero(out):
        if arr[b] >= 0:
            assert (arr[b] + 1) % stride == 0 and arr[b] < N_CYCLES
            assert np.all(got["dist_traj"][(arr[b] + 1) // stride - 1, b] < THR), (b, arr[b])
    assert np.all(arr[~ua] == -1)
    # the path and the distances.  With hold an arm that arrives at another check than the oracle's stops elsewhere: included arms only
    rows = inc if hold else np.ones(B, dtype=bool)
    eq = np.abs(got["q_traj"][:, rows].astype(np.float64) - ref["q_traj"][:, rows])
    print("q_traj max error %.3e (tolerance %.1e)" % (eq.max(), tol_q))
    assert eq.max() < tol_q
    has = rows & ua
    if no_goal is not None:
        has[no_goal] = False   # measured against an empty goal block: nothing the reference defines
    ed = np.abs(got["dist_traj"][:, has].astype(np.float64) - ref["dist_traj"][:, has])
    print("dist_traj max error %.3e m (tolerance %.1e), %.3e deg (tolerance %.1e)" % (ed[..., 0].max(), tol_d[0], ed[..., 1].max(), tol_d[1]))
    assert ed[..., 0].max() < tol_d[0] and ed[..., 1].max() < tol_d[1]
    # pending: exactly the count its own arrived[] implies, and the oracle's up to the left-out arms
    cyc = (np.arange(n_checks) + 1) * stride - 1
    own = np.array([np.count_nonzero(ua & ((arr < 0) | (arr > c))) for c in cyc])
    assert np.array_equal(got["pending"], own)
    assert np.abs(got["pending"].astype(np.int64) - ref["pending"]).max() <= np.count_nonzero(out & ua)
    assert np.array_equal(got["q"], got["q_traj"][-1])
    # gated arms: every row carries their start
    assert np.all(got["q_traj"][:, ~ua] == q0[~ua].astype(io_dtype))
    if hold:   # a held arm's rows after its arrival are its arrival row, bit for bit
        for b in np.flatnonzero(arr >= 0):
            k = (arr[b] + 1) // stride - 1
            assert np.all(got["q_traj"][k:, b] == got["q_traj"][k, b]) and np.all(got["dist_traj"][k:, b] == got["dist_traj"][k, b]), b
    # every arm's output rows are those of its last evaluated cycle
    ev = np.abs(got["qdot_out"][rows].astype(np.float64) - ref["qdot_out"][rows]).max()
    print("qdot_out max error %.3e (tolerance %.1e)" % (ev, tol_v))
    assert ev < tol_v
    return inc


def _goto(eng, q0, stride, hold, active=None, **kw):
    q_in = q0.astype(eng.io_dtype)
    keep = q_in.copy()
    got = eng.goto_host(q_in, N_CYCLES, DT, PREC, stride=stride, hold=hold, clamp=True, trajectory=True, want=("qdot_out", "status"),
                        active=active, **kw)
    assert np.array_equal(q_in, keep)   # io->q is never written
    return got


def test_basic_stride_1(env):
    """lwr, float64, no module flag, 200 arms (three full waves and a partial one), a check after every cycle, no hold."""
    chain, w, q0, active, params, ref = _reference(env, "lwr", 200, 0, 1, False)
    assert np.count_nonzero(ref["arrived"] >= 0) >= 0.99 * 200 and len(set(ref["arrived"])) > 10
    eng = _engine(env, chain, 200, np.float64, params, w)
    got = _goto(eng, q0, 1, False)
    _check(got, ref, q0, 1, False, np.float64)
    eng.close()


def _after_hold(env, eng, chain, w, params, ref, inc, got):
    """A plain cycle after the goto, from the oracle's final angles on both sides: the held arms' nullspace sign memory is where their
    arrival block left it (an advanced or reset memory flips the sign of the nullspace command)."""
    nxt = env.oc.cycle_batch(chain, params, ref["q"], w["fields"], w["nfields"], states=ref["states"], want=("qdot_out", "qdot_null"))
    out = eng.step_host(np.array(ref["q"]), want=("qdot_out", "qdot_null"))
    for k in ("qdot_out", "qdot_null"):
        err = np.abs(out[k][inc] - nxt[k][inc]).max()
        print("following cycle, %s max error %.3e" % (k, err))
        assert err < 1e-6, (k, err)


@pytest.mark.parametrize("robot,B,flags", [("lwr", 200, 5), ("lwr_dual14", 130, 7), ("powercube6", 130, 12)])
def test_hold_stride_4(env, robot, B, flags):
    """Checks every 4 cycles, arrived arms held: lwr with the nullspace module and the joint-limit task (blocks are in-kernel rollouts),
    lwr_dual14 with the mixer too and powercube6 with mixer and limiter (blocks are stepped launches)."""
    chain, w, q0, active, params, ref = _reference(env, robot, B, flags, 4, True)
    n_arr = len(set(ref["arrived"][ref["arrived"] >= 0]))
    print("oracle: %d arms arrive, at %d distinct checks" % (np.count_nonzero(ref["arrived"] >= 0), n_arr))
    eng = _engine(env, chain, B, np.float64, params, w)
    got = _goto(eng, q0, 4, True)
    inc = _check(got, ref, q0, 4, True, np.float64)
    st = got["status"]
    assert np.array_equal(st[inc], ref["status"][inc])   # status ORs over the blocks
    if flags & 1:
        _after_hold(env, eng, chain, w, params, ref, inc, got)
    eng.close()


def test_float32_hold_stride_4(env):
    """float32 I/O, 203 arms (q rows of 5684 bytes: every second row of the trace is not 16-byte aligned).  q to the lean rollout test's
    2e-6.  Distances: a q error of 2e-6 rad on each of 7 joints moves the tool by at most 7 * 2e-6 * 1.3 m (the arm's reach) = 1.8e-5 m and
    turns it by at most 1.4e-5 rad = 8e-4 deg; rounding a distance below 1 m to float32 adds 3e-8, an angle below 180 deg 8e-6."""
    B = 203
    chain, w, q0, active, params, ref = _reference(env, "lwr", B, 0, 4, True, io_dtype=np.float32)
    eng = _engine(env, chain, B, np.float32, params, w)
    got = _goto(eng, q0, 4, True)
    _check(got, ref, q0, 4, True, np.float32, tol_q=2e-6, tol_d=(2e-5, 1e-3), tol_v=2e-5)
    eng.close()


def test_gate_and_missing_goal(env):
    """The caller gates every third arm: never run, never arrived, not counted, every row of the path their start.  Arm 1 has no field
    at all: it runs and never arrives."""
    chain, w, q0, active, params, ref = _reference(env, "lwr", 200, 0, 4, True, gate=True, no_goal=1)
    eng = _engine(env, chain, 200, np.float64, params, w)
    got = _goto(eng, q0, 4, True, active=active)
    _check(got, ref, q0, 4, True, np.float64, active=active, no_goal=1)
    assert got["arrived"][1] == -1 and np.all(got["arrived"][::3] == -1)
    assert got["pending"][-1] >= 1 and got["pending"][0] <= np.count_nonzero(active)
    assert np.all(got["status"][::3] == 0) and np.all(got["qdot_out"][::3] == 0)   # nothing was ever stored for a gated arm
    eng.close()


def test_early_exit(env):
    """Only arms the oracle shows arriving: a goto of 4000 cycles that polls every 8 checks ends a poll after the last arrival, and gives
    what the un-polled goto of as many checks gives, bit for bit."""
    chain, w, q0, active, params, ref = _reference(env, "lwr", 200, 5, 4, True)
    out = _left_out(ref, np.ones(200, dtype=bool), np.float64)
    sel = np.flatnonzero(ref["arrived"] >= 0)
    assert len(sel) >= 190
    last = int((ref["arrived"][sel].max() + 1) // 4 - 1)   # the oracle's last arrival check
    bound = (last + 8 + 7) // 8 * 8 + (8 if out[sel].any() else 0)
    eng = env.engine.Engine(chain, len(sel), io_dtype=np.float64, max_slots=8, params=params)
    eng.set_fields(w["fields"][sel], w["nfields"][sel])
    kw = dict(stride=4, hold=True, clamp=True, trajectory=True, want=("qdot_out", "status"))
    a = eng.goto_host(q0[sel], 4000, DT, PREC, poll=8, **kw)
    print("checks_run %d (oracle's last arrival at check %d, bound %d)" % (a["checks_run"], last, bound))
    assert 0 < a["checks_run"] <= bound and a["checks_run"] % 8 == 0
    assert a["pending"].shape == (a["checks_run"],) and a["pending"][-1] == 0 and np.all(a["arrived"] >= 0)
    assert a["q_traj"].shape[0] == a["checks_run"] == a["dist_traj"].shape[0]
    eng.reset_state()
    b = eng.goto_host(q0[sel], a["checks_run"] * 4, DT, PREC, poll=0, **kw)
    assert b["checks_run"] == a["checks_run"]
    for k in ("q", "arrived", "pending", "q_traj", "dist_traj", "qdot_out", "status"):
        assert np.array_equal(a[k], b[k]), k
    eng.close()


def test_argument_errors(env):
    """Every refused call raises, enqueues nothing, and leaves the engine able to give the basic case's result."""
    chain, w, q0, active, params, ref = _reference(env, "lwr", 200, 0, 1, False)
    eng = _engine(env, chain, 200, np.float64, params, w)
    B, n = q0.shape
    arrived = np.zeros(B, dtype=np.int32)
    dummy = np.zeros((B, 16))

    def call(null_opts=False, **kw):
        io = env.engine.IO()
        io.q = q0.ctypes.data
        o = env.abi.GotoOpts()
        o.n_cycles, o.stride, o.dt, o.pos_prec, o.rot_prec, o.arrived = 160, 4, DT, PREC[0], PREC[1], arrived.ctypes.data
        for k, v in kw.items():
            setattr(io if hasattr(io, k) else o, k, v)
        return eng.lib.vfik_goto_host(eng.h, C.byref(io), None if null_opts else C.byref(o), 0, None)

    bad = [dict(null_opts=True), dict(arrived=None), dict(stride=0), dict(stride=-4), dict(n_cycles=0), dict(n_cycles=1000004), dict(n_cycles=10),
           dict(dt=float("nan")), dict(dt=float("inf")), dict(pos_prec=-1e-3), dict(rot_prec=-1e-3), dict(pos_prec=float("nan")),
           dict(rot_prec=float("nan")), dict(q_cmded=dummy.ctypes.data), dict(track_error=dummy.ctypes.data), dict(obj_dist=dummy.ctypes.data)]
    for kw in bad:
        rc = call(**kw)
        assert rc == -1, (kw, rc, eng.lib.vfik_last_error())   # VFIK_E_ARG
        with pytest.raises(env.engine.VfikError):
            eng._chk(rc)
    with pytest.raises(env.engine.VfikError):
        eng.goto_host(q0, 10, DT, PREC, stride=4)
    with pytest.raises(env.engine.VfikError):
        eng.goto_host(q0, 160, DT, (0.01, -0.05))
    assert call() == 0
    got = _goto(eng, q0, 1, False)
    _check(got, ref, q0, 1, False, np.float64)
    eng.close()


@pytest.mark.parametrize("robot,flags", [("lwr", 5), ("lwr_dual14", 7)])
def test_only_existing_kernels(env, robot, flags):
    """A goto launches cycle kernels the library has for vfik_rollout, and moves nothing a captured launch depends on."""
    chain, w, q0, active = _case(env, robot, 130)
    params = env.abi.default_params(flags=flags, max_vel=0.7)
    eng = _engine(env, chain, 130, np.float64, params, w)
    eng.launched_kernels()
    epoch = eng.launch_epoch
    got = eng.goto_host(q0, 16, DT, PREC, stride=4, hold=True, clamp=True)
    assert got["checks_run"] == 4
    names = eng.launched_kernels()
    built = {v.name for v in kv.library_variants()}
    assert names
    for nm in names:
        assert kv.parse(nm).kernel.startswith("cycle_") and nm in built, nm
    assert eng.launch_epoch == epoch
    eng.close()


def test_device_form_equals_host_form(env):
    """Engine.goto on torch tensors (rows of the float32 trace that are not 16-byte aligned) gives the host form's arrays."""
    import torch
    B = 130
    chain, w, q0, active = _case(env, "lwr", B, np.float32)
    params = env.abi.default_params(flags=5, max_vel=0.7)
    eng = _engine(env, chain, B, np.float32, params, w)
    host = eng.goto_host(q0, 48, DT, PREC, stride=4, hold=True, clamp=True, trajectory=True, want=("qdot_out",))
    eng.reset_state()
    dev = torch.device("cuda", 0)
    q = torch.from_numpy(q0.astype(np.float32)).to(dev)
    t = dict(arrived=torch.zeros(B, dtype=torch.int32, device=dev), pending=torch.full((12,), 7, dtype=torch.int32, device=dev),
             q_out=torch.zeros(B, 7, device=dev), q_traj=torch.zeros(12, B, 7, device=dev), dist_traj=torch.zeros(12, B, 2, device=dev))
    qd = torch.zeros(B, 7, device=dev)
    torch.cuda.synchronize()
    eng.goto(eng.make_io(q, qdot_out=qd), 48, DT, PREC, stride=4, hold=True, clamp=True, **t)
    eng.sync()
    for k, hk in (("arrived", "arrived"), ("pending", "pending"), ("q_out", "q"), ("q_traj", "q_traj"), ("dist_traj", "dist_traj")):
        assert np.array_equal(t[k].cpu().numpy(), host[hk]), k
    assert np.array_equal(qd.cpu().numpy(), host["qdot_out"]) and np.array_equal(q.cpu().numpy(), q0.astype(np.float32))
    eng.close()


def test_sharded_goto_equals_single_engine(env):
    """ShardedEngine over devices (0, 0): two handles, 100 arms each, give the single engine's result on the whole batch."""
    chain, w, q0, active, params, ref = _reference(env, "lwr", 200, 5, 4, True)
    eng = _engine(env, chain, 200, np.float64, params, w)
    one = _goto(eng, q0, 4, True)
    eng.close()
    sh = env.sharding.ShardedEngine(chain, 200, rank=0, world=1, devices=(0, 0), io_dtype=np.float64, max_slots=8, params=params)
    sh.set_fields(w["fields"], w["nfields"])
    two = sh.goto_host(q0, N_CYCLES, DT, PREC, stride=4, hold=True, clamp=True, trajectory=True, want=("qdot_out", "status"))
    sh.close()
    assert two["checks_run"] == one["checks_run"]
    for k in ("q", "arrived", "pending", "q_traj", "dist_traj", "qdot_out", "status"):
        assert np.array_equal(one[k], two[k]), k
