"""The joint-space goto (include/vfik.h: vfik_goto_js / vfik_goto_js_host; set_ref_js, handlers.py:544-576, for the batch) on the GPU
against its restatement with the oracle (tests/timed_reference.py: goto_js): which arm arrives at which check, the joint path, `diff`, the count
of arms still under way, the hold, the caller's gate, arms without a controller, the decision edges, the early exit of the host form, its
argument errors, the kernels it launches, the device form and the sharded form.

Inputs: synth.make_workload(chain, B, 3, seed=53); ref = U(0.7 q_lo, 0.7 q_hi), the start at ref + s U(-1, 1), s = U(0.02, 0.25) per arm,
default_rng(7); jp_kp 8, dt 0.01, 80 cycles, clamp on, prec[i] = 0.004 + 0.002 i, mixer weights [0, 0, 1, 0, 0, 0] with F_MIXER.

Arrival is a threshold decision: an arm of which some joint comes, in the ORACLE's run, within MARGIN of an edge ref -+ prec at any check
up to its arrival is left out of the exact comparison with the oracle.  float64: 1e-7 = 10 x the 1e-8 path tolerance asserted here (as
tests/test_gpu_goto.py); float32: 4e-6 = 2 x the suite's float32 path tolerance 2e-6.  At most 5 % / 10 % of the arms may be left out; the
cap is asserted on the oracle's numbers before the GPU's are looked at.  EVERY arm, left out or not, is held to the rule on the GPU's own
rows: `arrived` is the first check at which the helper's rule holds on the GPU's q_traj row, exactly."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import timed_reference as jr  # noqa: E402
import kernel_variants as kv  # noqa: E402

pytestmark = pytest.mark.gpu

N_CYCLES, DT, KP = 80, 0.01, 8.0
MIX_JOINT = [0.0, 0.0, 1.0, 0.0, 0.0, 0.0]
MIX_CART = [1.0, 1.0, 0.0, 0.0, 0.0, 0.0]
MARGIN = {np.dtype(np.float64): (1e-7, 0.05), np.dtype(np.float32): (4e-6, 0.10)}
TOL = {np.dtype(np.float64): (1e-8, 1e-7), np.dtype(np.float32): (2e-6, 2e-5)}   # q_traj, qdot_out


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


def _case(env, robot, B, io_dtype=np.float64):
    """The inputs of the module's docstring."""
    chain = env.robots.by_name(robot)
    w = env.synth.make_workload(chain, B, 3, seed=53, io_dtype=io_dtype)
    rng = np.random.default_rng(7)
    ref = rng.uniform(0.7 * chain.q_lo, 0.7 * chain.q_hi, size=(B, chain.n))
    s = rng.uniform(0.02, 0.25, size=(B, 1))
    q0 = (ref + s * rng.uniform(-1.0, 1.0, size=(B, chain.n))).astype(io_dtype).astype(np.float64)
    ref = ref.astype(io_dtype).astype(np.float64)
    return chain, w, q0, ref


def _params(env, flags=None, mix_w=MIX_JOINT):
    return env.abi.default_params(flags=env.abi.F_MIXER if flags is None else flags, mix_w=mix_w, jp_kp=KP)


def _reference(env, robot, B, stride, hold, io_dtype=np.float64, mixed=False):
    """The oracle's run of a case, computed once per module and never modified.  mixed: the fleet of test_mixed_fleet."""
    key = (robot, B, stride, hold, np.dtype(io_dtype).name, mixed)
    if key not in env.cache:
        chain, w, q0, ref = _case(env, robot, B, io_dtype)
        active = mixw = None
        params = _params(env)
        if mixed:
            params = _params(env, env.abi.F_NULLSPACE | env.abi.F_MIXER)
            mixw = np.tile(np.array(MIX_JOINT), (B, 1))
            mixw[1::2] = MIX_CART
            ref[1::2, 0] = np.nan
            active = np.ones(B, dtype=np.int32)
            active[::3] = 0
        out = jr.goto_js(env.oc, chain, params, q0, w["fields"], w["nfields"], ref, N_CYCLES, stride, DT, _prec(chain.n), hold=hold, clamp=True,
                         active=active, io_dtype=io_dtype, want=("qdot_out",), stepped=chain.n > 7, mix_w_arm=mixw)
        for v in out.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        env.cache[key] = (chain, w, q0, ref, active, mixw, params, out)
    return env.cache[key]


def _engine(env, chain, B, io_dtype, params, w, mixw=None):
    eng = env.engine.Engine(chain, B, io_dtype=io_dtype, max_slots=8, params=params)
    eng.set_fields(w["fields"], w["nfields"])
    if mixw is not None:
        eng.set_mixer_weights(mixw)
    return eng


def _left_out(ref, ua, io_dtype):
    """The arms within the margin of an edge in the oracle's run; the cap holds on the oracle's numbers alone."""
    margin, cap = MARGIN[np.dtype(io_dtype)]
    out = ref["closest"] < margin
    share = np.count_nonzero(out & ua) / max(np.count_nonzero(ua), 1)
    print("left out: %d of %d arms (%.1f %%, cap %.0f %%)" % (np.count_nonzero(out & ua), np.count_nonzero(ua), 100 * share, 100 * cap))
    assert share <= cap, share
    return out


def _first_pass(q_ref, q_traj, prec, stride):
    """(B,) what `arrived` must be given the q rows: the cycle index of the first check whose row passes the helper's rule, or -1."""
    ok = np.stack([jr.rule(q_ref, row.astype(np.float64), prec) for row in q_traj])      # (n_checks, B)
    return np.where(ok.any(axis=0), (np.argmax(ok, axis=0) + 1) * stride - 1, -1).astype(np.int32)


def _check(got, ref, q0, q_ref, stride, hold, io_dtype, active=None):
    io_dtype = np.dtype(io_dtype)
    B, n = q0.shape
    prec = _prec(n)
    ua = np.ones(B, dtype=bool) if active is None else active != 0
    n_checks = N_CYCLES // stride
    out = _left_out(ref, ua, io_dtype)
    inc = ~out
    arr = got["arrived"]
    tol_q, tol_v = TOL[io_dtype]
    assert got["checks_run"] == n_checks and got["q_traj"].shape == ref["q_traj"].shape
    print("arrived: %d of %d at %d distinct checks" % (np.count_nonzero(arr >= 0), np.count_nonzero(ua), len(set(arr[arr >= 0]))))
    # arrival: the oracle's outside the margin; the helper's rule on the GPU's own rows for every arm
    assert np.array_equal(arr[inc], ref["arrived"][inc]), np.flatnonzero(inc & (arr != ref["arrived"]))
    own = np.where(ua, _first_pass(q_ref, got["q_traj"], prec, stride), -1)
    assert np.array_equal(arr, own), np.flatnonzero(arr != own)
    assert np.all(arr[~ua] == -1)
    # the path.  With hold an arm that arrives at another check than the oracle's stops elsewhere: included arms only
    rows = inc if hold else np.ones(B, dtype=bool)
    eq = np.abs(got["q_traj"][:, rows].astype(np.float64) - ref["q_traj"][:, rows])
    eq = eq[~np.isnan(eq)]
    print("q_traj max error %.3e (tolerance %.1e)" % (eq.max(), tol_q))
    assert eq.max() < tol_q
    assert np.array_equal(np.isnan(got["q_traj"]), np.isnan(ref["q_traj"]))
    # pending: exactly the count its own arrived[] implies, and the oracle's up to the left-out arms
    cyc = (np.arange(n_checks) + 1) * stride - 1
    mine = np.array([np.count_nonzero(ua & ((arr < 0) | (arr > c))) for c in cyc])
    assert np.array_equal(got["pending"], mine)
    assert np.abs(got["pending"].astype(np.int64) - ref["pending"]).max() <= np.count_nonzero(out & ua)
    assert np.array_equal(got["q"], got["q_traj"][-1])
    # gated arms: every row carries their start
    assert np.all(got["q_traj"][:, ~ua] == q0[~ua].astype(io_dtype))
    # hold: a held arm's rows after its arrival are its arrival row, bit for bit
    last = np.full(B, n_checks - 1)
    if hold:
        for b in np.flatnonzero(arr >= 0):
            k = (arr[b] + 1) // stride - 1
            last[b] = k
            assert np.all(got["q_traj"][k:, b] == got["q_traj"][k, b]), b
    # diff: (T)(ref - q) of the last check the arm ran, bit for bit; a gated arm's row is never written
    want = (q_ref - got["q_traj"][last, np.arange(B)].astype(np.float64)).astype(io_dtype)
    want[~ua] = 0
    assert got["diff"].dtype == io_dtype and np.array_equal(got["diff"], want, equal_nan=True)
    ed = np.abs(got["diff"][rows].astype(np.float64) - ref["diff"][rows])
    assert ed[~np.isnan(ed)].max() < 2 * tol_q
    # every arm's output rows are those of its last evaluated cycle
    ev = np.abs(got["qdot_out"][rows].astype(np.float64) - ref["qdot_out"][rows]).max()
    print("qdot_out max error %.3e (tolerance %.1e)" % (ev, tol_v))
    assert ev < tol_v
    return inc


def _goto(eng, q0, q_ref, stride, hold, active=None, **kw):
    q_in, r_in = q0.astype(eng.io_dtype), q_ref.astype(eng.io_dtype)
    keep, keep_r = q_in.copy(), r_in.copy()
    got = eng.goto_js_host(q_in, r_in, N_CYCLES, DT, _prec(q0.shape[1]), stride=stride, hold=hold, clamp=True, trajectory=True,
                           want=("qdot_out", "status"), active=active, **kw)
    assert np.array_equal(q_in, keep) and np.array_equal(r_in, keep_r, equal_nan=True)   # io->q and io->q_ref are never written
    assert "dist_traj" not in got
    return got


def test_basic_stride_1(env):
    """lwr, float64, 200 arms (three full waves and a partial one), a check after every cycle, no hold."""
    chain, w, q0, q_ref, active, mixw, params, ref = _reference(env, "lwr", 200, 1, False)
    assert np.count_nonzero(ref["arrived"] >= 0) >= 0.99 * 200 and len(set(ref["arrived"])) > 10
    eng = _engine(env, chain, 200, np.float64, params, w)
    got = _goto(eng, q0, q_ref, 1, False)
    _check(got, ref, q0, q_ref, 1, False, np.float64)
    eng.close()


@pytest.mark.parametrize("robot", ["lwr", "lwr_dual14", "powercube6"])
def test_hold_stride_4(env, robot):
    """Checks every 4 cycles, arrived arms held, 130 arms: lwr (blocks are in-kernel rollouts), lwr_dual14 (stepped launches: q is handed
    over in the I/O type every cycle) and powercube6."""
    chain, w, q0, q_ref, active, mixw, params, ref = _reference(env, robot, 130, 4, True)
    print("oracle: %d arms arrive, at %d distinct checks" % (np.count_nonzero(ref["arrived"] >= 0), len(set(ref["arrived"]))))
    assert np.count_nonzero(ref["arrived"] >= 0) >= 100
    eng = _engine(env, chain, 130, np.float64, params, w)
    got = _goto(eng, q0, q_ref, 4, True)
    _check(got, ref, q0, q_ref, 4, True, np.float64)
    eng.close()


def test_float32_hold_stride_4(env):
    """float32 I/O, 203 arms (q rows of 5684 bytes: every second row of the trace is not 16-byte aligned), stride 4, hold."""
    B = 203
    chain, w, q0, q_ref, active, mixw, params, ref = _reference(env, "lwr", B, 4, True, io_dtype=np.float32)
    eng = _engine(env, chain, B, np.float32, params, w)
    got = _goto(eng, q0, q_ref, 4, True)
    _check(got, ref, q0, q_ref, 4, True, np.float32)
    eng.close()


def test_mixed_fleet(env):
    """Per-arm mixer weights: even arms under joint control, odd arms under Cartesian control with a reference row that starts with NaN
    (no controller); every third arm gated by the caller; nullspace module and mixer."""
    B = 200
    chain, w, q0, q_ref, active, mixw, params, ref = _reference(env, "lwr", B, 4, True, mixed=True)
    eng = _engine(env, chain, B, np.float64, params, w, mixw)
    got = _goto(eng, q0, q_ref, 4, True, active=active)
    _check(got, ref, q0, q_ref, 4, True, np.float64, active=active)
    ua = active != 0
    odd = np.arange(B) % 2 == 1
    arr = got["arrived"]
    # arms without a controller run (their tool follows the field), never arrive and count in pending
    assert np.all(arr[odd] == -1)
    moved = np.abs(got["q"][odd & ua] - q0[odd & ua]).max(axis=1)
    assert np.all(moved > 1e-6)
    assert got["pending"][-1] >= np.count_nonzero(odd & ua)
    assert np.all(np.isnan(got["diff"][odd & ua, 0])) and not np.isnan(got["diff"][odd & ua, 1:]).any()
    # gated arms carry their start, are not counted, and nothing was ever stored for them
    assert np.all(arr[~ua] == -1) and np.all(got["q_traj"][:, ~ua] == q0[~ua]) and got["pending"][0] <= np.count_nonzero(ua)
    assert np.all(got["status"][~ua] == 0) and np.all(got["qdot_out"][~ua] == 0) and np.all(got["diff"][~ua] == 0)
    assert np.count_nonzero(arr[~odd & ua] >= 0) >= 0.9 * np.count_nonzero(~odd & ua)
    eng.close()


@pytest.mark.parametrize("io_dtype", [np.float64, np.float32])
def test_decision_edges(env, io_dtype):
    """The rule at its edges, exactly.  n_cycles = stride = 1, dt = 0, clamp off: the block returns q0 (asserted bit for bit), so the
    check decides on the start the test chose.  4000 draws of ref = U(-2, 2) and prec = U(0.001, 0.3) on joint 0 (default_rng(3)), the
    other joints at their reference; prec is one host array per call, so every draw is a call of four arms that start at the edge
    fl(ref - prec), at its neighbour below, at fl(ref + prec) and at its neighbour above (float32: the nearest representable values inside
    and outside the edges, which are computed in double on the float32 reference).  Expected: arrive / not / arrive / not."""
    T = np.dtype(io_dtype)
    chain = env.robots.by_name("lwr")
    n, N = chain.n, 4000
    rng = np.random.default_rng(3)
    ref0 = rng.uniform(-2.0, 2.0, N).astype(T).astype(np.float64)
    prec0 = rng.uniform(0.001, 0.3, N)
    lo, hi = ref0 - prec0, ref0 + prec0
    lo_in = lo.astype(T)
    lo_in = np.where(lo_in.astype(np.float64) < lo, np.nextafter(lo_in, T.type(np.inf)), lo_in)
    hi_in = hi.astype(T)
    hi_in = np.where(hi_in.astype(np.float64) > hi, np.nextafter(hi_in, T.type(-np.inf)), hi_in)
    starts = np.stack([lo_in, np.nextafter(lo_in, T.type(-np.inf)), hi_in, np.nextafter(hi_in, T.type(np.inf))], axis=1).astype(T)   # (N, 4)
    expect = np.array([True, False, True, False])
    if T == np.float64:
        assert np.array_equal(starts[:, 0], lo) and np.array_equal(starts[:, 2], hi)
        with np.errstate(invalid="ignore"):
            fabs = np.abs(ref0[:, None] - starts) <= prec0[:, None]
        wrong = np.count_nonzero(fabs != expect[None, :], axis=0)
        print("rows an fabs(ref - q) <= prec rule gets wrong: %s of %d each" % (list(wrong), N))
        assert wrong.sum() >= 1000
    w = env.synth.make_workload(chain, 4, 3, seed=53, io_dtype=T.type)
    eng = _engine(env, chain, 4, T.type, _params(env), w)
    base = np.random.default_rng(4).uniform(0.5 * chain.q_lo, 0.5 * chain.q_hi, n).astype(T)
    q_ref = np.tile(base, (4, 1))
    q0 = q_ref.copy()
    prec = np.full(n, 0.01)
    arrived = np.zeros((N, 4), dtype=np.int32)
    for i in range(N):
        q_ref[:, 0] = ref0[i]
        q0[:, 0] = starts[i]
        prec[0] = prec0[i]
        got = eng.goto_js_host(q0, q_ref, 1, 0.0, prec, stride=1, hold=False, clamp=False, want=())
        assert np.array_equal(got["q"], q0), i
        arrived[i] = got["arrived"]
    bad = np.flatnonzero(np.any((arrived == 0) != expect[None, :], axis=1))
    assert np.all((arrived == 0) | (arrived == -1))
    assert len(bad) == 0, (len(bad), bad[:5], arrived[bad[:5]])
    eng.close()


def test_early_exit(env):
    """Only arms the oracle shows arriving: a call of 4000 cycles that polls every 2 checks ends a poll after the last arrival, and gives
    what the un-polled call of as many checks gives, bit for bit."""
    chain, w, q0, q_ref, active, mixw, params, ref = _reference(env, "lwr", 130, 4, True)
    out = _left_out(ref, np.ones(130, dtype=bool), np.float64)
    sel = np.flatnonzero(ref["arrived"] >= 0)
    assert len(sel) >= 100
    last = int((ref["arrived"][sel].max() + 1) // 4 - 1)   # the oracle's last arrival check
    bound = (last + 2 + 1) // 2 * 2 + (2 if out[sel].any() else 0)
    eng = env.engine.Engine(chain, len(sel), io_dtype=np.float64, max_slots=8, params=params)
    eng.set_fields(w["fields"][sel], w["nfields"][sel])
    kw = dict(stride=4, hold=True, clamp=True, trajectory=True, want=("qdot_out", "status"))
    a = eng.goto_js_host(q0[sel], q_ref[sel], 4000, DT, _prec(7), poll=2, **kw)
    print("checks_run %d (oracle's last arrival at check %d, bound %d)" % (a["checks_run"], last, bound))
    assert 0 < a["checks_run"] <= bound and a["checks_run"] % 2 == 0
    assert a["pending"].shape == (a["checks_run"],) and a["pending"][-1] == 0 and np.all(a["arrived"] >= 0)
    assert a["q_traj"].shape[0] == a["checks_run"]
    b = eng.goto_js_host(q0[sel], q_ref[sel], a["checks_run"] * 4, DT, _prec(7), poll=0, **kw)
    assert b["checks_run"] == a["checks_run"]
    for k in ("q", "arrived", "pending", "q_traj", "diff", "qdot_out", "status"):
        assert np.array_equal(a[k], b[k]), k
    eng.close()


def test_argument_errors(env):
    """Every refused call returns VFIK_E_ARG, enqueues nothing, leaves the launch epoch and the outputs as they were, and the engine able
    to give the basic case's result."""
    chain, w, q0, q_ref, active, mixw, params, ref = _reference(env, "lwr", 200, 1, False)
    eng = _engine(env, chain, 200, np.float64, params, w)
    B, n = q0.shape
    arrived = np.full(B, 7, dtype=np.int32)
    diff = np.full((B, n), 7.0)
    q_out = np.full((B, n), 7.0)
    dummy = np.zeros((B, 16))
    good = _prec(n)

    def call(null_opts=False, prec=good, **kw):
        io = env.engine.IO()
        io.q, io.q_ref = q0.ctypes.data, q_ref.ctypes.data
        o = env.abi.GotoJsOpts()
        o.n_cycles, o.stride, o.dt, o.arrived, o.diff, o.q_out = 80, 4, DT, arrived.ctypes.data, diff.ctypes.data, q_out.ctypes.data
        p = None if prec is None else np.ascontiguousarray(prec, dtype=np.float64)
        o.prec = None if p is None else p.ctypes.data
        for k, v in kw.items():
            setattr(io if hasattr(io, k) else o, k, v)
        return eng.lib.vfik_goto_js_host(eng.h, C.byref(io), None if null_opts else C.byref(o), 0, None)

    def with_prec(i, v):
        p = good.copy()
        p[i] = v
        return p

    epoch = eng.launch_epoch
    bad = [dict(null_opts=True), dict(arrived=None), dict(stride=0), dict(stride=-4), dict(n_cycles=0), dict(n_cycles=1000004), dict(n_cycles=10),
           dict(dt=float("nan")), dict(dt=float("inf")), dict(q_cmded=dummy.ctypes.data), dict(track_error=dummy.ctypes.data),
           dict(obj_dist=dummy.ctypes.data), dict(q_lo=dummy.ctypes.data), dict(q=None),
           dict(q_ref=None), dict(prec=None), dict(prec=with_prec(0, -1e-3)), dict(prec=with_prec(n - 1, -1e-3)),
           dict(prec=with_prec(3, float("nan"))), dict(prec=with_prec(0, -float("inf")))]
    for kw in bad:
        rc = call(**kw)
        assert rc == -1, (kw, rc, eng.lib.vfik_last_error())   # VFIK_E_ARG
        with pytest.raises(env.engine.VfikError):
            eng._chk(rc)
    assert eng.launch_epoch == epoch
    assert np.all(arrived == 7) and np.all(diff == 7.0) and np.all(q_out == 7.0)
    with pytest.raises(env.engine.VfikError):
        eng.goto_js_host(q0, q_ref, 10, DT, good, stride=4)
    with pytest.raises(ValueError):
        eng.goto_js_host(q0, q_ref, 80, DT, good[:-1])
    with pytest.raises(ValueError):
        eng.goto_js_host(q0, None, 80, DT, good)
    assert call(prec=with_prec(2, float("inf"))) == 0      # +inf is allowed: that joint never decides
    assert np.all((arrived == -1) | ((arrived + 1) % 4 == 0))
    assert eng.launch_epoch == epoch
    got = _goto(eng, q0, q_ref, 1, False)
    _check(got, ref, q0, q_ref, 1, False, np.float64)
    eng.close()


@pytest.mark.parametrize("robot", ["lwr", "lwr_dual14"])
def test_only_the_kernels_of_a_rollout_with_q_ref(env, robot):
    """A joint-space goto launches the cycle kernels a gated vfik_rollout with the same q_ref launches (it asks for no goal_dist), and
    moves nothing a captured launch depends on."""
    chain, w, q0, q_ref = _case(env, robot, 130)
    eng = _engine(env, chain, 130, np.float64, _params(env), w)
    eng.launched_kernels()
    eng.rollout_host(q0, 4, DT, clamp=True, q_ref=q_ref, active=np.ones(130, dtype=np.int32))
    of_rollout = eng.launched_kernels()
    epoch = eng.launch_epoch
    got = eng.goto_js_host(q0, q_ref, 16, DT, _prec(chain.n), stride=4, hold=True, clamp=True)
    assert got["checks_run"] == 4
    names = eng.launched_kernels()
    built = {v.name for v in kv.library_variants()}
    assert names and names <= of_rollout, names - of_rollout
    for nm in names:
        assert kv.parse(nm).kernel.startswith("cycle_") and nm in built, nm
    assert eng.launch_epoch == epoch
    eng.close()


def test_device_form_equals_host_form(env):
    """Engine.goto_js on torch tensors (rows of the float32 trace that are not 16-byte aligned) gives the host form's arrays."""
    import torch
    B = 131
    chain, w, q0, q_ref = _case(env, "lwr", B, np.float32)
    eng = _engine(env, chain, B, np.float32, _params(env), w)
    prec = _prec(7)
    host = eng.goto_js_host(q0, q_ref, 48, DT, prec, stride=4, hold=True, clamp=True, trajectory=True, want=("qdot_out",))
    dev = torch.device("cuda", 0)
    q = torch.from_numpy(q0.astype(np.float32)).to(dev)
    r = torch.from_numpy(q_ref.astype(np.float32)).to(dev)
    t = dict(arrived=torch.zeros(B, dtype=torch.int32, device=dev), pending=torch.full((12,), 7, dtype=torch.int32, device=dev),
             q_out=torch.zeros(B, 7, device=dev), q_traj=torch.zeros(12, B, 7, device=dev), diff=torch.zeros(B, 7, device=dev))
    qd = torch.zeros(B, 7, device=dev)
    torch.cuda.synchronize()
    eng.goto_js(eng.make_io(q, q_ref=r, qdot_out=qd), 48, DT, prec, stride=4, hold=True, clamp=True, **t)
    eng.sync()
    for k, hk in (("arrived", "arrived"), ("pending", "pending"), ("q_out", "q"), ("q_traj", "q_traj"), ("diff", "diff")):
        assert np.array_equal(t[k].cpu().numpy(), host[hk]), k
    assert np.array_equal(qd.cpu().numpy(), host["qdot_out"]) and np.array_equal(q.cpu().numpy(), q0.astype(np.float32))
    assert np.array_equal(r.cpu().numpy(), q_ref.astype(np.float32))
    with pytest.raises(env.engine.VfikError):
        eng.goto_js(eng.make_io(q, qdot_out=qd), 48, DT, prec, stride=4, **t)      # no q_ref
    eng.close()


def test_sharded_goto_js_equals_single_engine(env):
    """ShardedEngine over devices (0, 0): two handles give the single engine's result on the whole batch."""
    chain, w, q0, q_ref, active, mixw, params, ref = _reference(env, "lwr", 130, 4, True)
    eng = _engine(env, chain, 130, np.float64, params, w)
    one = _goto(eng, q0, q_ref, 4, True)
    eng.close()
    sh = env.sharding.ShardedEngine(chain, 130, rank=0, world=1, devices=(0, 0), io_dtype=np.float64, max_slots=8, params=params)
    sh.set_fields(w["fields"], w["nfields"])
    two = sh.goto_js_host(q0, q_ref, N_CYCLES, DT, _prec(7), stride=4, hold=True, clamp=True, trajectory=True, want=("qdot_out", "status"))
    sh.close()
    assert two["checks_run"] == one["checks_run"]
    for k in ("q", "arrived", "pending", "q_traj", "diff", "qdot_out", "status"):
        assert np.array_equal(one[k], two[k]), k
