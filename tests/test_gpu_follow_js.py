"""Posture lists (include/vfik.h: vfik_follow_js / vfik_follow_js_host: a script of set_ref_js calls, handlers.py:544-576, for the batch)
on the GPU against their restatement with the oracle (tests/timed_reference.py: follow_js): which arm reaches which posture at which check, the
posture index every check was made against, the joint path, `diff`, the count of arms under way, lists of different lengths, an arm
without a list, and what the call leaves of the handle.

Inputs: synth.make_workload(chain, B, 3, seed=53); W = 3 postures per arm: posture 0 = U(0.7 q_lo, 0.7 q_hi), every further one a step of
+-U(0.1, 0.2) rad on every joint (turned round where it would leave 0.7 x the limits); arms 3, 13, 23, ... have 2 postures, arms 7, 17, ...
have 1, arm 5 has none; the start at posture 0 + s U(-1, 1), s = U(0.02, 0.2) per arm; default_rng(7).  jp_kp 8, dt 0.01, 160 cycles,
clamp on, prec[i] = 0.004 + 0.002 i at the last posture, 3 x that at those before it, mixer [0, 0, 1, 0, 0, 0] with F_MIXER.

Margins and caps as tests/test_gpu_goto_js.py, asserted on the helper's `closest`.  EVERY arm is held to the state machine replayed with
the helper's rule on the GPU's own q rows: reached, next and way_traj are exact there."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import timed_reference as jr  # noqa: E402

pytestmark = pytest.mark.gpu

N_CYCLES, DT, KP, W = 160, 0.01, 8.0, 3
MIX_JOINT = [0.0, 0.0, 1.0, 0.0, 0.0, 0.0]
MARGIN = {np.dtype(np.float64): (1e-7, 0.05), np.dtype(np.float32): (4e-6, 0.10)}
TOL = {np.dtype(np.float64): (1e-8, 1e-7), np.dtype(np.float32): (2e-6, 2e-5)}   # q_traj, qdot_out


def _prec(n):
    return 0.004 + 0.002 * np.arange(n)


@pytest.fixture(scope="module")
def env():
    import __graft_entry__ as g
    g.build()
    from oracle import oracle_c
    from vfclik_amd import _abi, engine, robots, synth

    class E:
        pass

    e = E()
    e.oc, e.abi, e.engine, e.robots, e.synth = oracle_c, _abi, engine, robots, synth
    e.cache = {}
    return e


def _case(env, robot, B, io_dtype=np.float64):
    """The inputs of the module's docstring."""
    chain = env.robots.by_name(robot)
    n = chain.n
    w = env.synth.make_workload(chain, B, 3, seed=53, io_dtype=io_dtype)
    rng = np.random.default_rng(7)
    lo, hi = 0.7 * chain.q_lo, 0.7 * chain.q_hi
    wayq = np.zeros((B, W, n))
    wayq[:, 0] = rng.uniform(lo, hi, size=(B, n))
    for i in range(1, W):
        step = rng.uniform(0.1, 0.2, size=(B, n)) * rng.choice([-1.0, 1.0], size=(B, n))
        nxt = wayq[:, i - 1] + step
        wayq[:, i] = np.where((nxt < lo) | (nxt > hi), wayq[:, i - 1] - step, nxt)
    s = rng.uniform(0.02, 0.2, size=(B, 1))
    q0 = (wayq[:, 0] + s * rng.uniform(-1.0, 1.0, size=(B, n))).astype(io_dtype).astype(np.float64)
    wayq[3::10, 2] = np.nan
    wayq[7::10, 1, 0] = np.nan        # (the first element alone ends the list; the row behind it does not count either)
    wayq[5] = np.nan
    wayq = wayq.astype(io_dtype).astype(np.float64)
    return chain, w, q0, wayq


def _params(env):
    return env.abi.default_params(flags=env.abi.F_MIXER, mix_w=MIX_JOINT, jp_kp=KP)


def _reference(env, robot, B, stride, hold, io_dtype=np.float64, active=None):
    """The oracle's run of a case, computed once per module and never modified."""
    key = (robot, B, stride, hold, np.dtype(io_dtype).name, None if active is None else active.tobytes())
    if key not in env.cache:
        chain, w, q0, wayq = _case(env, robot, B, io_dtype)
        params = _params(env)
        p = _prec(chain.n)
        out = jr.follow_js(env.oc, chain, params, q0, w["fields"], w["nfields"], wayq, N_CYCLES, stride, DT, p, via_prec=3 * p, hold=hold,
                           clamp=True, active=active, io_dtype=io_dtype, want=("qdot_out",), stepped=chain.n > 7)
        for v in out.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        env.cache[key] = (chain, w, q0, wayq, params, out)
    return env.cache[key]


def _engine(env, chain, B, io_dtype, params, w):
    eng = env.engine.Engine(chain, B, io_dtype=io_dtype, max_slots=8, params=params)
    eng.set_fields(w["fields"], w["nfields"])
    return eng


def _follow(eng, q0, wayq, stride, hold, **kw):
    p = _prec(q0.shape[1])
    q_in = q0.astype(eng.io_dtype)
    keep = q_in.copy()
    got = eng.follow_js_host(q_in, wayq, N_CYCLES, DT, p, via_precision=3 * p, stride=stride, hold=hold, clamp=True, trajectory=True,
                             want=("qdot_out", "status"), **kw)
    assert np.array_equal(q_in, keep) and "dist_traj" not in got
    return got


def _replay(wayq, L, q_traj, stride, hold, prec, via, ua=None):
    """The helper's state machine on given q rows: (reached, next, way_traj, last check every arm ran).  ua: the caller's gate as
    booleans (None: every arm)."""
    n_checks, B, n = q_traj.shape
    kind = jr.list_kind(wayq, jr.POSTURE)
    assert np.array_equal(jr.lengths(kind), L)
    m = jr.replay(kind, wayq, np.ones(B, dtype=bool), q_traj, None, n_checks * stride, stride, (0.0, 0.0), prec, js_via_precision=via,
                  hold=hold, active=ua)
    return m.reached, m.next, m.way_traj, m.last_ran


def _check(got, ref, q0, wayq, stride, hold, io_dtype, active=None, n_checks=None):
    """active: the caller's gate of the run (None: every arm); n_checks: the checks the call is to have run (None: all of N_CYCLES), with
    `ref` then cut to as many."""
    io_dtype = np.dtype(io_dtype)
    B, n = q0.shape
    prec = _prec(n)
    n_checks = N_CYCLES // stride if n_checks is None else n_checks
    L = jr.list_lengths(wayq)
    assert np.array_equal(L, ref["length"]) and set(L) == {0, 1, 2, 3}
    ua = np.ones(B, dtype=bool) if active is None else active != 0
    part = (L > 0) & ua
    margin, cap = MARGIN[io_dtype]
    out = ref["closest"] < margin
    share = np.count_nonzero(out & part) / np.count_nonzero(part)
    print("left out: %d of %d arms (%.1f %%, cap %.0f %%)" % (np.count_nonzero(out & part), np.count_nonzero(part), 100 * share, 100 * cap))
    assert share <= cap, share
    done = ref["next"] == L
    print("oracle: %d of %d arms reach their last posture; %d decisions" % (np.count_nonzero(done & part), np.count_nonzero(part), ref["next"].sum()))
    assert np.count_nonzero(done & part) >= 0.9 * np.count_nonzero(part)
    inc = ~out
    tol_q, tol_v = TOL[io_dtype]
    assert got["checks_run"] == n_checks
    # against the oracle outside the margin
    for k in ("reached", "next"):
        assert np.array_equal(got[k][inc], ref[k][inc]), (k, np.flatnonzero(inc & np.any(np.atleast_2d(got[k].T != ref[k].T), axis=0)))
    assert np.array_equal(got["way_traj"][:, inc], ref["way_traj"][:, inc])
    # every arm against the state machine on the GPU's own rows
    r, nx, wt, last_ran = _replay(wayq, L, got["q_traj"], stride, hold, prec, 3 * prec, ua)
    assert np.array_equal(got["reached"], r) and np.array_equal(got["next"], nx) and np.array_equal(got["way_traj"], wt)
    rows = inc if hold else np.ones(B, dtype=bool)
    eq = np.abs(got["q_traj"][:, rows].astype(np.float64) - ref["q_traj"][:, rows]).max()
    print("q_traj max error %.3e (tolerance %.1e)" % (eq, tol_q))
    assert eq < tol_q
    # pending: the arms that take part and have postures left, from its own reached[]
    cyc = (np.arange(n_checks) + 1) * stride - 1
    fin = got["reached"][np.arange(B), np.maximum(L - 1, 0)]
    mine = np.array([np.count_nonzero(part & ((fin < 0) | (fin > c))) for c in cyc])
    assert np.array_equal(got["pending"], mine)
    assert np.array_equal(got["q"], got["q_traj"][-1])
    # the arm without a list, and one the caller gates off, is kept out: its rows carry its start, nothing is stored for it
    assert np.all(got["q_traj"][:, ~part] == q0[~part].astype(io_dtype)) and np.all(got["way_traj"][:, ~part] == -1)
    assert np.all(got["reached"][~part] == -1) and np.all(got["next"][~part] == 0)
    assert np.all(got["status"][~part] == 0) and np.all(got["qdot_out"][~part] == 0) and np.all(got["diff"][~part] == 0)
    if hold:   # an arm at its last posture repeats its rows, bit for bit
        for b in np.flatnonzero(part & (got["next"] == L)):
            k = (fin[b] + 1) // stride - 1
            assert np.all(got["q_traj"][k:, b] == got["q_traj"][k, b]) and np.all(got["way_traj"][k:, b] == L[b] - 1), b
    # diff: (T)(posture - q) of the last check the arm ran, against the posture that check was made against, bit for bit
    a = np.flatnonzero(part)
    want = np.zeros((B, n), dtype=io_dtype)
    want[a] = (wayq[a, got["way_traj"][last_ran[a], a]] - got["q_traj"][last_ran[a], a].astype(np.float64)).astype(io_dtype)
    assert got["diff"].dtype == io_dtype and np.array_equal(got["diff"], want)
    ev = np.abs(got["qdot_out"][rows].astype(np.float64) - ref["qdot_out"][rows]).max()
    print("qdot_out max error %.3e (tolerance %.1e)" % (ev, tol_v))
    assert ev < tol_v


@pytest.mark.parametrize("robot,B,stride,hold,io_dtype", [("lwr", 200, 1, False, np.float64), ("lwr", 203, 4, True, np.float32),
                                                          ("lwr_dual14", 130, 4, True, np.float64)])
def test_follow_js(env, robot, B, stride, hold, io_dtype):
    """lwr float64 with a check after every cycle; lwr float32 with 203 arms (rows that are not 16-byte aligned), stride 4 and hold;
    lwr_dual14 (stepped blocks) with stride 4 and hold."""
    chain, w, q0, wayq, params, ref = _reference(env, robot, B, stride, hold, io_dtype)
    eng = _engine(env, chain, B, io_dtype, params, w)
    got = _follow(eng, q0, wayq, stride, hold)
    _check(got, ref, q0, wayq, stride, hold, io_dtype)
    eng.close()


@pytest.mark.parametrize("poll", [0, 8])
@pytest.mark.parametrize("io_dtype", [np.float32, np.float64])
def test_traced_under_a_gate_and_early_exit(env, io_dtype, poll):
    """lwr, 203 arms, W = 3, stride 4, hold, with traces, under the caller's gate (arms 2, 9, 16, ... off) and with arm 5 without a list;
    once to the end and once polled every 8 checks.  The oracle (on the CPU) has every arm that takes part finish its list by check 28 of
    40, with arms under way at the polls before: the polled call ends after 32 checks.  An early end comes only once no arm that takes part
    is under way (pending == 0), so what is still short of its list then are the arms the gate keeps out -- they have postures left and
    must come back untouched.  With hold every arm stands still from the check that found it at its last posture, so the oracle's run
    cut to the checks that ran is the oracle's run of as many checks."""
    B, stride, hold = 203, 4, True
    active = np.ones(B, dtype=np.int32)
    active[2::7] = 0
    chain, w, q0, wayq, params, ref = _reference(env, "lwr", B, stride, hold, io_dtype, active)
    n_checks = N_CYCLES // stride
    L, ua = ref["length"], active != 0
    part = ua & (L > 0)
    zero = np.flatnonzero(ref["pending"] == 0)
    assert np.count_nonzero(ref["next"][part] == L[part]) >= 1 and np.any(~ua & (L > 0)) and np.all(ref["next"][~ua] == 0)
    assert len(zero) and ref["pending"][7] > 0 and ref["pending"][zero[0] - 1] > 0
    want_run = n_checks if poll == 0 else (zero[0] + 1 + poll - 1) // poll * poll
    assert poll == 0 or want_run < n_checks
    # an arm whose decision lies within the margin may be found a check later than the oracle finds it: none of them is among the last
    near = part & (ref["closest"] < MARGIN[np.dtype(io_dtype)][0])
    assert not near.any() or ref["reached"][near].max() + 3 * stride < (zero[0] + 1) * stride
    eng = _engine(env, chain, B, io_dtype, params, w)
    got = _follow(eng, q0, wayq, stride, hold, active=active, poll=poll)
    print("checks_run %d of %d (the oracle's pending is 0 from check %d on)" % (got["checks_run"], n_checks, zero[0]))
    assert got["checks_run"] == want_run
    for k in ("pending", "q_traj", "way_traj"):
        assert got[k].shape[0] == want_run, k
    assert got["pending"][-1] == 0 and (poll == 0 or got["pending"][want_run - poll - 1] > 0)   # under way at the poll before the last
    cut = dict(ref)
    for k in ("pending", "q_traj", "way_traj"):
        cut[k] = ref[k][:want_run]
    _check(got, cut, q0, wayq, stride, hold, io_dtype, active=active, n_checks=want_run)
    eng.close()


def test_one_posture_equals_goto_js(env):
    """W = 1 is vfik_goto_js, bit for bit -- with a list that is a view of a larger array (element-aligned, no more)."""
    chain, w, q0, wayq = _case(env, "lwr", 131, np.float32)
    sel = np.flatnonzero(~np.isnan(wayq[:, 0, 0]))
    q0, q_ref = q0[sel], wayq[sel, 0]
    eng = env.engine.Engine(chain, len(sel), io_dtype=np.float32, max_slots=8, params=_params(env))
    eng.set_fields(w["fields"][sel], w["nfields"][sel])
    p = _prec(7)
    kw = dict(stride=4, hold=True, clamp=True, trajectory=True, want=("qdot_out", "status"))
    g = eng.goto_js_host(q0, q_ref, 80, DT, p, **kw)
    f = eng.follow_js_host(q0, q_ref[:, None, :], 80, DT, p, via_precision=10 * p, **kw)
    assert np.array_equal(f["reached"][:, 0], g["arrived"]) and np.array_equal(f["next"], (g["arrived"] >= 0).astype(np.int32))
    for k in ("q", "pending", "q_traj", "diff", "qdot_out", "status"):
        assert np.array_equal(f[k], g[k]), k
    assert np.count_nonzero(g["arrived"] >= 0) > 60 and np.all(f["way_traj"] == 0)
    eng.close()


def test_the_handle_is_left_as_it_was(env):
    """Across a follow_js the launch epoch does not move, the goal image is untouched (goal_dist of a following step equals the one before
    the call at equal q), and a plain step with the caller's own q_ref behaves as before: the handle's reference row is read by nobody else."""
    chain, w, q0, wayq, params, ref = _reference(env, "lwr", 200, 1, False)
    eng = _engine(env, chain, 200, np.float64, params, w)
    own_ref = np.random.default_rng(11).uniform(0.5 * chain.q_lo, 0.5 * chain.q_hi, q0.shape)
    want = ("qdot_out", "goal_dist", "q_ref_out", "status")
    before = eng.step_host(q0, q_ref=own_ref, want=want)
    before_plain = eng.step_host(q0, want=("qdot_out", "goal_dist"))
    epoch, path, slots = eng.launch_epoch, eng.field_path, eng.slots_in_use
    got = _follow(eng, q0, wayq, 4, True)
    assert got["next"].sum() > 200
    assert (eng.launch_epoch, eng.field_path, eng.slots_in_use) == (epoch, path, slots)
    after = eng.step_host(q0, q_ref=own_ref, want=want)
    after_plain = eng.step_host(q0, want=("qdot_out", "goal_dist"))
    for k in want:
        assert np.array_equal(before[k], after[k]), k
    for k in ("qdot_out", "goal_dist"):
        assert np.array_equal(before_plain[k], after_plain[k]), k
    assert np.abs(before["qdot_out"] - KP * (own_ref - q0)).max() < 1e-12     # ... and it is the caller's reference that drives
    eng.close()


def test_argument_errors_and_device_form(env):
    """What vfik_follow_js refuses beyond vfik_goto's list; then Engine.follow_js on torch tensors equals the host form."""
    import ctypes as C
    import torch
    chain, w, q0, wayq, params, ref = _reference(env, "lwr", 200, 1, False)
    B, n = q0.shape
    eng = _engine(env, chain, B, np.float64, params, w)
    reached = np.full((B, W), 7, dtype=np.int32)
    nxt = np.full(B, 7, dtype=np.int32)
    good = _prec(n)

    def call(prec=good, via=None, **kw):
        io = env.engine.IO()
        io.q = q0.ctypes.data
        o = env.abi.FollowJsOpts()
        o.n_cycles, o.stride, o.dt, o.n_way = 16, 4, DT, W
        o.wayq, o.reached, o.next = wayq.ctypes.data, reached.ctypes.data, nxt.ctypes.data
        keep = [None if a is None else np.ascontiguousarray(a, dtype=np.float64) for a in (prec, via)]
        o.prec, o.via_prec = (None if a is None else a.ctypes.data for a in keep)
        for k, v in kw.items():
            setattr(io if hasattr(io, k) else o, k, v)
        return eng.lib.vfik_follow_js_host(eng.h, C.byref(io), C.byref(o), 0, None)

    def with_prec(i, v):
        p = good.copy()
        p[i] = v
        return p

    epoch = eng.launch_epoch
    bad = [dict(q_ref=q0.ctypes.data), dict(prec=None), dict(prec=with_prec(1, -1.0)), dict(prec=with_prec(6, float("nan"))),
           dict(via=with_prec(0, -1.0)), dict(via=with_prec(2, float("nan"))), dict(n_way=0), dict(wayq=None), dict(reached=None), dict(next=None),
           dict(wayq=wayq.ctypes.data + 4), dict(stride=0), dict(n_cycles=10), dict(dt=float("nan")), dict(q_cmded=q0.ctypes.data)]
    for kw in bad:
        rc = call(**kw)
        assert rc == -1, (kw, rc, eng.lib.vfik_last_error())   # VFIK_E_ARG
    assert eng.launch_epoch == epoch and np.all(reached == 7) and np.all(nxt == 7)
    assert call() == 0 and np.all(nxt[jr.list_lengths(wayq) > 0] <= W) and nxt[5] == 0
    p = good
    host = eng.follow_js_host(q0, wayq, 48, DT, p, via_precision=3 * p, stride=4, hold=True, clamp=True, trajectory=True, want=("qdot_out",))
    dev = torch.device("cuda", 0)
    q = torch.from_numpy(q0).to(dev)
    wq = torch.from_numpy(wayq).to(dev)
    t = dict(reached=torch.zeros(B, W, dtype=torch.int32, device=dev), next=torch.full((B,), 7, dtype=torch.int32, device=dev),
             pending=torch.full((12,), 7, dtype=torch.int32, device=dev), q_out=torch.zeros(B, n, dtype=torch.float64, device=dev),
             q_traj=torch.zeros(12, B, n, dtype=torch.float64, device=dev), diff=torch.zeros(B, n, dtype=torch.float64, device=dev),
             way_traj=torch.full((12, B), -1, dtype=torch.int32, device=dev))
    qd = torch.zeros(B, n, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    eng.follow_js(eng.make_io(q, qdot_out=qd), wq, 48, DT, p, via_precision=3 * p, stride=4, hold=True, clamp=True, **t)
    eng.sync()
    for k, hk in (("reached", "reached"), ("next", "next"), ("pending", "pending"), ("q_out", "q"), ("q_traj", "q_traj"), ("diff", "diff"),
                  ("way_traj", "way_traj")):
        assert np.array_equal(t[k].cpu().numpy(), host[hk]), k
    assert np.array_equal(qd.cpu().numpy(), host["qdot_out"])
    assert np.array_equal(wq.cpu().numpy(), wayq, equal_nan=True)
    eng.close()
