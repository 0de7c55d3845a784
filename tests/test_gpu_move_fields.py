"""Goals and obstacles that move on the device (ABI 6: vfik_move_fields).  The object feeder re-sends every primitive of an object
whose pose changed (object_feeder:214-354); vfik_move_fields writes the new goal frame / x y z radius into the images vfik_set_fields
packed, with one kernel on the handle's stream.  The yardstick throughout: an engine that got the moved scene through set_fields
holds the same BYTES, runs the same kernel and so returns the same bits; both are held to the oracle as well."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LEAN = ("qdot_out", "status")
FULL = ("qdot_out", "qdot_vf", "qdot_null", "pose", "v6", "qdist", "goal_dist", "status")


@pytest.fixture(scope="module")
def env():
    import __graft_entry__ as g
    g.build()
    import torch
    from oracle import oracle_c
    from vfclik_amd import _abi, engine, robots, sharding, synth

    class E:
        pass

    e = E()
    e.oc, e.abi, e.engine, e.robots, e.synth, e.torch, e.sharding = oracle_c, _abi, engine, robots, synth, torch, sharding
    return e


def _rnd(a, dt):
    return np.asarray(a, dtype=np.float64).astype(dt).astype(np.float64)


def _round(w, dt):
    w["q"] = _rnd(w["q"], dt)
    w["fields"]["p"] = _rnd(w["fields"]["p"], dt)
    w["fields"]["force"] = _rnd(w["fields"]["force"], dt)
    return w


# ---- scenes -------------------------------------------------------------------------------------------------------------------
def _scene(env, chain, kind, B, nobs, dt, seed):
    """-> (workload, max_slots, expected field path, expected uniform image, expected mixed orders)"""
    rng = np.random.default_rng(seed + 1000)
    if kind in ("plain", "ragged"):
        w = env.synth.make_workload(chain, B, nobs, seed=seed, io_dtype=dt)
        if kind == "ragged":                     # a shorter list is a prefix; some arms have no obstacle at all
            w["nfields"][:] = 1 + rng.integers(0, nobs + 1, B)
            w["nfields"][:3] = (1, 1 + nobs, 1)
        return _round(w, dt), nobs, 1, True, False
    if kind == "pairs":                          # per-arm safe distance and force: the compact image
        w = env.synth.make_workload(chain, B, nobs, seed=seed, io_dtype=dt)
        w["fields"]["p"][:, 1:1 + nobs, 4] = rng.uniform(0.001, 0.01, (B, nobs))
        w["fields"]["force"][:, 1:1 + nobs] = rng.uniform(-12.0, -8.0, (B, nobs))
        return _round(w, dt), nobs, 1, False, False
    if kind == "mixed":                          # integer orders that differ
        w = env.synth.make_workload(chain, B, nobs, seed=seed, io_dtype=dt)
        w["fields"]["p"][:, 1:1 + nobs, 5] = np.array([5, 20, 2, 7, 1, 3, 13, 3, 20, 5, 4, 6])[:nobs]
        return _round(w, dt), nobs, 1, True, True
    if kind == "path2":                          # goalAndNormal + a table (object_feeder:248-303,344-353)
        w = env.synth.make_workload(chain, B, nobs, seed=seed, io_dtype=dt, max_fields=nobs + 4)
        F = w["fields"]
        i = 1 + nobs
        F["id"][:, i], F["type"][:, i], F["force"][:, i] = 2, 5, 30.0            # funnel: general slots 0, 1
        F["p"][:, i, 0:3] = F["p"][:, 0, [3, 7, 11]]
        F["p"][:, i, 3:6] = F["p"][:, 0, [2, 6, 10]]
        F["p"][:, i, 6:10] = [0.15, 10.0, 0.15, 2.0]
        F["id"][:, i + 1], F["type"][:, i + 1], F["force"][:, i + 1] = 3, 2, -10.0   # near-goal repeller: compact slot 0, general slot 2
        F["p"][:, i + 1, 0:3] = F["p"][:, 0, [3, 7, 11]] - 0.05 * F["p"][:, 0, [2, 6, 10]]
        F["p"][:, i + 1, 3:6] = [0.2, 0.001, 5.0]
        F["id"][:, i + 2], F["type"][:, i + 2], F["force"][:, i + 2] = 40, 4, -50.0  # a table for every third arm
        F["p"][:, i + 2] = 0.0
        F["p"][:, i + 2, 0:8] = [0.0, 0.0, -0.3, 0.02, -0.01, 1.0, 0.05, 5.0]
        w["nfields"][:] = nobs + 3
        w["nfields"][::3] = nobs + 4
        return _round(w, dt), nobs + 5, 2, True, False
    if kind == "fractional":                     # field path 0
        w = env.synth.make_workload(chain, B, nobs, seed=seed, io_dtype=dt)
        w["fields"]["p"][1::3, 3, 5] = 2.5
        return _round(w, dt), nobs, 0, False, False
    if kind == "attractor2":                     # field path 0; the second attractor's three slots come BEFORE the obstacles
        w = env.synth.make_workload(chain, B, nobs, seed=seed, io_dtype=dt, max_fields=nobs + 2)
        F = w["fields"]
        i = 1 + nobs
        F["id"][:, i], F["type"][:, i], F["force"][:, i] = 2, 1, 0.3
        qg = rng.uniform(0.5 * chain.q_lo, 0.5 * chain.q_hi, (B, chain.n))
        F["p"][:, i, :16] = chain.fk(qg).reshape(B, 16)
        F["p"][:, i, 16] = 0.05
        w["nfields"][:] = nobs + 2
        return _round(w, dt), nobs + 3, 0, False, False
    raise KeyError(kind)


def _layout(w, b):
    """(index of the goal entry or None, indices of the decay repellers in ascending-id order) of arm b"""
    F = w["fields"]
    idx = [k for k in range(w["nfields"][b]) if F["type"][b, k] != 0]
    idx.sort(key=lambda k: F["id"][b, k])            # (stable: ties keep the array order, as the library's sort does)
    goal = next((k for k in idx if F["type"][b, k] == 1), None)
    return goal, [k for k in idx if F["type"][b, k] == 2]


def _make_move(env, chain, w, dt, seed, goal=True, reps=True, n_rep=None, first=0, n=None, nan_frac=0.0, active=None):
    """-> (w2 = w with the moved numbers in p[], goal16 (n,16) or None, rep4 (n,n_rep,4) or None), everything rounded to dt"""
    rng = np.random.default_rng(seed + 2000)
    B = w["q"].shape[0]
    n = B - first if n is None else n
    F2 = w["fields"].copy()
    counts = [len(_layout(w, b)[1]) for b in range(B)]
    n_rep = max(counts) if n_rep is None else n_rep
    g16 = r4 = None
    tool_pos = chain.fk(w["q"]).reshape(B, 16)[:, [3, 7, 11]]
    if goal:
        qg = rng.uniform(0.8 * chain.q_lo, 0.8 * chain.q_hi, (B, chain.n))
        g16 = _rnd(chain.fk(qg).reshape(B, 16), dt)[first:first + n]
        g16[rng.uniform(size=n) < nan_frac, 0] = np.nan
    if reps:
        r4 = np.empty((n, n_rep, 4))
        r4[:, :, 0:2] = rng.uniform(-0.8, 0.8, (n, n_rep, 2))
        r4[:, :, 2] = rng.uniform(0.0, 1.2, (n, n_rep))
        r4[:, :, 3] = rng.uniform(0.03, 0.10, (n, n_rep))
        d = rng.normal(size=(n, 3))                  # the first obstacle drifts to 15 cm from the tool: it matters
        r4[:, 0, 0:3] = tool_pos[first:first + n] + 0.15 * d / np.linalg.norm(d, axis=1, keepdims=True)
        r4[:, 0, 3] = 0.1
        r4 = _rnd(r4, dt)
        r4[rng.uniform(size=(n, n_rep)) < nan_frac, 0] = np.nan
    for j in range(n):
        b = first + j
        if active is not None and not active[j]:
            continue
        gi, ri = _layout(w, b)
        if goal and gi is not None and not np.isnan(g16[j, 0]):
            F2["p"][b, gi, :12] = g16[j, :12]
        for k, i in enumerate(ri[:n_rep] if reps else ()):
            if not np.isnan(r4[j, k, 0]):
                F2["p"][b, i, :4] = r4[j, k]
    w2 = dict(w)
    w2["fields"] = F2
    return w2, g16, r4


def _engine(env, chain, w, dt, max_slots, params, tool=None):
    eng = env.engine.Engine(chain, w["q"].shape[0], io_dtype=dt, max_slots=max_slots, device=0, params=params)
    eng.set_small_batch_kernel(0)
    eng.set_fields(w["fields"], w["nfields"])
    if tool is not None:
        eng.set_tool(tool, per_arm=True)
    return eng


def _dev(env, a, dt):
    return None if a is None else env.torch.from_numpy(np.ascontiguousarray(a.astype(dt))).cuda()


def _structure(eng):
    return (eng.field_path, eng.uniform_repellers, eng.mixed_orders, eng.slots_in_use, eng.launch_epoch)


def _steps(eng, w, wants, **kw):
    out = []
    for want in wants:
        eng.reset_state()                            # (the nullspace sign memory starts over, as the oracle's does)
        eng.launched_kernels()
        got = eng.step_host(w["q"], want=want, **kw)
        out.append((got, eng.launched_kernels()))
    return out


def _same_bits(a, b, what):
    for k in a:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), (what, k, np.abs(a[k].astype(np.float64) - b[k]).max())


def _vs_oracle(env, chain, params, w2, got, want, dt, tool=None):
    keys = tuple(k for k in want if k != "goal_dist")
    ref = env.oc.cycle_batch(chain, params, w2["q"], w2["fields"], w2["nfields"], tool=tool, want=keys)
    tol = 1e-9 if dt == np.float64 else 1e-6
    for k in keys:
        if k == "status":
            assert np.array_equal(got[k], ref[k])
        else:
            err = np.abs(got[k].astype(np.float64) - ref[k]).max()
            print("%-10s max|hip - oracle| = %.3e (bar %.0e)" % (k, err, tol))
            assert err < tol, (k, err)
    return ref


CASES = {
    # name: (robot, dtype, scene, obstacles, flags, per-arm tool, options of the move)
    "uniform_f32_lean": ("lwr", np.float32, "plain", 8, 0, False, {}),
    "uniform_f64": ("lwr", np.float64, "plain", 8, 0, False, {"nan_frac": 0.15}),
    "uniform_f32_nullspace": ("lwr", np.float32, "plain", 5, 3, False, {}),
    "compact_f32": ("lwr", np.float32, "pairs", 7, 0, False, {}),
    "compact_f64": ("lwr", np.float64, "pairs", 8, 7, False, {"nan_frac": 0.15}),
    "mixed_orders_f32": ("lwr", np.float32, "mixed", 8, 0, False, {}),
    "mixed_orders_f64": ("lwr", np.float64, "mixed", 11, 3, False, {}),
    "path2_f32": ("lwr", np.float32, "path2", 5, 0, False, {}),
    "path2_f64": ("lwr", np.float64, "path2", 5, 3, False, {}),
    "path2_tool_f32": ("lwr", np.float32, "path2", 5, 0, True, {}),
    "path2_tool_f64": ("lwr", np.float64, "path2", 4, 0, True, {"nan_frac": 0.15}),
    "path0_fractional_f64": ("lwr", np.float64, "fractional", 6, 0, False, {}),
    "path0_fractional_f32": ("lwr", np.float32, "fractional", 6, 3, False, {}),
    "path0_second_attractor_f32": ("lwr", np.float32, "attractor2", 5, 0, False, {}),
    "path0_second_attractor_f64": ("lwr", np.float64, "attractor2", 5, 0, False, {}),
    "dual14_f32": ("lwr_dual14", np.float32, "plain", 16, 7, False, {}),
    "dual14_f64": ("lwr_dual14", np.float64, "path2", 6, 0, False, {}),
    "powercube6_f32": ("powercube6", np.float32, "pairs", 3, 0, False, {}),
    "powercube6_f64": ("powercube6", np.float64, "plain", 4, 0, False, {}),
    "ragged_f32": ("lwr", np.float32, "ragged", 8, 0, False, {}),                 # n_rep = 8 > many arms' count
    "ragged_f64": ("lwr", np.float64, "ragged", 6, 3, False, {"n_rep": 6}),
    "partial_range_f32": ("lwr", np.float32, "plain", 8, 0, False, {"first": 37, "n": 64 * 4 + 11}),
    "partial_range_f64": ("lwr_dual14", np.float64, "pairs", 5, 0, False, {"first": 129, "n": 70}),
    "active_mask_f32": ("lwr", np.float32, "plain", 8, 0, False, {"active": 0.6}),
    "active_mask_f64": ("powercube6", np.float64, "path2", 4, 0, False, {"active": 0.6, "first": 5, "n": 300}),
    "nan_rows_f32": ("lwr", np.float32, "pairs", 8, 0, False, {"nan_frac": 0.5}),
    "goal_only_f32": ("lwr", np.float32, "plain", 8, 0, False, {"reps": False}),
    "goal_only_f64": ("lwr", np.float64, "path2", 5, 0, False, {"reps": False}),
    "repellers_only_f32": ("lwr", np.float32, "plain", 8, 0, False, {"goal": False}),
    "repellers_only_f64": ("lwr", np.float64, "attractor2", 5, 3, False, {"goal": False}),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_same_bytes_same_answer(env, name):
    """A: set_fields(w), move_fields, step.  B: set_fields(w'), step.  Bit-identical outputs, the same kernel, both within the oracle's
    bars (1e-9 float64, 1e-6 float32: tests/test_gpu_mixed_orders.py) -- and the move mattered."""
    robot, dt, kind, nobs, flags, per_arm_tool, opt = CASES[name]
    opt = dict(opt)
    chain = env.robots.by_name(robot)
    B = 64 * 6 + 23                                   # B % 64 != 0
    w, max_slots, path, uni, mixed = _scene(env, chain, kind, B, nobs, dt, seed=sum(map(ord, name)))
    params = env.abi.default_params(flags=flags)
    rng = np.random.default_rng(11)
    n = opt.get("n", B - opt.get("first", 0))
    if "active" in opt:
        opt["active"] = (rng.uniform(size=n) < opt["active"]).astype(np.int32)
    tool = None
    if per_arm_tool:
        tool = np.tile(np.eye(4).reshape(16), (B, 1))
        tool[:, [3, 7, 11]] = _rnd(rng.uniform(-0.05, 0.05, (B, 3)) + [0.0, 0.0, 0.15], dt)
    w2, g16, r4 = _make_move(env, chain, w, dt, seed=3, **opt)
    A = _engine(env, chain, w, dt, max_slots, params, tool)
    Bm = _engine(env, chain, w2, dt, max_slots, params, tool)
    assert A.field_path == path and A.uniform_repellers == uni and A.mixed_orders == mixed
    wants = (LEAN, FULL)
    before = _steps(A, w, wants)                      # the scene as it stood (and the images have been read once)
    s0 = _structure(A)
    gd, rd, ad = _dev(env, g16, dt), _dev(env, r4, dt), _dev(env, opt.get("active"), np.int32)
    env.torch.cuda.synchronize()
    A.move_fields(goal=gd, repellers=rd, active=ad, first_arm=opt.get("first", 0))
    assert _structure(A) == s0 and s0[:4] == _structure(Bm)[:4]      # nothing a launch decides has moved, the epoch included
    after = _steps(A, w, wants)
    there = _steps(Bm, w, wants)
    for want, (g0, _), (ga, ka), (gb, kb) in zip(wants, before, after, there):
        assert ka == kb and len(ka) == 1, (ka, kb)
        _same_bits(ga, gb, (name, want))
        for got in (ga, gb):
            _vs_oracle(env, chain, params, w2, got, want, dt, tool=tool)
        moved = np.abs(ga["qdot_out"].astype(np.float64) - g0["qdot_out"]).max()
        print("%s: max|qdot_out(w') - qdot_out(w)| = %.3f" % (name, moved))
        assert moved > 0.01
    A.close()
    Bm.close()


@pytest.mark.parametrize("dt,kind", [(np.float32, "plain"), (np.float64, "path2"), (np.float64, "attractor2")])
def test_nothing_structural_moved_probe_and_rollout_see_the_move(env, dt, kind):
    chain = env.robots.lwr()
    B = 64 * 4 + 7
    w, max_slots, path, uni, mixed = _scene(env, chain, kind, B, 5, dt, seed=5)
    params = env.abi.default_params(flags=0)
    w2, g16, r4 = _make_move(env, chain, w, dt, seed=7, nan_frac=0.1)
    A, Bm = _engine(env, chain, w, dt, max_slots, params), _engine(env, chain, w2, dt, max_slots, params)
    s0 = _structure(A)
    gd, rd = _dev(env, g16, dt), _dev(env, r4, dt)
    pose = _dev(env, chain.fk(w["q"]).reshape(B, 16), dt)
    tdt = env.torch.float32 if dt == np.float32 else env.torch.float64
    v6 = [env.torch.zeros(B, 6, dtype=tdt, device="cuda") for _ in range(2)]
    env.torch.cuda.synchronize()
    A.move_fields(goal=gd, repellers=rd)
    assert _structure(A) == s0 and s0[:4] == _structure(Bm)[:4]
    for eng, out in zip((A, Bm), v6):
        eng.probe_field(pose, out)
        eng.sync()
    assert np.array_equal(v6[0].cpu().numpy(), v6[1].cpu().numpy()) and np.abs(v6[0].cpu().numpy()).max() > 0
    ref = env.oc.probe_field(params, w2["fields"], w2["nfields"], chain.fk(w["q"]).reshape(B, 16).astype(dt).astype(np.float64))
    assert np.abs(v6[0].cpu().numpy() - ref).max() < (1e-9 if dt == np.float64 else 1e-6)
    ra = A.rollout_host(w["q"], 12, 0.01, want=("qdot_out", "status"))
    rb = Bm.rollout_host(w["q"], 12, 0.01, want=("qdot_out", "status"))
    _same_bits(ra, rb, "rollout")
    assert _structure(A) == s0
    A.close()
    Bm.close()


def test_closed_loop_on_the_device(env):
    """Every arm's goal translates by a fixed step per cycle and obstacle 0 drifts; torch tensors on the engine's stream integrate q and
    update the goal / repeller tensors, move_fields, step -- one synchronisation, at the end.  Against the oracle stepped on the host
    with the fields rewritten each cycle, at the bars of tests/test_gpu_rollout.py for 40 cycles: 1e-8 on q, 1e-7 on qdot_out."""
    torch = env.torch
    chain = env.robots.lwr()
    B, K, dt, nobs = 1024, 40, 0.01, 8
    w = env.synth.make_workload(chain, B, nobs, seed=31, io_dtype=np.float64)
    params = env.abi.default_params(flags=0)
    rng = np.random.default_rng(9)
    gstep = rng.uniform(-0.002, 0.002, (B, 3))
    drift = rng.uniform(-0.004, 0.004, (B, 3))
    eng = env.engine.Engine(chain, B, io_dtype=np.float64, max_slots=nobs, params=params)
    eng.set_fields(w["fields"], w["nfields"])
    s0 = _structure(eng)
    eng.use_stream(torch.cuda.current_stream().cuda_stream)
    epoch = eng.launch_epoch
    q = torch.from_numpy(w["q"]).cuda()
    qd = torch.zeros(B, 7, dtype=torch.float64, device="cuda")
    goal = torch.from_numpy(np.ascontiguousarray(w["fields"]["p"][:, 0, :16])).cuda()
    rep = torch.from_numpy(np.ascontiguousarray(w["fields"]["p"][:, 1:1 + nobs, :4])).cuda()
    gs, dr = torch.from_numpy(gstep).cuda(), torch.from_numpy(drift).cuda()
    io = eng.make_io(q, qdot_out=qd)
    for c in range(K):
        if c:
            q.add_(qd, alpha=dt)
            goal[:, 3] += gs[:, 0]
            goal[:, 7] += gs[:, 1]
            goal[:, 11] += gs[:, 2]
            rep[:, 0, :3] += dr
            eng.move_fields(goal=goal, repellers=rep)
        eng.step(io)
    q.add_(qd, alpha=dt)
    torch.cuda.synchronize()                          # the one synchronisation
    assert eng.launch_epoch == epoch and _structure(eng)[:4] == s0[:4]
    # the oracle, stepped on the host
    F = w["fields"].copy()
    qh = w["q"].copy()
    for c in range(K):
        if c:
            F["p"][:, 0, [3, 7, 11]] += gstep
            F["p"][:, 1, 0:3] += drift
        ref = env.oc.cycle_batch(chain, params, qh, F, w["nfields"], want=("qdot_out",))
        qh = qh + dt * ref["qdot_out"]
    eq = np.abs(q.cpu().numpy() - qh).max()
    ev = np.abs(qd.cpu().numpy() - ref["qdot_out"]).max()
    print("closed loop, 40 cycles: max|q - oracle| = %.3e (bar 1e-8), max|qdot_out - oracle| = %.3e (bar 1e-7)" % (eq, ev))
    assert eq < 1e-8 and ev < 1e-7
    # the scene did move: the same loop over the standing scene ends elsewhere
    still = env.oc.cycle_batch(chain, params, qh, w["fields"], w["nfields"], want=("qdot_out",))
    assert np.abs(still["qdot_out"] - ref["qdot_out"]).max() > 0.01
    eng.close()


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_leader_and_follower(env, dt):
    """Engine L's pose output tensor, unchanged, is engine F's goal16: F follows L's tool.  Equal, bit for bit, to F after set_fields
    with those poses as goals."""
    torch = env.torch
    chain = env.robots.lwr()
    B = 64 * 3 + 5
    wl = _round(env.synth.make_workload(chain, B, 3, seed=61, io_dtype=dt), dt)
    wf = _round(env.synth.make_workload(chain, B, 6, seed=62, io_dtype=dt), dt)
    params = env.abi.default_params(flags=0)
    L, Fa = _engine(env, chain, wl, dt, 3, params), _engine(env, chain, wf, dt, 6, params)
    tdt = torch.float32 if dt == np.float32 else torch.float64
    pose = torch.zeros(B, 16, dtype=tdt, device="cuda")
    ql = _dev(env, wl["q"], dt)
    torch.cuda.synchronize()
    qdl = torch.zeros(B, 7, dtype=tdt, device="cuda")
    L.step(L.make_io(ql, qdot_out=qdl, pose=pose))
    L.sync()
    Fa.move_fields(goal=pose)
    ga = Fa.step_host(wf["q"], want=FULL)
    w2 = dict(wf)
    w2["fields"] = wf["fields"].copy()
    ph = pose.cpu().numpy().astype(np.float64)
    assert np.abs(ph[:, :12]).max() > 0
    w2["fields"]["p"][:, 0, :12] = ph[:, :12]
    Fb = _engine(env, chain, w2, dt, 6, params)
    gb = Fb.step_host(wf["q"], want=FULL)
    _same_bits(ga, gb, "follower")
    _vs_oracle(env, chain, params, w2, ga, FULL, dt)
    for e in (L, Fa, Fb):
        e.close()


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_host_form_rounds_like_set_fields(env, dt):
    """move_fields_host with doubles == the device form with the same values rounded == set_fields with the doubles in p[]."""
    chain = env.robots.lwr()
    B = 64 * 2 + 9
    w, max_slots, *_ = _scene(env, chain, "path2", B, 4, dt, seed=71)
    params = env.abi.default_params(flags=0)
    w2r, g16, r4 = _make_move(env, chain, w, np.float64, seed=13, nan_frac=0.1, first=3, n=B - 10)   # doubles, NOT rounded to float32
    w2 = dict(w2r)
    w2["fields"] = w2r["fields"].copy()
    H, D, S = (_engine(env, chain, w, dt, max_slots, params) for _ in range(3))
    s0 = _structure(H)
    H.move_fields_host(goal=g16, repellers=r4, first_arm=3)
    assert _structure(H) == s0
    gd, rd = _dev(env, g16, dt), _dev(env, r4, dt)
    env.torch.cuda.synchronize()
    D.move_fields(goal=gd, repellers=rd, first_arm=3)
    S.set_fields(w2["fields"], w2["nfields"])         # the library rounds p[] itself
    outs = [e.step_host(w["q"], want=FULL) for e in (H, D, S)]
    _same_bits(outs[0], outs[1], "host vs device form")
    _same_bits(outs[0], outs[2], "host form vs set_fields")
    for e in (H, D, S):
        e.close()


def test_sharded_engine_moves_global_rows(env):
    """ShardedEngine.move_fields_host over two handles on one device splits global rows as set_fields does."""
    chain = env.robots.lwr()
    B, dt = 64 * 3 + 11, np.float64
    w, max_slots, *_ = _scene(env, chain, "pairs", B, 5, dt, seed=81)
    w2, g16, r4 = _make_move(env, chain, w, dt, seed=15)
    kw = dict(rank=0, world=1, devices=[0, 0], io_dtype=dt, max_slots=max_slots, params=env.abi.default_params(flags=0))
    a, b = env.sharding.ShardedEngine(chain, B, **kw), env.sharding.ShardedEngine(chain, B, **kw)
    assert len(a.engines) == 2
    a.set_fields(w["fields"], w["nfields"])
    a.move_fields_host(goal=g16, repellers=r4)
    b.set_fields(w2["fields"], w2["nfields"])
    ga, gb = a.step_host(w["q"], want=("qdot_out", "status")), b.step_host(w["q"], want=("qdot_out", "status"))
    _same_bits(ga, gb, "sharded")
    ref = env.oc.cycle_batch(chain, kw["params"], w2["q"], w2["fields"], w2["nfields"], want=("qdot_out",))
    assert np.abs(ga["qdot_out"] - ref["qdot_out"]).max() < 1e-9
    a.close()
    b.close()


def test_argument_and_state_errors(env):
    chain = env.robots.lwr()
    B = 100
    w = env.synth.make_workload(chain, B, 4, seed=91, io_dtype=np.float32)
    eng = env.engine.Engine(chain, B, io_dtype=np.float32, max_slots=4)
    g = env.torch.zeros(B, 16, dtype=env.torch.float32, device="cuda")
    r = env.torch.zeros(B, 5, 4, dtype=env.torch.float32, device="cuda")
    env.torch.cuda.synchronize()
    mv = eng.lib.vfik_move_fields
    p = lambda t: C.c_void_p(t.data_ptr())
    assert mv(eng.h, 0, B, p(g), None, 0, None) == -4                     # VFIK_E_STATE: no field sets yet
    assert eng.lib.vfik_move_fields_host(eng.h, 0, 1, np.zeros(16).ctypes.data, None, 0) == -4
    eng.set_fields(w["fields"], w["nfields"])
    epoch = eng.launch_epoch
    assert mv(eng.h, 0, B, None, None, 0, None) == -1                     # both NULL
    assert mv(eng.h, -1, B, p(g), None, 0, None) == -1                    # bad ranges
    assert mv(eng.h, 1, B, p(g), None, 0, None) == -1
    assert mv(eng.h, 0, 0, p(g), None, 0, None) == -1
    assert mv(eng.h, 0, B, p(g), p(r), -1, None) == -1                    # n_rep < 0
    assert mv(eng.h, 0, B, p(g), p(r), 5, None) == -1                     # n_rep > max_slots
    assert b"n_rep" in eng.lib.vfik_last_error()
    assert eng.launch_epoch == epoch
    with pytest.raises(ValueError):
        eng.move_fields(goal=g[:, :12])
    with pytest.raises(ValueError):
        eng.move_fields(goal=g.double())
    with pytest.raises(ValueError):
        eng.move_fields_host(goal=np.zeros((B, 12)))
    with pytest.raises(ValueError):
        eng.move_fields_host(goal=np.zeros((B, 16)), repellers=np.zeros((B - 1, 2, 4)))
    eng.close()
