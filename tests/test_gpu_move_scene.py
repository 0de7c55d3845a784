"""Funnels, hemispheres and further attractors that move on the device (vfik_move_scene).  `set goalAndNormal` re-sends the goal, the
approach funnel and the near-goal repeller when the target's pose changes (object_feeder:248-303), `set ObstacleH` a surface with its
normal (object_feeder:335-354); vfik_move_scene writes those coordinates into the images vfik_set_fields packed.  The yardstick is the
one of tests/test_gpu_move_fields.py: an engine that got the moved scene through set_fields holds the same BYTES, runs the same kernel and
returns the same bits; both are held to the oracle (1e-9 float64, 1e-6 float32).  Before any engine exists each case shows with the oracle
that every class it moves matters when moved ALONE: max |qdot_out(w') - qdot_out(w)| > 0.01 rad/s."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_move_fields as mf  # noqa: E402  (its helpers: the same engines, steps, bit comparison and oracle bars)

pytestmark = pytest.mark.gpu

LEAN, FULL = mf.LEAN, mf.FULL
CLASSES = ("goal", "rep", "fun", "hem", "att")
TYPE_OF = {"rep": 2, "fun": 5, "hem": 4, "att": 1}
HEAD = {"goal": 12, "rep": 4, "fun": 6, "hem": 6, "att": 12}     # how many of p[] a row replaces
N_RICH = 70                                                      # path-0 scene: the arms that make the batch general


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


_rnd = mf._rnd


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _tool_pos(chain, q, tool=None):
    T = chain.fk(q).reshape(-1, 4, 4)
    if tool is not None:
        T = T @ tool.reshape(-1, 4, 4)
    return T[:, :3, 3]


# ---- scenes -------------------------------------------------------------------------------------------------------------------
def _simple_arm(goal, obst, b, first_obstacle_id, ragged):
    """goalAndNormal + obstacles (+ a table for every third arm): goal 1, funnel 2, near-goal repeller 3, obstacles, hemisphere 40.
    ragged: some arms have no funnel and no near-goal repeller."""
    pos, axis = goal[[3, 7, 11]], goal[[2, 6, 10]]
    prims = [(1, 1, 1.0, list(goal) + [0.05])]
    if not (ragged and b % 7 == 5):
        prims.append((2, 5, 30.0, list(pos) + list(axis) + [0.15, 10.0, 0.15, 2.0]))
        prims.append((3, 2, -10.0, list(pos - 0.05 * axis) + [0.2, 0.001, 5.0]))
    prims += [(first_obstacle_id + k, 2, -10.0, list(o)) for k, o in enumerate(obst)]
    if b % 3 == 0:
        prims.append((40, 4, -50.0, [0.0, 0.0, -0.3, 0.02, -0.01, 1.0, 0.05, 5.0]))
    return prims


def _scene(env, chain, kind, B, nobs, dt, seed):
    """-> (workload, max_slots, expected field path).
    path2: every arm is a goalAndNormal arm (straight-line field path 2: the aux block is read).
    ragged: the same, some arms without a funnel.
    path0: arms [0, N_RICH) carry two funnels whose ids straddle the repellers (ids 2 and 30: general slots 0 and 10 + nobs), a second and a
    third attractor (ids 3, 4: general slots 2 and 5, BEFORE the obstacles), two hemispheres (ids 5, 31); the other arms are path2 arms."""
    rng = np.random.default_rng(seed + 1000)
    w0 = env.synth.make_workload(chain, B, nobs, seed=seed, io_dtype=dt)
    F0 = w0["fields"]
    arms = []
    for b in range(B):
        goal, obst = F0["p"][b, 0, :16], F0["p"][b, 1:1 + nobs, :6]
        if kind == "path0" and b < N_RICH:
            pos, axis = goal[[3, 7, 11]], goal[[2, 6, 10]]
            a2, a3 = (chain.fk(rng.uniform(0.5 * chain.q_lo, 0.5 * chain.q_hi, (1, chain.n))).reshape(16) for _ in range(2))
            prims = [(1, 1, 1.0, list(goal) + [0.05]),
                     (2, 5, 30.0, list(pos) + list(axis) + [0.15, 10.0, 0.15, 2.0]),
                     (3, 1, 0.8, list(a2) + [0.05]),
                     (4, 1, 0.6, list(a3) + [0.05]),
                     (5, 4, -50.0, [0.0, 0.0, -0.3, 0.02, -0.01, 1.0, 0.05, 5.0])]
            prims += [(6 + k, 2, -10.0, list(o)) for k, o in enumerate(obst)]
            prims.append((30, 5, 20.0, list(rng.uniform(-0.5, 0.5, 3) + [0.0, 0.0, 0.6]) + list(_unit(rng.normal(size=3))) + [0.2, 8.0, 0.1, 2.0]))
            prims.append((31, 4, -50.0, [1.5, 0.0, 0.0, -1.0, 0.0, 0.05, 0.05, 5.0]))
        else:
            prims = _simple_arm(goal, obst, b, 6 if kind == "path0" else 4, kind == "ragged")
        arms.append(prims)
    M = max(len(p) for p in arms)
    F = np.zeros((B, M), dtype=env.abi.FIELD_DTYPE)
    nf = np.zeros(B, dtype=np.int32)
    for b, prims in enumerate(arms):
        nf[b] = len(prims)
        for k, (vf_id, vf_type, force, p) in enumerate(prims):
            F["id"][b, k], F["type"][b, k], F["force"][b, k] = vf_id, vf_type, force
            F["p"][b, k, :len(p)] = p
    w = dict(q=w0["q"], fields=F, nfields=nf)
    max_slots = (2 + 3 + 3 + 2 + nobs + 2 + 2) if kind == "path0" else (2 + 1 + nobs + 2)
    return mf._round(w, dt), max_slots, (0 if kind == "path0" else 2)


def _layout(w, b):
    """per class the indices of arm b's primitives in ascending-id order; "goal": the lowest-id attractor, "att": those behind it"""
    F = w["fields"]
    idx = [k for k in range(w["nfields"][b]) if F["type"][b, k] != 0]
    idx.sort(key=lambda k: F["id"][b, k])
    att = [k for k in idx if F["type"][b, k] == 1]
    lay = {c: [k for k in idx if F["type"][b, k] == t] for c, t in TYPE_OF.items()}
    lay["goal"], lay["att"] = att[:1], att[1:]
    return lay


def _make_move(env, chain, w, dt, seed, classes=CLASSES, counts=None, first=0, n=None, nan_frac=0.0, active=None, feeder=False, tool=None):
    """-> rows = {class: array (n, 16) / (n, rows, 4 | 6 | 16)} rounded to dt.  feeder: goal, funnel 0 and repeller 0 follow ONE new target
    pose, as the object feeder derives them (object_feeder:248-303); otherwise every class moves on its own."""
    rng = np.random.default_rng(seed + 2000)
    B = w["q"].shape[0]
    n = B - first if n is None else n
    lay = [_layout(w, b) for b in range(B)]
    counts = dict(counts or {})
    for c in ("rep", "fun", "hem", "att"):
        counts.setdefault(c, max(1, max(len(l[c]) for l in lay)))
    if feeder:
        counts["rep"] = 1
    tp = _tool_pos(chain, w["q"], tool)[first:first + n]

    def frames():
        return chain.fk(rng.uniform(0.8 * chain.q_lo, 0.8 * chain.q_hi, (B, chain.n))).reshape(B, 16)[first:first + n]

    rows = {}
    target = frames()
    if "goal" in classes:
        rows["goal"] = target.copy()
    if "rep" in classes:
        r = np.empty((n, counts["rep"], 4))
        r[:, :, 0:2] = rng.uniform(-0.8, 0.8, (n, counts["rep"], 2))
        r[:, :, 2] = rng.uniform(0.0, 1.2, (n, counts["rep"]))
        r[:, :, 3] = rng.uniform(0.03, 0.10, (n, counts["rep"]))
        if feeder:                                       # the near-goal repeller: 5 cm behind the target along its approach axis
            r[:, 0, 0:3] = target[:, [3, 7, 11]] - 0.05 * target[:, [2, 6, 10]]
            r[:, 0, 3] = 0.2
        else:                                            # the first obstacle drifts to 15 cm from the tool: it matters
            r[:, 0, 0:3] = tp + 0.15 * _unit(rng.normal(size=(n, 3)))
            r[:, 0, 3] = 0.1
        rows["rep"] = r
    if "fun" in classes:
        f = np.empty((n, counts["fun"], 6))
        f[:, :, 0:3] = rng.uniform(-0.5, 0.5, (n, counts["fun"], 3)) + [0.0, 0.0, 0.6]
        f[:, :, 3:6] = _unit(rng.normal(size=(n, counts["fun"], 3)))
        src = target if feeder else frames()            # the approach funnel: apex at a target, axis its z
        f[:, 0, 0:3], f[:, 0, 3:6] = src[:, [3, 7, 11]], src[:, [2, 6, 10]]
        rows["fun"] = f
    if "hem" in classes:                                 # a plane 5 to 7 cm under the tool along its normal (safe distance 0.05)
        nrm = _unit(rng.normal(size=(n, counts["hem"], 3)))
        d = rng.uniform(0.05, 0.07, (n, counts["hem"], 1))
        rows["hem"] = np.concatenate([tp[:, None, :] - nrm * d, nrm], axis=2)
    if "att" in classes:
        rows["att"] = np.stack([frames() for _ in range(counts["att"])], axis=1)
    for c in rows:
        rows[c] = _rnd(rows[c], dt)
        if nan_frac:
            rows[c][rng.uniform(size=rows[c].shape[:-1]) < nan_frac, 0] = np.nan
    return rows


def _apply(w, rows, first=0, active=None, only=None):
    """w with the rows written into p[] as the library is to write them (NaN rows, inactive arms and rows beyond an arm's count stay)"""
    F2 = w["fields"].copy()
    for c, arr in rows.items():
        if only is not None and c != only:
            continue
        for j in range(arr.shape[0]):
            if active is not None and not active[j]:
                continue
            idx = _layout(w, first + j)[c]
            per_arm = arr[j][None] if c == "goal" else arr[j]
            for k, i in enumerate(idx[:per_arm.shape[0]]):
                if not np.isnan(per_arm[k, 0]):
                    F2["p"][first + j, i, :HEAD[c]] = per_arm[k, :HEAD[c]]
    w2 = dict(w)
    w2["fields"] = F2
    return w2


def _each_class_matters(env, chain, params, w, rows, first, active, tool, name):
    ref = env.oc.cycle_batch(chain, params, w["q"], w["fields"], w["nfields"], tool=tool, want=("qdot_out",))["qdot_out"]
    for c in rows:
        wc = _apply(w, rows, first, active, only=c)
        if not any(_layout(w, first + j)[c] for j in range(rows[c].shape[0])):
            assert wc["fields"].tobytes() == w["fields"].tobytes()        # no arm of the range has such a primitive: nothing to move
            continue
        got = env.oc.cycle_batch(chain, params, wc["q"], wc["fields"], wc["nfields"], tool=tool, want=("qdot_out",))["qdot_out"]
        moved = np.abs(got - ref).max()
        print("%s: oracle, %s moved alone: max|qdot_out(w') - qdot_out(w)| = %.3f" % (name, c, moved))
        assert moved > 0.01, (name, c, moved)


def _move(env, eng, rows, dt, first=0, active=None):
    dev = {c: mf._dev(env, a, dt) for c, a in rows.items()}
    ad = mf._dev(env, active, np.int32)
    env.torch.cuda.synchronize()
    eng.move_scene(goal=dev.get("goal"), repellers=dev.get("rep"), funnels=dev.get("fun"), hemispheres=dev.get("hem"),
                   attractors=dev.get("att"), active=ad, first_arm=first)


CASES = {
    # name: (robot, dtype, scene, obstacles, flags, per-arm tool, options of the move)
    "path2_funnels_f32": ("lwr", np.float32, "path2", 5, 0, False, {"classes": ("fun",)}),
    "path2_funnels_f64": ("lwr", np.float64, "path2", 5, 3, False, {"classes": ("fun",)}),
    "path2_hemispheres_f32": ("lwr", np.float32, "path2", 5, 0, False, {"classes": ("hem",)}),
    "path2_hemispheres_f64": ("lwr", np.float64, "path2", 4, 0, False, {"classes": ("hem",)}),
    "path2_feeder_f32": ("lwr", np.float32, "path2", 8, 0, False, {"classes": ("goal", "rep", "fun"), "feeder": True}),
    "path2_feeder_f64": ("lwr", np.float64, "path2", 5, 0, False, {"classes": ("goal", "rep", "fun"), "feeder": True}),
    "path2_everything_f32": ("lwr", np.float32, "path2", 5, 3, False, {"classes": ("goal", "rep", "fun", "hem")}),
    "path2_everything_f64": ("lwr", np.float64, "path2", 5, 0, False, {"classes": ("goal", "rep", "fun", "hem")}),
    "path0_f32": ("lwr", np.float32, "path0", 3, 0, False, {"classes": ("fun", "hem", "att")}),
    "path0_f64": ("lwr", np.float64, "path0", 3, 0, False, {"classes": ("fun", "hem", "att")}),
    "path0_everything_f64": ("lwr", np.float64, "path0", 2, 3, False, {}),
    "partial_range_f32": ("lwr", np.float32, "path2", 5, 0, False, {"classes": ("goal", "rep", "fun", "hem"), "first": 37, "n": 64 * 4 + 11}),
    "partial_range_f64": ("lwr", np.float64, "path0", 3, 0, False, {"first": 37, "n": 64 * 4 + 11}),
    "active_mask_f32": ("lwr", np.float32, "path2", 5, 0, False, {"classes": ("goal", "rep", "fun", "hem"), "active": 0.6}),
    "active_mask_f64": ("lwr", np.float64, "path0", 3, 0, False, {"active": 0.6, "first": 5, "n": 300}),
    "nan_rows_f32": ("lwr", np.float32, "path0", 3, 0, False, {"nan_frac": 0.15}),
    "nan_rows_f64": ("lwr", np.float64, "path2", 5, 0, False, {"classes": ("goal", "rep", "fun", "hem"), "nan_frac": 0.15}),
    # more rows than most arms have primitives (some arms have no funnel at all, two thirds no hemisphere, none a further attractor)
    "ragged_f32": ("lwr", np.float32, "ragged", 5, 0, False, {"counts": {"fun": 3, "hem": 3, "att": 2, "rep": 8}}),
    "ragged_f64": ("lwr", np.float64, "path0", 3, 0, False, {"counts": {"fun": 4, "hem": 3, "att": 5}}),
    "dual14_f64": ("lwr_dual14", np.float64, "path2", 6, 0, False, {"classes": ("goal", "rep", "fun", "hem")}),
    "powercube6_f32": ("powercube6", np.float32, "path2", 4, 0, False, {"classes": ("goal", "rep", "fun", "hem")}),
    "per_arm_tool_f32": ("lwr", np.float32, "path2", 5, 0, True, {"classes": ("goal", "rep", "fun", "hem")}),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_same_bytes_same_answer(env, name):
    """A: set_fields(w), move_scene, step.  B: set_fields(w'), step.  Bit-identical outputs, the same single kernel, both within the
    oracle's bars, nothing a launch decides moved -- and each class, moved alone, matters.  The path-0 scenes then replace their general
    arms in BOTH engines with goalAndNormal arms: the batch drops to field path 2, whose launches read the aux block of every other arm --
    written by the move in A, by set_fields in B."""
    robot, dt, kind, nobs, flags, per_arm_tool, opt = CASES[name]
    opt = dict(opt)
    chain = env.robots.by_name(robot)
    B = 64 * 6 + 23                                   # B % 64 != 0
    w, max_slots, path = _scene(env, chain, kind, B, nobs, dt, seed=sum(map(ord, name)))
    params = env.abi.default_params(flags=flags)
    rng = np.random.default_rng(11)
    first = opt.pop("first", 0)
    n = opt.pop("n", B - first)
    active = opt.pop("active", None)
    if active is not None:
        active = (rng.uniform(size=n) < active).astype(np.int32)
    tool = None
    if per_arm_tool:
        tool = np.tile(np.eye(4).reshape(16), (B, 1))
        tool[:, [3, 7, 11]] = _rnd(rng.uniform(-0.05, 0.05, (B, 3)) + [0.0, 0.0, 0.15], dt)
    rows = _make_move(env, chain, w, dt, seed=3, first=first, n=n, tool=tool, **opt)
    _each_class_matters(env, chain, params, w, rows, first, active, tool, name)      # on the CPU, before any GPU work
    w2 = _apply(w, rows, first, active)
    A = mf._engine(env, chain, w, dt, max_slots, params, tool)
    Bm = mf._engine(env, chain, w2, dt, max_slots, params, tool)
    assert A.field_path == path
    wants = (LEAN, FULL)
    before = mf._steps(A, w, wants)                   # the scene as it stood (and the images have been read once)
    s0 = mf._structure(A)
    _move(env, A, rows, dt, first, active)
    assert mf._structure(A) == s0 and s0[:4] == mf._structure(Bm)[:4]      # nothing a launch decides has moved, the epoch included
    after = mf._steps(A, w, wants)
    there = mf._steps(Bm, w, wants)
    for want, (g0, _), (ga, ka), (gb, kb) in zip(wants, before, after, there):
        assert ka == kb and len(ka) == 1, (ka, kb)
        mf._same_bits(ga, gb, (name, want))
        for got in (ga, gb):
            mf._vs_oracle(env, chain, params, w2, got, want, dt, tool=tool)
        moved = np.abs(ga["qdot_out"].astype(np.float64) - g0["qdot_out"]).max()
        print("%s: max|qdot_out(w') - qdot_out(w)| = %.3f" % (name, moved))
        assert moved > 0.01
    if kind == "path0":
        w3 = dict(w2)
        w3["fields"] = w2["fields"].copy()
        w3["nfields"] = w2["nfields"].copy()
        ws, _, _ = _scene(env, chain, "path2", N_RICH, nobs, dt, seed=77)
        m = ws["fields"].shape[1]
        w3["fields"][:N_RICH] = 0
        w3["fields"][:N_RICH, :m] = ws["fields"]
        w3["nfields"][:N_RICH] = ws["nfields"]
        for eng in (A, Bm):
            eng.set_fields(w3["fields"][:N_RICH], w3["nfields"][:N_RICH], first_arm=0)
            assert eng.field_path == 2
        low, there = mf._steps(A, w, wants), mf._steps(Bm, w, wants)
        for want, (ga, ka), (gb, kb) in zip(wants, low, there):
            assert ka == kb and len(ka) == 1, (ka, kb)
            mf._same_bits(ga, gb, (name, "aux block", want))
            mf._vs_oracle(env, chain, params, w3, ga, want, dt, tool=tool)
    A.close()
    Bm.close()


@pytest.mark.parametrize("dt,kind", [(np.float32, "path0"), (np.float64, "path2")])
def test_probe_and_rollout_see_the_move(env, dt, kind):
    chain = env.robots.lwr()
    B = 64 * 4 + 7
    w, max_slots, _ = _scene(env, chain, kind, B, 4, dt, seed=5)
    params = env.abi.default_params(flags=0)
    rows = _make_move(env, chain, w, dt, seed=7, nan_frac=0.1, classes=CLASSES if kind == "path0" else ("goal", "rep", "fun", "hem"))
    w2 = _apply(w, rows)
    A, Bm = mf._engine(env, chain, w, dt, max_slots, params), mf._engine(env, chain, w2, dt, max_slots, params)
    s0 = mf._structure(A)
    pose = mf._dev(env, chain.fk(w["q"]).reshape(B, 16), dt)
    tdt = env.torch.float32 if dt == np.float32 else env.torch.float64
    v6 = [env.torch.zeros(B, 6, dtype=tdt, device="cuda") for _ in range(3)]
    A.probe_field(pose, v6[2])                        # the scene as it stood
    A.sync()
    _move(env, A, rows, dt)
    assert mf._structure(A) == s0 and s0[:4] == mf._structure(Bm)[:4]
    for eng, out in zip((A, Bm), v6):
        eng.probe_field(pose, out)
        eng.sync()
    va, vb, v0 = (t.cpu().numpy() for t in v6)
    assert np.array_equal(va, vb) and np.abs(va - v0).max() > 0.01
    ref = env.oc.probe_field(params, w2["fields"], w2["nfields"], chain.fk(w["q"]).reshape(B, 16).astype(dt).astype(np.float64))
    assert np.abs(va - ref).max() < (1e-9 if dt == np.float64 else 1e-6)
    ra = A.rollout_host(w["q"], 12, 0.01, want=("qdot_out", "status"))
    rb = Bm.rollout_host(w["q"], 12, 0.01, want=("qdot_out", "status"))
    mf._same_bits(ra, rb, "rollout")
    assert mf._structure(A) == s0
    A.close()
    Bm.close()


@pytest.mark.parametrize("kind", ["path2", "path0"])
def test_host_form_rounds_like_set_fields(env, kind):
    """move_scene_host with doubles that float32 cannot hold == the device form with the same values rounded == set_fields with the
    doubles in p[]."""
    dt = np.float32
    chain = env.robots.lwr()
    B = 64 * 2 + 9
    w, max_slots, _ = _scene(env, chain, kind, B, 4, dt, seed=71)
    params = env.abi.default_params(flags=0)
    first, n = 3, B - 10
    rows = _make_move(env, chain, w, np.float64, seed=13, nan_frac=0.1, first=first, n=n)       # doubles, NOT rounded to float32
    for c, a in rows.items():
        ok = ~np.isnan(a)
        assert (a[ok].astype(np.float32).astype(np.float64) != a[ok]).any(), c
    w2 = _apply(w, rows, first)
    H, D, S = (mf._engine(env, chain, w, dt, max_slots, params) for _ in range(3))
    s0 = mf._structure(H)
    H.move_scene_host(goal=rows["goal"], repellers=rows["rep"], funnels=rows["fun"], hemispheres=rows["hem"], attractors=rows["att"],
                      first_arm=first)
    assert mf._structure(H) == s0
    _move(env, D, rows, dt, first)
    S.set_fields(w2["fields"], w2["nfields"])         # the library rounds p[] itself
    outs = [e.step_host(w["q"], want=FULL) for e in (H, D, S)]
    mf._same_bits(outs[0], outs[1], "host vs device form")
    mf._same_bits(outs[0], outs[2], "host form vs set_fields")
    for e in (H, D, S):
        e.close()


def test_unaligned_rows_take_the_scalar_loads(env):
    """Callers' arrays that start 4 bytes off a pair / quad boundary (a view into a larger tensor): the same bits."""
    torch = env.torch
    dt = np.float32
    chain = env.robots.lwr()
    B = 64 * 2 + 9
    w, max_slots, _ = _scene(env, chain, "path0", B, 3, dt, seed=72)
    params = env.abi.default_params(flags=0)
    rows = _make_move(env, chain, w, dt, seed=14)
    w2 = _apply(w, rows)
    A, Bm = mf._engine(env, chain, w, dt, max_slots, params), mf._engine(env, chain, w2, dt, max_slots, params)
    kw, keep = {}, []
    for c, name in (("goal", "goal"), ("rep", "repellers"), ("fun", "funnels"), ("hem", "hemispheres"), ("att", "attractors")):
        flat = torch.zeros(rows[c].size + 1, dtype=torch.float32, device="cuda")
        flat[1:] = torch.from_numpy(rows[c].astype(np.float32).reshape(-1)).cuda()
        keep.append(flat)
        kw[name] = flat[1:].view(*rows[c].shape)
        assert kw[name].data_ptr() % 8 == 4 and kw[name].is_contiguous()
    torch.cuda.synchronize()
    A.move_scene(**kw)
    mf._same_bits(A.step_host(w["q"], want=FULL), Bm.step_host(w["q"], want=FULL), "unaligned")
    A.close()
    Bm.close()


def test_sharded_engine_moves_global_rows(env):
    chain = env.robots.lwr()
    B, dt = 64 * 3 + 11, np.float64
    w, max_slots, _ = _scene(env, chain, "path0", B, 3, dt, seed=81)
    rows = _make_move(env, chain, w, dt, seed=15)
    w2 = _apply(w, rows)
    kw = dict(rank=0, world=1, devices=[0, 0], io_dtype=dt, max_slots=max_slots, params=env.abi.default_params(flags=0))
    a, b = env.sharding.ShardedEngine(chain, B, **kw), env.sharding.ShardedEngine(chain, B, **kw)
    assert len(a.engines) == 2
    a.set_fields(w["fields"], w["nfields"])
    a.move_scene_host(goal=rows["goal"], repellers=rows["rep"], funnels=rows["fun"], hemispheres=rows["hem"], attractors=rows["att"])
    b.set_fields(w2["fields"], w2["nfields"])
    ga, gb = a.step_host(w["q"], want=("qdot_out", "status")), b.step_host(w["q"], want=("qdot_out", "status"))
    mf._same_bits(ga, gb, "sharded")
    ref = env.oc.cycle_batch(chain, kw["params"], w2["q"], w2["fields"], w2["nfields"], want=("qdot_out",))
    assert np.abs(ga["qdot_out"] - ref["qdot_out"]).max() < 1e-9
    a.close()
    b.close()


def test_field_sets_flush_moves_the_scene(env):
    """FieldSets -> Engine: a funnel, a hemisphere and the goal re-sent with new numbers reach the device through move_scene_host (the
    epoch stays), and the engine then answers like one that got the sets through set_fields."""
    from vfclik_amd.fields import FieldSets
    chain = env.robots.lwr()
    B, dt = 64 + 5, np.float64
    w, max_slots, _ = _scene(env, chain, "path2", B, 3, dt, seed=83)
    rows = _make_move(env, chain, w, dt, seed=16, classes=("goal", "fun", "hem"))
    w2 = _apply(w, rows)
    params = env.abi.default_params(flags=0)
    A = env.engine.Engine(chain, B, io_dtype=dt, max_slots=max_slots, params=params)
    A.set_small_batch_kernel(0)
    fs = FieldSets(B, max_fields=w["fields"].shape[1])

    def load(ww):
        for b in range(B):
            F = ww["fields"][b, :ww["nfields"][b]]
            fs.set_arm(b, {int(f["id"]): [float(f["force"]), int(f["type"]), list(f["p"][:env.abi.FIELD_NPARAMS[int(f["type"])]])] for f in F})

    load(w)
    fs.flush(A)
    epoch = A.launch_epoch
    load(w2)
    assert fs.flush(A) == B
    assert A.launch_epoch == epoch                   # no set_fields call
    Bm = mf._engine(env, chain, w2, dt, max_slots, params)
    mf._same_bits(A.step_host(w["q"], want=FULL), Bm.step_host(w["q"], want=FULL), "FieldSets.flush")
    A.close()
    Bm.close()


def test_closed_loop_on_the_device(env):
    """Every arm's target translates each cycle; goal, funnel apex and near-goal repeller follow, computed with torch on the engine's
    stream; move_scene, step -- one synchronisation, at the end.  Against the oracle stepped on the host with the scene rebuilt each
    cycle, 20 cycles, at the float64 bar (1e-9) on q and qdot_out."""
    torch = env.torch
    chain = env.robots.lwr()
    B, K, dt, nobs = 64 * 6 + 23, 20, 0.01, 5
    w, max_slots, _ = _scene(env, chain, "path2", B, nobs, np.float64, seed=31)
    params = env.abi.default_params(flags=0)
    rng = np.random.default_rng(9)
    gstep = rng.uniform(-0.004, 0.004, (B, 3))
    eng = env.engine.Engine(chain, B, io_dtype=np.float64, max_slots=max_slots, params=params)
    eng.set_small_batch_kernel(0)
    eng.set_fields(w["fields"], w["nfields"])
    assert eng.field_path == 2
    eng.use_stream(torch.cuda.current_stream().cuda_stream)
    s0 = mf._structure(eng)
    F = w["fields"]                                   # array order = ascending id: goal 1, funnel 2, near-goal repeller 3, ...
    assert list(F["id"][0, :3]) == [1, 2, 3] and list(F["type"][0, :3]) == [1, 5, 2]
    q = torch.from_numpy(w["q"]).cuda()
    qd = torch.zeros(B, 7, dtype=torch.float64, device="cuda")
    goal = torch.from_numpy(np.ascontiguousarray(F["p"][:, 0, :16])).cuda()
    fun = torch.from_numpy(np.ascontiguousarray(F["p"][:, 1:2, :6])).cuda()
    rep = torch.from_numpy(np.ascontiguousarray(F["p"][:, 2:3, :4])).cuda()
    gs = torch.from_numpy(gstep).cuda()
    io = eng.make_io(q, qdot_out=qd)
    for c in range(K):
        if c:
            q.add_(qd, alpha=dt)
            goal[:, 3] += gs[:, 0]
            goal[:, 7] += gs[:, 1]
            goal[:, 11] += gs[:, 2]
            fun[:, 0, :3] += gs
            rep[:, 0, :3] += gs
            eng.move_scene(goal=goal, repellers=rep, funnels=fun)
        eng.step(io)
    q.add_(qd, alpha=dt)
    torch.cuda.synchronize()                          # the one synchronisation
    assert mf._structure(eng) == s0
    Fh = F.copy()
    qh = w["q"].copy()
    for c in range(K):
        if c:
            Fh["p"][:, 0, [3, 7, 11]] += gstep
            Fh["p"][:, 1, 0:3] += gstep
            Fh["p"][:, 2, 0:3] += gstep
        ref = env.oc.cycle_batch(chain, params, qh, Fh, w["nfields"], want=("qdot_out",))
        qh = qh + dt * ref["qdot_out"]
    eq = np.abs(q.cpu().numpy() - qh).max()
    ev = np.abs(qd.cpu().numpy() - ref["qdot_out"]).max()
    print("closed loop, 20 cycles: max|q - oracle| = %.3e, max|qdot_out - oracle| = %.3e (bar 1e-9)" % (eq, ev))
    assert eq < 1e-9 and ev < 1e-9
    # the scene did move: the same pose over the standing scene gives another command
    still = env.oc.cycle_batch(chain, params, qh - dt * ref["qdot_out"], w["fields"], w["nfields"], want=("qdot_out",))
    assert np.abs(still["qdot_out"] - ref["qdot_out"]).max() > 0.01
    eng.close()


def test_argument_and_state_errors(env):
    chain = env.robots.lwr()
    B = 100
    w, max_slots, _ = _scene(env, chain, "path2", B, 2, np.float32, seed=91)
    eng = env.engine.Engine(chain, B, io_dtype=np.float32, max_slots=max_slots)
    torch = env.torch
    g = torch.zeros(B, 16, dtype=torch.float32, device="cuda")
    f = torch.zeros(B, max_slots + 1, 6, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    lib = eng.lib

    def call(first=0, n=B, host=False, **kw):
        mv = env.abi.SceneMove()
        for k, v in kw.items():
            setattr(mv, k, v.data_ptr() if hasattr(v, "data_ptr") else v)
        return (lib.vfik_move_scene_host if host else lib.vfik_move_scene)(eng.h, first, n, C.byref(mv))

    assert call(goal16=g) == -4                                              # VFIK_E_STATE: no field sets yet
    hg = np.zeros((B, 16))
    assert call(host=True, goal16=hg.ctypes.data) == -4
    eng.set_fields(w["fields"], w["nfields"])
    epoch = eng.launch_epoch
    assert call() == -1                                                      # all five NULL
    assert lib.vfik_move_scene(eng.h, 0, B, None) == -1                      # no struct at all
    assert call(first=-1, goal16=g) == -1                                    # bad ranges
    assert call(first=1, goal16=g) == -1
    assert call(n=0, goal16=g) == -1
    for cnt in ("n_rep", "n_fun", "n_hem", "n_att"):
        assert call(fun6=f, **{cnt: -1}) == -1                               # a count < 0
        assert call(fun6=f, **{cnt: max_slots + 1}) == -1                    # a count > max_slots
        assert cnt.encode() in lib.vfik_last_error()
    act = np.ones(B, dtype=np.int32)
    assert call(host=True, goal16=hg.ctypes.data, active=act.ctypes.data) == -1      # the host form takes no mask
    assert call(fun6=f, n_fun=1) == 0 and call(host=True, goal16=hg.ctypes.data) == 0
    assert eng.launch_epoch == epoch
    with pytest.raises(ValueError):
        eng.move_scene(funnels=f[:, :2, :5])                                 # not contiguous
    with pytest.raises(ValueError):
        eng.move_scene(funnels=torch.zeros(B, 2, 5, dtype=torch.float32, device="cuda"))
    with pytest.raises(ValueError):
        eng.move_scene(hemispheres=f[:, :1].contiguous().double())
    with pytest.raises(ValueError):
        eng.move_scene(goal=g, funnels=f[:B - 1, :1].contiguous())
    with pytest.raises(ValueError):
        eng.move_scene(funnels=f.data_ptr(), n_arms=B)                       # a raw address needs its count
    with pytest.raises(ValueError):
        eng.move_scene_host(funnels=np.zeros((B, 2, 5)))
    with pytest.raises(ValueError):
        eng.move_scene_host(goal=np.zeros((B, 16)), hemispheres=np.zeros((B - 1, 2, 6)))
    with pytest.raises(ValueError):
        eng.move_scene_host()
    eng.close()
