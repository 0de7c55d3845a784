"""monitor_kernel held to the 50-digit reference of tests/hp_observers.py at its edges -- identical frames, angles from 1e-13 to a half turn,
distances from 0 to 1 km, frames that are no rotations to the last bit -- by the units derived there; and the fused observers of a cycle call
held, bit for bit, to the stand-alone kernels fed the published pose / twist.  tests/test_oracle_observers.py asserts the scenes' conditions
and the caps on the CPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hp_observers as ho  # noqa: E402

pytestmark = pytest.mark.gpu
DTYPES = [np.float32, np.float64]
IDS = ["f32", "f64"]


@pytest.fixture(scope="module")
def env():
    import __graft_entry__ as g
    g.build()
    from vfclik_amd import _abi, engine, robots, synth

    class E:
        pass

    e = E()
    e.abi, e.engine, e.robots, e.synth = _abi, engine, robots, synth
    yield e
    path = os.environ.get("VFIK_BACKEND_TABLE")
    if path:
        ho.write_table(path)
        ho.write_track_table(path)


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_monitor_kernel_at_its_edges(env, dt):
    pose, frames, kk = ho.monitor_scene(dt)
    ref = ho.reference(("monitor", dt), pose, frames)
    assert not ho.caps(kk, ref)
    B, O = frames.shape[:2]
    eng = env.engine.Engine(env.robots.lwr(), B, io_dtype=dt, max_slots=2)
    esz = np.dtype(dt).itemsize
    d_pose, d_fr, d_out = eng.dev_alloc(B * 16 * esz), eng.dev_alloc(B * O * 16 * esz), eng.dev_alloc(B * O * 2 * esz)
    try:
        eng.h2d(d_pose, pose.astype(dt))
        eng.h2d(d_fr, frames.astype(dt))
        eng.object_distances(d_pose, d_fr, O, d_out)
        got = np.zeros((B, O, 2), dtype=dt)
        eng.d2h(got, d_out)
    finally:
        for p in (d_pose, d_fr, d_out):
            eng.dev_free(p)
        eng.close()
    rD, rA = ho.ratios(got, ref, dt)
    print("monitor_kernel f%d: worst error / bar  D %.3f  angle %.3f" % (32 if dt == np.float32 else 64, rD.max(), rA.max()))
    ho.note("gpu", "monitor f%d" % (32 if dt == np.float32 else 64), "monitor_kernel", rD, rA, ref)
    worst = np.argwhere((rD >= 1.0) | (rA >= 1.0))[:6]
    assert rD.max() < 1.0 and rA.max() < 1.0, [(int(b), int(k), kk[b], float(rD[b, k]), float(rA[b, k])) for b, k in worst]
    same = [b for b, k in enumerate(kk) if k == "same"]
    assert np.all(got[same, :, 1] == 0.0) and np.all(got[same][:, [0, 6], 0] == 0.0)   # an identical frame: 0 and 0, exactly


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_track_kernel_at_its_edges(env, dt):
    """track_kernel fed the scene's frames and commands call by call -- perfectly tracking and antiparallel arms, frozen arms and zero commands
    (the (1, 0, 0) defaults), frame-to-frame rotations either side of has_axis, half turns, ext_int_diff next to 0.10, arms silent for some calls
    -- against the 50-digit reference over each arm's whole history; then track_reset, after which the same calls give the same rows."""
    poses, v6, active, kk = ho.track_scene(dt)
    ref = ho.track_reference(("track", dt), poses, v6, active)
    assert not ho.track_caps(kk, ref)
    T, B = poses.shape[:2]
    eng = env.engine.Engine(env.robots.lwr(), B, io_dtype=dt, max_slots=2)
    esz = np.dtype(dt).itemsize
    d_pose, d_v6, d_out, d_act = eng.dev_alloc(B * 16 * esz), eng.dev_alloc(B * 6 * esz), eng.dev_alloc(B * 8 * esz), eng.dev_alloc(B * 4)
    got = np.zeros((2, T, B, 8), dtype=dt)
    try:
        for rep in range(2):
            eng.h2d(d_out, np.zeros((B, 8), dtype=dt))
            for t in range(T):
                eng.h2d(d_pose, poses[t].astype(dt))
                eng.h2d(d_v6, v6[t].astype(dt))
                eng.h2d(d_act, active[t])
                eng.track_error(d_pose, d_v6, d_out, d_act)
                eng.d2h(got[rep, t], d_out)
            eng.track_reset()
    finally:
        for p in (d_pose, d_v6, d_out, d_act):
            eng.dev_free(p)
        eng.close()
    assert np.array_equal(got[0], got[1], equal_nan=True)   # track_reset: the history starts again
    for t in range(1, T):   # a silent arm's row stays
        assert np.array_equal(got[0, t][active[t] == 0], got[0, t - 1][active[t] == 0])
    ratio, wrong, amb = ho.track_ratios(got[0], ref, dt, active)
    print("track_kernel f%d: worst error / bar per output %s" % (32 if dt == np.float32 else 64, np.round(ratio.max(axis=(0, 1)), 3)))
    ho.note_track("gpu", "tracking f%d" % (32 if dt == np.float32 else 64), "track_kernel", ratio, amb, ref)
    miss = np.argwhere(ratio >= 1.0)[:6]
    assert ratio.max() < 1.0, [(int(t), int(b), kk[b], int(i), float(ratio[t, b, i])) for t, b, i in miss]
    assert not wrong.any(), [(int(t), int(b), kk[b]) for t, b in np.argwhere(wrong)[:6]]
    assert ref["valid"].sum() > B * (T - 6)


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_fused_observers_equal_the_stand_alone_kernels(env, dt):
    """io.track_error / io.obj_dist of a cycle call against track_kernel / monitor_kernel fed the PUBLISHED pose and v6 (the I/O-typed rows):
    bit for bit, over the estimator's whole history, with arms gated off in some cycles (their rows stay, their history does not move)."""
    abi = env.abi
    chain = env.robots.lwr()
    _, frames, kk = ho.monitor_scene(dt)
    gated = np.array([k == "gated" for k in kk])
    B, O = frames.shape[:2]
    K = 9
    w = env.synth.make_workload(chain, B, 2, seed=43, io_dtype=dt)
    eng = env.engine.Engine(chain, B, io_dtype=dt, max_slots=4, params=abi.default_params(flags=abi.F_NULLSPACE | abi.F_MIXER))
    alone = env.engine.Engine(chain, B, io_dtype=dt, max_slots=2)
    esz = np.dtype(dt).itemsize
    d_pose, d_v6, d_fr = alone.dev_alloc(B * 16 * esz), alone.dev_alloc(B * 6 * esz), alone.dev_alloc(B * O * 16 * esz)
    d_trk, d_mon, d_act = alone.dev_alloc(B * 8 * esz), alone.dev_alloc(B * O * 2 * esz), alone.dev_alloc(B * 4)
    try:
        eng.set_fields(w["fields"], w["nfields"])
        eng.set_objects(frames)
        alone.h2d(d_fr, frames.astype(dt))
        alone.h2d(d_trk, np.zeros((B, 8), dtype=dt))
        rng = np.random.default_rng(5)
        q = w["q"].copy()
        outs, trk, mon = None, np.zeros((B, 8), dtype=dt), np.zeros((B, O, 2), dtype=dt)
        values = 0
        for t in range(K):
            act = (rng.uniform(size=B) > 0.25) & ~gated if t in (2, 6) else np.ones(B, dtype=bool)   # the `gated` arms, and one in four others
            out = eng.step_host(q, want=("qdot_out", "pose", "v6", "track_error", "obj_dist"), active=None if act.all() else act, into=outs)
            prev_mon = mon.copy()
            alone.h2d(d_pose, out["pose"])
            alone.h2d(d_v6, out["v6"])
            alone.h2d(d_act, act.astype(np.int32))
            alone.track_error(d_pose, d_v6, d_trk, d_act)
            alone.object_distances(d_pose, d_fr, O, d_mon)
            alone.d2h(trk, d_trk)
            alone.d2h(mon, d_mon)
            mon[~act] = prev_mon[~act]   # (the stand-alone monitor has no gate: a gated arm's rows stay)
            if not act.all():
                assert not act[gated].any() and np.array_equal(out["obj_dist"][gated], prev_mon[gated])   # "a gated arm: its rows stay"
            assert np.array_equal(out["track_error"], trk, equal_nan=True), (t, np.argwhere(out["track_error"] != trk)[:5])
            assert np.array_equal(out["obj_dist"], mon, equal_nan=True), (t, np.argwhere(out["obj_dist"] != mon)[:5])
            values += int((trk[:, 2:6] != 0).any(axis=1).sum())
            outs = dict(out)
            follow = np.where(np.arange(B) % 5 == 0, 0.0, 0.8)[:, None]   # every fifth arm is frozen: the (1, 0, 0) defaults
            q = (q + (1.0 / 150.0) * follow * np.where(act[:, None], out["qdot_out"].astype(np.float64), 0.0)).astype(dt).astype(np.float64)
        assert values > B * (K - 6) // 2
    finally:
        for p in (d_pose, d_v6, d_fr, d_trk, d_mon, d_act):
            alone.dev_free(p)
        alone.close()
        eng.close()


def _goal_run(env, robot, dt, family):
    """One family's launch on the goal scene: (goal_dist (B, 2), reference, kinds, the kernels launched)."""
    import kernel_variants as kv
    from oracle import oracle_c
    tname = "turned" if family == "shared_tool" else None
    chain, params, w, kk, di, tool16 = ho.goal_scene(oracle_c, robot, dt, tname)
    F = w["fields"].copy()
    if family == "general":
        F["p"][:, 2, 5] = 4.5   # one fractional decay order: the general field path
    ref = ho.goal_reference((robot, dt, tname), chain, w["q"], F["p"][:, 0, :16], tool16)
    eng = env.engine.Engine(chain, len(kk), io_dtype=dt, max_slots=4, params=params)
    try:
        eng.set_small_batch_kernel(0)
        eng.set_fields(F, w["nfields"])
        if tool16 is not None:
            eng.set_tool(tool16)
        assert eng.field_path == (0 if family == "general" else 1)
        eng.launched_kernels()
        if family == "rollout":
            got = eng.rollout_host(w["q"], 1, 1e-3, want=("qdot_out", "goal_dist"))
        else:
            got = eng.step_host(w["q"], want=("qdot_out", "goal_dist", "status"))
        names = eng.launched_kernels()
    finally:
        eng.close()
    assert len(names) == 1, names
    v = kv.parse(next(iter(names)))
    a = v.args
    assert a["NJ"] == chain.n and a["T"] == ("float" if dt == np.float32 else "double"), v.name
    assert a.get("FASTF", True) == (family != "general") and bool(a.get("ROLL", False)) == (family == "rollout"), v.name
    assert bool(a["D"] & 2) == (family == "shared_tool"), v.name
    return got["goal_dist"], ref, kk, v.name


GOAL_CASES = [(r, t, f) for r in ho.GOAL_ROBOTS for t in DTYPES for f in ("straight", "general", "shared_tool", "rollout")
              if (f != "shared_tool" or t == np.float32)            # the shared-tool variants are float32 kernels
              and (f != "rollout" or r != "lwr_dual14")]            # chains beyond 7 joints have no in-kernel rollout: the caller steps them


@pytest.mark.parametrize("robot,dt,family", GOAL_CASES, ids=["%s-f%d-%s" % (r, 32 if t == np.float32 else 64, f) for r, t, f in GOAL_CASES])
def test_goal_distance_at_its_edges(env, robot, dt, family):
    """io.goal_dist of a straight-line-path single cycle, a general-field-path single cycle, a shared-tool float32 launch and an in-kernel
    one-cycle rollout -- each asserted by kernel name -- against the 50-digit reference: theta -> 0, D -> 0, either side of the s = 1e-4 switch
    between atan2_pos and the half-turn series, an exact half turn, goals that are no rotations to the last bit."""
    got, ref, kk, name = _goal_run(env, robot, dt, family)
    assert not ho.caps(kk, ref)
    rD, rA = ho.ratios(got[:, None, :], ref, dt)
    what = "goal %s f%d %s" % (robot, 32 if dt == np.float32 else 64, family)
    print("%s (%s): worst error / bar  D %.3f  angle %.3f" % (what, name.split("<")[0], rD.max(), rA.max()))
    ho.note("gpu", what, name.split("<")[0], rD, rA, ref)
    worst = np.argwhere((rD >= 1.0) | (rA >= 1.0))[:6]
    assert rD.max() < 1.0 and rA.max() < 1.0, [(int(b), kk[b], float(rD[b, 0]), float(rA[b, 0])) for b, _ in worst]


@pytest.mark.parametrize("robot", ho.GOAL_ROBOTS)
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_arrival_decisions_at_the_threshold(env, dt, robot):
    """goto_host with one cycle, one check and a batch-wide precision of (1e-3 m, 1e-3 rad), goals at threshold (1 +- {1e-9, 1e-6, 1e-3}) in D
    or in the angle: `arrived` equals the 50-digit reference's rule for every arm outside the band (at most 5 % inside, asserted on the CPU)."""
    from oracle import oracle_c
    chain, params, w, kk = ho.arrive_scene(oracle_c, robot, dt)
    ref = ho.goal_reference((robot, dt, "arrive"), chain, w["q"], w["fields"]["p"][:, 0, :16])
    arr, amb = ho.arrive_rule(ref, dt)
    assert amb.sum() <= ho.AMBIGUOUS_CAP * len(kk)
    eng = env.engine.Engine(chain, len(kk), io_dtype=dt, max_slots=4, params=params)
    try:
        eng.set_fields(w["fields"], w["nfields"])
        got = eng.goto_host(w["q"], 1, 1e-3, ho.ARRIVE_PREC, want=("qdot_out", "goal_dist"))
    finally:
        eng.close()
    mine = got["arrived"] >= 0
    assert np.all(got["arrived"][mine] == 0)
    wrong = np.flatnonzero((mine != arr) & ~amb)
    print("arrival %s f%d: %d arrive, %d in the band, %d wrong" % (robot, 32 if dt == np.float32 else 64, arr.sum(), amb.sum(), len(wrong)))
    assert len(wrong) == 0, [(int(b), kk[b], ho.arrive_delta(b)) for b in wrong[:8]]
    ho.note_track("gpu", "arrival %s f%d" % (robot, 32 if dt == np.float32 else 64), "goto_host", np.array([[[float(len(wrong))]]]), amb[None, :],
                  {"finite_only": np.zeros((1, len(kk), 1), dtype=bool)})


@pytest.mark.parametrize("robot", ho.GOAL_ROBOTS)
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_fused_object_0_against_goal_dist(env, dt, robot):
    """Object 0 of the fused monitor is the goal: its entry against the cycle kernel's own goal_dist on the goal-distance edge scene, D and
    the ANGLE.  The monitor words the rotation R^T G on the published (I/O-typed) pose, the cycle kernel G R^T on its own pose in doubles: each
    is held to the 50-digit reference of its wording, and their difference to the difference of the two references within the sum of the two
    bars -- the bar that allows for the wordings' difference (printed: some 1e-8 rad for float32 frames next to a half turn) and for nothing else."""
    from oracle import oracle_c
    chain, params, w, kk, di, _ = ho.goal_scene(oracle_c, robot, dt, None)
    goals = w["fields"]["p"][:, 0, :16]
    gref = ho.goal_reference((robot, dt, None), chain, w["q"], goals, None)
    eng = env.engine.Engine(chain, len(kk), io_dtype=dt, max_slots=4, params=params)
    try:
        eng.set_fields(w["fields"], w["nfields"])
        eng.set_objects(np.stack([goals, goals], axis=1))
        out = eng.step_host(w["q"], want=("qdot_out", "pose", "goal_dist", "obj_dist"))
    finally:
        eng.close()
    assert np.array_equal(out["obj_dist"][:, 0], out["obj_dist"][:, 1])
    mref = ho.reference(("object 0", robot, dt), out["pose"].astype(np.float64), goals[:, None, :])
    assert not ho.caps(kk, mref) and not ho.caps(kk, gref)
    mD, mA = ho.ratios(out["obj_dist"][:, :1], mref, dt)
    gD, gA = ho.ratios(out["goal_dist"][:, None, :], gref, dt)
    pD, pA = ho.pair_ratio(out["obj_dist"][:, 0], out["goal_dist"], mref, gref, dt)
    forms = np.abs((mref["ang"] - gref["ang"]) + (mref["ang_lo"] - gref["ang_lo"])).max() * np.pi / 180.0
    what = "object 0 %s f%d" % (robot, 32 if dt == np.float32 else 64)
    print("%s: worst / bar  monitor D %.3f angle %.3f  goal_dist D %.3f angle %.3f  pair D %.3f angle %.3f; the references differ by up to %.2e rad"
          % (what, mD.max(), mA.max(), gD.max(), gA.max(), pD.max(), pA.max(), forms))
    ho.note("gpu", what, "monitor vs cycle", pD[:, None], pA[:, None], mref)
    assert max(mD.max(), mA.max(), gD.max(), gA.max()) < 1.0
    worst = np.argwhere((pD >= 1.0) | (pA >= 1.0))[:6, 0]
    assert pD.max() < 1.0 and pA.max() < 1.0, [(int(b), kk[b], float(pD[b]), float(pA[b])) for b in worst]
