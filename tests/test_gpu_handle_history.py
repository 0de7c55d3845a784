"""One Engine, created once and then driven through setters, moves and launches of every family, held to the oracle all the way.

THE WALKS: tests/handle_model.py's seeded walks (CONFIGS x SEEDS; tests/test_handle_model.py shows on the CPU what they reach) on ONE handle
each.  After every operation a checkpoint: one launch of a drawn form -- lean step, publishing step, gated step, step with per-arm limits,
rollout of 3 cycles, goto of 4 cycles in two blocks -- whose every output equals `Model.reference` within the suite's own bars (1e-9 at
float64 I/O, 1e-6 at float32: hp_reference.S_BAR), status exactly, the rows of gated arms untouched.  After every vfik_set_fields the
handle's decisions equal the pure-host driver's plan of the model's whole field state packed in one call.  vfik_launch_epoch moves on
every accepted set_* / reset_state and on no move and no launch.  Every 8th operation and at the end a FRESH handle is built from the
model in one canonical order, both forget their sign memory and run one publishing step: where both launched the same kernels the outputs
are equal byte for byte, else both meet the bars; at least half of the comparisons of a walk are byte for byte.

THE DIRECTED SEQUENCES (a) ... (f): the transitions the walks are drawn for, each guaranteed, on the LWR at both I/O types.

Measured (MI355X): profiles/handle_history.txt, written by this file with VFIK_HANDLE_HISTORY_TABLE=<file>: the largest error against the
oracle per configuration and launch form, and the byte-for-byte counts."""
import collections
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import handle_model as hm  # noqa: E402
import hp_reference as hp  # noqa: E402
from test_scene_plan import ask, driver  # noqa: E402,F401  (driver: the fixture that builds tests/c_host/scene_plan.cpp)

pytestmark = pytest.mark.gpu

WORST = collections.defaultdict(float)      # (configuration, form) -> the largest |got - oracle| of any output
BYTES = {}                                  # walk -> (byte-for-byte comparisons, comparisons)
SENTINEL, SENTINEL_STATUS = -777.0, -7


@pytest.fixture(scope="module")
def env(driver):  # noqa: F811
    import __graft_entry__ as g
    g.build()
    from oracle import oracle_c
    from vfclik_amd import _abi, engine, robots
    oracle_c.build()

    class E:
        pass

    e = E()
    e.oc, e.abi, e.engine, e.robots, e.driver = oracle_c, _abi, engine, robots, driver
    yield e
    path = os.environ.get("VFIK_HANDLE_HISTORY_TABLE")
    if path and WORST:
        with open(path, "w") as f:
            f.write("# tests/test_gpu_handle_history.py on an MI355X: the largest |got - oracle| over every output of every checkpoint, per configuration\n"
                    "# (walks of both seeds, directed sequences) and launch form; bars 1e-6 (float32 I/O) and 1e-9 (float64 I/O), status exact\n")
            for (name, form), v in sorted(WORST.items()):
                f.write("%-22s %-8s %.3e\n" % (name, form, v))
            f.write("# comparisons with a fresh handle that were byte for byte (same kernels launched) / all, per walk\n")
            for name, (same, total) in sorted(BYTES.items()):
                f.write("%-22s %d / %d\n" % (name, same, total))


def sentinel_rows(eng, want):
    return {k: np.full(eng._out_spec(k)[0], SENTINEL_STATUS if k == "status" else SENTINEL, dtype=eng._out_spec(k)[1]) for k in want}


def compare(got, ref, io_dtype, active=None, sentinel=None):
    """[(key, arms that fail, largest error)] and the largest error of the launch"""
    bar = hp.S_BAR[np.dtype(io_dtype).type]
    act = np.ones(len(ref["status"]), dtype=bool) if active is None else np.asarray(active) != 0
    bad, worst = [], 0.0
    for k, g in got.items():
        if k not in ref:
            continue
        if k == "status":
            wrong = act & (g != ref[k])
        else:
            err = np.abs(g.astype(np.float64) - ref[k]).reshape(len(act), -1)
            err = np.where(np.isnan(err), np.inf, err).max(axis=1)
            worst = max(worst, float(err[act].max()) if act.any() else 0.0)
            wrong = act & ~(err <= bar)
        if sentinel is not None:    # a silent arm's rows are untouched
            wrong = wrong | (~act & np.any((g != sentinel[k]).reshape(len(act), -1), axis=1))
        if wrong.any():
            bad.append((k, np.flatnonzero(wrong)[:12].tolist(), float(err[wrong].max()) if k != "status" and (wrong & act).any() else None))
    return bad, worst


class Driven:
    """a handle and its model, side by side"""

    def __init__(self, env, name, chain, B, io_dtype, max_slots, params):
        self.env, self.name, self.io = env, name, np.dtype(io_dtype)
        self.model = hm.Model(env.oc, chain, B, io_dtype, max_slots, params)
        self.eng = env.engine.Engine(chain, B, io_dtype=io_dtype, max_slots=max_slots, params=hm.copy_params(params))
        self.watch = hm.SignWatch(self.model) if chain.n == 7 else None
        self.log = []

    def close(self):
        self.eng.close()

    def op(self, op):
        e0 = self.eng.launch_epoch
        ok_m, ok_e = hm.apply(self.model, op), hm.apply(self.eng, op)
        self.log.append(repr(op))
        assert ok_e == ok_m == (not op.refused), "%s: %s -- the handle %s, the model %s" % (self.where(), op, "accepted" if ok_e else "refused", "accepted" if ok_m else "refused")
        e1 = self.eng.launch_epoch
        if op.name.startswith("move_"):
            assert e1 == e0, "%s: %s moved vfik_launch_epoch" % (self.where(), op)
        elif ok_e:
            assert e1 > e0, "%s: %s left vfik_launch_epoch where it was" % (self.where(), op)
        return ok_e

    def call(self, name, *args, **kw):
        return self.op(hm.Op(name, args, kw))

    def where(self):
        return "%s, operation %d" % (self.name, len(self.log) - 1)

    def check(self, ck):
        eng = self.eng
        e0 = eng.launch_epoch
        eng.launched_kernels()
        sentinel = sentinel_rows(eng, hm.ALL_ROWS) if ck.form == "gate" else None
        keep = None if sentinel is None else {k: v.copy() for k, v in sentinel.items()}
        got = hm.launch(eng, ck, sentinel)
        ref = hm.expect(self.model, ck)
        kernels = sorted(eng.launched_kernels())
        # a condition on the inputs (tests/test_handle_model.py): no cycle of this launch brought a sign decision near its tie
        assert self.watch is None or self.watch.worst > 0.9, "%s: the null vector turned by acos(%.3f) within one cycle" % (self.where(), self.watch.worst)
        assert eng.launch_epoch == e0, "%s: a launch moved vfik_launch_epoch" % self.where()
        bad, worst = compare(got, ref, self.io, ck.active, keep)
        key = (self.name.split(" ")[0], ck.form)
        WORST[key] = max(WORST[key], worst)
        assert not bad, "%s (%s), %s checkpoint: %s\n  kernels %s\n  history %s" % (self.where(), self.log[-1] if self.log else "-", ck.form, bad, kernels, self.log[-6:])

    def step(self, q, form="publish", **kw):
        """a checkpoint of the directed sequences: all of them at the same joint angles"""
        B = self.model.B
        ctrl = np.linspace(-1.0, 1.0, 4 * B).reshape(B, 4).astype(self.io).astype(np.float64)
        self.check(hm.Check(form, q, ctrl, kw.get("active"), kw.get("q_lo"), kw.get("q_hi")))

    def plan_is(self, want):
        eng = self.eng
        got = dict(slots_used=eng.slots_in_use, field_path=eng.field_path, mixed_orders=int(eng.mixed_orders), uniform=int(eng.uniform_repellers),
                   one_chunk=int(eng.one_chunk))
        assert got == want, "%s (%s): the handle decides %s, a fresh pack of the same field state %s" % (self.where(), self.log[-1], got, want)

    def fresh(self):
        """a fresh handle built from the model in one canonical order: params, whole-batch fields, tool, weights, bridge rows, speed scales,
        external channels (and the small-batch knob, which changes no value but the launch)"""
        m = self.model
        eng = self.env.engine.Engine(m.chain, m.B, io_dtype=m.io_dtype, max_slots=m.max_slots, params=hm.copy_params(m.params))
        if m.fields_set:
            eng.set_fields(m.fields, m.counts)
        if np.all(m.tool == m.tool[0]):
            eng.set_tool(m.tool[0], per_arm=False)      # (stored as given: the model's values, whichever call rounded them)
        else:
            eng.set_tool(m.tool, per_arm=True)
        batch = np.concatenate([np.array(m.params.wy[:6]), np.array(m.params.wq[:m.n])])
        if not np.all(np.concatenate([m.wy, m.wq], axis=1) == batch):
            eng.set_arm_weights(wy=m.wy, wq=m.wq)
        if m.bridge:
            eng.set_mixer_weights(m.mix)
            eng.set_max_vel(m.max_vel)
        eng.set_speed_scale(m.speed)
        for ch in range(4):
            if np.any(m.ext[ch] != 0.0):
                eng.set_ext_cmd(2 + ch, m.ext[ch])
        if m.small_batch is not None:
            eng.set_small_batch_kernel(m.small_batch)
        return eng

    def against_fresh(self, q, ctrl):
        """True when the comparison was byte for byte"""
        other = self.fresh()
        try:
            self.eng.reset_state()
            other.reset_state()
            self.model.reset_state()
            self.eng.launched_kernels()
            a = self.eng.step_host(q, null_control=ctrl, want=hm.ALL_ROWS)
            b = other.step_host(q, null_control=ctrl, want=hm.ALL_ROWS)
            ka, kb = self.eng.launched_kernels(), other.launched_kernels()
            ref = self.model.reference(q, hm.ALL_ROWS, ctrl=ctrl)
            if ka == kb:
                diff = [k for k in hm.ALL_ROWS if a[k].tobytes() != b[k].tobytes()]
                assert not diff, "%s: %s differ from a fresh handle's that launched the same %s\n  history %s" % (self.where(), diff, sorted(ka), self.log[-8:])
            for who, got, kern in (("the old handle", a, ka), ("the fresh handle", b, kb)):
                bad, _ = compare(got, ref, self.io)
                assert not bad, "%s, against a fresh handle: %s misses the oracle: %s\n  kernels %s" % (self.where(), who, bad, sorted(kern))
            return ka == kb
        finally:
            other.close()


@pytest.mark.parametrize("seed", hm.SEEDS)
@pytest.mark.parametrize("cfg", hm.CONFIGS, ids=[c.name for c in hm.CONFIGS])
def test_a_long_lived_handle_stays_on_the_oracle(env, cfg, seed):
    chain, params0, steps = hm.walk(env.oc, seed, cfg)
    # the plans a fresh pack of the whole field state gives, for every accepted vfik_set_fields of the walk: one pass of the model alone
    m = hm.Model(env.oc, chain, cfg.B, cfg.io_dtype, cfg.max_slots, params0)
    requests = [hm.whole_plan_request(m) for op, _ in steps if hm.apply(m, op) and op.name == "set_fields"]
    plans = iter([hm.parse_plan(ln) for ln in ask(env.driver, "plan", requests)])
    d = Driven(env, "%s seed %d" % (cfg.name, seed), chain, cfg.B, cfg.io_dtype, cfg.max_slots, params0)
    same = total = 0
    try:
        for i, (op, ck) in enumerate(steps):
            if d.op(op) and op.name == "set_fields":
                d.plan_is(next(plans))
            d.check(ck)
            if (i + 1) % 8 == 0 or i == len(steps) - 1:
                same += int(d.against_fresh(ck.q, ck.ctrl))
                total += 1
    finally:
        d.close()
    BYTES["%s seed %d" % (cfg.name, seed)] = (same, total)
    # a condition on the walk's design (whole-batch operations bring the old handle back to the fresh one's kernels), not a measurement
    assert 2 * same >= total, "%d of %d comparisons with a fresh handle were byte for byte" % (same, total)


# ---- the directed sequences -----------------------------------------------------------------------------------------------------------
B_DIR = 203
IO = pytest.mark.parametrize("io_dtype", [np.float32, np.float64], ids=["f32", "f64"])


def directed(env, name, io_dtype, flags, n_rep=4):
    """(Driven, q, goals, tips, rng): the LWR, B_DIR arms, a feeder scene of n_rep repellers on every arm"""
    from vfclik_amd import synth
    chain = env.robots.lwr()
    w = synth.make_workload(chain, B_DIR, 0, seed=77, io_dtype=io_dtype)
    q = np.clip(w["q"], 0.9 * chain.q_lo, 0.9 * chain.q_hi).astype(io_dtype).astype(np.float64)
    goals = w["fields"]["p"][:, 0, :16].copy()
    tips = chain.fk(q).reshape(B_DIR, 16)[:, [3, 7, 11]]
    rng = np.random.default_rng(78)
    d = Driven(env, "directed-%s-%s" % (name, np.dtype(io_dtype).name), chain, B_DIR, io_dtype, 16, env.abi.default_params(flags=flags, max_vel=1.0))
    f, c = hm.records([hm.scene("feeder", goals[b], tips[b], rng, n_rep) for b in range(B_DIR)])
    d.call("set_fields", f, c)
    d.step(q)
    return d, q, goals, tips, rng


@IO
def test_a_moved_scene_through_image_flips(env, io_dtype):
    """(a) move every arm, then vfik_set_fields on the last arm alone flips the batch uniform -> compact -> general -> uniform: the moved
    coordinates of the arms the calls do not name are in force in each"""
    d, q, goals, tips, rng = directed(env, "a", io_dtype, hm.F_MIX)
    try:
        B = B_DIR
        g = goals.copy()
        g[:, [3, 7, 11]] += rng.uniform(-0.15, 0.15, (B, 3))
        dirs = rng.normal(size=(B, 4, 3))
        reps = np.concatenate([tips[:, None, :] + dirs / np.linalg.norm(dirs, axis=2, keepdims=True) * 0.2, np.full((B, 4, 1), 0.06)], axis=2)
        d.call("move_fields_host", goal=g, repellers=reps)
        assert d.eng.uniform_repellers and d.eng.field_path == 1
        d.step(q, "lean")
        for family, uniform, path in (("pair", False, 1), ("frac", False, 0), ("feeder", True, 1)):
            f, c = hm.records([hm.scene(family, goals[B - 1], tips[B - 1], rng)])
            d.call("set_fields", f, c, first_arm=B - 1)
            assert d.eng.uniform_repellers == uniform and d.eng.field_path == path, family
            d.step(q, "lean")
            d.step(q, "publish")
        assert np.array_equal(d.model.fields["p"][5, 0, :12], d.model.rnd(g[5, :12]))     # (the model kept the move, too)
    finally:
        d.close()


@IO
def test_promoted_weights_then_partial_ones(env, io_dtype):
    """(b) equal rows for the whole batch (promotion), wy alone on arms 60..70, vfik_set_params with the weights unchanged and another
    lambda, then with another wq"""
    d, q, *_ = directed(env, "b", io_dtype, hm.F_NS | hm.F_MIX)
    try:
        B = B_DIR
        d.call("set_arm_weights", wy=np.tile(hm.WY_ROWS[1], (B, 1)), wq=np.tile(hm.wq_row(7, 1), (B, 1)))
        d.step(q, "lean")
        d.call("set_arm_weights", wy=np.tile(hm.WY_ROWS[2], (11, 1)), first_arm=60)
        d.step(q, "lean")
        d.step(q, "publish")
        d.call("set_params", **{"lambda": 0.05})
        d.step(q, "lean")
        assert np.array_equal(d.model.wq[0], hm.wq_row(7, 1)) and np.array_equal(d.model.wy[65], hm.WY_ROWS[2])
        d.call("set_params", wq=hm.wq_row(7, 2))
        d.step(q, "lean")
        d.step(q, "rollout")
        assert np.array_equal(d.model.wy[65], np.ones(6))
    finally:
        d.close()


@IO
def test_equal_tools_one_other_equal_again_identity(env, io_dtype):
    """(c) per-arm tools: equal rows, one arm differs, equal again, the shared identity -- with values that are no float32 numbers"""
    d, q, *_ = directed(env, "c", io_dtype, hm.F_NS | hm.F_MIX)
    try:
        B = B_DIR
        t = np.tile(hm.tool_frame(1), (B, 1))
        assert np.any(t[0, :12] != t[0, :12].astype(np.float32))
        d.call("set_tool", t, per_arm=True)
        d.step(q, "lean")
        d.step(q, "publish")
        t2 = t.copy()
        t2[70] = hm.tool_frame(2)
        d.call("set_tool", t2, per_arm=True)
        d.step(q, "lean")
        d.step(q, "publish")
        d.call("set_tool", np.tile(hm.tool_frame(3), (B, 1)), per_arm=True)
        d.step(q, "publish")
        d.step(q, "rollout")
        d.call("set_tool", hm.tool_frame(0), per_arm=False)
        d.step(q, "lean")
        d.step(q, "publish")
    finally:
        d.close()


@IO
def test_sign_memory_across_kernel_families(env, io_dtype):
    """(d) the nullspace sign memory handed from family to family, the oracle's States carried through all of it"""
    d, q, *_ = directed(env, "d", io_dtype, hm.F_NS | hm.F_MIX)
    try:
        dq = 0.004 * np.sin(np.arange(q.size)).reshape(q.shape)
        at = lambda k: (q + k * dq).astype(io_dtype).astype(np.float64)  # noqa: E731
        d.step(at(1), "lean")
        d.step(at(2), "publish")
        d.call("set_small_batch_kernel", 0)
        d.step(at(3), "publish")
        d.step(at(4), "rollout")
        d.step(at(5), "gate", active=(np.arange(B_DIR) % 2).astype(np.int32))
        d.step(at(6), "lean")
        d.call("reset_state")
        d.step(at(7), "publish")
    finally:
        d.close()


@IO
def test_bridge_rows_through_params_and_resets(env, io_dtype):
    """(e) equal per-arm mixer rows and limiter speeds, vfik_set_params changing max_vel alone, vfik_set_mixer_weights(NULL), one arm's
    speed, vfik_set_params changing mix_w"""
    d, q, *_ = directed(env, "e", io_dtype, hm.F_NS | hm.F_MIX | hm.F_LIM)
    try:
        B = B_DIR
        d.call("set_mixer_weights", np.tile(hm.MIX_ROWS[2], (B, 1)))
        d.call("set_max_vel", np.full(B, 0.5))
        d.step(q, "lean")
        d.call("set_params", max_vel=0.25)
        d.step(q, "lean")
        assert np.all(d.model.max_vel == 0.25) and np.array_equal(d.model.mix[3], hm.MIX_ROWS[2])
        d.call("set_mixer_weights", None)
        d.step(q, "publish")
        d.call("set_max_vel", [0.75], first_arm=64)
        d.step(q, "lean")
        d.step(q, "publish")
        d.call("set_params", mix_w=hm.MIX_ROWS[1])
        d.step(q, "lean")
        d.step(q, "rollout")
        assert d.model.max_vel[64] == 0.75 and np.array_equal(d.model.mix[64], hm.MIX_ROWS[1])
    finally:
        d.close()


@IO
def test_speed_scales_through_fields_and_params(env, io_dtype):
    """(f) vfik_set_speed_scale on a range, vfik_set_fields on the same range (the speed stays), vfik_set_params with the speed_scale
    unchanged (stays), then changed (overwritten)"""
    d, q, goals, tips, rng = directed(env, "f", io_dtype, hm.F_MIX)
    try:
        d.call("set_speed_scale", np.full(11, 0.5), first_arm=60)
        d.step(q, "lean")
        f, c = hm.records([hm.scene("fewer", goals[b], tips[b], rng) for b in range(60, 71)])
        d.call("set_fields", f, c, first_arm=60)
        d.step(q, "lean")
        d.call("set_params", **{"lambda": 0.05})
        d.step(q, "lean")
        d.step(q, "publish")
        assert np.all(d.model.speed[60:71] == 0.5)
        d.call("set_params", speed_scale=0.75)
        d.step(q, "lean")
        d.step(q, "goto")
        assert np.all(d.model.speed == 0.75)
    finally:
        d.close()
