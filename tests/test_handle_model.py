"""The walks of tests/handle_model.py can catch what they are for: on the CPU, with the C oracle and the pure-host scene driver
(tests/c_host/scene_plan.cpp, built and asked as tests/test_scene_plan.py does it) alone, over exactly the configurations and seeds that
tests/test_gpu_handle_history.py runs on a handle.

`runs` walks every (configuration, seed) once with the right model and records, per step: whether the operation was refused, the plan of the
model's WHOLE field state packed in one call, the oracle's answer at the checkpoint, how far the operation moved that answer (the same
checkpoint on a copy of the model that did not get the operation), and how far every wrong-rule model is from the right one.  The tests
below read that record.

test_a_rounding_rule_is_seen: the three rounding rules (handle_model.ROUNDING_RULES) change half a float32 ulp of a coordinate -- 4e-9 m on
a tool translation of 0.12 m --, which on an ordinary scene moves qdot_out by 1e-7 .. 6e-6.  The walk's amplifier arm (handle_model.walk:
amp_op) stands 0.2 um from a goal with a slow-down distance of 0.5 um, where that much moves the twist by a percent: a model with one of
these rules wrong is then held to the same 1e-3 as the others, at the float32 configurations (at float64 I/O nothing is rounded and such a
model IS the right one)."""
import collections
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import handle_model as hm  # noqa: E402
from test_scene_plan import ask, driver  # noqa: E402,F401  (driver: the fixture that builds tests/c_host/scene_plan.cpp)

from vfclik_amd import _abi  # noqa: E402

MOVED_MIN = 1e-3          # FEATURE_MIN of tests/test_gpu_variants.py, for the same reason: far above every bar, small against a command
Rec = collections.namedtuple("Rec", "op accepted plan flags ref moved wrong named")


def copy_states(m, right):
    C.memmove(m.states, right.states, C.sizeof(m.states))


def named_arms(op):
    """[first, end) of the arms a vfik_set_fields names"""
    first = op.kw.get("first_arm", 0)
    return first, first + (op.args[0].shape[0] if op.name == "set_fields" else 0)


def run_walk(oc, drv, cfg, seed, variants):
    chain, params0, steps = hm.walk(oc, seed, cfg)
    right = hm.Model(oc, chain, cfg.B, cfg.io_dtype, cfg.max_slots, params0)
    wrong = {v: hm.Model(oc, chain, cfg.B, cfg.io_dtype, cfg.max_slots, params0, wrong=v) for v in variants}
    recs, requests, at = [], [], []
    for i, (op, ck) in enumerate(steps):
        before = right.clone() if (op.changes and not op.refused) else None
        accepted = hm.apply(right, op)
        for m in wrong.values():
            hm.apply(m, op)
        if accepted and op.name == "set_fields":
            requests.append(hm.whole_plan_request(right))
            at.append(i)
        flags = int(right.params.flags)
        after = right.clone() if (before is not None and ck.form == "gate") else None
        ref = hm.expect(right, ck)
        moved = None
        if before is not None and (flags & op.needs) == op.needs:
            if ck.form == "gate":    # (a gate may silence the one arm the call named: the same angles without it)
                ck_m = ck._replace(form="publish", active=None)
                moved = float(np.abs(hm.expect(before, ck_m)["qdot_out"] - hm.expect(after, ck_m)["qdot_out"]).max())
            else:
                moved = float(np.abs(hm.expect(before, ck)["qdot_out"] - ref["qdot_out"]).max())
        dist = {}
        for v, m in wrong.items():
            if m.same_values(right):
                copy_states(m, right)      # the same values give the same answer: no oracle call, the sign memory follows
                dist[v] = 0.0
            else:
                dist[v] = float(np.abs(hm.expect(m, ck)["qdot_out"] - ref["qdot_out"]).max())
        recs.append(Rec(op, accepted, None, flags, ref, moved, dist, named_arms(op)))
    plans = [hm.parse_plan(ln) for ln in ask(drv, "plan", requests)]
    plan, k = None, 0
    for i in range(len(recs)):
        if k < len(at) and at[k] == i:
            plan, k = plans[k], k + 1
        recs[i] = recs[i]._replace(plan=plan)
    return chain, steps, recs


@pytest.fixture(scope="module")
def runs(oracle_c, driver):  # noqa: F811
    variants = tuple(hm.WRONG_RULES) + tuple(hm.ROUNDING_RULES)
    return {(cfg.name, seed): run_walk(oracle_c, driver, cfg, seed, variants) for cfg in hm.CONFIGS for seed in hm.SEEDS}


def all_recs(runs):
    return [r for _, _, recs in runs.values() for r in recs]


def test_every_operation_range_and_refusal_occurs(runs):
    recs = all_recs(runs)
    kinds = collections.Counter(r.op.kind for r in recs)
    expected = {"set_fields", "set_params:flags", "set_params:lambda", "set_params:speed_scale", "set_params:same", "set_params:wq", "set_params:wy",
                "set_params:max_vel", "set_params:mix_w", "set_arm_weights", "set_mixer_weights", "set_mixer_weights:none", "set_max_vel",
                "set_tool:shared", "set_tool:per_arm", "set_speed_scale", "move_fields_host", "move_scene_host", "set_ext_cmd", "reset_state",
                "set_small_batch_kernel"}
    assert all(kinds[k] >= 3 for k in expected), {k: kinds[k] for k in expected if kinds[k] < 3}
    refusals = {"refused_too_many", "refused_weight", "refused_speed_negative", "refused_speed_nan", "refused_range", "refused_move_before_set"}
    assert all(kinds[k] >= 1 for k in refusals), kinds
    for r in recs:
        assert r.accepted != r.op.refused, r.op
    # ... and in every walk of 48 operations each range kind
    for (name, seed), (_, _, rs) in runs.items():
        if len(rs) >= 48:
            assert {r.op.range_kind for r in rs} >= {"whole", "one", "cross", "last"}, (name, seed)
    forms = collections.Counter(st.check.form for _, steps, _ in runs.values() for st in steps)
    assert all(forms[f] >= 10 for f in hm.FORMS), forms
    assert {r.flags for r in recs} == set(hm.FLAG_SETS)


def test_a_refused_call_changes_nothing(oracle_c):
    seen = set()
    for cfg in hm.CONFIGS[:5]:
        for seed in hm.SEEDS:
            chain, params0, steps = hm.walk(oracle_c, seed, cfg)
            m = hm.Model(oracle_c, chain, cfg.B, cfg.io_dtype, cfg.max_slots, params0)
            for op, _ in steps:
                before = m.clone() if op.refused else None
                hm.apply(m, op)
                if op.refused:
                    assert m.same_values(before) and m.fields_set == before.fields_set and m.bridge == before.bridge, op
                    seen.add(op.kind)
    assert len(seen) == 6, seen


def test_every_plan_is_reached_and_flipped_by_a_partial_call(runs):
    for (name, seed), (chain, _, recs) in runs.items():
        plans = [r.plan for r in recs if r.plan is not None]
        one_chunk_possible = name.endswith("f32") and chain.n <= 7
        if len(recs) >= 48:   # (the walk of 16 operations has a shorter program: it counts in the union below)
            assert {p["field_path"] for p in plans} == {0, 1, 2}, (name, seed)
            assert {p["uniform"] for p in plans} == {0, 1} and {p["mixed_orders"] for p in plans} == {0, 1}, (name, seed)
            assert {p["one_chunk"] for p in plans} == ({0, 1} if one_chunk_possible else {0}), (name, seed)
        seen = set()
        prev = None
        for r in recs:
            if r.accepted and r.op.name == "set_fields" and prev is not None:
                a, b = prev, r.plan
                partial = r.named[1] - r.named[0] < r.ref["qdot_out"].shape[0]     # at least one arm outside the call
                if partial:
                    straight = lambda p: p["field_path"] != 0  # noqa: E731
                    if straight(a) and straight(b) and a["uniform"] and not b["uniform"]:
                        seen.add("uniform->compact")
                    if straight(a) and straight(b) and not a["uniform"] and b["uniform"]:
                        seen.add("compact->uniform")
                    if straight(a) and not straight(b):
                        seen.add("straight->general")
                    if not straight(a) and straight(b):
                        seen.add("general->straight")
                    if b["slots_used"] < a["slots_used"]:
                        seen.add("slots drop")
            if r.plan is not None:
                prev = r.plan
        want = {"uniform->compact", "compact->uniform", "straight->general", "general->straight", "slots drop"}
        if len(recs) < 48:
            want -= {"slots drop"}
        assert seen >= want, (name, seed, want - seen)


def test_state_changing_operations_move_the_result(runs):
    """Every kind of state-changing operation moves the oracle's qdot_out by MOVED_MIN somewhere in the batch at its checkpoint at least
    twice; a new field set and a new lambda do so every time they are drawn.  (A limiter speed above every arm's command, an external
    command on a channel of weight 0, batch-wide weights equal to the promoted ones in force: drawn where they cannot matter.)"""
    moved = collections.defaultdict(list)
    for r in all_recs(runs):
        if r.moved is not None:
            moved[r.op.kind].append(r.moved)
    kinds = {"set_fields", "set_params:flags", "set_params:lambda", "set_params:speed_scale", "set_params:wq", "set_params:wy", "set_params:max_vel",
             "set_params:mix_w", "set_arm_weights", "set_mixer_weights", "set_mixer_weights:none", "set_max_vel", "set_tool:shared", "set_tool:per_arm",
             "set_speed_scale", "move_fields_host", "move_scene_host", "set_ext_cmd", "reset_state"}
    few = {k: sorted(moved[k])[-2:] for k in kinds if sum(1 for v in moved[k] if v >= MOVED_MIN) < 2}
    assert not few, few
    for k in ("set_fields", "set_params:lambda"):
        assert min(moved[k]) >= MOVED_MIN, (k, min(moved[k]))


@pytest.mark.parametrize("variant", sorted(hm.WRONG_RULES))
def test_a_wrong_rule_is_seen(runs, variant):
    """a handle with this one rule wrong is MOVED_MIN from the oracle at some checkpoint of EVERY configuration, in at least one seed"""
    worst = {cfg.name: max(r.wrong[variant] for seed in hm.SEEDS for r in runs[(cfg.name, seed)][2]) for cfg in hm.CONFIGS}
    print(variant, {k: "%.2e" % v for k, v in worst.items()})
    short = {k: v for k, v in worst.items() if not v >= MOVED_MIN}
    assert not short, (variant, short)


@pytest.mark.parametrize("variant", sorted(hm.ROUNDING_RULES))
def test_a_rounding_rule_is_seen(runs, variant):
    """the same for the rules that round, where there is something to round: every float32 configuration"""
    worst = {cfg.name: max(r.wrong[variant] for seed in hm.SEEDS for r in runs[(cfg.name, seed)][2]) for cfg in hm.CONFIGS}
    print(variant, {k: "%.2e" % v for k, v in worst.items()})
    for cfg in hm.CONFIGS:
        if cfg.io_dtype == np.float64:
            assert worst[cfg.name] == 0.0, (variant, cfg.name)
        else:
            assert worst[cfg.name] >= MOVED_MIN, (variant, worst)


def test_the_sign_decision_stays_away_from_its_tie(oracle_c):
    """A condition on the inputs: behind every cycle the oracle runs for a 7-joint arm -- each cycle of a rollout and of a goto block, not
    only each launch (handle_model.SignWatch) -- its previous and new null vector have a normalised dot product above 0.9 in magnitude, and
    no arm's status carries VFIK_ST_NULL_AMBIGUOUS.  (Chains of 8 and more joints carry that bit at every pose -- their nullspace has two
    dimensions and more, include/vfik.h -- and keep no sign.)  tests/test_gpu_handle_history.py asserts the same of every launch it makes,
    the directed sequences included."""
    for cfg in hm.CONFIGS:
        if hm.chain_of(cfg).n != 7:
            continue
        for seed in hm.SEEDS:
            chain, params0, steps = hm.walk(oracle_c, seed, cfg)
            m = hm.Model(oracle_c, chain, cfg.B, cfg.io_dtype, cfg.max_slots, params0)
            watch = hm.SignWatch(m)
            for i, (op, ck) in enumerate(steps):
                hm.apply(m, op)
                ref = hm.expect(m, ck)
                assert watch.worst > 0.9, (cfg.name, seed, i, op, watch.worst)
                if m.params.flags & _abi.F_NULLSPACE:
                    assert not np.any(ref["status"] & _abi.ST_NULL_AMBIGUOUS), (cfg.name, seed, i, op)


def test_the_model_is_the_oracle_for_batch_wide_state(oracle_c):
    """only batch-wide operations: Model.reference is one plain oracle call on the same arrays, bit for bit"""
    from vfclik_amd import robots, synth
    chain = robots.lwr()
    B = 37
    for io in (np.float32, np.float64):
        w = synth.make_workload(chain, B, 3, seed=5, io_dtype=io)
        tool = hm.tool_frame(1)
        ext = np.random.default_rng(2).uniform(-0.1, 0.1, (B, 7))
        kw = dict(flags=hm.F_NS | hm.F_MIX | hm.F_LIM, max_vel=0.5, speed_scale=0.75, wq=hm.wq_row(7, 1), mix_w=hm.MIX_ROWS[2], **{"lambda": 0.05})
        m = hm.Model(oracle_c, chain, B, io, 16)
        m.set_fields(w["fields"], w["nfields"])
        m.set_params(**kw)
        m.set_tool(tool)
        m.set_ext_cmd(2, ext)
        want = tuple(k for k in hm.ALL_ROWS)
        states = oracle_c.new_states(B, 7)
        e = np.zeros((4, B, 7))
        e[0] = m.rnd(ext)
        for step in range(3):
            q = w["q"] + 0.01 * step
            got = m.reference(q, want)
            ref = oracle_c.cycle_batch(chain, _abi.default_params(**kw), m.rnd(q), w["fields"], w["nfields"], tool=tool, ext_cmd=e, states=states, want=want)
            for k in want:
                assert got[k].tobytes() == ref[k].tobytes(), (np.dtype(io).name, step, k)
