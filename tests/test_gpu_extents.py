"""Every entry point that takes a caller's device array, held to the extents of those arrays (tests/guard_arena.py).

A case is one launch, or one short move, run up to five times on one handle with reset_state() (and the scene put back) between the
runs: on arrays allocated each on its own (`plain`), and on arrays carved from a guard arena at skew 0 and at skew 1, each with the
bands next to the inputs filled with NaN and with huge numbers.  Asserted for each case:

  * no band is damaged and no input was written (Arena.damaged() is empty after a synchronise);
  * every output array equals the plain run's byte for byte -- the rows a call leaves alone included: gated arms, rows outside
    first_rep .. first_rep + L - 1, checks that did not run; the alignment only chooses how rows travel, the arithmetic is the same;
  * the `nan` and `huge` runs are equal byte for byte: no result depends on bytes in front of or behind an input;
  * launched_kernels() is the same set in all runs, and a cycle variant's case launched the variant it is named for;
  * every output array was written somewhere (a call that stores nothing would pass all of the above).

The cycle kernels: every instantiation of the built library (tests/kernel_variants.py) under the recipe of tests/test_gpu_variants.py,
at the recipes' 205 arms (a partial last wave; 205 x 7 x 4 bytes is no multiple of 16) and at 192 (a full last wave: the tile store
runs to the array's very end); the two-waves variants keep their one big batch, at skew 0.  One gated launch per group.
The aux kernels' device forms at 1, 65 and 203 arms, the five timed moves' at 203 arms, and one move of each kind with every rule on.

With VFIK_EXTENTS_TABLE=<file> the record kept in profiles/extents.txt is written there."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import coupled_reference as cr  # noqa: E402
import guard_arena as ga  # noqa: E402
import kernel_variants as kv  # noqa: E402
import test_gpu_move_scene as ms  # noqa: E402
import test_gpu_variants as tv  # noqa: E402

pytestmark = pytest.mark.gpu

GROUPS = tv.GROUPS
B_FULL = 64 * 3                  # the last wave is full: a tile store runs to the array's very end
BATCHES = (tv.B_SMALL, B_FULL)
AUX_B = (1, 65, 203)
MOVE_B, MOVE_CYCLES, MOVE_W, MOVE_DT = 203, 8, 3, 0.01
RUNS = (("plain", 0, "nan"), ("arena", 0, "nan"), ("arena", 0, "huge"), ("arena", 1, "nan"), ("arena", 1, "huge"))
I32 = np.int32


@pytest.fixture(scope="module")
def env():
    import __graft_entry__ as g
    g.build()
    import torch
    from oracle import oracle_c
    from vfclik_amd import _abi, chain, engine, robots, synth

    class E:
        pass

    e = E()
    e.oc, e.abi, e.chain, e.engine, e.robots, e.synth, e.torch = oracle_c, _abi, chain, engine, robots, synth, torch
    e.dev = "cuda:0"
    e.variants = kv.by_group()
    e.record = {}
    yield e
    path = os.environ.get("VFIK_EXTENTS_TABLE")
    if path and e.record:
        with open(path, "a") as f:
            if f.tell() == 0:
                f.write("tests/test_gpu_extents.py on an MI355X: per case family the calls run (listed below it), the regions carved from guard arenas, the\n"
                        "band and input bytes held to their fill, the bands found damaged, and the pairs of runs compared byte for byte\n"
                        "(arena against plain, NaN fill against huge fill).\n\n")
            for fam in sorted(e.record):
                r = e.record[fam]
                f.write("%-34s calls %d, regions carved %d, band bytes checked %d, damaged bands %d, runs compared %d\n" % (
                    fam, len(r["calls"]), r["regions"], r["band_bytes"], r["damaged"], r["runs"]))
                for c in sorted(r["calls"]):
                    f.write("    %s\n" % c)


class Spec:
    def __init__(self, name, shape, dtype, role, init=None, arg=None):
        self.name, self.shape, self.dtype, self.role, self.init, self.arg = name, tuple(shape), np.dtype(dtype), role, init, arg or name


def _in(name, init, dtype, arg=None):
    a = np.ascontiguousarray(init, dtype=dtype)
    return Spec(name, a.shape, dtype, "in", a, arg)


def _out(name, shape, dtype, arg=None):
    return Spec(name, shape, dtype, "out", None, arg)


def run_case(env, family, what, specs, call, skews=(0, 1), untouched=None, seed=11):
    """The runs of one case.  ``call(arrays)`` makes the call(s) on ``{name: tensor}``, synchronises, and returns (launched kernels,
    {name: bytes of further results, compared like the output arrays}).  ``untouched``: {output name: mask over its first axis} --
    rows that must keep the bytes they started with, in every run.  Returns the failures as strings; the record is kept in env."""
    torch = env.torch
    cap = ga.capacity_for([(s.shape, s.dtype) for s in specs])
    rec = env.record.setdefault(family, dict(calls=set(), regions=0, band_bytes=0, damaged=0, runs=0))
    rec["calls"].add(what)
    bad, res = [], {}
    for kind, skew, fill in RUNS:
        if skew not in skews:
            continue
        a = ga.Arena(env.dev, seed, fill=fill, capacity=cap)
        for s in specs:
            a.carve(s.name, s.shape, s.dtype, s.role, 0 if s.arg in ga.ALIGN16 else skew, arg=s.arg)
            if s.init is not None:
                a.put(s.name, s.init)
        plain = kind == "plain"
        arrays = {s.name: (a.plain_copy(s.name) if plain else a.regions[s.name].view) for s in specs}
        torch.cuda.synchronize()
        launched, extra = call(arrays)
        torch.cuda.synchronize()
        tag = "%s: %s" % (what, "plain" if plain else "skew %d, %s" % (skew, fill))
        if plain:
            now = {s.name: ga.raw_bytes(arrays[s.name]) for s in specs}
            for s in specs:
                if s.role == "in" and not np.array_equal(now[s.name], a.initial_bytes(s.name)):
                    bad.append("%s: the input %s was written" % (tag, s.name))
        else:
            whole = a.snapshot()
            now = {s.name: a.bytes_of(s.name, whole) for s in specs}
            dmg = a.damaged()
            rec["regions"] += len(specs)
            rec["band_bytes"] += a.band_bytes()
            rec["damaged"] += len(dmg)
            if dmg:
                bad.append("%s: %s" % (tag, ga.describe(dmg)))
        outs = {s.name: now[s.name] for s in specs if s.role == "out"}
        for name, b in outs.items():   # (a call that stores nothing would pass everything below)
            if np.array_equal(b, a.initial_bytes(name)):
                bad.append("%s: the output %s was not written at all" % (tag, name))
        for name, mask in (untouched or {}).items():
            row = len(outs[name]) // len(mask)
            kept = outs[name].reshape(len(mask), row)[mask] == a.initial_bytes(name).reshape(len(mask), row)[mask]
            if not kept.all():
                bad.append("%s: %s: %d rows the call is to leave alone were written" % (tag, name, int((~kept.all(axis=1)).sum())))
        outs.update({"(%s)" % k: np.ascontiguousarray(v).reshape(-1).view(np.uint8) for k, v in extra.items()})
        res[(kind, skew, fill)] = (tag, outs, launched)
    ref_tag, ref, ref_launched = res[RUNS[0]]
    for key, (tag, outs, launched) in res.items():
        if key == RUNS[0]:
            continue
        rec["runs"] += 1
        if launched != ref_launched:
            bad.append("%s: launched %s, the plain run %s" % (tag, sorted(launched), sorted(ref_launched)))
        for name, b in outs.items():
            if not np.array_equal(b, ref[name]):
                d = np.flatnonzero(b != ref[name])
                bad.append("%s: %s differs from the plain run in %d bytes, offsets %d..%d of %d" % (tag, name, d.size, d[0], d[-1], b.size))
    for skew in skews:
        (ta, oa, _), (tb, ob, _) = res[("arena", skew, "nan")], res[("arena", skew, "huge")]
        rec["runs"] += 1
        for name in oa:
            if not np.array_equal(oa[name], ob[name]):
                d = np.flatnonzero(oa[name] != ob[name])
                bad.append("%s against huge: %s differs in %d bytes, offsets %d..%d: the result depends on bytes outside an input" % (
                    ta, name, d.size, d[0], d[-1]))
    return bad, ref_launched


# ---- a. the cycle kernels ---------------------------------------------------------------------------------------------------
def _cycle_specs(h, r, want, ctrl, limits, active=None):
    B, n, dt, eng = r.B, r.nj, r.t, h.eng
    specs = [_in("q", h.w["q"], dt)]
    if ctrl:
        specs.append(_in("null_control", h.ctrl, dt))
    if limits:
        specs += [_in("q_lo", h.q_lo, dt), _in("q_hi", h.q_hi, dt)]
    if active is not None:
        specs.append(_in("active", active, I32))
    outs = tuple(want) + (() if "status" in want else ("status",))
    for k in outs:
        shape, dtype = eng._out_specs[k]
        specs.append(_out(k, shape, dtype))
    if r.roll:
        specs.append(_out("q_out", (B, n), dt))
    return specs, outs


def _cycle_call(h, r, outs, cap):
    eng = h.eng

    def call(arr):
        eng.set_small_batch_kernel(cap)
        eng.reset_state()
        eng.launched_kernels()   # (clears the record)
        io = eng.make_io(arr["q"], null_control=arr.get("null_control"), active=arr.get("active"), q_lo=arr.get("q_lo"), q_hi=arr.get("q_hi"),
                         **{k: arr[k] for k in outs})
        if r.roll:
            eng.rollout(io, tv.ROLL_K, tv.ROLL_DT, q_out=arr["q_out"])
        else:
            eng.step(io)
        eng.sync()
        return eng.launched_kernels(), {}
    return call


@pytest.mark.parametrize("nj,io,ns", GROUPS, ids=["nj%d-f%d-%s" % (n, t, "ns" if ns else "plain") for n, t, ns in GROUPS])
def test_cycle_variants_stay_inside_the_callers_arrays(env, nj, io, ns):
    variants = env.variants.get((nj, io, ns), [])
    assert variants, "the library has no cycle kernel for %d joints, float%d I/O, nullspace %s" % (nj, io, ns)
    family = "cycle nj=%d float%d %s" % (nj, io, "ns" if ns else "plain")
    failures, handles, gated = [], {}, False
    try:
        for v in variants:
            for b_small in BATCHES:
                r = tv.Recipe(v, b_small=b_small)
                if r.big and b_small != BATCHES[0]:
                    continue             # (one big batch per two-waves variant)
                h = handles.get(r.key)
                if h is None:
                    h = handles[r.key] = tv.Handle(env, r, seed=1000 + 17 * len(handles))
                specs, outs = _cycle_specs(h, r, r.want, r.ctrl, r.limits)
                bad, launched = run_case(env, family, "%s %s B=%d" % ("vfik_rollout" if r.roll else "vfik_step", v.name, r.B), specs,
                                         _cycle_call(h, r, outs, r.cap),
                                         skews=(0,) if r.big else (0, 1))
                if v.name not in launched:
                    bad.append("%s B=%d: not launched by %r, which took %s" % (v.name, r.B, r, sorted(launched)))
                failures += bad
                # one gated launch per group: a single cycle that publishes every row, every third arm silent
                if not gated and not r.big and not r.roll and b_small == BATCHES[0]:
                    gated = True
                    active = (np.arange(r.B) % 3 != 1).astype(I32)
                    gs, gouts = _cycle_specs(h, r, tv.ROWS, r.ns and r.nj <= 7, r.limits, active=active)
                    quiet = active == 0
                    bad, _ = run_case(env, family, "vfik_step gated, B=%d on the handle of %s" % (r.B, v.name), gs, _cycle_call(h, r, gouts, 0),
                                      untouched={k: quiet for k in gouts})
                    failures += bad
                if r.big:   # (a big handle serves one variant)
                    handles.pop(r.key).close()
    finally:
        for h in handles.values():
            h.close()
    assert gated, "no variant of the group gave a gated launch"
    print("%s: %d variants, %d failures" % (family, len(variants), len(failures)))
    assert not failures, "%d failures:\n" % len(failures) + "\n".join(failures)


# ---- b. the aux kernels -------------------------------------------------------------------------------------------------------
AUX = [(B, io) for B in AUX_B for io in (32, 64)]
AUX_IDS = ["B%d-f%d" % c for c in AUX]
SPHERES = [(4, (0.01, -0.02, 0.03), 0.06), (6, (-0.02, 0.01, 0.0), 0.05), (7, (0.0, 0.02, -0.01), 0.07)]


def _dt(io):
    return np.float32 if io == 32 else np.float64


def _aux_engine(env, B, io, flags=0, mix_w=None, max_slots=8, nobs=3, seed=5):
    chain = env.robots.lwr()
    dt = _dt(io)
    w = env.synth.make_workload(chain, B, nobs, seed=seed, io_dtype=dt)
    kw = {} if mix_w is None else dict(mix_w=mix_w)
    eng = env.engine.Engine(chain, B, io_dtype=dt, max_slots=max_slots, params=env.abi.default_params(flags=flags, **kw))
    eng.set_fields(w["fields"], w["nfields"])
    return chain, dt, w, eng


def _points(chain, rng, B, n_rep, q):
    """spheres around every arm's own flange: some near, some far, one row NaN"""
    tip = chain.fk(q).reshape(B, 4, 4)[:, :3, 3]
    p = np.empty((B, n_rep, 4))
    p[:, :, :3] = tip[:, None, :] + rng.uniform(-0.25, 0.25, (B, n_rep, 3))
    p[:, :, 3] = rng.uniform(0.02, 0.08, (B, n_rep))
    p[:, n_rep // 2, 0] = np.nan
    return p


def _finish(env, family, bad):
    assert not bad, "%s, %d failures:\n" % (family, len(bad)) + "\n".join(bad)


@pytest.mark.parametrize("B,io", AUX, ids=AUX_IDS)
def test_link_points_extents(env, B, io):
    chain, dt, w, eng = _aux_engine(env, B, io)
    try:
        eng.set_link_spheres(SPHERES)
        L, first_rep, n_rep = len(SPHERES), 2, 7
        rng = np.random.default_rng(21)
        src = ((np.arange(B) + 1) % B).astype(I32)
        src[::9] = -1
        if B > 2:
            src[2] = B + 5            # a source outside the batch: NaN rows
        xform = np.tile(np.eye(3, 4).reshape(12), (B, 1)) + rng.uniform(-0.2, 0.2, (B, 12))
        specs = [_in("q", w["q"], dt), _in("src_arm", src, I32), _in("xform12", xform, dt), _out("out", (B, n_rep, 4), dt, arg="rep4")]

        def call(arr):
            eng.link_points(arr["q"], arr["src_arm"], arr["xform12"], out=arr["out"], first_rep=first_rep)
            eng.sync()
            return set(), {}
        # rows outside first_rep .. first_rep + L - 1 keep what they held: as a mask over the (B * n_rep) rows
        rows = np.tile((np.arange(n_rep) < first_rep) | (np.arange(n_rep) >= first_rep + L), B)
        bad, _ = run_case(env, "aux link_points", "vfik_link_points B=%d float%d first_rep=%d n_rep=%d L=%d" % (B, io, first_rep, n_rep, L),
                          specs, call, untouched={"out": rows})
    finally:
        eng.close()
    _finish(env, "link_points", bad)


@pytest.mark.parametrize("B,io", AUX, ids=AUX_IDS)
def test_link_clearance_extents(env, B, io):
    chain, dt, w, eng = _aux_engine(env, B, io)
    bad = []
    try:
        eng.set_link_spheres(SPHERES)
        n_rep = 33
        pts = _points(chain, np.random.default_rng(22), B, n_rep, w["q"])
        for count in (1, 5, 32):
            specs = [_in("q", w["q"], dt), _in("points", pts, dt, arg="pts4"), _out("out", (B,), dt), _out("pair", (B,), I32)]

            def call(arr):
                eng.link_clearance(arr["q"], arr["points"], first=1, count=count, out=arr["out"], pair=arr["pair"])
                eng.sync()
                return set(), {}
            bad += run_case(env, "aux link_clearance", "vfik_link_clearance B=%d float%d count=%d" % (B, io, count), specs, call)[0]
    finally:
        eng.close()
    _finish(env, "link_clearance", bad)


@pytest.mark.parametrize("B,io", AUX, ids=AUX_IDS)
def test_link_avoid_extents(env, B, io):
    abi = env.abi
    chain, dt, w, eng = _aux_engine(env, B, io, flags=abi.F_MIXER, mix_w=[1.0, 0.0, 0.0, 0.0, 1.0, 0.0])
    bad = []
    try:
        eng.set_link_spheres(SPHERES)
        n_rep = 9
        rng = np.random.default_rng(23)
        pts = _points(chain, rng, B, n_rep, w["q"])
        scale = rng.uniform(0.0, 2.0, B)
        ins = [_in("q", w["q"], dt), _in("points", pts, dt, arg="pts4"), _in("scale", scale, dt)]

        def call(arr):
            eng.link_avoid(arr["q"], arr["points"], first=1, count=8, gain=1.5, d0=0.3, scale=arr["scale"], out=arr["out"])
            eng.sync()
            return set(), {}
        bad += run_case(env, "aux link_avoid", "vfik_link_avoid B=%d float%d" % (B, io), ins + [_out("out", (B, chain.n), dt)], call)[0]
        # into mixer channel 4 of the handle's ext buffer, without an out: what the next cycle publishes is the result
        eng.set_ext_cmd(3, np.zeros((B, chain.n)))

        def call4(arr):
            eng._chk(eng.lib.vfik_link_avoid(eng.h, C.c_void_p(arr["q"].data_ptr()), C.c_void_p(arr["points"].data_ptr()), n_rep, 1, 8, None,
                                             1.5, 0.3, C.c_void_p(arr["scale"].data_ptr()), None, 4))
            eng.sync()
            eng.reset_state()
            eng.launched_kernels()
            got = eng.step_host(w["q"], want=("qdot_out",))
            return eng.launched_kernels(), got
        b4, _ = run_case(env, "aux link_avoid", "vfik_link_avoid channel=4 B=%d float%d" % (B, io), ins, call4)
        bad += b4
        cmd = eng.link_avoid_host(w["q"], pts, first=1, count=8, gain=1.5, d0=0.3, scale=scale)
        assert np.abs(cmd).max() > 1e-3, "no pair pushes: the channel case would compare zeros"
    finally:
        eng.close()
    _finish(env, "link_avoid", bad)


@pytest.mark.parametrize("B,io", AUX, ids=AUX_IDS)
def test_track_error_extents(env, B, io):
    chain, dt, w, eng = _aux_engine(env, B, io)
    try:
        rng = np.random.default_rng(24)
        pose = chain.fk(w["q"]).reshape(B, 16)
        v6 = rng.uniform(-0.2, 0.2, (B, 6))
        active = (np.arange(B) % 4 != 1).astype(I32)
        specs = [_in("pose", pose, dt), _in("v6", v6, dt), _in("active", active, I32), _out("out", (B, 8), dt)]

        def call(arr):
            eng.track_reset()
            for _ in range(6):       # the estimator publishes from its sixth frame on
                eng.track_error(arr["pose"], arr["v6"], arr["out"], arr["active"])
            eng.sync()
            return set(), {}
        bad, _ = run_case(env, "aux track_error", "vfik_track_error B=%d float%d" % (B, io), specs, call, untouched={"out": active == 0})
    finally:
        eng.close()
    _finish(env, "track_error", bad)


@pytest.mark.parametrize("B,io", AUX, ids=AUX_IDS)
def test_probe_field_extents(env, B, io):
    chain, dt, w, eng = _aux_engine(env, B, io)
    try:
        rng = np.random.default_rng(25)
        pose = chain.fk(rng.uniform(chain.q_lo, chain.q_hi, (B, chain.n))).reshape(B, 16)
        specs = [_in("pose", pose, dt), _out("v6", (B, 6), dt)]

        def call(arr):
            eng.probe_field(arr["pose"], arr["v6"])
            eng.sync()
            return set(), {}
        bad, _ = run_case(env, "aux probe_field", "vfik_probe_field B=%d float%d" % (B, io), specs, call)
    finally:
        eng.close()
    _finish(env, "probe_field", bad)


@pytest.mark.parametrize("B,io", AUX, ids=AUX_IDS)
def test_object_distances_extents(env, B, io):
    chain, dt, w, eng = _aux_engine(env, B, io)
    try:
        rng = np.random.default_rng(26)
        n_obj = 3
        pose = chain.fk(w["q"]).reshape(B, 16)
        frames = chain.fk(rng.uniform(chain.q_lo, chain.q_hi, (B * n_obj, chain.n))).reshape(B, n_obj, 16)
        specs = [_in("pose", pose, dt), _in("frames", frames, dt), _out("out", (B, n_obj, 2), dt)]

        def call(arr):
            eng.object_distances(arr["pose"], arr["frames"], n_obj, arr["out"])
            eng.sync()
            return set(), {}
        bad, _ = run_case(env, "aux object_distances", "vfik_object_distances B=%d float%d" % (B, io), specs, call)
    finally:
        eng.close()
    _finish(env, "object_distances", bad)


@pytest.mark.parametrize("B,io", AUX, ids=AUX_IDS)
def test_mix_extents(env, B, io):
    chain, dt, w, eng = _aux_engine(env, B, io)
    try:
        rng = np.random.default_rng(27)
        K = 5
        cmds = rng.uniform(-1, 1, (K, B, chain.n))
        weights = rng.uniform(0, 1, K)
        specs = [_in("cmds", cmds, dt), _out("out", (B, chain.n), dt)]

        def call(arr):
            eng.mix(arr["cmds"], weights, arr["out"])
            eng.sync()
            return set(), {}
        bad, _ = run_case(env, "aux mix", "vfik_mix B=%d float%d K=%d" % (B, io, K), specs, call)
    finally:
        eng.close()
    _finish(env, "mix", bad)


# the moves' own output is an image of the handle: the result is what a following publishing cycle gives
MOVES_B = 203
MOVE_RANGES = ((0, MOVES_B - 7), (5, 64 * 2 + 3), (64, 100))          # (first_arm, n_arms): every range ends short of the batch
PUBLISHED = ("qdot_vf", "qdot_out", "pose", "qdist", "status")


def _publish(eng, q):
    eng.reset_state()
    eng.launched_kernels()
    got = eng.step_host(q, want=PUBLISHED)
    return eng.launched_kernels(), got


@pytest.mark.parametrize("io", (32, 64), ids=("f32", "f64"))
def test_move_fields_extents(env, io):
    dt = _dt(io)
    chain = env.robots.lwr()
    B = MOVES_B
    w, max_slots, _path = ms._scene(env, chain, "path2", B, 4, dt, seed=31)
    eng = env.engine.Engine(chain, B, io_dtype=dt, max_slots=max_slots)
    bad = []
    try:
        for first, n in MOVE_RANGES:
            rows = ms._make_move(env, chain, w, dt, seed=32 + first, classes=("goal", "rep"), first=first, n=n, nan_frac=0.1)
            active = (np.arange(n) % 5 != 2).astype(I32)
            specs = [_in("goal16", rows["goal"], dt), _in("repellers", rows["rep"], dt, arg="rep4"), _in("active", active, I32)]

            def call(arr):
                eng.set_fields(w["fields"], w["nfields"])
                eng.move_fields(goal=arr["goal16"], repellers=arr["repellers"], active=arr["active"], first_arm=first)
                eng.sync()
                return _publish(eng, w["q"])
            bad += run_case(env, "aux move_fields", "vfik_move_fields float%d first_arm=%d n_arms=%d of %d" % (io, first, n, B), specs, call)[0]
            # (the move does change what is published: the comparison is not one of untouched images)
            moved = _publish(eng, w["q"])[1]
            eng.set_fields(w["fields"], w["nfields"])
            assert not np.array_equal(_publish(eng, w["q"])[1]["qdot_out"], moved["qdot_out"])
    finally:
        eng.close()
    _finish(env, "move_fields", bad)


@pytest.mark.parametrize("io", (32, 64), ids=("f32", "f64"))
def test_move_scene_extents(env, io):
    dt = _dt(io)
    chain = env.robots.lwr()
    B = MOVES_B
    w, max_slots, _path = ms._scene(env, chain, "path0", B, 3, dt, seed=33)
    eng = env.engine.Engine(chain, B, io_dtype=dt, max_slots=max_slots)
    bad = []
    try:
        for first, n in MOVE_RANGES:
            rows = ms._make_move(env, chain, w, dt, seed=34 + first, first=first, n=n, nan_frac=0.1)
            active = (np.arange(n) % 5 != 2).astype(I32)
            specs = [_in("goal16", rows["goal"], dt), _in("rep4", rows["rep"], dt), _in("fun6", rows["fun"], dt), _in("hem6", rows["hem"], dt),
                     _in("att16", rows["att"], dt), _in("active", active, I32)]

            def call(arr):
                eng.set_fields(w["fields"], w["nfields"])
                eng.move_scene(goal=arr["goal16"], repellers=arr["rep4"], funnels=arr["fun6"], hemispheres=arr["hem6"], attractors=arr["att16"],
                               active=arr["active"], first_arm=first)
                eng.sync()
                return _publish(eng, w["q"])
            bad += run_case(env, "aux move_scene", "vfik_move_scene float%d first_arm=%d n_arms=%d of %d" % (io, first, n, B), specs, call)[0]
            moved = _publish(eng, w["q"])[1]
            eng.set_fields(w["fields"], w["nfields"])
            assert not np.array_equal(_publish(eng, w["q"])[1]["qdot_out"], moved["qdot_out"])
    finally:
        eng.close()
    _finish(env, "move_scene", bad)


# ---- c. the timed moves -------------------------------------------------------------------------------------------------------
MOVES = ("goto", "follow", "goto_js", "follow_js", "script")
MIX_CART, MIX_JOINT = (1.0, 1.0, 0.0, 0.0, 1.0, 0.0), (0.0, 0.0, 1.0, 0.0, 1.0, 0.0)
PREC = cr.PREC


def _move_case(env, io, seed=7):
    """coupled_reference.pair_case on the LWR: goals, starts, frames on the way (W = 3), the partner's spheres; postures and a script."""
    dt = _dt(io)
    chain = env.robots.lwr()
    B, n = MOVE_B, chain.n
    c = cr.pair_case(chain, B, dt, seed=seed, n_way=MOVE_W)
    rng = np.random.default_rng(seed + 1)
    off = rng.uniform(-0.05, 0.05, (B, n))
    wayq = np.stack([np.clip(c["q0"] + (i + 1) / MOVE_W * off, chain.q_lo, chain.q_hi) for i in range(MOVE_W)], axis=1)
    wayq[5, 2:, 0] = np.nan
    wayq[8, :, 0] = np.nan
    kind = np.tile(np.array([2, 1, 1], dtype=I32), (B, 1))
    kind[:, 0], kind[:, 1:] = env.abi.STEP_POSTURE, env.abi.STEP_FRAME
    kind[5, 1:], kind[6, 2:], kind[8, :] = 0, 0, 0
    active = (np.arange(B) % 11 != 3).astype(I32)
    c.update(chain=chain, dt=dt, wayq=wayq, kind=kind, way_s=np.nan_to_num(c["way"]), wayq_s=np.nan_to_num(wayq), q_ref=wayq[:, 0].copy(),
             active=active)
    c["q_ref"][8] = c["q0"][8]
    return c


def _move_specs(c, move, stride, rules=False):
    B, n, dt, W = MOVE_B, c["chain"].n, c["dt"], MOVE_W
    k = MOVE_CYCLES // stride
    L = len(c["spheres"])
    specs = [_in("q", c["q0"], dt), _in("active", c["active"], I32), _out("qdot_out", (B, n), dt), _out("status", (B,), I32),
             _out("pending", (k,), I32), _out("q_out", (B, n), dt), _out("q_traj", (k, B, n), dt)]
    if move in ("goto", "goto_js"):
        specs.append(_out("arrived", (B,), I32))
    else:
        specs += [_out("reached", (B, W), I32), _out("next", (B,), I32), _out("way_traj", (k, B), I32)]
    if move in ("goto", "follow", "script"):
        specs.append(_out("dist_traj", (k, B, 2), dt))
    if move in ("goto_js", "follow_js", "script"):
        specs.append(_out("diff", (B, n), dt))
    if move == "goto_js":
        specs.append(_in("q_ref", c["q_ref"], dt))
    if move == "follow":
        specs.append(_in("way16", c["way"].reshape(B, W, 16), dt))
    if move == "follow_js":
        specs.append(_in("wayq", c["wayq"], dt))
    if move == "script":
        specs += [_in("kind", c["kind"], I32), _in("way16", c["way_s"].reshape(B, W, 16), dt), _in("wayq", c["wayq_s"], dt)]
    if rules:
        yields = (np.arange(B) % 2).astype(I32)
        scale = np.where(np.arange(B) % 5 == 0, 0.0, 1.0)
        specs += [_out("stalled", (B,), I32), _in("src_arm", c["src_arm"], I32), _in("xform", c["xform"], dt),
                  _out("link_traj", (k, B, L, 4), dt), _in("yields", yields, I32), _out("clear_traj", (k, B), dt),
                  _out("pair_traj", (k, B), I32), _out("waited", (B,), I32), _in("scale", scale, dt), _out("avoid_traj", (k, B, n), dt)]
    return specs


def _move_call(env, eng, c, move, stride, rules=False):
    n = c["chain"].n
    js, via = np.full(n, 0.02), np.full(n, 0.06)

    def call(arr):
        eng.set_fields(c["w"]["fields"], c["w"]["nfields"])
        eng.set_params(mix_w=MIX_JOINT if move in ("goto_js", "follow_js") else MIX_CART)
        if rules:
            eng.set_link_spheres(c["spheres"])
            eng.set_coupling(src_arm=arr["src_arm"], xform=arr["xform"], first_rep=c["first_rep"], link_traj=arr["link_traj"])
            eng.set_wait_rule(0.12, yields=arr["yields"], clear_traj=arr["clear_traj"], pair_traj=arr["pair_traj"], waited=arr["waited"])
            eng.set_avoid_rule(1.0, 0.10, channel=4, scale=arr["scale"], avoid_traj=arr["avoid_traj"])
            eng.set_stall_rule(2, eps=(2.5e-4, 2.5e-3), eps_js=2.5e-4, stop=True, stalled=arr["stalled"])
        eng.reset_state()
        eng.launched_kernels()
        io = eng.make_io(arr["q"], q_ref=arr.get("q_ref"), active=arr["active"], qdot_out=arr["qdot_out"], status=arr["status"])
        kw = dict(stride=stride, hold=True, clamp=True, pending=arr["pending"], q_out=arr["q_out"], q_traj=arr["q_traj"])
        for k in ("arrived", "reached", "next", "way_traj", "dist_traj", "diff"):
            if k in arr:
                kw[k] = arr[k]
        if move == "goto":
            eng.goto(io, MOVE_CYCLES, MOVE_DT, PREC, **kw)
        elif move == "follow":
            eng.follow(io, arr["way16"], MOVE_CYCLES, MOVE_DT, PREC, **kw)
        elif move == "goto_js":
            eng.goto_js(io, MOVE_CYCLES, MOVE_DT, js, **kw)
        elif move == "follow_js":
            eng.follow_js(io, arr["wayq"], MOVE_CYCLES, MOVE_DT, js, via_precision=via, **kw)
        else:
            eng.script(io, arr["kind"], arr["way16"], arr["wayq"], MOVE_CYCLES, MOVE_DT, PREC, js, js_via_precision=via, **kw)
        eng.sync()
        launched = eng.launched_kernels()
        if rules:   # the handle lets go of the run's arrays before they are
            eng.set_stall_rule(None)
            eng.set_coupling(None)
        return launched, {}
    return call


def _moves_engine(env, c):
    abi = env.abi
    params = abi.default_params(flags=abi.F_NULLSPACE | abi.F_MIXER, max_vel=0.7, mix_w=MIX_CART, jp_kp=8.0)
    return env.engine.Engine(c["chain"], MOVE_B, io_dtype=c["dt"], max_slots=8, params=params)


MOVE_CASES = [(io, stride) for io in (32, 64) for stride in (1, 4)]


@pytest.mark.parametrize("io,stride", MOVE_CASES, ids=["f%d-stride%d" % c for c in MOVE_CASES])
def test_timed_moves_stay_inside_the_callers_arrays(env, io, stride):
    c = _move_case(env, io)
    eng = _moves_engine(env, c)
    bad = []
    try:
        for move in MOVES:
            b, launched = run_case(env, "moves", "vfik_%s float%d stride=%d" % (move, io, stride), _move_specs(c, move, stride),
                                   _move_call(env, eng, c, move, stride))
            assert launched, "vfik_%s launched no cycle kernel" % move
            bad += b
    finally:
        eng.close()
    _finish(env, "timed moves", bad)


@pytest.mark.parametrize("io,stride", [(32, 4), (64, 1)], ids=["f32-stride4", "f64-stride1"])
def test_timed_moves_with_every_rule_stay_inside_the_callers_arrays(env, io, stride):
    c = _move_case(env, io)
    eng = _moves_engine(env, c)
    bad = []
    try:
        for move in MOVES:
            b, launched = run_case(env, "moves, every rule on", "vfik_%s float%d stride=%d with vfik_set_coupling, vfik_set_wait_rule, "
                                   "vfik_set_avoid_rule, vfik_set_stall_rule" % (move, io, stride), _move_specs(c, move, stride, rules=True),
                                   _move_call(env, eng, c, move, stride, rules=True))
            assert launched, "vfik_%s launched no cycle kernel" % move
            bad += b
    finally:
        eng.close()
    _finish(env, "timed moves under every rule", bad)
