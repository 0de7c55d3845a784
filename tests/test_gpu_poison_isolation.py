"""Per-arm isolation and recovery of every cycle kernel under non-finite inputs: the contract of include/vfik.h (C1, C2, C3) on the GPU.

test_every_built_variant_isolates_a_poisoned_q: EVERY cycle-kernel instantiation of the built library (tests/kernel_variants.py), under
the recipe of tests/test_gpu_variants.py that makes a launch take it.  Per variant, on one handle: the recipe's launch and a second, clean
cycle behind it with no reset in between -- once with clean inputs, once with q spoiled on the arms P (poison_reference.arms: first and
last lane of a wave, the lane next to a wave's end, the last arm of a partial wave; the four q kinds dealt out over them).  A recipe that
rolls out runs with the clamp off and on.  Asserted: both launches of both runs took the variant;

  C1  every row the recipe asks for, of every arm outside P, is the same BITS in the two runs -- in the poisoned launch and in the clean
      cycle behind it, which reads the per-arm device state (no oracle needed: the neighbours' numbers are tests/test_gpu_variants.py's job);
  C2  on P, against the C oracle stepped on the host with the same spoiled q (np.clip where the run clamps): wherever the oracle's element
      of a command row (qdot_vf, qdot_null, qdot_out) or of the integrated q is not finite the kernel's is not finite; where both are finite
      they agree within the suite's bars (tests/test_gpu_variants.py: 1e-6 / 1e-9 by I/O type, a rollout's q 2e-5 / 1e-9; the rows of a
      rollout's last cycle: tests/test_gpu_rollout.py's 2e-5 / 1e-7); VFIK_ST_NAN is set
      exactly where the oracle sets it; pose, pose_nt and qdist are compared where both sides are finite;
  C3  the clean cycle behind it equals the oracle's, which went through the same two cycles with its own state: every row, and the status.

test_poison_kinds_by_family: the other kinds (poison_reference.KINDS: /control, the joint reference, per-arm limits, an external command,
goal and repeller rows sent through vfik_move_fields_host) on one variant per family at both I/O types, the same three assertions; the
kinds the specification swallows (poison_reference.SWALLOWED) must come out finite and equal to the oracle, ST_NAN clear.  What the GPU
tests take for granted of the oracle's side is asserted on the CPU, on these very inputs: tests/test_poison_reference.py.

With VFIK_POISON_TABLE=<file> the worst finite error on P per group / family and kind is also written there (profiles/poison_isolation.txt)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_variants as kv  # noqa: E402,F401
import poison_reference as pr  # noqa: E402
import test_gpu_variants as tv  # noqa: E402

pytestmark = pytest.mark.gpu

GROUPS = tv.GROUPS
ROLL_K, ROLL_DT = tv.ROLL_K, tv.ROLL_DT


@pytest.fixture(scope="module")
def env():
    import __graft_entry__ as g
    g.build()
    from oracle import oracle_c
    from vfclik_amd import _abi, chain, engine, robots, synth

    class E:
        pass

    e = E()
    e.oc, e.abi, e.chain, e.engine, e.robots, e.synth = oracle_c, _abi, chain, engine, robots, synth
    e.variants = kv.by_group()
    e.table = []
    yield e
    path = os.environ.get("VFIK_POISON_TABLE")
    if path and e.table:
        with open(path, "a") as f:
            f.write("\n".join(e.table) + "\n")


def _tol(r, key):
    """the suite's bars: tests/test_gpu_variants.py's for a cycle's rows and for a rollout's q, tests/test_gpu_rollout.py's for the rows of a
    rollout's last cycle (the oracle is stepped with q rounded to a float32 I/O type every cycle, the kernel integrates in float64)"""
    if key == "q":
        return 2e-5 if r.t == np.float32 else 1e-9
    if r.roll:
        return 2e-5 if r.t == np.float32 else 1e-7
    return 1e-6 if r.t == np.float32 else 1e-9


def _rows(r):
    return tuple(r.want) + (("q",) if r.roll else ())


def _outside(B, P):
    m = np.ones(B, dtype=bool)
    m[P] = False
    return m


def _c1(a, a0, keys, out, what):
    """rows outside P, bit for bit"""
    return ["%s: C1 %s of %d arms outside P differs from the clean run" % (what, k, int(np.any((a[k][out] != a0[k][out]).reshape(out.sum(), -1), axis=1).sum()))
            for k in keys if not pr.same_bits(a[k][out], a0[k][out])]


def _c2(got, ref, keys, r, P, what, worst):
    bad = []
    for k in keys:
        g = np.asarray(got[k])[P]
        if k == "status":
            if not np.array_equal(pr.nan_bit(g), pr.nan_bit(ref[k])):
                bad.append("%s: C2 ST_NAN on P is %s, the oracle's %s" % (what, pr.nan_bit(g).astype(int), pr.nan_bit(ref[k]).astype(int)))
            continue
        tol = _tol(r, k)
        if k in pr.SOFT_ROWS:
            n, e = pr.soft_differences(g, ref[k], tol)
            if n:
                bad.append("%s: C2 %s differs where both are finite: %d elements, worst %.3e" % (what, k, n, e))
        else:
            laund, n, e = pr.laundered(g, ref[k], tol)
            if laund:
                bad.append("%s: C2 %s is finite in %d elements where the oracle's is not" % (what, k, laund))
            if n:
                bad.append("%s: C2 %s differs where both are finite: %d elements, worst %.3e (bar %.0e)" % (what, k, n, e, tol))
        worst[k] = max(worst.get(k, 0.0), e)
    return bad


def _c3(got, ref, keys, r, P, what, worst):
    bad = []
    for k in keys:
        g = np.asarray(got[k])[P]
        if k == "status":
            if not np.array_equal(g, ref[k]):
                bad.append("%s: C3 status on P is %s, the oracle's %s" % (what, g, ref[k]))
            continue
        if not np.isfinite(ref[k]).all():
            bad.append("%s: C3 the oracle's own %s is not finite" % (what, k))
            continue
        n, e = pr.unrecovered(g, ref[k], _tol(r, k))
        if n:
            bad.append("%s: C3 %s of %d arms of P has not recovered (worst %.3e, bar %.0e)" % (what, k, n, e, _tol(r, k)))
        worst[k] = max(worst.get(k, 0.0), e if np.isfinite(e) else 0.0)
    return bad


# ---- every variant, q spoiled -----------------------------------------------------------------------------------------------------------
def _launch(h, r, q, clamp):
    lim = dict(q_lo=h.q_lo, q_hi=h.q_hi) if r.limits else {}
    if r.roll:
        return h.eng.rollout_host(q, ROLL_K, ROLL_DT, clamp=clamp, want=r.want, **lim)
    return h.eng.step_host(q, null_control=h.ctrl if r.ctrl else None, want=r.want, **lim)


def _two_launches(h, r, q1, q2, clamp):
    eng = h.eng
    eng.set_small_batch_kernel(r.cap)
    eng.reset_state()
    eng.launched_kernels()   # (clears the record)
    a = _launch(h, r, q1, clamp)
    la = eng.launched_kernels()
    b = _launch(h, r, q2, clamp)
    return a, b, la, eng.launched_kernels()


def _oracle_two(env, h, r, q1, q2, P, clamp):
    st = env.oc.new_states(len(P), r.nj) if r.ns else None
    F, nf = h.w["fields"], h.w["nfields"]
    out = []
    for q in (q1, q2):
        if r.roll:
            qe, last = pr.oracle_rollout(env.oc, h.chain, h.params, F, nf, h.tool, q, P, r.t, ROLL_K, ROLL_DT, clamp, states=st)
            ref = {k: last[k] for k in last if k != "states"}
            ref["q"] = qe
        else:
            x = pr.Inputs(q, null_control=h.ctrl if r.ctrl else None, q_lo=h.q_lo if r.limits else None, q_hi=h.q_hi if r.limits else None)
            ref = pr.oracle_cycle(env.oc, h.chain, h.params, F, nf, h.tool, x, P, r.t, states=st)
            ref = {k: np.array(v, copy=True) for k, v in ref.items() if k != "states"}
        out.append(ref)
    return out


def _variant(env, h, r, worst):
    """the differences of one variant, as strings"""
    family = "two-waves" if r.big else "eight-lanes" if r.cap else None
    P = pr.arms(r.B, family)
    out = _outside(r.B, P)
    q1, q2 = h.w["q"], h.q2
    qp = pr.mixed_q(q1, P)
    keys = _rows(r)
    bad = []
    for clamp in ((False, True) if r.roll else (False,)):
        what = "clamp %s" % ("on" if clamp else "off") if r.roll else "cycle"
        a0, b0, la0, lb0 = _two_launches(h, r, q1, q2, clamp)
        a, b, la, lb = _two_launches(h, r, qp, q2, clamp)
        for launched in (la0, lb0, la, lb):
            if r.v.name not in launched:
                return ["not launched by %r, which took %s" % (r, sorted(launched))]
        bad += _c1(a, a0, keys, out, what + ", poisoned launch") + _c1(b, b0, keys, out, what + ", the clean cycle behind it")
        ref_a, ref_b = _oracle_two(env, h, r, qp, q2, P, clamp)
        bad += _c2(a, ref_a, keys, r, P, what, worst)
        bad += _c3(b, ref_b, keys, r, P, what, worst)
    return bad


@pytest.mark.parametrize("nj,io,ns", GROUPS, ids=["nj%d-f%d-%s" % (n, t, "ns" if ns else "plain") for n, t, ns in GROUPS])
def test_every_built_variant_isolates_a_poisoned_q(env, nj, io, ns):
    variants = env.variants.get((nj, io, ns), [])
    assert variants, "the library has no cycle kernel for %d joints, float%d I/O, nullspace %s" % (nj, io, ns)
    failures, handles, ok, worst, rolled = [], {}, 0, {}, 0
    try:
        for v in variants:
            r = tv.Recipe(v)
            h = handles.get(r.key)
            if h is None:
                h = handles[r.key] = tv.Handle(env, r, seed=pr.SEED + 17 * len(handles))
            bad = _variant(env, h, r, worst)
            rolled += r.roll
            if bad:
                failures.append("%s: %s" % (v.name, "; ".join(bad)))
            else:
                ok += 1
            if r.big:   # (a big handle serves one variant)
                handles.pop(r.key).close()
    finally:
        for h in handles.values():
            h.close()
    line = "variants nj=%d float%d %s: %d of %d isolate a poisoned q (%d rollouts, clamp off and on); worst finite error on P: %s" % (
        nj, io, "ns" if ns else "plain", ok, len(variants), rolled, ", ".join("%s %.2e" % kv_ for kv_ in sorted(worst.items())))
    print(line)
    env.table.append(line)
    assert not failures, "%d of %d variants:\n" % (len(failures), len(variants)) + "\n".join(failures)


# ---- the other kinds, one variant per family --------------------------------------------------------------------------------------------
def _family_cycle(h, r, x):
    """the setters and the launch of one cycle's inputs"""
    eng = h.eng
    if x.ext is not None:
        eng.set_ext_cmd(pr.EXT_CHANNEL, x.ext)
    eng.move_fields_host(goal=x.goal, repellers=x.rep)
    eng.launched_kernels()
    got = eng.step_host(x.q, null_control=x.null_control, q_ref=x.q_ref, q_lo=x.q_lo, q_hi=x.q_hi, want=r.want)
    return got, eng.launched_kernels()


def _family_run(h, r, first, second):
    h.eng.set_small_batch_kernel(r.cap)
    h.eng.reset_state()
    a, la = _family_cycle(h, r, first)
    b, lb = _family_cycle(h, r, second)
    return a, b, la, lb


CASES = [(f, io) for f in pr.FAMILIES for io in (32, 64) if (f, io) not in pr.NOT_BUILT]


@pytest.mark.parametrize("family,io", CASES, ids=["%s-f%d" % c for c in CASES])
def test_poison_kinds_by_family(env, family, io):
    r = pr.pick(env.variants, family, io)
    h = tv.Handle(env, r, seed=pr.SEED)
    failures = []
    try:
        pr.family_setup(h, family)
        P = pr.arms(r.B, family)
        out = _outside(r.B, P)
        clean, nxt = pr.family_inputs(h, r, family), pr.family_inputs(h, r, family, second=True)
        keys = tuple(r.want)
        F, nf = h.w["fields"], h.w["nfields"]
        a0, b0, la0, lb0 = _family_run(h, r, clean, nxt)
        assert r.v.name in la0 and r.v.name in lb0, "%s: not launched by %r, which took %s" % (r.v.name, r, sorted(la0 | lb0))
        for kind in pr.kinds_of(family, r):
            worst = {}
            x = pr.poison(kind, clean, P)
            a, b, la, lb = _family_run(h, r, x, nxt)
            bad = []
            if la != la0 or lb != lb0:
                bad.append("launched %s and %s, the clean run %s and %s" % (sorted(la), sorted(lb), sorted(la0), sorted(lb0)))
            bad += _c1(a, a0, keys, out, "poisoned launch") + _c1(b, b0, keys, out, "the clean cycle behind it")
            st = env.oc.new_states(len(P), r.nj) if r.ns else None
            ref_a = pr.oracle_cycle(env.oc, h.chain, h.params, F, nf, h.tool, x, P, r.t, states=st)
            ref_a = {k: np.array(v, copy=True) for k, v in ref_a.items() if k != "states"}
            ref_b = pr.oracle_cycle(env.oc, h.chain, h.params, F, nf, h.tool, nxt, P, r.t, states=st)
            bad += _c2(a, ref_a, keys, r, P, "poisoned launch", worst)
            if kind in pr.SWALLOWED:   # the specification swallows it: finite, and the oracle's numbers
                bad += _c3(a, ref_a, tuple(k for k in keys if k != "status"), r, P, "poisoned launch (swallowed)", worst)
            bad += _c3(b, ref_b, keys, r, P, "the clean cycle behind it", worst)
            if bad:
                failures.append("%s: %s" % (kind, "; ".join(bad)))
            env.table.append("family %-11s float%d %-17s worst finite error on P: %s" % (
                family, io, kind, ", ".join("%s %.2e" % kv_ for kv_ in sorted(worst.items()))))
    finally:
        h.close()
    print("%s float%d: %s, %d kinds" % (family, io, r.v.name, len(pr.kinds_of(family, r))))
    assert not failures, "%s (%s), %d kinds:\n" % (family, r.v.name, len(failures)) + "\n".join(failures)


# ---- the observers of the cycle call ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("io", (32, 64), ids=("f32", "f64"))
def test_observers_keep_a_poisoned_cycle_inside_its_arm(env, io):
    """io.track_error and io.obj_dist over 8 cycles of one handle, q spoiled on P in cycle 2 alone.  The neighbours' rows are the clean run's
    bits in every cycle.  P's own rows: obj_dist has no memory -- every cycle but the poisoned one is the clean run's bits, and in the poisoned one the rows are held
    to tests/hp_observers.py's exact monitor reference on the published pose (not finite where it is not) --; track_error keeps
    5 frames and 4 commands, and the cycles in which an input of cycle 2 can show are taken from tests/hp_observers.py's exact reference
    (poison_reference.observer_memory: the command of three calls ago, cycle 5, alone -- rows are zeros until the sixth frame): in every
    other cycle P's rows are the clean run's bits, in those they are held to that reference on the published pose and v6 rows."""
    import hp_observers as ho
    from vfclik_amd import robots
    dt = np.float32 if io == 32 else np.float64
    chain = robots.lwr()
    B, T, O = tv.B_SMALL, pr.OBS_CYCLES, 2
    P = pr.arms(B)
    out = _outside(B, P)
    memory = pr.observer_memory()
    assert memory and min(memory) > pr.OBS_POISONED and max(memory) < T - 1, memory
    w = env.synth.make_workload(chain, B, 2, seed=47, io_dtype=dt)
    rng = np.random.default_rng(48)
    frames = chain.fk(rng.uniform(0.7 * chain.q_lo, 0.7 * chain.q_hi, (B * O, chain.n))).reshape(B, O, 16)
    step = rng.normal(0, 0.004, (B, chain.n))
    qs = [(w["q"] + t * step).astype(dt).astype(np.float64) for t in range(T)]
    want = ("qdot_out", "pose", "v6", "track_error", "obj_dist", "status")

    def run(poisoned):
        eng = env.engine.Engine(chain, B, io_dtype=dt, max_slots=4, params=env.abi.default_params(flags=env.abi.F_NULLSPACE | env.abi.F_MIXER))
        try:
            eng.set_fields(w["fields"], w["nfields"])
            eng.set_objects(frames)
            rows = []
            for t in range(T):
                q = pr.mixed_q(qs[t], P) if (poisoned and t == pr.OBS_POISONED) else qs[t]
                rows.append(eng.step_host(q, want=want))
            return rows
        finally:
            eng.close()
    clean, pois = run(False), run(True)
    bad = []
    for t in range(T):
        for k in want:
            if not pr.same_bits(pois[t][k][out], clean[t][k][out]):
                bad.append("cycle %d: %s differs outside P" % (t, k))
        if t != pr.OBS_POISONED and not pr.same_bits(pois[t]["obj_dist"][P], clean[t]["obj_dist"][P]):
            bad.append("cycle %d: obj_dist of P differs from the clean run" % t)
        if t not in memory and t != pr.OBS_POISONED and not pr.same_bits(pois[t]["track_error"][P], clean[t]["track_error"][P]):
            bad.append("cycle %d: track_error of P differs from the clean run, the reference's memory is %s" % (t, memory))
    assert pr.nan_bit(pois[pr.OBS_POISONED]["status"][P]).all() and not np.isfinite(pois[pr.OBS_POISONED]["pose"][P]).all(axis=1).any()
    assert any((clean[t]["track_error"][P] != 0).any() for t in memory)        # (the estimator does have values by then)
    # the cycles the poison can show in: the exact reference on the published rows of P
    poses = np.stack([pois[t]["pose"][P].astype(np.float64) for t in range(T)])
    v6 = np.stack([pois[t]["v6"][P].astype(np.float64) for t in range(T)])
    got = np.stack([pois[t]["track_error"][P].astype(np.float64) for t in range(T)])
    assert all(np.isfinite(poses[t]).all() and np.isfinite(v6[t]).all() for t in range(T) if t != pr.OBS_POISONED)
    act = np.ones((T, len(P)), dtype=np.int32)
    ref = ho.track_reference(("poison", io), poses, v6, act)
    # The published twist of the poisoned cycle is not finite (0 * NaN in the field's sum, as the oracle's), so the command history holds a NaN
    # until that command has been used: the reference's row of such a cycle has NaN elements of its own.  C2, element by element: where the
    # reference is not finite the kernel is not finite; where both are finite they agree within the reference's bar (K_MARGIN units, a float32
    # row the half ulp of its store); the decision (element 7) is the reference's wherever the kernel's row is finite.
    worst = 0.0
    for t in memory:
        r7 = ref["out"][t, :, :7] + ref["out_lo"][t, :, :7]
        g7 = got[t, :, :7]
        assert ref["valid"][t].all() and (~np.isfinite(r7)).any(), "the reference's row of cycle %d does not show the poison" % t
        laund = ~np.isfinite(r7) & np.isfinite(g7)
        both = np.isfinite(r7) & np.isfinite(g7)
        err = np.where(both, np.abs((g7 - ref["out"][t, :, :7]) - ref["out_lo"][t, :, :7]), 0.0)
        if io == 32:
            err = np.maximum(0.0, err - np.where(both, 0.5 * np.spacing(np.abs(np.where(both, r7, 0.0)).astype(np.float32)).astype(np.float64), 0.0))
        with np.errstate(invalid="ignore", divide="ignore"):
            ratio = np.where(both & ~ref["finite_only"][t, :, :7] & (err > 0), err / (ho.K_MARGIN * ref["unit"][t, :, :7]), 0.0)
        ratio = np.where(np.isnan(ratio), np.inf, ratio)
        worst = max(worst, float(ratio.max()))
        with np.errstate(invalid="ignore"):
            ambiguous = np.abs(r7[:, 6] - ho.TRACK_TH) <= ho.K_MARGIN * ref["unit"][t, :, 6] + (0.5 * np.spacing(np.float32(ho.TRACK_TH)) if io == 32 else 0.0)
        decided = np.isfinite(got[t, :, 7]) & np.isfinite(g7[:, 6]) & ~ambiguous
        wrong = decided & (got[t, :, 7] != ref["out"][t, :, 7])
        if laund.any() or not (ratio.max() <= 1.0) or wrong.any():
            bad.append("cycle %d: track_error of P against the exact reference: finite in %d elements where the reference is not, worst error / bar %.3f, "
                       "%d wrong decisions" % (t, int(laund.sum()), ratio.max(), int(wrong.sum())))
    # obj_dist of P in the poisoned cycle: the exact monitor reference on the published pose of that cycle (a pose that is not finite has
    # no distance and no angle).  C2: where the reference is not finite the kernel is not finite; elsewhere within the reference's bar.
    mon = pois[pr.OBS_POISONED]["obj_dist"][P].astype(np.float64)
    mref = ho.reference(("poison-monitor", io), pois[pr.OBS_POISONED]["pose"][P].astype(np.float64), frames[P].astype(dt).astype(np.float64))
    assert (~np.isfinite(mref["D"])).any() and (~np.isfinite(mref["ang"])).any()
    for i, nm in enumerate(("D", "ang")):
        r = mref[nm] + mref[nm + "_lo"]
        g = mon[:, :, i]
        laund = ~np.isfinite(r) & np.isfinite(g)
        both = np.isfinite(r) & np.isfinite(g)
        err = np.where(both, np.abs((g - mref[nm]) - mref[nm + "_lo"]), 0.0)
        if io == 32:
            err = np.maximum(0.0, err - np.where(both, 0.5 * np.spacing(np.abs(np.where(both, r, 0.0)).astype(np.float32)).astype(np.float64), 0.0))
        with np.errstate(invalid="ignore", divide="ignore"):
            over = np.where(both & (err > 0), err / (ho.K_MARGIN * mref["unit_" + nm]), 0.0)
        over = np.where(np.isnan(over), np.inf, over)
        if laund.any() or not over.max() <= 1.0:
            bad.append("cycle %d: obj_dist %s of P against the exact reference: finite in %d elements where the reference is not, worst error / bar %.3f" % (
                pr.OBS_POISONED, nm, int(laund.sum()), over.max()))
    env.table.append("observers float%d: poison in cycle %d shows in track_error in cycle(s) %s alone (the reference's memory); worst error / bar there %.3f" % (
        io, pr.OBS_POISONED, memory, worst))
    assert not bad, "\n".join(bad)
