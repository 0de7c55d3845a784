"""The HIP kernels' bridge back end -- joint P controller as mixer channel 2, mixer, limiter, LWR command form, q_ref_out -- held to the CPython
restatement on the tie scenes of tests/backend_ties.py (the bars are derived there): every status bit and decision exact; at float64 I/O
everything but a limited row bit for bit, limited rows within 4 ulp; at float32 I/O the reference rounded to float32, with the counted allowance
on limited rows.  tests/test_oracle_backend_ties.py asserts the scenes' own conditions and holds the C oracle to the same reference.

The launches carry per-arm mixer weights (and limiter speeds), so they take the general single-cycle variants, which read those rows through the
staged LDS layout: every chain of ROBOTS x both I/O types x with and without the nullspace module, asserted by kernel name."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import backend_ties as bt  # noqa: E402
import kernel_variants as kv  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = [(r, t, ns) for r in bt.ROBOTS for t in (np.float32, np.float64) for ns in (False, True)]
IDS = ["%s-f%d-%s" % (r, 32 if t == np.float32 else 64, "ns" if ns else "plain") for r, t, ns in CASES]
SCENES = ("limiter", "joint", "joint_cycle", "form")


@pytest.fixture(scope="module")
def env():
    import __graft_entry__ as g
    g.build()
    from oracle import oracle_c
    from vfclik_amd import _abi, engine

    class E:
        pass

    e = E()
    e.oc, e.abi, e.engine = oracle_c, _abi, engine
    yield e
    path = os.environ.get("VFIK_BACKEND_TABLE")
    if path:
        bt.write_table(path)


def _flags(abi, s, ns, limiter=None):
    limiter = s.limiter if limiter is None else limiter
    return abi.F_MIXER | (abi.F_LIMITER if limiter else 0) | (abi.F_NULLSPACE if ns else 0)


def _engine(env, s, ns, **kw):
    params = env.abi.default_params(flags=_flags(env.abi, s, ns, kw.pop("limiter", None)), jp_kp=bt.JP_KP, jp_delta=bt.JP_DELTA, **kw)
    eng = env.engine.Engine(s.chain, s.B, io_dtype=s.dt, max_slots=4, device=0, params=params)
    eng.set_fields(s.w["fields"], s.w["nfields"])
    if s.mixw is not None:
        eng.set_mixer_weights(s.mixw)
    if s.max_vel is not None:
        eng.set_max_vel(s.max_vel)
    if s.ext is not None:
        for ch in range(4):
            eng.set_ext_cmd(2 + ch, s.ext[ch])
    return eng


def _io(s):
    kw = dict(q_ref=s.q_ref, q_cmded=s.q_cmded)
    if s.q_lo is not None:
        kw.update(q_lo=s.q_lo, q_hi=s.q_hi)
    return kw


def _general(launched, s, ns):
    """the launch took one kernel, a general single-cycle variant of the scene's joint count, I/O type and module"""
    assert len(launched) == 1, launched
    v = kv.parse(next(iter(launched)))
    a = v.args
    assert (a["NJ"], a["T"], a["NS"]) == (s.n, "float" if s.dt == np.float32 else "double", ns), v.name
    assert a["LEAN"] == 0 and not a["ROLL"] and v.heavy == (s.n >= 14), v.name
    return v.name


def _module_bits(env, s, ns):
    """ST_LIMIT_STOP / ST_NULL_AMBIGUOUS: the nullspace module's bits, which the back end does not touch -- the C oracle's"""
    if not ns:
        return np.zeros(s.B, dtype=np.int32)
    p = env.abi.default_params(flags=env.abi.F_NULLSPACE)
    kw = dict(q_lo=s.q_lo, q_hi=s.q_hi) if s.q_lo is not None else {}
    r = env.oc.cycle_batch(s.chain, p, s.q, s.w["fields"], s.w["nfields"], want=("status",), **kw)
    return r["status"] & (bt.ST_LIMIT_STOP | bt.ST_NULL_AMBIGUOUS)


def _hold(s, got, ref, what):
    """qdot_out by the module's bars; returns (worst over the bar, allowance rows)"""
    bad, worst, allow = bt.compare(got["qdot_out"], ref["qdot_out"], ref["limited"], s.dt)
    assert len(bad) == 0, "%s: qdot_out misses the bar on arms %s (kinds %s)" % (what, bad[:8], [s.kind_of(b) for b in bad[:8]])
    nlim = int(ref["limited"].sum())
    assert allow == 0 or allow < bt.ALLOWANCE_CAP * nlim, (what, allow, nlim)
    return worst, allow, nlim


@pytest.mark.parametrize("robot,dt,ns", CASES, ids=IDS)
def test_back_end_on_its_ties(env, robot, dt, ns):
    f32 = dt == np.float32
    for scene in SCENES:
        s = bt.make_scene(scene, robot, dt)
        what = "%s %s f%d %s" % (scene, robot, 32 if f32 else 64, "ns" if ns else "plain")
        eng = _engine(env, s, ns)
        try:
            eng.launched_kernels()
            want = ("qdot_vf", "qdot_null", "qdot_out", "status") + (("q_ref_out",) if s.q_ref is not None else ())
            got = eng.step_host(s.q, want=want, **_io(s))
            name = _general(eng.launched_kernels(), s, ns)
            # channels 0 and 1 carry weight 0 (a denormal in one kind): finite rows, so that their products are zeros
            assert np.isfinite(got["qdot_vf"]).all() and np.isfinite(got["qdot_null"]).all()
            ref = bt.restate(s)
            assert np.array_equal(got["status"], bt.status_bits(ref) | _module_bits(env, s, ns)), what
            worst, allow, nlim = _hold(s, got, ref, what)
            if s.q_ref is not None:
                kept = ref["q_ref_out"] if not f32 else ref["q_ref_out"].astype(np.float32).astype(np.float64)
                assert bt._same(got["q_ref_out"].astype(np.float64), kept).all(), what
            if scene == "joint" and robot == "lwr":
                # the stepped blocks of goto_js: a one-cycle rollout with q_ref keeps the same reference and reports the same status
                eng.reset_state()
                eng.launched_kernels()
                roll = eng.rollout_host(s.q, 1, 1e-3, want=("qdot_out", "status", "q_ref_out"), q_ref=s.q_ref)
                rolled = [kv.parse(k) for k in eng.launched_kernels()]
                assert len(rolled) == 1 and rolled[0].args["ROLL"] and rolled[0].args["NJ"] == 7 and rolled[0].args["NS"] == ns, rolled
                assert len(bt.compare(roll["qdot_out"], ref["qdot_out"], ref["limited"], dt)[0]) == 0, what
                assert np.array_equal(roll["status"], got["status"]), what
                assert bt._same(roll["q_ref_out"].astype(np.float64), got["q_ref_out"].astype(np.float64)).all(), what
            bt.note("gpu", what, name.split("<")[0] + (" heavy" if s.n >= 14 else ""), worst, allow, nlim)
        finally:
            eng.close()


@pytest.mark.parametrize("robot", ("powercube6", "lwr", "lwr_dual14"))
def test_limiter_on_the_mixed_command(env, robot):
    """Limiter, mixed input (float64 I/O): pass 1, limiter off, publishes qdot_vf, qdot_null and qdot_out, and the host mix of the published
    channels equals qdot_out bit for bit for EVERY arm; pass 2 limits every arm at the lead of its own pass-1 command, or one ulp to either
    side.  Both passes must take the same kernel, or the second pass's command would not be the first's."""
    dt, abi = np.float64, env.abi
    s = bt.mixed_scene(robot, dt)
    eng = _engine(env, s, True, limiter=False, mix_w=list(bt.MIXED_W))
    try:
        eng.set_max_vel(np.ones(s.B))   # (per-arm limiter speeds in both passes: the same launch options)
        eng.launched_kernels()
        want = ("qdot_vf", "qdot_null", "qdot_out", "status")
        g1 = eng.step_host(s.q, null_control=s.ctrl, want=want, q_ref=s.q_ref)
        k1 = eng.launched_kernels()
        ref1 = bt.restate(s, vf=g1["qdot_vf"], null=g1["qdot_null"], mix_w=bt.MIXED_W, limiter=False)
        same = bt._same(g1["qdot_out"], ref1["qdot_out"]).all(axis=1)
        assert same.all(), "the mixer's sum differs from the host mix of the published channels on arms %s" % np.nonzero(~same)[0][:10]
        assert np.array_equal((g1["status"] & abi.ST_JOINT_AT_GOAL) != 0, ref1["at_goal"]) and 0 < ref1["at_goal"].sum() < s.B
        assert not (g1["status"] & abi.ST_LIMITED).any()
        mv, kinds = bt.tie_speeds(g1["qdot_out"], dt)
        eng.set_params(flags=_flags(abi, s, True, True))
        eng.set_max_vel(mv)
        eng.reset_state()
        g2 = eng.step_host(s.q, null_control=s.ctrl, want=want, q_ref=s.q_ref)
        k2 = eng.launched_kernels()
        assert k1 == k2 and len(k1) == 1, (k1, k2)
        ref2 = bt.restate(s, vf=g1["qdot_vf"], null=g1["qdot_null"], mix_w=bt.MIXED_W, limiter=True, max_vel=mv)
        assert np.array_equal(ref2["limited"], kinds == 1)
        assert np.array_equal((g2["status"] & abi.ST_LIMITED) != 0, ref2["limited"])
        assert np.array_equal(g2["status"] & ~abi.ST_LIMITED, g1["status"])
        bad, worst, allow = bt.compare(g2["qdot_out"], ref2["qdot_out"], ref2["limited"], dt)
        assert len(bad) == 0, "arms %s miss the bar" % bad[:8]
        bt.note("gpu", "mixed %s f64 ns" % robot, "cycle_kernel_x" + (" heavy" if s.n >= 14 else ""), worst, allow, int(ref2["limited"].sum()))
    finally:
        eng.close()


def test_a_limiter_speed_of_infinity_is_no_limit(env):
    """vfik_set_max_vel takes +inf as vfik_params.max_vel does (no arm is limited), and still refuses a negative speed and NaN."""
    s = bt.limiter_scene("lwr", np.float64)
    eng = _engine(env, s, False)
    try:
        eng.set_max_vel(np.full(s.B, np.inf))
        got = eng.step_host(s.q, want=("qdot_out", "status"))
        assert not (got["status"] & env.abi.ST_LIMITED).any()
        assert bt._same(got["qdot_out"], s.cmd).all()
        for v in (-1.0, np.nan):
            with pytest.raises(env.engine.VfikError):
                eng.set_max_vel([v])
    finally:
        eng.close()
