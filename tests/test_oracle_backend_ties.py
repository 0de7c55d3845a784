"""The C oracle held to the CPython restatement of the bridge back end on the tie scenes of tests/backend_ties.py, bit for bit, and every
scene's construction conditions: a tie must be a tie in doubles, asserted on the constructed arrays.  The GPU side of the same scenes is
tests/test_gpu_backend_ties.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import backend_ties as bt  # noqa: E402

CASES = [(r, t) for r in bt.ROBOTS for t in (np.float32, np.float64)]
IDS = ["%s-f%d" % (r, 32 if t == np.float32 else 64) for r, t in CASES]
SCENES = ("limiter", "joint", "joint_cycle", "form")


def _oracle(oc, s, ns=False):
    """The C oracle arm by arm (its mixer weights and max_vel are batch-wide): qdot_out, the back end's status bits, mixed where it is the output."""
    from vfclik_amd import _abi
    B, n = s.B, s.n
    out, status = np.zeros((B, n)), np.zeros(B, dtype=np.int32)
    flags = _abi.F_MIXER | (_abi.F_LIMITER if s.limiter else 0) | (_abi.F_NULLSPACE if ns else 0)
    for b in range(B):
        sl = slice(b, b + 1)
        p = _abi.default_params(flags=flags, mix_w=s.mixw[b].tolist(), max_vel=float(s.max_vel[b]) if s.max_vel is not None else 1.0)
        ext = np.stack([s.ext[ch][sl] for ch in range(4)])
        at = 0
        if s.q_ref is not None and not np.isnan(s.q_ref[b, 0]):
            lo, hi = (s.q_lo[b], s.q_hi[b]) if s.q_lo is not None else (s.chain.q_lo, s.chain.q_hi)
            jc, flag = oc.joint_p(s.q_ref[sl], s.q[sl], lo, hi, bt.JP_KP, bt.JP_DELTA)
            ext[0], at = jc, int(flag[0])
        kw = dict(q_lo=s.q_lo[sl], q_hi=s.q_hi[sl]) if s.q_lo is not None else {}
        r = oc.cycle_batch(s.chain, p, s.q[sl], s.w["fields"][sl], s.w["nfields"][sl], ext_cmd=ext, want=("qdot_out", "status"), **kw)
        v = r["qdot_out"]
        if s.q_cmded is not None:
            v = oc.lwr_cmd(v, s.q[sl], s.q_cmded[sl], [bool(np.all(s.mixw[b] == 0.0))])
        out[b] = v[0]
        status[b] = (int(r["status"][0]) & bt.BACK_END_BITS) | (bt.ST_JOINT_AT_GOAL if at else 0)
    return out, status


@pytest.mark.parametrize("robot,dt", CASES, ids=IDS)
@pytest.mark.parametrize("scene", SCENES)
def test_scene_conditions_and_the_c_oracle(oracle_c, scene, robot, dt):
    s = bt.make_scene(scene, robot, dt)
    bad = bt.CONDITIONS[s.name](s)
    assert not bad, "\n".join(bad[:10])
    # the kinds whose condition needs a value finer than the float32 grid stay a small part of the scene
    assert s.f64_only.sum() <= s.B // 8
    ref = bt.restate(s)
    out, status = _oracle(oracle_c, s)
    same = bt._same(out, ref["qdot_out"]).all(axis=1)
    assert same.all(), "oracle_c differs from the CPython restatement on arms %s" % np.nonzero(~same)[0][:10]
    assert np.array_equal(status, bt.status_bits(ref))
    # the restatement's doubles give the float32 allowance to less than 1 % of the limited rows
    lim = ref["limited"]
    if lim.any():
        near = (bt.near_f32_boundary(ref["qdot_out"]) & lim[:, None]).any(axis=1).sum()
        assert near < bt.ALLOWANCE_CAP * lim.sum(), (near, lim.sum())
        bad_rows, worst, allow = bt.compare(out.astype(dt), ref["qdot_out"], lim, dt)
        assert len(bad_rows) == 0 and allow == 0 and worst == 0.0
    bad_rows, worst, allow = bt.compare(out.astype(dt), ref["qdot_out"], lim, dt)   # (every scene writes its row: no limited rows, 0 of 0)
    assert len(bad_rows) == 0 and allow == 0
    bt.note("cpu", "%s %s f%d" % (scene, robot, 32 if dt == np.float32 else 64), "oracle_c", worst, allow, int(lim.sum()))
    if scene == "limiter":
        # unlimited rows are the command, bit for bit; every decision is lead > max_vel on the finite entries
        un = ~lim
        assert bt._same(ref["qdot_out"][un], s.cmd[un]).all()
        with np.errstate(invalid="ignore"):
            lead = np.nanmax(np.abs(s.cmd), axis=1)
        assert np.array_equal(lim, lead > s.max_vel)
        assert lim.sum() >= s.B // 4 and un.sum() >= s.B // 4
    if scene.startswith("joint"):
        assert 0 < ref["at_goal"].sum() < s.B


@pytest.mark.parametrize("robot", ("powercube6", "lwr", "lwr_dual14"))
def test_mixed_input_limiter_on_the_c_oracle(oracle_c, robot):
    """Limiter, mixed input: the host mix of the oracle's published channels equals its qdot_out bit for bit for every arm; with max_vel the lead
    of each arm's own command, or one ulp to either side, every decision is lead > max_vel, unlimited rows are the command and limited rows
    vfik_numpy.limiter's, bit for bit."""
    from oracle import vfik_numpy as vn
    from vfclik_amd import _abi
    dt = np.float64
    s = bt.mixed_scene(robot, dt)
    flags = _abi.F_NULLSPACE | _abi.F_MIXER
    p = _abi.default_params(flags=flags, mix_w=list(bt.MIXED_W), jp_kp=bt.JP_KP, jp_delta=bt.JP_DELTA)
    jc, at = oracle_c.joint_p(s.q_ref, s.q, s.chain.q_lo, s.chain.q_hi, bt.JP_KP, bt.JP_DELTA)
    ext = s.ext.copy()
    ext[0] = jc
    r1 = oracle_c.cycle_batch(s.chain, p, s.q, s.w["fields"], s.w["nfields"], null_control=s.ctrl, ext_cmd=ext)
    ref1 = bt.restate(s, vf=r1["qdot_vf"], null=r1["qdot_null"], mix_w=bt.MIXED_W, limiter=False)
    assert np.array_equal(ref1["qdot_out"], r1["qdot_out"])
    assert np.array_equal(ref1["at_goal"], at != 0) and 0 < at.sum() < s.B
    for b in range(s.B):
        cmd = np.stack([r1["qdot_vf"][b], r1["qdot_null"][b], jc[b], ext[1][b], ext[2][b], ext[3][b]])
        assert np.array_equal(oracle_c.mix(cmd, np.array(bt.MIXED_W)), r1["qdot_out"][b]), b
    mv, kinds = bt.tie_speeds(r1["qdot_out"], dt)
    lead = np.abs(r1["qdot_out"]).max(axis=1)
    assert np.array_equal(mv[kinds == 0], lead[kinds == 0]) and np.all(mv[kinds == 1] < lead[kinds == 1]) and np.all(mv[kinds == 2] > lead[kinds == 2])
    for b in range(s.B):
        sl = slice(b, b + 1)
        pb = _abi.default_params(flags=flags | _abi.F_LIMITER, mix_w=list(bt.MIXED_W), max_vel=float(mv[b]))
        r2 = oracle_c.cycle_batch(s.chain, pb, s.q[sl], s.w["fields"][sl], s.w["nfields"][sl], null_control=s.ctrl[sl], ext_cmd=ext[:, sl])
        limited = bool(r2["status"][0] & _abi.ST_LIMITED)
        assert limited == (lead[b] > mv[b]) == (kinds[b] == 1), b
        want, lim = vn.limiter(r1["qdot_out"][b].tolist(), float(mv[b]))
        assert lim == limited and np.array_equal(r2["qdot_out"][0], np.array(want)), b
        if not limited:
            assert np.array_equal(r2["qdot_out"][0], r1["qdot_out"][b]), b


def test_the_table(oracle_c):
    """(the CPU rows of profiles/backend_observer_accuracy.txt, when VFIK_BACKEND_TABLE names a file)"""
    path = os.environ.get("VFIK_BACKEND_TABLE")
    if path:
        bt.write_table(path)
