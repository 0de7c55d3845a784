"""Coupled goto_host and follow_host under an avoid rule (include/vfik.h: vfik_set_avoid_rule) on the GPU against tests/avoid_reference.py,
the oracle-stepped coupled move with the push in front of every block.

The moves: avoid_reference.MOVES -- coupled_reference.pair_case scenes of 203 (the LWR) and 130 arms (two LWRs in series), nullspace module
and mixer, mix_w[4] = 1, float64 at stride 1, float32 and the 14-joint follow at stride 4, coupled_reference.N_CYCLES cycles -- under
avoid_reference.RULE on channel 4, chosen on the CPU so that in the ORACLE's run at least ten arms carry a nonzero command in some block,
at least one carries none in any, and at least one arm's tightest clearance is larger with the rule than without (asserted here on the
reference's run, and in tests/test_avoid_moves_reference.py).

Against the reference: arrived / reached / next exact for the arms outside coupled_reference.MARGIN of a threshold in the reference's run
(coupled_reference.left_out, with its cap on the share left out, before the GPU's rows are read); the joint path within
coupled_reference.PATH_BAR.  On the GPU's own rows, every arm: avoid_traj[k] equals link_avoid of q_traj[k - 1] and link_traj[k] bit for
bit.  One script_host run -- a posture, then two frames (avoid_reference.script_case) -- likewise.  With scale all zero the move equals the coupled move without a rule bit for bit; the rule goes with the coupling; the channel is
zero after the move."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import avoid_reference as ar  # noqa: E402
import coupled_reference as cr  # noqa: E402

pytestmark = pytest.mark.gpu

N_CYCLES, DT, PREC = cr.N_CYCLES, cr.DT, cr.PREC
KEYS = ("q_traj", "dist_traj", "pending", "q", "qdot_out", "status")


@pytest.fixture(scope="module")
def env():
    import __graft_entry__ as g
    g.build()
    from oracle import oracle_c
    from vfclik_amd import _abi, engine
    oracle_c.build()

    class E:
        pass

    e = E()
    e.oc, e.abi, e.engine = oracle_c, _abi, engine
    return e


def _engine(env, name, c, params, rule=True, scale=None):
    m = ar.MOVES[name]
    n_checks = N_CYCLES // m["stride"]
    eng = env.engine.Engine(c["chain"], m["B"], io_dtype=m["io_dtype"], max_slots=8, params=params)
    eng.set_fields(c["w"]["fields"], c["w"]["nfields"])
    eng.set_link_spheres(c["spheres"])
    eng.set_coupling(src_arm=c["src_arm"], xform=c["xform"], first_rep=c["first_rep"], trace_checks=n_checks)
    if rule:
        eng.set_avoid_rule(ar.RULE[name]["gain"], ar.RULE[name]["d0"], channel=ar.CHANNEL, scale=scale, trace_checks=n_checks)
    return eng


def _move(eng, name, c):
    m = ar.MOVES[name]
    q_in = c["q0"].astype(eng.io_dtype)
    common = dict(stride=m["stride"], hold=m["hold"], clamp=True, trajectory=True, want=("qdot_out", "status"))
    if c["way"] is None:
        return eng.goto_host(q_in, N_CYCLES, DT, PREC, **common)
    return eng.follow_host(q_in, c["way"], N_CYCLES, DT, PREC, **common)


@pytest.mark.parametrize("name", sorted(ar.MOVES))
def test_against_the_reference(env, name):
    c, params, ref = ar.reference(env.oc, name)
    _c, _p, off = ar.reference(env.oc, name, gain=0.0)
    m = ar.MOVES[name]
    B, io, L, n = m["B"], np.dtype(m["io_dtype"]), len(c["spheres"]), c["chain"].n
    n_checks = N_CYCLES // m["stride"]
    # the scene and who is left out: on the reference's run, before the GPU's is read
    pushed, never, wider = ar.conditions(ref, off)
    print("%s: reference: %d arms pushed, %d never, %d with more room at their tightest" % (name, pushed, never, wider))
    assert pushed >= 10 and never >= 1 and wider >= 1
    part = ref["length"] > 0
    out, near, share, cap = cr.left_out(ref, part, io, c["src_arm"], m["hold"])
    print("%s: left out %d of %d arms (%.1f %%, cap %.0f %%)" % (name, np.count_nonzero(out & part), np.count_nonzero(part), 100 * share, 100 * cap))
    assert share <= cap, share
    inc = ~out

    eng = _engine(env, name, c, params)
    got = _move(eng, name, c)
    cmd, link = eng.avoid_traj(), eng.link_traj()
    assert got["checks_run"] == n_checks and cmd.shape == (n_checks, B, n) and cmd.dtype == io

    # against the reference
    if c["way"] is None:
        assert np.array_equal(got["arrived"][inc], ref["arrived"][inc]), np.flatnonzero(inc & (got["arrived"] != ref["arrived"]))
    else:
        assert np.array_equal(got["reached"][inc], ref["reached"][inc]) and np.array_equal(got["next"][inc], ref["next"][inc])
    rows = inc if m["hold"] else np.ones(B, dtype=bool)
    eq = np.abs(got["q_traj"][:, rows].astype(np.float64) - ref["q_traj"][:, rows])
    ec = np.abs(cmd[:, rows].astype(np.float64) - ref["avoid_traj"][:, rows])
    print("%s: q_traj max error %.3e (bar %.1e); avoid_traj max error %.3e of %.3e" % (name, eq.max(), cr.PATH_BAR[io], ec.max(), np.abs(ref["avoid_traj"]).max()))
    assert eq.max() < cr.PATH_BAR[io]
    assert np.any(cmd != 0) and np.count_nonzero(np.any(cmd != 0, axis=(0, 2))) >= 10 and not np.all(np.any(cmd != 0, axis=(0, 2)))

    # every arm, on the GPU's own rows
    q_in = np.concatenate([c["q0"].astype(io)[None], got["q_traj"][:-1]], axis=0)
    for k in range(n_checks):
        want = eng.link_avoid_host(q_in[k].astype(np.float64), link[k].astype(np.float64), 0, L, gain=ar.RULE[name]["gain"], d0=ar.RULE[name]["d0"])
        assert np.array_equal(cmd[k].astype(np.float64), want), k
    eng.close()


def test_script_against_the_reference(env):
    """one script_host run, a posture and two frames, with the rule on channel 4 (in a script the weights of channels 4 and 5 are the
    arm's own row's: the push keeps its weight over both kinds of step)"""
    c, params, ref, off = ar.script_reference(env.oc)
    m = ar.SCRIPT
    B, io, L, n = m["B"], np.dtype(m["io_dtype"]), len(c["spheres"]), c["chain"].n
    n_checks = N_CYCLES // m["stride"]
    pushed, never, wider = ar.conditions(ref, off)
    assert pushed >= 10 and never >= 1 and wider >= 1
    part = ref["length"] > 0
    out, near, share, cap = cr.left_out(ref, part, io, c["src_arm"], m["hold"])
    print("script: left out %d of %d arms (%.1f %%, cap %.0f %%)" % (np.count_nonzero(out & part), np.count_nonzero(part), 100 * share, 100 * cap))
    assert share <= cap, share
    inc = ~out
    eng = env.engine.Engine(c["chain"], B, io_dtype=io, max_slots=8, params=params)
    eng.set_fields(c["w"]["fields"], c["w"]["nfields"])
    eng.set_link_spheres(c["spheres"])
    eng.set_coupling(src_arm=c["src_arm"], xform=c["xform"], first_rep=c["first_rep"], trace_checks=n_checks)
    eng.set_avoid_rule(m["gain"], m["d0"], channel=ar.CHANNEL, trace_checks=n_checks)
    got = eng.script_host(c["q0"].astype(io), c["kind"], c["way3"], c["wayq"], N_CYCLES, DT, PREC, np.full(n, ar.JS_PREC),
                          js_via_precision=np.full(n, ar.JS_VIA), stride=m["stride"], hold=m["hold"], clamp=True, trajectory=True, want=("qdot_out", "status"))
    cmd, link = eng.avoid_traj(), eng.link_traj()
    assert got["checks_run"] == n_checks
    assert np.array_equal(got["reached"][inc], ref["reached"][inc]) and np.array_equal(got["next"][inc], ref["next"][inc])
    eq = np.abs(got["q_traj"][:, inc].astype(np.float64) - ref["q_traj"][:, inc])
    print("script: q_traj max error %.3e (bar %.1e)" % (eq.max(), cr.PATH_BAR[io]))
    assert eq.max() < cr.PATH_BAR[io]
    q_in = np.concatenate([c["q0"].astype(io)[None], got["q_traj"][:-1]], axis=0)
    for k in range(n_checks):
        want = eng.link_avoid_host(q_in[k].astype(np.float64), link[k].astype(np.float64), 0, L, gain=m["gain"], d0=m["d0"])
        assert np.array_equal(cmd[k].astype(np.float64), want), k
    assert np.count_nonzero(np.any(cmd != 0, axis=(0, 2))) >= 10
    eng.close()


@pytest.mark.parametrize("name", ["goto64", "goto32"])
def test_scale_zero_and_rule_off_equal_the_coupled_move(env, name):
    c, params, _ref = ar.reference(env.oc, name)
    B = ar.MOVES[name]["B"]
    keys = KEYS + ("arrived",)
    plain = _engine(env, name, c, params, rule=False)
    want = _move(plain, name, c)
    want_link = plain.link_traj()
    # a rule under which no arm gives way: the kernel runs in front of every block and writes zeros
    none = _engine(env, name, c, params, scale=np.zeros(B))
    got = _move(none, name, c)
    assert not none.avoid_traj().any()
    for k in keys:
        assert np.array_equal(got[k], want[k]), k
    assert np.array_equal(none.link_traj(), want_link, equal_nan=True)
    # a move under the rule, then the rule off and the scene as it was: the coupled move
    eng = _engine(env, name, c, params)
    moved = _move(eng, name, c)
    assert eng.avoid_traj().any() and not np.array_equal(moved["q_traj"], want["q_traj"])
    eng.set_avoid_rule(None)
    eng.set_fields(c["w"]["fields"], c["w"]["nfields"])
    eng.reset_state()
    again = _move(eng, name, c)
    for k in keys:
        assert np.array_equal(again[k], want[k]), k
    with pytest.raises(env.engine.VfikError):
        eng.avoid_traj()
    for e in (plain, none, eng):
        e.close()


def test_sharded_form(env):
    """ShardedEngine over devices (0, 0): two handles of 102 arms give the single engine's commands, traces and move"""
    from vfclik_amd import robots, sharding
    chain, B, io = robots.lwr(), 204, np.float32
    c = cr.pair_case(chain, B, io, seed=9)
    params = env.abi.default_params(flags=env.abi.F_NULLSPACE | env.abi.F_MIXER, max_vel=0.7, mix_w=ar.MIX_W)
    scale = np.where(np.arange(B) % 3 == 0, 0.0, 1.0)
    kw = dict(stride=4, hold=True, clamp=True, trajectory=True, want=("qdot_out",))
    res = []
    for make in (lambda: env.engine.Engine(chain, B, io_dtype=io, max_slots=8, params=params),
                 lambda: sharding.ShardedEngine(chain, B, rank=0, world=1, devices=(0, 0), io_dtype=io, max_slots=8, params=params)):
        e = make()
        e.set_fields(c["w"]["fields"], c["w"]["nfields"])
        e.set_link_spheres(c["spheres"])
        e.set_coupling(src_arm=c["src_arm"], xform=c["xform"], first_rep=c["first_rep"], trace_checks=10)
        e.set_avoid_rule(0.4, 0.12, channel=4, scale=scale, trace_checks=10)
        got = e.goto_host(c["q0"].astype(io), 40, DT, PREC, **kw)
        traj, link = e.avoid_traj(), e.link_traj()
        cmd = e.link_avoid_host(c["q0"], link[0].astype(np.float64), gain=0.4, d0=0.12, scale=scale)
        e.set_avoid_rule(None)
        res.append((got, traj, cmd))
        e.close()
    (a, ta, ca), (b, tb, cb) = res
    assert ta.any() and not ta[:, scale == 0].any() and np.array_equal(ta, tb) and np.array_equal(ca, cb) and np.array_equal(ca.astype(io), ta[0])
    for k in ("q_traj", "arrived", "q", "qdot_out"):
        assert np.array_equal(a[k], b[k]), k


def test_the_channel_is_zero_after_the_move(env):
    """a velocity push must not outlive the move: the next step is that of a handle whose channel was zeroed with set_ext_cmd(4, None)"""
    name = "goto32"
    c, params, _ref = ar.reference(env.oc, name)
    eng = _engine(env, name, c, params)
    got = _move(eng, name, c)
    assert eng.avoid_traj()[-1].any()                                  # the last block did push
    q = got["q"].astype(np.float64)
    eng.reset_state()
    a = eng.step_host(q, want=("qdot_out",))["qdot_out"]
    eng.set_avoid_rule(None)
    eng.set_ext_cmd(ar.CHANNEL, None)
    eng.reset_state()
    b = eng.step_host(q, want=("qdot_out",))["qdot_out"]
    assert np.array_equal(a, b)
    eng.set_ext_cmd(ar.CHANNEL, np.full((ar.MOVES[name]["B"], c["chain"].n), 0.01))      # (and the channel does reach qdot_out)
    eng.reset_state()
    assert not np.array_equal(eng.step_host(q, want=("qdot_out",))["qdot_out"], b)
    eng.close()


def test_the_rule_goes_with_the_coupling_and_its_refusals(env):
    name = "goto32"
    c, params, _ref = ar.reference(env.oc, name)
    m = ar.MOVES[name]
    B, n = m["B"], c["chain"].n
    E = env.engine.VfikError
    eng = env.engine.Engine(c["chain"], B, io_dtype=m["io_dtype"], max_slots=8, params=params)
    eng.set_fields(c["w"]["fields"], c["w"]["nfields"])
    eng.set_link_spheres(c["spheres"])
    with pytest.raises(E, match="vfik_set_coupling"):
        eng.set_avoid_rule(0.4, 0.1)
    couple = lambda: eng.set_coupling(src_arm=c["src_arm"], xform=c["xform"], first_rep=c["first_rep"])
    couple()
    L = len(c["spheres"])
    for bad in (dict(d0=0.0), dict(d0=-1.0), dict(d0=np.inf), dict(d0=np.nan), dict(gain=np.nan), dict(gain=np.inf), dict(channel=2), dict(channel=6),
                dict(channel=-1), dict(mask=[1 << L] * L)):
        with pytest.raises(E):
            eng.set_avoid_rule(**dict(dict(gain=0.4, d0=0.1), **bad))
    r = env.abi.AvoidRule()
    r.gain, r.d0, r.channel, r.reserved = 0.4, 0.1, 4, 1
    import ctypes as C
    assert eng.lib.vfik_set_avoid_rule(eng.h, C.byref(r)) == -1        # reserved != 0
    host = np.zeros(B, dtype=m["io_dtype"])
    r.reserved, r.scale = 0, host.ctypes.data
    assert eng.lib.vfik_set_avoid_rule(eng.h, C.byref(r)) == -1        # scale is no device pointer
    cmd = np.full((B, n), 0.01)
    eng.set_ext_cmd(4, cmd)                                            # no rule yet: the channel is the caller's
    epoch = eng.lib.vfik_launch_epoch(eng.h)
    eng.set_avoid_rule(0.4, 0.1, channel=4)
    assert eng.lib.vfik_launch_epoch(eng.h) > epoch                    # a setter: the epoch moves
    with pytest.raises(E, match="avoid rule"):
        eng.set_ext_cmd(4, cmd)                                        # the rule's channel
    eng.set_ext_cmd(3, cmd)                                            # another channel stays the caller's
    eng.set_ext_cmd(3, None)
    for drop in (lambda: eng.set_coupling(None), lambda: eng.set_link_spheres(c["spheres"])):
        drop()
        eng.set_ext_cmd(4, cmd)                                        # the rule went with the coupling: the channel is the caller's again
        eng.set_ext_cmd(4, None)
        eng.set_link_spheres(c["spheres"])
        couple()
        eng.set_avoid_rule(0.4, 0.1, channel=4)
    eng.close()
    # a timed move under the rule needs the mixer
    bare = env.engine.Engine(c["chain"], B, io_dtype=m["io_dtype"], max_slots=8, params=env.abi.default_params(flags=0, max_vel=0.7))
    bare.set_fields(c["w"]["fields"], c["w"]["nfields"])
    bare.set_link_spheres(c["spheres"])
    bare.set_coupling(src_arm=c["src_arm"], xform=c["xform"], first_rep=c["first_rep"])
    bare.set_avoid_rule(0.4, 0.1)
    with pytest.raises(E, match="VFIK_F_MIXER"):
        bare.goto_host(c["q0"].astype(bare.io_dtype), 8, DT, PREC, stride=4)
    bare.set_avoid_rule(None)
    bare.goto_host(c["q0"].astype(bare.io_dtype), 8, DT, PREC, stride=4)
    bare.close()
