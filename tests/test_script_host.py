"""CPU-side checks of the motion scripts (include/vfik.h: vfik_script): the options struct and its ctypes mirror, the ABI version, the
exported symbols, and the oracle restatement (tests/timed_reference.py: script) against the list forms' entry points -- a script of
frames only is `follow`'s run, one of postures only `follow_js`'s, bit for bit -- and on a hand-made case of two steps."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from vfclik_amd import engine
    return engine.load_library()


def test_script_opts_size_matches_the_mirror(lib):
    from vfclik_amd import _abi
    assert lib.vfik_script_opts_size() == ctypes.sizeof(_abi.ScriptOpts) == 4 + 4 + 8 + 4 + 4 + 4 * 8 + 2 * 8 + 8 * 8 + 4 + 4 + 11 * 8
    o = _abi.ScriptOpts
    assert (o.n_cycles.offset, o.stride.offset, o.dt.offset, o.clamp_to_limits.offset, o.hold.offset) == (0, 4, 8, 16, 20)
    assert (o.pos_prec.offset, o.rot_prec.offset, o.via_pos_prec.offset, o.via_rot_prec.offset) == (24, 32, 40, 48)
    assert (o.prec.offset, o.via_prec.offset, o.mix_frame.offset, o.mix_posture.offset, o.n_way.offset) == (56, 64, 72, 104, 136)
    assert (o.kind.offset, o.way16.offset, o.wayq.offset, o.reached.offset, o.next.offset, o.pending.offset) == (144, 152, 160, 168, 176, 184)
    assert (o.q_out.offset, o.q_traj.offset, o.dist_traj.offset, o.diff.offset, o.way_traj.offset) == (192, 200, 208, 216, 224)
    assert (_abi.STEP_FRAME, _abi.STEP_POSTURE) == (1, 2) and _abi.MIX_FRAME == (1, 1, 0, 0) and _abi.MIX_POSTURE == (0, 0, 1, 0)


def test_abi_version_and_sizes_stay(lib):
    from vfclik_amd import _abi, engine
    assert lib.vfik_abi_version() == 6 == _abi.ABI_VERSION
    sizes = (ctypes.c_size_t * 4)()
    lib.vfik_struct_sizes(sizes)
    assert list(sizes) == [152, 1960, 304, 19 * 8] == [ctypes.sizeof(_abi.Field), ctypes.sizeof(_abi.Chain), ctypes.sizeof(_abi.Params), ctypes.sizeof(engine.IO)]
    assert lib.vfik_goto_opts_size() == 80 and lib.vfik_follow_opts_size() == 128 and lib.vfik_scene_move_size() == 64
    assert lib.vfik_goto_js_opts_size() == 72 and lib.vfik_follow_js_opts_size() == 112


def test_script_symbols_are_declared_and_exported(lib):
    hdr = open(os.path.join(ROOT, "include", "vfik.h")).read()
    types = open(os.path.join(ROOT, "include", "vfik_types.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    raw = ctypes.CDLL(os.path.join(ROOT, "vfclik_amd", "csrc", "libvfik_hip.so"))
    for name in ("vfik_script_opts_size", "vfik_script", "vfik_script_host"):
        assert re.search(r"\b%s\s*\(" % name, code), name + " is not declared in include/vfik.h"
        assert hasattr(raw, name), "libvfik_hip.so does not export " + name
    assert "typedef struct vfik_script_opts" in code and "handlers.py:189-211" in hdr
    assert re.search(r"#define VFIK_STEP_FRAME 1\b", types) and re.search(r"#define VFIK_STEP_POSTURE 2\b", types)


def test_engine_and_sharded_engine_have_the_methods(lib):
    from vfclik_amd import engine, sharding
    assert callable(engine.Engine.script) and callable(engine.Engine.script_host) and callable(sharding.ShardedEngine.script_host)


def test_script_lengths():
    import timed_reference as tr
    kind = np.array([[1, 2, 1, 2], [2, 2, 0, 1], [0, 1, 1, 1], [1, 3, 1, 1], [2, -1, 2, 2], [0, 0, 0, 0]], dtype=np.int32)
    assert list(tr.lengths(kind)) == [4, 2, 0, 1, 1, 0]


STRIDE, N_CYCLES, DT, PREC = 4, 160, 0.01, (0.01, 0.05)
JS_PREC = 0.01 * np.ones(7)


def _same(a, b, keys):
    for k in keys:
        assert np.array_equal(a[k], b[k], equal_nan=True), k


def test_frames_only_is_follow_reference(lib):
    """kind all FRAME (arm 2: one step, then none), mix_frame = params.mix_w[:4]: `follow`'s run with NaN rows ending the paths, bit
    for bit -- the caller gates arm 1.  The two entry points differ in who owns the mixer and in where the lengths come from."""
    import timed_reference as tr
    from oracle import oracle_c
    from vfclik_amd import _abi
    chain, w, qg, way, q0, params = tr.three_lwr_arms(_abi.F_NULLSPACE | _abi.F_MIXER | _abi.F_LIMITER)
    kind = np.full((3, 3), _abi.STEP_FRAME, dtype=np.int32)
    kind[2, 1:] = 0
    way_nan = way.copy()
    way_nan[2, 1:] = np.nan
    kw = dict(hold=True, clamp=True, active=[1, 0, 1], want=("qdot_out", "pose"))
    a = tr.follow(oracle_c, chain, params, q0, w["fields"], w["nfields"], way_nan, N_CYCLES, STRIDE, DT, PREC, via_precision=(0.03, 0.1), **kw)
    b = tr.script(oracle_c, chain, params, q0, w["fields"], w["nfields"], kind, way, qg, N_CYCLES, STRIDE, DT, PREC, JS_PREC,
                  via_precision=(0.03, 0.1), mix_frame=list(params.mix_w)[:4], **kw)
    assert list(a["next"]) == [3, 0, 1]
    _same(a, b, ("reached", "next", "length", "pending", "q_traj", "dist_traj", "way_traj", "q", "qdot_out", "pose", "status"))
    assert np.array_equal(a["fields"]["p"], b["fields"]["p"]) and np.array_equal(a["closest"], b["closest_c"])
    assert np.all(np.isinf(b["closest_j"])) and np.all(b["diff"] == 0) and np.all(np.isnan(b["q_ref"]))


def test_postures_only_is_follow_js_reference(lib):
    """kind all POSTURE, mix_posture = params.mix_w[:4]: `follow_js`'s run, bit for bit; without hold."""
    import timed_reference as tr
    from oracle import oracle_c
    from vfclik_amd import _abi
    chain, w, qg, way, q0, params = tr.three_lwr_arms(_abi.F_MIXER, mix_w=[0, 0, 1, 0, 0, 0], jp_kp=8.0)
    kind = np.full((3, 3), _abi.STEP_POSTURE, dtype=np.int32)
    kind[2, 1:] = 7
    wayq_nan = qg.copy()
    wayq_nan[2, 1:] = np.nan
    kw = dict(hold=False, clamp=True, active=[1, 0, 1], want=("qdot_out",))
    a = tr.follow_js(oracle_c, chain, params, q0, w["fields"], w["nfields"], wayq_nan, N_CYCLES, STRIDE, DT, JS_PREC, via_prec=3 * JS_PREC, **kw)
    b = tr.script(oracle_c, chain, params, q0, w["fields"], w["nfields"], kind, way, qg, N_CYCLES, STRIDE, DT, PREC, JS_PREC,
                  js_via_precision=3 * JS_PREC, mix_posture=list(params.mix_w)[:4], **kw)
    assert list(a["next"]) == [3, 0, 1]
    _same(a, b, ("reached", "next", "length", "pending", "q_traj", "way_traj", "q", "diff", "qdot_out", "status"))
    assert np.array_equal(a["closest"], b["closest_j"]) and np.all(np.isinf(b["closest_c"]))
    assert np.array_equal(b["fields"]["p"], w["fields"]["p"])      # no frame was ever sent


def test_two_steps_by_hand(lib):
    """lwr, mixer only, jp_kp 8.  Arm 0: posture P0 0.02 rad away, then the frame of P0 + 0.1 rad.  Arm 1: that frame first, then a
    posture.  Arm 2: no script (kind zeroed).  Posture steps are a pure P controller under [0, 0, 1, 0] -- the field takes no part --,
    so arm 0 reaches P0 when e0 (1 - kp dt)^c <= prec: cycle 11; the frame step then runs under [1, 1, 0, 0], where the reference row
    takes no part."""
    import timed_reference as tr
    from oracle import oracle_c
    from vfclik_amd import _abi
    chain, w, qg, way, q0, params = tr.three_lwr_arms(_abi.F_MIXER, jp_kp=8.0)
    F, P = _abi.STEP_FRAME, _abi.STEP_POSTURE
    kind = np.array([[P, F, 0], [F, P, 0], [0, F, P]], dtype=np.int32)
    sign = np.array([1, -1, 1, -1, 1, -1, 1.0])
    q0 = np.array([qg[0, 0] + 0.02 * sign, qg[1, 0] + 0.03 * sign, qg[2, 0]])
    n_cycles = 240
    r = tr.script(oracle_c, chain, params, q0, w["fields"], w["nfields"], kind, way, qg, n_cycles, STRIDE, DT, PREC, JS_PREC, hold=True,
                  clamp=True, want=("qdot_out",))
    assert list(r["length"]) == [2, 2, 0] and list(r["next"]) == [2, 2, 0]
    thr = np.array([PREC[0], PREC[1] * 180.0 / np.pi])
    # arm 0: the closed form of its posture step, then the frame
    k0 = 2
    assert r["reached"][0, 0] == 11 == (k0 + 1) * STRIDE - 1                                     # 0.92^12 < 0.01 / 0.02 < 0.92^8
    e = 0.02 * sign * (1.0 - 8.0 * DT) ** 12
    assert np.abs(r["q_traj"][k0, 0] - (qg[0, 0] + e)).max() < 1e-12
    assert np.array_equal(r["diff"][0], qg[0, 0] - r["q_traj"][k0, 0])                            # kept over the frame step
    k1 = (r["reached"][0, 1] + 1) // STRIDE - 1
    assert k1 > k0 and np.all(r["dist_traj"][k1, 0] < thr) and not np.all(r["dist_traj"][k1 - 1, 0] < thr)
    assert list(r["way_traj"][:k0 + 1, 0]) == [0] * (k0 + 1) and np.all(r["way_traj"][k0 + 1:, 0] == 1)
    assert np.array_equal(r["fields"]["p"][0, 0, :12], way[0, 1, :12]) and np.array_equal(r["q_ref"][0], qg[0, 0])
    # arm 1: no controller until its posture; the goal stays the frame it was sent first
    j0, j1 = [(c + 1) // STRIDE - 1 for c in r["reached"][1, :2]]
    assert 0 <= j0 < j1 and np.all(r["dist_traj"][j0, 1] < thr)
    assert tr.rule(qg[1:2, 1], r["q_traj"][j1, 1:2], JS_PREC).all() and not tr.rule(qg[1:2, 1], r["q_traj"][j1 - 1, 1:2], JS_PREC).any()
    assert np.array_equal(r["diff"][1], qg[1, 1] - r["q_traj"][j1, 1]) and np.array_equal(r["fields"]["p"][1, 0, :12], way[1, 0, :12])
    assert np.all(r["q_traj"][j1:, 1] == r["q_traj"][j1, 1])                                      # hold
    # between j0 and j1 arm 1 is a pure P controller towards its posture
    e1 = (qg[1, 1] - r["q_traj"][j0, 1]) * (1.0 - 8.0 * DT) ** ((j1 - j0) * STRIDE)
    assert np.abs(r["q_traj"][j1, 1] - (qg[1, 1] - e1)).max() < 1e-12
    # arm 2: kept out
    assert np.all(r["reached"][2] == -1) and np.all(r["q_traj"][:, 2] == q0[2]) and np.all(r["way_traj"][:, 2] == -1)
    assert np.all(np.isnan(r["dist_traj"][:, 2])) and np.all(np.isnan(r["q_ref"][2])) and np.array_equal(r["fields"]["p"][2], w["fields"]["p"][2])
    for k in range(n_cycles // STRIDE):
        cyc = (k + 1) * STRIDE - 1
        assert r["pending"][k] == sum(1 for b in (0, 1) if r["reached"][b, 1] > cyc)
    # the replay of the state machine on the run's own rows gives the run's decisions
    m = tr.replay(kind, qg, r["present"], r["q_traj"], r["dist_traj"], n_cycles, STRIDE, PREC, JS_PREC, hold=True)
    assert np.array_equal(m.reached, r["reached"]) and np.array_equal(m.next, r["next"]) and np.array_equal(m.way_traj, r["way_traj"])
    assert np.array_equal(m.pending, r["pending"]) and np.array_equal(m.diff, r["diff"])
