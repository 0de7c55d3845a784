"""CPU-side checks of the joint-space goto and the posture lists (include/vfik.h: vfik_goto_js / vfik_follow_js): the option structs and
their ctypes mirrors, the ABI version, the exported symbols, and the oracle restatement (tests/timed_reference.py: goto_js, follow_js) against the closed
form of a pure P controller."""
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


def test_goto_js_opts_size_matches_the_mirror(lib):
    from vfclik_amd import _abi
    assert lib.vfik_goto_js_opts_size() == ctypes.sizeof(_abi.GotoJsOpts) == 4 + 4 + 8 + 4 + 4 + 6 * 8
    o = _abi.GotoJsOpts
    assert (o.n_cycles.offset, o.stride.offset, o.dt.offset, o.clamp_to_limits.offset, o.hold.offset) == (0, 4, 8, 16, 20)
    assert (o.prec.offset, o.arrived.offset, o.pending.offset, o.q_out.offset, o.q_traj.offset, o.diff.offset) == (24, 32, 40, 48, 56, 64)


def test_follow_js_opts_size_matches_the_mirror(lib):
    from vfclik_amd import _abi
    assert lib.vfik_follow_js_opts_size() == ctypes.sizeof(_abi.FollowJsOpts) == 4 + 4 + 8 + 4 + 4 + 2 * 8 + 4 + 4 + 8 * 8
    o = _abi.FollowJsOpts
    assert (o.n_cycles.offset, o.stride.offset, o.dt.offset, o.clamp_to_limits.offset, o.hold.offset) == (0, 4, 8, 16, 20)
    assert (o.prec.offset, o.via_prec.offset, o.n_way.offset, o.wayq.offset, o.reached.offset, o.next.offset) == (24, 32, 40, 48, 56, 64)
    assert (o.pending.offset, o.q_out.offset, o.q_traj.offset, o.diff.offset, o.way_traj.offset) == (72, 80, 88, 96, 104)


def test_abi_version_and_sizes_stay(lib):
    from vfclik_amd import _abi, engine
    assert lib.vfik_abi_version() == 6 == _abi.ABI_VERSION
    sizes = (ctypes.c_size_t * 4)()
    lib.vfik_struct_sizes(sizes)
    assert list(sizes) == [ctypes.sizeof(_abi.Field), ctypes.sizeof(_abi.Chain), ctypes.sizeof(_abi.Params), ctypes.sizeof(engine.IO)]
    assert list(sizes) == [152, 1960, 304, 19 * 8]   # as before these entry points
    assert lib.vfik_goto_opts_size() == 80 and lib.vfik_follow_opts_size() == 128 and lib.vfik_scene_move_size() == 64


def test_js_symbols_are_declared_and_exported(lib):
    hdr = open(os.path.join(ROOT, "include", "vfik.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    raw = ctypes.CDLL(os.path.join(ROOT, "vfclik_amd", "csrc", "libvfik_hip.so"))
    for name in ("vfik_goto_js_opts_size", "vfik_goto_js", "vfik_goto_js_host", "vfik_follow_js_opts_size", "vfik_follow_js",
                 "vfik_follow_js_host"):
        assert re.search(r"\b%s\s*\(" % name, code), name + " is not declared in include/vfik.h"
        assert hasattr(raw, name), "libvfik_hip.so does not export " + name
    assert "typedef struct vfik_goto_js_opts" in code and "typedef struct vfik_follow_js_opts" in code and "handlers.py:544-576" in hdr
    assert "VFIK_F_MIXER" in hdr.split("Joint-space goto.")[1].split("typedef struct vfik_goto_js_opts")[0]   # what the flag's absence means


def test_engine_and_sharded_engine_have_the_methods(lib):
    from vfclik_amd import engine, sharding
    for name in ("goto_js", "goto_js_host", "follow_js", "follow_js_host"):
        assert callable(getattr(engine.Engine, name))
    for name in ("goto_js_host", "follow_js_host"):
        assert callable(getattr(sharding.ShardedEngine, name))


def test_rule_edges_are_computed_as_written():
    """The two edges are fl(ref - prec) and fl(ref + prec): a q equal to an edge passes, its neighbour outside does not, whatever
    |ref - q| <= prec says."""
    import timed_reference as tr
    rng = np.random.default_rng(3)
    ref = rng.uniform(-2, 2, (4000, 1))
    prec = rng.uniform(0.001, 0.3, (4000, 1))
    lo, hi = ref - prec, ref + prec
    assert tr.rule(ref, lo, prec).all() and tr.rule(ref, hi, prec).all()
    assert not tr.rule(ref, np.nextafter(lo, -np.inf), prec).any() and not tr.rule(ref, np.nextafter(hi, np.inf), prec).any()
    assert not tr.rule(ref, np.full_like(ref, np.nan), prec).any() and not tr.rule(np.full_like(ref, np.nan), lo, prec).any()
    assert tr.rule(ref, ref + 1e9, np.full_like(prec, np.inf)).all()    # +inf: the joint never decides
    fabs = np.abs(ref - lo) <= prec
    assert np.count_nonzero(~fabs) > 100                                # ... and |ref - q| <= prec is another function


def test_list_lengths():
    import timed_reference as tr
    way = np.zeros((5, 3, 7))
    way[1, 2, 0] = way[2, 1, 0] = way[3, 0, 0] = np.nan
    way[4, 1, 0] = way[4, 2, 5] = np.nan    # a NaN elsewhere in a row does not end a list; rows behind the first NaN row do not count
    way[3, 2, 0] = 1.0
    assert list(tr.list_lengths(way)) == [3, 2, 1, 0, 1]


KP, DT, STRIDE, N_CYCLES = 8.0, 0.01, 4, 80
PREC = 0.01 * np.ones(7)


def _predicted(e0, prec, stride, n_cycles):
    """Arrival of a pure P controller under Euler: e_c = e_0 (1 - kp dt)^c after c cycles; the first check whose c makes every joint's
    |e_c| <= prec.  Returns (arrived or -1, margin): margin = how far the deciding ratio is from 1 at the check before and at arrival."""
    f = 1.0 - KP * DT
    for k in range(n_cycles // stride):
        c = (k + 1) * stride
        worst = np.max(np.abs(e0) / prec) * f ** c
        if worst <= 1.0:
            return c - 1, min(1.0 - worst, np.max(np.abs(e0) / prec) * f ** (c - stride) - 1.0 if k else np.inf)
    return -1, np.inf


@pytest.fixture(scope="module")
def pure_p(lib):
    """lwr under pure joint control (mixer [0, 0, 1, 0, 0, 0], F_MIXER; the rollout's clamp off, nothing near a limit for arms 0-2):
    arm 0 starts 0.02 rad from its reference, arm 1 0.25 rad, arm 2 is gated off by the caller; arm 3's reference lies 0.1 rad BEYOND the
    upper limit of joint 0 with precision 0.01: the controller keeps the clamped value, the rule reads what the caller sent."""
    import timed_reference as tr
    from oracle import oracle_c
    from vfclik_amd import _abi, robots, synth
    chain = robots.lwr()
    w = synth.make_workload(chain, 4, 2, seed=53, io_dtype=np.float64)
    ref = np.array([[0.3, 0.5, -0.2, 1.0, 0.1, -0.6, 0.2]] * 4) * np.array([[1.0], [0.8], [-0.9], [0.5]])
    sign = np.array([1, -1, 1, -1, 1, -1, 1.0])
    q0 = ref + np.array([[0.02], [0.25], [0.1], [0.0]]) * sign
    ref[3, 0] = chain.q_hi[0] + 0.1
    q0[3, 0] = chain.q_hi[0] - 0.05
    params = _abi.default_params(flags=_abi.F_MIXER, mix_w=[0, 0, 1, 0, 0, 0], jp_kp=KP)
    out = tr.goto_js(oracle_c, chain, params, q0, w["fields"], w["nfields"], ref, N_CYCLES, STRIDE, DT, PREC, hold=True,
                               clamp=False, active=[1, 1, 0, 1])
    return chain, q0, ref, out


def test_reference_against_the_closed_form(pure_p):
    chain, q0, ref, out = pure_p
    n_checks = N_CYCLES // STRIDE
    for b in (0, 1):
        want, margin = _predicted(ref[b] - q0[b], PREC, STRIDE, N_CYCLES)
        assert margin > 1e-3 and want >= 0          # the prediction is no borderline case
        assert out["arrived"][b] == want, (b, out["arrived"][b], want)
        k = (want + 1) // STRIDE - 1
        e = (ref[b] - q0[b]) * (1.0 - KP * DT) ** (want + 1)
        assert np.abs(out["q_traj"][k, b] - (ref[b] - e)).max() < 1e-12
        assert np.all(out["q_traj"][k:, b] == out["q_traj"][k, b])                       # hold
        assert np.array_equal(out["diff"][b], ref[b] - out["q_traj"][k, b])              # the difference of the arm's last check
        assert out["closest"][b] > 1e-4
    assert out["arrived"][0] == 11 and out["arrived"][1] == 39                           # 0.92^12 < 0.01 / 0.02, 0.92^40 < 0.01 / 0.25
    # the gated arm: never runs, never arrives, not counted; its rows carry its start and its diff is never written
    assert out["arrived"][2] == -1 and np.all(out["q_traj"][:, 2] == q0[2]) and np.all(out["diff"][2] == 0)
    # the reference beyond the limit: joint 0 converges to the limit, 0.1 rad short of what the caller sent
    assert out["arrived"][3] == -1
    assert abs(out["q"][3, 0] - chain.q_hi[0]) < 1e-3 and abs(out["diff"][3, 0] - 0.1) < 1e-3
    assert np.abs(out["diff"][3, 1:]).max() == 0.0
    for k in range(n_checks):
        cyc = (k + 1) * STRIDE - 1
        assert out["pending"][k] == sum(1 for b in (0, 1, 3) if out["arrived"][b] < 0 or out["arrived"][b] > cyc)


def test_reference_posture_list(pure_p):
    """Three postures 0.1 rad apart, via precision 3 x: one advance per check at most, the last posture under the tight precision; a
    one-row list; an arm without a list is kept out.  W = 1 is the goto."""
    import timed_reference as tr
    from oracle import oracle_c
    from vfclik_amd import _abi, robots, synth
    chain, q0, ref, out = pure_p
    w = synth.make_workload(chain, 3, 2, seed=53, io_dtype=np.float64)
    step = 0.1 * np.array([1, -1, 1, 1, -1, 1, -1.0])
    wayq = np.stack([ref[:3] + i * step for i in range(3)], axis=1)
    wayq[1, 1:] = np.nan
    wayq[2] = np.nan
    params = _abi.default_params(flags=_abi.F_MIXER, mix_w=[0, 0, 1, 0, 0, 0], jp_kp=KP)
    f = tr.follow_js(oracle_c, chain, params, q0[:3], w["fields"], w["nfields"], wayq, 160, STRIDE, DT, PREC, via_prec=3 * PREC,
                               hold=True)
    assert list(f["length"]) == [3, 1, 0] and list(f["next"]) == [3, 1, 0]
    r = f["reached"][0]
    assert np.all(np.diff(r) > 0) and np.all(r % STRIDE == STRIDE - 1)
    # posture 0 under 3 x precision: 0.92^c <= 0.03 / 0.02 holds at the first check; posture 1 from e = 0.1 + what was left
    assert r[0] == STRIDE - 1
    for wi, cyc in enumerate(r):
        k = (cyc + 1) // STRIDE - 1
        assert f["way_traj"][k, 0] == wi
        assert tr.rule(wayq[:1, wi], f["q_traj"][k, :1], PREC if wi == 2 else 3 * PREC).all()
    assert f["reached"][1, 0] == out["arrived"][1] and np.all(f["reached"][1, 1:] == -1)
    assert np.all(f["reached"][2] == -1) and np.all(f["q_traj"][:, 2] == q0[2]) and np.all(f["way_traj"][:, 2] == -1)
    assert f["pending"][0] == 2 and f["pending"][-1] == 0
    g = tr.goto_js(oracle_c, chain, params, q0[:2], w["fields"][:2], w["nfields"][:2], ref[:2], N_CYCLES, STRIDE, DT, PREC, hold=True)
    f1 = tr.follow_js(oracle_c, chain, params, q0[:2], w["fields"][:2], w["nfields"][:2], ref[:2, None, :], N_CYCLES, STRIDE, DT,
                                PREC, hold=True)
    assert np.array_equal(g["arrived"], f1["reached"][:, 0]) and np.array_equal(g["q_traj"], f1["q_traj"]) and np.array_equal(g["diff"], f1["diff"])
