"""CPU-side checks of the batched goto (include/vfik.h: vfik_goto): the options struct and its ctypes mirror, the ABI version, the
exported symbols, and the oracle restatement (tests/timed_reference.py: goto) on a hand-made case of three arms."""
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


def test_goto_opts_size_matches_the_mirror(lib):
    from vfclik_amd import _abi
    lib.vfik_goto_opts_size.restype = ctypes.c_size_t
    assert lib.vfik_goto_opts_size() == ctypes.sizeof(_abi.GotoOpts) == 4 + 4 + 8 + 4 + 4 + 8 + 8 + 5 * 8
    o = _abi.GotoOpts
    assert (o.n_cycles.offset, o.stride.offset, o.dt.offset, o.clamp_to_limits.offset, o.hold.offset) == (0, 4, 8, 16, 20)
    assert (o.pos_prec.offset, o.rot_prec.offset, o.arrived.offset, o.pending.offset) == (24, 32, 40, 48)
    assert (o.q_out.offset, o.q_traj.offset, o.dist_traj.offset) == (56, 64, 72)


def test_abi_version_and_sizes_stay(lib):
    from vfclik_amd import _abi, engine
    assert lib.vfik_abi_version() == 6 == _abi.ABI_VERSION
    sizes = (ctypes.c_size_t * 4)()
    lib.vfik_struct_sizes(sizes)
    assert list(sizes) == [ctypes.sizeof(_abi.Field), ctypes.sizeof(_abi.Chain), ctypes.sizeof(_abi.Params), ctypes.sizeof(engine.IO)]


def test_goto_symbols_are_declared_and_exported(lib):
    hdr = open(os.path.join(ROOT, "include", "vfik.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    raw = ctypes.CDLL(os.path.join(ROOT, "vfclik_amd", "csrc", "libvfik_hip.so"))
    for name in ("vfik_goto_opts_size", "vfik_goto", "vfik_goto_host"):
        assert re.search(r"\b%s\s*\(" % name, code), name + " is not declared in include/vfik.h"
        assert hasattr(raw, name), "libvfik_hip.so does not export " + name
    assert "typedef struct vfik_goto_opts" in code and "handlers.py:346-440" in hdr


@pytest.fixture(scope="module")
def three_arms(lib):
    """lwr, nullspace + joint-limit task: arm 0 starts 0.03 rad from its goal configuration, arm 1 is gated off by the caller, arm 2
    starts 0.2 rad away.  40 cycles of 10 ms, checks every 4, precision (0.01 m, 0.05 rad), once with hold and once without."""
    import timed_reference as tr
    from oracle import oracle_c
    from vfclik_amd import _abi
    chain, w, qg, way, q0, params = tr.three_lwr_arms(_abi.F_NULLSPACE | _abi.F_JOINT_LIMIT_TASK)
    w["fields"]["p"][:, 0, :16] = way[:, 0]
    q0[2] = qg[2, 0] + 0.2 * np.array([1, -1, 1, -1, 1, -1, 1.0])
    kw = dict(n_cycles=40, stride=4, dt=0.01, precision=(0.01, 0.05), clamp=True, active=[1, 0, 1], want=("qdot_out", "pose"))
    held = tr.goto(oracle_c, chain, params, q0, w["fields"], w["nfields"], hold=True, **kw)
    free = tr.goto(oracle_c, chain, params, q0, w["fields"], w["nfields"], hold=False, **kw)
    return q0, held, free, chain, w, params


def test_reference_arrival_rule_on_three_arms(three_arms):
    import timed_reference as tr
    q0, held, free, chain, w, params = three_arms
    for r in (held, free):
        a = r["arrived"]
        assert a[1] == -1 and a[0] >= 0 and (a[2] == -1 or a[2] > a[0])   # the near arm first, the gated one never
        assert a[0] % 4 == 3                                              # a check's cycle: (k + 1) * stride - 1
        k0 = (a[0] + 1) // 4 - 1
        thr = np.array([0.01, 0.05 * 180.0 / np.pi])
        assert np.all(r["dist_traj"][k0, 0] < thr)                        # under both thresholds at its check ...
        assert k0 == 0 or not np.all(r["dist_traj"][k0 - 1, 0] < thr)     # ... and at none before
        # the distances are those of the pose of the block's last cycle against the goal frame
        goal = tr.goal_frames(w["fields"], w["nfields"])
        assert np.allclose(goal, w["fields"]["p"][:, 0, :16])
        # pending: the arms the caller lets run that have not arrived yet
        for k in range(10):
            cyc = (k + 1) * 4 - 1
            assert r["pending"][k] == sum(1 for b in (0, 2) if a[b] < 0 or a[b] > cyc)
        assert np.all(r["q_traj"][:, 1] == q0[1])                         # the gated arm's rows carry its start
        assert np.all(np.isnan(r["dist_traj"][:, 1]))                     # ... and nothing was ever measured for it
        assert r["q"] is not r["q_traj"] and np.array_equal(r["q"], r["q_traj"][-1])


def test_reference_hold_freezes_an_arrived_arm(three_arms):
    q0, held, free, chain, w, params = three_arms
    assert np.array_equal(held["arrived"], free["arrived"]) or held["arrived"][2] != free["arrived"][2]   # arm 0 and 1 never differ
    assert held["arrived"][0] == free["arrived"][0]
    k0 = (held["arrived"][0] + 1) // 4 - 1
    assert k0 < 9
    assert np.all(held["q_traj"][k0:, 0] == held["q_traj"][k0, 0])        # with hold the rows repeat, bit for bit
    assert np.all(held["dist_traj"][k0:, 0] == held["dist_traj"][k0, 0])
    assert np.any(free["q_traj"][k0 + 1:, 0] != free["q_traj"][k0, 0])    # without it the arm keeps tracking
    assert np.array_equal(held["q_traj"][: k0 + 1], free["q_traj"][: k0 + 1])
    # the held arm's output rows are those of its last evaluated cycle: the pose whose distance passed the check
    import timed_reference as tr
    d = tr.goal_distance(held["pose"][:1], w["fields"]["p"][:1, 0, :16])
    assert np.array_equal(d[0], held["dist_traj"][k0, 0])
