"""CPU-side checks of the waypoint lists (include/vfik.h: vfik_follow): the options struct and its ctypes mirror, the ABI version, the
exported symbols, and the oracle restatement (tests/timed_reference.py: follow) on a hand-made case of three arms."""
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


def test_follow_opts_size_matches_the_mirror(lib):
    from vfclik_amd import _abi
    lib.vfik_follow_opts_size.restype = ctypes.c_size_t
    assert lib.vfik_follow_opts_size() == ctypes.sizeof(_abi.FollowOpts) == 4 + 4 + 8 + 4 + 4 + 4 * 8 + 4 + 4 + 8 * 8
    o = _abi.FollowOpts
    assert (o.n_cycles.offset, o.stride.offset, o.dt.offset, o.clamp_to_limits.offset, o.hold.offset) == (0, 4, 8, 16, 20)
    assert (o.pos_prec.offset, o.rot_prec.offset, o.via_pos_prec.offset, o.via_rot_prec.offset, o.n_way.offset) == (24, 32, 40, 48, 56)
    assert (o.way16.offset, o.reached.offset, o.next.offset, o.pending.offset) == (64, 72, 80, 88)
    assert (o.q_out.offset, o.q_traj.offset, o.dist_traj.offset, o.way_traj.offset) == (96, 104, 112, 120)


def test_abi_version_and_sizes_stay(lib):
    from vfclik_amd import _abi, engine
    assert lib.vfik_abi_version() == 6 == _abi.ABI_VERSION
    sizes = (ctypes.c_size_t * 4)()
    lib.vfik_struct_sizes(sizes)
    assert list(sizes) == [ctypes.sizeof(_abi.Field), ctypes.sizeof(_abi.Chain), ctypes.sizeof(_abi.Params), ctypes.sizeof(engine.IO)]
    assert list(sizes) == [152, 1960, 304, 19 * 8]   # as before this entry point
    assert lib.vfik_goto_opts_size() == 80 and lib.vfik_scene_move_size() == 64


def test_follow_symbols_are_declared_and_exported(lib):
    hdr = open(os.path.join(ROOT, "include", "vfik.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    raw = ctypes.CDLL(os.path.join(ROOT, "vfclik_amd", "csrc", "libvfik_hip.so"))
    for name in ("vfik_follow_opts_size", "vfik_follow", "vfik_follow_host"):
        assert re.search(r"\b%s\s*\(" % name, code), name + " is not declared in include/vfik.h"
        assert hasattr(raw, name), "libvfik_hip.so does not export " + name
    assert "typedef struct vfik_follow_opts" in code and "handlers.py:346-387" in hdr


STRIDE, N_CYCLES, PREC = 4, 160, (0.01, 0.05)


@pytest.fixture(scope="module")
def three_arms(lib):
    """lwr, nullspace + joint-limit task, three waypoints 0.1 rad apart in joint space: arm 0 starts 0.03 rad from its first waypoint's
    configuration, arm 1 is gated off by the caller, arm 2 has a one-row path (rows 1 and 2 start with NaN).  160 cycles of 10 ms,
    checks every 4, precision (0.01 m, 0.05 rad) at every waypoint, hold on."""
    import timed_reference as tr
    from oracle import oracle_c
    from vfclik_amd import _abi
    chain, w, qg, way, q0, params = tr.three_lwr_arms(_abi.F_NULLSPACE | _abi.F_JOINT_LIMIT_TASK)
    way[2, 1:] = np.nan
    start = np.array(w["fields"], copy=True)
    ref = tr.follow(oracle_c, chain, params, q0, w["fields"], w["nfields"], way, N_CYCLES, STRIDE, 0.01, PREC, hold=True, clamp=True,
                    active=[1, 0, 1], want=("qdot_out", "pose"))
    assert np.array_equal(start["p"], w["fields"]["p"])   # the caller's field array is not the mutable one
    return q0, way, ref, w


def test_reference_path_lengths():
    import timed_reference as tr
    way = np.zeros((5, 3, 16))
    way[1, 2, 0] = way[2, 1, 0] = way[3, 0, 0] = np.nan
    way[4, 1, 0] = way[4, 2, 5] = np.nan    # a NaN elsewhere in a row does not end a path; rows behind the first NaN row do not count
    way[3, 2, 0] = 1.0
    assert list(tr.list_lengths(way)) == [3, 2, 1, 0, 1]


def test_reference_rule_on_three_arms(three_arms):
    q0, way, ref, w = three_arms
    r, nx = ref["reached"], ref["next"]
    thr = np.array([PREC[0], PREC[1] * 180.0 / np.pi])
    assert list(ref["length"]) == [3, 3, 1]
    assert list(nx) == [3, 0, 1] and np.all(r[1] == -1) and np.all(r[2, 1:] == -1)   # the near arm goes all the way, the gated one nowhere
    for b in (0, 2):
        got = r[b, : nx[b]]
        assert np.all(np.diff(got) > 0)                       # strictly ascending along the path: one waypoint per check at most
        assert np.all(got % STRIDE == STRIDE - 1)             # each entry a check's cycle, (k + 1) * stride - 1
        for wi, cyc in enumerate(got):
            k = (cyc + 1) // STRIDE - 1
            assert ref["way_traj"][k, b] == wi                # measured against this waypoint ...
            assert np.all(ref["dist_traj"][k, b] < thr)       # ... under both thresholds at its check ...
            first = wi == 0 and k == 0
            if not first:                                     # ... and not at the one before (which, for wi > 0, may have measured wi - 1)
                assert ref["way_traj"][k - 1, b] != wi or not np.all(ref["dist_traj"][k - 1, b] < thr)
    # pending: the arms that take part and are not at their last waypoint
    for k in range(N_CYCLES // STRIDE):
        cyc = (k + 1) * STRIDE - 1
        assert ref["pending"][k] == sum(1 for b in (0, 2) if r[b, ref["length"][b] - 1] < 0 or r[b, ref["length"][b] - 1] > cyc)
    assert np.all(ref["q_traj"][:, 1] == q0[1]) and np.all(np.isnan(ref["dist_traj"][:, 1])) and np.all(ref["way_traj"][:, 1] == -1)
    # hold: rows repeat from the check of the last waypoint on
    for b in (0, 2):
        k = (r[b, nx[b] - 1] + 1) // STRIDE - 1
        assert np.all(ref["q_traj"][k:, b] == ref["q_traj"][k, b]) and np.all(ref["way_traj"][k:, b] == nx[b] - 1)
    # the goal afterwards: waypoint min(next, L - 1) for arms that took part, untouched for the gated one
    p = ref["fields"]["p"]
    assert np.array_equal(p[0, 0, :12], way[0, 2, :12]) and np.array_equal(p[2, 0, :12], way[2, 0, :12])
    assert np.array_equal(p[1], w["fields"]["p"][1]) and np.array_equal(p[:, 0, 12:], w["fields"]["p"][:, 0, 12:])
