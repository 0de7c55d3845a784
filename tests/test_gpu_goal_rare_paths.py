"""The goal attractor's rare paths (vfik_kernel.hip: rot_axis_angle) against the oracle.

The rotation angle theta between tool and goal is only evaluated by a wave with a lane inside the rotational slow-down
angle (cos theta > cos rot_slowdown), and the half-turn neighbourhood (sin theta < 1e-4, cos theta < 0) takes its axis from
the symmetric part of G R^T under a second wave-uniform test.  With rot_slowdown below pi/8 the first path is a short
arctangent without atan2_pos's reductions, and the half-turn block a two-term series.  A batch of random goals puts a
few arms in a thousand on these paths; here every wave is built for them: the goals are the ORACLE'S OWN tool pose turned by a
chosen angle about a random axis, so that the arms sit

  * just inside and just outside the slow-down angle, and deep inside it,
  * at a half turn -+ 1e-6,
  * at a half turn in a wave (and in an eight-lane group of the small-batch kernel) that also has a slow-down lane,

with rot_slowdown 0.3 (the default: the short path), 0.5 (> pi/8: atan2_pos with its reductions) and with goal_dist requested
(the angle is published: atan2_pos whatever its size).  The CPU-only test asserts from the oracle's poses that every lane
meets the branch condition it was built for, and the GPU tests assert that every launch ran on the straight-line field path
(the only one whose kernels carry the short arctangent), by the handle's field path and the names of the kernels launched.
Bars: the suite's (tests/test_gpu_parity.py) -- 1e-9 at float64 I/O, 1e-6 at float32 I/O.  goal_dist's angle is published in
DEGREES: at float32 I/O a value near 180 has an ulp of 1.5e-5, so no float32 output can hold it to 1e-6; the bar there is
1e-5 degrees (half an ulp is 7.6e-6), which is 1.7e-7 rad -- tighter than 1e-6 in the unit the other outputs are held in."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_variants as kv  # noqa: E402

TOL64 = 1e-9
TOL32 = 1e-6
TAN_PI_8 = math.tan(math.pi / 8)

# lane kinds, one per arm: 8 consecutive arms (one group of the eight-lanes kernel) repeat the pattern of their wave's type
FAR, INSIDE, DEEP, OUTSIDE, HALF_LO, HALF_HI = range(6)
WAVE_TYPES = (
    (FAR,) * 8,                                                            # the main line: no lane on either path
    (INSIDE, FAR, OUTSIDE, DEEP, FAR, INSIDE, OUTSIDE, FAR),               # slow-down path alone
    (HALF_LO, FAR, HALF_HI, FAR, FAR, HALF_LO, FAR, HALF_HI),              # half-turn path alone
    (HALF_LO, INSIDE, HALF_HI, OUTSIDE, DEEP, FAR, HALF_LO, INSIDE),       # both in one wave and in one group of eight
)
ROBOTS = {6: "powercube6", 7: "lwr", 14: "lwr_dual14"}


def _rodrigues(u, th):
    K = np.array([[0.0, -u[2], u[1]], [u[2], 0.0, -u[0]], [-u[1], u[0], 0.0]])
    return np.eye(3) + math.sin(th) * K + (1.0 - math.cos(th)) * (K @ K)


def _angle_of(kind, rot_slow, rng):
    if kind == FAR:
        return rng.uniform(rot_slow + 0.3, 2.8)
    if kind == INSIDE:
        return rot_slow - 1e-3
    if kind == DEEP:
        return rng.uniform(1e-3, 0.5 * rot_slow)
    if kind == OUTSIDE:
        return rot_slow + 1e-3
    return math.pi - 1e-6 if kind == HALF_LO else math.pi + 1e-6


def _scene(oc, nj, io_dtype, rot_slow, B=1024, seed=7):
    """Workload of B arms whose goal frames are the oracle's tool pose turned by the angle of the lane's kind; returns
    (chain, params, w, kinds, sin, cos) -- sin / cos of the goal rotation as both sides will see it (inputs rounded to io_dtype)."""
    from vfclik_amd import _abi, robots, synth
    chain = robots.by_name(ROBOTS[nj])
    params = _abi.default_params(rot_slowdown=rot_slow)
    w = synth.make_workload(chain, B, 2, seed=seed, io_dtype=io_dtype)
    pose = oc.cycle_batch(chain, params, w["q"], w["fields"], w["nfields"], want=("pose",))["pose"].reshape(B, 4, 4)
    rng = np.random.default_rng(seed + 1)
    kinds = np.array([WAVE_TYPES[(b // 64) % len(WAVE_TYPES)][b % 8] for b in range(B)])
    for b in range(B):
        u = rng.normal(size=3)
        u /= np.linalg.norm(u)
        G = np.eye(4)
        G[:3, :3] = _rodrigues(u, _angle_of(kinds[b], rot_slow, rng)) @ pose[b, :3, :3]
        G[:3, 3] = pose[b, :3, 3] + rng.uniform(-0.3, 0.3, 3)
        w["fields"]["p"][b, 0, :16] = G.reshape(16).astype(io_dtype).astype(np.float64)
    Gr = w["fields"]["p"][:, 0, :16].reshape(B, 4, 4)[:, :3, :3]
    E = Gr @ np.transpose(pose[:, :3, :3], (0, 2, 1))
    anti = 0.5 * np.stack([E[:, 2, 1] - E[:, 1, 2], E[:, 0, 2] - E[:, 2, 0], E[:, 1, 0] - E[:, 0, 1]], 1)
    return chain, params, w, kinds, np.linalg.norm(anti, axis=1), 0.5 * (np.trace(E, axis1=1, axis2=2) - 1.0)


@pytest.mark.parametrize("nj", [6, 7, 14])
@pytest.mark.parametrize("io_dtype", [np.float32, np.float64])
@pytest.mark.parametrize("rot_slow", [0.3, 0.5])
def test_every_constructed_lane_meets_its_branch_condition(oracle_c, nj, io_dtype, rot_slow):
    _, _, _, kinds, s, c = _scene(oracle_c, nj, io_dtype, rot_slow)
    cos_slow = math.cos(rot_slow)
    inside = (kinds == INSIDE) | (kinds == DEEP)
    half = (kinds == HALF_LO) | (kinds == HALF_HI)
    for k in range(6):
        assert (kinds == k).sum() >= 32
    assert np.all(c[inside] > cos_slow) and np.all(s[inside] >= 1e-4)            # the slow-down path, not the half-turn one
    assert np.all(c[kinds == OUTSIDE] < cos_slow) and np.all(c[kinds == OUTSIDE] > cos_slow - 1e-3)
    assert np.all(c[kinds == FAR] < cos_slow) and not np.any((s[kinds == FAR] < 1e-4) & (c[kinds == FAR] < 0.0))
    assert np.all(s[half] < 1e-4) and np.all(c[half] < 0.0) and np.all(s[half] > 5e-7)   # (sin ~ 1e-6: the axis' sign is well defined)
    t = s[inside] / c[inside]
    if rot_slow < math.pi / 8:   # the short arctangent: neither reduction of atan2_pos could fire
        assert t.max() < TAN_PI_8 and t.max() > 0.3
    else:                        # ... and the full one does reduce: the arguments straddle tan(pi/8)
        assert t.max() > TAN_PI_8 and t.min() < TAN_PI_8
    # per wave and per group of eight: the paths the wave's type was built for, and no other
    wave_any = lambda m: m.reshape(-1, 64).any(axis=1)
    group_any = lambda m: m.reshape(-1, 8).any(axis=1)
    wt = np.arange(len(wave_any(inside))) % len(WAVE_TYPES)
    assert np.array_equal(wave_any(c > cos_slow), (wt == 1) | (wt == 3))
    assert np.array_equal(wave_any((s < 1e-4) & (c < 0.0)), (wt == 2) | (wt == 3))
    gt = np.repeat(wt, 8)
    assert np.array_equal(group_any(c > cos_slow), (gt == 1) | (gt == 3))
    assert np.array_equal(group_any((s < 1e-4) & (c < 0.0)), (gt == 2) | (gt == 3))


def _engine_env():
    import __graft_entry__ as g
    g.build()
    from oracle import oracle_c as oc
    from vfclik_amd import engine
    oc.build()
    return oc, engine


def _assert_straight_line(names, nj, sub8):
    """The launch's kernels: the eight-lanes kernel, or a cycle kernel whose sixth template argument (FASTF, the straight-line field
    path: `<io type, joints, nullspace, PLAIN, rollout, FASTF, ...>`) is true."""
    assert names, "no kernel recorded"
    for name in names:
        v = kv.parse(name)
        assert v.args["NJ"] == nj, name
        if sub8:
            assert v.kernel.startswith("cycle_sub8_kernel"), name
        else:
            assert v.kernel in ("cycle_kernel_s", "cycle_kernel_x") and v.args["FASTF"] is True, name


@pytest.mark.gpu
@pytest.mark.parametrize("nj", [6, 7, 14])
@pytest.mark.parametrize("io_dtype,tol", [(np.float32, TOL32), (np.float64, TOL64)])
@pytest.mark.parametrize("rot_slow", [0.3, 0.5])
def test_rare_goal_paths_against_the_oracle(nj, io_dtype, tol, rot_slow):
    """qdot_out alone (the lean kernels; chains of up to 8 joints also on eight lanes per arm) and with the published rows."""
    oc, engine = _engine_env()
    chain, params, w, kinds, _, _ = _scene(oc, nj, io_dtype, rot_slow)
    B = len(kinds)
    ref = oc.cycle_batch(chain, params, w["q"], w["fields"], w["nfields"], want=("qdot_out", "qdot_vf", "pose", "status"))
    assert np.abs(ref["qdot_out"]).max() > 0.1
    runs = [(0, ("qdot_out", "status")), (0, ("qdot_out", "qdot_vf", "pose", "status"))]
    if nj <= 8:
        runs.append((4096, ("qdot_out", "status")))
    for small, want in runs:
        eng = engine.Engine(chain, B, io_dtype=io_dtype, max_slots=4, params=params)
        eng.set_small_batch_kernel(small)
        eng.set_fields(w["fields"], w["nfields"])
        assert eng.field_path == 1                    # goal + decay repellers of one order: the straight-line path
        eng.launched_kernels()                        # (clears the record)
        got = eng.step_host(w["q"], want=want)
        assert eng.small_batch_launches == (1 if small else 0)
        _assert_straight_line(eng.launched_kernels(), nj, bool(small))
        eng.close()
        assert np.array_equal(got["status"], ref["status"])
        for k in want[:-1]:
            err = np.abs(got[k].astype(np.float64) - ref[k]).max(axis=1)
            print("nj %d %s rot_slow %.1f small %d %-8s max err %.3e (kind of the worst arm: %d)"
                  % (nj, np.dtype(io_dtype).name, rot_slow, small, k, err.max(), kinds[int(np.argmax(err))]))
            assert np.all(np.isfinite(got[k])) and err.max() < tol, (k, small, err.max(), int(np.argmax(err)))


@pytest.mark.gpu
@pytest.mark.parametrize("nj", [6, 7, 14])
@pytest.mark.parametrize("io_dtype,tol,tol_deg", [(np.float32, TOL32, 1e-5), (np.float64, TOL64, 1e-9)])
def test_rare_goal_paths_with_goal_dist_requested(nj, io_dtype, tol, tol_deg):
    """goal_dist publishes the angle: every wave evaluates it in full, the half-turn lanes through the series."""
    from oracle import vfik_numpy as vn
    oc, engine = _engine_env()
    chain, params, w, kinds, _, _ = _scene(oc, nj, io_dtype, 0.3)
    B = len(kinds)
    ref = oc.cycle_batch(chain, params, w["q"], w["fields"], w["nfields"], want=("qdot_out", "pose", "status"))
    eng = engine.Engine(chain, B, io_dtype=io_dtype, max_slots=4, params=params)
    eng.set_small_batch_kernel(0)
    eng.set_fields(w["fields"], w["nfields"])
    assert eng.field_path == 1
    eng.launched_kernels()
    got = eng.step_host(w["q"], want=("qdot_out", "goal_dist", "status"))
    _assert_straight_line(eng.launched_kernels(), nj, False)
    eng.close()
    assert np.array_equal(got["status"], ref["status"])
    err = np.abs(got["qdot_out"].astype(np.float64) - ref["qdot_out"]).max()
    gd = np.array([vn.goal_distance(ref["pose"][b], w["fields"]["p"][b, 0, :16]) for b in range(B)])
    ed = np.abs(got["goal_dist"].astype(np.float64) - gd).max(axis=0)
    print("nj %d %s goal_dist: qdot_out err %.3e, distance err %.3e, angle err %.3e deg" % (nj, np.dtype(io_dtype).name, err, ed[0], ed[1]))
    assert err < tol
    assert ed[0] < tol and ed[1] < tol_deg
    half = (kinds == HALF_LO) | (kinds == HALF_HI)
    assert np.all(np.abs(gd[half, 1] - 180.0) < 1e-4) and np.all(gd[kinds == INSIDE, 1] < 0.3 * 180.0 / math.pi)
