"""The distance monitor's edge scenes (tests/hp_observers.py) on the CPU: every scene's construction conditions and the finite-only cap from
the 50-digit reference alone, and the double-precision restatement of the monitor's form held to the derived bar -- before any GPU number is
looked at (tests/test_gpu_observer_edges.py)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hp_observers as ho  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _tables():
    """(the CPU rows of profiles/backend_observer_accuracy.txt, when VFIK_BACKEND_TABLE names a file: written once every test of the file ran)"""
    yield
    path = os.environ.get("VFIK_BACKEND_TABLE")
    if path:
        ho.write_table(path)
        ho.write_track_table(path)


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["f32", "f64"])
def test_monitor_scene_and_the_double_restatement(dt):
    pose, frames, kk = ho.monitor_scene(dt)
    assert np.array_equal(pose, pose.astype(dt).astype(np.float64)) and np.array_equal(frames, frames.astype(dt).astype(np.float64))
    ref = ho.reference(("monitor", dt), pose, frames)
    bad = ho.scene_conditions(dt, kk, ref) + ho.caps(kk, ref)
    assert not bad, "\n".join(bad[:10])
    got = ho.monitor_double(pose, frames)
    if dt == np.float32:
        got = got.astype(np.float32)
    rD, rA = ho.ratios(got, ref, dt)
    print("monitor f%d double restatement: worst error / bar  D %.3f  angle %.3f" % (32 if dt == np.float32 else 64, rD.max(), rA.max()))
    assert rD.max() < 1.0 and rA.max() < 1.0, (rD.max(), rA.max(), np.argwhere(rA >= 1.0)[:5])
    ho.note("cpu", "monitor f%d" % (32 if dt == np.float32 else 64), "numpy double", rD, rA, ref)
    # the restatement that floors the angle (vfik_numpy.rot_log returns 0 below |a| = 1e-12) is NOT the monitor's statement: the kernel publishes
    # atan2 as it is, and the 1e-13 kind sits below that floor
    small = [b for b, k in enumerate(kk) if k == "1e-13"]
    if dt == np.float64:
        assert np.all(ref["ang"][small] > 0.0) and np.all(got[small, :, 1] > 0.0)


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["f32", "f64"])
def test_tracking_scene_and_the_numpy_restatement(dt):
    """The tracking-error scenes' own conditions and the caps (finite-only arms, arms inside the decision's band) from the 50-digit reference
    alone; then vfik_numpy.TrackingError, stepped over every arm's whole history, meets the derived bar."""
    poses, v6, active, kk = ho.track_scene(dt)
    for a in (poses, v6):
        assert np.array_equal(a, a.astype(dt).astype(np.float64))
    ref = ho.track_reference(("track", dt), poses, v6, active)
    bad = ho.track_conditions(dt, kk, ref, v6) + ho.track_caps(kk, ref)
    assert not bad, "\n".join(bad[:10])
    got = ho.numpy_tracking(poses, v6, active)
    if dt == np.float32:
        got = got.astype(np.float32)
    ratio, wrong, amb = ho.track_ratios(got, ref, dt, active)
    print("tracking f%d numpy restatement: worst error / bar per output %s" % (32 if dt == np.float32 else 64, np.round(ratio.max(axis=(0, 1)), 3)))
    assert ratio.max() < 1.0, np.argwhere(ratio >= 1.0)[:8]
    assert not wrong.any(), np.argwhere(wrong)[:8]
    ho.note_track("cpu", "tracking f%d" % (32 if dt == np.float32 else 64), "vfik_numpy", ratio, amb, ref)


@pytest.mark.parametrize("robot", ho.GOAL_ROBOTS)
@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["f32", "f64"])
def test_goal_scene_and_the_double_restatement(oracle_c, dt, robot):
    """The goal-distance scenes' conditions and the finite-only cap from the 50-digit reference (its own forward kinematics); then the G R^T form
    in doubles on the oracle's pose meets the derived bar."""
    for tname in (None, "turned"):
        chain, params, w, kk, di, tool16 = ho.goal_scene(oracle_c, robot, dt, tname)
        goals = w["fields"]["p"][:, 0, :16]
        ref = ho.goal_reference((robot, dt, tname), chain, w["q"], goals, tool16)
        bad = ho.goal_conditions(dt, kk, di, ref) + ho.caps(kk, ref)
        assert not bad, "\n".join(bad[:10])
        pose = oracle_c.cycle_batch(chain, params, w["q"], w["fields"], w["nfields"], tool=tool16, want=("pose",))["pose"]
        got = ho.goal_double(pose, goals)
        rD, rA = ho.ratios(got.astype(dt), ref, dt)
        print("goal %s f%d tool %s: worst error / bar  D %.3f  angle %.3f" % (robot, 32 if dt == np.float32 else 64, tname, rD.max(), rA.max()))
        assert rD.max() < 1.0 and rA.max() < 1.0, (np.argwhere(rD >= 1)[:5], np.argwhere(rA >= 1)[:5])
        ho.note("cpu", "goal %s f%d%s" % (robot, 32 if dt == np.float32 else 64, " tool" if tname else ""), "oracle pose", rD, rA, ref)


@pytest.mark.parametrize("robot", ho.GOAL_ROBOTS)
@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["f32", "f64"])
def test_arrival_scene_and_the_oracle_stepped_reference(oracle_c, dt, robot):
    """Goals at threshold (1 +- {1e-9, 1e-6, 1e-3}): the scene's conditions and the 5 % cap from the 50-digit reference, then the suite's
    oracle-stepped goto (tests/timed_reference.py) decides every arm outside the band as the reference's rule does."""
    import timed_reference as tr
    chain, params, w, kk = ho.arrive_scene(oracle_c, robot, dt)
    ref = ho.goal_reference((robot, dt, "arrive"), chain, w["q"], w["fields"]["p"][:, 0, :16])
    bad = ho.arrive_conditions(dt, kk, ref)
    assert not bad, "\n".join(bad[:10])
    arr, amb = ho.arrive_rule(ref, dt)
    got = tr.goto(oracle_c, chain, params, w["q"], w["fields"], w["nfields"], 1, 1, 1e-3, ho.ARRIVE_PREC, io_dtype=dt)
    mine = got["reached"][:, 0] >= 0
    assert np.array_equal(mine[~amb], arr[~amb]), np.flatnonzero((mine != arr) & ~amb)[:10]
    assert 0.2 * len(kk) < arr.sum() < 0.8 * len(kk)
    ho.note_track("cpu", "arrival %s f%d" % (robot, 32 if dt == np.float32 else 64), "oracle-stepped", np.array([[[float(((mine != arr) & ~amb).sum())]]]),
                  amb[None, :], {"finite_only": np.zeros((1, len(kk), 1), dtype=bool)})


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["f32", "f64"])
def test_the_numpy_monitor_with_its_floor(dt):
    """vfik_numpy.object_distances on the monitor's edge scene.  It words the relative rotation as G R^T and returns NO rotation below
    |a| = 1e-12 (rot_log), so it is held to the 50-digit reference of ITS wording, with one allowance: a pair whose reference angle is at or below
    1e-12 rad may come out as 0 -- an error of up to 1e-12 rad, 1e4 bars, which is the floor's and not the arithmetic's.  The kernel has no such
    floor (tests/test_gpu_observer_edges.py holds it to atan2 as it is).  The two wordings' references differ for frames that are no
    rotations: the figure is printed and bounded by what rounding to the I/O type can do."""
    pose, frames, kk = ho.monitor_scene(dt)
    ref = ho.reference_grt(("monitor", dt), pose, frames)
    assert not ho.caps(kk, ref)
    got = ho.numpy_monitor(pose, frames)
    if dt == np.float32:
        got = got.astype(np.float32)
    rD, rA = ho.ratios(got, ref, dt)
    fl = ho.floored(ref)
    used = fl & (rA >= 1.0)
    assert np.all(got[used][:, 1] == 0.0)                      # the allowance is the floor's value, nothing else
    rA = np.where(used, 0.0, rA)
    print("numpy monitor f%d: worst error / bar  D %.3f  angle %.3f; %d pairs on the floor's allowance" % (32 if dt == np.float32 else 64, rD.max(), rA.max(), used.sum()))
    assert rD.max() < 1.0 and rA.max() < 1.0, (np.argwhere(rD >= 1)[:5], np.argwhere(rA >= 1)[:5])
    small = np.array([k in ("same", "1e-13") for k in kk])
    assert not used[~small].any()                               # only identical frames and the 1e-13 kind sit below the floor
    if dt == np.float64:
        assert used[[b for b, k in enumerate(kk) if k == "1e-13"]].all()
    ho.note("cpu", "monitor f%d (G R^T, floor)" % (32 if dt == np.float32 else 64), "vfik_numpy", rD, rA, ref)
    own = ho.reference(("monitor", dt), pose, frames)
    diff = np.abs((ref["ang"] - own["ang"]) + (ref["ang_lo"] - own["ang_lo"])) * (np.pi / 180.0)
    print("  the two wordings' references differ by up to %.2e rad" % diff.max())
    assert diff.max() < (1e-14 if dt == np.float64 else 1e-6) and (dt == np.float64 or diff.max() > 1e-9)
