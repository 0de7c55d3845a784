#!/usr/bin/env python
"""Writes tests/golden/timed_reference.npz: what tests/timed_reference.py gives on the small cases of the host tests -- three lwr arms, at
most 240 cycles at stride 4, one case per timed move and one with a stall rule, each in float64 and float32 I/O.  The numbers are those of
the five helper modules of commit REV (goto_reference.py, follow_reference.py, goto_js_reference.py, script_reference.py,
stall_reference.py), which tests/timed_reference.py replaced after it had been shown to give their every array bit for bit
(profiles/timed_reference_refactor.txt).  tests/test_timed_reference.py holds the module to the fixture: integers exactly, float rows to
the tolerance the GPU is held to on the same rows.

    python tests/golden/make_timed_reference.py        (needs the built oracle; no GPU)

Exact integers are safe only away from the thresholds: a case in which any arm's decision came within MARGIN of its threshold is refused.
The inputs are not stored: CASES rebuilds them from tests/timed_reference.py:three_lwr_arms, for this script and for the test alike."""
import os
import sys

import numpy as np

REV = "5e07c96"
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
FIXTURE = os.path.join(ROOT, "tests", "golden", "timed_reference.npz")
INTS = ("arrived", "reached", "next", "length", "pending", "way_traj", "stalled")
FLOATS = ("q_traj", "dist_traj", "diff")
CLOSEST = ("closest", "closest_c", "closest_j", "closest_s", "closest_sj")
MARGIN = {"float64": 1e-6, "float32": 4e-6}
STRIDE, DT, PREC = 4, 0.01, (0.01, 0.05)
SIGN = np.array([1, -1, 1, -1, 1, -1, 1.0])


def _goto(tr, oc, io_dtype, rule=None):
    """the goal one step of 0.1 rad per joint away, a value of the I/O type as the GPU tests' goals are; arm 2 has no goal block.  (No
    mixer, no limiter: REV's stall_reference.goto ran a goto under the script's rounded mixer and sent the goal frame, its
    goto_reference.goto_reference did neither; here, as at every call site of the two, both give the same arrays.)"""
    from vfclik_amd import _abi
    chain, w, qg, way, q0, params = tr.three_lwr_arms(_abi.F_NULLSPACE | _abi.F_JOINT_LIMIT_TASK)
    w["fields"]["p"][:, 0, :16] = way[:, 1].astype(io_dtype).astype(np.float64)
    w["nfields"][2] = 0
    return tr.goto(oc, chain, params, q0, w["fields"], w["nfields"], 160, STRIDE, DT, PREC, hold=True, clamp=True, io_dtype=io_dtype, rule=rule)


def _goto_stall(tr, oc, io_dtype):
    """... and stalls at check 2 under a rule of patience 3"""
    return _goto(tr, oc, io_dtype, rule=tr.Rule(3, eps=(1e-3, 1e-2)))


def _follow(tr, oc, io_dtype):
    """three waypoints, looser via pair; the caller gates arm 1, arm 2's path has one row"""
    from vfclik_amd import _abi
    chain, w, qg, way, q0, params = tr.three_lwr_arms(_abi.F_NULLSPACE | _abi.F_MIXER | _abi.F_LIMITER)
    way[2, 1:] = np.nan
    return tr.follow(oc, chain, params, q0, w["fields"], w["nfields"], way, 160, STRIDE, DT, PREC, via_precision=(0.03, 0.1), hold=True,
                     clamp=True, active=[1, 0, 1], io_dtype=io_dtype)


def _goto_js(tr, oc, io_dtype):
    """pure joint control; arm 2's reference starts with NaN: no controller"""
    from vfclik_amd import _abi
    chain, w, qg, way, q0, params = tr.three_lwr_arms(_abi.F_MIXER, mix_w=[0, 0, 1, 0, 0, 0], jp_kp=8.0)
    q_ref = qg[:, 0].copy()
    q_ref[2, 0] = np.nan
    return tr.goto_js(oc, chain, params, q0, w["fields"], w["nfields"], q_ref, 160, STRIDE, DT, 0.01 * np.ones(7), hold=True, clamp=True,
                      io_dtype=io_dtype)


def _follow_js(tr, oc, io_dtype):
    """three postures, via band 3 x, no hold; the caller gates arm 1, arm 2's list has one row"""
    from vfclik_amd import _abi
    chain, w, qg, way, q0, params = tr.three_lwr_arms(_abi.F_MIXER, mix_w=[0, 0, 1, 0, 0, 0], jp_kp=8.0)
    qg[2, 1:] = np.nan
    p = 0.01 * np.ones(7)
    return tr.follow_js(oc, chain, params, q0, w["fields"], w["nfields"], qg, 160, STRIDE, DT, p, via_prec=3 * p, hold=False, clamp=True,
                        active=[1, 0, 1], io_dtype=io_dtype)


def _script(tr, oc, io_dtype):
    """arm 0: a posture, then a frame; arm 1: that frame, then a posture; arm 2: no script.  The goals as they stand are the frames of the
    first postures: an arm at a posture step is measured against its goal as it stands, and the angles stay small enough for a float32
    distance row to be held to 2e-6 degrees."""
    from vfclik_amd import _abi
    chain, w, qg, way, q0, params = tr.three_lwr_arms(_abi.F_MIXER, jp_kp=8.0)
    w["fields"]["p"][:, 0, :16] = way[:, 0]
    F, P = tr.FRAME, tr.POSTURE
    kind = np.array([[P, F, 0], [F, P, 0], [0, F, P]], dtype=np.int32)
    q0 = np.array([qg[0, 0] + 0.02 * SIGN, qg[1, 0] + 0.03 * SIGN, qg[2, 0]])
    return tr.script(oc, chain, params, q0, w["fields"], w["nfields"], kind, way, qg, 240, STRIDE, DT, PREC, 0.01 * np.ones(7), hold=True,
                     clamp=True, io_dtype=io_dtype)


CASES = {"goto": _goto, "goto_stall": _goto_stall, "follow": _follow, "goto_js": _goto_js, "follow_js": _follow_js, "script": _script}
JOINT_SPACE = ("goto_js", "follow_js")      # these report no distances: dist_traj is not stored for them


def main():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import timed_reference as tr
    from oracle import oracle_c
    oracle_c.build()
    out = {"readme": np.array("tests/timed_reference.py on the cases of tests/golden/make_timed_reference.py; the numbers of the five "
                              "helper modules of commit %s, bit for bit" % REV)}
    for name, case in CASES.items():
        for io in ("float64", "float32"):
            r = case(tr, oracle_c, np.dtype(io))
            near = min(float(np.min(r[k])) for k in CLOSEST if k in r)
            if near < MARGIN[io]:
                raise SystemExit("%s %s: a decision came within %.3e of its threshold (margin %.1e): choose another case" % (name, io, near, MARGIN[io]))
            for k in INTS + FLOATS:
                if k in r and not (k == "dist_traj" and name in JOINT_SPACE):
                    out["%s/%s/%s" % (name, io, k)] = r[k] if k in INTS else r[k].astype(io)
            angle = 0.0 if name in JOINT_SPACE else np.nanmax(r["dist_traj"][..., 1], initial=0.0)
            if angle >= 32.0:
                raise SystemExit("%s %s: an angle of %.1f degrees: a float32 distance row cannot be held to 2e-6 there" % (name, io, angle))
            print("%-10s %s  nearest decision %.3e  largest angle %.2f deg  next %s" % (name, io, near, angle, r["next"].tolist()))
    np.savez_compressed(FIXTURE, **out)
    print("%s: %d arrays, %d bytes" % (os.path.relpath(FIXTURE, ROOT), len(out), os.path.getsize(FIXTURE)))


if __name__ == "__main__":
    main()
