"""tests/coupled_reference.py on the CPU: the oracle-stepped timed move with the other arm's link spheres in its loop.

  * every source -1: the result is timed_reference's, bit for bit -- the coupling writes nothing, and nothing else of the loop moved;
  * arms in pairs b <-> b ^ 1: EVERY paired arm's q_traj leaves the uncoupled run by more than 100 x the suite's path bar of the move's I/O
    type, 1e-6 rad at float64 and 2e-4 at float32 (measured: 7.8e-4 or more) -- what the GPU is held to under a coupling is not what it
    computes without one.  The arm without a partner stays on the uncoupled path bit for bit, the static obstacle in front of the coupled repellers stays put, and
    the repellers end where the last block put them;
  * link_traj[k] is the host's link points of q_traj[k - 1] (k = 0: of the start), rounded to the I/O type;
  * with `hold`, an arm that arrived is an obstacle at the posture it holds: its spheres stop moving in its partner's rows while the partner
    still runs;
  * the seeds of tests/test_gpu_coupled_moves.py keep the share of arms that test leaves out of the exact comparison -- near a threshold, and
    under `hold` the arms those are the source of -- under the suite's cap, on the reference's numbers."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import coupled_reference as cr  # noqa: E402

GOTOS = ("goto64", "goto32", "stall64")


def _equal(a, b, keys):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in keys)


@pytest.mark.parametrize("name", GOTOS + ("follow",))
def test_no_source_is_the_uncoupled_move(oracle_c, name):
    _c, _p, none = cr.reference(oracle_c, name, "none")
    _c, _p, off = cr.reference(oracle_c, name, "off")
    keys = ("q_traj", "dist_traj", "reached", "next", "pending", "way_traj", "q", "qdot_out", "status")
    assert _equal(none, off, keys)
    assert np.array_equal(none["fields"], off["fields"])
    assert np.isnan(none["link_traj"]).all()


@pytest.mark.parametrize("name", GOTOS)
def test_pairs_leave_the_uncoupled_path(oracle_c, name):
    c, _p, r = cr.reference(oracle_c, name)
    _c, _p, off = cr.reference(oracle_c, name, "off")
    m = cr.MOVES[name]
    B, io = m["B"], np.dtype(m["io_dtype"])
    d = np.abs(r["q_traj"] - off["q_traj"]).max(axis=(0, 2))
    print("%s: paired arms leave the uncoupled path by %.2e .. %.2e rad, median %.2e (100 x the path bar of %s: %.1e)"
          % (name, d[:B - 1].min(), d[:B - 1].max(), np.median(d[:B - 1]), io.name, 100 * cr.PATH_BAR[io]))
    assert B % 2 == 1 and c["src_arm"][B - 1] == -1
    assert d[:B - 1].min() > 100 * cr.PATH_BAR[io]
    assert d[B - 1] == 0.0                                   # no partner: the uncoupled path
    f0, f1 = c["w"]["fields"], r["fields"]
    ns = c["first_rep"]
    assert np.array_equal(f1["p"][:, 1:1 + ns], f0["p"][:, 1:1 + ns])       # the static obstacle stays put
    assert np.array_equal(f1["p"][:, :, 4:], f0["p"][:, :, 4:]) and np.array_equal(f1["force"], f0["force"])
    last = r["link_traj"][-1]
    assert np.array_equal(f1["p"][:B - 1, 1 + ns:, 0:4], last[:B - 1])       # where the last block put them
    assert np.all(f1["p"][B - 1, 1 + ns:, 0:3] == cr.PARKED)
    # the arms arrive at many distinct checks: under `hold` the GPU test sees arms that hold while their partners still run
    assert len(set(r["arrived"][r["arrived"] >= 0])) >= 15


@pytest.mark.parametrize("name", GOTOS + ("follow",))
def test_link_traj_is_the_previous_row(oracle_c, name):
    c, _p, r = cr.reference(oracle_c, name)
    io = cr.MOVES[name]["io_dtype"]
    for k in range(r["q_traj"].shape[0]):
        q = c["q0"] if k == 0 else r["q_traj"][k - 1]
        assert np.array_equal(r["link_traj"][k], cr.place(c["chain"], c["spheres"], q, c["src_arm"], c["xform"], io), equal_nan=True), k


def test_held_arm_is_an_obstacle_where_it_stopped(oracle_c):
    c, _p, r = cr.reference(oracle_c, "goto32")
    stride, arr, B = cr.MOVES["goto32"]["stride"], r["arrived"], cr.MOVES["goto32"]["B"]
    seen = 0
    for b in range(B - 1):
        p = b ^ 1
        if arr[b] < 0:
            continue
        k = (arr[b] + 1) // stride   # the first block that starts from b's arrival row
        if k >= r["link_traj"].shape[0] - 1 or (0 <= arr[p] <= arr[b]):
            continue
        rows = r["link_traj"][k:, p]                       # b's spheres as p sees them
        assert np.all(rows == rows[0]), (b, p)
        assert np.any(r["q_traj"][k:, p] != r["q_traj"][k - 1, p])   # ... while p still moves
        seen += 1
    assert seen >= 10, seen


def test_held_arm_kept_out_of_a_list_is_an_obstacle(oracle_c):
    """follow: arm 8 has no list -- it never runs, and arm 9 sees its spheres at its start posture in every block"""
    c, _p, r = cr.reference(oracle_c, "follow")
    assert r["length"][8] == 0 and r["length"][5] == 2
    assert np.all(r["q_traj"][:, 8] == c["q0"][8])
    assert np.all(r["link_traj"][:, 9] == r["link_traj"][0, 9]) and not np.isnan(r["link_traj"][0, 9]).any()


@pytest.mark.parametrize("name", GOTOS + ("follow",))
def test_seeds_stay_under_the_cap(oracle_c, name):
    c, _p, r = cr.reference(oracle_c, name)
    io = cr.MOVES[name]["io_dtype"]
    part = r["length"] > 0
    out, near, share, cap = cr.left_out(r, part, io, c["src_arm"], cr.MOVES[name]["hold"])
    print("%s: %d of %d arms left out, %d of them within the margin (%.1f %%, cap %.0f %%)"
          % (name, np.count_nonzero(out & part), np.count_nonzero(part), np.count_nonzero(near & part), 100 * share, 100 * cap))
    assert share <= cap
