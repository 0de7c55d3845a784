"""tests/clearance_reference.py on the CPU: the oracle-stepped coupled move with the wait rule in front of every block.

  * the scene of tests/test_gpu_wait_rule.py (the coupled moves, the odd arms yielding, MIN_CLEARANCE per move) meets its three conditions
    ON THE REFERENCE'S RUN: at least ten arms wait for at least one block and later run again, at least one arm waits through the last
    block, at least half of the yielding arms never wait;
  * the share of arms that test leaves out of the exact comparison -- near an arrival threshold, near min_clearance at any block, and the
    partners of both -- stays under the suite's cap;
  * what waiting means: a waiting arm's rows repeat, it is an arm that yields, it stays in pending, and it is an obstacle at the posture it
    holds; waited is the rule replayed on the run's own clearance rows; an even arm never waits;
  * a rule under which nobody yields, and one whose min_clearance nobody reaches, are coupled_reference's move bit for bit."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clearance_reference as wr  # noqa: E402
import coupled_reference as cr  # noqa: E402

MOVES = ("goto64", "goto32", "follow")


def left_out(name, c, r):
    """(out, part, share, cap) of a run under the rule: coupled_reference.left_out with the arms near min_clearance, partners always included"""
    m = cr.MOVES[name]
    part = r["length"] > 0
    near = wr.near_rule(r, wr.yields_of(m["B"]), wr.MIN_CLEARANCE[name], m["io_dtype"])
    out, _near, share, cap = cr.left_out(r, part, m["io_dtype"], c["src_arm"], True, near)
    return out, part, share, cap


@pytest.mark.parametrize("name", MOVES)
def test_the_scene_meets_its_conditions(oracle_c, name):
    c, _p, r = wr.reference(oracle_c, name)
    m = cr.MOVES[name]
    yl = wr.yields_of(m["B"])
    again, last, never = wr.conditions(r, yl)
    out, part, share, cap = left_out(name, c, r)
    print("%s, min_clearance %.3f: %d arms wait and run again, %d wait through the last block, %.0f %% of the yielding arms never wait; "
          "left out %d of %d (%.1f %%, cap %.0f %%)" % (name, wr.MIN_CLEARANCE[name], again, last, 100 * never, np.count_nonzero(out & part),
                                                       np.count_nonzero(part), 100 * share, 100 * cap))
    assert again >= 10 and last >= 1 and never >= 0.5
    assert share <= cap


@pytest.mark.parametrize("name", MOVES)
def test_what_waiting_means(oracle_c, name):
    c, _p, r = wr.reference(oracle_c, name)
    m = cr.MOVES[name]
    B, yl = m["B"], wr.yields_of(m["B"]) != 0
    wt, gt = r["wait_traj"], r["gate_traj"]
    assert not wt[:, ~yl].any() and not (wt & ~gt).any()
    wait, waited = wr.replay_rule(r["clear_traj"], gt, yl, wr.MIN_CLEARANCE[name])
    assert np.array_equal(wait, wt) and np.array_equal(waited, r["waited"])
    q_in = np.concatenate([c["q0"][None], r["q_traj"][:-1]], axis=0)
    for k, b in zip(*np.nonzero(wt)):
        assert np.array_equal(r["q_traj"][k, b], q_in[k, b])                 # its row repeats
        if k + 1 < wt.shape[0] and (b ^ 1) < B:
            assert np.array_equal(r["link_traj"][k + 1, b ^ 1], r["link_traj"][k, b ^ 1])   # ... and so do its spheres in its partner's rows
    # a waiting arm stays in pending: the arms that wait through the last block are under way
    under_way = (r["length"] > 0) & (r["next"] < r["length"])
    assert np.all(under_way[wt[-1]]) and r["pending"][-1] == np.count_nonzero(under_way)
    # the rows measured: the partner's links as placed for that block, NaN -> +inf for the arm without a partner
    alone = c["src_arm"] < 0
    assert np.all(np.isposinf(r["clear_traj"][:, alone])) and np.all(r["pair_traj"][:, alone] == -1)
    assert np.isfinite(r["clear_traj"][:, ~alone]).all() and (name == "follow" or alone.any())


@pytest.mark.parametrize("name", ("goto32", "follow"))
def test_a_rule_nobody_meets_is_the_coupled_move(oracle_c, name):
    c, params, want = cr.reference(oracle_c, name)
    m = cr.MOVES[name]
    keys = ("q_traj", "dist_traj", "reached", "next", "pending", "way_traj", "q", "qdot_out", "status", "link_traj")
    kw = dict(hold=m["hold"], clamp=True, io_dtype=m["io_dtype"], stepped=c["chain"].n > 7, want=("qdot_out",))
    args = (oracle_c, c["chain"], params, c["q0"], c["w"]["fields"], c["w"]["nfields"])
    coup = dict(spheres=c["spheres"], src_arm=c["src_arm"], xform=c["xform"], first_rep=c["first_rep"])
    for rule in (dict(min_clearance=10.0, yields=np.zeros(m["B"], dtype=np.int32)), dict(min_clearance=-10.0, yields=None)):
        if c["way"] is None:
            r = wr.goto(*args, cr.N_CYCLES, m["stride"], cr.DT, cr.PREC, coup, rule, **kw)
        else:
            r = wr.follow(*args, c["way"], cr.N_CYCLES, m["stride"], cr.DT, cr.PREC, coup, rule, **kw)
        assert all(np.array_equal(r[k], want[k], equal_nan=True) for k in keys)
        assert not r["waited"].any()
