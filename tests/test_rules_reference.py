"""tests/rules_reference.py on the CPU: the three wrappers of the suite stacked around the oracle.

  * with only one rule present the stack IS the wrapper that is left: clearance_reference, avoid_reference (its script too) and
    coupled_reference with a stall rule, bit for bit on their own cached cases;
  * with min_clearance = -inf, gain = 0 and no stall rule it is coupled_reference's move bit for bit;
  * the scenes of tests/test_gpu_rules_together.py meet their conditions ON THE REFERENCE'S RUN, move by move and over the moves together,
    and the share of arms that test leaves out of the exact comparison stays under the suite's cap;
  * what the rules mean where they meet: an arm that waits is met by no arrival and no stall rule and stays in pending, its command is
    traced and not taken, a held or stalled arm below min_clearance does not count as waiting."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import avoid_reference as ar  # noqa: E402
import clearance_reference as wr  # noqa: E402
import coupled_reference as cr  # noqa: E402
import rules_reference as rr  # noqa: E402
import timed_reference as tr  # noqa: E402


def _equal(a, b, skip=()):
    assert set(a) - set(skip) == set(b) - set(skip), set(a) ^ set(b)
    for k in b:
        if k in skip:
            continue
        if isinstance(b[k], np.ndarray):
            assert np.array_equal(a[k], b[k], equal_nan=True) if b[k].dtype.kind == "f" else np.array_equal(a[k], b[k]), k


def _args(oracle_c, c, params):
    return (oracle_c, c["chain"], params, c["q0"], c["w"]["fields"], c["w"]["nfields"])


def _coup(c):
    return dict(spheres=c["spheres"], src_arm=c["src_arm"], xform=c["xform"], first_rep=c["first_rep"])


def _one(oracle_c, m, c, params, wait=None, avoid=None, rule=None):
    kw = dict(hold=m["hold"], clamp=True, io_dtype=m["io_dtype"], stepped=c["chain"].n > 7, want=("qdot_out",))
    if rule is not None:
        kw["rule"] = rule
    if c["way"] is None:
        return rr.goto(*_args(oracle_c, c, params), cr.N_CYCLES, m["stride"], cr.DT, cr.PREC, _coup(c), wait, avoid, **kw)
    return rr.follow(*_args(oracle_c, c, params), c["way"], cr.N_CYCLES, m["stride"], cr.DT, cr.PREC, _coup(c), wait, avoid, **kw)


@pytest.mark.parametrize("name", ["goto64", "goto32", "follow"])
def test_wait_rule_alone_is_clearance_reference(oracle_c, name):
    c, params, want = wr.reference(oracle_c, name)
    m = cr.MOVES[name]
    got = _one(oracle_c, m, c, params, wait=dict(min_clearance=wr.MIN_CLEARANCE[name], yields=wr.yields_of(m["B"]), mask=None))
    _equal(got, want, skip=("states",))
    assert want["waited"].any()


@pytest.mark.parametrize("name", sorted(ar.MOVES))
def test_avoid_rule_alone_is_avoid_reference(oracle_c, name):
    c, params, want = ar.reference(oracle_c, name)
    got = _one(oracle_c, ar.MOVES[name], c, params, avoid=dict(ar.RULE[name], channel=ar.CHANNEL))
    _equal(got, want, skip=("states",))
    assert np.any(np.nan_to_num(want["avoid_traj"]) != 0)


def test_avoid_rule_alone_in_a_script_is_avoid_reference(oracle_c):
    c, params, want, _off = ar.script_reference(oracle_c)
    m, n = ar.SCRIPT, c["chain"].n
    got = rr.script(*_args(oracle_c, c, params), c["kind"], c["way3"], c["wayq"], cr.N_CYCLES, m["stride"], cr.DT, cr.PREC, np.full(n, ar.JS_PREC),
                    _coup(c), None, dict(gain=m["gain"], d0=m["d0"], channel=ar.CHANNEL), js_via_precision=np.full(n, ar.JS_VIA),
                    io_dtype=m["io_dtype"], hold=m["hold"], clamp=True, want=("qdot_out",))
    _equal(got, want, skip=("states",))


def test_stall_rule_alone_is_coupled_reference(oracle_c):
    rule = tr.Rule(patience=5, eps=(1e-3, 1e-2))            # tests/test_gpu_coupled_moves.py: its coupled move under the stall rule
    c, params, want = cr.reference(oracle_c, "stall64", rule=rule)
    got = _one(oracle_c, cr.MOVES["stall64"], c, params, rule=rule)
    _equal(got, want, skip=("states",))
    assert np.count_nonzero(want["stalled"] >= 0) >= 10


@pytest.mark.parametrize("name", ["goto32", "follow"])
def test_rules_that_do_nothing_are_the_coupled_move(oracle_c, name):
    c, params, want = cr.reference(oracle_c, name)
    m = cr.MOVES[name]
    got = _one(oracle_c, m, c, params, wait=dict(min_clearance=-np.inf, yields=None, mask=None), avoid=dict(gain=0.0, d0=0.12, channel=4))
    for k in want:
        if isinstance(want[k], np.ndarray):
            assert np.array_equal(got[k], want[k], equal_nan=want[k].dtype.kind == "f"), k
    assert not got["waited"].any() and not np.nan_to_num(got["avoid_traj"]).any()


@pytest.mark.parametrize("scene,move", rr.ALL, ids=["%s-%s" % sm for sm in rr.ALL])
def test_the_scene_meets_its_conditions(oracle_c, scene, move):
    c, _p, r = rr.reference(oracle_c, scene, move)
    B = rr.SCENES[scene]["B"]
    cond = rr.conditions(c, r)
    out, part, share, cap = rr.left_out(c, r)
    print("%s %s: %s; left out %d of %d (%.1f %%, cap %.0f %%)" % (scene, move, cond, np.count_nonzero(out & part), np.count_nonzero(part),
                                                                 100 * share, 100 * cap))
    assert rr.conditions_hold(cond, B), cond
    assert share <= cap, share
    # what the rules mean where they meet
    wt, gt = r["wait_traj"], r["gate_traj"]
    yl = rr.yields_of(B) != 0
    stride = rr.SCENES[scene]["stride"]
    assert not wt[:, ~yl].any() and not (wt & ~gt).any()
    q_in = np.concatenate([c["q0"][None], r["q_traj"][:-1]], axis=0)
    assert np.array_equal(r["q_traj"][wt], q_in[wt])                                   # a waiting arm's row repeats, whatever its command
    assert np.any(np.nan_to_num(r["avoid_traj"])[wt] != 0)                             # ... and some of them carry one
    # no arrival and no stall rule meets an arm in a block it waits through: the checks that decided are not among them
    k_st = np.where(r["stalled"] >= 0, (r["stalled"] + 1) // stride - 1, -1)
    st = np.flatnonzero(k_st >= 0)
    assert not wt[k_st[st], st].any()
    rc = r["reached"][r["reached"] >= 0]
    kk, bb = (r["reached"] + 1) // stride - 1, np.broadcast_to(np.arange(B)[:, None], r["reached"].shape)
    assert not wt[kk[r["reached"] >= 0], bb[r["reached"] >= 0]].any() and len(rc) >= 4
    # a stalled arm (stop) and a held arm leave the gate for good: they never wait again, however little room they have
    for b in st:
        assert not gt[k_st[b] + 1:, b].any()
    # an arm that waits through the last block is still under way and counted
    under_way = (r["length"] > 0) & (r["next"] < r["length"]) & (r["stalled"] < 0)
    assert wt[-1].any() and np.all(under_way[wt[-1]]) and r["pending"][-1] == np.count_nonzero(under_way)
    # ... and waiting alone can hold it up: an arm that waits from some block to the end, never arrives and never stalls
    dead = wt[-1] & (r["stalled"] < 0) & (r["next"] < r["length"])
    assert dead.any()


def test_the_conditions_over_the_moves_together(oracle_c):
    tot = dict(partner=0, far=0, below=0, far_included=0)
    for scene, move in rr.CASES:
        c, _p, r = rr.reference(oracle_c, scene, move)
        cond = rr.conditions(c, r)
        for k in ("partner", "far", "below"):
            tot[k] += cond[k]
        # the far arm that waits and stalls later is among the arms compared exactly: its stall check is held to the reference's
        tot["far_included"] += int(np.count_nonzero(~rr.left_out(c, r)[0][cond["far_arms"]]))
    print(tot)
    assert tot["partner"] >= 1 and tot["far"] >= 1 and tot["below"] >= 1 and tot["far_included"] >= 1


def test_the_poll_case_ends_early(oracle_c):
    """nobody yields: every arm arrives or stalls, and pending reaches 0 before the move's last check"""
    c, _p, r = rr.poll_reference(oracle_c)
    assert not r["waited"].any() and np.count_nonzero(r["stalled"] >= 0) >= 4
    n_checks = len(r["pending"])
    assert np.any(r["pending"][1:n_checks - 1:2] == 0), r["pending"]
    out, part, share, cap = rr.left_out(c, r)
    assert share <= cap
