"""tests/avoid_reference.py on the CPU: that the scene of tests/test_gpu_avoid_moves.py is not vacuous, and that the wrapper does what it
says.  On the ORACLE's run of every move: at least ten arms carry a nonzero command in some block, at least one arm carries none in any
block, and for at least one arm the smallest clearance over the move is larger with the rule than without (gain 0: the same loop, a
command of zeros)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import avoid_reference as ar  # noqa: E402
import coupled_reference as cr  # noqa: E402
import hp_avoid as ha  # noqa: E402


@pytest.fixture(scope="module")
def oc():
    import __graft_entry__ as g
    g.build()
    from oracle import oracle_c
    oracle_c.build()
    return oracle_c


@pytest.mark.parametrize("name", sorted(ar.MOVES))
def test_the_scene_is_not_vacuous(oc, name):
    c, _params, r = ar.reference(oc, name)
    _c, _p, off = ar.reference(oc, name, gain=0.0)
    pushed, never, wider = ar.conditions(r, off)
    moved = np.abs(r["q_traj"] - off["q_traj"]).max(axis=(0, 2))
    print("%s: %d arms pushed, %d never, %d with more room at their tightest; the paths differ by up to %.3e rad (median arm %.3e)" % (
        name, pushed, never, wider, moved.max(), np.median(moved)))
    assert pushed >= 10 and never >= 1 and wider >= 1
    assert not np.any(np.nan_to_num(off["avoid_traj"]) != 0)
    assert moved.max() > 1e3 * cr.PATH_BAR[np.dtype(ar.MOVES[name]["io_dtype"])]      # the push is seen in the path, far above its bar
    # an arm that is never pushed and whose partner is never pushed runs the move it runs without the rule
    quiet = ~np.any(np.nan_to_num(r["avoid_traj"]) != 0, axis=(0, 2))
    src = c["src_arm"]
    alone = quiet & np.where(src >= 0, quiet[np.maximum(src, 0)], True)
    assert np.array_equal(r["q_traj"][:, alone], off["q_traj"][:, alone])


def test_the_script_is_not_vacuous(oc):
    """the script of tests/test_gpu_avoid_moves.py: pushed arms, arms never pushed, more room; and both kinds of step are met under way"""
    c, _params, r, off = ar.script_reference(oc)
    pushed, never, wider = ar.conditions(r, off)
    posture, frame, goal = (int(np.count_nonzero(r["reached"][:, k] >= 0)) for k in range(3))
    print("script: %d arms pushed, %d never, %d with more room; %d reach the posture, %d the first frame, %d the goal" % (pushed, never, wider, posture, frame, goal))
    assert pushed >= 10 and never >= 1 and wider >= 1
    assert posture >= 100 and goal >= 50 and goal < posture
    # arms on a posture step and arms on a frame step ran in one block: the cycle took more than one controller group
    mixed = [(r["way_traj"][k] == 0).any() and (r["way_traj"][k] >= 1).any() for k in range(r["way_traj"].shape[0])]
    assert any(mixed)
    assert np.all(r["next"][8] == 0) and r["length"][8] == 0 and r["length"][5] == 1


def test_the_wrapper_adds_the_host_command():
    """every block's avoid_traj row is host_avoid of the block's input row and the coupling's rows, I/O-typed, and holds for the block"""
    class Spy:
        def __init__(self):
            self.ext = []

        def cycle_batch(self, chain, params, q, fields, nfields, **kw):
            self.ext.append(np.array(kw["ext_cmd"], copy=True))
            return {}

    from vfclik_amd import robots
    chain = robots.lwr()
    c = cr.pair_case(chain, 6, np.float32, seed=9)
    spy = Spy()
    rule = dict(gain=0.4, d0=0.5, channel=4)
    coup = dict(spheres=c["spheres"], src_arm=c["src_arm"], xform=c["xform"], first_rep=c["first_rep"])
    a, cp = ar._wrap(spy, chain, coup, rule, 2, 4, np.float32)
    fields = np.array(c["w"]["fields"], copy=True)
    qs = [c["q0"], c["q0"] + 0.01, c["q0"] + 0.02, c["q0"] + 0.03]
    for q in qs:
        base = np.zeros((4, 6, chain.n))
        base[0] = 0.25
        cp.cycle_batch(chain, None, q, fields, c["w"]["nfields"], ext_cmd=base)
    for k in (0, 1):
        want = ha.host_avoid(chain, c["spheres"], qs[2 * k], cp.link_traj[k], 0, len(c["spheres"]), None, 0.4, 0.5, None).astype(np.float32).astype(np.float64)
        assert np.any(want != 0) and np.array_equal(a.avoid_traj[k], want)
        for e in spy.ext[2 * k:2 * k + 2]:
            assert np.array_equal(e[2], want) and np.all(e[0] == 0.25) and not e[1].any() and not e[3].any()
