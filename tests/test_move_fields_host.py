"""Goals and obstacles that move (ABI 6, vfik_move_fields), the host side: FieldSets.flush tells a re-sent primitive with new
coordinates (object_feeder:214-354 re-sends every primitive of an object whose pose changed) from a change of structure, and sends
the first through ``engine.move_fields_host`` and the second through ``engine.set_fields``.  A recording stand-in engine; no GPU."""
import ctypes

import numpy as np
import pytest

from vfclik_amd import _abi
from vfclik_amd.fields import FieldSets


class _Recorder:
    """Keeps what FieldSets hands over."""

    def __init__(self):
        self.calls = []

    def set_fields(self, fields, counts, first_arm=0):
        self.calls.append(("set", first_arm, fields.copy(), counts.copy()))

    def move_fields_host(self, goal=None, repellers=None, first_arm=0):
        self.calls.append(("move", first_arm, None if goal is None else goal.copy(), None if repellers is None else repellers.copy()))


class _SetOnly:
    """An engine object of before ABI 6 (the stand-ins of tests/test_ccb_host.py and tests/test_sharding_gloo.py are such)."""

    def __init__(self):
        self.calls = []

    def set_fields(self, fields, counts, first_arm=0):
        self.calls.append(("set", first_arm, fields.copy(), counts.copy()))


def _goal(x=0.4, y=0.1, z=0.5, slow=0.05):
    T = np.eye(4)
    T[:3, 3] = (x, y, z)
    return list(T.reshape(16)) + [slow]


def _scene(xyz=(0.4, 0.1, 0.5)):
    """goalAndNormal-like: goal 1, funnel 2, near-goal repeller 3, hemisphere 40, obstacles 4, 5"""
    return {1: [1.0, 1, _goal(*xyz)],
            2: [30.0, 5, [0.4, 0.1, 0.5, 0.0, 0.0, 1.0, 0.15, 10.0, 0.15, 2.0]],
            3: [-10.0, 2, [0.4, 0.1, 0.45, 0.2, 0.001, 5.0]],
            4: [-10.0, 2, [0.1, 0.2, 0.3, 0.05, 0.001, 5.0]],
            5: [-10.0, 2, [-0.3, 0.2, 0.6, 0.07, 0.001, 5.0]],
            40: [-50.0, 4, [0.0, 0.0, -0.3, 0.0, 0.0, 1.0, 0.05, 5.0]]}


def _fresh(batch=6, engine=None):
    fs = FieldSets(batch, max_fields=8)
    eng = engine if engine is not None else _Recorder()
    for a in range(batch):
        fs.set_arm(a, _scene())
    assert fs.flush(eng) == batch
    assert [c[0] for c in eng.calls] == ["set"] and eng.calls[0][1] == 0    # a first flush has nothing to move
    eng.calls.clear()
    return fs, eng


def _edit(fs, arm, vf_id, force=None, vf_type=None, **p):
    f = fs.sets[arm]
    s = {k: [v[0], v[1], list(v[2])] for k, v in f.items()}
    if force is not None:
        s[vf_id][0] = force
    if vf_type is not None:
        s[vf_id][1] = vf_type
    for k, v in p.items():
        s[vf_id][2][int(k[1:])] = v
    fs.set_arm(arm, s)


def test_resent_goal_and_obstacle_flush_as_a_move():
    fs, eng = _fresh()
    _edit(fs, 1, 1, p3=0.45, p7=0.12)                  # arm 1: the goal translated
    _edit(fs, 2, 5, p0=-0.25, p3=0.08)                 # arm 2: obstacle id 5 (the arm's third decay repeller: ids 3, 4, 5) moved and grew
    _edit(fs, 2, 1, p11=0.55)                          #        and its goal too
    _edit(fs, 4, 3, p2=0.4)                            # arm 4 (not adjacent): the near-goal repeller
    assert fs.flush(eng) == 3
    assert [c[0] for c in eng.calls] == ["move", "move"]
    (_, lo, goal, rep), (_, lo4, goal4, rep4) = eng.calls
    assert lo == 1 and goal.shape == (2, 16) and rep.shape == (2, 3, 4)
    rec, _ = fs.records([1, 2, 4])
    assert np.array_equal(goal[:, :12], rec["p"][:2, 0, :12])           # what records() holds, rows 0-2 of the frame
    assert np.isnan(rep[0]).all()                                       # arm 1: no repeller row
    assert np.isnan(rep[1, :2]).all() and np.array_equal(rep[1, 2], rec["p"][1, 4, :4])
    assert lo4 == 4 and goal4 is None and rep4.shape == (1, 1, 4)
    assert np.array_equal(rep4[0, 0], rec["p"][2, 2, :4])
    # the same numbers once more: nothing changed, nothing is sent
    _edit(fs, 4, 3, p2=0.4)
    eng.calls.clear()
    fs.flush(eng)
    assert eng.calls == []


def test_param_bottle_re_add_is_a_move():
    from vfclik_amd.ports import Bottle
    fs, eng = _fresh(2)
    b = Bottle()
    b.addString("add")
    b.addInt(4)
    b.addDouble(-10.0)
    b.addInt(2)
    lst = b.addList()
    for v in (0.15, 0.25, 0.35, 0.05, 0.001, 5.0):
        lst.addDouble(v)
    assert fs.handle_param(1, b)
    fs.flush(eng)
    assert [c[0] for c in eng.calls] == ["move"]
    _, lo, goal, rep = eng.calls[0]
    assert lo == 1 and goal is None and rep.shape == (1, 2, 4)
    assert np.isnan(rep[0, 0]).all() and list(rep[0, 1]) == [0.15, 0.25, 0.35, 0.05]


@pytest.mark.parametrize("what", ["force", "order", "safe", "type", "slowdown", "funnel", "hemisphere", "new_id", "removed_id", "goal_row3"])
def test_a_change_of_structure_flushes_through_set_fields(what):
    fs, eng = _fresh(3)
    if what == "force":
        _edit(fs, 1, 4, force=-12.0)
    elif what == "order":
        _edit(fs, 1, 4, p5=20.0)
    elif what == "safe":
        _edit(fs, 1, 4, p4=0.002)
    elif what == "type":
        s = _scene()
        s[5] = [-10.0, 4, [-0.3, 0.2, 0.6, 0.0, 0.0, 1.0, 0.05, 5.0]]
        fs.set_arm(1, s)
    elif what == "slowdown":
        _edit(fs, 1, 1, p16=0.1)
    elif what == "funnel":
        _edit(fs, 1, 2, p0=0.45)
    elif what == "hemisphere":
        _edit(fs, 1, 40, p2=-0.25)
    elif what == "new_id":
        s = _scene()
        s[6] = [-10.0, 2, [0.0, 0.0, 0.9, 0.05, 0.001, 5.0]]
        fs.set_arm(1, s)
    elif what == "removed_id":
        s = _scene()
        del s[5]
        fs.set_arm(1, s)
    elif what == "goal_row3":
        _edit(fs, 1, 1, p15=2.0)
    _edit(fs, 2, 1, p3=0.5)                            # the neighbour merely moved its goal
    fs.flush(eng)
    kinds = sorted(c[0] for c in eng.calls)
    assert kinds == ["move", "set"]
    st = [c for c in eng.calls if c[0] == "set"][0]
    rec, cnt = fs.records([1])
    assert st[1] == 1 and np.array_equal(st[3], cnt) and st[2].tobytes() == rec.tobytes()
    mv = [c for c in eng.calls if c[0] == "move"][0]
    assert mv[1] == 2 and mv[3] is None and mv[2][0, 3] == 0.5
    # from here on the new structure is the one remembered: the same arm moving again is a move
    eng.calls.clear()
    if what != "removed_id":
        _edit(fs, 1, 5, p1=0.33) if what != "type" else _edit(fs, 1, 4, p1=0.33)
    else:
        _edit(fs, 1, 4, p1=0.33)
    fs.flush(eng)
    assert [c[0] for c in eng.calls] == ["move"]


def test_an_engine_without_move_fields_host_gets_set_fields_only():
    fs, eng = _fresh(4, _SetOnly())
    _edit(fs, 0, 1, p3=0.45)
    _edit(fs, 1, 4, p0=0.2)
    _edit(fs, 3, 4, force=-11.0)
    assert fs.flush(eng) == 3
    assert [(c[0], c[1], c[2].shape[0]) for c in eng.calls] == [("set", 0, 2), ("set", 3, 1)]
    rec, cnt = fs.records([0, 1])
    assert eng.calls[0][2].tobytes() == rec.tobytes() and np.array_equal(eng.calls[0][3], cnt)


def test_another_engine_starts_from_set_fields():
    fs, eng = _fresh(2)
    other = _Recorder()
    _edit(fs, 0, 1, p3=0.45)
    fs.flush(other)                                    # the new engine never saw the structure
    assert [c[0] for c in other.calls] == ["set"]
    _edit(fs, 0, 1, p3=0.5)
    fs.flush(other)
    assert [c[0] for c in other.calls] == ["set", "move"]
    fs.forget()
    _edit(fs, 0, 1, p3=0.55)
    fs.flush(other)
    assert [c[0] for c in other.calls] == ["set", "move", "set"]


def test_second_attractor_is_not_the_goal():
    """The goal block is the LOWEST-id attractor: a further attractor that changes is structure."""
    fs = FieldSets(1, max_fields=4)
    eng = _Recorder()
    fs.set_arm(0, {3: [1.0, 1, _goal()], 7: [0.5, 1, _goal(0.1, 0.1, 0.9)]})
    fs.flush(eng)
    eng.calls.clear()
    fs.set_arm(0, {3: [1.0, 1, _goal()], 7: [0.5, 1, _goal(0.1, 0.2, 0.9)]})
    fs.flush(eng)
    assert [c[0] for c in eng.calls] == ["set"]
    fs.set_arm(0, {3: [1.0, 1, _goal(0.3, 0.3, 0.3)], 7: [0.5, 1, _goal(0.1, 0.2, 0.9)]})
    fs.flush(eng)
    assert [c[0] for c in eng.calls] == ["set", "move"] and eng.calls[1][2][0, 3] == 0.3


def test_sharded_engine_splits_move_rows_like_set_fields():
    from vfclik_amd import robots, sharding

    made = []

    def factory(chain, batch, device=0, **kw):
        e = _Recorder()
        e.batch = batch
        made.append(e)
        return e

    se = sharding.ShardedEngine(robots.lwr(), 10, rank=0, world=1, devices=[0, 1, 2], engine_factory=factory)
    goal = np.arange(160, dtype=np.float64).reshape(10, 16)
    rep = np.arange(10 * 2 * 4, dtype=np.float64).reshape(10, 2, 4)
    se.move_fields_host(goal=goal, repellers=rep)
    rows = [(a, b) for a, b, _ in se.parts]
    assert rows == [(0, 4), (4, 7), (7, 10)]
    for (a, b), e in zip(rows, made):
        (kind, lo, g, r), = e.calls
        assert kind == "move" and lo == 0 and np.array_equal(g, goal[a:b]) and np.array_equal(r, rep[a:b])
    se.move_fields_host(repellers=rep)
    assert all(e.calls[-1][2] is None for e in made)
    with pytest.raises(ValueError):
        se.move_fields_host(goal=goal[:9])


def test_engine_methods_exist_and_abi_is_6():
    from vfclik_amd import engine
    assert _abi.ABI_VERSION == 6
    assert callable(engine.Engine.move_fields) and callable(engine.Engine.move_fields_host)
    from vfclik_amd import sharding
    assert callable(sharding.ShardedEngine.move_fields_host)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from vfclik_amd import engine
    return engine.load_library()


def test_null_handle_is_an_argument_error(lib):
    assert lib.vfik_abi_version() == 6
    assert lib.vfik_move_fields(None, 0, 1, None, None, 0, None) == -1          # VFIK_E_ARG
    assert b"null handle" in lib.vfik_last_error()
    g = (ctypes.c_double * 16)()
    assert lib.vfik_move_fields_host(None, 0, 1, g, None, 0) == -1
