"""Funnels, hemispheres and further attractors that move (vfik_move_scene), the host side: for an engine that has ``move_scene_host``
FieldSets.flush sends a re-sent funnel / hemisphere / further attractor with new coordinates as ONE scene move that carries exactly the
changed rows; everything a move does not carry is still structure, goal-only arms still arrive through ``move_fields_host``, and an
engine without the new method sees the calls it saw before.  Recording stand-in engines; no GPU."""
import ctypes

import numpy as np
import pytest

from vfclik_amd import _abi
from vfclik_amd import ports as yarp
from vfclik_amd.fields import FieldSets

SCENE_KEYS = ("goal", "repellers", "funnels", "hemispheres", "attractors")


class _SceneRecorder:
    """Keeps what FieldSets hands over; has all three ways in."""

    def __init__(self):
        self.calls = []

    def set_fields(self, fields, counts, first_arm=0):
        self.calls.append(("set", first_arm, fields.copy(), counts.copy()))

    def move_fields_host(self, goal=None, repellers=None, first_arm=0):
        self.calls.append(("move", first_arm, None if goal is None else goal.copy(), None if repellers is None else repellers.copy()))

    def move_scene_host(self, goal=None, repellers=None, funnels=None, hemispheres=None, attractors=None, first_arm=0):
        given = dict(goal=goal, repellers=repellers, funnels=funnels, hemispheres=hemispheres, attractors=attractors)
        self.calls.append(("scene", first_arm, {k: None if v is None else np.array(v, dtype=np.float64) for k, v in given.items()}))


class _MoveOnly:
    """An engine object of ABI 6 before vfik_move_scene (the recorder of tests/test_move_fields_host.py is such)."""

    def __init__(self):
        self.calls = []

    def set_fields(self, fields, counts, first_arm=0):
        self.calls.append(("set", first_arm, fields.copy(), counts.copy()))

    def move_fields_host(self, goal=None, repellers=None, first_arm=0):
        self.calls.append(("move", first_arm, None if goal is None else goal.copy(), None if repellers is None else repellers.copy()))


def _goal(x=0.4, y=0.1, z=0.5, slow=0.05):
    T = np.eye(4)
    T[:3, 3] = (x, y, z)
    return list(T.reshape(16)) + [slow]


def _scene():
    """goalAndNormal-like: goal 1, funnel 2, near-goal repeller 3, obstacles 4, 5, a second attractor 6, a second funnel 7, hemispheres
    40 and 41"""
    return {1: [1.0, 1, _goal()],
            2: [30.0, 5, [0.4, 0.1, 0.5, 0.0, 0.0, 1.0, 0.15, 10.0, 0.15, 2.0]],
            3: [-10.0, 2, [0.4, 0.1, 0.45, 0.2, 0.001, 5.0]],
            4: [-10.0, 2, [0.1, 0.2, 0.3, 0.05, 0.001, 5.0]],
            5: [-10.0, 2, [-0.3, 0.2, 0.6, 0.07, 0.001, 5.0]],
            6: [0.7, 1, _goal(0.1, 0.1, 0.9)],
            7: [20.0, 5, [0.2, 0.2, 0.7, 1.0, 0.0, 0.0, 0.2, 8.0, 0.1, 2.0]],
            40: [-50.0, 4, [0.0, 0.0, -0.3, 0.0, 0.0, 1.0, 0.05, 5.0]],
            41: [-50.0, 4, [0.9, 0.0, 0.0, -1.0, 0.0, 0.0, 0.05, 5.0]]}


def _fresh(batch=6, engine=None):
    fs = FieldSets(batch, max_fields=10)
    eng = engine if engine is not None else _SceneRecorder()
    for a in range(batch):
        fs.set_arm(a, _scene())
    assert fs.flush(eng) == batch
    assert [c[0] for c in eng.calls] == ["set"] and eng.calls[0][1] == 0
    eng.calls.clear()
    return fs, eng


def _edit(fs, arm, vf_id, force=None, **p):
    s = {k: [v[0], v[1], list(v[2])] for k, v in fs.sets[arm].items()}
    if force is not None:
        s[vf_id][0] = force
    for k, v in p.items():
        s[vf_id][2][int(k[1:])] = v
    fs.set_arm(arm, s)


def _only(rows, *keep):
    """every row of the array is NaN except those listed"""
    mask = np.ones(rows.shape[:-1], dtype=bool)
    for idx in keep:
        mask[idx] = False
    return np.isnan(rows[mask]).all() and not np.isnan(rows[~mask]).any()


def test_a_funnel_edit_is_one_scene_move_with_exactly_that_row():
    fs, eng = _fresh()
    _edit(fs, 2, 7, p0=0.25, p4=0.6, p5=0.8)           # arm 2: its SECOND funnel (ids 2, 7): apex and axis
    assert fs.flush(eng) == 1
    (kind, lo, kw), = eng.calls
    assert kind == "scene" and lo == 2
    assert [k for k in SCENE_KEYS if kw[k] is not None] == ["funnels"]
    assert kw["funnels"].shape == (1, 2, 6) and _only(kw["funnels"], (0, 1))
    assert list(kw["funnels"][0, 1]) == [0.25, 0.2, 0.7, 1.0, 0.6, 0.8]


def test_a_hemisphere_edit_is_one_scene_move_with_exactly_that_row():
    fs, eng = _fresh()
    _edit(fs, 4, 40, p2=-0.25, p3=0.1)                 # the first hemisphere (ids 40, 41)
    assert fs.flush(eng) == 1
    (kind, lo, kw), = eng.calls
    assert kind == "scene" and lo == 4
    assert [k for k in SCENE_KEYS if kw[k] is not None] == ["hemispheres"]
    assert kw["hemispheres"].shape == (1, 1, 6) and list(kw["hemispheres"][0, 0]) == [0.0, 0.0, -0.25, 0.1, 0.0, 1.0]


def test_a_further_attractor_edit_is_one_scene_move_with_exactly_that_row():
    fs, eng = _fresh()
    _edit(fs, 0, 6, p3=0.15, p11=0.8)                  # the attractor behind the goal: row 0 of `attractors`
    assert fs.flush(eng) == 1
    (kind, lo, kw), = eng.calls
    assert kind == "scene" and lo == 0
    assert [k for k in SCENE_KEYS if kw[k] is not None] == ["attractors"]
    rec, _ = fs.records([0])
    assert kw["attractors"].shape == (1, 1, 16)
    assert np.array_equal(kw["attractors"][0, 0, :12], rec["p"][0, 5, :12]) and kw["attractors"][0, 0, 3] == 0.15
    assert list(kw["attractors"][0, 0, 12:]) == [0.0, 0.0, 0.0, 1.0]


def test_a_run_of_arms_is_one_call_and_unchanged_rows_are_nan():
    """Arms 1..3 adjacent: arm 1 moves goal + funnel + near-goal repeller (the feeder's re-send), arm 2 its second hemisphere, arm 3 an
    obstacle and the further attractor.  One call; every row nobody changed is NaN."""
    fs, eng = _fresh()
    _edit(fs, 1, 1, p3=0.45, p7=0.12)
    _edit(fs, 1, 2, p0=0.45, p1=0.12)
    _edit(fs, 1, 3, p0=0.45, p1=0.12)
    _edit(fs, 2, 41, p0=0.95)
    _edit(fs, 3, 5, p2=0.65)
    _edit(fs, 3, 6, p7=0.3)
    assert fs.flush(eng) == 3
    (kind, lo, kw), = eng.calls
    assert kind == "scene" and lo == 1
    rec, _ = fs.records([1, 2, 3])                     # ascending id: 1 2 3 4 5 6 7 40 41
    assert kw["goal"].shape == (3, 16) and _only(kw["goal"], 0) and np.array_equal(kw["goal"][0, :12], rec["p"][0, 0, :12])
    assert kw["repellers"].shape == (3, 3, 4) and _only(kw["repellers"], (0, 0), (2, 2))
    assert np.array_equal(kw["repellers"][0, 0], rec["p"][0, 2, :4]) and np.array_equal(kw["repellers"][2, 2], rec["p"][2, 4, :4])
    assert kw["funnels"].shape == (3, 1, 6) and _only(kw["funnels"], (0, 0)) and np.array_equal(kw["funnels"][0, 0], rec["p"][0, 1, :6])
    assert kw["hemispheres"].shape == (3, 2, 6) and _only(kw["hemispheres"], (1, 1))
    assert np.array_equal(kw["hemispheres"][1, 1], rec["p"][1, 8, :6])
    assert kw["attractors"].shape == (3, 1, 16) and _only(kw["attractors"], (2, 0))
    assert np.array_equal(kw["attractors"][2, 0, :12], rec["p"][2, 5, :12])
    # the same numbers once more: nothing is sent
    _edit(fs, 2, 41, p0=0.95)
    eng.calls.clear()
    fs.flush(eng)
    assert eng.calls == []


@pytest.mark.parametrize("what", ["cut_angle", "angle_order", "cut_dist", "dist_order", "funnel_force", "safe", "hemi_order", "hemi_force",
                                  "att_force", "att_slowdown", "att_row3"])
def test_what_a_scene_move_does_not_carry_is_still_structure(what):
    fs, eng = _fresh(3)
    edits = {"cut_angle": (2, dict(p6=0.2)), "angle_order": (2, dict(p7=8.0)), "cut_dist": (7, dict(p8=0.12)), "dist_order": (2, dict(p9=3.0)),
             "funnel_force": (7, dict(force=25.0)), "safe": (40, dict(p6=0.06)), "hemi_order": (41, dict(p7=4.0)),
             "hemi_force": (40, dict(force=-40.0)), "att_force": (6, dict(force=0.8)), "att_slowdown": (6, dict(p16=0.1)),
             "att_row3": (6, dict(p15=2.0))}
    vf_id, kw = edits[what]
    _edit(fs, 1, vf_id, **kw)
    _edit(fs, 1, 2, p0=0.41)                           # (coordinates moved as well: the arm still needs set_fields)
    _edit(fs, 2, 2, p0=0.5)                            # the neighbour merely moved its funnel
    fs.flush(eng)
    assert sorted(c[0] for c in eng.calls) == ["scene", "set"]
    st = [c for c in eng.calls if c[0] == "set"][0]
    rec, cnt = fs.records([1])
    assert st[1] == 1 and np.array_equal(st[3], cnt) and st[2].tobytes() == rec.tobytes()
    sc = [c for c in eng.calls if c[0] == "scene"][0]
    assert sc[1] == 2 and sc[2]["funnels"][0, 0, 0] == 0.5
    # the new structure is the one remembered
    eng.calls.clear()
    _edit(fs, 1, 40, p2=-0.2)
    fs.flush(eng)
    assert [c[0] for c in eng.calls] == ["scene"]


def test_goal_only_arms_still_arrive_through_move_fields_host():
    """The arguments of tests/test_move_fields_host.py's first test, unchanged by the presence of move_scene_host; the arm between them
    that moved a funnel goes its own way."""
    fs, eng = _fresh()
    _edit(fs, 1, 1, p3=0.45, p7=0.12)
    _edit(fs, 2, 5, p0=-0.25, p3=0.08)
    _edit(fs, 2, 1, p11=0.55)
    _edit(fs, 3, 2, p2=0.55)                           # adjacent, but a scene move
    _edit(fs, 4, 3, p2=0.4)
    assert fs.flush(eng) == 4
    assert [c[0] for c in eng.calls] == ["move", "move", "scene"]
    (_, lo, goal, rep), (_, lo4, goal4, rep4), (_, lo3, kw) = eng.calls
    rec, _ = fs.records([1, 2, 4])
    assert lo == 1 and goal.shape == (2, 16) and rep.shape == (2, 3, 4)
    assert np.array_equal(goal[:, :12], rec["p"][:2, 0, :12])
    assert np.isnan(rep[0]).all() and np.isnan(rep[1, :2]).all() and np.array_equal(rep[1, 2], rec["p"][1, 4, :4])
    assert lo4 == 4 and goal4 is None and rep4.shape == (1, 1, 4) and np.array_equal(rep4[0, 0], rec["p"][2, 2, :4])
    assert lo3 == 3 and kw["goal"] is None and kw["repellers"] is None and kw["funnels"][0, 0, 2] == 0.55


def test_an_engine_without_move_scene_host_sees_the_calls_it_saw_before():
    fs, eng = _fresh(4, _MoveOnly())
    _edit(fs, 0, 1, p3=0.45)                           # goal: a move
    _edit(fs, 1, 2, p0=0.45)                           # funnel: structure for this engine
    _edit(fs, 2, 40, p2=-0.25)                         # hemisphere: structure
    _edit(fs, 3, 6, p3=0.2)                            # further attractor: structure
    assert fs.flush(eng) == 4
    assert [(c[0], c[1]) for c in eng.calls] == [("set", 1), ("move", 0)]
    rec, cnt = fs.records([1, 2, 3])
    assert eng.calls[0][2].tobytes() == rec.tobytes() and np.array_equal(eng.calls[0][3], cnt)
    assert eng.calls[1][3] is None and eng.calls[1][2][0, 3] == 0.45


def _port(name, strict=False):
    p = yarp.BufferedPortBottle()
    p.open(name)
    p.setStrict(strict)
    return p


def test_object_feeder_second_pose_flushes_without_set_fields():
    """`set goalAndNormal` and `set ObstacleH` twice with different poses: the feeder re-sends goal 1, funnel 2, near-goal repeller 3 and
    hemisphere 5 (object_feeder:248-303,335-354); the second flush holds no set_fields call and its rows are what records() holds."""
    from vfclik_amd.object_feeder import ObjectFeeder
    base = "/0/scene/right"
    param_in = _port(base + "/vectorField/param", strict=True)
    of = ObjectFeeder(base)
    user = _port("/scene_user")
    yarp.Network.connect("/scene_user", base + "/ofeeder/object")
    fs, eng = FieldSets(1, max_fields=8), _SceneRecorder()

    def send(*items):
        b = user.prepare()
        b.clear()
        for it in items:
            b.add(it)
        user.writeStrict()
        of.spin_once()
        while True:
            pb = param_in.read(False)
            if pb is None:
                break
            fs.handle_param(0, pb)

    def gan(x, y, z, ax):
        n = np.array(ax, dtype=float)
        return [1.0, 0.0, 0.0, x, 0.0, -1.0, 0.0, y, 0.0, 0.0, -1.0, z, 0.0, 0.0, 0.0, 1.0] + list(n) + [0.1, 0.15, 0.15]

    def hemi(x, y, z, nrm):
        return [1.0, 0.0, 0.0, x, 0.0, 1.0, 0.0, y, 0.0, 0.0, 1.0, z, 0.0, 0.0, 0.0, 1.0] + list(nrm) + [0.05, 5.0]

    send("set", "goalAndNormal", gan(0.4, -0.4, 0.4, (0.0, -1.0, 0.0)))
    send("set", "ObstacleH", 0, hemi(0.0, -0.4, 0.3, (0.0, 0.0, 1.0)))
    fs.flush(eng)
    assert [c[0] for c in eng.calls] == ["set"]
    eng.calls.clear()
    send("set", "goalAndNormal", gan(0.45, -0.35, 0.42, (0.0, -0.6, 0.8)))
    send("set", "ObstacleH", 0, hemi(0.05, -0.4, 0.32, (0.0, 0.6, 0.8)))
    assert fs.flush(eng) == 1
    (kind, lo, kw), = eng.calls                         # no set_fields: one scene move
    assert kind == "scene" and lo == 0 and kw["attractors"] is None
    rec, cnt = fs.records([0])
    assert list(rec["id"][0, :cnt[0]]) == [1, 2, 3, 5] and list(rec["type"][0, :cnt[0]]) == [1, 5, 2, 4]
    assert np.array_equal(kw["goal"][0, :12], rec["p"][0, 0, :12]) and kw["goal"][0, 3] == 0.45
    assert kw["funnels"].shape == (1, 1, 6) and np.array_equal(kw["funnels"][0, 0], rec["p"][0, 1, :6])
    assert list(kw["funnels"][0, 0]) == [0.45, -0.35, 0.42, 0.0, -0.6, 0.8]
    assert kw["repellers"].shape == (1, 1, 4) and np.array_equal(kw["repellers"][0, 0], rec["p"][0, 2, :4])
    assert kw["hemispheres"].shape == (1, 1, 6) and np.array_equal(kw["hemispheres"][0, 0], rec["p"][0, 3, :6])
    assert list(kw["hemispheres"][0, 0]) == [0.05, -0.4, 0.32, 0.0, 0.6, 0.8]
    of.close()


def test_sharded_engine_splits_scene_rows_like_set_fields():
    from vfclik_amd import robots, sharding

    made = []

    def factory(chain, batch, device=0, **kw):
        e = _SceneRecorder()
        e.batch = batch
        made.append(e)
        return e

    se = sharding.ShardedEngine(robots.lwr(), 10, rank=0, world=1, devices=[0, 1, 2], engine_factory=factory)
    rng = np.random.default_rng(0)
    arrs = dict(goal=rng.normal(size=(10, 16)), repellers=rng.normal(size=(10, 2, 4)), funnels=rng.normal(size=(10, 1, 6)),
                hemispheres=rng.normal(size=(10, 2, 6)), attractors=rng.normal(size=(10, 3, 16)))
    se.move_scene_host(**arrs)
    rows = [(a, b) for a, b, _ in se.parts]
    assert rows == [(0, 4), (4, 7), (7, 10)]
    for (a, b), e in zip(rows, made):
        (kind, lo, kw), = e.calls
        assert kind == "scene" and lo == 0
        for k in SCENE_KEYS:
            assert np.array_equal(kw[k], arrs[k][a:b]), k
    se.move_scene_host(funnels=arrs["funnels"])
    assert all(e.calls[-1][2]["goal"] is None and e.calls[-1][2]["funnels"] is not None for e in made)
    with pytest.raises(ValueError):
        se.move_scene_host(hemispheres=arrs["hemispheres"][:9])


def test_engine_methods_exist():
    from vfclik_amd import engine, sharding
    assert callable(engine.Engine.move_scene) and callable(engine.Engine.move_scene_host)
    assert callable(sharding.ShardedEngine.move_scene_host)
    assert _abi.ABI_VERSION == 6


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from vfclik_amd import engine
    return engine.load_library()


def test_null_handle_is_an_argument_error_and_the_abi_is_still_6(lib):
    assert lib.vfik_abi_version() == 6
    mv = _abi.SceneMove()
    g = (ctypes.c_double * 16)()
    mv.goal16 = ctypes.addressof(g)
    assert lib.vfik_move_scene(None, 0, 1, ctypes.byref(mv)) == -1                # VFIK_E_ARG
    assert b"null handle" in lib.vfik_last_error()
    assert lib.vfik_move_scene_host(None, 0, 1, ctypes.byref(mv)) == -1


def test_scene_move_size_matches_the_mirror(lib):
    assert lib.vfik_scene_move_size() == ctypes.sizeof(_abi.SceneMove) == 6 * 8 + 4 * 4
    sizes = (ctypes.c_size_t * 4)()
    lib.vfik_struct_sizes(sizes)                                                   # (still four entries, as before)
    from vfclik_amd import engine
    assert list(sizes) == [ctypes.sizeof(_abi.Field), ctypes.sizeof(_abi.Chain), ctypes.sizeof(_abi.Params), ctypes.sizeof(engine.IO)]
