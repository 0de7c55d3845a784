"""Field-set maintenance of the vector-field executor, batched.

Each reference ``vf`` process keeps ``vectorFields = {id: [force, type, params]}`` and edits it from
``/param`` bottles (/root/reference/scripts/vf:145,209-275); on every message it rebuilds the summed
field (vf:276-293).  Here one :class:`FieldSets` keeps those dictionaries for B arms, applies the same
acceptance rules to each bottle, and hands the arms whose set changed to ``Engine.set_fields`` -- the
batched equivalent of the rebuild -- or, when only a goal frame or obstacle coordinates moved, to
``Engine.move_fields_host`` (with a funnel, a hemisphere or a further attractor among them: ``Engine.move_scene_host``), which
rewrites those numbers on the device without repacking.  Malformed bottles are reported and ignored, never raised, like the
reference (vf:264-266,275).
"""
import logging
import weakref

import numpy as np

from . import _abi

log = logging.getLogger("vfclik_amd.fields")

#: primitive types of the library (keys of vfl.vfl.vectorFieldLibrary() the reference uses: vf:148,238)
KNOWN_TYPES = (0, 1, 2, 4, 5)


class FieldSets:
    def __init__(self, batch, max_fields=16):
        self.batch = int(batch)
        self.max_fields = int(max_fields)
        self.sets = [dict() for _ in range(self.batch)]  # id -> [force, type, params]
        self.dirty = set()
        # per arm the set flushed last ({id: [force, type, params]}, None: never) and the engine it went to: what tells a move from a new structure
        self._flushed = [None] * self.batch
        self._flushed_to = None

    # -- one /param bottle for one arm (vf:212-275) ---------------------------------------------
    def handle_param(self, arm, bottle):
        """Apply an ``add`` / ``remove`` bottle.  Returns True when the arm's set changed."""
        if bottle is None or bottle.size() < 1:
            return False
        action = bottle.get(0).toString()
        vf = self.sets[arm]
        if action == "add":
            if bottle.size() != 5:  # vf:227,265-266
                log.warning("arm %d: wrong number of values, expected 5, ignoring", arm)
                return False
            vf_id = bottle.get(1).asInt()
            force = bottle.get(2).asDouble()
            vf_type = bottle.get(3).asInt()
            if vf_type not in KNOWN_TYPES:  # vf:238,263-264
                log.warning("arm %d: unknown vector field type %d, ignoring", arm, vf_type)
                return False
            plist = bottle.get(4).asList()
            params = [plist.get(i).asDouble() for i in range(plist.size())] if plist is not None else []
            need = _abi.FIELD_NPARAMS[vf_type]
            if len(params) < need:
                # the reference would fail later inside vfl's setParams; the batched library refuses here
                log.warning("arm %d: type %d needs %d parameters, got %d, ignoring", arm, vf_type, need, len(params))
                return False
            if vf_id not in vf and len(vf) >= self.max_fields:
                log.warning("arm %d: field capacity %d reached, ignoring id %d", arm, self.max_fields, vf_id)
                return False
            vf[vf_id] = [force, vf_type, params[:need]]
        elif action == "remove":
            if bottle.size() != 2:  # vf:268,274-275
                log.warning("arm %d: wrong number of values, expected 2", arm)
                return False
            vf_id = bottle.get(1).asInt()
            if vf_id not in vf:  # vf:269-273: silently nothing
                return False
            del vf[vf_id]
        else:
            return False
        self.dirty.add(arm)
        return True

    # -- direct (array) interface -------------------------------------------------------------------
    def set_arm(self, arm, fields):
        """fields: {id: [force, type, params]} replacing the arm's whole set."""
        for vf_id, (force, vf_type, params) in fields.items():
            if vf_type not in KNOWN_TYPES or len(params) < _abi.FIELD_NPARAMS[vf_type]:
                raise ValueError("field %d: bad type / parameter count" % vf_id)
        if len(fields) > self.max_fields:
            raise ValueError("more than %d fields" % self.max_fields)
        self.sets[arm] = {int(k): [float(v[0]), int(v[1]), [float(x) for x in v[2]]] for k, v in fields.items()}
        self.dirty.add(arm)

    def records(self, arms):
        """Structured array (len(arms), max_fields) + counts, ascending id, for Engine.set_fields."""
        arms = list(arms)
        rec = np.zeros((len(arms), self.max_fields), dtype=_abi.FIELD_DTYPE)
        cnt = np.zeros(len(arms), dtype=np.int32)
        for j, a in enumerate(arms):
            for k, vf_id in enumerate(sorted(self.sets[a])):
                force, vf_type, params = self.sets[a][vf_id]
                r = rec[j, k]
                r["id"], r["type"], r["force"] = vf_id, vf_type, force
                r["p"][: len(params)] = params
            cnt[j] = len(self.sets[a])
        return rec, cnt

    # -- what a move carries (Engine.move_fields_host) ---------------------------------------------
    @staticmethod
    def _goal_id(fields):
        """The id of the goal block: the lowest-id attractor (vfik_set_fields packs that one into the goal planes)."""
        ids = [i for i in sorted(fields) if fields[i][1] == _abi.FIELD_ATTRACTOR]
        return ids[0] if ids else None

    def _move_of(self, arm, scene=False):
        """How the arm's set differs from what was flushed last: None when the structure changed (ids, types, forces, or a
        parameter a move does not carry -- the arm needs set_fields), else (goal12 or None, {k: [x, y, z, radius]}, scene rows) with
        the new goal frame rows 0-2 and the new coordinates of the k-th decay repeller in ascending-id order; all empty when
        nothing changed at all.  scene (an engine with ``move_scene_host``): new coordinates of a funnel, a hemisphere or an
        attractor behind the goal are a move too -- scene rows = ({k: p[:6]} funnels, {k: p[:6]} hemispheres, {k: p[:12]}
        attractors), k counting that class in ascending-id order; without it they are structure and the three stay empty."""
        old, new = self._flushed[arm], self.sets[arm]
        if old is None or sorted(old) != sorted(new):
            return None
        goal_id = self._goal_id(new)
        goal, reps, k = None, {}, 0
        rows = {_abi.FIELD_FUNNEL: {}, _abi.FIELD_HEMISPHERE: {}, _abi.FIELD_ATTRACTOR: {}}
        seen = {_abi.FIELD_FUNNEL: 0, _abi.FIELD_HEMISPHERE: 0, _abi.FIELD_ATTRACTOR: 0}
        for vf_id in sorted(new):
            (f0, t0, p0), (f1, t1, p1) = old[vf_id], new[vf_id]
            if t0 != t1 or f0 != f1:
                return None
            if vf_id == goal_id:
                if p0[12:] != p1[12:]:      # the frame's last row and the slow-down distance stay
                    return None
                if p0[:12] != p1[:12]:
                    goal = p1[:12]
            elif t1 == _abi.FIELD_REPELLER:
                if p0[4:] != p1[4:]:        # safe distance and order stay
                    return None
                if p0[:4] != p1[:4]:
                    reps[k] = p1[:4]
                k += 1
            elif scene and t1 in rows:
                head = 12 if t1 == _abi.FIELD_ATTRACTOR else 6
                if p0[head:] != p1[head:]:  # cut angle, orders, distances; the frame's last row and the slow-down distance stay
                    return None
                if p0[:head] != p1[:head]:
                    rows[t1][seen[t1]] = p1[:head]
                seen[t1] += 1
            elif p0 != p1:                  # funnels, hemispheres, further attractors: moved by move_scene_host only
                return None
        return goal, reps, (rows[_abi.FIELD_FUNNEL], rows[_abi.FIELD_HEMISPHERE], rows[_abi.FIELD_ATTRACTOR])

    def forget(self):
        """Forget what was flushed: the next flush sends every changed arm through set_fields (for a caller that wrote
        field sets to the engine behind this object's back)."""
        self._flushed = [None] * self.batch
        self._flushed_to = None

    @staticmethod
    def _runs(arms):
        start = prev = arms[0]
        for a in arms[1:]:
            if a != prev + 1:
                yield start, prev
                start = a
            prev = a
        yield start, prev

    def flush(self, engine):
        """Upload the sets of all arms that changed since the last flush, as contiguous arm ranges.  Arms whose change leaves
        the structure flushed last intact -- a goal frame and / or x y z radius of decay repellers re-sent with new numbers, what
        the object feeder does for an object that moves (object_feeder:214-354) -- go through ``engine.move_fields_host`` (rows
        that did not change are NaN: they stay); every other arm, and every arm of an engine without that method, goes through
        ``engine.set_fields``.  An engine that also has ``move_scene_host`` gets the arms whose funnel (the approach direction of
        `set goalAndNormal`, object_feeder:248-303), hemisphere (`set ObstacleH`, object_feeder:335-354) or further attractor came
        with new coordinates through that method, their goal and repeller rows in the same call.  The device holds the same field
        sets either way."""
        if not self.dirty:
            return 0
        arms = sorted(self.dirty)
        self.dirty.clear()
        if self._flushed_to is None or self._flushed_to() is not engine:
            self.forget()
        can_move = hasattr(engine, "move_fields_host")
        can_scene = can_move and hasattr(engine, "move_scene_host")
        moves, scenes, full = {}, {}, []
        for a in arms:
            mv = self._move_of(a, scene=can_scene) if can_move else None
            if mv is None:
                full.append(a)
            elif any(mv[2]):
                scenes[a] = mv
            elif mv[0] is not None or mv[1]:
                moves[a] = mv
        for lo, hi in (self._runs(full) if full else ()):
            rec, cnt = self.records(range(lo, hi + 1))
            engine.set_fields(rec, cnt, first_arm=lo)
        for lo, hi in (self._runs(sorted(moves)) if moves else ()):
            n = hi - lo + 1
            n_rep = max(max(moves[a][1], default=-1) for a in range(lo, hi + 1)) + 1
            goal = rep = None
            if any(moves[a][0] is not None for a in range(lo, hi + 1)):
                goal = np.full((n, 16), np.nan)
            if n_rep:
                rep = np.full((n, n_rep, 4), np.nan)
            for a in range(lo, hi + 1):
                g, reps, _ = moves[a]
                if g is not None:
                    goal[a - lo, :12] = g
                    goal[a - lo, 12:] = (0.0, 0.0, 0.0, 1.0)
                for k, xyzr in reps.items():
                    rep[a - lo, k] = xyzr
            engine.move_fields_host(goal=goal, repellers=rep, first_arm=lo)
        for lo, hi in (self._runs(sorted(scenes)) if scenes else ()):
            n = hi - lo + 1
            run = [scenes[a] for a in range(lo, hi + 1)]
            kw = {}
            if any(mv[0] is not None for mv in run):
                kw["goal"] = np.full((n, 16), np.nan)
            for name, width, pick in (("repellers", 4, lambda mv: mv[1]), ("funnels", 6, lambda mv: mv[2][0]),
                                      ("hemispheres", 6, lambda mv: mv[2][1]), ("attractors", 16, lambda mv: mv[2][2])):
                rows = max(max(pick(mv), default=-1) for mv in run) + 1
                if rows:
                    kw[name] = np.full((n, rows, width), np.nan)
            for j, mv in enumerate(run):
                if mv[0] is not None:
                    kw["goal"][j, :12] = mv[0]
                    kw["goal"][j, 12:] = (0.0, 0.0, 0.0, 1.0)
                for k, xyzr in mv[1].items():
                    kw["repellers"][j, k] = xyzr
                for k, p6 in mv[2][0].items():
                    kw["funnels"][j, k] = p6
                for k, p6 in mv[2][1].items():
                    kw["hemispheres"][j, k] = p6
                for k, p12 in mv[2][2].items():
                    kw["attractors"][j, k, :12] = p12
                    kw["attractors"][j, k, 12:] = (0.0, 0.0, 0.0, 1.0)
            engine.move_scene_host(first_arm=lo, **kw)
        try:
            self._flushed_to = weakref.ref(engine)
        except TypeError:
            self._flushed_to = (lambda e=engine: e)
        for a in arms:
            self._flushed[a] = {i: [f, t, list(p)] for i, (f, t, p) in self.sets[a].items()}
        return len(arms)
