"""What a vfik_handle holds, per arm, after any sequence of setter calls -- as plain Python, from the documentation alone: include/vfik.h,
DESIGN.md and the comments of vfclik_amd/csrc/vfik_abi.cpp.

`Model` keeps VALUES only (no device representation: no promoted weights beside per-arm images, no uniform / compact / general slot images,
no shared tool beside a per-arm one): per arm a field list, a tool (16), wy, wq, a mixer row (6), max_vel, a speed scale, the external
channels 2..5, the oracle's `State` (the nullspace sign memory), and the vfik_params the caller passed last.  Every method mirrors the
`Engine` call of the same name and signature and applies the documented rule, so that one operation can be applied to a Model and to an
Engine alike (`apply`).  `Model.reference` is the C oracle's answer for the state the model holds.

`walk` is a seeded generator of operations over those methods (OpMaker makes them), each followed by a checkpoint (one launch of a drawn
form at the next joint angles of a slow loop).  A walk of 48 operations (schedule_48) interleaves, at seeded places: the set_fields program
(FIELDS_PROGRAM: every plan of vfik_scene.h, and every flip between plans through a call that names a few arms), the rules program
(rules_program: one block in which every history-dependent rule of the setters is met in the order that makes it matter), the flag sets,
a refused call, and operations drawn from all kinds with drawn ranges and values.  The walk of 16 operations on the large batch
(schedule_16) is a fixed order: its two seeds share the rules program between them.  tests/test_handle_model.py checks on the CPU that
the walks of CONFIGS x SEEDS reach what they are for; tests/test_gpu_handle_history.py drives one long-lived Engine through the same walks
and holds every launch to `Model.reference`.

WRONG_RULES lists the history-dependent rules, each as the name of a Model variant that has this one rule inverted or removed.

A helper of the suite, not a conftest.py."""
import collections
import ctypes as C

import numpy as np

from vfclik_amd import _abi
from vfclik_amd.engine import VfikError

F_NS, F_JL, F_MIX, F_LIM = _abi.F_NULLSPACE, _abi.F_JOINT_LIMIT_TASK, _abi.F_MIXER, _abi.F_LIMITER
FLAG_SETS = (0, F_MIX, F_NS | F_MIX, F_NS | F_MIX | F_LIM, F_NS | F_JL | F_MIX)
MAXF = 18                                    # fields per arm the model keeps room for (a refused call offers 17 repellers and a goal)
SLOTS_OF = {_abi.FIELD_NULL: 0, _abi.FIELD_ATTRACTOR: 3, _abi.FIELD_REPELLER: 1, _abi.FIELD_HEMISPHERE: 2, _abi.FIELD_FUNNEL: 2}
ALL_ROWS = ("qdot_vf", "qdot_null", "qdot_out", "pose", "pose_nt", "v6", "qdist", "status")
ROLL_K, ROLL_DT = 3, 0.01
GOTO_CYCLES, GOTO_STRIDE = 4, 2

Config = collections.namedtuple("Config", "name chain io_dtype B max_slots n_ops")
CONFIGS = (
    Config("lwr-f32", "lwr", np.float32, 203, 16, 48),
    Config("lwr-f64", "lwr", np.float64, 203, 16, 48),
    Config("powercube6-f32", "powercube6", np.float32, 203, 16, 48),
    Config("lwr_dual14-f32", "lwr_dual14", np.float32, 203, 16, 48),
    Config("chain10-f64", "chain10", np.float64, 203, 16, 48),
    Config("lwr-f32-big", "lwr", np.float32, 4096 + 64 + 37, 16, 16),   # beyond the eight-lanes sizes
)
SEEDS = (1, 2)

# one rule each, inverted or removed (Model(wrong=name)); the rule in the words of include/vfik.h or the issue behind it
WRONG_RULES = {
    "speed_unchanged_overwrites": "vfik_set_params with an UNCHANGED speed_scale leaves the per-arm speed scales",
    "speed_changed_ignored": "vfik_set_params with a CHANGED speed_scale overwrites every arm's",
    "weights_unchanged_overwrite": "vfik_set_params whose wy / wq equal what the caller passed last leaves the arms' own (and promoted) weights",
    "weights_changed_ignored": "vfik_set_params that CHANGES wy or wq replaces every arm's own weights",
    "maxvel_changed_ignored": "vfik_set_params that CHANGES max_vel writes it to every arm",
    "maxvel_unchanged_overwrites": "vfik_set_params with an unchanged max_vel leaves the per-arm limiter speeds",
    "mixw_changed_ignored": "vfik_set_params that CHANGES mix_w writes the new weights to every arm",
    "mixw_unchanged_overwrites": "vfik_set_params with an unchanged mix_w leaves the per-arm mixer rows",
    "absent_weights_reset": "vfik_set_arm_weights: an array that is NULL keeps its rows",
    "outside_arms_from_params": "vfik_set_arm_weights: arms outside the range hold the batch's CURRENT weights (promoted ones, not vfik_params')",
    "mixer_null_resets_speeds": "vfik_set_mixer_weights(NULL) leaves the per-arm limiter speeds",
    "mixer_null_keeps_rows": "vfik_set_mixer_weights(NULL) returns every arm's weights to vfik_params.mix_w",
    "set_fields_resets_speed": "vfik_set_fields leaves the arm's speedScale",
    "moves_forgotten_by_set_fields": "a vfik_set_fields on OTHER arms leaves the moved coordinates of the arms it does not name",
    "bridge_starts_from_defaults": "per-arm bridge state starts from the batch-wide vfik_params values",
}
# ... and the rounding rules.  What they change is half an ulp of a float32 coordinate (4e-9 m on a tool translation of 0.1 m, nothing at
# float64 I/O): the walk's amplifier arm (walk: amp_op) is what makes that much move a command.
ROUNDING_RULES = {
    "equal_tools_unrounded": "a per-arm tool array whose rows are all equal is stored rounded to the I/O type",
    "shared_tool_rounded": "a shared tool (per_arm = 0) is stored as given",
    "moves_unrounded": "vfik_move_*_host rounds to the I/O type exactly as vfik_set_fields rounds vfik_field.p[]",
}


# ---- field sets -----------------------------------------------------------------------------------------------------------------------
def _field(id_, type_, force, p):
    f = np.zeros((), dtype=_abi.FIELD_DTYPE)
    f["id"], f["type"], f["force"] = id_, type_, force
    f["p"][:len(p)] = p
    return f


def scene(family, goal16, near, rng, n_rep=None):
    """One arm's field list of a family that lands in a given plan (vfik_scene.h: plan_scene), as a list of records in ascending id.
    goal16: the arm's goal frame; near: where its tool is at the start of the walk -- the repellers stand 0.15 .. 0.35 m from there, near
    enough for an order-5 decay to move the arm's command."""
    def rep(k, order=5.0, force=-10.0, safe=0.001):
        d = rng.normal(size=3)
        pos = list(np.asarray(near) + d / np.linalg.norm(d) * rng.uniform(0.15, 0.35))
        return _field(4 + k, _abi.FIELD_REPELLER, force, pos + [rng.uniform(0.03, 0.10), safe, order])
    goal = _field(1, _abi.FIELD_ATTRACTOR, 1.0, list(goal16) + [0.05])
    funnel = lambda id_, d_order=2.0: _field(id_, _abi.FIELD_FUNNEL, 1.0, [goal16[3], goal16[7], goal16[11], 0.0, 0.0, 1.0, 0.5, 10.0, 0.3, d_order])  # noqa: E731
    hemi = _field(3, _abi.FIELD_HEMISPHERE, -10.0, [0.0, 0.0, -0.2, 0.05, -0.02, 1.0, 0.05, 5.0])
    if family == "none":
        return []
    if family == "feeder":        # goal + up to 8 order-5 repellers with the feeder's pair: the uniform image (one chunk at float32)
        return [goal] + [rep(k) for k in range(8 if n_rep is None else n_rep)]
    if family == "fewer":
        return [goal] + [rep(k) for k in range(2 if n_rep is None else n_rep)]
    if family == "pair":          # another (safe, force) on this arm: the compact image
        return [goal] + [rep(k, force=-5.0) for k in range(3)]
    if family == "orders":        # integer orders that differ by field: the order planes
        return [goal] + [rep(k, order=(5.0, 4.0, 2.0)[k % 3]) for k in range(4)]
    if family == "normal":        # goalAndNormal: goal, approach funnel, near-goal repeller: the aux block
        return [goal, funnel(2)] + [rep(k) for k in range(2)]
    if family == "hemi":
        return [goal, hemi] + [rep(k) for k in range(3)]
    if family == "funnel2":       # a second funnel: the general path
        return [goal, funnel(2), funnel(3, 3.0)] + [rep(k) for k in range(2)]
    if family == "frac":          # a fractional order: the general path
        return [goal] + [rep(k, order=2.5 if k == 1 else 5.0) for k in range(3)]
    if family == "too_many":      # 17 slots on a handle of 16: refused
        return [goal] + [rep(k) for k in range(17)]
    raise ValueError(family)


def records(arms, max_fields=None):
    """(fields[n_arms][max_fields], counts[n_arms]) of lists of records"""
    max_fields = max_fields or max([len(a) for a in arms] + [1])
    f = np.zeros((len(arms), max_fields), dtype=_abi.FIELD_DTYPE)
    for j, a in enumerate(arms):
        for k, fd in enumerate(a):
            f[j, k] = fd
    return f, np.array([len(a) for a in arms], dtype=np.int32)


def slots_needed(f):
    """vfik_scene.h: slots_needed -- the first attractor is free; -1: an unknown type"""
    need, have_goal = 0, False
    for t in f["type"]:
        if int(t) not in SLOTS_OF:
            return -1
        if t == _abi.FIELD_ATTRACTOR and not have_goal:
            have_goal = True
            continue
        need += SLOTS_OF[int(t)]
    return need


def whole_plan_request(model):
    """the model's whole field state as ONE vfik_set_fields call to a fresh handle, for tests/c_host/scene_plan.cpp's plan mode"""
    from test_scene_plan import request
    arms = [list(model.fields[b, :model.counts[b]]) for b in range(model.B)]
    return request(dict(nj=model.n, B=model.B, S=model.max_slots), 32 if model.io_dtype == np.float32 else 64, [(0, arms)])


PLAN_KEYS = ("slots_used", "field_path", "mixed_orders", "uniform", "one_chunk")


def parse_plan(line):
    """the driver's line -> what Engine.slots_in_use, field_path, mixed_orders, uniform_repellers and one_chunk report"""
    kv = dict(t.split("=") for t in line.split() if "=" in t and not t.startswith("pair="))
    return {k: int(kv[k]) for k in PLAN_KEYS}


def copy_params(p, **kw):
    out = _abi.Params()
    C.memmove(C.byref(out), C.byref(p), C.sizeof(out))
    for k, v in kw.items():
        k = "lambda_" if k == "lambda" else k
        if k in ("wy", "wq", "mix_w"):
            arr = getattr(out, k)
            for i, x in enumerate(v):
                arr[i] = float(x)
        else:
            setattr(out, k, v)
    return out


# ---- the model ------------------------------------------------------------------------------------------------------------------------
class Model:
    def __init__(self, oc, chain, B, io_dtype, max_slots, params=None, wrong=None):
        self.oc, self.chain, self.B, self.n = oc, chain, int(B), chain.n
        self.io_dtype, self.max_slots, self.wrong = np.dtype(io_dtype), int(max_slots), wrong
        self.fields = np.zeros((self.B, MAXF), dtype=_abi.FIELD_DTYPE)
        self.counts = np.zeros(self.B, dtype=np.int32)
        self.fields_set = False
        self.tool = np.tile(np.eye(4).reshape(16), (self.B, 1))
        self.params = copy_params(params if params is not None else _abi.default_params())
        self.wy = np.tile(np.array(self.params.wy[:6]), (self.B, 1))
        self.wq = np.tile(np.array(self.params.wq[:self.n]), (self.B, 1))
        self.promoted = False                     # (read by a wrong-rule variant alone: the right model needs no such bit)
        self.bridge = False                       # per-arm bridge state exists: mix / max_vel are the arms'; else vfik_params' are
        self.mix = np.zeros((self.B, _abi.MIX_CHANNELS))
        self.max_vel = np.zeros(self.B)
        self.speed = np.full(self.B, self.rnd(self.params.speed_scale))
        self.ext = np.zeros((4, self.B, self.n))
        self.small_batch = None
        self.states = oc.new_states(self.B, self.n)

    def clone(self, wrong=None):
        m = Model.__new__(Model)
        m.__dict__.update(self.__dict__)
        m.wrong = wrong if wrong is not None else self.wrong
        m.__dict__.pop("sign_watch", None)
        for k in ("fields", "counts", "tool", "wy", "wq", "mix", "max_vel", "speed", "ext"):
            setattr(m, k, getattr(self, k).copy())
        m.params = copy_params(self.params)
        m.states = (self.oc.State * self.B)()
        C.memmove(m.states, self.states, C.sizeof(m.states))
        return m

    def same_values(self, o):
        """every value a launch reads is equal (the sign memory apart)"""
        return (all(np.array_equal(getattr(self, k), getattr(o, k), equal_nan=True) for k in ("counts", "tool", "wy", "wq", "speed", "ext"))
                and self.fields.tobytes() == o.fields.tobytes() and bytes(self.params) == bytes(o.params)
                and np.array_equal(self.bridge_rows(), o.bridge_rows()))

    def rnd(self, a):
        """as the I/O type holds it"""
        return np.asarray(a, dtype=np.float64).astype(self.io_dtype).astype(np.float64)

    def _arms(self, first_arm, n_arms):
        if first_arm < 0 or n_arms < 1 or first_arm + n_arms > self.B:
            raise VfikError("arm range [%d, %d) outside batch %d" % (first_arm, first_arm + n_arms, self.B))
        return slice(first_arm, first_arm + n_arms)

    # -- vfik_set_params --
    def set_params(self, **kw):
        new, old = copy_params(self.params, **kw), self.params
        if not (new.lambda_ >= 0.0 and np.isfinite(new.lambda_) and new.speed_scale >= 0.0 and new.max_vel >= 0.0):
            raise VfikError("lambda, speed_scale and max_vel must be finite and >= 0")
        if (new.flags & F_JL) and not (new.flags & F_NS):
            raise VfikError("VFIK_F_JOINT_LIMIT_TASK needs VFIK_F_NULLSPACE")
        n, w = self.n, self.wrong
        speed_changed = new.speed_scale != old.speed_scale
        weights_changed = list(new.wy[:6]) != list(old.wy[:6]) or list(new.wq[:n]) != list(old.wq[:n])
        maxvel_changed = new.max_vel != old.max_vel
        mixw_changed = list(new.mix_w[:]) != list(old.mix_w[:])
        self.params = new
        if (speed_changed and w != "speed_changed_ignored") or w == "speed_unchanged_overwrites":
            self.speed[:] = self.rnd(new.speed_scale)
        if (weights_changed and w != "weights_changed_ignored") or w == "weights_unchanged_overwrite":
            self.wy[:], self.wq[:], self.promoted = np.array(new.wy[:6]), np.array(new.wq[:n]), False
        if self.bridge:
            if (maxvel_changed and w != "maxvel_changed_ignored") or w == "maxvel_unchanged_overwrites":
                self.max_vel[:] = new.max_vel
            if (mixw_changed and w != "mixw_changed_ignored") or w == "mixw_unchanged_overwrites":
                self.mix[:] = np.array(new.mix_w[:])

    # -- vfik_set_arm_weights --
    def set_arm_weights(self, wy=None, wq=None, first_arm=0):
        arrs = [None if a is None else np.asarray(a, dtype=np.float64) for a in (wy, wq)]
        if arrs[0] is None and arrs[1] is None:
            raise VfikError("give wy, wq or both")
        n_arms = (arrs[0] if arrs[0] is not None else arrs[1]).shape[0]
        sl = self._arms(first_arm, n_arms)
        if any(a is not None and not np.all(np.isfinite(a)) for a in arrs):
            raise VfikError("a weight is not finite")
        whole = first_arm == 0 and n_arms == self.B and arrs[0] is not None and arrs[1] is not None
        equal = whole and np.all(arrs[0] == arrs[0][0]) and np.all(arrs[1] == arrs[1][0])
        if self.wrong == "outside_arms_from_params" and self.promoted and not equal:
            self.wy[:], self.wq[:] = np.array(self.params.wy[:6]), np.array(self.params.wq[:self.n])
        for mine, a, batch in ((self.wy, arrs[0], self.params.wy), (self.wq, arrs[1], self.params.wq)):
            if a is not None:
                mine[sl] = a
            elif self.wrong == "absent_weights_reset":
                mine[sl] = np.array(batch[:mine.shape[1]])
        self.promoted = bool(equal)

    # -- the bridge: vfik_set_mixer_weights, vfik_set_max_vel --
    def _ensure_bridge(self):
        if not self.bridge:
            self.bridge = True
            if self.wrong == "bridge_starts_from_defaults":
                d = _abi.default_params()
                self.mix[:], self.max_vel[:] = np.array(d.mix_w[:]), d.max_vel
            else:
                self.mix[:], self.max_vel[:] = np.array(self.params.mix_w[:]), self.params.max_vel

    def set_mixer_weights(self, weights, first_arm=0):
        if weights is None:
            if self.bridge:
                if self.wrong != "mixer_null_keeps_rows":
                    self.mix[:] = np.array(self.params.mix_w[:])
                if self.wrong == "mixer_null_resets_speeds":
                    self.max_vel[:] = self.params.max_vel
            return
        w = np.asarray(weights, dtype=np.float64).reshape(-1, _abi.MIX_CHANNELS)
        sl = self._arms(first_arm, w.shape[0])
        self._ensure_bridge()
        self.mix[sl] = w

    def set_max_vel(self, values, first_arm=0):
        v = np.asarray(values, dtype=np.float64).reshape(-1)
        sl = self._arms(first_arm, len(v))
        if not np.all(v >= 0.0):
            raise VfikError("max_vel must be >= 0")
        self._ensure_bridge()
        self.max_vel[sl] = v

    def bridge_rows(self):
        """(B, 7): mixer row and limiter speed of every arm as a launch reads them -- the arms' own in the I/O type, else vfik_params' doubles"""
        if self.bridge:
            return self.rnd(np.concatenate([self.mix, self.max_vel[:, None]], axis=1))
        return np.tile(np.array(list(self.params.mix_w[:]) + [self.params.max_vel]), (self.B, 1))

    # -- vfik_set_tool --
    def set_tool(self, tool16, per_arm=False):
        t = np.asarray(tool16, dtype=np.float64)
        if per_arm:
            t = t.reshape(self.B, 16)
            equal = np.all(t[:, :12] == t[0, :12])
            self.tool = t.copy() if (equal and self.wrong == "equal_tools_unrounded") else self.rnd(t)
        else:
            t = t.reshape(16)
            self.tool = np.tile(self.rnd(t) if self.wrong == "shared_tool_rounded" else t, (self.B, 1))
        self.tool[:, 12:] = [0.0, 0.0, 0.0, 1.0]   # (rows 0..2 are the tool: the twelve numbers of include/vfik.h)

    # -- vfik_set_speed_scale --
    def set_speed_scale(self, values, first_arm=0):
        v = np.asarray(values, dtype=np.float64).reshape(-1)
        sl = self._arms(first_arm, len(v))
        if not (np.all(v >= 0.0) and np.all(np.isfinite(v))):
            raise VfikError("speedScale must be finite and >= 0")
        self.speed[sl] = self.rnd(v)

    # -- vfik_set_fields and the moves --
    def set_fields(self, fields, counts, first_arm=0):
        f = np.asarray(fields, dtype=_abi.FIELD_DTYPE)
        c = np.asarray(counts, dtype=np.int32)
        sl = self._arms(first_arm, f.shape[0])
        for j in range(f.shape[0]):
            if c[j] < 0 or c[j] > f.shape[1]:
                raise VfikError("count outside [0, max_fields]")
            need = slots_needed(f[j, :c[j]])
            if need < 0 or need > self.max_slots:
                raise VfikError("arm %d needs %d slots, handle capacity is %d" % (first_arm + j, need, self.max_slots))
        if self.wrong == "moves_forgotten_by_set_fields" and hasattr(self, "_as_set"):
            self.fields = self._as_set.copy()
        new = np.zeros((f.shape[0], MAXF), dtype=_abi.FIELD_DTYPE)
        for j in range(f.shape[0]):
            new[j, :c[j]] = f[j, :c[j]]
        new["p"], new["force"] = self.rnd(new["p"]), self.rnd(new["force"])   # (as pack_fields' put<T> rounds every scalar)
        self.fields[sl], self.counts[sl] = new, c
        self.fields_set = True
        if self.wrong == "set_fields_resets_speed":
            self.speed[sl] = self.rnd(self.params.speed_scale)
        if self.wrong == "moves_forgotten_by_set_fields":
            self._as_set = self.fields.copy()

    def _class_rows(self, b, type_, skip_first=False):
        """indices into arm b's list of its primitives of a type in ascending-id order"""
        f = self.fields[b, :self.counts[b]]
        idx = np.flatnonzero(f["type"] == type_)
        idx = idx[np.argsort(f["id"][idx], kind="stable")]
        return idx[1:] if skip_first else idx

    def move_scene_host(self, goal=None, repellers=None, funnels=None, hemispheres=None, attractors=None, first_arm=0):
        given = [None if a is None else np.asarray(a, dtype=np.float64) for a in (goal, repellers, funnels, hemispheres, attractors)]
        if all(a is None for a in given):
            raise VfikError("give at least one array")
        n_arms = next(a for a in given if a is not None).shape[0]
        self._arms(first_arm, n_arms)
        for a in given[1:]:
            if a is not None and a.shape[1] > self.max_slots:
                raise VfikError("a count is outside [0, max_slots]")
        if not self.fields_set:
            raise VfikError("a move before any vfik_set_fields: there is nothing to move")
        rnd = (lambda a: a) if self.wrong == "moves_unrounded" else self.rnd
        g = None if given[0] is None else rnd(given[0].reshape(n_arms, 16))
        classes = ((given[1], _abi.FIELD_REPELLER, 4, False), (given[2], _abi.FIELD_FUNNEL, 6, False),
                   (given[3], _abi.FIELD_HEMISPHERE, 6, False), (given[4], _abi.FIELD_ATTRACTOR, 12, True))
        for j in range(n_arms):
            b = first_arm + j
            if g is not None and not np.isnan(g[j, 0]):
                att = self._class_rows(b, _abi.FIELD_ATTRACTOR)
                if len(att):                                   # (an arm without a goal block ignores its row)
                    self.fields["p"][b, att[0], :12] = g[j, :12]
            for rows, type_, width, skip in classes:
                if rows is None:
                    continue
                r = rnd(rows.reshape(n_arms, rows.shape[1], -1))
                idx = self._class_rows(b, type_, skip)
                for k in range(min(len(idx), r.shape[1])):     # (rows at or beyond the arm's count are ignored)
                    if not np.isnan(r[j, k, 0]):
                        self.fields["p"][b, idx[k], :width] = r[j, k, :width]

    def move_fields_host(self, goal=None, repellers=None, first_arm=0):
        self.move_scene_host(goal=goal, repellers=repellers, first_arm=first_arm)

    # -- the rest --
    def set_ext_cmd(self, channel, cmd):
        if channel < 2 or channel >= _abi.MIX_CHANNELS:
            raise VfikError("only channels 2..5 are external")
        self.ext[channel - 2] = 0.0 if cmd is None else self.rnd(cmd)

    def reset_state(self):
        self.states = self.oc.new_states(self.B, self.n)

    def set_small_batch_kernel(self, max_batch):
        self.small_batch = int(max_batch)        # changes no value, only the launch

    # -- the oracle's answer --
    def groups(self):
        """[(vfik_params, arms)]: the oracle takes one vfik_params per call, so one call per set of arms whose wy, wq, mixer row, limiter
        speed and speed scale are equal"""
        key = np.concatenate([self.wy, self.wq, self.bridge_rows(), self.speed[:, None]], axis=1)
        uniq, inv = np.unique(key, axis=0, return_inverse=True)
        inv = inv.reshape(-1)
        n = self.n
        return [(copy_params(self.params, wy=row[:6], wq=row[6:6 + n], mix_w=row[6 + n:12 + n], max_vel=row[12 + n], speed_scale=row[13 + n]),
                 inv == g) for g, row in enumerate(uniq)]

    def loop_in_kernel(self):
        """include/vfik.h, vfik_rollout: all cycles run inside one kernel, q in double between them, on chains of up to 7 revolute joints
        (every such chain of the suite: tests/test_kconst.py) with the identity tool and unit IK weights on every arm; every other handle
        hands q from cycle to cycle in the I/O type.
        The handle decides by REPRESENTATION, not by value: a per-arm tool image or a per-arm weight image makes the rollout stepped
        whatever it holds.  This method reads values, and the two agree only because the palettes below never offer a per-arm tool row
        that is the identity or a per-arm weight row of ones (tool_frame(0) goes in as the shared tool alone; WY_ROWS[0] and wq_row(n, 0)
        only through vfik_params): a palette that did would need a representation bit here."""
        return bool(self.n <= 7 and np.all(self.tool == np.eye(4).reshape(16)) and np.all(self.wy == 1.0) and np.all(self.wq == 1.0))

    def reference(self, q, want, ctrl=None, active=None, q_lo=None, q_hi=None, rollout=None):
        """The C oracle's rows named in `want` (float64) for the model's state, the sign memory advanced.  ctrl: /nullspace/control (B, 4); active: the launch's gate (the
        rows of silent arms are zeros here).  rollout = (K, dt, clamp) or (K, dt, clamp, stride): the oracle stepped K times with
        q += dt * qdot_out and the clamp if asked, q rounded to the I/O type behind every block of `stride` cycles (K without it), as
        tests/timed_reference.py does it, and behind every cycle on a handle whose rollouts are single-cycle launches (loop_in_kernel); the
        rows are the last cycle's, status ORs, and "q" holds the joint angles afterwards."""
        B, n = self.B, self.n
        q = self.rnd(q)
        act = np.ones(B, dtype=bool) if active is None else (np.asarray(active) != 0)
        K, dt, clamp = (1, 0.0, False) if rollout is None else rollout[:3]
        stride = K if rollout is None or len(rollout) < 4 else rollout[3]
        keys = tuple(sorted((set(want) | {"qdot_out", "status"}) - {"q"}))
        lo = self.chain.q_lo if q_lo is None else self.rnd(q_lo)
        hi = self.chain.q_hi if q_hi is None else self.rnd(q_hi)
        groups = [(p, sel & act) for p, sel in self.groups()]
        shapes = {"qdot_vf": (B, n), "qdot_null": (B, n), "qdot_out": (B, n), "pose": (B, 16), "pose_nt": (B, 16), "v6": (B, 6), "qdist": (B, n)}
        rows = {k: np.zeros(shapes[k]) for k in keys if k != "status"}
        rows["status"] = np.zeros(B, dtype=np.int32)
        status = np.zeros(B, dtype=np.int32)
        qb = q.copy()
        nc = None if ctrl is None else self.rnd(ctrl)
        watch = getattr(self, "sign_watch", None)
        if watch is not None:
            watch.begin()
        for c in range(K):
            for p, sel in groups:
                if sel.any():
                    self.oc.cycle_batch(self.chain, p, qb, self.fields, self.counts, tool=self.tool, null_control=nc, ext_cmd=self.ext, states=self.states,
                                        want=keys, q_lo=None if q_lo is None else lo, q_hi=None if q_hi is None else hi,
                                        active=sel.astype(np.int32), into=rows)
            status |= np.where(act, rows["status"], 0)
            if watch is not None:
                watch.cycle(act)
            if rollout is not None:
                qn = qb + dt * rows["qdot_out"]
                if clamp:
                    qn = np.clip(qn, lo, hi)
                qb = np.where(act[:, None], qn, qb)
                if (c + 1) % stride == 0 or not self.loop_in_kernel():
                    qb = self.rnd(qb)
        out = {k: rows[k] for k in keys}
        out["status"] = status
        out["q"] = qb
        return out


class SignWatch:
    """The condition under which a sign memory can be compared at all: behind EVERY cycle the oracle runs for a 7-joint model (each cycle of
    a rollout and of a goto block too), the normalised dot product of an arm's previous and new null vector.  `worst` is the smallest
    magnitude seen; near 0 the sign decision is a tie that float32 storage of the vector (d_lastvec) may decide the other way."""
    STATE = np.dtype([("lastvec", "<f8", (_abi.MAX_JOINTS * _abi.MAX_JOINTS,)), ("sig", "<i4", (_abi.MAX_JOINTS,))])

    def __init__(self, model):
        assert model.n == 7 and C.sizeof(model.oc.State) == self.STATE.itemsize
        self.model, self.worst, self.prev = model, 1.0, None
        model.sign_watch = self

    def vectors(self):
        return np.frombuffer(bytes(self.model.states), dtype=self.STATE)["lastvec"][:, :7].copy()

    def begin(self):
        self.prev = self.vectors()      # (read again at every launch: vfik_reset_state replaces the states)

    def cycle(self, act):
        new = self.vectors()
        a, b = np.linalg.norm(self.prev, axis=1), np.linalg.norm(new, axis=1)
        had = act & (a > 0) & (b > 0)
        if had.any():
            self.worst = min(self.worst, float((np.abs(np.sum(self.prev * new, axis=1)[had]) / (a * b)[had]).min()))
        self.prev = new


# ---- operations and checkpoints -------------------------------------------------------------------------------------------------------
class Op:
    """One Engine / Model call: name(*args, **kw).  kind: what the coverage counts; range_kind: the range it names; refused: it must raise
    VfikError and change nothing; changes: it changes a value some launch reads; needs: flags under which it can matter (0: any)."""

    def __init__(self, name, args=(), kw=None, kind=None, range_kind=None, refused=False, changes=True, needs=0, note=""):
        self.name, self.args, self.kw = name, tuple(args), dict(kw or {})
        self.kind, self.range_kind, self.refused, self.changes, self.needs, self.note = kind or name, range_kind, refused, changes, needs, note

    def __repr__(self):
        return "%s[%s%s%s]" % (self.kind, self.range_kind or "-", " refused" if self.refused else "", (" " + self.note) if self.note else "")


def apply(target, op):
    """the operation on a Model or an Engine; True when it was accepted"""
    try:
        getattr(target, op.name)(*op.args, **op.kw)
    except VfikError:
        return False
    return True


Check = collections.namedtuple("Check", "form q ctrl active q_lo q_hi")
FORMS = ("lean", "publish", "gate", "limits", "rollout", "goto")
FORM_WEIGHTS = (3, 3, 2, 1, 2, 1)
Step = collections.namedtuple("Step", "op check")


def launch(eng, ck, sentinel=None):
    """The checkpoint's launch on an Engine.  Returns the outputs by name; "q" with the rollout forms."""
    if ck.form == "lean":
        return eng.step_host(ck.q, null_control=ck.ctrl, want=("qdot_out", "status"))
    if ck.form == "publish":
        return eng.step_host(ck.q, null_control=ck.ctrl, want=ALL_ROWS)
    if ck.form == "gate":
        return eng.step_host(ck.q, null_control=ck.ctrl, want=ALL_ROWS, active=ck.active, into=sentinel)
    if ck.form == "limits":
        return eng.step_host(ck.q, null_control=ck.ctrl, want=("qdot_out", "qdot_null", "qdist", "status"), q_lo=ck.q_lo, q_hi=ck.q_hi)
    if ck.form == "rollout":
        return eng.rollout_host(ck.q, ROLL_K, ROLL_DT, null_control=ck.ctrl, clamp=True, want=("qdot_out", "status"))
    # precision (0, 0): both compares of the arrival rule are strict, so no arm arrives and every arm takes every cycle
    r = eng.goto_host(ck.q, GOTO_CYCLES, ROLL_DT, (0.0, 0.0), stride=GOTO_STRIDE, hold=False, want=("qdot_out", "status"), null_control=ck.ctrl)
    return {k: r[k] for k in ("qdot_out", "status", "q")}


def expect(model, ck):
    """... and the model's answer for it"""
    if ck.form == "lean":
        return model.reference(ck.q, ("qdot_out", "status"), ctrl=ck.ctrl)
    if ck.form == "publish":
        return model.reference(ck.q, ALL_ROWS, ctrl=ck.ctrl)
    if ck.form == "gate":
        return model.reference(ck.q, ALL_ROWS, ctrl=ck.ctrl, active=ck.active)
    if ck.form == "limits":
        return model.reference(ck.q, ("qdot_out", "qdot_null", "qdist", "status"), ctrl=ck.ctrl, q_lo=ck.q_lo, q_hi=ck.q_hi)
    if ck.form == "rollout":
        return model.reference(ck.q, ("qdot_out", "status", "q"), ctrl=ck.ctrl, rollout=(ROLL_K, ROLL_DT, True))
    return model.reference(ck.q, ("qdot_out", "status", "q"), ctrl=ck.ctrl, rollout=(GOTO_CYCLES, ROLL_DT, False, GOTO_STRIDE))


def chain_of(cfg):
    from vfclik_amd import robots
    from vfclik_amd.chain import Chain
    if cfg.chain == "chain10":
        import kernel_variants
        return kernel_variants.chain10(robots, Chain)
    return robots.by_name(cfg.chain)


# palettes: every per-arm bridge, speed and weight value is exact in float32, so that the groups stay few and no rounding hides in them.
# Per-arm IK weight rows come from index 1 and 2 only, per-arm tools from tool_frame(1..3) only: see Model.loop_in_kernel.
SPEEDS = (0.5, 0.75, 1.0, 1.25)
MAX_VELS = (0.25, 0.5, 0.75, 1.0)
MIX_ROWS = ((1.0, 1.0, 0.0, 0.0, 0.0, 0.0), (1.0, 0.5, 0.25, 0.0, 0.0, 0.0), (0.5, 1.0, 0.25, 0.5, 0.0, 0.0), (0.75, 0.25, 0.0, 0.5, 0.0, 0.0))
WY_ROWS = ((1.0, 1.0, 1.0, 1.0, 1.0, 1.0), (1.0, 1.0, 1.0, 0.25, 0.25, 0.25), (0.25, 0.5, 0.25, 1.0, 1.0, 1.0))
LAMBDAS = (0.1, 0.05, 0.2)


def wq_row(n, k):
    return [(1.0,) * n, tuple(1.0 if i % 2 else 0.25 for i in range(n)), tuple(0.5 if i < n // 2 else 1.0 for i in range(n))][k]


def tool_frame(k):
    """tools whose translations (and rotation entries) are NOT float32 numbers: the rounding rules of vfik_set_tool have something to round"""
    if k == 0:
        return np.eye(4).reshape(16)
    a, t = (0.3, (0.0123456789, -0.02000000011, 0.1234567891)) if k == 1 else ((-0.7, (0.05000000013, 0.0300000007, 0.0800000003)) if k == 2
                                                                                  else (1.1, (-0.0400000009, 0.0100000003, 0.1500000001)))
    T = np.eye(4)
    T[:3, :3] = [[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]]
    T[:3, 3] = t
    return T.reshape(16)


AMP_ARM = 17     # the arm of the "one" range


def ranges(B):
    """the four range kinds: (first_arm, n_arms)"""
    return {"whole": (0, B), "one": (AMP_ARM, 1), "cross": (60, 11), "last": (B - 1, 1)}


class OpMaker:
    """The operations of a walk, each built from the generator's own copy of the state (`m`: moves start from where things are, the amplifier
    stands where the tool is), the vfik_params passed last (`cur`) and the walk's random stream."""

    def __init__(self, oc, seed, cfg):
        import zlib

        from vfclik_amd import synth
        self.cfg, self.chain = cfg, chain_of(cfg)
        chain = self.chain
        self.B, self.n, self.io = cfg.B, chain.n, np.dtype(cfg.io_dtype)
        self.rng = np.random.default_rng([seed, zlib.crc32(cfg.name.encode())])
        w = synth.make_workload(chain, self.B, 0, seed=100 + seed, io_dtype=self.io.type)
        self.goals = w["fields"]["p"][:, 0, :16].copy()
        self.q0 = np.clip(w["q"], 0.9 * chain.q_lo, 0.9 * chain.q_hi)
        self.tips = chain.fk(self.q0).reshape(self.B, 16)[:, [3, 7, 11]]
        self.params0 = _abi.default_params(flags=F_NS | F_MIX, max_vel=1.0)
        self.m = Model(oc, chain, self.B, self.io, cfg.max_slots, self.params0)
        self.cur = dict(speed_scale=1.0, max_vel=1.0, wy=WY_ROWS[0], wq=wq_row(self.n, 0), mix_w=MIX_ROWS[0], flags=F_NS | F_MIX, **{"lambda": 0.1})
        self.R = ranges(self.B)
        self.q_now = None          # the joint angles of the checkpoint behind the operation being made

    def pick_range(self):
        return ("whole", "one", "cross", "last")[self.rng.integers(4)]

    def other(self, palette, now, weights=None):
        c = [v for v in palette if v != now]
        if weights is None:
            return c[self.rng.integers(len(c))]
        p = np.array([wt for v, wt in zip(palette, weights) if v != now], dtype=float)
        return c[self.rng.choice(len(c), p=p / p.sum())]

    def fields(self, family, rk, n_rep=None, refused=False, note=None):
        first, cnt = self.R[rk]
        f, c = records([scene(family, self.goals[first + j], self.tips[first + j], self.rng, n_rep) for j in range(cnt)])
        return Op("set_fields", (f, c), dict(first_arm=first), kind="refused_too_many" if refused else "set_fields", range_kind=rk,
                  refused=refused, note=note or family)

    def move_before_set(self):
        g0 = np.tile(np.eye(4).reshape(16), (self.B, 1))
        return Op("move_fields_host", kw=dict(goal=g0), kind="refused_move_before_set", range_kind="whole", refused=True)

    def refusal(self, kind):
        if kind == "too_many":
            return self.fields("too_many", "cross", refused=True, note="17 slots")
        if kind == "weight_nan":
            wy = np.tile(WY_ROWS[1], (11, 1))
            wy[5, 2] = np.nan
            return Op("set_arm_weights", (), dict(wy=wy, first_arm=60), kind="refused_weight", range_kind="cross", refused=True)
        if kind in ("speed_negative", "speed_nan"):
            v = np.full(11, 0.5)
            v[3] = -0.25 if kind == "speed_negative" else np.nan
            return Op("set_speed_scale", (v,), dict(first_arm=60), kind="refused_" + kind, range_kind="cross", refused=True)
        return Op("set_max_vel", (np.full(11, 0.5),), dict(first_arm=self.B - 5), kind="refused_range", refused=True)

    def params(self, what, val=None):
        cur, n = self.cur, self.n
        if what == "same":
            return Op("set_params", kw=dict(cur), kind="set_params:same", changes=False)
        if val is None:
            val = {"flags": lambda: self.other(FLAG_SETS, cur["flags"], (1, 2, 3, 6, 2)), "lambda": lambda: self.other(LAMBDAS, cur["lambda"]),
                   "speed_scale": lambda: self.other(SPEEDS, cur["speed_scale"]), "wq": lambda: self.other([wq_row(n, k) for k in range(3)], cur["wq"]),
                   "wy": lambda: self.other(WY_ROWS, cur["wy"]), "max_vel": lambda: self.other(MAX_VELS, cur["max_vel"]),
                   "mix_w": lambda: self.other(MIX_ROWS, cur["mix_w"])}[what]()
        changes = cur[what] != val
        cur[what] = val
        return Op("set_params", kw=dict(cur), kind="set_params:" + what, needs={"max_vel": F_LIM, "mix_w": F_MIX}.get(what, 0), changes=changes)

    def params_many(self, **vals):
        """one vfik_set_params call that changes several members"""
        self.cur.update(vals)
        return Op("set_params", kw=dict(self.cur), kind="set_params:many", note=",".join(sorted(vals)))

    def weights(self, rk, form, equal):
        first, cnt = self.R[rk]
        rows = lambda pal: np.array([pal[(0 if equal else j % 2) + 1] for j in range(cnt)])  # noqa: E731
        kw = dict(first_arm=first)
        if form in ("wy", "both"):
            kw["wy"] = rows(WY_ROWS)
        if form in ("wq", "both"):
            kw["wq"] = rows([wq_row(self.n, k) for k in range(3)])
        return Op("set_arm_weights", kw=kw, range_kind=rk, note=form + (" equal" if equal else ""))

    def mixer(self, rk, row=None):
        if rk is None:
            return Op("set_mixer_weights", (None,), kind="set_mixer_weights:none", needs=F_MIX)
        first, cnt = self.R[rk]
        return Op("set_mixer_weights", (np.tile(row, (cnt, 1)),), dict(first_arm=first), range_kind=rk, needs=F_MIX)

    def maxvel(self, rk, v):
        first, cnt = self.R[rk]
        return Op("set_max_vel", (np.full(cnt, v),), dict(first_arm=first), range_kind=rk, needs=F_LIM)

    def speed(self, rk, v):
        first, cnt = self.R[rk]
        return Op("set_speed_scale", (np.full(cnt, v),), dict(first_arm=first), range_kind=rk)

    def ext(self, ch, cmd=True):
        return Op("set_ext_cmd", (ch, self.rng.uniform(-0.2, 0.2, (self.B, self.n)) if cmd else None), needs=F_MIX, range_kind="whole")

    def tool(self, what, k):
        if what == "shared":
            return Op("set_tool", (tool_frame(k),), dict(per_arm=False), kind="set_tool:shared", range_kind="whole")
        return Op("set_tool", (np.tile(tool_frame(k), (self.B, 1)),), dict(per_arm=True), kind="set_tool:per_arm", range_kind="whole", note="equal")

    def small_batch(self):
        return Op("set_small_batch_kernel", (int((0, 4096, 64)[self.rng.integers(3)]),), changes=False)

    def amplifier(self, name):
        """Arm AMP_ARM's goal 0.2 um (float64 I/O: 0.4 mm) in front of where its tool is at this operation's checkpoint, with a slow-down
        distance of 0.5 um (1 mm).  Inside it the attractor's twist is speed * (goal - tip) / slow-down: half a float32 ulp of a tool
        translation or of a goal coordinate, 1e-9 .. 3e-8 m, moves it by 2e-3 .. 6e-2 m/s -- what the rounding rules of vfik_set_tool and
        of the host moves need in order to show.  Every input of the launch is the same float32 number on both sides and the arithmetic
        is float64 on both, so the oracle and a kernel differ there by 1e-15 m / 0.5 um = 2e-9, far under the bar."""
        b = AMP_ARM
        ds, off = (0.5e-6, 0.2e-6) if self.io == np.float32 else (1e-3, 0.4e-3)
        X = self.chain.fk(self.q_now[b:b + 1])[0] @ self.m.tool[b].reshape(4, 4)
        X[0, 3] += off
        if name == "set_fields":
            f, c = records([[_field(1, _abi.FIELD_ATTRACTOR, 1.0, list(X.reshape(16)) + [ds])]])
            return Op("set_fields", (f, c), dict(first_arm=b), range_kind="one", note="amplifier")
        return Op("move_fields_host", kw=dict(goal=X.reshape(1, 16), first_arm=b), range_kind="one", note="amplifier")

    def move(self, kind, rk):
        rng, m = self.rng, self.m
        first, cnt = self.R[rk]
        g = m.fields["p"][first:first + cnt, 0, :16].copy()
        g[:, [3, 7, 11]] += rng.uniform(-0.15, 0.15, (cnt, 3))
        g[m.counts[first:first + cnt] == 0] = np.eye(4).reshape(16)
        if cnt > 1:
            g[1, 0] = np.nan                               # leave that arm's goal
        d = rng.normal(size=(cnt, 3, 3))
        xyz = self.tips[first:first + cnt, None, :] + d / np.linalg.norm(d, axis=2, keepdims=True) * rng.uniform(0.15, 0.35, (cnt, 3, 1))
        reps = np.concatenate([xyz, rng.uniform(0.03, 0.1, (cnt, 3, 1))], axis=2)
        reps[:, 1, 0] = np.nan                             # leave every arm's second repeller
        if kind == "move_fields_host":
            kw = dict(goal=g, repellers=reps, first_arm=first) if rng.integers(2) else dict(goal=g, first_arm=first)
            return Op(kind, kw=kw, range_kind=rk)
        fun = np.concatenate([g[:, [3, 7, 11]] + 0.01, np.tile([0.0, 0.6, 0.8], (cnt, 1))], axis=1)[:, None, :]
        hem = np.tile([0.1, 0.0, -0.15, 0.0, 0.0, 1.0], (cnt, 1))[:, None, :]
        return Op(kind, kw=dict(goal=g, repellers=reps, funnels=fun, hemispheres=hem, attractors=g[:, None, :], first_arm=first), range_kind=rk)

    def draw(self, bridge_is_the_programs):
        """an operation of a drawn kind, with a drawn range and drawn values"""
        rng = self.rng
        kind = ("set_params", "set_params", "set_params", "set_arm_weights", "set_arm_weights", "set_mixer_weights", "set_mixer_weights", "set_max_vel",
                "set_tool", "set_tool", "set_speed_scale", "move_fields_host", "move_fields_host", "move_scene_host", "set_ext_cmd", "reset_state",
                "set_small_batch_kernel")[rng.integers(17)]
        if kind in ("set_mixer_weights", "set_max_vel") and bridge_is_the_programs and not self.m.bridge:
            kind = "set_params"          # (the first per-arm bridge state is the rules program's: it must find vfik_params moved)
        if kind == "set_params":
            return self.params(("flags", "lambda", "speed_scale", "same", "wq", "wy", "max_vel", "mix_w")[rng.integers(8)])
        if kind == "set_arm_weights":
            rk = self.pick_range()
            return self.weights(rk, ("wy", "wq", "both", "both")[rng.integers(4)], rk != "whole" or rng.integers(2) == 0)
        if kind == "set_mixer_weights":
            return self.mixer(None) if rng.integers(3) == 0 else self.mixer(self.pick_range(), MIX_ROWS[1 + rng.integers(3)])
        if kind == "set_max_vel":
            return self.maxvel(self.pick_range(), MAX_VELS[rng.integers(3)])
        if kind == "set_tool":
            what = rng.integers(4)
            if what == 0:
                return self.tool("shared", rng.integers(4))
            t = np.tile(tool_frame(1 + rng.integers(3)), (self.B, 1))
            if what >= 2:                                      # one arm, or every other arm, with another hand
                t[(self.B - 1) if what == 2 else slice(0, self.B, 2)] = tool_frame(1 + rng.integers(3))
            return Op("set_tool", (t,), dict(per_arm=True), kind="set_tool:per_arm", range_kind="whole", note="equal" if what == 1 else "differ")
        if kind == "set_speed_scale":
            return self.speed(self.pick_range(), self.other(SPEEDS, None))
        if kind in ("move_fields_host", "move_scene_host"):
            return self.move(kind, self.pick_range())
        if kind == "set_ext_cmd":
            ch = int((2, 2, 3, 3, 4, 5)[rng.integers(6)])
            return self.ext(ch, cmd=rng.integers(4) != 0)
        if kind == "reset_state":
            return Op("reset_state", needs=F_NS)
        return self.small_batch()


REFUSALS = ("too_many", "weight_nan", "speed_negative", "range", "speed_nan")
# the set_fields program of a walk of 48 operations: every plan, and every flip between plans caused by a call that names a few arms only
FIELDS_PROGRAM = (("feeder", "whole", 3), ("feeder", "cross", 8), ("fewer", "cross", 2),           # ... a drop in slots_used
                  ("pair", "last", None), ("feeder", "last", 3),                                     # uniform -> compact -> uniform
                  ("frac", "one", None), ("fewer", "one", 1),                                        # straight -> general -> straight
                  ("orders", "cross", None), ("normal", "cross", None), ("hemi", "one", None), ("funnel2", "last", None),
                  ("none", "cross", None), ("feeder", "whole", 8))


def rules_program(o):
    """One block of consecutive operations (as callables: each is made when its turn comes): every history-dependent rule of the setters
    (WRONG_RULES, ROUNDING_RULES) met once in the order that makes it matter, under the flags that read the state it leaves."""
    return [lambda: o.params("flags", F_NS | F_MIX | F_LIM),
            lambda: o.params("mix_w", MIX_ROWS[1]), lambda: o.params("max_vel", 0.5), lambda: o.ext(2),
            lambda: o.mixer("cross", MIX_ROWS[2]), lambda: o.maxvel("cross", 0.25),                # the bridge state starts from THOSE values
            lambda: o.speed("cross", 0.5),
            lambda: o.weights("whole", "both", True), lambda: o.weights("last", "wy", True),       # promotion, then wy alone on one arm
            lambda: o.move("move_fields_host", "whole"), lambda: o.move("move_scene_host", "last"),
            lambda: o.fields("fewer", "cross", 2),                                                 # the speed scales and the other arms' moves stay
            lambda: o.params("lambda"),                          # unchanged speed_scale, weights, max_vel and mix_w: the arms' own stay
            lambda: o.params("same"),
            lambda: o.mixer(None),                                                                 # rows back, speeds stay
            lambda: o.params("max_vel", 0.75), lambda: o.mixer("one", MIX_ROWS[3]), lambda: o.params("mix_w", MIX_ROWS[2]), lambda: o.ext(3),
            lambda: o.tool("shared", 1), lambda: o.amplifier("set_fields"),                        # stored as given: the amplifier arm reads it
            lambda: o.tool("equal", 2), lambda: o.amplifier("move_fields_host"),                   # stored rounded; the move rounds its rows
            lambda: o.params("speed_scale"), lambda: o.params("wq"), lambda: o.params("wy"),
            lambda: Op("reset_state", needs=F_NS)]


def schedule_48(o, seed):
    """{operation index: callable}: the walk of 48 operations.  The rules program is one block at a seeded place; the set_fields program (in
    its order), one refused call, the flag sets and one vfik_set_small_batch_kernel stand at seeded places around it; the rest is drawn."""
    rng, cfg = o.rng, o.cfg
    k0 = [c.name for c in CONFIGS].index(cfg.name) + seed
    refusals = [REFUSALS[k0 % 5]]      # (with the move before any vfik_set_fields that every walk starts with: the walks together make each)
    flags = [int(f) for f in rng.permutation([F_MIX, 0, F_NS | F_JL | F_MIX, F_NS | F_MIX | F_LIM])]
    rules = rules_program(o)
    n_prog = len(FIELDS_PROGRAM) - 1
    start = int(rng.integers(2, cfg.n_ops - len(rules) + 1))
    at = dict(zip(range(start, start + len(rules)), rules))
    free = np.array([i for i in range(2, cfg.n_ops) if i not in at])
    rest = np.sort(rng.choice(free, size=n_prog + len(refusals) + len(flags) + 1, replace=False))
    slots = rng.permutation(len(rest))
    for i, (fam, rk, k) in zip(sorted(rest[slots[:n_prog]].tolist()), FIELDS_PROGRAM[1:]):
        at[i] = lambda fam=fam, rk=rk, k=k: o.fields(fam, rk, k)
    for i, kind in zip(rest[slots[n_prog:n_prog + len(refusals)]].tolist(), refusals):
        at[i] = lambda kind=kind: o.refusal(kind)
    for i, f in zip(rest[slots[n_prog + len(refusals):]].tolist(), flags + [-1]):
        at[i] = (lambda f=f: o.params("flags", f)) if f >= 0 else o.small_batch
    at[0], at[1] = o.move_before_set, lambda: o.fields(*FIELDS_PROGRAM[0])
    return at


def schedule_16(o, seed):
    """{operation index: callable}: the walk of 16 operations, in a fixed order.  Sixteen operations do not hold the whole rules program, so
    the two seeds share it: one walk takes the bridge state and the speed scales, the other the IK weights, the moves, the tools and the
    amplifier; each keeps the set_fields calls that flip the batch uniform -> compact -> uniform -> general -> straight, of which the
    calls on arms 60..70 are also the ones the rules need (the speed scale stays, the other arms' moves stay)."""
    k0 = [c.name for c in CONFIGS].index(o.cfg.name) + seed
    first = [o.move_before_set, lambda: o.fields("feeder", "whole", 8)]
    if seed % 2:
        return dict(enumerate(first + [
            lambda: o.params_many(flags=F_NS | F_MIX | F_LIM, mix_w=MIX_ROWS[1], max_vel=0.5),
            lambda: o.fields("pair", "last"),
            lambda: o.mixer("cross", MIX_ROWS[2]), lambda: o.maxvel("cross", 0.25),               # the bridge state starts from THOSE values
            lambda: o.fields("feeder", "last", 2),
            lambda: o.speed("cross", 0.5),
            lambda: o.fields("frac", "cross"),                                                    # the speed scale stays
            lambda: o.params("lambda"),                                      # unchanged speed_scale, max_vel and mix_w: the arms' own stay
            lambda: o.mixer(None),                                                                # rows back, speeds stay
            lambda: o.refusal(REFUSALS[k0 % 5]),
            lambda: o.params_many(max_vel=0.75, mix_w=MIX_ROWS[2], speed_scale=0.75),             # changed: every arm's
            lambda: o.fields("fewer", "cross", 2)]))
    return dict(enumerate(first + [
        lambda: o.weights("whole", "both", True), lambda: o.weights("last", "wy", True),          # promotion, then wy alone on one arm
        lambda: o.fields("pair", "last"),
        lambda: o.params("lambda"),                                                               # unchanged weights leave both
        lambda: o.params("wq"),                                                                   # changed: every arm's
        lambda: o.fields("feeder", "last", 2),
        lambda: o.move("move_fields_host", "whole"),
        lambda: o.fields("frac", "cross"),                                                        # the other arms' moves stay
        lambda: o.tool("shared", 1), lambda: o.amplifier("set_fields"),                           # stored as given
        lambda: o.tool("equal", 2), lambda: o.amplifier("move_fields_host"),                      # stored rounded; the move rounds its rows
        lambda: o.fields("fewer", "cross", 2),
        lambda: o.refusal(REFUSALS[k0 % 5])]))


def walk(oc, seed, cfg):
    """The walk of one configuration and seed: (chain, params the handle is created with, [Step])."""
    o = OpMaker(oc, seed, cfg)
    rng, chain, B, n, io = o.rng, o.chain, o.B, o.n, o.io
    at = schedule_48(o, seed) if cfg.n_ops >= 48 else schedule_16(o, seed)
    phase = rng.uniform(0.0, 2.0 * np.pi, (B, n))
    steps = []
    for i in range(cfg.n_ops):
        # the joint angles follow a slow loop around the regular start poses: at most 0.05 * 2 pi / 24 = 0.013 rad a step in any joint
        q = np.clip(o.q0 + 0.05 * np.sin(2.0 * np.pi * i / 24.0 + phase), 0.9 * chain.q_lo, 0.9 * chain.q_hi)
        q = q.astype(io).astype(np.float64)
        o.q_now = q
        op = at[i]() if i in at else o.draw(bridge_is_the_programs=cfg.n_ops >= 48)
        assert apply(o.m, op) != op.refused, op
        form = FORMS[rng.choice(len(FORMS), p=np.array(FORM_WEIGHTS) / float(sum(FORM_WEIGHTS)))]
        active = q_lo = q_hi = None
        if form == "gate":
            active = (rng.integers(0, 3, B) > 0).astype(np.int32)
            active[0], active[1], active[AMP_ARM] = 1, 0, 1
        if form == "limits":
            s = rng.uniform(0.93, 1.0, (B, 1))
            q_lo, q_hi = (s * chain.q_lo).astype(io).astype(np.float64), (s * chain.q_hi).astype(io).astype(np.float64)
        # /nullspace/control: without it no output reads the sign memory.  Only where the nullspace has one dimension (include/vfik.h,
        # vfik_io.null_control): with two and more the reference moves along a basis that cannot be restated, and the C oracle does so too
        ctrl = rng.uniform(-1.0, 1.0, (B, _abi.NULL_CONTROLS)).astype(io).astype(np.float64) if n == 7 else None
        steps.append(Step(op, Check(form, q, ctrl, active, q_lo, q_hi)))
    return chain, o.params0, steps
