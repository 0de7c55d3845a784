"""The timed moves under a coupling AND an avoid rule (include/vfik.h: vfik_set_avoid_rule) restated on the host: coupled_reference's
oracle-stepped move with the push in front of every block.

The route is clearance_reference's.  `Avoiding` wraps the oracle object INSIDE a coupled_reference.Coupled, which calls its `cycle_batch`
right after it placed the partner's spheres for the block.  At a block's first cycle -- q is then the block's input row, I/O-typed, gated
and held arms carrying the row they hold -- it computes every arm's command on the host in float64 (hp_avoid.host_avoid: the law as
written, own spheres and joint frames from Chain.fk of the truncated chains, the partner's rows as Coupled rounded them), rounds it to
the I/O type, keeps it as avoid_traj[k], and adds it to `ext_cmd[channel - 2]` of every cycle of the block: the mixer channel the device
writes.  Beside it, for the tests' scene conditions only, the arm's clearance in front of the block (hp_clearance.host_clearance).
`timed_reference.py`, `coupled_reference.py` and `clearance_reference.py` are untouched.

A helper of the suite, not a conftest.py: tests/test_avoid_moves_reference.py checks it on the CPU, tests/test_gpu_avoid_moves.py holds the
GPU to it."""
import numpy as np

import coupled_reference as cr
import hp_avoid as ha
import hp_clearance as hc
import timed_reference as tr
from vfclik_amd import _abi


class Avoiding:
    """The oracle object with the avoid rule in front of every block's first cycle; everything else of `oc` passes through.  `coupled` is
    set by the caller: its link_traj[k] are the partner's rows of block k."""

    def __init__(self, oc, chain, spheres, gain, d0, channel, scale, mask, stride, n_checks, io_dtype):
        self.oc, self.chain, self.spheres, self.stride, self.n_checks, self.io_dtype = oc, chain, list(spheres), int(stride), n_checks, io_dtype
        self.gain, self.d0, self.channel, self.mask = float(gain), float(d0), int(channel), mask
        self.scale = None if scale is None else np.asarray(scale, dtype=np.float64).astype(io_dtype).astype(np.float64)
        self.coupled = None
        self.cycles = 0
        self.last_ext = None
        self.cmd = None

    def __getattr__(self, name):
        return getattr(self.oc, name)

    def cycle_batch(self, chain, params, q, fields, nfields, **kw):
        # `_run` makes one ext_cmd array per cycle and hands the same one to every controller group: a new array is a new cycle
        new_cycle = kw.get("ext_cmd") is None or kw["ext_cmd"] is not self.last_ext
        self.last_ext = kw.get("ext_cmd")
        if new_cycle and self.cycles % self.stride == 0:
            k = self.cycles // self.stride
            B, L = q.shape[0], len(self.spheres)
            if self.cmd is None:
                self.avoid_traj = np.full((self.n_checks, B, chain.n), np.nan)
                self.clear_traj = np.full((self.n_checks, B), np.nan)
            rows = self.coupled.link_traj[k]
            self.cmd = ha.host_avoid(self.chain, self.spheres, q, rows, 0, L, self.mask, self.gain, self.d0, self.scale)
            self.cmd = self.cmd.astype(self.io_dtype).astype(np.float64)
            self.avoid_traj[k] = self.cmd
            self.clear_traj[k] = hc.host_clearance(self.chain, self.spheres, q, rows, 0, L, self.mask)[0]
        self.cycles += int(new_cycle)
        ext = np.array(kw["ext_cmd"], dtype=np.float64, copy=True) if kw.get("ext_cmd") is not None else np.zeros((4,) + q.shape)
        ext[self.channel - 2] += self.cmd
        kw["ext_cmd"] = ext
        return self.oc.cycle_batch(chain, params, q, fields, nfields, **kw)


class CoupledPerCycle(cr.Coupled):
    """coupled_reference.Coupled for a move whose cycles may take SEVERAL cycle_batch calls (a script's controller groups: arms on a frame
    step and arms on a posture step run under different mixer rows).  The first call of a cycle -- told by its ext_cmd array, as above --
    goes through Coupled, which counts it and places the partner's spheres at a block's first cycle; the others go straight on."""
    last_ext = None

    def cycle_batch(self, chain, params, q, fields, nfields, **kw):
        new_cycle = kw.get("ext_cmd") is None or kw["ext_cmd"] is not self.last_ext
        self.last_ext = kw.get("ext_cmd")
        if new_cycle:
            return super().cycle_batch(chain, params, q, fields, nfields, **kw)
        return self.oc.cycle_batch(chain, params, q, fields, nfields, **kw)


def _wrap(oc, chain, coupling, rule, stride, n_cycles, io_dtype, per_cycle=False):
    a = Avoiding(oc, chain, coupling["spheres"], rule["gain"], rule["d0"], rule.get("channel", 4), rule.get("scale"), rule.get("mask"), stride,
                 n_cycles // stride, io_dtype)
    c = cr._coupled(a, chain, coupling, stride, n_cycles, io_dtype)
    if per_cycle:
        c.__class__ = CoupledPerCycle
    a.coupled = c
    return a, c


def _finish(r, a, c, n_cycles):
    r["link_traj"] = c.done(n_cycles)
    r["avoid_traj"], r["clear_traj"] = a.avoid_traj, a.clear_traj
    r["closest"] = r["closest_c"]
    return r


def goto(oc, chain, params, q0, fields, nfields, n_cycles, stride, dt, precision, coupling, rule, io_dtype=np.float64, **kw):
    """coupled_reference.goto under rule = dict(gain, d0, channel, scale, mask).  Returns its dict with avoid_traj (n_checks, B, n), the
    I/O-typed command of every block, and clear_traj (n_checks, B), the float64 clearance in front of it."""
    a, c = _wrap(oc, chain, coupling, rule, stride, n_cycles, io_dtype)
    r = tr.goto(c, chain, params, q0, fields, nfields, n_cycles, stride, dt, precision, io_dtype=io_dtype, **kw)
    return _finish(r, a, c, n_cycles)


def follow(oc, chain, params, q0, fields, nfields, way, n_cycles, stride, dt, precision, coupling, rule, via_precision=None,
           io_dtype=np.float64, **kw):
    """coupled_reference.follow under a rule; as goto."""
    a, c = _wrap(oc, chain, coupling, rule, stride, n_cycles, io_dtype)
    r = tr.follow(c, chain, params, q0, fields, nfields, way, n_cycles, stride, dt, precision, via_precision, io_dtype=io_dtype, **kw)
    return _finish(r, a, c, n_cycles)


def script(oc, chain, params, q0, fields, nfields, kind, way, wayq, n_cycles, stride, dt, precision, js_precision, coupling, rule,
           io_dtype=np.float64, **kw):
    """timed_reference.script under a coupling and a rule: the script's own mixer rows 0..3, weights 4 and 5 from params -- the rule's
    channel keeps its weight over frame and posture steps alike.  As goto; closest is the smaller of closest_c and closest_j."""
    a, c = _wrap(oc, chain, coupling, rule, stride, n_cycles, io_dtype, per_cycle=True)
    r = tr.script(c, chain, params, q0, fields, nfields, kind, way, wayq, n_cycles, stride, dt, precision, js_precision, io_dtype=io_dtype, **kw)
    r = _finish(r, a, c, n_cycles)
    r["closest"] = np.minimum(r["closest_c"], r["closest_j"])
    return r


# ---- the scene of tests/test_gpu_avoid_moves.py ---------------------------------------------------------------------------------------
# coupled_reference.pair_case scenes, every handle with the nullspace module and the mixer, mix_w[4] = 1: the rule writes channel 4.
MIX_W = (1.0, 1.0, 0.0, 0.0, 1.0, 0.0)
MOVES = {"goto64": dict(robot="lwr", B=203, io_dtype=np.float64, stride=1, hold=False, flags=_abi.F_NULLSPACE | _abi.F_MIXER, seed=9),
         "goto32": dict(robot="lwr", B=203, io_dtype=np.float32, stride=4, hold=True, flags=_abi.F_NULLSPACE | _abi.F_MIXER, seed=9),
         "follow": dict(robot="lwr_dual14", B=130, io_dtype=np.float64, stride=4, hold=True, seed=9, n_way=3,
                        flags=_abi.F_NULLSPACE | _abi.F_JOINT_LIMIT_TASK | _abi.F_MIXER)}
# gain and d0 per move, chosen on the CPU from the ORACLE's run so that the three conditions of `conditions` hold (asserted on the
# reference's run by both tests).  d0 in metres of room between an arm's spheres and its partner's; with gain 0.4 a pair half way into d0
# pushes a joint half a metre away with 0.1 rad/s, a seventh of the limiter's 0.7.
RULE = {"goto64": dict(gain=0.4, d0=0.12), "goto32": dict(gain=0.4, d0=0.12), "follow": dict(gain=0.4, d0=0.15)}
CHANNEL = 4
_CACHE = {}


def reference(oc, name, gain=None):
    """(case, params, result) of MOVES[name] under RULE[name] (gain: another gain -- 0 is the coupled move with a rule that never pushes);
    computed once per process and never modified."""
    key = (name, gain)
    if key not in _CACHE:
        from vfclik_amd import robots
        m = MOVES[name]
        chain = robots.by_name(m["robot"])
        c = cr.pair_case(chain, m["B"], m["io_dtype"], seed=m["seed"], n_way=m.get("n_way", 0))
        c["chain"] = chain
        params = _abi.default_params(flags=m["flags"], max_vel=0.7, mix_w=MIX_W)
        kw = dict(hold=m["hold"], clamp=True, io_dtype=m["io_dtype"], stepped=chain.n > 7, want=("qdot_out",))
        args = (oc, chain, params, c["q0"], c["w"]["fields"], c["w"]["nfields"])
        coup = dict(spheres=c["spheres"], src_arm=c["src_arm"], xform=c["xform"], first_rep=c["first_rep"])
        rule = dict(RULE[name], channel=CHANNEL)
        if gain is not None:
            rule["gain"] = gain
        if c["way"] is None:
            r = goto(*args, cr.N_CYCLES, m["stride"], cr.DT, cr.PREC, coup, rule, **kw)
        else:
            r = follow(*args, c["way"], cr.N_CYCLES, m["stride"], cr.DT, cr.PREC, coup, rule, **kw)
        for v in list(r.values()) + [c["q0"], c["xform"], c["src_arm"], c["w"]["fields"], c["w"]["nfields"]]:
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _CACHE[key] = (c, params, r)
    return _CACHE[key]


def conditions(r, r_off):
    """The scene's three conditions on a run and on the same move with gain 0: (arms that carry a nonzero command in some block, arms
    that carry none in any block, arms whose smallest clearance over the move is larger with the rule than without)."""
    pushed = np.any(np.nan_to_num(r["avoid_traj"]) != 0, axis=(0, 2))
    with np.errstate(invalid="ignore"):
        lo_on, lo_off = np.nanmin(r["clear_traj"], axis=0), np.nanmin(r_off["clear_traj"], axis=0)
        wider = np.isfinite(lo_on) & np.isfinite(lo_off) & (lo_on > lo_off)
    return int(np.count_nonzero(pushed)), int(np.count_nonzero(~pushed)), int(np.count_nonzero(wider))


# ---- one script under the rule: a posture, then two frames --------------------------------------------------------------------------------
SCRIPT = dict(robot="lwr", B=203, io_dtype=np.float64, stride=4, hold=True, flags=_abi.F_NULLSPACE | _abi.F_MIXER, seed=9, gain=0.4, d0=0.12)
JS_PREC, JS_VIA = 0.02, 0.06


def script_case(chain):
    """coupled_reference.pair_case with two waypoints as a script of three steps: the posture q0 + 0.08 rad in every joint, the frame half
    way to the goal, the goal.  Arm 8 has no script (pair_case ends its list at once), arm 5's ends behind the posture."""
    m = SCRIPT
    c = cr.pair_case(chain, m["B"], m["io_dtype"], seed=m["seed"], n_way=2)
    B, n = c["q0"].shape
    way = np.concatenate([np.zeros((B, 1, 16)), c["way"]], axis=1)
    wayq = np.zeros((B, 3, n))
    wayq[:, 0] = np.clip(c["q0"] + 0.08, chain.q_lo, chain.q_hi)
    kind = np.tile(np.array([tr.POSTURE, tr.FRAME, tr.FRAME], dtype=np.int32), (B, 1))
    kind[8, :] = 0
    kind[5, 1:] = 0
    c.update(chain=chain, kind=kind, way3=np.nan_to_num(way), wayq=wayq)
    return c


def script_reference(oc):
    """(case, params, result, result with gain 0) of the script; computed once per process and never modified."""
    if "script" not in _CACHE:
        from vfclik_amd import robots
        m = SCRIPT
        chain = robots.by_name(m["robot"])
        c = script_case(chain)
        params = _abi.default_params(flags=m["flags"], max_vel=0.7, mix_w=MIX_W)
        coup = dict(spheres=c["spheres"], src_arm=c["src_arm"], xform=c["xform"], first_rep=c["first_rep"])
        n = chain.n
        runs = []
        for gain in (m["gain"], 0.0):
            runs.append(script(oc, chain, params, c["q0"], c["w"]["fields"], c["w"]["nfields"], c["kind"], c["way3"], c["wayq"], cr.N_CYCLES,
                               m["stride"], cr.DT, cr.PREC, np.full(n, JS_PREC), coup, dict(gain=gain, d0=m["d0"], channel=CHANNEL),
                               js_via_precision=np.full(n, JS_VIA), io_dtype=m["io_dtype"], hold=m["hold"], clamp=True, want=("qdot_out",)))
        for r in runs:
            for v in r.values():
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)
        _CACHE["script"] = (c, params, runs[0], runs[1])
    return _CACHE["script"]
