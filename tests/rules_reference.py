"""The five timed moves with EVERY rule of the handle switched on -- the coupling (include/vfik.h: vfik_set_coupling), the wait rule
(vfik_set_wait_rule), the avoid rule (vfik_set_avoid_rule) and the stall rule (vfik_set_stall_rule) -- restated on the host: the three
wrappers of the suite stacked around the oracle in the order the device's loop applies them in front of every block,

    coupled_reference.Coupled      outermost: places the partner's spheres, keeps link_traj[k]
    clearance_reference.Waiting    measures the clearance against those rows, clears the gate of the arms that wait, narrows `active`
    avoid_reference.Avoiding       computes every arm's push against those rows -- a waiting arm's too: it is traced, and never taken,
                                   because the oracle does not evaluate an arm that is not active -- and adds it to the rule's channel
    the oracle

and the stall rule where it always was: a timed_reference.Rule inside timed_reference._run's state machine, which meets only the arms
that ran the block.  Any rule can be absent; without a rule the stack is the wrapper that is left.  Nothing of the loop is repeated: the
five forms call `timed_reference._run` with the handle's (or the script's) mixer wrapped by `Waiting.mixer`, the way
clearance_reference.goto does, and a script tells its cycles apart by avoid_reference's rule -- a new ext_cmd array is a new cycle --
in all three wrappers.

A helper of the suite, not a conftest.py: tests/test_rules_reference.py checks it on the CPU, tests/test_gpu_rules_together.py holds the
GPU to it."""
import numpy as np

import avoid_reference as ar
import clearance_reference as wr
import coupled_reference as cr
import timed_reference as tr
from vfclik_amd import _abi


class Stack:
    """The wrappers of one move.  wait: dict(min_clearance, yields, mask) or None; avoid: dict(gain, d0, channel, scale, mask) or None."""

    def __init__(self, oc, chain, coupling, wait, avoid, stride, n_cycles, io_dtype, per_cycle=False):
        n_checks = n_cycles // stride
        self.n_cycles = n_cycles
        self.a = self.w = None
        inner = oc
        if avoid is not None:
            self.a = inner = ar.Avoiding(inner, chain, coupling["spheres"], avoid["gain"], avoid["d0"], avoid.get("channel", 4), avoid.get("scale"),
                                         avoid.get("mask"), stride, n_checks, io_dtype)
        if wait is not None:
            self.w = inner = wr.Waiting(inner, chain, coupling["spheres"], wait["min_clearance"], wait.get("yields"), wait.get("mask"), stride,
                                        n_checks, io_dtype)
            self.w.per_cycle = per_cycle
        self.c = cr._coupled(inner, chain, coupling, stride, n_cycles, io_dtype)
        if per_cycle:
            self.c.__class__ = ar.CoupledPerCycle
        for x in (self.a, self.w):
            if x is not None:
                x.coupled = self.c

    def mixer(self, inner):
        return inner if self.w is None else self.w.mixer(inner)

    def finish(self, r, closest):
        r["link_traj"] = self.c.done(self.n_cycles)
        a, w = self.a, self.w
        if a is not None:
            r["avoid_traj"], r["clear_traj"] = a.avoid_traj, a.clear_traj          # (the float64 clearance, as avoid_reference returns it)
        if w is not None:
            r["waited"], r["clear_traj"], r["pair_traj"], r["gate_traj"], r["wait_traj"] = w.waited, w.clear_traj, w.pair_traj, w.gate_traj, w.wait_traj
        r["closest"] = closest(r)
        return r


def _cart(r):
    return r["closest_c"]


def _joint(r):
    return r["closest_j"]


def _both(r):
    return np.minimum(r["closest_c"], r["closest_j"])


def goto(oc, chain, params, q0, fields, nfields, n_cycles, stride, dt, precision, coupling, wait=None, avoid=None, io_dtype=np.float64, **kw):
    """vfik_goto under the coupling and the rules.  **kw here and below: timed_reference._run's hold, clamp, active, null_control, want,
    stepped and rule (the stall rule).  Returns _run's dict with arrived, link_traj (n_checks, B, L, 4), with a wait rule waited (B,),
    clear_traj, pair_traj, gate_traj, wait_traj (n_checks, B), with an avoid rule avoid_traj (n_checks, B, n), with a stall rule stalled."""
    s = Stack(oc, chain, coupling, wait, avoid, stride, n_cycles, io_dtype)
    B, n = q0.shape
    slot = tr.goal_slot(fields, nfields)
    way = np.where((slot >= 0)[:, None], fields["p"][np.arange(B), np.maximum(slot, 0), :16], 0.0)
    r = tr._run(s.c, chain, params, q0, fields, nfields, np.full((B, 1), tr.FRAME, dtype=np.int32), way[:, None, :], np.zeros((B, 1, n)),
                n_cycles, stride, dt, precision, np.zeros(n), mixer=s.mixer(tr.handle_mixer(params)), send_frames=False, io_dtype=io_dtype, **kw)
    r["arrived"] = r["reached"][:, 0]
    return s.finish(r, _cart)


def follow(oc, chain, params, q0, fields, nfields, way, n_cycles, stride, dt, precision, coupling, wait=None, avoid=None, via_precision=None,
           io_dtype=np.float64, **kw):
    """vfik_follow; as goto."""
    s = Stack(oc, chain, coupling, wait, avoid, stride, n_cycles, io_dtype)
    B, n = q0.shape
    way = np.asarray(way, dtype=np.float64).reshape(B, -1, 16)
    r = tr._run(s.c, chain, params, q0, fields, nfields, tr.list_kind(way, tr.FRAME), way, np.zeros((B, way.shape[1], n)), n_cycles, stride,
                dt, precision, np.zeros(n), via_precision, mixer=s.mixer(tr.handle_mixer(params)), io_dtype=io_dtype, **kw)
    return s.finish(r, _cart)


def goto_js(oc, chain, params, q0, fields, nfields, q_ref, n_cycles, stride, dt, prec, coupling, wait=None, avoid=None, io_dtype=np.float64, **kw):
    """vfik_goto_js; as goto, closest = closest_j."""
    s = Stack(oc, chain, coupling, wait, avoid, stride, n_cycles, io_dtype)
    B, n = q0.shape
    r = tr._run(s.c, chain, params, q0, fields, nfields, np.full((B, 1), tr.POSTURE, dtype=np.int32), np.zeros((B, 1, 16)),
                np.asarray(q_ref, dtype=np.float64)[:, None, :], n_cycles, stride, dt, (0.0, 0.0), prec, mixer=s.mixer(tr.handle_mixer(params)),
                io_dtype=io_dtype, **kw)
    r["arrived"] = r["reached"][:, 0]
    return s.finish(r, _joint)


def follow_js(oc, chain, params, q0, fields, nfields, wayq, n_cycles, stride, dt, prec, coupling, wait=None, avoid=None, via_prec=None,
              io_dtype=np.float64, **kw):
    """vfik_follow_js; as goto_js."""
    s = Stack(oc, chain, coupling, wait, avoid, stride, n_cycles, io_dtype)
    B, n = q0.shape
    wayq = np.asarray(wayq, dtype=np.float64).reshape(B, -1, n)
    r = tr._run(s.c, chain, params, q0, fields, nfields, tr.list_kind(wayq, tr.POSTURE), np.zeros((B, wayq.shape[1], 16)), wayq, n_cycles, stride,
                dt, (0.0, 0.0), prec, None, via_prec, mixer=s.mixer(tr.handle_mixer(params)), io_dtype=io_dtype, **kw)
    return s.finish(r, _joint)


def script(oc, chain, params, q0, fields, nfields, kind, way, wayq, n_cycles, stride, dt, precision, js_precision, coupling, wait=None, avoid=None,
           via_precision=None, js_via_precision=None, mix_frame=_abi.MIX_FRAME, mix_posture=_abi.MIX_POSTURE, bridge_arm=None,
           io_dtype=np.float64, **kw):
    """vfik_script: the script's own mixer rows 0..3, weights 4 and 5 from params.  As goto; closest is the smaller of closest_c and
    closest_j."""
    s = Stack(oc, chain, coupling, wait, avoid, stride, n_cycles, io_dtype, per_cycle=True)
    mixer = tr.script_mixer(params, q0.shape[0], np.dtype(io_dtype), mix_frame, mix_posture, bridge_arm)
    r = tr._run(s.c, chain, params, q0, fields, nfields, kind, way, wayq, n_cycles, stride, dt, precision, js_precision, via_precision,
                js_via_precision, mixer=s.mixer(mixer), io_dtype=io_dtype, **kw)
    return s.finish(r, _both)


# ---- the scenes of tests/test_gpu_rules_together.py -----------------------------------------------------------------------------------
# coupled_reference.pair_case at the smallest batches that still have a full wave, a second wave and a tail (the last arm has no
# partner), every handle with the nullspace module and the mixer, mix_w[4] = 1: the avoid rule writes channel 4.  The odd arms yield; every
# eighth arm (3, 11, 19, ..: yielding arms) has its goal, its frames and its postures out of reach.
SCENES = {"lwr64": dict(robot="lwr", B=131, io_dtype=np.float64, stride=1, seed=7, js_prec=(0.02, 0.06)),
          "lwr32": dict(robot="lwr", B=131, io_dtype=np.float32, stride=4, seed=7, js_prec=(0.10, 0.15)),
          "dual64": dict(robot="lwr_dual14", B=67, io_dtype=np.float64, stride=4, seed=9, js_prec=(0.02, 0.06))}      # the stepped long-chain path
MOVES = ("goto", "follow", "goto_js", "follow_js", "script_pffp", "script_fpf", "script_ch3")
SCRIPTS = {"script_pffp": "PFFP", "script_fpf": "FPF", "script_ch3": "PFF"}
FLAGS = _abi.F_NULLSPACE | _abi.F_MIXER
MIX_CART, MIX_JOINT = (1.0, 1.0, 0.0, 0.0, 1.0, 0.0), (0.0, 0.0, 1.0, 0.0, 1.0, 0.0)
MIX_CH3 = (1.0, 1.0, 0.0, 0.0, 0.0, 0.0)          # script_ch3: the rule's channel 3 takes its weight from the script's own rows
MIX_FRAME_CH3, MIX_POSTURE_CH3 = (1.0, 1.0, 0.0, 1.0), (0.0, 0.0, 1.0, 1.0)
W, KP = 3, 8.0                          # jp_kp as tests/test_gpu_goto_js.py
FAR = slice(3, None, 8)
BEYOND = 0.2                                      # a far arm's posture lies this far beyond a joint limit: more than any js_prec


def yields_of(B):
    return wr.yields_of(B)


def case(scene, move):
    """The inputs of one move in one scene: coupled_reference.pair_case with
      follow       W = 3 frames on the way to the goal (pair_case's: arm 5's list has two rows, arm 8's none)
      goto_js      the posture q0 + U(-0.35, 0.35) per joint
      follow_js    W = 3 postures q0 + (w + 1) / W of that offset, arm 5's list two rows, arm 8's none
      scripts      P: the next of those postures, F: the next of pair_case's two frames (the last one is the goal); arm 5's script ends
                   behind its first step, arm 6's behind its second, arm 8 has none
    and for the far arms every frame's position times 3 and every posture BEYOND its limit in the joint that starts nearest to one."""
    from vfclik_amd import robots
    s = SCENES[scene]
    chain = robots.by_name(s["robot"])
    B, io = s["B"], s["io_dtype"]
    letters = SCRIPTS.get(move)
    n_way = W if move == "follow" else (letters.count("F") if letters else 0)
    seed = tuned(scene, move)["seed"]
    c = cr.pair_case(chain, B, io, seed=seed, n_way=n_way, far=FAR)
    n = chain.n
    far = np.zeros(B, dtype=bool)
    far[FAR] = True
    off = np.random.default_rng(seed + 1).uniform(-0.35, 0.35, size=(B, n))
    room = np.minimum(c["q0"] - chain.q_lo, chain.q_hi - c["q0"])
    j = np.argmin(room, axis=1)
    up = (chain.q_hi - c["q0"])[np.arange(B), j] < (c["q0"] - chain.q_lo)[np.arange(B), j]

    def postures(count):
        p = np.stack([np.clip(c["q0"] + (i + 1) / count * off, chain.q_lo, chain.q_hi) for i in range(count)], axis=1)
        for b in np.flatnonzero(far):
            p[b, :, j[b]] = chain.q_hi[j[b]] + BEYOND if up[b] else chain.q_lo[j[b]] - BEYOND
        return p.astype(io).astype(np.float64)
    if c["way"] is not None:
        way = np.array(c["way"], copy=True)
        way[far, :, 3] *= 3.0
        way[far, :, 7] *= 3.0
        way[far, :, 11] *= 3.0
        c["way"] = way.astype(io).astype(np.float64)
    if move == "goto_js":
        c["q_ref"] = postures(1)[:, 0]
    elif move == "follow_js":
        c["wayq"] = postures(W)
        c["wayq"][5, 2:, 0] = np.nan
        c["wayq"][8, :, 0] = np.nan
    elif letters:
        Wn = len(letters)
        ps, fi, pi = postures(letters.count("P")), 0, 0
        way, wayq, kind = np.zeros((B, Wn, 16)), np.zeros((B, Wn, n)), np.zeros((B, Wn), dtype=np.int32)
        for i, ch in enumerate(letters):
            if ch == "P":
                kind[:, i], wayq[:, i] = tr.POSTURE, ps[:, pi]
                pi += 1
            else:
                kind[:, i], way[:, i] = tr.FRAME, np.nan_to_num(c["way"][:, fi])
                fi += 1
        kind[5, 1:], kind[6, 2:], kind[8, :] = 0, 0, 0
        c.update(kind=kind, way_s=way, wayq_s=wayq)
    c.update(chain=chain, far=far, scene=scene, move=move)
    return c


def params_of(move):
    mix = MIX_CH3 if move == "script_ch3" else (MIX_JOINT if move in ("goto_js", "follow_js") else MIX_CART)
    return _abi.default_params(flags=FLAGS, max_vel=0.7, mix_w=mix, jp_kp=KP)


def run(oc, c, params, wait=None, avoid=None, rule=None, hold=True, n_cycles=None):
    """The move of case `c` under the coupling and the given rules (None: absent)."""
    s, move, chain = SCENES[c["scene"]], c["move"], c["chain"]
    n = chain.n
    coup = dict(spheres=c["spheres"], src_arm=c["src_arm"], xform=c["xform"], first_rep=c["first_rep"])
    args = (oc, chain, params, c["q0"], c["w"]["fields"], c["w"]["nfields"])
    N = cr.N_CYCLES if n_cycles is None else n_cycles
    kw = dict(hold=hold, clamp=True, io_dtype=s["io_dtype"], stepped=n > 7, want=("qdot_out",), rule=rule)
    prec, via = np.full(n, s["js_prec"][0]), np.full(n, s["js_prec"][1])
    if move == "goto":
        return goto(*args, N, s["stride"], cr.DT, cr.PREC, coup, wait, avoid, **kw)
    if move == "follow":
        return follow(*args, c["way"], N, s["stride"], cr.DT, cr.PREC, coup, wait, avoid, **kw)
    if move == "goto_js":
        return goto_js(*args, c["q_ref"], N, s["stride"], cr.DT, prec, coup, wait, avoid, **kw)
    if move == "follow_js":
        return follow_js(*args, c["wayq"], N, s["stride"], cr.DT, prec, coup, wait, avoid, via_prec=via, **kw)
    ch3 = move == "script_ch3"
    return script(*args, c["kind"], c["way_s"], c["wayq_s"], N, s["stride"], cr.DT, cr.PREC, prec, coup, wait, avoid, js_via_precision=via,
                  mix_frame=MIX_FRAME_CH3 if ch3 else _abi.MIX_FRAME, mix_posture=MIX_POSTURE_CH3 if ch3 else _abi.MIX_POSTURE, **kw)


# ---- the rules, chosen on the CPU from the ORACLE's run so that the conditions of `conditions` hold in every move of every scene (both
# tests assert them on the reference's run).  min_clearance and d0 in metres of room between an arm's spheres and its partner's; the
# stall rule's eps per check, so in proportion to the stride: 1 mm, 0.01 rad (angle) and 1 mrad (joints) per four cycles at float64.
# float32: ten times that -- a hundred times the suite's float32 margin, so that few progress compares come near their threshold.
# The avoid gain is 1 everywhere: on the 14-joint chain the ORACLE's own goto under gain 2 leaves itself by 2.8e-5 rad when its start is
# perturbed by 1e-14, a scene no two implementations repeat to 1e-8; under gain 1 that is 2.2e-11 and less in every move.
MIN_CLEARANCE = {"lwr64": 0.12, "lwr32": 0.12, "dual64": 0.11}
AVOID = {"lwr64": dict(gain=1.0, d0=0.10), "lwr32": dict(gain=1.0, d0=0.10), "dual64": dict(gain=1.0, d0=0.13)}
RULE = {"lwr64": dict(patience=3, eps=(2.5e-4, 2.5e-3), eps_js=2.5e-4, stop=True),
        "lwr32": dict(patience=5, eps=(1e-2, 1e-1), eps_js=1e-2, stop=True),
        "dual64": dict(patience=5, eps=(1e-3, 1e-2), eps_js=1e-3, stop=True)}


def _rule(patience, scale, stride=4):
    return dict(patience=patience, eps=(1e-3 * stride / 4 * scale, 1e-2 * stride / 4 * scale), eps_js=1e-3 * stride / 4 * scale, stop=True)


# A move's own numbers over its scene's: min_clearance and eps where the reference's run of THAT move keeps the share of arms within the
# suite's margin of a clearance, arrival or progress compare -- and the arms those are the source of -- under the cap (`left_out`).
TUNE = {("lwr64", "script_fpf"): dict(min_clearance=0.11, rule=_rule(5, 2.0, stride=1)),
        ("lwr64", "follow"): dict(min_clearance=0.10, rule=_rule(5, 2.0, stride=1)),
        ("lwr32", "goto"): dict(min_clearance=0.12, rule=_rule(3, 10.0)),
        ("lwr32", "follow"): dict(min_clearance=0.09, rule=_rule(3, 30.0)),
        ("lwr32", "script_pffp"): dict(min_clearance=0.13, rule=_rule(5, 20.0)),
        ("lwr32", "script_fpf"): dict(min_clearance=0.12, rule=_rule(3, 20.0)),
        ("lwr32", "script_ch3"): dict(min_clearance=0.13, rule=_rule(5, 20.0))}
ALL = CASES = [(sc, mv) for sc in SCENES for mv in MOVES]      # every scene and move, in both tests
POLL_CASE, POLL_CYCLES = ("dual64", "goto_js"), 240
_CACHE = {}


def tuned(scene, move):
    """dict(seed, min_clearance, avoid, rule) of a scene's move: the scene's numbers with the move's own (TUNE) over them"""
    t = dict(seed=SCENES[scene]["seed"], min_clearance=MIN_CLEARANCE[scene], avoid=AVOID[scene], rule=RULE[scene])
    t.update(TUNE.get((scene, move), {}))
    return t


def channel_of(move):
    return 3 if move == "script_ch3" else 4


def rules_of(scene, move):
    """(wait, avoid, stall) of a scene's move: the dicts `run` takes and the timed_reference.Rule"""
    B, t = SCENES[scene]["B"], tuned(scene, move)
    return (dict(min_clearance=t["min_clearance"], yields=yields_of(B), mask=None), dict(t["avoid"], channel=channel_of(move)),
            tr.Rule(**t["rule"]))


def reference(oc, scene, move):
    """(case, params, result) of a scene's move under coupling + wait + avoid + stall, hold on; computed once per process, never modified."""
    key = (scene, move)
    if key not in _CACHE:
        c, params = case(scene, move), params_of(move)
        wait, avoid, rule = rules_of(scene, move)
        r = run(oc, c, params, wait, avoid, rule)
        for v in list(r.values()) + [x for x in c.values() if isinstance(x, np.ndarray)] + [c["w"]["fields"], c["w"]["nfields"]]:
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _CACHE[key] = (c, params, r)
    return _CACHE[key]


def conditions(c, r):
    """The scene conditions on a run, as a dict of counts (B = the batch):
      again      arms that wait a block and run a later one             (every move: >= 8)
      pushed     arms with a nonzero command in some block              (>= 8)
      never      arms that are never pushed                             (>= B / 3)
      stalled, arrived                                                  (>= 4 each)
      partner    (arm, block) pairs: the arm waits while its non-yielding partner carries a nonzero command          (over the moves: >= 1)
      far        yielding far arms that wait in some block and stall in a later one                                  (over the moves: >= 1)
      far_arms   the indices of those arms
      below      (arm, block) pairs: a held or stalled arm -- out of the gate in front of the rule -- that yields and sits below
                 min_clearance, and does not count as waiting                                                           (over the moves: >= 1)"""
    wt, gt = r["wait_traj"], r["gate_traj"]
    B = wt.shape[1]
    yl = yields_of(B) != 0
    stride = SCENES[c["scene"]]["stride"]
    again = ((np.cumsum(wt, axis=0) > 0)[:-1] & (gt & ~wt)[1:]).any(axis=0)
    cmd = np.any(np.nan_to_num(r["avoid_traj"]) != 0, axis=2)                       # (checks, B)
    pushed = cmd.any(axis=0)
    src = c["src_arm"]
    partner = wt & np.where(src >= 0, cmd[:, np.maximum(src, 0)] & ~yl[np.maximum(src, 0)], False)
    last_wait = np.where(wt.any(axis=0), wt.shape[0] - 1 - np.argmax(wt[::-1], axis=0), wt.shape[0])
    far = c["far"] & yl & (r["stalled"] >= 0) & ((r["stalled"] + 1) // stride - 1 > last_wait)
    with np.errstate(invalid="ignore"):
        below = ~gt & (r["length"] > 0)[None, :] & yl[None, :] & (r["clear_traj"] < r_min(c))
    assert not (below & wt).any()
    arrived = (r["length"] > 0) & (r["next"] == r["length"])
    return dict(again=int(again.sum()), pushed=int(pushed.sum()), never=int((~pushed).sum()), stalled=int(np.count_nonzero(r["stalled"] >= 0)),
                arrived=int(arrived.sum()), partner=int(partner.sum()), far=int(far.sum()), below=int(below.sum()),
                far_arms=np.flatnonzero(far))


def r_min(c):
    return tuned(c["scene"], c["move"])["min_clearance"]


def conditions_hold(cond, B):
    return (cond["again"] >= 8 and cond["pushed"] >= 8 and 3 * cond["never"] >= B and cond["stalled"] >= 4 and cond["arrived"] >= 4)


def left_out(c, r):
    """(out, part, share, cap): the arms left out of the exact comparison with the reference -- within coupled_reference.MARGIN of an
    arrival threshold, of min_clearance at any block, or of a stall eps step in the REFERENCE's run, and (hold and stop are on) the arms
    those are the source of -- and their share of the arms that take part against the suite's cap"""
    io = SCENES[c["scene"]]["io_dtype"]
    margin = cr.MARGIN[np.dtype(io)][0]
    part = r["length"] > 0
    near = wr.near_rule(r, yields_of(len(part)), r_min(c), io) | (r["closest_s"] < margin) | (r["closest_sj"] < margin)
    out, _near, share, cap = cr.left_out(r, part, io, c["src_arm"], True, near)
    return out, part, share, cap


def poll_reference(oc):
    """(case, params, result) of POLL_CASE over POLL_CYCLES cycles under all the rules with NOBODY yielding: every arm arrives or stalls,
    so pending reaches 0 and a polling host form ends early."""
    if "poll" not in _CACHE:
        scene, move = POLL_CASE
        c, params = case(scene, move), params_of(move)
        wait, avoid, rule = rules_of(scene, move)
        wait["yields"] = np.zeros(SCENES[scene]["B"], dtype=np.int32)
        r = run(oc, c, params, wait, avoid, rule, n_cycles=POLL_CYCLES)
        for v in list(r.values()) + [x for x in c.values() if isinstance(x, np.ndarray)] + [c["w"]["fields"], c["w"]["nfields"]]:
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _CACHE["poll"] = (c, params, r)
    return _CACHE["poll"]
