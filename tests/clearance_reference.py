"""The timed moves under a coupling AND a wait rule (include/vfik.h: vfik_set_wait_rule) restated on the host: coupled_reference's
oracle-stepped move with the rule in front of every block.

The route.  `timed_reference._run` hands the state machine's gate array -- the very array `Machine.check` reads afterwards as "who ran" --
to its `mixer(gate, kind)` hook in front of every block, and `cycle_batch` then sees the block's input q.  So `Waiting` is two small hooks
around one state: `mixer` keeps the array, and `cycle_batch`, at the first cycle of a block (coupled_reference.Coupled calls it right
after it placed the partner's spheres for that block), measures every arm's clearance on the host in float64
(hp_clearance.host_clearance: own spheres from Chain.fk of the truncated chains, the partner's rows as Coupled rounded them to the I/O
type), rounds it to the I/O type, CLEARS the gate entries of the arms that wait IN PLACE -- from there on `_run` treats them as arms that
do not run: their q, status and distance rows repeat, the check applies no rule to them and keeps them in pending -- and narrows `active`
for the block's oracle calls (`_run` formed its controller groups from the gate before the hook's caller could clear it).  The check
rebuilds the gate from the state machine alone, so the next block's hook starts from "everybody who takes part runs".

`timed_reference.goto` / `follow` build their mixer themselves, so the two forms here call `timed_reference._run` with the handle's mixer
wrapped; their few lines of argument shaping are repeated, nothing of the loop is.  `timed_reference.py` and `coupled_reference.py` are
untouched.

A helper of the suite, not a conftest.py: tests/test_wait_reference.py checks it on the CPU, tests/test_gpu_wait_rule.py holds the GPU to it."""
import numpy as np

import coupled_reference as cr
import hp_clearance as hc
import timed_reference as tr


class Waiting:
    """The oracle object with the wait rule in front of every block's first cycle; everything else of `oc` passes through.  It sits INSIDE
    a coupled_reference.Coupled (`coupled`, set by the caller), whose link_traj[k] are the partner's rows of block k."""

    def __init__(self, oc, chain, spheres, min_clearance, yields, mask, stride, n_checks, io_dtype):
        self.oc, self.chain, self.spheres, self.stride, self.n_checks, self.io_dtype = oc, chain, list(spheres), int(stride), n_checks, io_dtype
        self.min_clearance, self.mask = float(min_clearance), mask
        self.yields = None if yields is None else (np.asarray(yields) != 0)
        self.coupled = None
        self.gate = None
        self.calls = 0
        self.waiting = None
        self.per_cycle = False     # a script (tests/rules_reference.py): several calls per cycle, told apart as avoid_reference does
        self.last_ext = None

    def __getattr__(self, name):
        return getattr(self.oc, name)

    def mixer(self, inner):
        def groups(gate, kd):
            self.gate = gate            # the machine's own array: cleared in place by the first cycle of the block
            return inner(gate, kd)
        return groups

    def cycle_batch(self, chain, params, q, fields, nfields, **kw):
        # `calls` counts cycles: every call is one, or with `per_cycle` every call that brings a new ext_cmd array (`_run` makes one per cycle
        # and hands the same one to every controller group)
        new_cycle = not self.per_cycle or kw.get("ext_cmd") is None or kw["ext_cmd"] is not self.last_ext
        self.last_ext = kw.get("ext_cmd")
        if new_cycle and self.calls % self.stride == 0:
            k = self.calls // self.stride
            B, L = q.shape[0], len(self.spheres)
            if self.waiting is None:
                self.clear_traj = np.full((self.n_checks, B), np.nan)
                self.pair_traj = np.full((self.n_checks, B), -1, dtype=np.int32)
                self.gate_traj = np.zeros((self.n_checks, B), dtype=bool)    # the gate in front of the rule
                self.wait_traj = np.zeros((self.n_checks, B), dtype=bool)
                self.waited = np.zeros(B, dtype=np.int32)
            clear, pair, _d = hc.host_clearance(self.chain, self.spheres, q, self.coupled.link_traj[k], 0, L, self.mask)
            clear = clear.astype(self.io_dtype).astype(np.float64)
            yl = np.ones(B, dtype=bool) if self.yields is None else self.yields
            with np.errstate(invalid="ignore"):
                wait = self.gate & yl & (clear < self.min_clearance)
            self.clear_traj[k], self.pair_traj[k], self.gate_traj[k], self.wait_traj[k] = clear, pair, self.gate, wait
            self.waited = wait.astype(np.int32) if k == 0 else self.waited + wait
            self.gate[wait] = False
            self.waiting = wait
        self.calls += int(new_cycle)
        if "active" in kw and kw["active"] is not None:
            kw["active"] = (np.asarray(kw["active"]) != 0) & ~self.waiting
        else:
            kw["active"] = ~self.waiting
        kw["active"] = kw["active"].astype(np.int32)
        return self.oc.cycle_batch(chain, params, q, fields, nfields, **kw)


def _wrap(oc, chain, coupling, rule, stride, n_cycles, io_dtype):
    w = Waiting(oc, chain, coupling["spheres"], rule["min_clearance"], rule.get("yields"), rule.get("mask"), stride, n_cycles // stride, io_dtype)
    c = cr._coupled(w, chain, coupling, stride, n_cycles, io_dtype)
    w.coupled = c
    return w, c


def _finish(r, w, c, n_cycles):
    r["link_traj"] = c.done(n_cycles)
    r["waited"], r["clear_traj"], r["pair_traj"], r["gate_traj"], r["wait_traj"] = w.waited, w.clear_traj, w.pair_traj, w.gate_traj, w.wait_traj
    r["closest"] = r["closest_c"]
    return r


def goto(oc, chain, params, q0, fields, nfields, n_cycles, stride, dt, precision, coupling, rule, io_dtype=np.float64, **kw):
    """coupled_reference.goto under rule = dict(min_clearance, yields, mask).  Returns its dict with waited (B,), clear_traj and pair_traj
    (n_checks, B), gate_traj (the gate in front of the rule) and wait_traj (who waited), both (n_checks, B) bool."""
    w, c = _wrap(oc, chain, coupling, rule, stride, n_cycles, io_dtype)
    B, n = q0.shape
    slot = tr.goal_slot(fields, nfields)
    way = np.where((slot >= 0)[:, None], fields["p"][np.arange(B), np.maximum(slot, 0), :16], 0.0)
    r = tr._run(c, chain, params, q0, fields, nfields, np.full((B, 1), tr.FRAME, dtype=np.int32), way[:, None, :], np.zeros((B, 1, n)),
                n_cycles, stride, dt, precision, np.zeros(n), mixer=w.mixer(tr.handle_mixer(params)), send_frames=False, io_dtype=io_dtype, **kw)
    r["arrived"] = r["reached"][:, 0]
    return _finish(r, w, c, n_cycles)


def follow(oc, chain, params, q0, fields, nfields, way, n_cycles, stride, dt, precision, coupling, rule, via_precision=None,
           io_dtype=np.float64, **kw):
    """coupled_reference.follow under a rule; as goto."""
    w, c = _wrap(oc, chain, coupling, rule, stride, n_cycles, io_dtype)
    B, n = q0.shape
    way = np.asarray(way, dtype=np.float64).reshape(B, -1, 16)
    r = tr._run(c, chain, params, q0, fields, nfields, tr.list_kind(way, tr.FRAME), way, np.zeros((B, way.shape[1], n)), n_cycles, stride,
                dt, precision, np.zeros(n), via_precision, mixer=w.mixer(tr.handle_mixer(params)), io_dtype=io_dtype, **kw)
    return _finish(r, w, c, n_cycles)


# ---- the scene of tests/test_gpu_wait_rule.py: the coupled moves of coupled_reference.MOVES, the odd arms yielding --------------------
# min_clearance per move, chosen on the CPU from the ORACLE's run so that the three conditions of `conditions` hold (they are asserted on
# the reference's run by both tests): metres of room between an odd arm's spheres and its even partner's.
MIN_CLEARANCE = {"goto64": 0.058, "goto32": 0.052, "follow": 0.072}
_CACHE = {}


def yields_of(B):
    return (np.arange(B) % 2 == 1).astype(np.int32)


def reference(oc, name):
    """(case, params, result) of coupled_reference.MOVES[name] under the rule of MIN_CLEARANCE[name], the odd arms yielding; computed once
    per process and never modified."""
    if name not in _CACHE:
        from vfclik_amd import _abi, robots
        m = cr.MOVES[name]
        chain = robots.by_name(m["robot"])
        c = cr.pair_case(chain, m["B"], m["io_dtype"], seed=m["seed"], n_way=m.get("n_way", 0), far=m.get("far"))
        c["chain"] = chain
        params = _abi.default_params(flags=m["flags"], max_vel=0.7)
        kw = dict(hold=m["hold"], clamp=True, io_dtype=m["io_dtype"], stepped=chain.n > 7, want=("qdot_out",))
        args = (oc, chain, params, c["q0"], c["w"]["fields"], c["w"]["nfields"])
        coup = dict(spheres=c["spheres"], src_arm=c["src_arm"], xform=c["xform"], first_rep=c["first_rep"])
        rule = dict(min_clearance=MIN_CLEARANCE[name], yields=yields_of(m["B"]), mask=None)
        if c["way"] is None:
            r = goto(*args, cr.N_CYCLES, m["stride"], cr.DT, cr.PREC, coup, rule, **kw)
        else:
            r = follow(*args, c["way"], cr.N_CYCLES, m["stride"], cr.DT, cr.PREC, coup, rule, **kw)
        for v in list(r.values()) + [c["q0"], c["xform"], c["src_arm"], c["w"]["fields"], c["w"]["nfields"]]:
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _CACHE[name] = (c, params, r)
    return _CACHE[name]


def conditions(r, yields):
    """The scene's three conditions on a run: (arms that waited at least one block and ran a later one, arms that waited through the last
    block, the share of the yielding arms that never waited)."""
    wt, gt = r["wait_traj"], r["gate_traj"]
    ran = gt & ~wt
    again = ((np.cumsum(wt, axis=0) > 0)[:-1] & ran[1:]).any(axis=0)
    yl = np.asarray(yields) != 0
    return int(np.count_nonzero(again)), int(np.count_nonzero(wt[-1])), float(np.count_nonzero(yl & (r["waited"] == 0)) / max(np.count_nonzero(yl), 1))


def near_rule(r, yields, min_clearance, io_dtype):
    """(B,) the yielding arms whose clearance in this run comes within the suite's margin of min_clearance at any block"""
    margin = cr.MARGIN[np.dtype(io_dtype)][0]
    with np.errstate(invalid="ignore"):
        return (np.asarray(yields) != 0) & (np.abs(r["clear_traj"] - min_clearance) < margin).any(axis=0)


def replay_rule(clear_traj, gate_in, yields, min_clearance):
    """The rule alone on rows somebody else computed: clear_traj (checks, B) of I/O-typed values, gate_in (checks, B) the gate in front of
    the rule.  Returns (wait (checks, B) bool, waited (B,) int32)."""
    with np.errstate(invalid="ignore"):
        wait = (np.asarray(gate_in) != 0) & (np.asarray(yields) != 0)[None, :] & (clear_traj.astype(np.float64) < min_clearance)
    return wait, wait.sum(axis=0).astype(np.int32)
