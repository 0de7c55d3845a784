"""The stall rule of the timed moves (include/vfik.h: vfik_set_stall_rule) restated on the host.

`StallState` is the rule alone, a small state machine per arm: best (B, 2), count (B,), stalled (B,), fed one progress measure per check.
`Machine` is tests/script_reference.py's state machine with the rule in it: an arm that ran its block, is under way and did not arrive
at this check is measured --

    frame     (d, a): the distance pair as the arrival rule forms it, NaN for an arm without a goal block
    posture   e = max |ref - q| over the joints whose precision in force is finite (0 without one; NaN stays NaN)

-- progress is d < best_d - eps_pos or a < best_a - eps_rot (posture: e < best_e - eps_js), all strict; on progress best becomes the
componentwise minimum and count 0, else count + 1, and count == patience stalls the arm at cycle (k + 1) * stride - 1.  A stalled arm
meets no rule again, leaves pending and, with `stop`, the gate.  The check that advances an arm resets its best and count.

`stall_reference` is ONE oracle-stepped loop for every timed move, script_reference's with this Machine: a goto is a script of one frame
step (`goto`), a joint-space goto one of one posture step (`goto_js`); with `rule=None` the Machine is script_reference's own.  `replay`
runs the Machine on the rows a GPU run returned.

A helper of the suite, not a conftest.py: tests/test_stall_host.py checks it on the CPU, tests/test_gpu_stall.py holds the GPU to it."""
import numpy as np

import follow_reference as fr
import goto_js_reference as gjr
import goto_reference as gr
import script_reference as sr
from vfclik_amd import _abi

FRAME, POSTURE = sr.FRAME, sr.POSTURE


class Rule:
    """vfik_stall_rule without its output pointer"""

    def __init__(self, patience, eps=(0.0, 0.0), eps_js=0.0, stop=True):
        self.patience, self.eps, self.eps_js, self.stop = int(patience), (float(eps[0]), float(eps[1])), float(eps_js), bool(stop)


class StallState:
    """The rule alone.  step() is one evaluation for the arms in `sel`; closest and closest_j (B,) are the nearest any progress decision of
    the arm under the Cartesian and under the joint rule came to flipping: |m - (best - eps)|; for a frame, of the compare(s) whose change
    would change `d-progress or a-progress`."""

    def __init__(self, B, rule):
        self.rule = rule
        self.best = np.full((B, 2), np.inf)
        self.count = np.zeros(B, dtype=np.int32)
        self.stalled = np.full(B, -1, dtype=np.int32)
        self.closest = np.full(B, np.inf)
        self.closest_j = np.full(B, np.inf)

    def reset(self, sel):
        self.best[sel] = np.inf
        self.count[sel] = 0

    def step(self, sel, joint, m0, m1, cycle):
        """sel, joint (B,) bool; m0, m1 (B,) the measure (m1 is not read where joint).  Returns the arms this evaluation stalls."""
        r = self.rule
        eps0 = np.where(joint, r.eps_js, r.eps[0])
        with np.errstate(invalid="ignore"):
            thr0, thr1 = self.best[:, 0] - eps0, self.best[:, 1] - r.eps[1]
            p0, p1 = m0 < thr0, ~joint & (m1 < thr1)
            # what would flip `p0 | p1`: the nearer compare while both fail, the one that holds while one does, the farther while both hold
            n0, n1 = np.abs(m0 - thr0), np.where(joint, np.inf, np.abs(m1 - thr1))
            n0, n1 = np.where(np.isnan(n0), np.inf, n0), np.where(np.isnan(n1), np.inf, n1)
            near = np.where(p0 & p1, np.maximum(n0, n1), np.where(p0, n0, np.where(p1, n1, np.minimum(n0, n1))))
            low0, low1 = m0 < self.best[:, 0], ~joint & (m1 < self.best[:, 1])
        self.closest = np.where(sel & ~joint, np.minimum(self.closest, near), self.closest)
        self.closest_j = np.where(sel & joint, np.minimum(self.closest_j, near), self.closest_j)
        prog = sel & (p0 | p1)
        self.best[:, 0] = np.where(prog & low0, m0, self.best[:, 0])
        self.best[:, 1] = np.where(prog & low1, m1, self.best[:, 1])
        self.count = np.where(prog, 0, self.count + (sel & ~prog)).astype(np.int32)
        new = sel & ~prog & (self.count == r.patience)
        self.stalled[new] = cycle
        return new


def joint_measure(ref, q, prec):
    """(B,) max |ref - q| over the joints with a finite precision: ref, q, prec (B, n).  0 without such a joint, NaN if one of them is."""
    with np.errstate(invalid="ignore"):
        v = np.where(np.isfinite(prec), np.abs(ref - q), 0.0)
    return np.max(v, axis=1, initial=0.0)


class Machine(sr.Machine):
    """script_reference.Machine with the stall rule; rule None: that machine itself."""

    def __init__(self, *args, rule=None, **kw):
        super().__init__(*args, **kw)
        self.st = None if rule is None else StallState(len(self.arms), rule)

    @property
    def stalled(self):
        return self.st.stalled

    def check(self, k, q, dist):
        if self.st is None:
            return super().check(k, q, dist)
        # KEEP IN STEP with script_reference.Machine.check: from here to `self.next = ...` this is that method's body statement for
        # statement, with `& ~gone` in `decides` as the only change; the rule follows it, and `gate` and `pending` get its two terms.
        # (tests/test_stall_host.py: with a patience above n_checks this method must give what the parent's gives, bit for bit.)
        st = self.st
        ran = self.gate
        gone = st.stalled >= 0                      # left the state machine at an earlier check
        at, kd = self.at(), self.kind_at()
        self.way_traj[k] = np.where(ran, at, self.way_traj[k - 1] if k > 0 else -1)
        last = self.next >= self.L - 1
        decides = ran & (self.next < self.L) & ~gone
        joint = kd == POSTURE
        dec_c, dec_j = decides & (kd == FRAME), decides & joint
        pp, rp = np.where(last, self.prec[0], self.via[0]), np.where(last, self.prec[1], self.via[1])
        d, a = dist[:, 0], dist[:, 1] * np.pi / 180.0
        cur = self.wayq[self.arms, at]
        p_now = np.where(last[:, None], self.js_prec[None, :], self.js_via[None, :])
        with np.errstate(invalid="ignore"):
            ok_c = dec_c & self.present & (d < pp) & (a < rp)
            near = np.where(dec_c, np.minimum(np.abs(d - pp), np.abs(a - rp)), np.nan)
            ok_j = dec_j & gjr.rule(cur, q, p_now)
            at_posture = ran & joint
            self.diff = np.where(at_posture[:, None], (cur - q).astype(self.io_dtype), self.diff)
        self.closest_c = np.where(np.isnan(near), self.closest_c, np.minimum(self.closest_c, near))
        self.closest_j = np.where(dec_j, np.minimum(self.closest_j, gjr.edge_distance(cur, q, p_now)), self.closest_j)
        ok = ok_c | ok_j
        cycle = (k + 1) * self.stride - 1
        self.reached[self.arms[ok], self.next[ok]] = cycle
        self.next = self.next + ok.astype(np.int32)
        # the rule: every arm that decided and did not arrive; arrival goes first
        m0 = np.where(joint, joint_measure(cur, q, p_now), np.where(self.present, d, np.nan))
        m1 = np.where(self.present, a, np.nan)
        st.step(decides & ~ok, joint, m0, m1, cycle)
        st.reset(ok)
        gone = st.stalled >= 0
        self.gate = self.part & ~(self.hold & (self.next == self.L)) & ~(st.rule.stop & gone)
        self.pending[k] = int(np.count_nonzero(self.part & (self.next < self.L) & ~gone))
        return ran, ok & (self.next < self.L)


def replay(kind, wayq, present, q_traj, dist_traj, n_cycles, stride, precision, js_precision, via_precision=None, js_via_precision=None,
           hold=False, active=None, io_dtype=np.float64, rule=None):
    """The Machine on the rows a run returned, as script_reference.replay: q_traj (checks, B, n), dist_traj (checks, B, 2) or None (a
    joint-space move has no distances)."""
    m = Machine(kind, wayq, present, n_cycles, stride, precision, js_precision, via_precision, js_via_precision, hold, active, io_dtype,
                rule=rule)
    done = q_traj.shape[0]
    for k in range(done):
        dist = np.full((q_traj.shape[1], 2), np.nan) if dist_traj is None else dist_traj[k].astype(np.float64)
        m.check(k, q_traj[k].astype(np.float64), dist)
    m.pending, m.way_traj = m.pending[:done], m.way_traj[:done]
    return m


def stall_reference(oc, chain, params, q0, fields, nfields, kind, way, wayq, n_cycles, stride, dt, precision, js_precision,
                    via_precision=None, js_via_precision=None, mix_frame=_abi.MIX_FRAME, mix_posture=_abi.MIX_POSTURE, hold=False,
                    clamp=False, active=None, io_dtype=np.float64, null_control=None, want=("qdot_out",), stepped=False, bridge_arm=None,
                    rule=None):
    """script_reference.script_reference's loop, statement for statement, around the Machine above.  Returns its dict plus, with a rule,
    stalled (B,) int32 and closest_s, closest_sj (B,): the nearest any progress decision of the arm at a frame step, at a posture step,
    came to its threshold."""
    io_dtype = np.dtype(io_dtype)

    def rnd(a):
        return a.astype(io_dtype).astype(np.float64)
    B, n = q0.shape
    way = rnd(np.asarray(way, dtype=np.float64).reshape(B, -1, 16))
    fields = np.array(fields, copy=True)
    slot = fr._goal_slot(fields, nfields)
    present = slot >= 0
    m = Machine(kind, wayq, present, n_cycles, stride, precision, js_precision, via_precision, js_via_precision, hold, active, io_dtype,
                rule=rule)
    quads = {FRAME: rnd(np.asarray(mix_frame, dtype=np.float64)), POSTURE: rnd(np.asarray(mix_posture, dtype=np.float64))}
    tail = np.tile([params.mix_w[4], params.mix_w[5], params.max_vel], (B, 1)) if bridge_arm is None else np.asarray(bridge_arm, dtype=np.float64)
    bridge = np.zeros((B, 7))
    bridge[:, 4:] = rnd(tail)
    q_ref = np.full((B, n), np.nan)

    def send(sel):
        at, kd = m.at(), m.kind_at()
        for b in np.flatnonzero(sel):
            if kd[b] == FRAME:
                if present[b]:
                    fields["p"][b, slot[b], :12] = way[b, at[b], :12]
            else:
                q_ref[b] = m.wayq[b, at[b]]
            bridge[b, :4] = quads[int(kd[b])]
    send(m.part)
    q = rnd(np.array(q0, dtype=np.float64))
    states = oc.new_states(B, n) if params.flags & _abi.F_NULLSPACE else None
    q_traj = np.zeros((m.n_checks, B, n))
    dist_traj = np.full((m.n_checks, B, 2), np.nan)
    status = np.zeros(B, dtype=np.int32)
    keys = tuple(k for k in want if k != "status")
    rows = None
    for k in range(m.n_checks):
        qb = q.copy()
        gate = m.gate
        has = ~np.isnan(q_ref[:, 0])
        groups = [(sr._with_bridge(params, row), gate & np.all(bridge == row, axis=1)) for row in np.unique(bridge[gate], axis=0)]
        for c in range(stride):
            jc, _ = oc.joint_p(np.where(has[:, None], q_ref, 0.0), qb, chain.q_lo, chain.q_hi, params.jp_kp, params.jp_delta)
            ext = np.zeros((4, B, n))
            ext[0] = np.where(has[:, None], jc, 0.0)
            for p, sel in groups:
                ref = oc.cycle_batch(chain, p, qb, fields, nfields, null_control=null_control, ext_cmd=ext, states=states,
                                     want=tuple(set(keys) | {"qdot_out", "pose", "status"}), active=sel.astype(np.int32), into=rows)
                rows = {kk: ref[kk] for kk in ref if kk != "states"}
            if rows is None:
                break
            status |= np.where(gate, rows["status"], 0)
            qn = qb + dt * rows["qdot_out"]
            if clamp:
                qn = np.clip(qn, chain.q_lo, chain.q_hi)
            qb = np.where(gate[:, None], qn, qb)
            if stepped:
                qb = rnd(qb)
        q = np.where(gate[:, None], rnd(qb), q)
        if rows is not None:
            goal = np.nan_to_num(gr.goal_frames(fields, nfields, io_dtype))
            dist = rnd(gr.goal_distance(rows["pose"], goal))
        else:
            dist = np.full((B, 2), np.nan)
        dist[~present] = np.nan
        dist_traj[k] = np.where(gate[:, None], dist, dist_traj[k - 1] if k > 0 else np.nan)
        ran, advanced = m.check(k, q, dist_traj[k])
        send(advanced)
        q_traj[k] = q
    out = dict(reached=m.reached, next=m.next, length=m.L, pending=m.pending, q_traj=q_traj, dist_traj=dist_traj, way_traj=m.way_traj,
               q=q.copy(), diff=m.diff.astype(np.float64), states=states, closest_c=m.closest_c, closest_j=m.closest_j, status=status,
               fields=fields, q_ref=q_ref, present=present)
    if rule is not None:
        out["stalled"], out["closest_s"], out["closest_sj"] = m.st.stalled, m.st.closest, m.st.closest_j
    for kk in keys:
        out[kk] = rnd(rows[kk]) if rows is not None else np.zeros((B, n))
    return out


def goto(oc, chain, params, q0, fields, nfields, n_cycles, stride, dt, precision, rule=None, **kw):
    """vfik_goto as a script of ONE frame step: every arm's own goal frame as it stands, under the handle's mixer weights.  Returns
    stall_reference's dict with arrived (B,) = reached[:, 0]."""
    B, n = q0.shape
    slot = fr._goal_slot(fields, nfields)
    way = np.where((slot >= 0)[:, None], fields["p"][np.arange(B), np.maximum(slot, 0), :16], 0.0)
    r = stall_reference(oc, chain, params, q0, fields, nfields, np.full((B, 1), FRAME, dtype=np.int32), way[:, None, :], np.zeros((B, 1, n)),
                        n_cycles, stride, dt, precision, np.zeros(n), mix_frame=list(params.mix_w)[:4], rule=rule, **kw)
    r["arrived"] = r["reached"][:, 0]
    return r


def goto_js(oc, chain, params, q0, fields, nfields, q_ref, n_cycles, stride, dt, prec, rule=None, **kw):
    """vfik_goto_js as a script of ONE posture step under the handle's mixer weights.  Returns stall_reference's dict with arrived."""
    B, n = q0.shape
    r = stall_reference(oc, chain, params, q0, fields, nfields, np.full((B, 1), POSTURE, dtype=np.int32), np.zeros((B, 1, 16)),
                        np.asarray(q_ref, dtype=np.float64)[:, None, :], n_cycles, stride, dt, (0.0, 0.0), prec,
                        mix_posture=list(params.mix_w)[:4], rule=rule, **kw)
    r["arrived"] = r["reached"][:, 0]
    return r
