"""Motion scripts (include/vfik.h: vfik_script) restated on the host with the oracle, built from what tests/follow_reference.py and
tests/goto_js_reference.py do: `oracle_c.cycle_batch` stepped cycle by cycle, run once per controller group -- the arms whose mixer
weights and limiter speed are the same, `active = gate & group`, `mix_w[0..3]` the quad of the kind of step they are under way to --,
mixer channel 2 from `oracle_c.joint_p` on the arm's current reference row (NaN in its first element until the arm's first posture:
no controller), a per-arm mutable goal in a copy of the field array, the rollout's Euler update and clamp, q rounded to the I/O type
at block boundaries (every cycle with `stepped`: chains over 7 joints), and after every block of `stride` cycles the rule of the kind
of the step the arm is under way to:

    frame     present & (d < pos) & (a < rot)                           on the distance pair against the arm's goal as it stands
    posture   ((ref - prec) <= q) & ((ref + prec) >= q)).all()          on the posture as the caller sent it

with the via pair / via band at every step but the arm's last.  `Machine` is the state machine alone -- lengths, gate, rule, reached,
next, way_traj, pending, diff -- fed one block's q and distance rows at a time: `script_reference` feeds it the oracle's rows,
`replay` those a GPU run returned.

A helper of the suite, not a conftest.py: tests/test_script_host.py checks it on the CPU against follow_reference, follow_js_reference
and a hand-made case, tests/test_gpu_script.py holds the GPU to it."""
import ctypes as C

import numpy as np

import follow_reference as fr
import goto_js_reference as gjr
import goto_reference as gr
from vfclik_amd import _abi

FRAME, POSTURE = _abi.STEP_FRAME, _abi.STEP_POSTURE


def script_lengths(kind):
    """(B,) number of leading steps of kind (B, W) that are a frame or a posture."""
    ok = (kind == FRAME) | (kind == POSTURE)
    return np.where(ok.all(axis=1), kind.shape[1], np.argmin(ok, axis=1)).astype(np.int32)


class Machine:
    """vfik_script's state machine on rows somebody else computed.  check(k, q, dist) is the check after block k: q (B, n) and dist
    (B, 2) are float64 arrays of I/O-typed values, read only for the arms that ran the block (`gate` on entry)."""

    def __init__(self, kind, wayq, present, n_cycles, stride, precision, js_precision, via_precision=None, js_via_precision=None,
                 hold=False, active=None, io_dtype=np.float64):
        assert n_cycles % stride == 0 and stride >= 1
        self.io_dtype = np.dtype(io_dtype)
        self.kind = np.asarray(kind, dtype=np.int32)
        B, W = self.kind.shape
        self.wayq = np.asarray(wayq, dtype=np.float64).astype(self.io_dtype).astype(np.float64).reshape(B, W, -1)
        n = self.wayq.shape[2]
        self.present = np.asarray(present, dtype=bool)
        self.stride, self.hold, self.n_checks = stride, bool(hold), n_cycles // stride
        self.prec = precision
        self.via = precision if via_precision is None else via_precision
        self.js_prec = np.asarray(js_precision, dtype=np.float64)
        self.js_via = self.js_prec if js_via_precision is None else np.asarray(js_via_precision, dtype=np.float64)
        self.L = script_lengths(self.kind)
        ua = np.ones(B, dtype=bool) if active is None else (np.asarray(active) != 0)
        self.part = ua & (self.L > 0)
        self.arms = np.arange(B)
        self.next = np.zeros(B, dtype=np.int32)
        self.gate = self.part.copy()
        self.reached = np.full((B, W), -1, dtype=np.int32)
        self.pending = np.zeros(self.n_checks, dtype=np.int32)
        self.way_traj = np.full((self.n_checks, B), -1, dtype=np.int32)
        self.diff = np.zeros((B, n), dtype=self.io_dtype)
        self.closest_c = np.full(B, np.inf)
        self.closest_j = np.full(B, np.inf)

    def at(self):
        """(B,) the step every arm is under way to (the one its next check is made against): min(next, L - 1)"""
        return np.minimum(self.next, np.maximum(self.L - 1, 0))

    def kind_at(self):
        return self.kind[self.arms, self.at()]

    def check(self, k, q, dist):
        """The check after block k.  Returns (ran, advanced): the arms that ran the block, and those found at their step -- whose
        following step, if they have one, is to be sent (kind_at() and at() tell which afterwards)."""
        ran = self.gate
        at, kd = self.at(), self.kind_at()
        self.way_traj[k] = np.where(ran, at, self.way_traj[k - 1] if k > 0 else -1)
        last = self.next >= self.L - 1
        decides = ran & (self.next < self.L)
        dec_c, dec_j = decides & (kd == FRAME), decides & (kd == POSTURE)
        pp, rp = np.where(last, self.prec[0], self.via[0]), np.where(last, self.prec[1], self.via[1])
        d, a = dist[:, 0], dist[:, 1] * np.pi / 180.0
        cur = self.wayq[self.arms, at]
        p_now = np.where(last[:, None], self.js_prec[None, :], self.js_via[None, :])
        with np.errstate(invalid="ignore"):
            ok_c = dec_c & self.present & (d < pp) & (a < rp)
            near = np.where(dec_c, np.minimum(np.abs(d - pp), np.abs(a - rp)), np.nan)
            ok_j = dec_j & gjr.rule(cur, q, p_now)
            at_posture = ran & (kd == POSTURE)
            self.diff = np.where(at_posture[:, None], (cur - q).astype(self.io_dtype), self.diff)
        self.closest_c = np.where(np.isnan(near), self.closest_c, np.minimum(self.closest_c, near))
        self.closest_j = np.where(dec_j, np.minimum(self.closest_j, gjr.edge_distance(cur, q, p_now)), self.closest_j)
        ok = ok_c | ok_j
        self.reached[self.arms[ok], self.next[ok]] = (k + 1) * self.stride - 1
        self.next = self.next + ok.astype(np.int32)
        self.gate = self.part & ~(self.hold & (self.next == self.L))
        self.pending[k] = int(np.count_nonzero(self.part & (self.next < self.L)))
        return ran, ok & (self.next < self.L)


def replay(kind, wayq, present, q_traj, dist_traj, n_cycles, stride, precision, js_precision, via_precision=None, js_via_precision=None,
           hold=False, active=None, io_dtype=np.float64):
    """The state machine on the rows a run returned: q_traj (checks, B, n), dist_traj (checks, B, 2).  Returns the Machine after the
    last check that ran: reached, next, way_traj, pending (both cut to the checks that ran), diff (I/O type)."""
    m = Machine(kind, wayq, present, n_cycles, stride, precision, js_precision, via_precision, js_via_precision, hold, active, io_dtype)
    done = q_traj.shape[0]
    for k in range(done):
        m.check(k, q_traj[k].astype(np.float64), dist_traj[k].astype(np.float64))
    m.pending, m.way_traj = m.pending[:done], m.way_traj[:done]
    return m


def _with_bridge(params, row):
    """params with the mixer weights 0..5 and the limiter speed of one controller group"""
    p = _abi.Params()
    C.memmove(C.byref(p), C.byref(params), C.sizeof(p))
    for i in range(_abi.MIX_CHANNELS):
        p.mix_w[i] = float(row[i])
    p.max_vel = float(row[6])
    return p


def script_reference(oc, chain, params, q0, fields, nfields, kind, way, wayq, n_cycles, stride, dt, precision, js_precision,
                     via_precision=None, js_via_precision=None, mix_frame=_abi.MIX_FRAME, mix_posture=_abi.MIX_POSTURE, hold=False,
                     clamp=False, active=None, io_dtype=np.float64, null_control=None, want=("qdot_out",), stepped=False, bridge_arm=None):
    """B arms from q0 along their scripts: kind (B, W), way (B, W, 16), wayq (B, W, n).  Returns a dict:
      reached (B, W) int32, next (B,) int32, length (B,) int32, pending (n_checks,) int32, q_traj (n_checks, B, n), dist_traj
      (n_checks, B, 2) (NaN rows: never measured, or no goal block), way_traj (n_checks, B) int32 (-1: the arm never ran), q (B, n) = the
      last q_traj row, diff (B, n) (rounded to the I/O type; zeros for an arm no posture check was made for), the rows named in `want`
      of every arm's last evaluated cycle, status (OR over the cycles), states, fields (every arm's goal = the last frame it was sent),
      q_ref (B, n) the reference rows as the run left them, and
      closest_c, closest_j (B,): the nearest that any frame decision, and any posture decision, of the arm came to its threshold.
    bridge_arm (B, 3): every arm's mixer weights 4, 5 and limiter speed (vfik_set_mixer_weights, vfik_set_max_vel), None: params'."""
    io_dtype = np.dtype(io_dtype)

    def rnd(a):
        return a.astype(io_dtype).astype(np.float64)
    B, n = q0.shape
    way = rnd(np.asarray(way, dtype=np.float64).reshape(B, -1, 16))
    fields = np.array(fields, copy=True)
    slot = fr._goal_slot(fields, nfields)
    present = slot >= 0
    m = Machine(kind, wayq, present, n_cycles, stride, precision, js_precision, via_precision, js_via_precision, hold, active, io_dtype)
    quads = {FRAME: rnd(np.asarray(mix_frame, dtype=np.float64)), POSTURE: rnd(np.asarray(mix_posture, dtype=np.float64))}
    tail = np.tile([params.mix_w[4], params.mix_w[5], params.max_vel], (B, 1)) if bridge_arm is None else np.asarray(bridge_arm, dtype=np.float64)
    bridge = np.zeros((B, 7))
    bridge[:, 4:] = rnd(tail)
    q_ref = np.full((B, n), np.nan)

    def send(sel):
        """the step every arm in sel is under way to: a frame into its goal (rows 0..2, where it has a goal block), a posture into its
        reference row, the quad of the step's kind into its mixer row"""
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
        has = ~np.isnan(q_ref[:, 0])          # a row that starts with NaN: no controller, channel 2 stays the (zero) external command
        groups = [(_with_bridge(params, row), gate & np.all(bridge == row, axis=1)) for row in np.unique(bridge[gate], axis=0)]
        for c in range(stride):
            jc, _ = oc.joint_p(np.where(has[:, None], q_ref, 0.0), qb, chain.q_lo, chain.q_hi, params.jp_kp, params.jp_delta)
            ext = np.zeros((4, B, n))
            ext[0] = np.where(has[:, None], jc, 0.0)
            for p, sel in groups:
                ref = oc.cycle_batch(chain, p, qb, fields, nfields, null_control=null_control, ext_cmd=ext, states=states,
                                     want=tuple(set(keys) | {"qdot_out", "pose", "status"}), active=sel.astype(np.int32), into=rows)
                rows = {kk: ref[kk] for kk in ref if kk != "states"}
            if rows is None:
                break   # nobody runs: nothing to integrate
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
    for kk in keys:
        out[kk] = rnd(rows[kk]) if rows is not None else np.zeros((B, n))
    return out
