"""Waypoint lists (include/vfik.h: vfik_follow) restated on the host with the oracle, as tests/goto_reference.py restates the batched
goto: `oracle_c.cycle_batch` stepped cycle by cycle with the rollout's Euler update and clamp, the distance pair of /dmonitor/distOut
from the oracle's pose and the arm's CURRENT goal frame, and after every block of `stride` cycles the rule of the header: the arm found
at waypoint next[b] -- both compares strict; (via_pos, via_rot) while a waypoint follows, precision at the arm's last one -- notes the
check's cycle in reached[b][next], advances, and gets the following waypoint as its goal: a per-arm mutable goal in a copy of the field
array (the frame of the arm's lowest-id attractor, rows 0..2, rounded to the I/O type as the device image holds it).

A helper of the suite, not a conftest.py: tests/test_follow_host.py checks it on the CPU against a hand-made case,
tests/test_gpu_follow.py holds the GPU to it."""
import numpy as np

import goto_reference as gr
from vfclik_amd import _abi


def path_lengths(way):
    """(B,) number of leading rows of way (B, W, 16) whose first element is not NaN."""
    ok = ~np.isnan(way[:, :, 0])
    return np.where(ok.all(axis=1), way.shape[1], np.argmin(ok, axis=1)).astype(np.int32)


def _goal_slot(fields, nfields):
    """(B,) index of every arm's lowest-id attractor in its field row, -1 without one."""
    slot = np.full(fields.shape[0], -1)
    for b in range(fields.shape[0]):
        f = fields[b, : int(nfields[b])]
        idx = np.flatnonzero(f["type"] == _abi.FIELD_ATTRACTOR)
        if len(idx):
            slot[b] = idx[np.argmin(f["id"][idx])]
    return slot


def follow_reference(oc, chain, params, q0, fields, nfields, way, n_cycles, stride, dt, precision, via_precision=None, hold=False,
                     clamp=False, active=None, io_dtype=np.float64, null_control=None, want=("qdot_out",), stepped=False):
    """B arms from q0 along way (B, W, 16).  Returns a dict:
      reached (B, W) int32, next (B,) int32, length (B,) int32, pending (n_checks,) int32, q_traj (n_checks, B, n),
      dist_traj (n_checks, B, 2) (NaN rows: never measured), way_traj (n_checks, B) int32 (-1: never measured),
      q (B, n) = the last q_traj row, the rows named in `want` of every arm's last evaluated cycle, status (OR over the cycles), states,
      fields: the field array as the run left it (every arm's goal = the waypoint it was last sent to), and
      closest (B,): the smallest |distance - threshold| or |angle [rad] - threshold| over all the arm's decisions, against the pair in
      force at that check -- how near any decision of the arm came to its threshold.
    float32 I/O: as goto_reference (q at block boundaries, every cycle with `stepped`; the distances before the rule reads them)."""
    assert n_cycles % stride == 0 and stride >= 1
    io_dtype = np.dtype(io_dtype)
    via = precision if via_precision is None else via_precision

    def rnd(a):
        return a.astype(io_dtype).astype(np.float64)
    B, n = q0.shape
    way = rnd(np.asarray(way, dtype=np.float64).reshape(B, -1, 16))
    W = way.shape[1]
    n_checks = n_cycles // stride
    L = path_lengths(way)
    ua = np.ones(B, dtype=bool) if active is None else (np.asarray(active) != 0)
    part = ua & (L > 0)
    fields = np.array(fields, copy=True)
    slot = _goal_slot(fields, nfields)
    present = slot >= 0
    arms = np.arange(B)

    def send(sel, w):
        """waypoint w[b] becomes the goal of the arms in sel that have a goal block: rows 0..2 of the frame"""
        for b in np.flatnonzero(sel & present):
            fields["p"][b, slot[b], :12] = way[b, w[b], :12]
    nxt = np.zeros(B, dtype=np.int32)
    send(part, nxt)
    gate = part.copy()
    q = rnd(np.array(q0, dtype=np.float64))
    states = oc.new_states(B, n) if params.flags & _abi.F_NULLSPACE else None
    reached = np.full((B, W), -1, dtype=np.int32)
    pending = np.zeros(n_checks, dtype=np.int32)
    q_traj = np.zeros((n_checks, B, n))
    dist_traj = np.full((n_checks, B, 2), np.nan)
    way_traj = np.full((n_checks, B), -1, dtype=np.int32)
    closest = np.full(B, np.inf)
    status = np.zeros(B, dtype=np.int32)
    keys = tuple(k for k in want if k != "status")
    rows = None
    for k in range(n_checks):
        qb = q.copy()
        for c in range(stride):
            ref = oc.cycle_batch(chain, params, qb, fields, nfields, null_control=null_control, states=states,
                                 want=tuple(set(keys) | {"qdot_out", "pose", "status"}), active=gate.astype(np.int32), into=rows)
            rows = {kk: ref[kk] for kk in ref if kk != "states"}
            status |= np.where(gate, ref["status"], 0)
            qn = qb + dt * ref["qdot_out"]
            if clamp:
                qn = np.clip(qn, chain.q_lo, chain.q_hi)
            qb = np.where(gate[:, None], qn, qb)
            if stepped:
                qb = rnd(qb)
        q = np.where(gate[:, None], rnd(qb), q)
        goal = np.nan_to_num(gr.goal_frames(fields, nfields, io_dtype))
        dist = rnd(gr.goal_distance(ref["pose"], goal))
        dist[~present] = np.nan
        ran = gate
        dist_traj[k] = np.where(ran[:, None], dist, dist_traj[k - 1] if k > 0 else np.nan)
        way_traj[k] = np.where(ran, np.minimum(nxt, np.maximum(L - 1, 0)), way_traj[k - 1] if k > 0 else -1)
        last = nxt == L - 1
        pp, rp = np.where(last, precision[0], via[0]), np.where(last, precision[1], via[1])
        d, a = dist_traj[k, :, 0], dist_traj[k, :, 1] * np.pi / 180.0
        decides = ran & (nxt < L)
        with np.errstate(invalid="ignore"):
            ok = decides & present & (d < pp) & (a < rp)
            near = np.where(decides, np.minimum(np.abs(d - pp), np.abs(a - rp)), np.nan)
        closest = np.where(np.isnan(near), closest, np.minimum(closest, near))
        reached[arms[ok], nxt[ok]] = (k + 1) * stride - 1
        nxt = nxt + ok.astype(np.int32)
        send(ok & (nxt < L), nxt)
        gate = part & ~(bool(hold) & (nxt == L))
        pending[k] = int(np.count_nonzero(part & (nxt < L)))
        q_traj[k] = q
    out = dict(reached=reached, next=nxt, length=L, pending=pending, q_traj=q_traj, dist_traj=dist_traj, way_traj=way_traj, q=q.copy(),
               states=states, closest=closest, status=status, fields=fields)
    for kk in keys:
        out[kk] = rnd(rows[kk])
    return out
