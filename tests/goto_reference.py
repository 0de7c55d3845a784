"""The batched goto (include/vfik.h: vfik_goto) restated on the host with the oracle: `oracle_c.cycle_batch` stepped cycle by cycle
with the Euler update and the clamp of tests/test_gpu_rollout.py:_oracle_rollout, the distance pair of /dmonitor/distOut from the
oracle's pose and the arm's goal frame (xyz norm, rotation angle in degrees: monitor_distance:76-84,161-172), and after every block
of `stride` cycles the arrival rule of handlers.py:374-381 (pos_dist < precision[0] and orient_dist * pi / 180 < precision[1], both
strict), the hold and the gate.

A helper of the suite, not a conftest.py: tests/test_goto_host.py checks it on the CPU against a hand-made case,
tests/test_gpu_goto.py holds the GPU to it."""
import numpy as np

from vfclik_amd import _abi

RAD2DEG = 57.295779513082320877


def goal_frames(fields, nfields, io_dtype=np.float64):
    """(B, 16) goal frame of every arm -- its lowest-id attractor, the goal block of vfik_set_fields -- rounded to the I/O type as the
    device image holds it; NaN rows for arms without one."""
    B = fields.shape[0]
    out = np.full((B, 16), np.nan)
    for b in range(B):
        f = fields[b, : int(nfields[b])]
        att = f[f["type"] == _abi.FIELD_ATTRACTOR]
        if len(att):
            g = att[np.argmin(att["id"], axis=0)] if len(att) > 1 else att[0]
            out[b] = np.asarray(g["p"][:16], dtype=io_dtype).astype(np.float64)
    return out


def goal_distance(pose, goal):
    """(B, 2): xyz distance and rotation angle in DEGREES between pose (B, 16) and goal (B, 16), as io->goal_dist reports them."""
    P, G = pose.reshape(-1, 4, 4), goal.reshape(-1, 4, 4)
    d = np.linalg.norm(G[:, :3, 3] - P[:, :3, 3], axis=1)
    E = np.einsum("bki,bkj->bij", P[:, :3, :3], G[:, :3, :3])   # R_cur^T R_goal
    ax = 0.5 * np.stack([E[:, 2, 1] - E[:, 1, 2], E[:, 0, 2] - E[:, 2, 0], E[:, 1, 0] - E[:, 0, 1]], 1)
    c = 0.5 * (E[:, 0, 0] + E[:, 1, 1] + E[:, 2, 2] - 1.0)
    ang = np.arctan2(np.linalg.norm(ax, axis=1), c)
    return np.stack([d, ang * RAD2DEG], 1)


def goto_reference(oc, chain, params, q0, fields, nfields, n_cycles, stride, dt, precision, hold=False, clamp=False, active=None,
                   io_dtype=np.float64, null_control=None, want=("qdot_out",), stepped=False):
    """The goto of B arms from q0.  Returns a dict:
      arrived (B,) int32, pending (n_checks,) int32, q_traj (n_checks, B, n), dist_traj (n_checks, B, 2) (NaN rows: no goal block),
      q (B, n) = the last q_traj row, the rows named in `want` of every arm's last evaluated cycle, status (OR over the cycles),
      states (the oracle's nullspace states at the end, or None), and
      closest (B,): the smallest |distance - precision[0]| or |angle [rad] - precision[1]| over all checks -- how near the arm's
      arrival decision ever came to its threshold.
    float32 I/O: q, the outputs and the distances are rounded where the device buffers hold them -- q at block boundaries (every
    cycle with `stepped`: the launches of a stepped rollout hand q over in the I/O type), the distances before the rule reads them."""
    assert n_cycles % stride == 0 and stride >= 1
    io_dtype = np.dtype(io_dtype)

    def rnd(a):
        return a.astype(io_dtype).astype(np.float64)
    B, n = q0.shape
    n_checks = n_cycles // stride
    ua = np.ones(B, dtype=bool) if active is None else (np.asarray(active) != 0)
    gate = ua.copy()
    goal = goal_frames(fields, nfields, io_dtype)
    present = ~np.isnan(goal[:, 0])
    q = rnd(np.array(q0, dtype=np.float64))
    states = oc.new_states(B, n) if params.flags & _abi.F_NULLSPACE else None
    arrived = np.full(B, -1, dtype=np.int32)
    pending = np.zeros(n_checks, dtype=np.int32)
    q_traj = np.zeros((n_checks, B, n))
    dist_traj = np.full((n_checks, B, 2), np.nan)
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
        dist = rnd(goal_distance(ref["pose"], np.nan_to_num(goal)))
        dist[~present] = np.nan
        ran = gate
        dist_traj[k] = np.where(ran[:, None], dist, dist_traj[k - 1] if k > 0 else np.nan)
        d, a = dist_traj[k, :, 0], dist_traj[k, :, 1] * np.pi / 180.0
        with np.errstate(invalid="ignore"):
            ok = ran & (arrived < 0) & present & (d < precision[0]) & (a < precision[1])
            near = np.minimum(np.abs(d - precision[0]), np.abs(a - precision[1]))
        closest = np.where(np.isnan(near), closest, np.minimum(closest, near))
        arrived[ok] = (k + 1) * stride - 1
        gate = ua & ~(bool(hold) & (arrived >= 0))
        pending[k] = int(np.count_nonzero(ua & (arrived < 0)))
        q_traj[k] = q
    out = dict(arrived=arrived, pending=pending, q_traj=q_traj, dist_traj=dist_traj, q=q.copy(), states=states, closest=closest,
               status=status)
    for kk in keys:
        out[kk] = rnd(rows[kk])
    return out
