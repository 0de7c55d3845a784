"""The timed moves under a coupling (include/vfik.h: vfik_set_coupling) restated on the host: tests/timed_reference.py's oracle-stepped loop
with the other arm's link spheres written into the field array at the start of every block.

`timed_reference._run` hands its mutable field array and the current q to `oc.cycle_batch` every cycle, once per controller group.  Under the
handle's mixer with batch-wide weights that is ONE call per cycle, so the call number tells the block: `Coupled` wraps the oracle object,
and in front of the first cycle of every block -- q is then the block's input row, rounded to the I/O type, gated and held arms carrying the
row they hold -- it

  * computes every arm's partner spheres on the host in float64 (hp_links.host_points: Chain.fk of the chain truncated at the sphere's link,
    times the centre, through xform[b] = [R_b | t_b]) from q[src_arm[b]], rounded to the I/O type;
  * writes sphere j into `fields["p"][b, slot, 0:4]` (x y z radius) of the arm's (first_rep + j)-th decay repeller in ascending-id order;
    safe distance, order and force stay.  A NaN row -- a source outside the batch, a NaN in its q -- leaves the repeller as it is, and so
    does a row beyond the arm's repeller count;
  * keeps the rows as link_traj[k] (n_checks, B, L, 4).

The state machine, the integration, the rounding and the distance rows are timed_reference's, untouched.  A helper of the suite, not a
conftest.py: tests/test_coupled_reference.py checks it on the CPU, tests/test_gpu_coupled_moves.py holds the GPU to it."""
import numpy as np

import hp_links as hl
import timed_reference as tr
from vfclik_amd import _abi


def repeller_slots(fields, nfields):
    """per arm the indices into its field row of its decay repellers in ascending-id order"""
    out = []
    for b in range(fields.shape[0]):
        f = fields[b, : int(nfields[b])]
        idx = np.flatnonzero(f["type"] == _abi.FIELD_REPELLER)
        out.append(idx[np.argsort(f["id"][idx], kind="stable")])
    return out


def place(chain, spheres, q, src_arm, xform, io_dtype):
    """(B, L, 4) the rows of one block: host float64, rounded to the I/O type"""
    return hl.host_points(chain, spheres, q, src_arm, xform).astype(io_dtype).astype(np.float64)


class Coupled:
    """The oracle object with the coupling in front of every block's first cycle; everything else of `oc` passes through."""

    def __init__(self, oc, chain, spheres, src_arm, xform, first_rep, stride, n_checks, io_dtype):
        self.oc, self.chain, self.spheres, self.first_rep, self.stride, self.io_dtype = oc, chain, list(spheres), int(first_rep), int(stride), io_dtype
        self.src_arm = None if src_arm is None else np.asarray(src_arm, dtype=np.int64)
        self.xform = None if xform is None else np.asarray(xform, dtype=np.float64).astype(io_dtype).astype(np.float64)
        self.calls = 0
        self.link_traj = None
        self.n_checks = n_checks
        self.slots = None

    def __getattr__(self, name):
        return getattr(self.oc, name)

    def cycle_batch(self, chain, params, q, fields, nfields, **kw):
        if self.calls % self.stride == 0:
            k = self.calls // self.stride
            B = q.shape[0]
            if self.link_traj is None:
                self.link_traj = np.full((self.n_checks, B, len(self.spheres), 4), np.nan)
                self.slots = repeller_slots(fields, nfields)
            rows = place(self.chain, self.spheres, q, self.src_arm, self.xform, self.io_dtype)
            self.link_traj[k] = rows
            for b in range(B):
                for j in range(len(self.spheres)):
                    r = self.first_rep + j
                    if r < len(self.slots[b]) and not np.isnan(rows[b, j, 0]):
                        fields["p"][b, self.slots[b][r], 0:4] = rows[b, j]
        self.calls += 1
        return self.oc.cycle_batch(chain, params, q, fields, nfields, **kw)


    def done(self, n_cycles):
        """link_traj, after the run: the block is told from the number of calls, which holds only while `_run` makes exactly one per cycle
        (one controller group, somebody running in every cycle)"""
        assert self.calls == n_cycles, "cycle_batch was called %d times in %d cycles: the blocks were not told apart" % (self.calls, n_cycles)
        return self.link_traj


def _coupled(oc, chain, coupling, stride, n_cycles, io_dtype):
    return Coupled(oc, chain, coupling["spheres"], coupling.get("src_arm"), coupling.get("xform"), coupling.get("first_rep", 0), stride,
                   n_cycles // stride, io_dtype)


def goto(oc, chain, params, q0, fields, nfields, n_cycles, stride, dt, precision, coupling, io_dtype=np.float64, **kw):
    """timed_reference.goto under a coupling = dict(spheres, src_arm, xform, first_rep).  Batch-wide mixer weights only.  Returns its dict
    with link_traj (n_checks, B, L, 4): the rows every block started from."""
    assert "mix_w_arm" not in kw, "one cycle_batch call per cycle: batch-wide mixer weights only"
    c = _coupled(oc, chain, coupling, stride, n_cycles, io_dtype)
    r = tr.goto(c, chain, params, q0, fields, nfields, n_cycles, stride, dt, precision, io_dtype=io_dtype, **kw)
    r["link_traj"] = c.done(n_cycles)
    return r


def follow(oc, chain, params, q0, fields, nfields, way, n_cycles, stride, dt, precision, coupling, via_precision=None, io_dtype=np.float64, **kw):
    """timed_reference.follow under a coupling; as goto."""
    assert "mix_w_arm" not in kw, "one cycle_batch call per cycle: batch-wide mixer weights only"
    c = _coupled(oc, chain, coupling, stride, n_cycles, io_dtype)
    r = tr.follow(c, chain, params, q0, fields, nfields, way, n_cycles, stride, dt, precision, via_precision, io_dtype=io_dtype, **kw)
    r["link_traj"] = c.done(n_cycles)
    return r


# ---- the scene of the coupled tests ---------------------------------------------------------------------------------------------------
PARKED = (10.0, 10.0, 10.0)   # where the partner's repellers sit until the first block moves them: out of everybody's reach


def pair_case(chain, B, io_dtype, seed=7, n_static=1, links=None, gap=0.3, n_way=0, far=None, force=-2.0, order=2.0, spread=(0.05, 0.25)):
    """Arms in pairs b <-> b ^ 1 (the last arm of an odd batch has no partner: source -1) that share a workspace.

    Every arm: a goal chain.fk(qg), qg = U(0.6 q_lo, 0.6 q_hi), a start qg + s U(-1, 1) with s = U(0.05, 0.25) per arm, `n_static` static
    obstacles of synth.make_workload (ids 4 ..; the feeder's force -10 and order 5), and behind them one decay repeller per partner sphere
    (ids 20 ..; safe distance 0.001, `force` -2, `order` 2), parked at PARKED.  Spheres: radius 0.05 .. 0.08 m on links 4, 6 and n (a 14-joint chain: 4, 6, 11
    and n), centres a few centimetres off the link origins.
    The partner's base is a pure translation away: xform[b] = [I | t_b], t_{b^1} = -t_b, and t_b of the even arm is chosen so that AT THE
    GOALS the origin of the odd arm's link n - 1 stands `gap` metres (in x) from the even arm's flange -- both goals lie in the shared
    region, each arm ends beside spheres of the other.
    Why force -2 and order 2 for the partner's spheres.  A repeller pushes with |force| ((radius + safe) / D)^order against the goal's unit
    pull, and the sum is normalised.  The feeder's -10 and order 5 is a wall: 5e-3 of the goal's pull at 0.3 m, more than the goal's pull
    inside 0.1 m -- a scene in which every pair feels it has arms pressed into a sphere that covers their goal, and those amplify a
    perturbation of the start by 1e-13 to 1e-10 .. 1e-2 (measured at gaps of 0.2 m and less): a move that no two implementations repeat
    to 1e-8.  With -2 and order 2 the push is 0.1 of the goal's pull at 0.3 m and passes it only inside 1.4 radii: every paired arm's
    joint path leaves the uncoupled one by 7.8e-4 rad or more (the median arm by 1.5e-2), and a perturbation of 1e-13 stays 3e-13.
    far: these arms' goal positions times 3, out of reach (tests/test_gpu_stall.py): they never arrive.
    n_way > 0: way (B, n_way, 16), the frames of q0 + (w + 1) / n_way (qg - q0) -- the last one is the goal --; arm 5's list has two rows and
    arm 8's none (a NaN row ends a list): arm 8 is kept out, and is an obstacle for arm 9 at the posture it starts in.
    Returns dict(w, q0, spheres, src_arm, xform, first_rep, way)."""
    from vfclik_amd import synth
    n = chain.n
    rng = np.random.default_rng(seed)
    links = links or ((4, 6, 11, n) if n > 7 else (4, 6, n))
    spheres = [(l, tuple(rng.uniform(-0.03, 0.03, size=3)), float(rng.uniform(0.05, 0.08))) for l in links]
    L = len(spheres)
    w = synth.make_workload(chain, B, n_static, seed=seed, io_dtype=io_dtype, max_fields=1 + n_static + L)
    qg = rng.uniform(0.6 * chain.q_lo, 0.6 * chain.q_hi, size=(B, n))
    s = rng.uniform(spread[0], spread[1], size=(B, 1))
    q0 = (qg + s * rng.uniform(-1.0, 1.0, size=(B, n))).astype(io_dtype).astype(np.float64)
    goal = chain.fk(qg).reshape(B, 16)
    if far is not None:
        goal[far, 3::4] *= [3.0, 3.0, 3.0, 1.0]   # out of reach (tests/test_gpu_stall.py): such an arm never arrives
    w["fields"]["p"][:, 0, :16] = goal.astype(io_dtype).astype(np.float64)
    for j in range(L):
        f = w["fields"][:, 1 + n_static + j]
        f["id"], f["type"], f["force"] = 20 + j, _abi.FIELD_REPELLER, force
        f["p"][:, 0:3] = PARKED
        f["p"][:, 3] = np.float64(io_dtype(spheres[j][2]))
        f["p"][:, 4] = np.float64(io_dtype(0.001))
        f["p"][:, 5] = order
    w["nfields"][:] = 1 + n_static + L
    b = np.arange(B)
    src = (b ^ 1).astype(np.int32)
    src[src >= B] = -1
    flange = chain.fk(qg)[:, :3, 3]
    wrist = hl.truncated(chain, n - 1).fk(qg[:, :n - 1])[:, :3, 3]
    xform = np.tile(np.eye(3, 4).reshape(12), (B, 1))
    for e in range(0, B - 1, 2):
        t = flange[e] - wrist[e + 1] + np.array([gap, 0.0, 0.0])   # the odd arm's base as the even arm sees it
        xform[e, [3, 7, 11]] = t
        xform[e + 1, [3, 7, 11]] = -t
    xform = xform.astype(io_dtype).astype(np.float64)
    way = None
    if n_way:
        qw = np.stack([q0 + (i + 1) / n_way * (qg - q0) for i in range(n_way)], axis=1)
        qw[:, -1] = qg
        way = chain.fk(qw.reshape(B * n_way, n)).reshape(B, n_way, 16).astype(io_dtype).astype(np.float64)
        way[5, 2:, 0] = np.nan
        way[8, 0:, 0] = np.nan
    return dict(w=w, q0=q0, spheres=spheres, src_arm=src, xform=xform, first_rep=n_static, way=way)


# ---- the moves of tests/test_gpu_coupled_moves.py, each computed once per process and never modified ------------------------------------
N_CYCLES, DT, PREC = 160, 0.01, (0.01, 0.05)
MARGIN = {np.dtype(np.float64): (1e-6, 0.05), np.dtype(np.float32): (1e-4, 0.15)}   # the suite's margin around a threshold and the cap
PATH_BAR = {np.dtype(np.float64): 1e-8, np.dtype(np.float32): 2e-6}                 # ... and its bars on the joint path
MOVES = {"goto64": dict(robot="lwr", B=203, io_dtype=np.float64, stride=1, hold=False, flags=_abi.F_NULLSPACE | _abi.F_MIXER, seed=9),
         "goto32": dict(robot="lwr", B=203, io_dtype=np.float32, stride=4, hold=True, flags=0, seed=9),
         "stall64": dict(robot="lwr", B=203, io_dtype=np.float64, stride=4, hold=True, flags=0, seed=9, far=slice(3, None, 8)),
         "follow": dict(robot="lwr_dual14", B=130, io_dtype=np.float64, stride=4, hold=True, seed=9, n_way=3,
                        flags=_abi.F_NULLSPACE | _abi.F_JOINT_LIMIT_TASK | _abi.F_MIXER)}
_CACHE = {}


def reference(oc, name, coupling="pairs", rule=None):
    """(case, params, result) of MOVES[name].  coupling: "pairs" (the case's), "none" (the coupling set, every source -1) or "off"
    (timed_reference alone).  rule: a timed_reference.Rule."""
    key = (name, coupling, None if rule is None else (rule.patience, rule.eps, rule.eps_js, rule.stop))
    if key not in _CACHE:
        from vfclik_amd import robots
        m = MOVES[name]
        chain = robots.by_name(m["robot"])
        c = pair_case(chain, m["B"], m["io_dtype"], seed=m["seed"], n_way=m.get("n_way", 0), far=m.get("far"))
        c["chain"] = chain
        params = _abi.default_params(flags=m["flags"], max_vel=0.7)
        kw = dict(hold=m["hold"], clamp=True, io_dtype=m["io_dtype"], stepped=chain.n > 7, want=("qdot_out",), rule=rule)
        args = (oc, chain, params, c["q0"], c["w"]["fields"], c["w"]["nfields"])
        coup = dict(spheres=c["spheres"], src_arm=c["src_arm"] if coupling == "pairs" else np.full(m["B"], -1, dtype=np.int32),
                    xform=c["xform"], first_rep=c["first_rep"])
        if c["way"] is None:
            r = (tr.goto(*args, N_CYCLES, m["stride"], DT, PREC, **kw) if coupling == "off" else
                 goto(*args, N_CYCLES, m["stride"], DT, PREC, coup, **kw))
        else:
            r = (tr.follow(*args, c["way"], N_CYCLES, m["stride"], DT, PREC, **kw) if coupling == "off" else
                 follow(*args, c["way"], N_CYCLES, m["stride"], DT, PREC, coup, **kw))
        for v in list(r.values()) + [c["q0"], c["xform"], c["src_arm"], c["w"]["fields"], c["w"]["nfields"]]:
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _CACHE[key] = (c, params, r)
    return _CACHE[key]


def left_out(r, part, io_dtype, src_arm=None, hold=False, extra=None):
    """(out, near, share, cap): the arms within the margin of a threshold in the REFERENCE's run (`extra`: further such arms), the arms
    left out of the exact comparison -- those and, under `hold`, the arms they are the source of: an arm that stops at another check than
    the reference's is another obstacle for its partner from there on -- and their share of the arms that take part"""
    margin, cap = MARGIN[np.dtype(io_dtype)]
    near = r["closest"] < margin
    if extra is not None:
        near = near | extra
    out = near.copy()
    if hold and src_arm is not None:
        out |= np.where(src_arm >= 0, near[np.maximum(src_arm, 0)], False)
    return out, near, np.count_nonzero(out & part) / max(np.count_nonzero(part), 1), cap
