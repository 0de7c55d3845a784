"""Non-finite inputs in the rows of a few arms of a batch (`poison`), and what the C oracle makes of them: the yardstick of the
isolation contract of include/vfik.h (C1 isolation, C2 no laundering, C3 recovery).

A poison KIND is one way of spoiling the rows of the arms P, and of P alone:

    q_nan_first, q_nan_last      NaN in the first / the last joint angle
    q_pos_inf, q_neg_inf         +inf / -inf in the middle joint angle
    null_control_nan             NaN in /control (element 0: the one a one-dimensional null space reads)
    q_ref_nan                    NaN in an element of the joint controller's reference other than the first (a NaN FIRST element is
                                 the "no controller" convention of io->q_ref)
    q_lo_nan, q_hi_nan           NaN in this cycle's per-arm joint limits
    ext_nan                      NaN in the arm's row of mixer channel 3 (vfik_set_ext_cmd)
    goal_pos_nan, goal_rot_nan,  a goal row sent through vfik_move_fields_host whose first element is finite and whose x position
    goal_pos_inf, goal_rot_inf   (element 3) / a rotation entry (element 1) is NaN / +inf
    rep_nan, rep_inf             row REP_K of the repeller rows of the same call with y (element 1) NaN / +inf

(A repeller's radius is no poison kind: include/vfik.h puts radius >= 0 on the caller.  Non-finite orders, types and forces change the
launch plan and are no kinds either.)  Scene kinds do not touch what plan_scene decides: both runs launch the same kernels.

`Inputs` is one cycle's inputs of the whole batch, `poison(kind, inputs, P)` a spoiled copy, `oracle_cycle` the C oracle on the rows of
a few arms with its own nullspace states -- the joint controller by vfo_joint_p into channel 2 as the kernels form it, the moved scene
by `moved_fields`, the host model of vfik_move_fields_host --, `oracle_rollout` the same stepped with the Euler update and np.clip
where the run clamps (np.clip keeps a NaN; tests/test_gpu_rollout.py:_oracle_rollout).

The comparators are the contract's sentences: `laundered` (C2: wherever the oracle's element is not finite the kernel's is not finite
either; where both are finite they agree within `tol`), `soft_differences` (pose, v6, qdist, goal_dist of a poisoned arm: compared only
where both sides are finite -- the kernels' DH pattern skips arithmetic on structural zeros where the oracle's general product has
0 * NaN) and `unrecovered` (C3: every row of the oracle that is finite again is the kernel's within `tol`).

SWALLOWED lists the kinds the SPECIFICATION itself swallows -- the oracle's command row stays finite --, each with the lines of
oracle/vfik_oracle.c that do it; tests/test_poison_reference.py asserts the list against the oracle, and everything a GPU test takes for
granted about the oracle's side.

A helper of the suite, not a conftest.py."""
import ctypes as C

import numpy as np

from vfclik_amd import _abi

Q_KINDS = ("q_nan_first", "q_nan_last", "q_pos_inf", "q_neg_inf")
OPTION_KINDS = ("null_control_nan", "q_ref_nan", "q_lo_nan", "q_hi_nan", "ext_nan")
SCENE_KINDS = ("goal_pos_nan", "goal_rot_nan", "goal_pos_inf", "goal_rot_inf", "rep_nan", "rep_inf")
KINDS = Q_KINDS + OPTION_KINDS + SCENE_KINDS
EXT_CHANNEL = 3      # the mixer channel of ext_nan (2 is the joint controller's)
REP_K = 1            # the decay repeller (ascending id) of rep_nan / rep_inf
COMMAND_ROWS = ("qdot_vf", "qdot_null", "qdot_out")
SOFT_ROWS = ("pose", "pose_nt", "v6", "qdist", "goal_dist")

# What the specification swallows: a goal ROTATION that is not finite.  The attractor's turn is guarded by `th > EPS_LEN`, which a NaN angle
# fails, and its slow-down scalar by fmin(1.0, x), which returns 1.0 for a NaN x: such a goal turns the arm nowhere and the rest of the
# field acts as before.  (A goal POSITION or a repeller row that is not finite is not swallowed: the pull, or the push, is NaN, the sum is,
# and normCart keeps it -- `!(n <= EPS_LEN)`, a NaN is no short length --, so the command is NaN and VFIK_ST_NAN is set.)
SWALLOWED = {
    "goal_rot_nan": "oracle/vfik_oracle.c:131-132 (th = rot_log is NaN, `th > EPS_LEN` fails: no turn) and :135 (fmin(1.0, NaN) = 1.0)",
    "goal_rot_inf": "oracle/vfik_oracle.c:131-132 (th, or the axis over it, is not finite) and :194 (`nr > EPS_LEN` fails on the NaN sum: no turn)",
}


def arms(B, family=None):
    """P of a batch of B arms with a partial last wave: first and last lane of the first wave, first lane of the second, the last arm;
    the eight-lanes kernel (8 arms a wave): also the last arm of its first wave and the first of its second; the two-waves build: the
    first arm beyond one wave per SIMD of 256 CUs instead of arm 64."""
    assert B % 64 != 0 and B > 65
    if family == "two-waves":
        assert B > 65537
        return np.array([0, 63, 65536, B - 1])
    if family == "eight-lanes":
        return np.array([0, 7, 8, 63, 64, B - 1])
    return np.array([0, 63, 64, B - 1])


class Inputs:
    """One cycle's inputs of the whole batch: q (B, n) and, each an array or None, null_control (B, 4), q_ref, q_lo, q_hi, ext (B, n)
    (mixer channel EXT_CHANNEL), goal (B, 16) and rep (B, K, 4) (the rows of one vfik_move_fields_host call)."""
    NAMES = ("q", "null_control", "q_ref", "q_lo", "q_hi", "ext", "goal", "rep")

    def __init__(self, q, **kw):
        self.q = q
        for k in self.NAMES[1:]:
            setattr(self, k, kw.pop(k, None))
        assert not kw, kw

    def copy(self):
        return Inputs(**{k: (None if getattr(self, k) is None else np.array(getattr(self, k), dtype=np.float64, copy=True)) for k in self.NAMES})


def needs(kind):
    """the member of Inputs a kind spoils"""
    if kind in Q_KINDS:
        return "q"
    return {"null_control_nan": "null_control", "q_ref_nan": "q_ref", "q_lo_nan": "q_lo", "q_hi_nan": "q_hi", "ext_nan": "ext"}.get(
        kind, "goal" if kind.startswith("goal") else "rep")


def poison(kind, inputs, P):
    """A copy of `inputs` with the rows of the arms P spoiled; every other row, and every other member, bit for bit as it was."""
    assert kind in KINDS, kind
    x = inputs.copy()
    a = getattr(x, needs(kind))
    assert a is not None, "%s needs %s" % (kind, needs(kind))
    n = x.q.shape[1]
    if kind == "q_nan_first":
        a[P, 0] = np.nan
    elif kind == "q_nan_last":
        a[P, n - 1] = np.nan
    elif kind == "q_pos_inf":
        a[P, n // 2] = np.inf
    elif kind == "q_neg_inf":
        a[P, n // 2] = -np.inf
    elif kind == "null_control_nan":
        a[P, 0] = np.nan
    elif kind in ("q_ref_nan", "q_lo_nan", "q_hi_nan", "ext_nan"):
        a[P, 1 + (n // 2)] = np.nan
    elif kind.startswith("goal"):
        assert np.all(np.isfinite(a[P, 0]))
        a[P, 3 if "pos" in kind else 1] = np.nan if kind.endswith("nan") else np.inf
    else:
        assert np.all(np.isfinite(a[P, REP_K, 0]))
        a[P, REP_K, 1] = np.nan if kind.endswith("nan") else np.inf
    return x


# ---- the moved scene ------------------------------------------------------------------------------------------------------------------
def goal_slot(fields, nfields):
    """(B,) index of every arm's lowest-id attractor -- its goal block --, -1 without one"""
    slot = np.full(fields.shape[0], -1)
    for b in range(fields.shape[0]):
        f = fields[b, : int(nfields[b])]
        idx = np.flatnonzero(f["type"] == _abi.FIELD_ATTRACTOR)
        if len(idx):
            slot[b] = idx[np.argmin(f["id"][idx])]
    return slot


def moved_fields(fields, nfields, goal, rep, io_dtype):
    """vfik_move_fields_host on the host: a copy of `fields` (b, M) with rows 0-2 of `goal` (b, 16) in every arm's goal block and row k of
    `rep` (b, K, 4) = x y z radius in its k-th decay repeller in ascending-id order, rounded to the I/O type.  A row whose FIRST element
    is NaN leaves its primitive alone; a NaN or an infinity behind a finite first element goes in as it is."""
    F = np.array(fields, copy=True)

    def rnd(a):
        return np.asarray(a, dtype=np.float64).astype(io_dtype).astype(np.float64)
    slot = goal_slot(F, nfields)
    for b in range(F.shape[0]):
        if goal is not None and slot[b] >= 0 and not np.isnan(goal[b, 0]):
            F["p"][b, slot[b], :12] = rnd(goal[b, :12])
        if rep is not None:
            f = F[b, : int(nfields[b])]
            idx = np.flatnonzero(f["type"] == _abi.FIELD_REPELLER)
            idx = idx[np.argsort(f["id"][idx], kind="stable")]
            for k in range(min(len(idx), rep.shape[1])):
                if not np.isnan(rep[b, k, 0]):
                    F["p"][b, idx[k], 0:4] = rnd(rep[b, k])
    return F


# ---- the oracle on the rows of a few arms ---------------------------------------------------------------------------------------------
def joint_channel(oc, chain, params, q_ref, q, q_lo, q_hi):
    """(b, n) the joint P controller's command (vfo_joint_p, per arm on its own limits) and (b,) whether the arm has a controller: a row
    that starts with NaN has none"""
    fn = oc.lib().vfo_joint_p
    fn.restype = C.c_int
    b, n = q.shape
    out = np.zeros((b, n))
    has = ~np.isnan(q_ref[:, 0])
    for i in np.flatnonzero(has):
        lo = np.ascontiguousarray(chain.q_lo if q_lo is None else q_lo[i], dtype=np.float64)
        hi = np.ascontiguousarray(chain.q_hi if q_hi is None else q_hi[i], dtype=np.float64)
        r, qq = np.ascontiguousarray(q_ref[i], dtype=np.float64), np.ascontiguousarray(q[i], dtype=np.float64)
        fn(oc._p(r), oc._p(qq), oc._p(lo), oc._p(hi), C.c_int(n), C.c_double(params.jp_kp), C.c_double(params.jp_delta), oc._p(out[i]))
    return out, has


def oracle_cycle(oc, chain, params, fields, nfields, tool, inputs, idx, io_dtype, states=None,
                 want=COMMAND_ROWS + ("pose", "pose_nt", "v6", "qdist", "status")):
    """One cycle of the C oracle on the arms idx of the batch: fields / nfields / tool (None, (16,) or (B, 16)) and every member of
    `inputs` are the whole batch's.  states: the oracle's nullspace states of these arms (oracle_c.new_states(len(idx), n)), kept by
    the caller from cycle to cycle.  Returns oracle_c.cycle_batch's dict."""
    idx = np.asarray(idx)
    x = inputs

    def rows(a):
        return None if a is None else np.asarray(a, dtype=np.float64)[idx]
    q = rows(x.q)
    F = moved_fields(fields[idx], nfields[idx], rows(x.goal), rows(x.rep), io_dtype)
    ext = None
    if x.ext is not None or x.q_ref is not None:
        ext = np.zeros((4, len(idx), chain.n))
        if x.ext is not None:
            ext[EXT_CHANNEL - 2] = rows(x.ext)
        if x.q_ref is not None:
            jc, has = joint_channel(oc, chain, params, rows(x.q_ref), q, rows(x.q_lo), rows(x.q_hi))
            ext[0] = np.where(has[:, None], jc, ext[0])
    t = tool
    if t is not None and np.ndim(t) == 2:
        t = np.asarray(t)[idx]
    kw = {} if x.q_lo is None else dict(q_lo=rows(x.q_lo), q_hi=rows(x.q_hi))
    return oc.cycle_batch(chain, params, q, F, nfields[idx], tool=t, null_control=rows(x.null_control), ext_cmd=ext, states=states,
                          want=tuple(k for k in want if k not in ("q", "goal_dist")), **kw)


def oracle_rollout(oc, chain, params, fields, nfields, tool, q, idx, io_dtype, n_cycles, dt, clamp, states=None):
    """n_cycles cycles of the C oracle on the arms idx from q (B, n): q += dt qdot_out, np.clip to the chain's limits where `clamp`
    (a NaN stays a NaN), rounded to a float32 I/O type every cycle as tests/test_gpu_variants.py steps it.  Returns (q (b, n) after the
    last cycle, the last cycle's rows)."""
    qb = np.array(q, dtype=np.float64)[np.asarray(idx)]
    ref = None
    sub = np.arange(len(qb))
    for _ in range(n_cycles):
        ref = oracle_cycle(oc, chain, params, fields[idx], nfields[idx], tool if tool is None or np.ndim(tool) == 1 else np.asarray(tool)[idx],
                           Inputs(qb), sub, io_dtype, states=states, want=COMMAND_ROWS + ("pose", "status"))
        qb = qb + dt * ref["qdot_out"]
        if clamp:
            qb = np.clip(qb, chain.q_lo, chain.q_hi)
        if np.dtype(io_dtype) == np.float32:
            qb = qb.astype(np.float32).astype(np.float64)
    return qb, ref


# ---- the contract's sentences -----------------------------------------------------------------------------------------------------------
def laundered(got, ref, tol):
    """C2 on one row set of the arms P (got, ref: (p, K)).  Returns (the number of elements where the oracle is not finite and the kernel
    is, the number where both are finite and differ by `tol` or more, the largest difference where both are finite -- 0.0 without one)."""
    g, r = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    both = np.isfinite(g) & np.isfinite(r)
    with np.errstate(invalid="ignore"):
        err = np.where(both, np.abs(g - r), 0.0)
    return int(np.count_nonzero(~np.isfinite(r) & np.isfinite(g))), int(np.count_nonzero(err >= tol)), float(err.max(initial=0.0))


def soft_differences(got, ref, tol):
    """pose, v6, qdist, goal_dist of a poisoned arm: (the number of elements finite on both sides that differ by `tol` or more, the
    largest such difference)"""
    _, n, e = laundered(got, ref, tol)
    return n, e


def unrecovered(got, ref, tol):
    """C3 on one row set of the arms P: the number of arms whose oracle row is finite throughout while the kernel's is not, or is `tol` or
    more away; and the largest difference over the rows that are finite on the oracle's side."""
    g, r = np.asarray(got, dtype=np.float64).reshape(len(got), -1), np.asarray(ref, dtype=np.float64).reshape(len(ref), -1)
    fin = np.all(np.isfinite(r), axis=1)
    with np.errstate(invalid="ignore"):
        err = np.where(np.isfinite(g[fin]), np.abs(g[fin] - r[fin]), np.inf)
    worst = err.max(axis=1, initial=0.0) if err.size else np.zeros(0)
    return int(np.count_nonzero(~(worst < tol))), float(worst.max(initial=0.0))


def nan_bit(status):
    return (np.asarray(status) & _abi.ST_NAN) != 0


def same_bits(a, b):
    """bit-for-bit equality of two arrays of one dtype (a NaN equals itself only with the same payload)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- the families of cycle kernels, and the handles of tests/test_gpu_variants.py without a device --------------------------------------
FAMILIES = ("lean", "publishing", "eight-lanes", "MIXO", "general", "uniform", "heavy", "two-waves")
NOT_BUILT = {("two-waves", 64)}      # the two-waves-per-SIMD build exists for float32 I/O alone (vfik_kernel.h: plan_detail::route)
SEED = 4242
RECOVERY_CYCLES = 1                  # the oracle's rows of P are finite again in the first clean cycle, with no reset (asserted on the CPU)
MIX_W = (1.0, 1.0, 0.5, 0.25, 0.0, 0.0)   # the joint controller's channel and EXT_CHANNEL with weights of their own


def _tv():
    import test_gpu_variants as tv
    return tv


def family_of(r):
    """the family a tests/test_gpu_variants.py Recipe belongs to (a variant may be in none: the rollouts, the stepped cycles, ...)"""
    a = r.v.args
    if r.roll:
        return None
    if r.v.kernel.startswith("cycle_sub8"):
        return "eight-lanes"
    if r.mixo:
        return "MIXO"
    if r.big:
        return "two-waves"
    if r.v.heavy:
        return "heavy"
    if not r.fastf:
        return "general" if a["LEAN"] == 0 else None
    if r.uni:
        return "uniform"
    if a["LEAN"] == 1 and not r.fun:
        return "lean"
    if a["LEAN"] == 0 and r.plain and not r.fun:
        return "publishing"
    return None


def pick(by_group, family, io):
    """The variant a family is tried on at an I/O type: the 7-joint chain (heavy: 14 joints) on its DH pattern, no shared tool or IK
    weights, with the nullspace module where the family has such a variant, publishing where it can (so that every row is looked at)."""
    tv = _tv()
    nj = 14 if family == "heavy" else 7
    best = None
    for ns in (True, False):
        for v in by_group.get((nj, io, ns), []):
            r = tv.Recipe(v)
            if family_of(r) != family:
                continue
            score = (r.plain, not r.shared_tool and not r.shared_wts, r.pattern, r.want == tv.ROWS, v.args.get("CF", -1) == -1)
            if best is None or score > best[0]:
                best = (score, r)
        if best is not None:
            break
    assert best is not None, "no %s variant for float%d I/O in the library" % (family, io)
    return best[1]


def full_launch(r):
    """the recipe's launch takes per-arm options (CycleFamily::Full): the joint controller, per-arm limits, an external command"""
    return r.v.args.get("LEAN", 3) == 0 and r.plain


def kinds_of(family, r):
    kinds = list(Q_KINDS)
    if r.ctrl:
        kinds.append("null_control_nan")
    if full_launch(r):
        assert r.limits
        kinds += ["q_ref_nan", "q_lo_nan", "q_hi_nan", "ext_nan"]
    return tuple(kinds) + SCENE_KINDS


def host_env():
    """what tests/test_gpu_variants.py's fixture holds, with an engine module that needs no device: its Engine takes the setters and answers
    the structure questions as the recipe says (the GPU tests ask the real one)"""
    from oracle import oracle_c
    from vfclik_amd import _abi, chain, robots, synth
    oracle_c.build()

    class E:
        pass
    e = E()
    e.oc, e.abi, e.chain, e.robots, e.synth = oracle_c, _abi, chain, robots, synth
    return e


class _NoDevice:
    def __init__(self, r):
        self.field_path = 0 if r.fields == "general" else 2 if r.fields in ("fun", "mixo_fun") else 1
        self.uniform_repellers = r.fields not in ("pairs", "general")
        self.mixed_orders = r.fields in ("mixo", "mixo_fun")

    def Engine(self, *a, **kw):
        return self

    def set_fields(self, *a, **kw):
        pass

    set_tool = close = set_fields


def host_handle(env, r, seed):
    """tests/test_gpu_variants.py's Handle of a recipe -- chain, fields, tool, limits, /control, the second cycle's q -- without an engine"""
    class E:
        pass
    e = E()
    e.__dict__.update(env.__dict__)
    e.engine = _NoDevice(r)
    return _tv().Handle(e, r, seed)


def family_setup(h, family):
    """mixer weights for the joint controller's and the external channel (the handle's own params object: the engine's too)"""
    for i, w in enumerate(MIX_W):
        h.params.mix_w[i] = w
    if hasattr(h.eng, "set_params"):
        h.eng.set_params()


def family_inputs(h, r, family, second=False):
    """The clean inputs of a family's launch: the recipe's (q, /control and per-arm limits where it takes them), a scene move that shifts
    the goal and the repellers a little, and for the launches that take per-arm options a joint reference near q and an external command.
    second: the cycle behind it (the handle's second q, the scene moved on)."""
    B, n = h.w["q"].shape
    rng = np.random.default_rng(SEED + (1 if second else 0))
    q = h.q2 if second else h.w["q"]
    F = h.w["fields"]
    goal = np.array(F["p"][:, 0, :16], copy=True)
    goal[:, [3, 7, 11]] += rng.uniform(-0.01, 0.01, (B, 3))
    rep = np.array(F["p"][:, 1:4, 0:4], copy=True)
    rep[:, :, 0:3] += rng.uniform(-0.01, 0.01, (B, 3, 3))
    x = Inputs(q, goal=goal, rep=rep)
    if r.ctrl:
        x.null_control = h.ctrl
    if r.limits:
        x.q_lo, x.q_hi = h.q_lo, h.q_hi
    if full_launch(r):
        dt = r.t
        x.q_ref = (q + rng.uniform(-0.2, 0.2, (B, n))).astype(dt).astype(np.float64)
        x.q_ref[1::5, 0] = np.nan        # some arms without a controller: the "leave alone" convention beside the poison
        x.ext = rng.uniform(-0.1, 0.1, (B, n)).astype(dt).astype(np.float64)
    return x


def mixed_q(q, P):
    """q with the four q kinds dealt out over the arms of P in turn"""
    x = Inputs(np.array(q, dtype=np.float64, copy=True))
    for i, kind in enumerate(Q_KINDS):
        if len(P[i::4]):
            x = poison(kind, x, P[i::4])
    return x.q


# ---- the five timed moves with a poisoned start ---------------------------------------------------------------------------------------------
MOVES = ("goto", "follow", "goto_js", "follow_js", "script")
MOVE_B, MOVE_CYCLES, MOVE_STRIDE, MOVE_DT = 130, 24, 4, 0.02
MOVE_PREC, MOVE_VIA = (0.01, 0.05), (0.03, 0.15)
MOVE_RULE = dict(patience=2, eps=(1e-4, 1e-3), eps_js=1e-4, stop=True)
MOVE_MIX = (1.0, 1.0, 1.0, 0.0, 0.0, 0.0)     # the handle's mixer of goto, follow and the two js forms: field, nullspace and joint controller
MOVE_WANT = ("qdot_out", "status")
MOVE_MARGIN = {np.dtype(np.float64): 1e-7, np.dtype(np.float32): 4e-6}   # (tests/test_gpu_goto_js.py: an arm this near a threshold in the oracle's run)
MOVE_TOL = {np.dtype(np.float64): (1e-8, 1e-7), np.dtype(np.float32): (2e-6, 2e-5)}   # q_traj, qdot_out (tests/test_gpu_goto_js.py)


def move_js_prec(n):
    return 0.004 + 0.002 * np.arange(n), 3.0 * (0.004 + 0.002 * np.arange(n))


def move_case(io_dtype, poisoned):
    """130 LWR arms, each near a posture of its own: goal frame and joint reference are that posture's, the lists pass half way first
    (every fifth arm's list is one step long), the scripts mix frames and postures.  poisoned: q[P, 2] = NaN at the start."""
    from vfclik_amd import robots, synth
    io_dtype = np.dtype(io_dtype)

    def rnd(a):
        return np.asarray(a, dtype=np.float64).astype(io_dtype).astype(np.float64)
    chain = robots.lwr()
    B, n = MOVE_B, chain.n
    w = synth.make_workload(chain, B, 2, seed=61, io_dtype=io_dtype.type)
    rng = np.random.default_rng(62)
    qg = rnd(rng.uniform(0.6 * chain.q_lo, 0.6 * chain.q_hi, size=(B, n)))
    s = np.where(np.arange(B) % 2 == 0, 0.004, 0.04)[:, None]
    q0 = rnd(qg + s * rng.uniform(-1.0, 1.0, size=(B, n)))
    mid = rnd(0.5 * (q0 + qg))
    way = rnd(np.stack([chain.fk(mid).reshape(B, 16), chain.fk(qg).reshape(B, 16)], axis=1))
    wayq = np.stack([mid, qg], axis=1)
    w["fields"]["p"][:, 0, :16] = way[:, 1]
    way_l, wayq_l = way.copy(), wayq.copy()
    way_l[::5, 1, 0] = np.nan
    wayq_l[::5, 1, 0] = np.nan
    F_, P_ = _abi.STEP_FRAME, _abi.STEP_POSTURE
    kind = np.array([[P_, F_], [F_, P_], [F_, F_], [P_, P_], [P_, 0]], dtype=np.int32)[np.arange(B) % 5]
    P = arms(B)
    if poisoned:
        q0 = q0.copy()
        q0[P, 2] = np.nan
    params = _abi.default_params(flags=_abi.F_NULLSPACE | _abi.F_MIXER, mix_w=list(MOVE_MIX), jp_kp=8.0)
    return dict(chain=chain, w=w, q0=q0, q_ref=qg, way=way_l, wayq=wayq_l, way_s=way, wayq_s=wayq, kind=kind, P=P, params=params, io_dtype=io_dtype)


def move_reference(oc, c, move, clamp, hold, rule):
    """tests/timed_reference.py's run of a case"""
    import timed_reference as tr
    chain, w, io = c["chain"], c["w"], c["io_dtype"]
    prec, via = move_js_prec(chain.n)
    kw = dict(hold=hold, clamp=clamp, io_dtype=io, want=MOVE_WANT, rule=tr.Rule(**MOVE_RULE) if rule else None)
    a = (oc, chain, c["params"], c["q0"], w["fields"], w["nfields"])
    t = (MOVE_CYCLES, MOVE_STRIDE, MOVE_DT)
    if move == "goto":
        return tr.goto(*a, *t, MOVE_PREC, **kw)
    if move == "follow":
        return tr.follow(*a, c["way"], *t, MOVE_PREC, MOVE_VIA, **kw)
    if move == "goto_js":
        return tr.goto_js(*a, c["q_ref"], *t, prec, **kw)
    if move == "follow_js":
        return tr.follow_js(*a, c["wayq"], *t, prec, via, **kw)
    return tr.script(*a, c["kind"], c["way_s"], c["wayq_s"], *t, MOVE_PREC, prec, MOVE_VIA, via, **kw)


def under_way(r, n_checks, stride):
    """(n_checks, B) bool: the arms that count in pending after every check, from a run's own arrays (arrived, or reached / next with the
    lengths `length`; stalled where a rule ran): taking part, not at the end of the list, not stalled by then."""
    cyc = (np.arange(n_checks)[:, None] + 1) * stride - 1
    if "arrived" in r:
        last = r["arrived"][None, :]
        part = np.ones(last.shape[1], dtype=bool) if "length" not in r else r["length"] > 0
    else:
        L = r["length"]
        part = L > 0
        last = r["reached"][np.arange(len(L)), np.maximum(L - 1, 0)][None, :]
    uw = part[None, :] & ~((last >= 0) & (last <= cyc))
    if "stalled" in r:
        st = r["stalled"][None, :]
        uw &= ~((st >= 0) & (st <= cyc))
    return uw


def poll_prediction(pending, poll):
    """checks_run of a host form under `poll`: the first multiple of poll at which pending is 0, if it comes before the end"""
    n = len(pending)
    zero = np.flatnonzero((np.asarray(pending)[poll - 1::poll] == 0) & (np.arange(poll, n + 1, poll) < n))
    return int(poll * (zero[0] + 1)) if len(zero) else n


# ---- finite but far-out joint angles ----------------------------------------------------------------------------------------------------
FAR_SCALES = (10.0, 1e3, 1e5)
FAR_B = 64 + 13
FAR_CHAINS = ("powercube6", "lwr", "lwr_dual14", "lwr eight-lanes")   # sin / cos: the table (6 and 7 joints), table-free (14), the eight-lanes kernel's


def far_case(name, scale, io_dtype):
    """(chain, q): FAR_B arms with every |q_i| in [scale / 2, scale], signs mixed, rounded to the I/O type"""
    from vfclik_amd import robots
    chain = robots.by_name(name.split()[0])
    rng = np.random.default_rng(int(scale) + chain.n)
    q = rng.uniform(0.5, 1.0, (FAR_B, chain.n)) * rng.choice([-1.0, 1.0], (FAR_B, chain.n)) * scale
    return chain, q.astype(io_dtype).astype(np.float64)


def far_units(chain):
    """The error units of a published frame: (E_R, E_p).  Each joint multiplies the frame by a rotation whose sine and cosine are good to an
    ulp of a number at most 1, and rounds its products: u per joint for a rotation entry, u times the chain's reach per joint for the
    position (u = 2^-53; the reach: the lengths of the fixed frames' offsets)."""
    u = 2.0 ** -53
    reach = float(sum(np.linalg.norm(np.asarray(chain.B[i])[:3, 3]) for i in range(chain.n + 1)))
    return chain.n * u, chain.n * u * max(reach, 1.0)


def far_reference(name, scale, io_dtype, chain, q):
    """(hi, lo) (B, 12) each: the 50-digit tool frame (tests/hp_reference.py), rows 0-2 of the published 4 x 4"""
    import hp_reference as hp
    kin = hp.kinematics(("far", name.split()[0], np.dtype(io_dtype).name, float(scale)), chain, q)
    hi, lo = np.zeros((len(q), 12)), np.zeros((len(q), 12))
    for b, (T, _J) in enumerate(kin):
        for r in range(3):
            for c in range(4):
                hi[b, 4 * r + c], lo[b, 4 * r + c] = hp._hilo(T[r][c])
    return hi, lo


def far_offsets(name):
    """(n,) the DH angle offsets the kernels' form of the chain adds to the joint angles (KConst::dh[i].off, vfik_kconst.h: multiples of pi for
    these robots), read from the recorded device constants of tests/golden/kconst_images.npz"""
    import os
    import test_kconst as tk
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kconst_images.npz"))
    robot = name.split()[0]
    names = [str(x) for x in z["names"]]
    ends = np.cumsum(z["lengths"])
    i = names.index(robot)
    nj = {"powercube6": 6, "lwr": 7, "lwr_dual14": 14}[robot]
    dt = tk.kconst_dtype(nj)
    img = z["images"][ends[i] - z["lengths"][i]:ends[i]]
    return np.array(img[:dt.itemsize].view(dt)[0]["dh"]["off"], dtype=np.float64)


def far_angle_term(q, offsets):
    """(B,) what forming fl(q_i + off_i) can cost an arm, in radians: half an ulp of the sum, (|q_i| + |off_i|) 2^-53, for every joint whose
    offset is not zero (q + 0 is q).  A joint angle off by d moves a rotation entry by at most d and the position by at most reach x d."""
    on = np.asarray(offsets) != 0.0
    return ((np.abs(q) + np.abs(offsets)[None, :]) * on[None, :]).sum(axis=1) * 2.0 ** -53


def far_errors(pose, ref, io_dtype):
    """(B,) the largest error of a rotation entry and of a position entry of pose (B, 16); a float32 row is allowed the half ulp of its store"""
    hi, lo = ref
    err = np.abs((np.asarray(pose, dtype=np.float64)[:, :12] - hi) - lo)
    if np.dtype(io_dtype) == np.float32:
        err = np.maximum(err - 2.0 ** -24 * np.maximum(np.abs(hi), 2.0 ** -126), 0.0)
    rot = np.ones(12, dtype=bool)
    rot[[3, 7, 11]] = False
    return err[:, rot].max(axis=1), err[:, ~rot].max(axis=1)


def far_ratio(pose, ref, units, io_dtype):
    """the worst error of pose (B, 16) in its units, rotation entries and position apart: (ratio, worst absolute error); a float32 row
    is allowed the half ulp of its store"""
    hi, lo = ref
    err = np.abs((np.asarray(pose, dtype=np.float64)[:, :12] - hi) - lo)
    if np.dtype(io_dtype) == np.float32:
        err = np.maximum(err - 2.0 ** -24 * np.maximum(np.abs(hi), 2.0 ** -126), 0.0)
    rot = np.ones(12, dtype=bool)
    rot[[3, 7, 11]] = False
    return max(float(err[:, rot].max()) / units[0], float(err[:, ~rot].max()) / units[1]), float(err.max())


# ---- the observers of the cycle call ------------------------------------------------------------------------------------------------------
OBS_CYCLES, OBS_POISONED = 8, 2


def observer_memory():
    """The cycles in which io.track_error can show an input of cycle OBS_POISONED, from tests/hp_observers.py's exact reference (never from
    the kernel): the estimator is stepped over one arm's finite history twice, the second time with that cycle's frame and command moved,
    and the cycles whose row changes are returned (sorted).  The history is 5 frames and 4 commands: a row is formed from the last two
    frames and the command of three calls ago, and rows are zeros until the sixth frame."""
    import hp_observers as ho
    from vfclik_amd import robots
    chain = robots.lwr()
    rng = np.random.default_rng(8)
    T = OBS_CYCLES
    q = rng.uniform(0.5 * chain.q_lo, 0.5 * chain.q_hi, (1, chain.n)) + 0.01 * np.arange(T)[:, None, None] * rng.normal(size=(1, 1, chain.n))
    poses = np.stack([chain.fk(q[t]).reshape(1, 16) for t in range(T)])
    v6 = rng.normal(0, 0.1, (T, 1, 6))
    act = np.ones((T, 1), dtype=np.int32)
    a = ho.track_reference(("poison-memory", 0), poses, v6, act)
    poses2, v62 = poses.copy(), v6.copy()
    poses2[OBS_POISONED] = chain.fk(q[OBS_POISONED] + 0.05).reshape(1, 16)
    v62[OBS_POISONED] += 0.05
    b = ho.track_reference(("poison-memory", 1), poses2, v62, act)
    changed = np.any((a["out"] != b["out"]) | (a["out_lo"] != b["out_lo"]), axis=(1, 2))
    return [int(t) for t in np.flatnonzero(changed)]
