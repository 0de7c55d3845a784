"""The bridge back end of a control cycle on its ties: the joint P controller as mixer channel 2, the six-channel mixer, the bridge's
velocity limiter, the LWR position-command form and q_ref_out -- scenes whose arms sit ON the decisions, and the reference they are held to.

A helper of the suite, not a conftest.py: tests/test_oracle_backend_ties.py holds the C oracle to the reference on the CPU and asserts every
scene's construction conditions, tests/test_gpu_backend_ties.py holds the HIP kernels to it on the GPU.

The reference is oracle/vfik_numpy.py's `joint_p_controller`, `limiter` and `lwr_command` and the mixer's sum (command_mixer.py:78-82, `mix`
below, the loop of `CommandMixer.read`), evaluated op by op in CPython doubles: the reference project's own arithmetic, pinned by the
reference-made goldens.  Nothing here is high precision: every decision of the back end (`lead > max_vel`, `err < delta` signed,
`ref < lo` / `ref > hi`, "every mixer weight == 0") acts on exact doubles, and so does the reference.

Inputs are rounded to the I/O type before either side sees them; per-arm mixer weights and limiter speeds are stored in the I/O type by the
library, so the scenes choose values that type represents.

Every scene has B_ARMS = 192 arms (three waves, groups of eight); arm b has kind b mod (number of kinds) -- every scene has at least eight
kinds, so any eight consecutive arms hold eight different kinds -- and round g = b div (number of kinds), which moves the joint a kind acts on
(first, last, middle), its sign and the kind's sub-case.

Two statements about values that are NOT numbers, both the spec's to decide and therefore kept out of the scenes' disagreeing corner:

  * CPython's `max(map(abs, qdot))` (bridge:190) keeps a NaN that comes FIRST and drops one that comes later; the C oracle and the kernels
    form the lead with fmax, which drops every NaN.  The `nan` kind puts its NaN behind joint 0 on arms that are limited, and on joint 0
    only where no other joint exceeds max_vel: there all three agree.
  * an infinite command entry gives lead = inf, ratio = max_vel / inf = 0, so the finite joints go to (signed) zero and the infinite one to
    NaN (ST_NAN | ST_LIMITED).  The kernels' Newton reciprocal is stated for finite leads; the limiter takes 0 for an infinite one.

The limiter's stated range: rcp_nr(lead) is good for a NORMAL lead, |command| >= 2^-1022 (2.2e-308 rad/s).  A limited arm has lead > max_vel, so a
denormal lead needs max_vel below 2.2e-308 -- zero in practice: the reference then sends 0 (0 / lead), the kernels 0 * rcp_nr(denormal), which
is 0 down to a lead of 2^-1024 and NaN (flagged ST_NAN) below, where the reciprocal overflows.  No scene has such a kind: commands of 1e-308 rad/s
are outside what the bridge is specified for, and the bound is written down here and in DESIGN 5.6 instead.

The bars (derived, not measured).  Status bits and decisions: exact.  At float64 I/O the mixer's output, the controller's command, q_ref_out,
the command form and unlimited rows: bit for bit (-0.0 == 0.0, NaN where the reference has NaN).  Limited rows: LIMITED_ULP = 4 ulp of the
reference's double -- the restatement's v * (max_vel / lead) carries two roundings, the kernels' v * (max_vel * rcp_nr(lead)) three, with rcp_nr
good to 1 ulp as vfik_kernel.hip states it (two Newton steps on v_rcp_f64: the second leaves the square of a 2^-40 residual and its own
rounding): 0.5 + 0.5 ulp on one side, 1 + 0.5 + 0.5 on the other, 3 apart, and one more for a result next to a power of two, where the ulp
halves.  At float32 I/O a value
equals the reference rounded to float32; where the reference's double lies within that bar of a float32 rounding boundary the float32 on the
boundary's other side is accepted, and `compare` counts the rows that used this allowance: below ALLOWANCE_CAP = 1 % of the limited rows."""
import math

import numpy as np

B_ARMS = 192
ROBOTS = ("powercube6", "lwr", "rand10", "lwr_dual14")
LIMITED_ULP = 4.0
ALLOWANCE_CAP = 0.01
JP_DELTA, JP_KP = 2.0 ** -4, 2.0
MIXED_W = (1.0, 0.5, 0.7, 0.0, 0.25, 0.0)   # tests/test_gpu_joint_controller.py: test_joint_p_controller_is_mixer_channel_2
ST_NAN, ST_LIMIT_STOP, ST_NULL_AMBIGUOUS, ST_LIMITED, ST_JOINT_AT_GOAL = 1, 2, 4, 8, 16

LIMITER_KINDS = ("tie", "below", "above", "two_tie", "zero", "inf_max", "nan", "inf", "regular", "free")
JP_KINDS = ("err_tie", "err_below", "err_above", "neg_large", "hi_tie", "hi_beyond", "hi_inside", "lo_edge", "inf_ref", "nan_first",
            "nan_later", "regular")
FORM_KINDS = ("regular", "all_zero", "minus_zero", "denormal", "free", "two_channels", "denormal_vf", "standstill")
LO_SUB = ("tie", "beyond", "inside")


def chain_of(robot):
    """The robots of the suite; `rand10`: the 10-joint chain of tests/test_gpu_variants.py (_chain(env, 10, False): kernel_variants.chain10)."""
    from vfclik_amd import chain, robots
    if robot != "rand10":
        return robots.by_name(robot)
    import kernel_variants as kv
    return kv.chain10(robots, chain.Chain)


def _f(a, dt):
    """rounded to the I/O type, as doubles"""
    return np.asarray(a, dtype=np.float64).astype(dt).astype(np.float64)


def _next(x, up, dt):
    """the neighbour of a value of the I/O type, in the I/O type"""
    return float(np.nextafter(dt(x), dt(np.inf if up else -np.inf)))


def _beyond(x, up, dt):
    """the value of the I/O type next to the double x, strictly above (up) or below it"""
    t = float(dt(x))
    if (t > x) if up else (t < x):
        return t
    return _next(t, up, dt)


def _tiny(dt):
    return float(np.nextafter(dt(0), dt(1)))   # the smallest denormal of the I/O type


def _lead_joint(g, n):
    return (0, n - 1, n // 2)[g % 3]


class Scene:
    """The inputs of one launch: chain, I/O type, make_workload's q and field set, and what the kind of each arm sets."""

    def __init__(self, name, robot, dt, kind_names, seed):
        from vfclik_amd import synth
        self.name, self.robot, self.dt, self.kind_names = name, robot, dt, kind_names
        self.chain = chain_of(robot)
        self.n, self.B = self.chain.n, B_ARMS
        self.w = synth.make_workload(self.chain, self.B, 2, seed=seed, io_dtype=dt)
        self.q = self.w["q"]
        self.kind = np.arange(self.B) % len(kind_names)
        self.round = np.arange(self.B) // len(kind_names)
        self.rng = np.random.default_rng(seed + 100)
        self.mixw = self.max_vel = self.ext = self.q_ref = self.q_lo = self.q_hi = self.q_cmded = None
        self.limiter = False
        self.f64_only = np.zeros(self.B, dtype=bool)   # arms whose condition needs a value finer than the float32 grid

    def kind_of(self, b):
        return self.kind_names[self.kind[b]]

    def limits(self, b):
        if self.q_lo is not None:
            return list(zip(self.q_lo[b].tolist(), self.q_hi[b].tolist()))
        return list(zip(self.chain.q_lo.tolist(), self.chain.q_hi.tolist()))


def limiter_scene(robot, dt, seed=41):
    """Limiter, exact input: per-arm weights [0,0,0,1,0,0] and the command on channel 3, so the mixed command is the command; per-arm max_vel
    exactly the lead, its neighbour below or above in the I/O type, and the kinds of LIMITER_KINDS."""
    s = Scene("limiter", robot, dt, LIMITER_KINDS, seed)
    n, B, rng = s.n, s.B, s.rng
    cmd = _f(rng.uniform(-1, 1, (B, n)), dt)
    mv = np.zeros(B)
    s.lead_joint = np.zeros(B, dtype=int)
    for b in range(B):
        k, g = s.kind_of(b), int(s.round[b])
        jl = _lead_joint(g, n)
        s.lead_joint[b] = jl
        sign = -1.0 if (g // 3) % 2 else 1.0
        cmd[b, jl] = sign * float(dt(1.0 + 0.37 * rng.uniform()))
        lead = abs(cmd[b, jl])
        if k == "tie":
            mv[b] = lead
        elif k == "below":
            mv[b] = _next(lead, False, dt)
        elif k == "above":
            mv[b] = _next(lead, True, dt)
        elif k == "two_tie":
            cmd[b, (jl + 2) % n] = -cmd[b, jl]
            mv[b] = lead if g % 2 else _next(lead, False, dt)
        elif k == "zero":
            cmd[b] = 0.0
            mv[b] = 0.0
        elif k == "inf_max":
            mv[b] = np.inf
        elif k == "nan":
            if g % 2 == 0:   # behind joint 0, on a limited arm
                jn = (jl + 1) % n or 1
                cmd[b, jn] = np.nan
                mv[b] = _next(lead, False, dt)
            else:            # on joint 0, no other joint above max_vel
                cmd[b, 0] = np.nan
                mv[b] = _next(float(np.nanmax(np.abs(cmd[b]))), True, dt)
        elif k == "inf":
            cmd[b, jl] = sign * np.inf
            mv[b] = np.inf if g % 2 else 0.5
        elif k == "regular":
            mv[b] = float(dt(0.3 + 0.001 * b))
        else:
            mv[b] = 2.0
    s.ext = np.zeros((4, B, n))
    s.ext[1] = cmd
    s.cmd = cmd
    s.mixw = np.tile(np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0]), (B, 1))
    s.max_vel = mv
    s.limiter = True
    return s


def joint_scene(robot, dt, per_cycle, seed=43):
    """Joint controller: jp_delta = 2^-4 and jp_kp = 2; err == delta exactly and one ulp to either side, a large negative error, ref on a limit,
    one ulp beyond and inside it, ref = +-inf, NaN in ref[0] (no controller: channel 2 is the external command) and in a later element.
    `per_cycle`: the limits go in as this cycle's q_lo / q_hi (values of the I/O type, every other round at 0.95 of the chain's), so a reference
    can sit ON a limit at float32 too; against the chain's own limits (doubles) that condition holds at float64 only (f64_only)."""
    s = Scene("joint_cycle" if per_cycle else "joint", robot, dt, JP_KINDS, seed)
    n, B, rng, chain = s.n, s.B, s.rng, s.chain
    q = s.q
    if per_cycle:
        scale = np.where(s.round % 2 == 1, 0.95, 1.0)[:, None]
        s.q_lo, s.q_hi = _f(scale * chain.q_lo[None, :], dt), _f(scale * chain.q_hi[None, :], dt)
    ref = _f(q + rng.uniform(-0.03, 0.03, (B, n)), dt)
    s.joint = np.zeros(B, dtype=int)
    s.sub = [""] * B
    for b in range(B):
        k, g = s.kind_of(b), int(s.round[b])
        j = _lead_joint(g, n)
        s.joint[b] = j
        lo, hi = s.limits(b)[j]
        if k in ("err_tie", "err_below", "err_above"):
            q[b, j] = 0.5 + int(rng.integers(0, 256)) * 2.0 ** -10   # (10 bits: q and q + delta are values of both I/O types)
            t = q[b, j] + JP_DELTA
            ref[b, j] = t if k == "err_tie" else _next(t, k == "err_above", dt)
        elif k == "neg_large":
            ref[b] = _f(q[b] - 1.0, dt)
        elif k in ("hi_tie", "hi_beyond", "hi_inside"):
            ref[b, j] = float(dt(hi)) if k == "hi_tie" else _beyond(hi, k == "hi_beyond", dt)
            s.f64_only[b] = k == "hi_tie" and float(dt(hi)) != hi
        elif k == "lo_edge":
            s.sub[b] = LO_SUB[g % 3]
            ref[b, j] = float(dt(lo)) if s.sub[b] == "tie" else _beyond(lo, s.sub[b] == "inside", dt)
            s.f64_only[b] = s.sub[b] == "tie" and float(dt(lo)) != lo
        elif k == "inf_ref":
            ref[b, j] = np.inf if g % 2 else -np.inf
        elif k == "nan_first":
            ref[b, 0] = np.nan
        elif k == "nan_later":
            ref[b, j or 1] = np.nan
        else:
            ref[b] = _f(rng.uniform(1.3 * chain.q_lo, 1.3 * chain.q_hi), dt)
    s.q = s.w["q"] = _f(q, dt)
    s.q_ref = ref
    s.ext = np.zeros((4, B, n))
    s.ext[0] = _f(rng.uniform(-1, 1, (B, n)), dt)   # what channel 2 carries for an arm without a controller
    s.mixw = np.tile(np.array([0.0, 0.0, 1.0, 0.0, 0.0, 0.0]), (B, 1))
    s.mixw[s.round % 2 == 1, 2] = 0.5
    return s


def form_scene(robot, dt, seed=47):
    """Command form: q_cmded is given; arms whose weights are all zero -- a -0.0 among them too -- are direct, arms with one denormal weight are
    not.  The command sits on channels 3 (and 5), the limiter is on."""
    s = Scene("form", robot, dt, FORM_KINDS, seed)
    n, B, rng = s.n, s.B, s.rng
    s.ext = np.zeros((4, B, n))
    s.ext[1] = _f(rng.uniform(-1, 1, (B, n)), dt)
    s.ext[3] = _f(rng.uniform(-1, 1, (B, n)), dt)
    s.q_cmded = _f(s.q + rng.normal(0, 0.01, (B, n)), dt)
    s.mixw = np.zeros((B, 6))
    s.max_vel = np.full(B, 0.5)
    tiny = _tiny(dt)
    for b in range(B):
        k, g = s.kind_of(b), int(s.round[b])
        if k == "regular":
            s.mixw[b, 3] = 1.0
        elif k == "minus_zero":
            s.mixw[b, g % 6] = -0.0
        elif k == "denormal":
            s.mixw[b, 3 + g % 3] = tiny
        elif k == "free":
            s.mixw[b, 3] = 1.0
            s.max_vel[b] = 2.0
        elif k == "two_channels":
            s.mixw[b, 3], s.mixw[b, 5] = 0.5, 0.25
            s.max_vel[b] = 0.25
        elif k == "denormal_vf":   # (qdot_vf times the smallest denormal is absorbed by -q_cmded + q, whose entries are not zero)
            s.mixw[b, 0] = tiny
        elif k == "standstill":
            s.mixw[b, 3] = 1.0
            s.ext[1][b] = 0.0
            s.q_cmded[b] = s.q[b]
        if k in ("regular", "two_channels"):
            # A limited arm's lead joint comes out as max_vel (1 +- a few u), and max_vel is a value of the I/O type: -q_cmded + q + that
            # lands on a float32 rounding boundary for every fourth echo or so, whatever the arithmetic.  The lead joint's echo is q itself,
            # so that the sum rounds to max_vel from either side.
            s.ext[1][b, _lead_joint(g, n)] = float(dt(-0.9 if (g // 3) % 2 else 0.9))
            jm = int(np.argmax(np.abs(mix([[0.0] * n, [0.0] * n, [0.0] * n] + [s.ext[ch][b].tolist() for ch in (1, 2, 3)], s.mixw[b].tolist()))))
            s.q_cmded[b, jm] = s.q[b, jm]
    s.limiter = True
    return s


def mixed_scene(robot, dt=np.float64, seed=53):
    """Limiter, mixed input: the batch-wide weights MIXED_W over qdot_vf, qdot_null, the joint controller and three external channels; the ties
    come from the first pass's own qdot_out (tie_speeds).  /control is zero where the null space has more than one dimension."""
    s = Scene("mixed", robot, dt, ("tie", "below", "above"), seed)
    n, B, rng, chain = s.n, s.B, s.rng, s.chain
    ref = _f(rng.uniform(1.3 * chain.q_lo, 1.3 * chain.q_hi, (B, n)), dt)
    ref[:40] = _f(s.q[:40] + rng.uniform(-0.05, 0.05, (40, n)), dt)
    s.q_ref = ref
    s.ext = _f(rng.uniform(-1, 1, (4, B, n)), dt)
    s.ctrl = _f(rng.uniform(-1, 1, (B, 4)), dt) if n - 6 <= 1 else np.zeros((B, 4))
    return s


def tie_speeds(qdot_out, dt):
    """Limiter, mixed input: per-arm max_vel = the lead of an arm's own mixed command (kind 0), its neighbour below (1) or above (2) in the
    I/O type.  Returns (max_vel, kinds); float64 I/O, where the lead is a value of the I/O type."""
    lead = np.abs(qdot_out).max(axis=1)
    kinds = np.arange(len(lead)) % 3
    mv = np.array([l if k == 0 else _next(l, k == 2, dt) for l, k in zip(lead.tolist(), kinds.tolist())])
    return mv, kinds


# ---- the reference ------------------------------------------------------------------------------------------------------------------
def mix(cmds, w):
    """command_mixer.py:78-82, the loop of vfik_numpy.CommandMixer.read"""
    result = [0.0] * len(cmds[0])
    for v, wk in zip(cmds, w):
        for i in range(len(v)):
            result[i] += v[i] * wk
    return result


def kept_reference(ref, limits):
    """joint_p_controller:89-99 (check_limits), the first lines of vfik_numpy.joint_p_controller: what the controller keeps"""
    ref_out = list(ref)
    for i in range(len(limits)):
        if ref[i] < limits[i][0]:
            ref_out[i] = limits[i][0]
        elif ref[i] > limits[i][1]:
            ref_out[i] = limits[i][1]
    return ref_out


def restate(s, vf=None, null=None, max_vel=None, mix_w=None, limiter=None):
    """The back end of every arm of a scene in CPython doubles.  vf / null: channels 0 and 1 ((B, n) rows as published; zeros where their
    weights are zero).  Returns mixed, qdot_out (B, n), limited, nan, at_goal, direct (B,) and q_ref_out (B, n; the row as given for an arm
    without a controller)."""
    from oracle import vfik_numpy as vn
    B, n = s.B, s.n
    limiter = s.limiter if limiter is None else limiter
    out = dict(mixed=np.zeros((B, n)), qdot_out=np.zeros((B, n)), limited=np.zeros(B, dtype=bool), nan=np.zeros(B, dtype=bool),
               at_goal=np.zeros(B, dtype=bool), direct=np.zeros(B, dtype=bool), q_ref_out=np.zeros((B, n)))
    zero = [0.0] * n
    for b in range(B):
        w = (s.mixw[b] if mix_w is None else np.asarray(mix_w)).tolist()
        ext = [s.ext[ch][b].tolist() if s.ext is not None else zero for ch in range(4)]
        ch2 = ext[0]
        if s.q_ref is not None:
            r = s.q_ref[b].tolist()
            out["q_ref_out"][b] = r
            if not math.isnan(r[0]):
                ch2, reached = vn.joint_p_controller(r, s.q[b].tolist(), s.limits(b), JP_KP, JP_DELTA)
                out["at_goal"][b] = reached
                out["q_ref_out"][b] = kept_reference(r, s.limits(b))
        cmds = [zero if vf is None else vf[b].tolist(), zero if null is None else null[b].tolist(), ch2, ext[1], ext[2], ext[3]]
        v = mix(cmds, w)
        out["mixed"][b] = v
        if limiter:
            v, out["limited"][b] = vn.limiter(v, float((s.max_vel if max_vel is None else max_vel)[b]))
        out["nan"][b] = any(math.isnan(x) for x in v)
        out["direct"][b] = all(x == 0.0 for x in w)
        if s.q_cmded is not None:
            v = vn.lwr_command(v, s.q[b].tolist(), s.q_cmded[b].tolist(), bool(out["direct"][b]))
        out["qdot_out"][b] = v
    return out


def status_bits(r):
    return (ST_LIMITED * r["limited"] + ST_NAN * r["nan"] + ST_JOINT_AT_GOAL * r["at_goal"]).astype(np.int32)


BACK_END_BITS = ST_LIMITED | ST_NAN | ST_JOINT_AT_GOAL


# ---- the comparison -----------------------------------------------------------------------------------------------------------------
def _same(a, b):
    """bit for bit, with -0.0 == 0.0 and NaN where the other has NaN"""
    return (a == b) | (np.isnan(a) & np.isnan(b))


def near_f32_boundary(ref):
    """elements of the reference's doubles within LIMITED_ULP ulp of a float32 rounding boundary"""
    with np.errstate(invalid="ignore", over="ignore"):
        r32 = ref.astype(np.float32)
        lo = np.where(r32.astype(np.float64) <= ref, r32, np.nextafter(r32, np.float32(-np.inf)))
        mid = 0.5 * (lo.astype(np.float64) + np.nextafter(lo, np.float32(np.inf)).astype(np.float64))
        return np.isfinite(ref) & (np.abs(ref - mid) <= LIMITED_ULP * np.spacing(np.abs(ref)))


def compare(got, ref, limited, dt):
    """`got` (B, n) against the reference's doubles by the module's bars.  Returns (bad, worst, allowance): the arms that miss, the worst error
    of a limited row in ulp of the reference's double over LIMITED_ULP (float64 I/O; 0 at float32), and the limited rows that used the float32
    allowance."""
    got = np.asarray(got, dtype=np.float64)
    lim = np.asarray(limited, dtype=bool)[:, None]
    with np.errstate(invalid="ignore", over="ignore"):
        if dt == np.float64:
            ulps = np.where(_same(got, ref), 0.0, np.abs(got - ref) / np.spacing(np.abs(ref)))
            ulps = np.where(np.isnan(ulps), np.inf, ulps)
            ok = np.where(lim, ulps <= LIMITED_ULP, ulps == 0.0)
            worst = float((ulps * lim).max() / LIMITED_ULP) if lim.any() else 0.0
            return np.nonzero(~ok.all(axis=1))[0], worst, 0
        exp = ref.astype(np.float32)
        exact = _same(got, exp.astype(np.float64))
        other = np.where(got > exp, np.nextafter(exp, np.float32(np.inf)), np.nextafter(exp, np.float32(-np.inf))).astype(np.float64)
        allowed = lim & ~exact & (got == other) & near_f32_boundary(ref)
        ok = exact | allowed
        return np.nonzero(~ok.all(axis=1))[0], 0.0, int(allowed.any(axis=1).sum())


# ---- the scenes' own conditions -----------------------------------------------------------------------------------------------------
def eight_kinds(s):
    return all(len(set(s.kind[b:b + 8].tolist())) == 8 for b in range(s.B - 7))


def _is_type(a, dt):
    with np.errstate(invalid="ignore", over="ignore"):
        return bool(np.all(_same(np.asarray(a, dtype=np.float64), _f(a, dt))))


def limiter_conditions(s):
    """What each arm's kind names, asserted on the constructed doubles.  Returns the failures as strings."""
    from oracle import vfik_numpy as vn
    bad = []
    dt = s.dt
    if not (eight_kinds(s) and _is_type(s.cmd, dt) and _is_type(s.max_vel, dt) and _is_type(s.q, dt)):
        bad.append("kinds do not cycle, or an input is no value of the I/O type")
    seen = set()
    for b in range(s.B):
        k, g = s.kind_of(b), int(s.round[b])
        v, mv = s.cmd[b].tolist(), float(s.max_vel[b])
        lead = max(abs(x) for x in v)                      # bridge:190, CPython's max
        fin = [abs(x) for x in v if not math.isnan(x)]
        out, limited = vn.limiter(v, mv)
        jl = int(s.lead_joint[b])
        ok = True
        if k == "tie":
            ok = lead == mv and not limited and abs(v[jl]) == lead and fin.count(lead) == 1
            seen.add((jl, v[jl] < 0))
        elif k == "below":
            ok = mv < lead and _next(mv, True, dt) == lead and limited
        elif k == "above":
            ok = mv > lead and _next(mv, False, dt) == lead and not limited
        elif k == "two_tie":
            ok = fin.count(lead) == 2 and (v.count(lead), v.count(-lead)) == (1, 1) and limited == (g % 2 == 0) and (lead == mv or _next(mv, True, dt) == lead)
        elif k == "zero":
            ok = all(x == 0.0 for x in v) and mv == 0.0 and not limited
        elif k == "inf_max":
            ok = mv == math.inf and not limited and math.isfinite(lead)
        elif k == "nan":
            nn = [i for i, x in enumerate(v) if math.isnan(x)]
            ok = len(nn) == 1 and ((nn[0] != 0 and limited and max(fin) > mv) or (nn[0] == 0 and not limited and max(fin) < mv))
            ok = ok and any(math.isnan(x) for x in out)
        elif k == "inf":
            ok = sum(math.isinf(x) for x in v) == 1 and limited == (g % 2 == 0) and any(math.isnan(x) for x in out) == (g % 2 == 0)
        elif k == "regular":
            ok = limited and lead > 1.5 * mv
        else:
            ok = not limited and 1.2 * lead < mv
        if not ok:
            bad.append("arm %d (%s, round %d) does not meet its condition" % (b, k, g))
    if len({j for j, _ in seen}) != 3 or len({neg for _, neg in seen}) != 2:
        bad.append("the lead is not first, last and in the middle, positive and negative")
    return bad


def joint_conditions(s):
    bad = []
    dt = s.dt
    if not (eight_kinds(s) and _is_type(s.q_ref, dt) and _is_type(s.q, dt) and (s.q_lo is None or (_is_type(s.q_lo, dt) and _is_type(s.q_hi, dt)))):
        bad.append("kinds do not cycle, or an input is no value of the I/O type")
    if not (math.log2(JP_DELTA).is_integer() and math.log2(JP_KP).is_integer()):
        bad.append("jp_delta and jp_kp are no powers of two")
    r = restate(s)
    for b in range(s.B):
        k, j = s.kind_of(b), int(s.joint[b])
        ref, q, lim = s.q_ref[b].tolist(), s.q[b].tolist(), s.limits(b)
        lo, hi = lim[j]
        kept = r["q_ref_out"][b].tolist()
        err = [kept[i] - q[i] for i in range(s.n)]
        others = all(e < JP_DELTA for i, e in enumerate(err) if i != j)
        inside = all(lim[i][0] < ref[i] < lim[i][1] for i in range(s.n))
        at = bool(r["at_goal"][b])
        ok = True
        if k == "err_tie":
            ok = ref[j] - q[j] == JP_DELTA and others and inside and not at
        elif k == "err_below":
            ok = ref[j] - q[j] < JP_DELTA and _next(ref[j], True, dt) - q[j] == JP_DELTA and others and inside and at
        elif k == "err_above":
            ok = ref[j] - q[j] > JP_DELTA and _next(ref[j], False, dt) - q[j] == JP_DELTA and others and inside and not at
        elif k == "neg_large":
            ok = all(e <= 0.0 for e in err) and min(err) < -0.5 and at   # (a reference below the limit is clamped: the error stays negative)
        elif k == "hi_tie":
            ok = (ref[j] == hi and kept[j] == hi) if not s.f64_only[b] else (dt == np.float32 and ref[j] == float(dt(hi)) != hi)
        elif k == "hi_beyond":
            ok = ref[j] > hi and kept[j] == hi and not _beyond(hi, True, dt) < ref[j]
        elif k == "hi_inside":
            ok = ref[j] < hi and kept[j] == ref[j] and not _beyond(hi, False, dt) > ref[j]
        elif k == "lo_edge":
            sub = s.sub[b]
            if sub == "tie":
                ok = (ref[j] == lo and kept[j] == lo) if not s.f64_only[b] else (dt == np.float32 and ref[j] == float(dt(lo)) != lo)
            elif sub == "beyond":
                ok = ref[j] < lo and kept[j] == lo
            else:
                ok = ref[j] > lo and kept[j] == ref[j] and not _beyond(lo, True, dt) < ref[j]
        elif k == "inf_ref":
            ok = math.isinf(ref[j]) and kept[j] == (hi if ref[j] > 0 else lo)
        elif k == "nan_first":
            ok = math.isnan(ref[0]) and not at and np.array_equal(r["mixed"][b], s.ext[0][b] * s.mixw[b, 2]) and not r["nan"][b]
        elif k == "nan_later":
            ok = not math.isnan(ref[0]) and sum(math.isnan(x) for x in ref) == 1 and not at and bool(r["nan"][b])
        if not ok:
            bad.append("arm %d (%s %s, joint %d) does not meet its condition" % (b, k, s.sub[b], j))
    if s.dt == np.float64 and s.f64_only.any():
        bad.append("a float64 scene has arms marked float64-only")
    if s.q_lo is not None and s.f64_only.any():
        bad.append("per-cycle limits are values of the I/O type: no arm may be float64-only")
    for k in ("err_below", "neg_large"):
        if not r["at_goal"][[b for b in range(s.B) if s.kind_of(b) == k]].all():
            bad.append("%s arms are not at the goal" % k)
    return bad


def form_conditions(s):
    bad = []
    dt = s.dt
    if not (eight_kinds(s) and _is_type(s.mixw, dt) and _is_type(s.max_vel, dt) and _is_type(s.q_cmded, dt) and _is_type(s.ext, dt)):
        bad.append("kinds do not cycle, or an input is no value of the I/O type")
    r = restate(s)
    for b in range(s.B):
        k = s.kind_of(b)
        w = s.mixw[b]
        d = bool(r["direct"][b])
        ok = True
        if k == "all_zero":
            ok = d and not np.signbit(w).any() and np.all(r["qdot_out"][b] == 0.0)
        elif k == "minus_zero":
            ok = d and np.signbit(w).sum() == 1 and np.all(w == 0.0) and np.all(r["qdot_out"][b] == 0.0)
        elif k in ("denormal", "denormal_vf"):
            nz = w[w != 0.0]
            ok = not d and len(nz) == 1 and 0.0 < nz[0] < float(np.finfo(dt).tiny) and np.all(s.q[b] - s.q_cmded[b] != 0.0)
        elif k == "standstill":
            ok = not d and np.all(r["qdot_out"][b] == 0.0)
        elif k in ("regular", "two_channels"):
            ok = not d and bool(r["limited"][b])
        else:
            ok = not d and not r["limited"][b]
        if not ok:
            bad.append("arm %d (%s) does not meet its condition" % (b, k))
    return bad


CONDITIONS = {"limiter": limiter_conditions, "joint": joint_conditions, "joint_cycle": joint_conditions, "form": form_conditions}


def make_scene(name, robot, dt):
    if name == "limiter":
        return limiter_scene(robot, dt)
    if name == "form":
        return form_scene(robot, dt)
    return joint_scene(robot, dt, per_cycle=name == "joint_cycle")


# ---- the table ----------------------------------------------------------------------------------------------------------------------
TABLE = {}


def note(side, case, family, worst, allowance, limited):
    TABLE[(side, case, family)] = (worst, allowance, limited)


def write_table(path):
    """One line per (side, case, kernel family): the worst error of a limited row over LIMITED_ULP ulp, the rows on the float32 allowance, the limited rows."""
    with open(path, "a") as f:
        for (side, case, family), (worst, allowance, limited) in sorted(TABLE.items()):
            f.write("backend  %-4s %-34s %-12s worst/bar %6.3f  allowance %3d of %3d limited rows\n" % (side, case, family, worst, allowance, limited))
    TABLE.clear()
