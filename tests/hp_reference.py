"""A high-precision restatement of the kinematics and the damped-least-squares solve, and the poses of the conditioning sweep.

A helper of the suite, not a conftest.py: tests/test_oracle_conditioning.py holds the C oracle to it on the CPU, tests/test_gpu_conditioning.py
and tests/test_gpu_set_params.py hold the HIP kernels to it on the GPU.

The reference.  From a Chain, rows of q, a twist per arm, lambda, wy, wq, in 50-digit arithmetic (mpmath; numpy.longdouble with a 64-bit
mantissa where mpmath cannot be imported):

  * forward kinematics in chain.py's z-normal form, T = B[0] Jz(q_1) B[1] ... Jz(q_n) B[n], the doubles of chain.B and of q taken as exact;
  * the geometric Jacobian about the flange origin in the base frame, rows (v, w) as oracle_c.jacobian orders them;
  * qdot = Wq Jw^T (Jw Jw^T + lambda^2 I)^-1 Wy tw with Jw = Wy J Wq (identity tool: the twist is taken at the flange);
  * with a tool (16 doubles taken as exact, nothing assumed of its 3 x 3 block): the tool pose T_tip = T_flange Tool as a 3 x 4 product
    (vf:321-332), AB = p_flange - p_tip, and the solve -- flange Jacobian, unchanged -- of the twist (v + w x AB, w)
    (Twist.RefPoint, vf:456-459).  `pose` is then the tool pose and `pose_nt` the flange; the error unit of such a case is
    cond u (max |qdot| + max |qdot_shift|), qdot_shift the solve of (w x AB, 0) alone (unit_scale): w x AB can cancel v.  The tools are
    the named table TOOLS / tool() below; tests/test_oracle_tool.py and tests/test_gpu_tool.py hold the oracles and the kernels to it.

The twist is an INPUT (the oracle's v6 for the same, already rounded inputs): what is held here is the kinematics and the solve.  The field
evaluation is NOT well conditioned everywhere (decay orders up to 127, cancelling forces, normCart, the 1e-9 floors) and is held to a
50-digit reference of its own at its decision edges by tests/hp_field.py, tests/test_oracle_field_edges.py and
tests/test_gpu_field_edges.py.  Per arm the helper also returns cond = (s1^2 + lambda^2) / (s6^2 + lambda^2), s the
singular values of Jw (numpy.linalg.svd of the rounded high-precision Jw), and the solve's own relative residual |A y - Wy tw| / |Wy tw|.

Results are returned as pairs of doubles (hi, lo) with hi + lo = the high-precision value to ~32 digits, so that `error` does not add the
half ulp a reference rounded to one double would carry.

The kinematics of a pose set and each solve are cached at module level: the kernel-family runs of one case share one reference, and the
tools of one pose set share one forward kinematics (the tool product and the solve are cached by pose set and tool name).

The poses (make_case).  B = 192 arms = three waves = twenty-four groups of eight; arm b has pattern index p = b mod 24, kind p mod 6 and
offset eps = EPS[p div 6], so that every eight consecutive arms hold every kind:

  kind 0  every odd-indexed joint = +-eps     shoulder, elbow and wrist singular together
  kind 1  joint 3 = +-eps                     elbow stretched
  kind 2  joint n-2 = +-eps                   wrist
  kind 3  every joint = +-eps                 the zero pose
  kind 4  q_i = (k_i + (b mod 2)/2) pi/32, integer k_i in [-20, 20], clipped to 0.95 of the limits:
          the nodes of the sin / cos table and the midpoints between them, where the rounding to a node is a tie
  kind 5  the regular pose of synth.make_workload

(joint indices from 0).  q is rounded to the I/O type before either side sees it.  The `regular` pose set is make_workload's own (kind 5
throughout): lambda = 0, and the chain whose limits of +-64 rad put the angles up to eight turns away."""
import math

import numpy as np

try:
    import mpmath as _mpm
    _mpm.mp.dps = 50
    BACKEND = "mpmath"
    _num, _sin, _cos = _mpm.mpf, _mpm.sin, _mpm.cos
    RESIDUAL_BAR = 1e-30
except ImportError:   # the fall-back: a 64-bit mantissa, u_ref = 2^-64 = u / 2048.  Anything shorter is no reference: fail, do not skip.
    assert np.finfo(np.longdouble).eps < 1.2e-19, "no mpmath, and numpy.longdouble is no wider than double here"
    BACKEND = "longdouble"
    _num, _sin, _cos = np.longdouble, np.sin, np.cos
    RESIDUAL_BAR = 64 * float(np.finfo(np.longdouble).eps)

_HP = type(_num(0))
U = 2.0 ** -53
B_ARMS = 192
EPS = (0.0, 1e-9, 1e-6, 1e-3)
N_KINDS = 6
ROBOTS = ("powercube6", "lwr", "lwr_dual14", "lwr_wide")
LAMBDAS = (0.1, 1e-2, 1e-3)
WY = (1.0, 1.0, 1.0, 0.3, 0.3, 0.1)
WQ_HEAD = (1.0, 0.5, 1.0, 0.7, 1.0, 0.4)
S_BAR = {np.float32: 1e-6, np.float64: 1e-9}   # the suite's bars (tests/test_gpu_parity.py)
K_MARGIN = 8.0


def weights(name, n):
    """(wy, wq): `unit`, or the sweep's weights (wq = 1, 0.5, 1, 0.7, 1, 0.4, 1, 1, ...)."""
    if name == "unit":
        return (1.0,) * 6, (1.0,) * n
    assert name == "weighted"
    return WY, tuple((WQ_HEAD + (1.0,) * n)[:n])


def chain_of(robot):
    from vfclik_amd import chain, robots
    if robot == "lwr_wide":   # the LWR's DH table (the same pattern, hence the same lean kernels) with limits of +-64 rad
        lim = np.full(7, 64.0)
        return chain.Chain.from_dh(robots._LWR_DH, -lim, lim, name="lwr_wide")
    return robots.by_name(robot)


def pattern(B=B_ARMS):
    """(kind, index into EPS) per arm"""
    p = np.arange(B) % (N_KINDS * len(EPS))
    return p % N_KINDS, p // N_KINDS


def make_case(robot, io_dtype, poses="mixed"):
    """(chain, workload, kinds, eps) -- B_ARMS arms of make_workload(seed 3, two obstacles); `mixed`: the joints overwritten by kind."""
    from vfclik_amd import synth
    chain = chain_of(robot)
    n, B = chain.n, B_ARMS
    w = synth.make_workload(chain, B, 2, seed=3, io_dtype=io_dtype)
    if poses == "regular":
        return chain, w, np.full(B, 5), np.zeros(B)
    assert poses == "mixed" and robot != "lwr_wide"
    kinds, ie = pattern(B)
    eps = np.asarray(EPS)[ie]
    rng = np.random.default_rng(31)
    sign = rng.choice([-1.0, 1.0], size=(B, n))
    knode = rng.integers(-20, 21, size=(B, n))
    q = w["q"]
    for b in range(B):
        k = kinds[b]
        if k == 0:
            q[b, 1::2] = eps[b] * sign[b, 1::2]
        elif k == 1:
            q[b, 3] = eps[b] * sign[b, 3]
        elif k == 2:
            q[b, n - 2] = eps[b] * sign[b, n - 2]
        elif k == 3:
            q[b, :] = eps[b] * sign[b, :]
        elif k == 4:
            q[b, :] = np.clip((knode[b] + 0.5 * (b % 2)) * (math.pi / 32), 0.95 * chain.q_lo, 0.95 * chain.q_hi)
    w["q"] = q.astype(io_dtype).astype(np.float64)
    return chain, w, kinds, eps


# ---- the arithmetic ----------------------------------------------------------------------------------------------------------------
def _frame(B12):
    return [[_num(float(B12[r, c])) for c in range(4)] for r in range(3)]


def _mul(X, Y):
    """3x4 frames with the implicit last row (0 0 0 1)"""
    Z = [[None] * 4 for _ in range(3)]
    for i in range(3):
        for j in range(4):
            s = X[i][0] * Y[0][j] + X[i][1] * Y[1][j] + X[i][2] * Y[2][j]
            Z[i][j] = s + X[i][3] if j == 3 else s
    return Z


def _fk_jac(chain, q):
    """one arm: (T 3x4, J 6 x n) in the high-precision type"""
    n = chain.n
    X = _frame(chain.B[0])
    z, o = [], []
    for i in range(n):
        z.append([X[0][2], X[1][2], X[2][2]])
        o.append([X[0][3], X[1][3], X[2][3]])
        qi = _num(float(q[i]))
        if chain.jtype[i] == 0:   # X Jz(q): columns 0 and 1 turn
            c, s = _cos(qi), _sin(qi)
            for r in range(3):
                X[r][0], X[r][1] = X[r][0] * c + X[r][1] * s, X[r][1] * c - X[r][0] * s
        else:                     # a shift along z
            for r in range(3):
                X[r][3] = X[r][3] + X[r][2] * qi
        X = _mul(X, _frame(chain.B[i + 1]))
    pe = [X[0][3], X[1][3], X[2][3]]
    J = [[_num(0)] * n for _ in range(6)]
    for i in range(n):
        if chain.jtype[i] == 0:
            r = [pe[k] - o[i][k] for k in range(3)]
            zi = z[i]
            v = [zi[1] * r[2] - zi[2] * r[1], zi[2] * r[0] - zi[0] * r[2], zi[0] * r[1] - zi[1] * r[0]]
            for k in range(3):
                J[k][i], J[3 + k][i] = v[k], zi[k]
        else:
            for k in range(3):
                J[k][i] = z[i][k]
    return X, J


def _asnum(x):
    """a double taken as exact, or a value already in the high-precision type"""
    return x if isinstance(x, _HP) else _num(float(x))


def _solve(J, n, tw, lam, wy, wq, extra=None):
    """one arm: (qdot [n], relative residual, Jw as doubles); with `extra`, a second twist solved by the same factorisation (one more
    back-substitution), its qdot comes fourth"""
    wy = [_num(float(x)) for x in wy]
    wq = [_num(float(x)) for x in wq]
    Jw = [[wy[r] * J[r][i] * wq[i] for i in range(n)] for r in range(6)]
    lam2 = _num(float(lam)) * _num(float(lam))
    A = [[None] * 6 for _ in range(6)]
    for r in range(6):
        for c in range(r + 1):
            s = _num(0)
            for i in range(n):
                s = s + Jw[r][i] * Jw[c][i]
            A[r][c] = A[c][r] = s + lam2 if r == c else s
    rhs = [wy[r] * _asnum(tw[r]) for r in range(6)]
    # LDL^T (A is symmetric positive definite, or semi-definite with a positive pivot sequence at lambda = 0 off the singularities)
    L = [[_num(0)] * 6 for _ in range(6)]
    d = [None] * 6
    for j in range(6):
        s = A[j][j]
        for k in range(j):
            s = s - L[j][k] * L[j][k] * d[k]
        d[j] = s
        for i in range(j + 1, 6):
            t = A[i][j]
            for k in range(j):
                t = t - L[i][k] * L[j][k] * d[k]
            L[i][j] = t / s

    def back(rhs):
        y = [None] * 6
        for i in range(6):
            s = rhs[i]
            for k in range(i):
                s = s - L[i][k] * y[k]
            y[i] = s
        for i in range(6):
            y[i] = y[i] / d[i]
        for i in range(5, -1, -1):
            s = y[i]
            for k in range(i + 1, 6):
                s = s - L[k][i] * y[k]
            y[i] = s
        return y

    def joints(y):
        qd = []
        for i in range(n):
            s = _num(0)
            for r in range(6):
                s = s + Jw[r][i] * y[r]
            qd.append(wq[i] * s)
        return qd

    y = back(rhs)
    res2 = nrm2 = _num(0)
    for r in range(6):
        s = -rhs[r]
        for c in range(6):
            s = s + A[r][c] * y[c]
        res2, nrm2 = res2 + s * s, nrm2 + rhs[r] * rhs[r]
    qd = joints(y)
    resid = math.sqrt(float(res2 / nrm2)) if nrm2 != 0 else 0.0
    Jwd = [[float(x) for x in row] for row in Jw]
    if extra is None:
        return qd, resid, Jwd
    return qd, resid, Jwd, joints(back([wy[r] * _asnum(extra[r]) for r in range(6)]))


def _hilo(x):
    hi = float(x)
    return hi, float(x - _num(hi))


# ---- cached, batched ---------------------------------------------------------------------------------------------------------------
_KIN, _SOL = {}, {}


def kinematics(key, chain, q):
    """[(T, J) per arm] of the pose set `key` (any hashable: robot, I/O type, pose set), computed once."""
    if key not in _KIN:
        _KIN[key] = (np.array(q, dtype=np.float64), [_fk_jac(chain, row) for row in np.asarray(q, dtype=np.float64)])
    q0, kin = _KIN[key]
    assert np.array_equal(q0, q), "kinematics(%r): another q under the same key" % (key,)
    return kin


def _put(out, name, b, T):
    for r in range(3):
        for c in range(4):
            out[name][b, 4 * r + c], out[name + "_lo"][b, 4 * r + c] = _hilo(T[r][c])


def _arm(out, b, T, J, n, tw, lam, wy, wq, tool16):
    """one arm's row of `out`.  With a tool (16 doubles taken as exact; nothing is assumed of its 3 x 3 block): the tool pose is the 3 x 4
    product of the flange frame and the tool's rows 0..2, AB = p_flange - p_tip, and the solve -- flange Jacobian, unchanged -- takes the
    twist (v + w x AB, w) (Twist.RefPoint, vf:456-459).  qshift: max |qdot| of the solve of (w x AB, 0) alone."""
    if tool16 is None:
        qd, out["resid"][b], Jw = _solve(J, n, tw, lam, wy, wq)
        Tt = T
    else:
        Tt = _mul(T, _frame(np.asarray(tool16, dtype=np.float64).reshape(4, 4)))
        AB = [T[k][3] - Tt[k][3] for k in range(3)]
        v = [_num(float(x)) for x in tw[:3]]
        w = [_num(float(x)) for x in tw[3:6]]
        sh = [w[1] * AB[2] - w[2] * AB[1], w[2] * AB[0] - w[0] * AB[2], w[0] * AB[1] - w[1] * AB[0]]
        zero = _num(0)
        qd, out["resid"][b], Jw, qs = _solve(J, n, [v[0] + sh[0], v[1] + sh[1], v[2] + sh[2]] + w, lam, wy, wq, extra=sh + [zero] * 3)
        out["qshift"][b] = max(abs(float(x)) for x in qs)
    for i in range(n):
        out["qdot"][b, i], out["qdot_lo"][b, i] = _hilo(qd[i])
    _put(out, "pose", b, Tt)
    _put(out, "pose_nt", b, T)
    s = np.linalg.svd(np.array(Jw), compute_uv=False)
    out["cond"][b] = (s[0] ** 2 + lam * lam) / (s[5] ** 2 + lam * lam)


def _empty(B, n):
    out = dict(qdot=np.zeros((B, n)), qdot_lo=np.zeros((B, n)), pose=np.zeros((B, 16)), pose_lo=np.zeros((B, 16)),
               pose_nt=np.zeros((B, 16)), pose_nt_lo=np.zeros((B, 16)), cond=np.zeros(B), resid=np.zeros(B), qshift=np.zeros(B))
    out["pose"][:, 15] = out["pose_nt"][:, 15] = 1.0
    return out


def reference(key, chain, q, tw, lam, wy, wq, wkey, tool=None, tname=None, arms=None):
    """The reference of one case.  key: the pose set's (see kinematics); tw (B, 6); wy (6,) or (B, 6), wq (n,) or (B, n); wkey names
    the weights in the cache.  tool: None (the identity: the twist is taken at the flange), (16,) or (B, 16) doubles taken as exact,
    and tname its name in the cache -- the tools of one pose set share one forward kinematics.  Returns dict(qdot, qdot_lo (B, n),
    pose, pose_lo (the tool pose), pose_nt, pose_nt_lo (the flange) (B, 16), cond, resid, qshift (B,)), not to be written to.
    arms: only these rows are computed (the others stay zero) and nothing is cached -- for an oracle too slow for the whole batch,
    whose twists are its own."""
    assert (tool is None) == (tname is None)
    ck = (key, float(lam), wkey) if tool is None else (key, float(lam), wkey, tname)
    if arms is None and ck in _SOL:
        tw0, tool0, out = _SOL[ck]
        assert np.array_equal(tw0, tw), "reference(%r): another twist under the same key" % (ck,)
        assert tool is None or np.array_equal(tool0, tool), "reference(%r): another tool under the same key" % (ck,)
        return out
    kin = kinematics(key, chain, q)
    B, n = len(kin), chain.n
    wy = np.broadcast_to(np.asarray(wy, dtype=np.float64), (B, 6))
    wq = np.broadcast_to(np.asarray(wq, dtype=np.float64)[..., :n], (B, n))
    tools = None if tool is None else np.broadcast_to(np.asarray(tool, dtype=np.float64), (B, 16))
    out = _empty(B, n)
    for b in (range(B) if arms is None else arms):
        T, J = kin[b]
        _arm(out, b, T, J, n, tw[b], lam, wy[b], wq[b], None if tools is None else tools[b])
    for v in out.values():
        v.setflags(write=False)
    if arms is None:
        _SOL[ck] = (np.array(tw, dtype=np.float64), None if tool is None else np.array(tool, dtype=np.float64), out)
    return out


def unit_scale(ref):
    """per arm: max |qdot| + max |qdot_shift| -- w x AB can cancel v, and the error of either part stays (0 more without a tool)"""
    return np.abs(ref["qdot"]).max(axis=1) + ref["qshift"]


def error(got, ref, name):
    """|got - reference| per element, the reference taken as hi + lo"""
    return np.abs((np.asarray(got, dtype=np.float64) - ref[name]) - ref[name + "_lo"])


def ratio(got_qdot, ref):
    """per arm: max_i |got - reference| / (cond u max_i |qdot|) -- the error in units of what the conditioning allows"""
    err = error(got_qdot, ref, "qdot").max(axis=1)
    scale = ref["cond"] * U * unit_scale(ref)
    return err / scale, err


# ---- the bar of the GPU tests (tests/test_gpu_conditioning.py documents it) -----------------------------------------------------------
def bars(ref, io_dtype, R):
    """(B, n) bar of qdot against the reference of one case; R: the oracle's worst ratio on it"""
    K = K_MARGIN * max(1.0, R)
    arm = np.maximum(S_BAR[io_dtype], K * ref["cond"] * U * unit_scale(ref))
    bar = np.repeat(arm[:, None], ref["qdot"].shape[1], axis=1)
    if io_dtype == np.float32:
        bar = bar + 2.0 ** -24 * np.abs(ref["qdot"])
    return bar


def check_qdot(got, ref, io_dtype, R, what, kinds, eps, failures, row=None):
    """Compares one (B, n) output with the reference; appends to `failures`; returns (worst ratio, its arm).  The ratio is
    err / (cond u |qdot|) with float32's half ulp of the store taken off the error first."""
    got = np.asarray(got, dtype=np.float64)
    err = error(got, ref, "qdot")
    bar = bars(ref, io_dtype, R)
    store = 2.0 ** -24 * np.abs(ref["qdot"]) if io_dtype == np.float32 else 0.0
    rat = (np.maximum(err - store, 0.0)).max(axis=1) / (ref["cond"] * U * unit_scale(ref))
    b = int(np.argmax(rat))
    over = err / bar
    wb = int(np.argmax(over.max(axis=1)))
    print("    %-28s ratio %9.3f (arm %3d kind %d eps %-5g cond %.2e)  worst err / bar %.3f (arm %d kind %d eps %g: err %.3e)"
          % (what, rat[b], b, kinds[b], eps[b], ref["cond"][b], over.max(), wb, kinds[wb], eps[wb], err[wb].max()))
    if row is not None:
        row.append((what, rat[b], kinds[b], eps[b], over.max()))
    if not np.all(np.isfinite(got)):
        failures.append("%s: %d values are not finite" % (what, int((~np.isfinite(got)).sum())))
    elif not np.all(err <= bar):
        failures.append("%s: err / bar = %.2f on arm %d (kind %d, eps %g, cond %.2e): ratio %.1f against K = %.1f"
                        % (what, over.max(), wb, kinds[wb], eps[wb], ref["cond"][wb], rat[wb], K_MARGIN * max(1.0, R)))
    return rat[b], b


def oracle_case(oc, robot, io_dtype, lam, wname, poses):
    """One case on the C oracle and its reference: (chain, params, workload, kinds, eps, oracle outputs, reference, R) with R the oracle's
    worst ratio of the case."""
    from vfclik_amd import _abi
    chain, w, kinds, eps = make_case(robot, io_dtype, poses)
    wy, wq = weights(wname, chain.n)
    params = _abi.default_params(wy=wy, wq=list(wq) + [1.0] * (_abi.MAX_JOINTS - chain.n), **{"lambda": lam})
    orc = oc.cycle_batch(chain, params, w["q"], w["fields"], w["nfields"], want=("qdot_vf", "qdot_out", "pose", "v6", "status"))
    ref = reference((robot, np.dtype(io_dtype).name, poses), chain, w["q"], orc["v6"], lam, wy, wq, wname)
    R = float(ratio(orc["qdot_vf"], ref)[0].max())
    return chain, params, w, kinds, eps, orc, ref, R


# ---- the tools (tests/test_oracle_tool.py, tests/test_gpu_tool.py) ---------------------------------------------------------------------
# Each from one construction, then rounded as stated.  `kind` names the band of the defect max |Rtool Rtool^T - I| (DEFECT_BANDS):
# a later edit cannot quietly make every tool orthonormal again.
TOOLS = ("hand", "turned", "long", "f32", "typed4", "typed3", "rows", "per-arm", "flat")
PER_ARM_OF = ("hand", "turned", "long", "f32", "typed4", "typed3")   # arm b of `per-arm` takes tool b mod 6 of these
DEFECT_BANDS = {"exact": (0.0, 1e-15), "f32": (1e-8, 1e-7), "typed": (1e-5, 1e-3), "singular": (0.0625, 1.5)}   # (singular: beyond VFIK_TOOL_MAX_DEFECT, include/vfik.h)
TOOL_KIND = {"hand": "exact", "turned": "exact", "long": "exact", "f32": "f32", "typed4": "typed", "typed3": "typed", "rows": "typed",
             "flat": "singular"}


def _turned():
    """2.5 rad about (1, 2, 3) / sqrt(14), in doubles (Rodrigues): strongly non-symmetric"""
    a = np.array([1.0, 2.0, 3.0]) / math.sqrt(14.0)
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return math.cos(2.5) * np.eye(3) + math.sin(2.5) * K + (1.0 - math.cos(2.5)) * np.outer(a, a)


def _tool16(R, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T.reshape(16)


def tool(name, io_dtype, B=B_ARMS):
    """(what set_tool gets, per_arm, what the oracle and the reference get) of a tool of the table.

      hand     identity rotation, t = (0, 0, 0.2) (old/README.old:84)
      turned   _turned(), t = (0.02, -0.01, 0.2)
      long     turned's rotation, t = (0.3, -0.4, 1.0): the lever is longer than the arm, the point shift dominates v
      f32      turned, every entry rounded to float32 -- given to BOTH I/O types
      typed4   turned, every entry rounded to 4 decimals;   typed3: to 3 decimals
      rows     typed4 as (B, 16) equal rows, per_arm: the library stores it as the shared tool, rounded to the I/O type (the reference
               gets the rounded values)
      per-arm  arm b takes tool b mod 6 of the above plus a seeded offset in +-0.5 m per axis, rounded to the I/O type
      flat     turned with the last column of its 3 x 3 block zero: a block that has no inverse"""
    R, t = _turned(), np.array([0.02, -0.01, 0.2])
    if name == "hand":
        T = _tool16(np.eye(3), [0.0, 0.0, 0.2])
    elif name == "turned":
        T = _tool16(R, t)
    elif name == "long":
        T = _tool16(R, [0.3, -0.4, 1.0])
    elif name == "f32":
        T = _tool16(R, t).astype(np.float32).astype(np.float64)
    elif name in ("typed4", "typed3", "rows"):
        T = np.round(_tool16(R, t), 3 if name == "typed3" else 4)
    elif name == "flat":
        T = _tool16(R, t)
        T[[2, 6, 10]] = 0.0
    else:
        assert name == "per-arm"
        T = np.stack([tool(PER_ARM_OF[b % 6], io_dtype)[2] for b in range(B)])
        T[:, [3, 7, 11]] += np.random.default_rng(41).uniform(-0.5, 0.5, (B, 3))
        T = T.astype(io_dtype).astype(np.float64)
        return T, True, T
    if name == "rows":
        return np.tile(T, (B, 1)), True, T.astype(io_dtype).astype(np.float64)
    return T, False, T


def defect(T16):
    """max |Rtool Rtool^T - I| of a tool (16,) or of each row of (B, 16)"""
    R = np.asarray(T16, dtype=np.float64).reshape(-1, 4, 4)[:, :3, :3]
    return np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max(axis=(1, 2))


def per_arm_kinds(io_dtype, B=B_ARMS):
    """the band of each row of `per-arm`: an exact row rounded to float32 I/O is an `f32` row"""
    k = [TOOL_KIND[PER_ARM_OF[b % 6]] for b in range(B)]
    return ["f32" if (x == "exact" and io_dtype == np.float32 and PER_ARM_OF[b % 6] != "hand") else x for b, x in enumerate(k)]


def oracle_tool_case(oc, robot, io_dtype, lam, tname, poses="mixed", chain=None):
    """oracle_case with a tool of the table, unit weights: (chain, params, workload, kinds, eps, oracle outputs, reference, R, tool triple).
    chain: a Chain of the caller's (regular poses) under the name `robot`."""
    from vfclik_amd import _abi, synth
    if chain is None:
        chain, w, kinds, eps = make_case(robot, io_dtype, poses)
    else:
        assert poses == "regular"
        w = synth.make_workload(chain, B_ARMS, 2, seed=3, io_dtype=io_dtype)
        kinds, eps = np.full(B_ARMS, 5), np.zeros(B_ARMS)
    wy, wq = weights("unit", chain.n)
    params = _abi.default_params(**{"lambda": lam})
    tl = None if tname is None else tool(tname, io_dtype)
    orc = oc.cycle_batch(chain, params, w["q"], w["fields"], w["nfields"], tool=None if tl is None else tl[2],
                         want=("qdot_vf", "qdot_out", "pose", "pose_nt", "v6", "status"))
    ref = reference((robot, np.dtype(io_dtype).name, poses), chain, w["q"], orc["v6"], lam, wy, wq, "unit",
                    tool=None if tl is None else tl[2], tname=tname)
    R = float(ratio(orc["qdot_vf"], ref)[0].max())
    return chain, params, w, kinds, eps, orc, ref, R, tl


def tool_cases():
    """(robot, lambda, tool) of the tool tests"""
    out = [("lwr", 0.1, t) for t in TOOLS] + [("lwr", 1e-3, t) for t in ("turned", "typed4")]
    for robot in ("powercube6", "lwr_dual14"):
        out += [(robot, 0.1, t) for t in ("turned", "long", "typed4", "per-arm")]
    return out


def cases():
    """(robot, lambda, weights, pose set) of the sweep: the three dampings on the mixed poses, lambda = 0 on the regular poses alone (at a
    singular pose it divides by a zero pivot on both sides), every damping on the wide-limits chain's regular poses."""
    out = []
    for robot in ROBOTS:
        for wname in ("unit", "weighted"):
            for lam in LAMBDAS:
                out.append((robot, lam, wname, "regular" if robot == "lwr_wide" else "mixed"))
            out.append((robot, 0.0, wname, "regular"))
    return out


def case_id(c):
    return "%s-lam%g-%s-%s" % c
