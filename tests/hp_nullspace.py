"""A high-precision restatement of the nullspace module: restrict / nullspace / move_in_nullspace, the joint-limit task and check_limits.

A helper of the suite like hp_reference.py, not a conftest.py: it reuses hp_reference's back end (mpmath at 50 digits; numpy.longdouble
where mpmath cannot be imported), its (hi, lo) result pairs and its cached 50-digit kinematics().  tests/test_oracle_nullspace.py holds the
C oracle to it on the CPU, tests/test_gpu_nullspace.py the HIP kernels on the GPU.

The reference (`reference`), per arm, from the arm's 50-digit J, its q and its limits:

  sigma, gap   the six singular values of the rounded high-precision J (numpy.linalg.svd), gap = sigma_6 / sigma_1;
  z            the joint-limit task's descent direction, in doubles exactly as vfo_cycle forms it:
               z_i = -jl_gain (q_i - mid_i) / half_i^2, mid = (lo + hi) / 2, half = (hi - lo) / 2;
  Pz           z - J^T (J J^T)^-1 J z, the solve (LDL^T of J J^T) in the high-precision type, with its relative residual
               |J J^T y - J z| / |J z| (`resid`; 0 where J z = 0);
  v            n = 7 only: the unit null vector from the seven signed 6 x 6 minors of J (v_i = (-1)^i det(J without column i): J v = 0 by
               Laplace expansion), with the oracle's raw sign -- the first component with |v_i| > 1e-9 is negative -- and its residual
               |J v| / sigma_1 (`vres`).

`cycle` composes one control cycle from it: the published vector after sign continuity against the previous cycle's REFERENCE vector
(scripts/nullspace:101-105: the sign for which v . v_prev >= 0; no previous vector or a dot product of exactly zero keeps the sign
memory), qn = c0 v + Pz, the stop decision (some q_i + lookahead qn_i outside the limits) and qdot_null = 0 or null_gain qn.

Chains of 8 and more joints follow the rule that include/vfik_types.h states (VFIK_PROJ_ROW_MIN; the kernels' projector goes through
J J^T, which cannot serve sigma_6 / sigma_1 below about 1e-6, so J's weak directions are dropped by one stated threshold): the rows of J in
their order, row j kept when its pivot of the LDL^T of J J^T -- the squared length of its part orthogonal to the rows kept before it -- is
above 1e-6 of the largest squared row length; Pz = z - Jk^T (Jk Jk^T)^-1 Jk z over the kept rows Jk.  There `gap` is
sigma_min / sigma_max of Jk (what the bar's conditioning is about) and `kept` (B, 6) names the rows.

Three masks, computed from the reference alone:

  zone        up to 7 joints: gap < ZONE_GAP = 1e-10.  The kernels keep a row of J whose residual is above 1e-12 of its norm, which is
              guaranteed when sigma_6 / sigma_1 >= 1e-12; the factor of 100 is the margin.  8 and more joints: some pivot within a
              factor RULE_MARGIN = 4 of the rule's threshold (the kernels' pivots are good to 1e-10 of it; the 4 is margin), and
              nothing else: an exactly singular pose is decided by the rule like any other.  (An arm whose solve the longdouble fall-back cannot bring under
              hp_reference.RESIDUAL_BAR, or whose minors all vanish, counts as zone too.)  In the zone the rank decision is the
              implementation's own and `check_zone` asks only: every output finite, |qdot_null| <= null_gain (|c0| + sqrt(n) max|z|)
              (1 + 1e-6) -- a projector does not lengthen --, status bits a subset of those the case can raise.
  sign_amb    some |v_i| in (1e-10, 1e-8) (the raw sign rule's 1e-9), or |v . v_prev| < 1e-6 (the kernels keep the previous vector as
              float32 between launches; tests/test_gpu_sign_boundary.py): compared up to sign.
  stop_amb    some joint's q_i + lookahead qn_i within STOP_BAND (1e-6 at float64 I/O, 1e-4 at float32) of a limit: asserted is only
              "qdot_null is the reference's value or zero, with LIMIT_STOP set exactly when it is zero".

Caps (`assert_caps`), asserted on the reference before any measured number is looked at: zone <= 1/3 of the arms of a case, no arm of kind 4
or kind 5 in the zone, each ambiguous set <= 5 %.

Bars (`bar`), per arm: max(S, K u (sigma_1 / sigma_6) scale): S = hp_reference.S_BAR, u = 2^-53, scale = 1 for v, max|z| for Pz and
|c0| + max|z| for their sum (the error of a sum is at most the sum of the errors); sigma_1 / sigma_6 is the sensitivity of J's row space
(hence of the projector and of the null vector) to a relative perturbation of J, which is what a backward stable method is allowed."""
import math

import numpy as np

import hp_reference as hp

_num = hp._num
ZONE_GAP = 1e-10
PROJ_ROW_MIN = 1e-6      # VFIK_PROJ_ROW_MIN of include/vfik_types.h (tests/test_oracle_nullspace.py checks that the two agree)
RULE_MARGIN = 4.0
STOP_BAND = {np.float32: 1e-4, np.float64: 1e-6}
RAW_SIGN = 1e-9
ST_NAN, ST_LIMIT_STOP, ST_NULL_AMBIGUOUS = 1, 2, 4
NS_ROBOTS = ("powercube6", "lwr", "lwr_dual14")


def descent(q, lo, hi, jl_gain):
    """z of the joint-limit task in doubles, operation by operation as vfo_cycle writes it"""
    mid, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
    return -jl_gain * (q - mid) / (half * half)


def _project(J, n, z):
    """one arm: (Pz [n], relative residual of the solve, rows kept [6], rule margin); None when a pivot vanishes (J exactly rank
    deficient) on a chain of up to 7 joints.  Chains of 8 and more joints follow the stated rule (PROJ_ROW_MIN): row j is kept when its
    pivot -- the squared length of its part orthogonal to the rows kept before it -- is above PROJ_ROW_MIN of the largest squared row
    length; the margin is the smallest factor between a pivot and that threshold, on either side."""
    zz = [_num(float(x)) for x in z]
    rule = n >= 8
    keep, margin = [True] * 6, math.inf
    A = [[None] * 6 for _ in range(6)]
    for r in range(6):
        for c in range(r + 1):
            s = _num(0)
            for i in range(n):
                s = s + J[r][i] * J[c][i]
            A[r][c] = A[c][r] = s
    rhs = []
    for r in range(6):
        s = _num(0)
        for i in range(n):
            s = s + J[r][i] * zz[i]
        rhs.append(s)
    gmax = max(A[r][r] for r in range(6))
    L = [[_num(0)] * 6 for _ in range(6)]
    d = [_num(0)] * 6
    for j in range(6):
        s = A[j][j]
        for k in range(j):
            s = s - L[j][k] * L[j][k] * d[k]
        if rule:
            thr = _num(PROJ_ROW_MIN) * gmax
            if s > 0 and thr > 0:
                f = float(s / thr)
                margin = min(margin, f if f > 1 else 1 / f)
            if not s > thr:
                keep[j] = False     # (its column of L and its d stay 0: the later pivots are taken against the kept rows alone)
                continue
        elif not s > 0:
            return None
        d[j] = s
        for i in range(j + 1, 6):
            t = A[i][j]
            for k in range(j):
                t = t - L[i][k] * L[j][k] * d[k]
            L[i][j] = t / s
    y = [_num(0)] * 6
    for i in range(6):
        s = rhs[i]
        for k in range(i):
            s = s - L[i][k] * y[k]
        y[i] = s
    for i in range(6):
        y[i] = y[i] / d[i] if keep[i] else _num(0)
    for i in range(5, -1, -1):
        s = y[i]
        for k in range(i + 1, 6):
            s = s - L[k][i] * y[k]
        y[i] = s if keep[i] else _num(0)
    res2 = nrm2 = _num(0)
    for r in range(6):
        if not keep[r]:
            continue
        s = -rhs[r]
        for c in range(6):
            s = s + A[r][c] * y[c]
        res2, nrm2 = res2 + s * s, nrm2 + rhs[r] * rhs[r]
    Pz = []
    for i in range(n):
        s = zz[i]
        for r in range(6):
            s = s - J[r][i] * y[r]
        Pz.append(s)
    return Pz, (math.sqrt(float(res2 / nrm2)) if nrm2 != 0 else 0.0), keep, margin


def _det6(M):
    """determinant of a 6 x 6 list of lists by elimination with partial pivoting (M is overwritten)"""
    det = _num(1)
    for c in range(6):
        p = max(range(c, 6), key=lambda r: abs(M[r][c]))
        if M[p][c] == 0:
            return _num(0)
        if p != c:
            M[p], M[c] = M[c], M[p]
            det = -det
        det = det * M[c][c]
        for r in range(c + 1, 6):
            f = M[r][c] / M[c][c]
            for k in range(c + 1, 6):
                M[r][k] = M[r][k] - f * M[c][k]
    return det


def _null_vector(J, sigma1):
    """n = 7: (unit null vector with the raw sign, |J v| / sigma_1); None when every minor vanishes"""
    v = []
    for i in range(7):
        m = _det6([[J[r][c] for c in range(7) if c != i] for r in range(6)])
        v.append(-m if i % 2 else m)
    n2 = _num(0)
    for x in v:
        n2 = n2 + x * x
    if not n2 > 0:
        return None
    nrm = hp._mpm.sqrt(n2) if hp.BACKEND == "mpmath" else np.sqrt(n2)
    v = [x / nrm for x in v]
    for x in v:
        if abs(float(x)) > RAW_SIGN:
            if x > 0:
                v = [-y for y in v]
            break
    r2 = _num(0)
    for r in range(6):
        s = _num(0)
        for i in range(7):
            s = s + J[r][i] * v[i]
        r2 = r2 + s * s
    return v, math.sqrt(float(r2)) / sigma1


_REF = {}


def reference(key, chain, q, jl_gain, q_lo=None, q_hi=None, lim_key=None):
    """The reference of one pose set (key as hp_reference.kinematics takes it), computed once.  q_lo / q_hi: the chain's unless given.
    Returns a dict, not to be written to: sigma (B, 6), gap, z (B, n), Pz / Pz_lo (B, n), resid (B,), v / v_lo (B, n) and vres (B,) for
    n = 7 (zeros otherwise), zone (B,) bool, lo / hi (B, n); `mp`: the high-precision Pz and v per arm (None where there is none)."""
    ck = (key, float(jl_gain), lim_key)   # lim_key names per-arm limits in the cache
    if ck in _REF:
        return _REF[ck]
    kin = hp.kinematics(key, chain, q)
    B, n = len(kin), chain.n
    lo = np.array(np.broadcast_to(np.asarray(chain.q_lo if q_lo is None else q_lo, dtype=np.float64), (B, n)))
    hi = np.array(np.broadcast_to(np.asarray(chain.q_hi if q_hi is None else q_hi, dtype=np.float64), (B, n)))
    out = dict(sigma=np.zeros((B, 6)), gap=np.zeros(B), z=descent(np.asarray(q, dtype=np.float64), lo, hi, jl_gain),
               Pz=np.zeros((B, n)), Pz_lo=np.zeros((B, n)), resid=np.zeros(B), v=np.zeros((B, n)), v_lo=np.zeros((B, n)),
               vres=np.zeros(B), zone=np.zeros(B, dtype=bool), kept=np.ones((B, 6), dtype=bool), lo=lo, hi=hi)
    mp_pz, mp_v = [None] * B, [None] * B
    for b, (_, J) in enumerate(kin):
        Jd = np.array([[float(x) for x in row] for row in J])
        s = np.linalg.svd(Jd, compute_uv=False)
        out["sigma"][b] = s
        out["gap"][b] = s[5] / s[0]
        zone = out["gap"][b] < ZONE_GAP
        pr = _project(J, n, out["z"][b])
        if n >= 8:   # the stated rule: what is projected off is the span of the kept rows, and the decision is open only at the threshold
            sk = np.linalg.svd(Jd[np.array(pr[2])], compute_uv=False)
            out["gap"][b] = sk[-1] / sk[0]
            out["kept"][b] = pr[2]
            zone = pr[3] < RULE_MARGIN
        if pr is None or not pr[1] < hp.RESIDUAL_BAR:
            zone = True
            out["resid"][b] = np.inf if pr is None else pr[1]
        else:
            mp_pz[b], out["resid"][b] = pr[:2]
            for i in range(n):
                out["Pz"][b, i], out["Pz_lo"][b, i] = hp._hilo(pr[0][i])
        if n == 7:
            nv = _null_vector(J, s[0])
            if nv is None:
                zone = True
                out["vres"][b] = np.inf
            else:
                mp_v[b], out["vres"][b] = nv
                for i in range(n):
                    out["v"][b, i], out["v_lo"][b, i] = hp._hilo(nv[0][i])
        out["zone"][b] = zone
    for a in out.values():
        a.setflags(write=False)
    out["mp"] = (mp_pz, mp_v)
    _REF[ck] = out
    return out


def raw_sign_ambiguous(ref):
    """(B,) some component of the raw null vector within a decade of the sign rule's 1e-9"""
    a = np.abs(ref["v"])
    return ((a > 1e-10) & (a < 1e-8)).any(axis=1)


def cycle(ref, n, c0, jl_task, null_gain, lookahead, io_dtype, q, prev=None, sig=None):
    """One control cycle on the reference.  c0 (B,); prev: the previous cycle's published reference vectors (B, n) or None (cold start);
    sig (B,) the sign memory (+-1) or None.  Returns dict: vpub (B, n) the published unit vector as doubles (zeros where there is none), sig,
    qn / qn_lo (B, n) before check_limits and the gain, stop, qdot_null / qdot_null_lo (B, n), sign_amb, stop_amb (B,) bool,
    margin (B,) the smallest distance of q + lookahead qn to a limit."""
    B = len(ref["gap"])
    mp_pz, mp_v = ref["mp"]
    c0 = np.broadcast_to(np.asarray(c0, dtype=np.float64), (B,))
    sig = np.ones(B) if sig is None else np.array(sig, dtype=np.float64)
    out = dict(vpub=np.zeros((B, n)), sig=sig, qn=np.zeros((B, n)), qn_lo=np.zeros((B, n)), stop=np.zeros(B, dtype=bool),
               qdot_null=np.zeros((B, n)), qdot_null_lo=np.zeros((B, n)), sign_amb=np.zeros(B, dtype=bool),
               stop_amb=np.zeros(B, dtype=bool), margin=np.full(B, np.inf))
    if n == 7:
        out["sign_amb"] |= raw_sign_ambiguous(ref)
    g, look = _num(float(null_gain)), float(lookahead)
    for b in range(B):
        if ref["zone"][b]:
            continue
        s = 1.0
        if n == 7:
            if prev is not None and np.any(prev[b] != 0.0):
                dot = float(ref["v"][b] @ prev[b])
                if abs(dot) < 1e-6:
                    out["sign_amb"][b] = True
                if sig[b] * dot < 0:
                    sig[b] = -sig[b]
            s = sig[b]
            out["vpub"][b] = s * ref["v"][b]
        qn = []
        for i in range(n):
            t = _num(0)
            if n == 7:
                t = t + _num(float(c0[b] * s)) * mp_v[b][i]
            if jl_task:
                t = t + mp_pz[b][i]
            qn.append(t)
            out["qn"][b, i], out["qn_lo"][b, i] = hp._hilo(t)
        d = q[b] + look * out["qn"][b]
        out["stop"][b] = np.any(d < ref["lo"][b]) or np.any(d > ref["hi"][b])
        out["margin"][b] = min(np.abs(d - ref["lo"][b]).min(), np.abs(d - ref["hi"][b]).min())
        out["stop_amb"][b] = out["margin"][b] < STOP_BAND[io_dtype]
        if not out["stop"][b]:
            for i in range(n):
                out["qdot_null"][b, i], out["qdot_null_lo"][b, i] = hp._hilo(g * qn[i])
    return out


def assert_caps(ref, cyc, kinds, what):
    B = len(kinds)
    zone = ref["zone"]
    assert zone.sum() * 3 <= B, "%s: %d of %d arms in the zone" % (what, zone.sum(), B)
    assert not np.any(zone & (kinds >= 4)), "%s: an arm of kind 4 or 5 in the zone" % what
    for name in ("sign_amb", "stop_amb"):
        m = cyc[name] & ~zone
        assert m.sum() * 20 <= B, "%s: %d of %d arms %s" % (what, m.sum(), B, name)


def bar(ref, io_dtype, K, scale):
    """(B,) max(S, K u (sigma_1 / sigma_6) scale); scale a number or (B,)"""
    with np.errstate(divide="ignore"):
        return np.maximum(hp.S_BAR[io_dtype], K * hp.U / ref["gap"] * scale)


def error(got, cyc, name):
    return np.abs((np.asarray(got, dtype=np.float64) - cyc[name]) - cyc[name + "_lo"])


def check_zone(got_null, status, ref, c0, jl_task, null_gain, allowed, what, failures, others=()):
    """The zone's three conditions on the arms of ref['zone']."""
    m = ref["zone"]
    if not m.any():
        return
    n = got_null.shape[1]
    g = np.asarray(got_null, dtype=np.float64)[m]
    for o in (g,) + tuple(np.asarray(x, dtype=np.float64)[m] for x in others):
        if not np.all(np.isfinite(o)):
            failures.append("%s: zone: values that are not finite" % what)
            return
    zmax = np.abs(ref["z"][m]).max(axis=1) if jl_task else 0.0
    c = np.abs(np.broadcast_to(np.asarray(c0, dtype=np.float64), m.shape)[m]) if n <= 7 else 0.0
    bound = abs(null_gain) * (c + math.sqrt(n) * zmax) * (1 + 1e-6)
    nrm = np.linalg.norm(g, axis=1)
    if np.any(nrm > bound):
        failures.append("%s: zone: |qdot_null| = %.3e above %.3e" % (what, nrm[np.argmax(nrm - bound)], np.broadcast_to(bound, nrm.shape)[np.argmax(nrm - bound)]))
    if np.any(np.asarray(status)[m] & ~allowed):
        failures.append("%s: zone: status bits outside %d" % (what, allowed))


def check_null(got_null, status, ref, cyc, io_dtype, K, scale, null_gain, expect_status, what, kinds, eps, failures, row=None):
    """qdot_null and status of the arms outside the zone against one reference cycle; returns the worst err / (u sigma_1 / sigma_6 scale
    null_gain) with float32's half ulp of the store taken off first.  Sign-ambiguous arms are compared up to sign; a stop-ambiguous arm is
    the reference's value (stopped or not) with LIMIT_STOP set exactly when it is zero."""
    got = np.asarray(got_null, dtype=np.float64)
    status = np.asarray(status)
    held = ~ref["zone"]
    B, n = got.shape
    scale = np.broadcast_to(np.asarray(scale, dtype=np.float64), (B,))
    b0 = bar(ref, io_dtype, K, scale) * abs(null_gain)
    # the value the arm would publish if it did not stop (a stop-ambiguous arm may take either decision)
    free = np.zeros((B, n))
    free_lo = np.zeros((B, n))
    g = float(null_gain)
    free[:], free_lo[:] = g * cyc["qn"], g * cyc["qn_lo"]   # (null_gain = 0.5 by default: exact; otherwise within the bar's S)
    err_free = np.abs((got - free) - free_lo)
    err_flip = np.abs((got + free) + free_lo)
    store = 2.0 ** -24 * np.abs(free) if io_dtype == np.float32 else np.zeros((B, n))
    barn = b0[:, None] + store
    stopped_g = (status & ST_LIMIT_STOP) != 0
    worst, wb = 0.0, -1
    bad = []
    for b in np.nonzero(held)[0]:
        if not np.all(np.isfinite(got[b])):
            bad.append("arm %d not finite" % b)
            continue
        if (status[b] & ~ST_LIMIT_STOP) != expect_status:
            bad.append("arm %d (kind %d eps %g): status %d, expected %d (+ stop)" % (b, kinds[b], eps[b], status[b], expect_status))
            continue
        want_stop = cyc["stop"][b]
        if cyc["stop_amb"][b]:
            want_stop = stopped_g[b]
        elif stopped_g[b] != want_stop:
            bad.append("arm %d (kind %d eps %g): LIMIT_STOP %d, reference %d at margin %.2e" % (b, kinds[b], eps[b], stopped_g[b], want_stop, cyc["margin"][b]))
            continue
        if want_stop:
            if np.any(got[b] != 0.0):
                bad.append("arm %d: stopped, but qdot_null is not zero" % b)
            continue
        e = err_free[b]
        if cyc["sign_amb"][b] and err_flip[b].max() < e.max():
            e = err_flip[b]
        r = (np.maximum(e - store[b], 0.0)).max() / (hp.U / ref["gap"][b] * scale[b] * abs(g)) if scale[b] > 0 else 0.0
        if r > worst:
            worst, wb = r, b
        if not np.all(e <= barn[b]):
            bad.append("arm %d (kind %d eps %g gap %.2e): err %.3e / bar %.3e = %.2f" % (b, kinds[b], eps[b], ref["gap"][b], e.max(), b0[b], (e / barn[b]).max()))
    print("    %-30s ratio %9.3f (arm %3d kind %s eps %-5s gap %s)  held %d, zone %d, sign-ambiguous %d, stop-ambiguous %d, stops %d"
          % (what, worst, wb, kinds[wb] if wb >= 0 else "-", eps[wb] if wb >= 0 else "-", "%.2e" % ref["gap"][wb] if wb >= 0 else "-",
             held.sum(), (~held).sum(), (cyc["sign_amb"] & held).sum(), (cyc["stop_amb"] & held).sum(), (cyc["stop"] & held).sum()))
    if row is not None:
        row.append((what, worst, int(kinds[wb]) if wb >= 0 else -1, float(eps[wb]) if wb >= 0 else 0.0))
    if bad:
        failures.append("%s: %d arms:\n      " % (what, len(bad)) + "\n      ".join(bad[:12]))
    return worst


# ---- the cases -----------------------------------------------------------------------------------------------------------------------
NODE_GAP = 1e-6
ELBOW_ARM, ELBOW_EPS = 7, 3e-8
NEAR_LIMIT = 0.02
PSETS = ("v", "Pz", "both")      # c0 = +-1 without the joint-limit task; c0 = 0 with it; both
MIX_W = (1.0, 0.7)
POSES = "mixed-ns"


def _gap_of(chain, q):
    J = hp._fk_jac(chain, q)[1]
    s = np.linalg.svd(np.array([[float(x) for x in row] for row in J]), compute_uv=False)
    return s[5] / s[0]


def make_case(robot, io_dtype):
    """hp_reference.make_case's mixed poses, with the kind-4 arms (nodes and midpoints of the sin / cos table) that sit ON a singularity
    -- a joint at node 0, or at +-pi/2 -- moved along the table: joint 0, 1, ... in turn goes one node (pi/32) towards the middle of its
    range until sigma_6 / sigma_1 >= NODE_GAP.  Kinds 0-3 are the singular poses; kind 4 is about the table, and the caps keep it out of
    the zone."""
    chain, w, kinds, eps = hp.make_case(robot, io_dtype)
    q, n = w["q"], chain.n
    mid = 0.5 * (chain.q_lo + chain.q_hi)
    # One arm between the kernels' rank threshold and a looser one: the stretched elbow at ELBOW_EPS rad has sigma_6 / sigma_1 = 4e-10
    # (4 times the zone's edge) and a row whose squared residual is 3e-14 of its squared length.  hp_reference's ladder has nothing
    # between 1e-9 rad (in the zone) and 1e-6 rad (residual 2e-12 and more).  One arm only: at such a pose components of the null
    # vector are of the size of the sign rule's 1e-9, so each such arm joins the sign-ambiguous set, whose cap stays.
    if n == 7:
        assert kinds[ELBOW_ARM] == 1 and eps[ELBOW_ARM] == 1e-9
        eps = eps.copy()
        eps[ELBOW_ARM] = ELBOW_EPS
        q[ELBOW_ARM, 3] = np.asarray(math.copysign(ELBOW_EPS, q[ELBOW_ARM, 3])).astype(io_dtype).astype(np.float64)
    # Regular arms put next to a limit of the chain, where c0 v decides whether the lookahead leaves the range: every other kind-5 arm,
    # joints in turn, at NEAR_LIMIT rad from its upper or lower limit in turn
    for i, b in enumerate(np.nonzero(kinds == 5)[0][::2]):
        j = i % n
        q[b, j] = np.asarray((chain.q_hi[j] - NEAR_LIMIT) if i % 2 else (chain.q_lo[j] + NEAR_LIMIT)).astype(io_dtype).astype(np.float64)
    for b in np.nonzero(kinds == 4)[0]:
        t = 0
        while _gap_of(chain, q[b]) < NODE_GAP:
            j = t % n
            q[b, j] += math.copysign(math.pi / 32, mid[j] - q[b, j] if q[b, j] != mid[j] else 1.0)
            q[b, j] = np.asarray(q[b, j]).astype(io_dtype).astype(np.float64)
            t += 1
            assert t <= 4 * n, (robot, b)
    w["q"] = q
    return chain, w, kinds, eps


def pset_inputs(pset, B):
    """(null_control (B, 4), joint-limit task) of a parameter set: c0 = +-1 per arm"""
    assert pset in PSETS
    ctrl = np.zeros((B, 4))
    if pset != "Pz":
        ctrl[:, 0] = np.where(np.arange(B) % 5 < 3, 1.0, -1.0)   # period 5 against the kinds' 24: both signs in every group of eight
    return ctrl, pset != "v"


def pset_params(pset, **kw):
    from vfclik_amd import _abi
    flags = _abi.F_NULLSPACE | _abi.F_MIXER | (_abi.F_JOINT_LIMIT_TASK if pset != "v" else 0)
    return _abi.default_params(flags=flags, mix_w=list(MIX_W) + [0.0] * (_abi.MIX_CHANNELS - 2), **kw)


def scale_of(ref, ctrl, jl_task, n):
    """(B,) the bar's scale: |c0| (chains of 7 joints: elsewhere /control is not honoured) + max|z|"""
    s = np.abs(ctrl[:, 0]) if n == 7 else np.zeros(len(ctrl))
    return s + (np.abs(ref["z"]).max(axis=1) if jl_task else 0.0)


def expected_status(n):
    """outside the zone: 6 joints have no nullspace, 7 a unique direction, 8 and more an ambiguous basis"""
    return ST_NULL_AMBIGUOUS if n >= 8 else 0


_ORC = {}


def oracle_case(oc, robot, io_dtype, pset):
    """One case on the C oracle and its reference: dict(chain, params, w, kinds, eps, ctrl, jl, orc, ref, cyc, scale, R) with R the
    oracle's worst ratio err / (u sigma_1 / sigma_6 scale null_gain) over the arms outside the zone."""
    ck = (robot, np.dtype(io_dtype).name, pset)
    if ck in _ORC:
        return _ORC[ck]
    chain, w, kinds, eps = make_case(robot, io_dtype)
    params = pset_params(pset)
    ctrl, jl = pset_inputs(pset, hp.B_ARMS)
    # (8 and more joints: the oracle moves along an SVD basis that cannot be restated -- VFIK_ST_NULL_AMBIGUOUS -- while the kernels
    # ignore /control there (vfik_io.null_control): the oracle gets zeros, the kernels get c0 and must ignore it)
    orc = oc.cycle_batch(chain, params, w["q"], w["fields"], w["nfields"], null_control=ctrl if chain.n <= 7 else 0.0 * ctrl,
                         want=("qdot_vf", "qdot_null", "qdot_out", "v6", "status"))
    ref = reference((robot, np.dtype(io_dtype).name, POSES), chain, w["q"], params.jl_gain)
    cyc = cycle(ref, chain.n, ctrl[:, 0], jl, params.null_gain, params.lookahead, io_dtype, w["q"])
    scale = scale_of(ref, ctrl, jl, chain.n)
    case = dict(chain=chain, params=params, w=w, kinds=kinds, eps=eps, ctrl=ctrl, jl=jl, orc=orc, ref=ref, cyc=cyc, scale=scale)
    held = ~ref["zone"] & ~cyc["stop"] & ~cyc["sign_amb"] & (scale > 0)
    err = error(orc["qdot_null"], cyc, "qdot_null").max(axis=1)
    rat = np.where(held, err / (hp.U / np.maximum(ref["gap"], 1e-300) * np.where(held, scale, 1.0) * abs(params.null_gain)), 0.0)
    case["R"] = float(rat.max())
    case["R_arm"] = int(np.argmax(rat))
    _ORC[ck] = case
    return case


def check_out(got_out, ref, cyc, refvf, vf_bar, null_bar, mix_w, null_gain, io_dtype, what, kinds, eps, failures, row=None):
    """qdot_out = w0 qdot_vf + w1 qdot_null of a lean launch against w0 (hp_reference's solve) + w1 (this reference's cycle), per arm
    outside the zone: bar |w0| vf_bar + |w1| null_bar (+ half an ulp of the stored value at float32 I/O).  A sign-ambiguous arm may
    carry the null part with either sign, a stop-ambiguous arm the null part or zero.  Returns the worst err / bar."""
    got = np.asarray(got_out, dtype=np.float64)
    B, n = got.shape
    w0, w1, g = float(mix_w[0]), float(mix_w[1]), float(null_gain)
    bar_ = abs(w0) * vf_bar + abs(w1) * np.asarray(null_bar)[:, None]
    base = got - w0 * refvf["qdot"] - w0 * refvf["qdot_lo"]        # what is left for the null part
    worst, wb, bad = 0.0, -1, []
    for b in np.nonzero(~ref["zone"])[0]:
        if not np.all(np.isfinite(got[b])):
            bad.append("arm %d not finite" % b)
            continue
        free, free_lo = w1 * g * cyc["qn"][b], w1 * g * cyc["qn_lo"][b]
        cands = []
        if not cyc["stop"][b] or cyc["stop_amb"][b]:
            cands.append((free, free_lo))
            if cyc["sign_amb"][b]:
                cands.append((-free, -free_lo))
        if cyc["stop"][b] or cyc["stop_amb"][b]:
            cands.append((0.0 * free, 0.0 * free))
        best = np.inf
        for c, c_lo in cands:
            e = np.abs((base[b] - c) - c_lo)
            bb = bar_[b] + (2.0 ** -24 * np.abs(w0 * refvf["qdot"][b] + c) if io_dtype == np.float32 else 0.0)
            best = min(best, (e / bb).max())
        if best > worst:
            worst, wb = best, b
        if not best <= 1.0:
            bad.append("arm %d (kind %d eps %g gap %.2e): err / bar %.2f" % (b, kinds[b], eps[b], ref["gap"][b], best))
    print("    %-30s worst err / bar %.3f (arm %d kind %s eps %s)" % (what, worst, wb, kinds[wb] if wb >= 0 else "-", eps[wb] if wb >= 0 else "-"))
    if row is not None:
        row.append((what + " /bar", worst, int(kinds[wb]) if wb >= 0 else -1, float(eps[wb]) if wb >= 0 else 0.0))
    if not np.all(np.isfinite(got[ref["zone"]])):
        bad.append("zone: values that are not finite")
    if bad:
        failures.append("%s: %d arms:\n      " % (what, len(bad)) + "\n      ".join(bad[:12]))
    return worst


# ---- cycle sequence A (7 joints): cold, warm with one projection, warm with two, cold again ---------------------------------------------
SEQ_TURN = 0.05
SEQ_RHO = 0.2
SEQ_STEPS = ("q1 cold", "q2 warm, one projection", "q3 warm, two projections", "q4 cold again")
_SEQ = {}


def _null_double(chain, q):
    """the null vector of a 7-joint arm in plain doubles (pose construction only)"""
    J = np.array([[float(x) for x in row] for row in hp._fk_jac(chain, q)[1]])
    return np.linalg.svd(J)[2][-1]


def sequence_a(io_dtype, robot="lwr"):
    """The four pose sets of the sequence, their references and their chained reference cycles (set `v`: c0 = +-1, no joint-limit task).

    q1 the mixed poses (cold start); q2 = q1 (the stored vector is the new one to float32: one projection); q3 = q2 + a turn along a
    unit direction per arm, SEQ_TURN = 0.05 rad scaled so that rho below comes out near SEQ_RHO (two projections); q4 a regular pose per arm, of twelve draws the
    one that keeps least of the stored vector (a jump).  Per step k and arm, from the REFERENCE vectors
    (v_old = the previous step's published reference vector rounded to float32, as the kernels store it between launches):
      keep   (v_new . v_old)^2, the part of the stored vector that survives the projection -- the kernels stay warm above 1/4;
      rho    sqrt(1 - keep), the length of its row-space part; the largest coefficient removed lies in [rho / sqrt 6, rho] -- the
             kernels project once up to 1e-2 and twice above.
    `built` (4, B): the lane clears its step's branch condition by a factor of 4 -- q2: keep > 13/16 (the lost part 1 - keep below a
    quarter of the 3/4 allowed) and rho <= 1e-2 / 4; q3: keep > 13/16 and rho / sqrt 6 >= 4e-2; q4: keep < 1/16.  An arm whose warm /
    cold decision is not cleared by that margin, or that was in the zone at an earlier step (what the kernels stored there is their own
    business), is held up to sign at that step; one projection against two needs no such care, since either branch must meet the bar."""
    from vfclik_amd import synth
    ck = (np.dtype(io_dtype).name, robot)
    if ck in _SEQ:
        return _SEQ[ck]
    chain, w, kinds, eps = make_case(robot, io_dtype)
    B, n = w["q"].shape
    params = pset_params("v")
    ctrl, _ = pset_inputs("v", B)
    d = np.random.default_rng(53).normal(size=(B, n))
    d /= np.linalg.norm(d, axis=1)[:, None]
    rnd = lambda x: x.astype(io_dtype).astype(np.float64)  # noqa: E731
    q1 = w["q"]
    # the turn per arm: SEQ_TURN scaled (twice, in doubles) so that the row-space part of the old vector comes out near SEQ_RHO
    t = np.full(B, SEQ_TURN)
    v1 = np.array([_null_double(chain, row) for row in q1])
    for _ in range(2):
        q3 = np.clip(q1 + t[:, None] * d, 0.97 * chain.q_lo, 0.97 * chain.q_hi)
        c = np.abs((np.array([_null_double(chain, row) for row in q3]) * v1).sum(axis=1))
        r = np.sqrt(np.maximum(1.0 - c * c, 1e-12))
        t = np.clip(t * SEQ_RHO / r, 0.02, 0.6)
    q3 = rnd(np.clip(q1 + t[:, None] * d, 0.97 * chain.q_lo, 0.97 * chain.q_hi))
    # the jump per arm: of twelve draws of regular poses, the one whose null vector keeps least of q3's (in doubles)
    v3 = np.array([_null_double(chain, row) for row in q3])
    cand = [rnd(synth.make_workload(chain, B, 2, seed=11 + i, io_dtype=io_dtype)["q"]) for i in range(12)]
    kept = np.array([[abs(_null_double(chain, c[b]) @ v3[b]) for b in range(B)] for c in cand])
    q4 = np.array([cand[i][b] for b, i in enumerate(kept.argmin(axis=0))])
    qs = [q1, q1, q3, q4]
    keys = [POSES, POSES, "seq-q3", "seq-q4"]
    refs = [reference((robot, np.dtype(io_dtype).name, k), chain, q, params.jl_gain) for q, k in zip(qs, keys)]
    cycs, built = [], np.zeros((4, B), dtype=bool)
    keep, rho = np.full((4, B), np.nan), np.full((4, B), np.nan)
    prev = sig = None
    dirty = np.zeros(B, dtype=bool)
    for k in range(4):
        cyc = cycle(refs[k], n, ctrl[:, 0], False, params.null_gain, params.lookahead, io_dtype, qs[k], prev=prev, sig=sig)
        if k:
            old = prev.astype(np.float32).astype(np.float64)
            has = np.any(old != 0.0, axis=1) & ~refs[k]["zone"]
            nrm = np.where(has, np.linalg.norm(old, axis=1), 1.0)
            dot = (refs[k]["v"] * old).sum(axis=1) / nrm
            keep[k] = np.where(has, dot * dot, np.nan)
            rho[k] = np.sqrt(np.maximum(1.0 - keep[k], 0.0))
            warm_clear, cold_clear = keep[k] > 13 / 16, keep[k] < 1 / 16
            built[k] = has & ~dirty & {1: warm_clear & (rho[k] <= 1e-2 / 4), 2: warm_clear & (rho[k] / math.sqrt(6) >= 4e-2), 3: cold_clear}[k]
            cyc["sign_amb"] |= ~refs[k]["zone"] & (dirty | ~(warm_clear | cold_clear))
        dirty = dirty | refs[k]["zone"]
        cycs.append(cyc)
        prev, sig = cyc["vpub"], cyc["sig"]
    out = dict(chain=chain, w=w, kinds=kinds, eps=eps, params=params, ctrl=ctrl, qs=qs, refs=refs, cycs=cycs, built=built, keep=keep, rho=rho,
               keys=[(robot, np.dtype(io_dtype).name, k) for k in keys])
    _SEQ[ck] = out
    return out


def sequence_oracle(oc, seq):
    """the C oracle over the sequence (its own double state): [outputs per step], [R per step]"""
    states = oc.new_states(len(seq["ctrl"]), seq["chain"].n)
    outs, Rs = [], []
    g = abs(seq["params"].null_gain)
    for k in range(4):
        o = oc.cycle_batch(seq["chain"], seq["params"], seq["qs"][k], seq["w"]["fields"], seq["w"]["nfields"], null_control=seq["ctrl"],
                           states=states, want=("qdot_null", "status"))
        ref, cyc = seq["refs"][k], seq["cycs"][k]
        held = ~ref["zone"] & ~cyc["stop"] & ~cyc["sign_amb"]
        err = error(o["qdot_null"], cyc, "qdot_null").max(axis=1)
        Rs.append(float(np.where(held, err / (hp.U / np.maximum(ref["gap"], 1e-300) * g), 0.0).max()))
        outs.append(o)
    return outs, Rs



# ---- per-arm limits: narrow ranges that the joint-limit task overshoots, and ranges it stays inside -------------------------------------
LIM_NEAR, LIM_STOP, LIM_STAY = 0.02, 0.3, 1.2


def narrow_limits(chain, q, io_dtype):
    """(q_lo, q_hi) (B, n), rounded to the I/O type: the chain's, but for every arm b with b mod 4 = 1 joint (b // 4) mod n gets the range
    [q - LIM_NEAR, q + w] (mirrored for every other such arm), w = LIM_STOP or LIM_STAY in turn.  The task's descent on that joint is
    g (w - LIM_NEAR) / 2 / ((w + LIM_NEAR) / 2)^2 towards the far limit: 2.7 for w = 0.3, where lookahead 0.3 times it passes the far
    limit unless the projector takes most of it away, and 0.8 for w = 1.2, where it cannot.  Which arms stop is the reference's to say."""
    B, n = q.shape
    lo, hi = np.tile(chain.q_lo, (B, 1)), np.tile(chain.q_hi, (B, 1))
    for b in range(1, B, 4):
        i = b // 4
        j, w = i % n, (LIM_STOP if i % 2 == 0 else LIM_STAY)
        if (i // 2) % 2 == 0:
            lo[b, j], hi[b, j] = q[b, j] - LIM_NEAR, q[b, j] + w
        else:
            lo[b, j], hi[b, j] = q[b, j] - w, q[b, j] + LIM_NEAR
    lo, hi = lo.astype(io_dtype).astype(np.float64), hi.astype(io_dtype).astype(np.float64)
    assert np.all(lo < q) and np.all(q < hi)
    return lo, hi


_LIM = {}


def limits_case(oc, robot, io_dtype):
    """set `both` under narrow_limits: the oracle, the reference and its cycle, as oracle_case returns them (+ q_lo, q_hi)"""
    ck = (robot, np.dtype(io_dtype).name)
    if ck in _LIM:
        return _LIM[ck]
    base = oracle_case(oc, robot, io_dtype, "both")
    chain, params, w, ctrl = base["chain"], base["params"], base["w"], base["ctrl"]
    lo, hi = narrow_limits(chain, w["q"], io_dtype)
    orc = oc.cycle_batch(chain, params, w["q"], w["fields"], w["nfields"], null_control=ctrl if chain.n <= 7 else 0.0 * ctrl,
                         q_lo=lo, q_hi=hi, want=("qdot_vf", "qdot_null", "qdot_out", "v6", "status"))
    ref = reference((robot, np.dtype(io_dtype).name, POSES), chain, w["q"], params.jl_gain, q_lo=lo, q_hi=hi, lim_key="narrow")
    cyc = cycle(ref, chain.n, ctrl[:, 0], True, params.null_gain, params.lookahead, io_dtype, w["q"])
    scale = scale_of(ref, ctrl, True, chain.n)
    case = dict(base, orc=orc, ref=ref, cyc=cyc, scale=scale, q_lo=lo, q_hi=hi)
    held = ~ref["zone"] & ~cyc["stop"] & ~cyc["sign_amb"] & (scale > 0)
    err = error(orc["qdot_null"], cyc, "qdot_null").max(axis=1)
    rat = np.where(held, err / (hp.U / np.maximum(ref["gap"], 1e-300) * np.where(held, scale, 1.0) * abs(params.null_gain)), 0.0)
    case["R"], case["R_arm"] = float(rat.max()), int(np.argmax(rat))
    _LIM[ck] = case
    return case


def assert_stops(ref, cyc, what, least):
    """on the reference: at least `least` arms outside the zone clearly stop, and as many clearly do not"""
    clear = ~ref["zone"] & ~cyc["stop_amb"]
    assert (clear & cyc["stop"]).sum() >= least, "%s: %d arms stop" % (what, (clear & cyc["stop"]).sum())
    assert (clear & ~cyc["stop"]).sum() >= least


# ---- the null vector's own residual ---------------------------------------------------------------------------------------------------
def null_residual(v, key, chain, q, ref):
    """(B,) |J v| / sigma_1 of unit vectors v (B, 7) given as doubles, J the 50-digit Jacobian (rows of zeros in v give 0)"""
    kin = hp.kinematics(key, chain, q)
    out = np.zeros(len(kin))
    for b, (_, J) in enumerate(kin):
        if not np.any(v[b]):
            continue
        vv = [_num(float(x)) for x in v[b]]
        r2 = _num(0)
        for r in range(6):
            t = _num(0)
            for i in range(7):
                t = t + J[r][i] * vv[i]
            r2 = r2 + t * t
        out[b] = math.sqrt(float(r2)) / ref["sigma"][b, 0]
    return out


def check_residual(got_null, status, c0, null_gain, key, chain, q, ref, cyc, io_dtype, K, what, kinds, eps, failures, row=None):
    """Set `v` (qdot_null = null_gain c0 v): |J v| / sigma_1 of the published vector, arms outside the zone that do not stop.
    A vector that is off by delta along J's weakest direction -- all that the bar of qdot_null can see is |delta| <= K u sigma_1 /
    sigma_6 -- has a residual of sigma_6 |delta| / sigma_1 = K u: what a backward stable method leaves is a few u WHATEVER the
    conditioning, while a row-space part left behind by a projection through a basis that is orthonormal only to u sigma_1 / sigma_6
    shows in full.  Bar: K u, plus sqrt(7) 2^-24 at float32 I/O (the stored components).  Returns the worst residual / u."""
    got = np.asarray(got_null, dtype=np.float64)
    m = ~ref["zone"] & ~cyc["stop"] & ~cyc["stop_amb"] & ((np.asarray(status) & ST_LIMIT_STOP) == 0) & np.all(np.isfinite(got), axis=1)
    v = np.where(m[:, None], got / (float(null_gain) * np.asarray(c0, dtype=np.float64))[:, None], 0.0)
    res = null_residual(v, key, chain, q, ref)
    barv = K * hp.U + (math.sqrt(7) * 2.0 ** -24 if io_dtype == np.float32 else 0.0)
    b = int(np.argmax(res))
    print("    %-30s |J v| / sigma_1 = %8.2f u (arm %3d kind %d eps %-5g gap %.2e), bar %.1f u" % (what, res[b] / hp.U, b, kinds[b], eps[b], ref["gap"][b], barv / hp.U))
    if row is not None:
        row.append((what + " /u", res[b] / hp.U, int(kinds[b]), float(eps[b])))
    if res[b] > barv:
        bad = np.nonzero(res > barv)[0]
        failures.append("%s: |J v| / sigma_1 over %.1f u on %d arms, worst %.1f u on arm %d (kind %d eps %g gap %.2e)"
                        % (what, barv / hp.U, len(bad), res[b] / hp.U, b, kinds[b], eps[b], ref["gap"][b]))
    return res[b] / hp.U
