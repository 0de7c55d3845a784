"""The observers at their edges: 50-digit references, the error units derived from those references alone, and the scenes -- the distance
monitor (monitor_kernel; scripts/monitor_distance:76-84,148-167) first, then, each under its own heading further down, the tracking-error
estimator (track_kernel), the cycle kernels' goal distance (io.goal_dist) and the arrival decision of goto's first check.

A helper of the suite, not a conftest.py: tests/test_oracle_observers.py asserts the scenes' own conditions, the caps and that the
double-precision restatement meets the bar on the CPU; tests/test_gpu_observer_edges.py holds the kernels on the GPU.  It reuses
tests/hp_reference.py's back end (mpmath at 50 digits, numpy.longdouble where mpmath cannot be imported) and its K_MARGIN.

The reference (inputs taken as exact doubles), as monitor_kernel words it: D = |p - o|; E = R_cur^T R_obj, a = the axial vector of
(E - E^T) / 2, c = (tr E - 1) / 2, theta = atan2(|a|, c) 180 / pi.  Nothing is assumed of the two 3 x 3 blocks: frames rounded to float32 or
typed with four decimals are no rotations, and the kernel is held to this form for them too (the G R^T form of vfik_numpy.rot_log and of the
cycle kernels' goal distance agrees with it for rotations only).  There is NO floor on the angle: the kernel publishes atan2 as it is, where
vfik_numpy.rot_log returns 0 below |a| = 1e-12.

The units.  Per output, unit = u (sum_i |d out / d x_i| |x_i| + |out|), u = 2^-53: what rounding every input entry once and the result once
moves the output by -- the condition of the output in its own inputs, from the reference alone.  The derivatives are taken by perturbing each
input entry by 2^-40 of itself in the reference's arithmetic.  The bar is K_MARGIN = 8 units; at float32 I/O half an ulp of the stored value is
taken off the error first.  An output whose bar exceeds 1e-3 of its natural scale (1e-3 rad for the angle; 1e-3 max(1 m, D) for the distance)
is finite-only: at most 1/8 of a case's arms may have such an output, and no arm of a regular kind.

The scenes.  B_ARMS = 192 arms, O = 8 objects each.  Arm b has angle kind b mod 14 (any eight consecutive arms hold eight kinds); its object k
sits at the distance DIST[k] along a random direction, turned from the arm's pose by the kind's angle about a random axis (composed in the
reference's arithmetic, then rounded to the I/O type).  Kinds that need an angle or a position finer than the float32 grid are built at
float32 too, but their condition is asserted at float64 only (F64_ONLY, as in tests/hp_field.py).  The `gated` kind is a regular frame for the
stand-alone kernel, which has no gate; the fused test gates exactly these arms off in two of its cycles and asserts that their rows stay."""
import math

import numpy as np

import hp_reference as hp

U, K_MARGIN, B_ARMS, O = hp.U, hp.K_MARGIN, hp.B_ARMS, 8
_num = hp._num
if hp.BACKEND == "mpmath":
    import mpmath as _mpm
    _sqrt, _atan2, _sin, _cos = _mpm.sqrt, _mpm.atan2, _mpm.sin, _mpm.cos
    _PI = +_mpm.pi
else:
    _sqrt, _atan2, _sin, _cos = np.sqrt, np.arctan2, np.sin, np.cos
    _PI = np.arctan2(np.longdouble(0), np.longdouble(-1))
_DEG = _num(180) / _PI

ANGLE_KINDS = ("same", "1e-13", "1e-10", "1e-6", "1e-3", "pi/2", "pi-1e-3", "pi-1e-4(1-1e-3)", "pi-1e-4(1+1e-3)", "pi-1e-6", "half_turn",
               "typed4", "gated", "regular")
THETA = {"same": 0.0, "1e-13": 1e-13, "1e-10": 1e-10, "1e-6": 1e-6, "1e-3": 1e-3, "pi/2": math.pi / 2, "pi-1e-3": math.pi - 1e-3,
         "pi-1e-4(1-1e-3)": math.pi - 1e-4 * (1 - 1e-3), "pi-1e-4(1+1e-3)": math.pi - 1e-4 * (1 + 1e-3), "pi-1e-6": math.pi - 1e-6,
         "half_turn": math.pi}
F64_ONLY = ("1e-13", "1e-10", "1e-6", "pi-1e-4(1-1e-3)", "pi-1e-4(1+1e-3)", "pi-1e-6")
REGULAR = ("typed4", "gated", "regular")
DIST = (0.0, 1e-12, 1e-6, 1.0, 1e3, 0.25, 0.0, 1.0)
DIST_F64_ONLY = (1e-12, 1e-6)
FINITE_ONLY_CAP, ANGLE_SCALE = 1.0 / 8.0, 1e-3


# ---- the reference ------------------------------------------------------------------------------------------------------------------
def _dist(p, o):
    return _sqrt((p[0] - o[0]) ** 2 + (p[1] - o[1]) ** 2 + (p[2] - o[2]) ** 2)


def _angle_deg(P, F):
    """P, F: 3 x 3 blocks as rows of high-precision numbers; E = P^T F"""
    E = [[P[0][i] * F[0][j] + P[1][i] * F[1][j] + P[2][i] * F[2][j] for j in range(3)] for i in range(3)]
    a0, a1, a2 = (E[2][1] - E[1][2]) / 2, (E[0][2] - E[2][0]) / 2, (E[1][0] - E[0][1]) / 2
    c = (E[0][0] + E[1][1] + E[2][2] - 1) / 2
    return _atan2(_sqrt(a0 * a0 + a1 * a1 + a2 * a2), c) * _DEG


def _split(f16):
    A = [_num(float(x)) for x in f16]
    return [A[0:3], A[4:7], A[8:11]], [A[3], A[7], A[11]]


def _sens(fn, args, base):
    """sum_i |d fn / d x_i| |x_i| over every entry of the nested lists `args`, by perturbing each entry by 2^-40 of itself"""
    h = _num(2.0 ** -40)
    tot = _num(0)
    for arr in args:
        for row in (arr if isinstance(arr[0], list) else [arr]):
            for i, x in enumerate(row):
                if x == 0:
                    continue
                row[i] = x + x * h
                tot += abs(fn(*args) - base) / h
                row[i] = x
    return tot


_REF = {}


def reference(key, pose, frames):
    """{D, ang (degrees), unit_D, unit_ang} as (B, O) arrays of the pose (B, 16) and object frames (B, O, 16), doubles taken as exact; D and ang
    come with D_lo / ang_lo (hi + lo = the high-precision value).  Cached by `key`."""
    if key in _REF:
        return _REF[key]
    B, n_obj = frames.shape[:2]
    out = {k: np.zeros((B, n_obj)) for k in ("D", "D_lo", "ang", "ang_lo", "unit_D", "unit_ang")}
    for b in range(B):
        RP, p = _split(pose[b])
        for k in range(n_obj):
            RF, o = _split(frames[b, k])
            D, ang = _dist(p, o), _angle_deg(RP, RF)
            out["D"][b, k], out["D_lo"][b, k] = hp._hilo(D)
            out["ang"][b, k], out["ang_lo"][b, k] = hp._hilo(ang)
            out["unit_D"][b, k] = U * float(_sens(_dist, [p, o], D) + abs(D))
            out["unit_ang"][b, k] = U * float(_sens(_angle_deg, [RP, RF], ang) + abs(ang))
    _REF[key] = out
    return out


def ratios(got, ref, io_dtype):
    """got (B, O, 2) against the reference: (error over bar for D and the angle (B, O) each, finite-only masks).  At float32 I/O half an ulp of
    the stored value is taken off the error first; a finite-only output counts 0 if it is finite, inf if not."""
    got = np.asarray(got, dtype=np.float64)
    res = []
    for i, name in enumerate(("D", "ang")):
        err = np.abs((got[:, :, i] - ref[name]) - ref[name + "_lo"])
        if io_dtype == np.float32:
            err = np.maximum(0.0, err - 0.5 * np.spacing(np.abs(ref[name]).astype(np.float32)).astype(np.float64))
        bar = K_MARGIN * ref["unit_" + name]
        fo = finite_only(ref)[i]
        r = np.where(fo, np.where(np.isfinite(got[:, :, i]), 0.0, np.inf), err / bar)
        res.append(np.where(np.isnan(r), np.inf, r))
    return res[0], res[1]


def finite_only(ref):
    fo_D = K_MARGIN * ref["unit_D"] > 1e-3 * np.maximum(1.0, ref["D"])
    fo_ang = K_MARGIN * ref["unit_ang"] * (math.pi / 180.0) > ANGLE_SCALE
    return fo_D, fo_ang


def monitor_double(pose, frames):
    """The double-precision restatement of the same form, in NumPy doubles with math.atan2: (B, O, 2)"""
    B, n_obj = frames.shape[:2]
    out = np.zeros((B, n_obj, 2))
    for b in range(B):
        A = pose[b].reshape(4, 4)
        for k in range(n_obj):
            G = frames[b, k].reshape(4, 4)
            E = A[:3, :3].T @ G[:3, :3]
            a = 0.5 * np.array([E[2, 1] - E[1, 2], E[0, 2] - E[2, 0], E[1, 0] - E[0, 1]])
            c = 0.5 * (E[0, 0] + E[1, 1] + E[2, 2] - 1.0)
            d = A[:3, 3] - G[:3, 3]
            out[b, k] = math.sqrt(float(d @ d)), math.atan2(math.sqrt(float(a @ a)), c) * (180.0 / math.pi)
    return out


# ---- the scenes ---------------------------------------------------------------------------------------------------------------------
def _rot(axis, th):
    """Rodrigues, in the reference's arithmetic"""
    x, y, z = (_num(float(v)) for v in axis)
    nrm = _sqrt(x * x + y * y + z * z)
    x, y, z = x / nrm, y / nrm, z / nrm
    c, s = _cos(_num(th)), _sin(_num(th))
    v = 1 - c
    return [[c + x * x * v, x * y * v - z * s, x * z * v + y * s], [y * x * v + z * s, c + y * y * v, y * z * v - x * s],
            [z * x * v - y * s, z * y * v + x * s, c + z * z * v]]


def kinds(B=B_ARMS):
    return [ANGLE_KINDS[b % len(ANGLE_KINDS)] for b in range(B)]


_SCENE = {}


def monitor_scene(io_dtype):
    """(pose (B, 16), frames (B, O, 16), kinds) as doubles that are values of the I/O type"""
    if io_dtype in _SCENE:
        return _SCENE[io_dtype]
    from vfclik_amd import robots
    chain = robots.lwr()
    rng = np.random.default_rng(71)
    B = B_ARMS

    def fk(count):
        return chain.fk(rng.uniform(chain.q_lo, chain.q_hi, (count, 7))).reshape(count, 16)

    def rnd(a):
        return np.asarray(a, dtype=np.float64).astype(io_dtype).astype(np.float64)
    pose = rnd(fk(B))
    other = fk(B * O).reshape(B, O, 16)
    frames = np.zeros((B, O, 16))
    frames[:, :, 15] = 1.0
    kk = kinds(B)
    for b in range(B):
        RP, p = _split(pose[b])
        for k in range(O):
            kind = kk[b]
            if kind in REGULAR:
                f = np.round(other[b, k], 4) if kind == "typed4" else other[b, k]
            else:
                f = pose[b].copy()
                if kind == "half_turn":
                    f[[0, 1, 4, 5, 8, 9]] *= -1.0   # R_cur Rz(pi): columns x and y negated
                elif kind != "same":
                    R = _rot(rng.normal(size=3), THETA[kind])
                    M = [[RP[i][0] * R[0][j] + RP[i][1] * R[1][j] + RP[i][2] * R[2][j] for j in range(3)] for i in range(3)]
                    for i in range(3):
                        for j in range(3):
                            f[4 * i + j] = float(M[i][j])
                d = rng.normal(size=3)
                d /= np.linalg.norm(d)
                for i in range(3):
                    f[4 * i + 3] = float(p[i] + _num(DIST[k]) * _num(float(d[i])))
            frames[b, k] = f
    frames = rnd(frames)
    _SCENE[io_dtype] = (pose, frames, kk)
    return _SCENE[io_dtype]


def scene_conditions(io_dtype, kk, ref):
    """Each (arm, object) meets what its kind names, on the reference of the ROUNDED frames.  Returns the failures as strings."""
    bad = []
    f64 = io_dtype == np.float64
    tol_a = 2e-15 if f64 else 1e-6      # rad: what rounding the two blocks to the I/O type can move the angle by
    if not all(len(set(kk[b:b + 8])) == 8 for b in range(len(kk) - 7)):
        bad.append("eight consecutive arms do not hold eight kinds")
    for b, kind in enumerate(kk):
        if kind in REGULAR:
            continue
        for k in range(O):
            ang = ref["ang"][b, k] * math.pi / 180.0
            if f64 or kind not in F64_ONLY:
                if kind == "same" and ang != 0.0:
                    bad.append("arm %d object %d: an identical frame at angle %g" % (b, k, ang))
                if abs(ang - THETA[kind]) > tol_a:
                    bad.append("arm %d object %d (%s): angle off by %.1e rad" % (b, k, kind, ang - THETA[kind]))
            D = ref["D"][b, k]
            if f64 or DIST[k] not in DIST_F64_ONLY:
                if (DIST[k] == 0.0 and D != 0.0) or abs(D - DIST[k]) > (4e-16 if f64 else 2e-7) * max(1.0, DIST[k]):
                    bad.append("arm %d object %d: distance %g for %g" % (b, k, D, DIST[k]))
    return bad


def caps(kk, ref):
    """The caps, on the reference alone: failures as strings"""
    fo_D, fo_ang = finite_only(ref)
    fo = (fo_D | fo_ang).any(axis=1)
    bad = []
    if fo.sum() > FINITE_ONLY_CAP * len(kk):
        bad.append("%d of %d arms are finite-only" % (fo.sum(), len(kk)))
    if any(fo[b] for b, kind in enumerate(kk) if kind in REGULAR):
        bad.append("a regular-kind arm is finite-only")
    return bad


# ---- the table ----------------------------------------------------------------------------------------------------------------------
TABLE = {}


def note(side, case, family, rD, rA, ref):
    fo_D, fo_ang = finite_only(ref)
    TABLE[(side, case, family)] = (float(rD.max()), float(rA.max()), int((fo_D | fo_ang).any(axis=1).sum()))


def write_table(path):
    with open(path, "a") as f:
        for (side, case, family), (rD, rA, fo) in sorted(TABLE.items()):
            f.write("observer %-4s %-34s %-16s worst/bar D %6.3f angle %6.3f  finite-only arms %d\n" % (side, case, family, rD, rA, fo))
    TABLE.clear()


# =====================================================================================================================================
# The tracking-error estimator (track_kernel; vf:349-428 as vfik_numpy.TrackingError words it) over an arm's whole history
# =====================================================================================================================================
# The reference, per call that has six frames behind it: ext = diff(previous frame, this frame) -- vel = p_b - p_a, rot = axis * theta of
# E = R_b R_a^T, theta = atan2(|a|, c), the axis a / |a|, or from the symmetric part next to a half turn (|a| < 1e-4, c < 0), and NO rotation
# below |a| = 1e-12 (has_axis) --, cmd = the command of three calls earlier (the oldest of the buffer of four); outputs acos of the clamped dot
# products of the unit vectors ((1,0,0) where a magnitude is zero), |ext.vel| 150, |ext.rot| 150, |cmd.vel|, |cmd.rot| / 5, |sum - sum| and
# the < 0.10 decision.  A silent call appends nothing.
#
# Units (u = 2^-53; inputs exact).  Magnitudes: u (sum |d out / d x_i| |x_i| + |out|), the norm's derivatives in closed form (v_i / |v|), the
# angle's by perturbing the 18 rotation entries; ext_int_diff adds its four terms' units and the two sums' roundings.  The two acos angles:
# the dot product d of two normalised vectors carries K_DOT = 24 roundings (two subtractions, two norms of 3 squares + 2 additions + root,
# 6 divisions, 3 products + 2 additions, rounded up), delta_d = K_DOT u, times (1 + 1 / sin(theta_ext)) for the rotation angle, whose measured
# axis a / |a| divides an absolute error of a few u by |a| = sin(theta_ext) (as tests/hp_field.py documents for its axis); the angle's unit is
# min(delta_d / sqrt(1 - d^2), sqrt(2 delta_d)) + u |out|.  An EXACT half turn leaves the sign of the axis to rounding noise (a = 0): its
# rotation angle is finite-only.  Natural scales for the finite-only rule: 1 rad for the angles, max(1, |value|) for the magnitudes.
TRACK_KINDS = ("perfect", "anti", "frozen", "zero_cmd", "both_zero", "rot1e-13", "rot1e-11", "rot1e-6", "half_turn", "threshold", "silent",
               "regular")
TRACK_F64_ONLY = ("rot1e-13", "rot1e-11", "rot1e-6", "threshold")
TRACK_REGULAR = ("silent", "regular")
N_CALLS, K_DOT, TRACK_TH, AMBIGUOUS_CAP = 10, 24.0, 0.10, 0.05
TH_DELTA = (1e-9, -1e-9, 1e-6, -1e-6, 1e-3, -1e-3)
SILENT_CALLS = (3, 7)


def _rod(w):
    """Rodrigues in doubles: the rotation by |w| about w"""
    th = float(np.linalg.norm(w))
    if th == 0.0:
        return np.eye(3)
    k = np.asarray(w, dtype=np.float64) / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(th) * K + (1.0 - math.cos(th)) * (K @ K)


_TRACK = {}


def track_scene(io_dtype):
    """(poses (T, B, 16), v6 (T, B, 6), active (T, B) int32, kinds): N_CALLS calls of B_ARMS arms, values of the I/O type"""
    if io_dtype in _TRACK:
        return _TRACK[io_dtype]
    from vfclik_amd import robots
    chain = robots.lwr()
    rng = np.random.default_rng(91)
    B, T = B_ARMS, N_CALLS
    kk = [TRACK_KINDS[b % len(TRACK_KINDS)] for b in range(B)]
    P0 = chain.fk(rng.uniform(chain.q_lo, chain.q_hi, (B, 7))).reshape(B, 4, 4)
    poses, v6, active = np.zeros((T, B, 16)), np.zeros((T, B, 6)), np.ones((T, B), dtype=np.int32)
    for b, kind in enumerate(kk):
        g = b // len(TRACK_KINDS)
        v0, w0, r0, s0 = rng.normal(size=3), rng.normal(size=3), rng.normal(size=3), rng.normal(size=3)
        v0 *= rng.uniform(0.05, 0.2) / np.linalg.norm(v0)
        r0 *= rng.uniform(0.1, 0.5) / np.linalg.norm(r0)
        axis = rng.normal(size=3)
        axis /= np.linalg.norm(axis)
        for t in range(T):   # the commands change from call to call: the delay of three calls matters
            v6[t, b, :3] = v0 + 0.05 * t * np.linalg.norm(v0) * w0
            v6[t, b, 3:] = r0 + 0.05 * t * np.linalg.norm(r0) * s0
        if kind in ("zero_cmd", "both_zero"):
            v6[:, b] = 0.0
        if kind == "threshold":
            v6[:, b] = 0.0
            v6[:, b, 0] = TRACK_TH * (1.0 + TH_DELTA[g % 6])
        if kind == "silent":
            active[list(SILENT_CALLS), b] = 0
        v6[:, b] = v6[:, b].astype(io_dtype).astype(np.float64)
        R, p = P0[b, :3, :3].copy(), P0[b, :3, 3].copy()
        for t in range(T):
            cv, cr = v6[max(t - 3, 0), b, :3], v6[max(t - 3, 0), b, 3:]
            if t > 0 and active[t, b]:
                if kind == "perfect":
                    p, R = p + cv / 150.0, _rod(cr / 150.0) @ R
                elif kind == "anti":
                    p, R = p - cv / 150.0, _rod(-cr / 150.0) @ R
                elif kind in ("rot1e-13", "rot1e-11", "rot1e-6"):
                    p, R = p + 1e-3 * axis[::-1], _rod(float(kind[3:]) * axis) @ R
                elif kind == "half_turn":
                    p = p + 1e-3 * axis
                    R = (R * np.array([-1.0, -1.0, 1.0])) if g % 2 else _rod((math.pi - 1e-5) * axis) @ R
                elif kind in ("zero_cmd", "silent", "regular"):
                    p = p + 0.8 * (v0 + rng.normal(0, 0.01, 3)) / 150.0
                    R = _rod(0.8 * (r0 + rng.normal(0, 0.02, 3)) / 150.0) @ R
            f = np.eye(4)
            f[:3, :3], f[:3, 3] = R, p
            poses[t, b] = f.reshape(16)
            # (the rounded frame is what the next one is built on, so that a frozen or exactly turned arm stays exact)
            f = poses[t, b].astype(io_dtype).astype(np.float64).reshape(4, 4)
            R, p = f[:3, :3].copy(), f[:3, 3].copy()
    poses = poses.astype(io_dtype).astype(np.float64)
    _TRACK[io_dtype] = (poses, v6, active, kk)
    return _TRACK[io_dtype]


def _theta(A, Bm):
    """theta and |a| of E = Bm A^T (rows of high-precision numbers)"""
    E = [[Bm[i][0] * A[j][0] + Bm[i][1] * A[j][1] + Bm[i][2] * A[j][2] for j in range(3)] for i in range(3)]
    a = [(E[2][1] - E[1][2]) / 2, (E[0][2] - E[2][0]) / 2, (E[1][0] - E[0][1]) / 2]
    c = (E[0][0] + E[1][1] + E[2][2] - 1) / 2
    s = _sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2])
    return _atan2(s, c), s, a, c, E


def _theta_only(A, Bm):
    return _theta(A, Bm)[0]


def _acos(d):
    d = min(_num(1), max(_num(-1), d))
    return _atan2(_sqrt((1 - d) * (1 + d)), d)


def _one_track(fa, fb, c6):
    """8 outputs (high precision), their units (floats) and finite-only flags for the frames fa -> fb and the command c6"""
    A, pa = _split(fa)
    Bm, pb = _split(fb)
    cmd = [_num(float(x)) for x in c6]
    ev = [pb[i] - pa[i] for i in range(3)]
    th, s, a, c, E = _theta(A, Bm)
    half = s < _num(1e-4) and c < 0
    has_axis = half or s >= _num(1e-12)
    if half:
        k = max(range(3), key=lambda i: E[i][i])
        ax = [(E[k][j] + E[j][k]) / 2 - (c if j == k else 0) for j in range(3)]
        if ax[0] * a[0] + ax[1] * a[1] + ax[2] * a[2] < 0:
            ax = [-x for x in ax]
        n = _sqrt(ax[0] ** 2 + ax[1] ** 2 + ax[2] ** 2)
        ax = [x / n for x in ax]
    elif has_axis:
        ax = [x / s for x in a]
    evm = _sqrt(ev[0] ** 2 + ev[1] ** 2 + ev[2] ** 2)
    erm = th if has_axis else _num(0)
    cvm = _sqrt(cmd[0] ** 2 + cmd[1] ** 2 + cmd[2] ** 2)
    crm = _sqrt(cmd[3] ** 2 + cmd[4] ** 2 + cmd[5] ** 2)
    one = [_num(1), _num(0), _num(0)]
    eu = [x / evm for x in ev] if evm > 0 else one
    cu = [x / cvm for x in cmd[:3]] if cvm > 0 else one
    er = ax if erm > 0 else one
    cr = [x / crm for x in cmd[3:]] if crm > 0 else one
    dv = sum(x * y for x, y in zip(cu, eu))
    dr = sum(x * y for x, y in zip(cr, er))
    o = [abs(_acos(dv)), abs(_acos(dr)), evm * 150, erm * 150, cvm, crm / 5]
    o.append(abs((o[4] + o[5]) - (o[2] + o[3])))
    o.append(_num(1) if o[6] < _num(TRACK_TH) else _num(0))
    # ---- units
    unit = [0.0] * 8

    def acos_unit(d, dd, out):
        d = float(min(_num(1), max(_num(-1), d)))
        flat = math.sqrt(max(1.0 - d * d, 0.0))
        return min(dd / flat if flat > 0.0 else math.inf, math.sqrt(2.0 * dd)) + U * float(out)
    unit[0] = acos_unit(dv, K_DOT * U, o[0])
    weight = 1.0 + (1.0 / float(s) if (erm > 0 and not half) else 0.0)
    unit[1] = acos_unit(dr, K_DOT * U * weight, o[1])
    mags = [abs(float(pa[i])) + abs(float(pb[i])) for i in range(3)]
    slope = [abs(float(ev[i] / evm)) for i in range(3)] if evm > 0 else [1.0] * 3
    unit[2] = U * (150.0 * sum(sl * m for sl, m in zip(slope, mags)) + float(o[2]))
    unit[3] = U * (150.0 * float(_sens(_theta_only, [A, Bm], th)) + float(o[3]))
    unit[4] = 2.0 * U * float(o[4])
    unit[5] = 3.0 * U * float(o[5])
    unit[6] = unit[2] + unit[3] + unit[4] + unit[5] + U * float(o[4] + o[5] + o[2] + o[3]) + U * float(o[6])
    fo = [K_MARGIN * unit[i] > 1e-3 * (1.0 if i < 2 else max(1.0, float(o[i]))) for i in range(7)] + [False]
    if half and float(s) < 64 * U:
        fo[1] = True   # an exact half turn: the sign of the axis is rounding noise
    return o, unit, fo


def track_reference(key, poses, v6, active):
    """{out, out_lo, unit (T, B, 8), finite_only (T, B, 8), valid (T, B)}: the estimator stepped over every arm's history.  Cached by key."""
    if key in _REF:
        return _REF[key]
    T, B = poses.shape[:2]
    r = dict(out=np.zeros((T, B, 8)), out_lo=np.zeros((T, B, 8)), unit=np.zeros((T, B, 8)), finite_only=np.zeros((T, B, 8), dtype=bool),
             valid=np.zeros((T, B), dtype=bool))
    for b in range(B):
        frames, cmds = [], []
        for t in range(T):
            if not active[t, b]:
                continue
            cmds = (cmds + [v6[t, b]])[-4:]
            frames.append(poses[t, b])
            if len(frames) <= 5:
                continue
            o, unit, fo = _one_track(frames[-2], frames[-1], cmds[0])
            r["valid"][t, b] = True
            for i in range(8):
                r["out"][t, b, i], r["out_lo"][t, b, i] = hp._hilo(o[i])
            r["unit"][t, b], r["finite_only"][t, b] = unit, fo
    _REF[key] = r
    return r


def track_ratios(got, ref, io_dtype, active):
    """got (T, B, 8): (error over bar (T, B, 7) -- 0 where a call has no value yet, which must then be all zeros --, wrong decisions outside the
    ambiguous band (T, B), ambiguous (T, B)).  Calls an arm was silent in are not judged here: its row stays, which the caller asserts."""
    got = np.asarray(got, dtype=np.float64)
    err = np.abs((got[:, :, :7] - ref["out"][:, :, :7]) - ref["out_lo"][:, :, :7])
    if io_dtype == np.float32:
        err = np.maximum(0.0, err - 0.5 * np.spacing(np.abs(ref["out"][:, :, :7]).astype(np.float32)).astype(np.float64))
    bar = K_MARGIN * ref["unit"][:, :, :7]
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(ref["finite_only"][:, :, :7], np.where(np.isfinite(got[:, :, :7]), 0.0, np.inf), np.where(err == 0.0, 0.0, err / bar))
    ratio = np.where(np.isnan(ratio), np.inf, ratio)
    v = ref["valid"]
    ratio = np.where(v[:, :, None], ratio, np.where(got[:, :, :7] == 0.0, 0.0, np.inf))
    ratio = np.where(np.asarray(active, dtype=bool)[:, :, None], ratio, 0.0)
    ambiguous = v & (np.abs(ref["out"][:, :, 6] - TRACK_TH) <= bar[:, :, 6] + (0.5 * np.spacing(np.float32(TRACK_TH)) if io_dtype == np.float32 else 0.0))
    wrong = v & ~ambiguous & (got[:, :, 7] != ref["out"][:, :, 7])
    wrong |= ~v & np.asarray(active, dtype=bool) & (got[:, :, 7] != 0.0)
    return ratio, wrong, ambiguous


def track_caps(kk, ref):
    bad = []
    fo = ref["finite_only"].any(axis=(0, 2))
    if fo.sum() > FINITE_ONLY_CAP * len(kk):
        bad.append("%d of %d arms are finite-only" % (fo.sum(), len(kk)))
    if any(fo[b] for b, k in enumerate(kk) if k in TRACK_REGULAR):
        bad.append("a regular-kind arm is finite-only")
    amb = (ref["valid"] & (np.abs(ref["out"][:, :, 6] - TRACK_TH) <= K_MARGIN * ref["unit"][:, :, 6])).any(axis=0)
    if amb.sum() > AMBIGUOUS_CAP * len(kk):
        bad.append("%d of %d arms are inside the decision's band" % (amb.sum(), len(kk)))
    return bad


def track_conditions(io_dtype, kk, ref, v6):
    """What each kind names, on the reference of the rounded inputs (failures as strings)"""
    bad = []
    f64 = io_dtype == np.float64
    o, v = ref["out"], ref["valid"]
    if not all(len(set(kk[b:b + 8])) == 8 for b in range(len(kk) - 7)):
        bad.append("eight consecutive arms do not hold eight kinds")
    for b, kind in enumerate(kk):
        tt = np.nonzero(v[:, b])[0]
        want_calls = N_CALLS - 5 - (len(SILENT_CALLS) if kind == "silent" else 0)
        ok = len(tt) == want_calls
        x = o[tt, b]
        if kind == "perfect":
            ok = ok and np.all(x[:, 0] < 1e-3) and np.all(x[:, 1] < 1e-3)
        elif kind == "anti":
            ok = ok and np.all(x[:, 0] > math.pi - 1e-3) and np.all(x[:, 1] > math.pi - 1e-3)
        elif kind == "frozen":
            ok = ok and np.all(x[:, 2:4] == 0.0) and np.all(x[:, 4:6] > 0.0)
        elif kind == "zero_cmd":
            ok = ok and np.all(x[:, 4:6] == 0.0) and np.all(x[:, 2:4] > 0.0)
        elif kind == "both_zero":
            ok = ok and np.all(x[:, :7] == 0.0) and np.all(x[:, 7] == 1.0)
        elif kind == "rot1e-13" and f64:
            ok = ok and np.all(x[:, 3] == 0.0)                       # below has_axis: no rotation
        elif kind == "rot1e-11" and f64:
            ok = ok and np.all(np.abs(x[:, 3] / 150.0 - 1e-11) < 1e-15)
        elif kind == "rot1e-6" and f64:
            ok = ok and np.all(np.abs(x[:, 3] / 150.0 - 1e-6) < 1e-15)
        elif kind == "half_turn":
            ok = ok and np.all(np.abs(x[:, 3] / 150.0 - math.pi) < (2e-5 if f64 else 1e-3))
        elif kind == "threshold":
            d = TH_DELTA[(b // len(TRACK_KINDS)) % 6]
            ok = ok and np.all(x[:, 2:4] == 0.0) and np.all(x[:, 6] == v6[0, b, 0])
            if f64:
                ok = ok and np.all(np.abs(x[:, 6] / TRACK_TH - 1.0 - d) < 1e-12) and np.all(x[:, 7] == (1.0 if d < 0 else 0.0))
        if not ok:
            bad.append("arm %d (%s) does not meet its condition" % (b, kind))
    return bad


def numpy_tracking(poses, v6, active):
    """vfik_numpy.TrackingError stepped over the scene: (T, B, 8), zeros while the history is short or the arm is silent"""
    from oracle import vfik_numpy as vn
    T, B = poses.shape[:2]
    out = np.zeros((T, B, 8))
    for b in range(B):
        est = vn.TrackingError()
        for t in range(T):
            if active[t, b]:
                r = est.update(vn.listToKdlFrame(poses[t, b]), v6[t, b, :3], v6[t, b, 3:])
                if r is not None:
                    out[t, b] = r
            elif t:
                out[t, b] = out[t - 1, b]   # a silent arm's row stays
    return out


TRACK_TABLE = {}


def note_track(side, case, family, ratio, ambiguous, ref):
    TRACK_TABLE[(side, case, family)] = (float(ratio.max()), int(ambiguous.any(axis=0).sum()), int(ref["finite_only"].any(axis=(0, 2)).sum()))


def write_track_table(path):
    with open(path, "a") as f:
        for (side, case, family), (worst, amb, fo) in sorted(TRACK_TABLE.items()):
            f.write("observer %-4s %-34s %-16s worst/bar %6.3f  ambiguous arms %d  finite-only arms %d\n" % (side, case, family, worst, amb, fo))
    TRACK_TABLE.clear()


# =====================================================================================================================================
# The goal distance of the cycle kernels (io.goal_dist): the object-0 entry of /dmonitor/distOut, a by-product of the goal attractor
# =====================================================================================================================================
# The reference: D = |g - p| and theta = atan2(|a|, c) 180 / pi of E = G R^T (rot_axis_angle's wording; NOT the monitor's R^T G: the two agree
# for rotations only), R and p from hp_reference.kinematics() -- the 50-digit forward kinematics of the rounded q --, times a tool of
# hp_reference.TOOLS where the kernel family has one; the goal's 12 numbers taken as exact.  No floor on the angle.
#
# Units.  The inputs of the published value are the goal (12 entries, rounded once: exact here) and the pose, which the kernel COMPUTES: a
# product of n + 1 frames, each entry rounded about once per joint, the position a sum of n terms of the size of the arm's reach.  So
# unit = u (n sum_pose |d out / d x_i| w_i + sum_goal |d out / d x_i| |x_i| + |out|), w_i = |x_i| for the rotation's entries and the batch's
# reach (max |p|) for the position's.  K_MARGIN units, half an ulp of the stored value off at float32 I/O, the finite-only rule as above.
GOAL_KINDS = ("same", "1e-13", "1e-10", "1e-6", "1e-3", "pi/2", "pi-1e-3", "pi-1e-4(1-1e-3)", "pi-1e-4(1+1e-3)", "pi-1e-6", "half_turn", "regular")
GOAL_DIST = (0.0, 1e-12, 1e-6, 1.0, 1e3)
GOAL_ROBOTS = ("powercube6", "lwr", "lwr_dual14")
_GOAL = {}


def goal_scene(oc, robot, io_dtype, tname=None):
    """(chain, params, workload, kinds, dist index, tool16 or None): goals placed relative to the ORACLE'S tool pose (as
    tests/test_gpu_goal_rare_paths.py does), turned by the kind's angle about a random axis and DIST away along a random direction."""
    key = (robot, io_dtype, tname)
    if key in _GOAL:
        return _GOAL[key]
    from vfclik_amd import _abi, robots, synth
    chain = robots.by_name(robot)
    B = B_ARMS
    params = _abi.default_params()
    w = synth.make_workload(chain, B, 2, seed=61, io_dtype=io_dtype)
    tool16 = None if tname is None else hp.tool(tname, io_dtype)[2]
    pose = oc.cycle_batch(chain, params, w["q"], w["fields"], w["nfields"], tool=tool16, want=("pose",))["pose"]
    rng = np.random.default_rng(62)
    kk = [GOAL_KINDS[b % len(GOAL_KINDS)] for b in range(B)]
    di = [(b // len(GOAL_KINDS)) % len(GOAL_DIST) for b in range(B)]
    for b, kind in enumerate(kk):
        if kind == "regular":
            continue
        RP, p = _split(pose[b])
        f = pose[b].copy()
        if kind == "half_turn":
            f[[0, 1, 4, 5, 8, 9]] *= -1.0
        elif kind != "same":
            R = _rot(rng.normal(size=3), THETA[kind])
            for i in range(3):
                for j in range(3):
                    f[4 * i + j] = float(R[i][0] * RP[0][j] + R[i][1] * RP[1][j] + R[i][2] * RP[2][j])   # G = Rot R
        d = rng.normal(size=3)
        d /= np.linalg.norm(d)
        for i in range(3):
            f[4 * i + 3] = float(p[i] + _num(GOAL_DIST[di[b]]) * _num(float(d[i])))
        w["fields"]["p"][b, 0, :16] = f.astype(io_dtype).astype(np.float64)
    _GOAL[key] = (chain, params, w, kk, di, tool16)
    return _GOAL[key]


def _goal_angle_deg(R, G):
    """E = G R^T"""
    return _theta(R, G)[0] * _DEG


def goal_reference(key, chain, q, goals, tool16=None):
    """The shape of `reference` ((B, 1) arrays), for the goal distance; cached by key (which names the pose set for hp_reference too)."""
    if ("goal", key) in _REF:
        return _REF[("goal", key)]
    kin = hp.kinematics(key[:2] + ("arrive" if key[2] == "arrive" else "goal",), chain, q)   # (the tools of one pose set share one FK)
    B, n = len(kin), chain.n
    out = {k: np.zeros((B, 1)) for k in ("D", "D_lo", "ang", "ang_lo", "unit_D", "unit_ang")}
    tips = []
    for b in range(B):
        T = kin[b][0]
        if tool16 is not None:
            T = hp._mul(T, hp._frame(np.asarray(tool16, dtype=np.float64).reshape(4, 4)))
        tips.append(T)
    reach = max(float(_sqrt(T[0][3] ** 2 + T[1][3] ** 2 + T[2][3] ** 2)) for T in tips)
    for b, T in enumerate(tips):
        R, p = [list(T[i][:3]) for i in range(3)], [T[i][3] for i in range(3)]
        G, g = _split(goals[b])
        D, ang = _dist(p, g), _goal_angle_deg(R, G)
        out["D"][b, 0], out["D_lo"][b, 0] = hp._hilo(D)
        out["ang"][b, 0], out["ang_lo"][b, 0] = hp._hilo(ang)
        slope = [abs(float((p[i] - g[i]) / D)) for i in range(3)] if D > 0 else [1.0] * 3
        out["unit_D"][b, 0] = U * (n * reach * sum(slope) + sum(sl * abs(float(x)) for sl, x in zip(slope, g)) + float(D))
        sR = float(_sens(lambda r: _goal_angle_deg(r, G), [R], ang))
        sG = float(_sens(lambda gg: _goal_angle_deg(R, gg), [G], ang))
        out["unit_ang"][b, 0] = U * (n * sR + sG + float(ang))
    _REF[("goal", key)] = out
    return out


def goal_double(pose, goals):
    """The double-precision restatement of the same form on a pose computed in doubles (the oracle's): (B, 1, 2)"""
    B = len(pose)
    out = np.zeros((B, 1, 2))
    for b in range(B):
        A, G = pose[b].reshape(4, 4), goals[b].reshape(4, 4)
        E = G[:3, :3] @ A[:3, :3].T
        a = 0.5 * np.array([E[2, 1] - E[1, 2], E[0, 2] - E[2, 0], E[1, 0] - E[0, 1]])
        c = 0.5 * (E[0, 0] + E[1, 1] + E[2, 2] - 1.0)
        d = G[:3, 3] - A[:3, 3]
        out[b, 0] = math.sqrt(float(d @ d)), math.atan2(math.sqrt(float(a @ a)), c) * (180.0 / math.pi)
    return out


def goal_conditions(io_dtype, kk, di, ref):
    bad = []
    f64 = io_dtype == np.float64
    if not all(len(set(kk[b:b + 8])) == 8 for b in range(len(kk) - 7)):
        bad.append("eight consecutive arms do not hold eight kinds")
    for b, kind in enumerate(kk):
        if kind == "regular":
            continue
        ang, D, nom = ref["ang"][b, 0] * math.pi / 180.0, ref["D"][b, 0], GOAL_DIST[di[b]]
        if (f64 or kind not in F64_ONLY) and abs(ang - THETA[kind]) > (1e-14 if f64 else 1e-6):
            bad.append("arm %d (%s): angle off by %.1e rad" % (b, kind, ang - THETA[kind]))
        if (f64 or nom not in DIST_F64_ONLY) and abs(D - nom) > (1e-14 if f64 else 1e-6) * max(1.0, nom):
            bad.append("arm %d: distance %g for %g" % (b, D, nom))
    half = [b for b, k in enumerate(kk) if k.startswith("pi-1e-4")]
    s = np.sin(ref["ang"][half, 0] * math.pi / 180.0)
    if f64 and not ((s < 1e-4).any() and (s > 1e-4).any()):
        bad.append("the s = 1e-4 switch is not straddled")
    return bad


# ---- arrival: goto's first check -------------------------------------------------------------------------------------------------------
# One cycle, one check, a batch-wide precision of (1e-3 m, 1e-3 rad).  The check measures the tool pose of the cycle it follows -- the pose at
# the q that went in (tests/timed_reference.py: _run takes dist from the rows of the last evaluated cycle) -- reads the goal distance as the
# I/O type stores it, and arrives on D < pos_prec and theta_deg pi / 180 < rot_prec, both strict, in doubles (include/vfik.h: vfik_goto).
# The reference's rule is the same two compares on the 50-digit D and theta.  A decision is exact outside the band |value - threshold| <= bar,
# bar = K_MARGIN units (+ half an ulp of the stored value at float32 I/O; the angle's + 2 u theta for the conversion to radians); at most 5 % of
# a case's arms may be inside, asserted on the reference first -- which is why the 1e-9 offsets, inside the band at float32 I/O, take one
# round in twelve.
ARRIVE_KINDS = ("D_above", "D_below", "th_above", "th_below", "same", "far", "regular", "inside")
ARRIVE_PREC = (1e-3, 1e-3)
_ARRIVE = {}


def arrive_delta(b):
    g = b // len(ARRIVE_KINDS)
    return 1e-9 if g % 12 == 11 else (1e-6 if g % 2 else 1e-3)


def arrive_scene(oc, robot, io_dtype):
    """goal_scene's construction with the goals at threshold (1 +- delta) in D or in the angle, the other well inside"""
    key = (robot, io_dtype)
    if key in _ARRIVE:
        return _ARRIVE[key]
    from vfclik_amd import _abi, robots, synth
    chain = robots.by_name(robot)
    B = B_ARMS
    params = _abi.default_params()
    w = synth.make_workload(chain, B, 2, seed=67, io_dtype=io_dtype)
    pose = oc.cycle_batch(chain, params, w["q"], w["fields"], w["nfields"], want=("pose",))["pose"]
    rng = np.random.default_rng(68)
    kk = [ARRIVE_KINDS[b % len(ARRIVE_KINDS)] for b in range(B)]
    for b, kind in enumerate(kk):
        if kind == "regular":
            continue
        dl = arrive_delta(b)
        D = {"D_above": ARRIVE_PREC[0] * (1 + dl), "D_below": ARRIVE_PREC[0] * (1 - dl), "same": 0.0, "far": 0.2}.get(kind, 1e-5)
        th = {"th_above": ARRIVE_PREC[1] * (1 + dl), "th_below": ARRIVE_PREC[1] * (1 - dl), "same": 0.0, "far": 0.5}.get(kind, 1e-4)
        RP, p = _split(pose[b])
        f = pose[b].copy()
        if th:
            R = _rot(rng.normal(size=3), th)
            for i in range(3):
                for j in range(3):
                    f[4 * i + j] = float(R[i][0] * RP[0][j] + R[i][1] * RP[1][j] + R[i][2] * RP[2][j])
        d = rng.normal(size=3)
        d /= np.linalg.norm(d)
        for i in range(3):
            f[4 * i + 3] = float(p[i] + _num(D) * _num(float(d[i])))
        w["fields"]["p"][b, 0, :16] = f.astype(io_dtype).astype(np.float64)
    _ARRIVE[key] = (chain, params, w, kk)
    return _ARRIVE[key]


def arrive_rule(ref, io_dtype):
    """(arrives (B,), ambiguous (B,)) of a goal_reference"""
    D, th = ref["D"][:, 0] + ref["D_lo"][:, 0], (ref["ang"][:, 0] + ref["ang_lo"][:, 0]) * (math.pi / 180.0)
    bar_D, bar_th = K_MARGIN * ref["unit_D"][:, 0], K_MARGIN * ref["unit_ang"][:, 0] * (math.pi / 180.0) + 2 * U * th
    if io_dtype == np.float32:
        bar_D = bar_D + 0.5 * np.spacing(ref["D"][:, 0].astype(np.float32)).astype(np.float64)
        bar_th = bar_th + 0.5 * np.spacing(ref["ang"][:, 0].astype(np.float32)).astype(np.float64) * (math.pi / 180.0)
    amb = (np.abs(D - ARRIVE_PREC[0]) <= bar_D) | (np.abs(th - ARRIVE_PREC[1]) <= bar_th)
    return (D < ARRIVE_PREC[0]) & (th < ARRIVE_PREC[1]), amb


def arrive_conditions(io_dtype, kk, ref):
    bad = []
    arr, amb = arrive_rule(ref, io_dtype)
    if amb.sum() > AMBIGUOUS_CAP * len(kk):
        bad.append("%d of %d arms are inside the decision's band" % (amb.sum(), len(kk)))
    if not all(len(set(kk[b:b + 8])) == 8 for b in range(len(kk) - 7)):
        bad.append("eight consecutive arms do not hold eight kinds")
    D, th = ref["D"][:, 0], ref["ang"][:, 0] * math.pi / 180.0
    for b, kind in enumerate(kk):
        dl, ok = arrive_delta(b), True
        if kind in ("same", "inside"):
            ok = arr[b] and not amb[b]
        elif kind == "far":
            ok = not arr[b] and not amb[b]
        elif io_dtype == np.float64 and kind != "regular":
            v, t, other = (D[b], ARRIVE_PREC[0], th[b] < 0.5 * ARRIVE_PREC[1]) if kind[0] == "D" else (th[b], ARRIVE_PREC[1], D[b] < 0.5 * ARRIVE_PREC[0])
            sign = 1.0 if kind.endswith("above") else -1.0
            ok = other and abs(v / t - 1.0 - sign * dl) < 1e-11 and arr[b] == (sign < 0) and not amb[b]
        if not ok:
            bad.append("arm %d (%s, delta %g) does not meet its condition" % (b, kind, dl))
    return bad


# ---- the two wordings of the relative rotation -------------------------------------------------------------------------------------
# monitor_kernel words it E = R_cur^T R_obj, the cycle kernels' goal distance and vfik_numpy.rot_log E = G R^T.  For rotations the angle is
# the same; for frames rounded to float32, or typed with four decimals, it is not (next to a half turn by some 1e-8 rad).  Each side is held to
# the reference of its OWN wording; where two sides of different wordings are compared with each other, the difference of their references goes
# in as it is and only the two bars remain.
def reference_grt(key, pose, frames):
    """`reference` for the G R^T wording of the same frames ((B, O) arrays; D is the same number)"""
    if ("grt", key) in _REF:
        return _REF[("grt", key)]
    B, n_obj = frames.shape[:2]
    out = {k: np.zeros((B, n_obj)) for k in ("D", "D_lo", "ang", "ang_lo", "unit_D", "unit_ang")}
    for b in range(B):
        RP, p = _split(pose[b])
        for k in range(n_obj):
            RF, o = _split(frames[b, k])
            D, ang = _dist(p, o), _goal_angle_deg(RP, RF)
            out["D"][b, k], out["D_lo"][b, k] = hp._hilo(D)
            out["ang"][b, k], out["ang_lo"][b, k] = hp._hilo(ang)
            out["unit_D"][b, k] = U * float(_sens(_dist, [p, o], D) + abs(D))
            out["unit_ang"][b, k] = U * float(_sens(_goal_angle_deg, [RP, RF], ang) + abs(ang))
    _REF[("grt", key)] = out
    return out


FLOOR_RAD = 1e-12   # vfik_numpy.rot_log: no rotation below |a| = 1e-12 (EPS_LEN)


def numpy_monitor(pose, frames):
    """vfik_numpy.object_distances (rot_log: the G R^T wording, with its floor) over the scene: (B, O, 2)"""
    from oracle import vfik_numpy as vn
    B, n_obj = frames.shape[:2]
    out = np.zeros((B, n_obj, 2))
    for b in range(B):
        for k, (_, d, ang) in enumerate(vn.object_distances(pose[b], {k: frames[b, k] for k in range(n_obj)})):
            out[b, k] = d, ang
    return out


def floored(ref):
    """pairs whose reference angle is at or below the restatement's floor (with the bar's width): there it may publish 0"""
    return ref["ang"] * (math.pi / 180.0) <= FLOOR_RAD + K_MARGIN * ref["unit_ang"] * (math.pi / 180.0)


def pair_ratio(a, b, ref_a, ref_b, io_dtype):
    """Two published (B, 2) rows of different wordings against each other: |(a - b) - (ref_a - ref_b)| over bar_a + bar_b (+ half an ulp of each
    stored value at float32 I/O), for D and the angle; pairs with a finite-only side count 0.  ref_*: (B, 1) references."""
    res = []
    fo = np.logical_or(*finite_only(ref_a)) | np.logical_or(*finite_only(ref_b))
    for i, name in enumerate(("D", "ang")):
        want = (ref_a[name] - ref_b[name]) + (ref_a[name + "_lo"] - ref_b[name + "_lo"])
        err = np.abs((np.asarray(a, dtype=np.float64)[:, i] - np.asarray(b, dtype=np.float64)[:, i]) - want[:, 0])
        bar = K_MARGIN * (ref_a["unit_" + name] + ref_b["unit_" + name])[:, 0]
        if io_dtype == np.float32:
            bar = bar + 0.5 * (np.spacing(np.abs(ref_a[name][:, 0]).astype(np.float32)) + np.spacing(np.abs(ref_b[name][:, 0]).astype(np.float32))).astype(np.float64)
        r = np.where(fo[:, 0], 0.0, err / bar)
        res.append(np.where(np.isnan(r), np.inf, r))
    return res[0], res[1]
