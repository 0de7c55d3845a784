"""A high-precision restatement of DESIGN 2.1's field, its condition numbers, and the edge scenes of the field sweep.

A helper of the suite like hp_reference.py (whose back end and (hi, lo) result pairs it shares), not a conftest.py:
tests/test_oracle_field_edges.py holds the two CPU oracles to it, tests/test_gpu_field_edges.py the HIP kernels.

The reference.  From the doubles of an arm's field records (taken as exact), a tool pose (hp_reference's 50-digit FK for the cycle
kernels; doubles taken as exact for the probe), rot_slowdown and speedScale:

  * the primitives of types 0, 1, 2, 4, 5 with EPS_LEN = 1e-12, the 1e-9 floors and the 1e6 cap as DESIGN 2.1 words them;
  * total = sum force_k vec_k, S = product of the scalars, normCart, v = speedScale S0 t^, w = speedScale S1 r^;
  * v6 = (v, w): the tools here are the identity, so v6 is the twist the solve sees.

Per arm, from the reference alone:

  kappa_sum   per 3-vector part sum_k (1 + n_k) |force_k vec_k| / |sum_k force_k vec_k|, n_k the largest decay order of primitive k
              whose power is not clipped at that arm (0 for attractors and for clipped terms); the larger of the two parts.
              ADDED: in the rotational part an attractor's term is weighted by 1 / sin(theta_k) instead of 1 (see below);
  kappa_pose  sum over six perturbed evaluations of |delta v6|_inf / DELTA, DELTA = 1e-20: the tool moved by DELTA metres along each
              base axis, and turned by DELTA rad about each base axis; 0 for the probe, whose pose is an exact input;
  kappa_rel   ADDED to the issue's two (see below): sum over the primitives k and the three axes of |delta v6|_inf / DELTA with
              primitive k alone seeing the tool moved by DELTA |w_k| along the axis, w_k = tool - primitive.

  E = u (kappa_pose + kappa_rel + (4 + kappa_sum) max|v6|),  u = 2^-53.

Why kappa_rel.  Every implementation forms w_k = p - o_k, dot products and differences of it (h = w.n^, perp = w - (w.a^) a^, |w|) in
double arithmetic: errors of size u |w_k|, which act like a move of primitive k by that much.  Inside a 1e-9 floor the spec's own
Lipschitz constant is force / 1e-9 (times the 1e6 cap for a repeller), and on a funnel's axis perp is ALL rounding error.  kappa_pose
sees this for the cycle kernels, through the tool position all primitives share -- but it is 0 for the probe by definition, where nothing
else in E would carry the 1e9: the plain-double C oracle itself misses 8 u (4 + kappa_sum) max|v6| on the on-axis funnel arms of the probe
scenes by four orders of magnitude.  The term is the reference's own sensitivity, computed without any implementation's output.

Why 1 / sin(theta).  The spec takes an attractor's axis as a / |a|, a the antisymmetric part of G R^T: differences of entries of size 1
with |a| = sin(theta), so the entries' rounding (and the tool rotation's, which FK leaves orthogonal to u only) reaches the axis
amplified by 1 / sin(theta).  A perturbation that keeps R a rotation, which is all kappa_pose tries, does not see it.  Two regular
goals of make_workload's 192 lie at theta = 3.13: the C oracle is 15 E off there without the weight.

An arm whose 8 E exceeds 1e-3 max|v6| is FINITE-ONLY: there the spec itself amplifies rounding to more than a part in a thousand of the
answer, and only finiteness, the status and the speed limit are held.

The scenes (make_scene).  192 arms = three waves at the regular poses of synth.make_workload (seed 3); every primitive under test is
placed relative to the ORACLE'S OWN tool pose along seeded random unit directions, kinds cycling arm by arm so that any eight
consecutive arms hold eight different kinds; inputs are rounded to the I/O type before either side sees them.  After the positions are
rounded, the free scalar of the kind (radius, safe distance, cut angle, cut distance, slow-down distance, a force) is recomputed from the
ROUNDED geometry, so that ratio edges (1 +- 1e-6, 1 +- 1e-3, the cap) are met at float32 I/O as well.  Edges that need a POSITION finer
than the float32 grid at 0.5 m (3e-8: D or h of 1e-10 ... 1e-6, phi within 1e-9 rad of a boundary, ratio 1 +- 1e-9, cancellation to
1e-6) cannot exist at float32 I/O: those arms are still built and compared there, but their kind's condition is asserted at float64 I/O
only (F64_ONLY).

Scene ids: "1-oN" one integer order N, safe distance and force differing (compact image); "1-o5-pc6" the same on the powercube6;
"2-oN" shared safe distance and force (uniform image); "3" orders (5, 20) (MIXO, the 2^j shortcut); "4" (3, 7) (MIXO, two orders);
"5" (2, 5, 20), and on every fourth arm orders of its own with 0 and 127 among them (MIXO, per lane); "6" funnel and hemisphere (aux
block) beside two order-5 repellers that cancel to 1e-3 / 1e-6 on two arms in five; "7" orders 2.5 and 128, a second funnel, hemisphere and attractor (general path); "P-rep", "P-aux": the probe, pose given."""
import math

import numpy as np

import hp_reference as hp

_num = hp._num
if hp.BACKEND == "mpmath":
    import mpmath as _mpm
    _sqrt, _atan2, _powf = _mpm.sqrt, _mpm.atan2, _mpm.power
    DELTA = _num(10) ** -20
else:
    _sqrt, _atan2, _powf = np.sqrt, np.arctan2, np.power
    DELTA = _num(2.0) ** -30
EPS_LEN, D_FLOOR, MAG_CAP = _num("1e-12"), _num("1e-9"), _num("1e6")
ZERO, ONE = _num(0), _num(1)
U = hp.U
B_ARMS = hp.B_ARMS
LAMBDA = 0.1
FINITE_ONLY = 1e-3

T_NULL, T_ATT, T_REP, T_HEM, T_FUN = 0, 1, 2, 4, 5


def _powr(x, n):
    """x^n, x >= 0, n a double"""
    if n == int(n):
        return x ** int(n)
    return ZERO if x == 0 else _powf(x, _num(n))


def _norm(v):
    return _sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])


def _f(x):
    return _num(float(x))


def _prim(ftype, p, T, rot_slow):
    """One primitive at tool pose T (3x4): (vec_t, vec_r, s0, s1, n_k, |w_k|, info).  vec without the force."""
    z3 = [ZERO, ZERO, ZERO]
    pt = [T[0][3], T[1][3], T[2][3]]
    if ftype == T_REP:
        d = [_f(p[i]) - pt[i] for i in range(3)]
        Dn = _norm(d)
        D = Dn if Dn > D_FLOOR else D_FLOOR
        rs, order = _f(p[3]) + _f(p[4]), float(p[5])
        raw = _powr(rs / D, order)
        clipped = raw > MAG_CAP
        m = MAG_CAP if clipped else raw
        return [m * x / D for x in d], z3, ONE, ONE, (0.0 if clipped else order), Dn, dict(D=Dn, ratio=rs / D, clipped=clipped, m=m, rs=rs)
    if ftype == T_HEM:
        n = [_f(p[3 + i]) for i in range(3)]
        nn = _norm(n)
        w = [pt[i] - _f(p[i]) for i in range(3)]
        if not nn > EPS_LEN:
            return z3, z3, ONE, ONE, 0.0, _norm(w), dict(off=True)
        nh = [x / nn for x in n]
        h = w[0] * nh[0] + w[1] * nh[1] + w[2] * nh[2]
        safe, order = _f(p[6]), float(p[7])
        raw = _powr(safe / (h if h > D_FLOOR else D_FLOOR), order)
        clipped = raw > MAG_CAP
        m = MAG_CAP if clipped else raw
        return [-m * x for x in nh], z3, ONE, ONE, (0.0 if clipped else order), _norm(w), dict(off=False, h=h, clipped=clipped, m=m, nn=nn)
    if ftype == T_FUN:
        a = [_f(p[3 + i]) for i in range(3)]
        an = _norm(a)
        w = [pt[i] - _f(p[i]) for i in range(3)]
        dist = _norm(w)
        if not an > EPS_LEN:
            return z3, z3, ONE, ONE, 0.0, dist, dict(off=True)
        ah = [x / an for x in a]
        along = w[0] * ah[0] + w[1] * ah[1] + w[2] * ah[2]
        perp = [w[i] - along * ah[i] for i in range(3)]
        P = _norm(perp)
        phi = _atan2(P, along)
        cutA, ordA, cutD, ordD = _f(p[6]), float(p[7]), _f(p[8]), float(p[9])
        n_k = 0.0
        ga, ga_clipped = ONE, True
        if cutA > 0:
            raw = _powr(phi / cutA, ordA)
            ga_clipped = raw > 1
            ga = ONE if ga_clipped else raw
            if not ga_clipped:
                n_k = max(n_k, ordA)
        raw = _powr(cutD / (dist if dist > D_FLOOR else D_FLOOR), ordD)
        gd_clipped = raw > 1
        gd = ONE if gd_clipped else raw
        if not gd_clipped:
            n_k = max(n_k, ordD)
        Pf = P if P > D_FLOOR else D_FLOOR
        return [-x / Pf * ga * gd for x in perp], z3, ONE, ONE, n_k, dist, dict(off=False, phi=phi, P=P, along=along, dist=dist,
                                                                                   ga_clipped=ga_clipped, gd_clipped=gd_clipped)
    if ftype == T_ATT:
        G = [[_f(p[4 * r + c]) for c in range(4)] for r in range(3)]
        d = [G[i][3] - pt[i] for i in range(3)]
        D = _norm(d)
        E = [[G[i][0] * T[j][0] + G[i][1] * T[j][1] + G[i][2] * T[j][2] for j in range(3)] for i in range(3)]
        a = [(E[2][1] - E[1][2]) / 2, (E[0][2] - E[2][0]) / 2, (E[1][0] - E[0][1]) / 2]
        c = (E[0][0] + E[1][1] + E[2][2] - 1) / 2
        s = _norm(a)
        assert not (s < _num("1e-4") and c < 0), "a goal at a half turn: tests/test_gpu_goal_rare_paths.py holds those, not this reference"
        th = _atan2(s, c)
        vt = [x / D for x in d] if D > EPS_LEN else z3
        vr = [x / s for x in a] if (th > EPS_LEN and s >= EPS_LEN) else z3   # r / theta = a / s
        ds = _f(p[16])
        s0 = (D / ds if D < ds else ONE) if ds > 0 else ONE
        rsl = _f(rot_slow)
        s1 = (th / rsl if th < rsl else ONE) if rsl > 0 else ONE
        return vt, vr, s0, s1, 0.0, D, dict(D=D, ds=ds, s0=s0, theta=th), (ONE / s if s >= EPS_LEN else ONE)
    assert ftype == T_NULL, ftype
    return z3, z3, ONE, ONE, 0.0, ZERO, {}


def _combine(terms, forces, speed):
    """(v6, kappa_sum) from the primitives' terms"""
    v6, kap = [], 0.0
    S = [ONE, ONE]
    for t in terms:
        S[0], S[1] = S[0] * t[2], S[1] * t[3]
    for part in (0, 1):
        tot, mass = [ZERO, ZERO, ZERO], ZERO
        for t, f in zip(terms, forces):
            fv = [f * x for x in t[part]]
            tot = [tot[i] + fv[i] for i in range(3)]
            mass = mass + ((1 + t[4]) if part == 0 else (t[7] if len(t) > 7 else 1)) * _norm(fv)
        n = _norm(tot)
        if n > EPS_LEN:
            v6 += [speed * S[part] * x / n for x in tot]
            kap = max(kap, float(mass / n))
        else:
            v6 += [ZERO, ZERO, ZERO]
    return v6, kap


def _dinf(a, b):
    return max(abs(x - y) for x, y in zip(a, b))


def _arm(rec, nf, T, rot_slow, speed, with_pose):
    order = sorted(range(int(nf)), key=lambda k: int(rec["id"][k]))   # ascending id, as the field is rebuilt
    prims = [(int(rec["type"][k]), rec["p"][k]) for k in order]
    forces = [_f(rec["force"][k]) for k in order]
    sp = _f(speed)
    terms = [_prim(t, p, T, rot_slow) for t, p in prims]
    v6, kap_sum = _combine(terms, forces, sp)
    kap_pose = kap_rel = ZERO
    for ax in range(3):
        if with_pose:
            Tt = [row[:] for row in T]
            Tt[ax][3] = Tt[ax][3] + DELTA
            kap_pose = kap_pose + _dinf(_combine([_prim(t, p, Tt, rot_slow) for t, p in prims], forces, sp)[0], v6) / DELTA
            # turned by DELTA about base axis ax: R' = (I + DELTA [e_ax]x) R; only the attractors see the rotation
            i, j = (ax + 1) % 3, (ax + 2) % 3
            Tr = [row[:] for row in T]
            for c in range(3):
                Tr[i][c], Tr[j][c] = T[i][c] - DELTA * T[j][c], T[j][c] + DELTA * T[i][c]
            tr = [_prim(t, p, Tr, rot_slow) if t == T_ATT else terms[k] for k, (t, p) in enumerate(prims)]
            kap_pose = kap_pose + _dinf(_combine(tr, forces, sp)[0], v6) / DELTA
        for k, (t, p) in enumerate(prims):
            if t == T_NULL or terms[k][5] == 0:
                continue
            Tt = [row[:] for row in T]
            Tt[ax][3] = Tt[ax][3] + DELTA * terms[k][5]
            tk = terms[:k] + [_prim(t, p, Tt, rot_slow)] + terms[k + 1:]
            kap_rel = kap_rel + _dinf(_combine(tk, forces, sp)[0], v6) / DELTA
    return v6, kap_sum, float(kap_pose), float(kap_rel), [t[6] for t in terms], order


_REF = {}


def reference(key, fields, nfields, rot_slow, speed, chain=None, q=None, poses=None, kin_key=None):
    """The reference of one scene, cached under `key`.  Cycle kernels: chain and q (the pose is hp_reference's 50-digit FK, cached under
    the same key); probe: poses (B, 16) doubles, exact.  Returns dict(v6, v6_lo (B, 6), kappa_sum, kappa_pose, kappa_rel, E, vmax (B,),
    finite_only (B,) bool, info: per arm the primitives' measured quantities in ascending-id order, order: their record indices)."""
    if key in _REF:
        f0, out = _REF[key]
        assert f0 == (fields.tobytes(), np.asarray(nfields).tobytes()), "reference(%r): another field set under the same key" % (key,)
        return out
    B = fields.shape[0]
    if poses is None:
        Ts = [T for T, _ in hp.kinematics(kin_key or key, chain, q)]
    else:
        Ts = [[[_f(poses[b, 4 * r + c]) for c in range(4)] for r in range(3)] for b in range(B)]
    out = dict(v6=np.zeros((B, 6)), v6_lo=np.zeros((B, 6)), kappa_sum=np.zeros(B), kappa_pose=np.zeros(B), kappa_rel=np.zeros(B),
               info=[], order=[])
    for b in range(B):
        v6, out["kappa_sum"][b], out["kappa_pose"][b], out["kappa_rel"][b], info, order = _arm(fields[b], nfields[b], Ts[b], rot_slow,
                                                                                               speed, poses is None)
        for i in range(6):
            out["v6"][b, i], out["v6_lo"][b, i] = hp._hilo(v6[i])
        out["info"].append(info)
        out["order"].append(order)
    out["vmax"] = np.abs(out["v6"]).max(axis=1)
    out["E"] = U * (out["kappa_pose"] + out["kappa_rel"] + (4.0 + out["kappa_sum"]) * out["vmax"])
    out["finite_only"] = hp.K_MARGIN * out["E"] > FINITE_ONLY * out["vmax"]
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _REF[key] = ((fields.tobytes(), np.asarray(nfields).tobytes()), out)
    return out


def v6_error(got, ref):
    return np.abs((np.asarray(got, dtype=np.float64) - ref["v6"]) - ref["v6_lo"])


def v6_ratio(got, ref, io_dtype=np.float64):
    """per arm max_i err / E, float32's half ulp of the stored value taken off first; finite-only arms 0"""
    err = v6_error(got, ref)
    if io_dtype == np.float32:
        err = np.maximum(err - 2.0 ** -24 * np.abs(ref["v6"]), 0.0)
    r = err.max(axis=1) / ref["E"]
    return np.where(ref["finite_only"], 0.0, r)


def v6_bar(ref, io_dtype, R):
    """(B, 6): max(S, K E), K = 8 max(1, R) [+ half an ulp of the float32 store]"""
    K = hp.K_MARGIN * max(1.0, R)
    bar = np.repeat(np.maximum(hp.S_BAR[io_dtype], K * ref["E"])[:, None], 6, axis=1)
    if io_dtype == np.float32:
        bar = bar + 2.0 ** -24 * np.abs(ref["v6"])
    return bar


# ---- the scenes ----------------------------------------------------------------------------------------------------------------------
SCENE1_ORDERS = (0, 1, 2, 5, 20, 127)
CYCLE_SCENES = tuple("1-o%d" % n for n in SCENE1_ORDERS) + ("1-o5-pc6", "2-o5", "2-o20", "3", "4", "5", "6", "7")
PROBE_SCENES = ("P-rep", "P-aux")
SCENES = CYCLE_SCENES + PROBE_SCENES
CODE_PATH_SCENES = CYCLE_SCENES   # every one reaches kappa_sum >= 1e3 on some arm (asserted)

R_KINDS = ("floor10", "floor-", "floor+", "D1e-6", "cap+6", "cap-6", "cap+3", "cap-3", "ratio+9", "ratio-9", "far50", "rs0", "force0",
           "force+", "cancel3", "cancel6", "goal+6", "goal-6", "regular")
H_KINDS = ("h-0.1", "h1e-10", "hfloor-", "hfloor+", "hcap+6", "hcap-6", "hsafe", "h50safe", "n3", "n1e-3", "n1e-13")
F_KINDS = tuple("phi%d%s" % (k, s) for k in range(1, 8) for s in "+-") + ("cutang+6", "cutang-6", "cutdist+6", "cutdist-6", "axis_front",
                                                                            "axis_behind", "apex", "cutang0")
P_R_KINDS = R_KINDS + ("D0",)
R6_KINDS = ("regular", "cancel3", "regular", "cancel6", "regular")   # scene 6: the aux block under cancellation (its repellers are not the edge)
P_H_KINDS = H_KINDS + ("h0",)
P_F_KINDS = F_KINDS + ("perp0",)
# kinds that need a position finer than the float32 grid: their condition is asserted at float64 I/O only
F64_ONLY = {"floor10", "floor-", "floor+", "D1e-6", "ratio+9", "ratio-9", "cancel6", "h1e-10", "hfloor-", "hfloor+", "axis_front",
            "axis_behind", "apex"} | {k for k in F_KINDS if k.startswith("phi")}
FUNNEL_ORDERS = (0, 1, 2, 10, 127)
HEM_ORDERS = (5, 0, 1, 2, 20, 127)
ARM_ORDERS = (0, 127, 1, 3, 7, 13)   # scene 5: every fourth arm's own orders


def robot_of(sid):
    return "powercube6" if sid.endswith("-pc6") else "lwr"


def _orders_of(sid, b):
    """decay orders of the arm's repeller slots (A, B[, C])"""
    if sid.startswith("1-o") or sid.startswith("2-o"):
        n = float(sid.split("-")[1][1:])
        return (n, n)
    if sid == "3":
        return (5.0, 20.0)
    if sid == "4":
        return (3.0, 7.0)
    if sid == "5":
        if b % 4 == 3:
            k = b // 4
            return (float(ARM_ORDERS[k % 6]), float(ARM_ORDERS[(k + 1 + k // 6) % 6] or 5), float(ARM_ORDERS[(k + 3) % 6]))
        return (2.0, 5.0, 20.0)
    if sid == "7":
        return (2.5, 128.0)
    if sid == "P-rep":
        return ((5.0, 20.0), (2.5, 128.0), (0.0, 1.0), (127.0, 2.0))[b % 4]
    return (5.0, 5.0)


def _unit(rng):
    v = rng.normal(size=3)
    return v / np.linalg.norm(v)


def _perp_unit(rng, a):
    v = rng.normal(size=3)
    v -= (v @ a) * a
    return v / np.linalg.norm(v)


def _toward(x, io, up):
    """the io-type neighbour of x above (up) or below"""
    return float(np.nextafter(io(x), io(np.inf if up else -np.inf)))


def _fix(value, io, ok):
    """value rounded to io, nudged by up to 8 neighbours either way until ok(value) holds (the side of an edge); the rounded value if none does"""
    v0 = float(io(value))
    for up in (True, False):
        v = v0
        for _ in range(9):
            if ok(v):
                return v
            v = _toward(v, io, up)
    return v0


def make_scene(oc, sid, io_dtype):
    """dict(sid, chain, params, w, pose: the oracle's tool pose (B, 16) -- for a probe scene the pose GIVEN, rounded to the I/O type --,
    probe, rk / hk / fk: per arm the kind names of its repeller A, hemisphere and funnel (None where it has none), slots: record index of
    (repA, repB, hemisphere, funnel) or None, max_slots, uniform: shared safe distance and force)"""
    from vfclik_amd import _abi, synth
    io = io_dtype
    rnd = lambda x: np.asarray(x, dtype=np.float64).astype(io).astype(np.float64)
    chain = hp.chain_of(robot_of(sid))
    probe = sid in PROBE_SCENES
    aux = sid in ("6", "7", "P-aux")
    reps = sid != "P-aux"
    nrep = 0 if not reps else (3 if sid == "5" else 2)
    B = B_ARMS
    M = 1 + nrep + (2 if aux else 0) + (3 if sid == "7" else 0)
    params = _abi.default_params(**{"lambda": LAMBDA})
    w = synth.make_workload(chain, B, nrep, seed=3, io_dtype=io, max_fields=M)
    w["nfields"][:] = M
    F = w["fields"]
    pose = oc.cycle_batch(chain, params, w["q"], F[:, :1 + nrep], np.full(B, 1 + nrep, dtype=np.int32), want=("pose",))["pose"]
    if probe:   # the pose given: rotations exact at either I/O type (signed permutations), the oracle's positions rounded
        ROTS = (np.eye(3), np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 1]]), np.array([[1.0, 0, 0], [0, 0, -1], [0, 1, 0]]),
                np.array([[0.0, 0, 1], [0, 1, 0], [-1, 0, 0]]))
        for b in range(B):
            P4 = np.eye(4)
            P4[:3, :3] = ROTS[b % 4]
            P4[:3, 3] = rnd(pose[b, [3, 7, 11]])
            pose[b] = P4.reshape(16)
    p = pose[:, [3, 7, 11]].copy()
    rng = np.random.default_rng(17)
    uniform = sid.startswith("2-") or sid == "5"
    rkinds, hkinds, fkinds = (P_R_KINDS, P_H_KINDS, P_F_KINDS) if probe else (R6_KINDS if sid == "6" else R_KINDS, H_KINDS, F_KINDS)
    rk, hk, fk = [None] * B, [None] * B, [None] * B
    iA, iB = (1, 2) if nrep >= 2 else ((1, None) if nrep == 1 else (None, None))
    iH, iF = (1 + nrep, 2 + nrep) if aux else (None, None)
    safeA, safeB = float(io(0.001)), float(io(0.001 if uniform else 0.002))
    fA, fB = -10.0, (-10.0 if uniform else -7.0)
    dist = lambda b, o: float(np.linalg.norm(np.asarray(o) - p[b]))

    for b in range(B):
        if nrep >= 2:
            kind = rkinds[b % len(rkinds)]
            if uniform and kind in ("force0", "force+"):   # one force for the batch: these arms are regular ones there
                kind = "regular"
            rk[b] = kind
            orders = _orders_of(sid, b)
            oA, oB = orders[0], orders[1]
            A, Bq = F[b, iA], F[b, iB]
            A["p"][4], Bq["p"][4], A["force"], Bq["force"] = safeA, safeB, fA, fB
            for i, o in zip(range(1, 1 + nrep), orders):
                F[b, i]["p"][5] = o
            if nrep == 3:
                F[b, 3]["p"][4], F[b, 3]["force"] = safeA, fA
            n = _unit(rng)
            rad = 0.05
            rs = rad + safeA
            cap = rs * 1e6 ** (-1.0 / oA) if oA > 0 else 0.5 * rs
            D = {"floor10": 1e-10, "floor-": 1e-9 * (1 - 1e-3), "floor+": 1e-9 * (1 + 1e-3), "D1e-6": 1e-6, "cap+6": cap * (1 + 1e-6),
                 "cap-6": cap * (1 - 1e-6), "cap+3": cap * (1 + 1e-3), "cap-3": cap * (1 - 1e-3), "ratio+9": rs, "ratio-9": rs,
                 "far50": 50 * rad, "rs0": 0.08, "D0": 0.0}.get(kind)
            if kind.startswith("cancel"):   # a magnitude of 32 at the higher orders: under the cap at order 127 as well
                D = rs * 32.0 ** (-1.0 / oA) if oA >= 5 else 0.5 * rs
            if kind in ("force0", "force+", "goal+6", "goal-6", "regular"):
                D = None   # repeller A stays where make_workload put it
            if D is not None:
                A["p"][0:3] = rnd(p[b] + D * n) if D > 0 else p[b]
                Da = dist(b, A["p"][0:3])
                if kind.startswith("cap") and oA > 0:
                    eps = float(kind[3] + "1e-" + kind[4])
                    tgt = Da / (1e6 ** (-1.0 / oA) * (1 + eps))
                    clipped = eps < 0
                    A["p"][3] = _fix(tgt - safeA, io, lambda r: ((r + safeA) / Da) ** oA > 1e6 if clipped else ((r + safeA) / Da) ** oA < 1e6)
                elif kind.startswith("ratio"):
                    above = kind[5] == "+"
                    tgt = Da * (1 + 1e-9 if above else 1 - 1e-9)
                    A["p"][3] = _fix(tgt - safeA, io, lambda r: (r + safeA > Da) if above else (r + safeA < Da))
                elif kind == "rs0":
                    A["p"][3] = -safeA
                else:
                    A["p"][3] = float(io(rad))
            if kind == "force0":
                A["force"] = 0.0
            elif kind == "force+":
                A["force"] = 10.0
            if kind.startswith("cancel"):   # B opposite A, its term (1 - eps) of A's
                eps = 1e-3 if kind == "cancel3" else 1e-6
                if not uniform:
                    A["force"] = Bq["force"] = -1e4
                Bq["p"][0:3] = rnd(p[b] - (0.6 * rs) * n)
                Da, Db = dist(b, A["p"][0:3]), dist(b, Bq["p"][0:3])
                mA = min(((A["p"][3] + safeA) / Da) ** oA, 1e6)
                if oB > 0:
                    mB = mA * float(A["force"]) / float(Bq["force"]) * (1 - eps)
                    Bq["p"][3] = float(io(Db * mB ** (1.0 / oB) - safeB))
                else:   # order 0: the magnitude is 1 whatever the radius -- the force carries the (1 - eps)
                    Bq["force"] = float(io(float(A["force"]) * mA * (1 - eps)))
            if kind.startswith("goal"):
                above = kind[4] == "+"
                G = F[b, 0]["p"]
                ds0 = 0.05
                G[[3, 7, 11]] = rnd(p[b] + ds0 * n)
                Dg = dist(b, G[[3, 7, 11]])
                G[16] = _fix(Dg / (1 + 1e-6 if above else 1 - 1e-6), io, lambda s: (Dg > s) if above else (Dg < s))
        if aux:
            hkind, fkind = hkinds[(b + b // len(fkinds)) % len(hkinds)], fkinds[b % len(fkinds)]   # (shifted: a funnel kind meets every hemisphere kind)
            hk[b], fk[b] = hkind, fkind
            # ---- the hemisphere
            H = F[b, iH]
            H["id"], H["type"], H["force"] = 40, T_HEM, -50.0
            order = float(HEM_ORDERS[(b // len(hkinds)) % len(HEM_ORDERS)])
            if hkind.startswith("hcap") and order == 0:
                order = 5.0
            safe = 0.05
            L = {"n3": 3.0, "n1e-3": 1e-3, "n1e-13": 1e-13}.get(hkind, 1.0)
            nh = _unit(rng)
            tang = 0.1 * _perp_unit(rng, nh)
            capf = 1e6 ** (-1.0 / order) if order > 0 else 1.0
            h = {"h-0.1": -0.1, "h1e-10": 1e-10, "hfloor-": 1e-9 * (1 - 1e-3), "hfloor+": 1e-9 * (1 + 1e-3), "hcap+6": safe * capf,
                 "hcap-6": safe * capf, "hsafe": safe, "h50safe": 0.5, "h0": 0.0}.get(hkind, 0.02)
            nvec = rnd(L * nh)
            H["p"][3:6] = nvec
            nhr = nvec / np.linalg.norm(nvec)
            tang -= (tang @ nhr) * nhr
            H["p"][0:3] = p[b] if hkind == "h0" else rnd(p[b] - h * nhr - tang)
            ha = float((p[b] - H["p"][0:3]) @ nhr)
            if hkind.startswith("hcap"):
                clipped = hkind[4] == "-"
                tgt = ha / (capf * (1 - 1e-6 if clipped else 1 + 1e-6))
                safe = _fix(tgt, io, lambda s: (s / ha) ** order > 1e6 if clipped else (s / ha) ** order < 1e6)
            elif hkind == "hsafe":
                safe = float(io(ha))
            elif hkind == "h50safe":
                safe = float(io(ha / 50.0))
            H["p"][6], H["p"][7] = float(io(safe)), order
            # ---- the funnel
            Fu = F[b, iF]
            Fu["id"], Fu["type"], Fu["force"] = 2, T_FUN, 30.0
            j = b // len(fkinds)
            ordA, ordD = float(FUNNEL_ORDERS[j % 5]), float(FUNNEL_ORDERS[(j + 1 + b % 3) % 5])
            a = rnd(_unit(rng))
            ah = a / np.linalg.norm(a)
            e = _perp_unit(rng, ah)
            r = 0.1
            cutA, cutD = 0.15, (0.15 if b % 2 else 0.05)
            if fkind.startswith("phi"):
                phi = int(fkind[3]) * math.pi / 8 + (1e-9 if fkind[4] == "+" else -1e-9)
                cutA = 3.0
            else:
                phi = {"axis_front": 0.0, "axis_behind": math.pi}.get(fkind, 0.7)
            wv = r * (math.cos(phi) * ah + math.sin(phi) * e)
            if fkind == "apex":
                wv = np.zeros(3)
            if fkind == "perp0":   # exactly on the axis: w and the axis both along z
                a = np.array([0.0, 0.0, 1.0])
                ah = a
                wv = np.array([0.0, 0.0, 0.125])
            Fu["p"][3:6] = a
            Fu["p"][0:3] = rnd(p[b] - wv) if fkind != "perp0" else np.array([p[b, 0], p[b, 1], float(io(p[b, 2] - 0.125))])
            wa = p[b] - Fu["p"][0:3]
            al = float(wa @ ah)
            Pa = float(np.linalg.norm(wa - al * ah))
            phia, da = math.atan2(Pa, al), float(np.linalg.norm(wa))
            if fkind.startswith("cutang") and fkind != "cutang0":
                above = fkind[6] == "+"    # phi / cutAngle = 1 + 1e-6: clipped
                cutA = _fix(phia / (1 + 1e-6 if above else 1 - 1e-6), io, lambda c: (phia > c) if above else (phia < c))
                ordA = ordA or 2.0
            elif fkind == "cutang0":
                cutA = 0.0
            elif fkind.startswith("cutdist"):
                above = fkind[7] == "+"    # |w| = cutDist (1 + 1e-6): cutDist / |w| < 1, not clipped
                cutD = _fix(da / (1 + 1e-6 if above else 1 - 1e-6), io, lambda c: (da > c) if above else (da < c))
                ordD = ordD or 2.0
            Fu["p"][6:10] = [float(io(cutA)), ordA, float(io(cutD)), ordD]
    if sid == "7":   # a second funnel, hemisphere and attractor: regular ones
        i2 = 3 + nrep
        F["id"][:, i2], F["type"][:, i2], F["force"][:, i2] = 3, T_FUN, 5.0
        F["p"][:, i2, :10] = rnd([0.3, 0.2, 0.5, 0.1, 0.2, -0.9, 0.6, 2.5, 0.15, 2.0])
        F["id"][:, i2 + 1], F["type"][:, i2 + 1], F["force"][:, i2 + 1] = 41, T_HEM, -20.0
        F["p"][:, i2 + 1, :8] = rnd([0.0, 0.0, -0.3, 0.02, -0.01, 1.0, 0.05, 5.0])
        F["id"][:, i2 + 2], F["type"][:, i2 + 2], F["force"][:, i2 + 2] = 42, T_ATT, 0.5
        F["p"][:, i2 + 2, :17] = np.roll(F["p"][:, 0, :17], 7, axis=0)   # another arm's goal
        F["p"][:, i2 + 2, 16] = float(io(0.05))
    F["p"] = rnd(F["p"])
    F["force"] = rnd(F["force"])
    return dict(sid=sid, chain=chain, params=params, w=w, pose=pose, probe=probe, rk=rk, hk=hk, fk=fk, slots=(iA, iB, iH, iF),
                max_slots=(4 if not aux else 16), uniform=uniform, io=io)


def kin_key(sc):
    """the scenes of one robot and I/O type share their poses, hence hp_reference's kinematics"""
    return ("field", robot_of(sc["sid"]), np.dtype(sc["io"]).name)


def scene_reference(sc):
    key = ("field", sc["sid"], np.dtype(sc["io"]).name)
    w, prm = sc["w"], sc["params"]
    if sc["probe"]:
        return reference(key, w["fields"], w["nfields"], prm.rot_slowdown, prm.speed_scale, poses=sc["pose"])
    return reference(key, w["fields"], w["nfields"], prm.rot_slowdown, prm.speed_scale, chain=sc["chain"], q=w["q"], kin_key=kin_key(sc))


def _info_of(ref, b, rec_index):
    return ref["info"][b][ref["order"][b].index(rec_index)]


def kind_failures(sc, ref):
    """Every constructed arm against the condition its kind names, from the reference's own quantities.  Returns a list of messages."""
    bad = []
    f64 = sc["io"] == np.float64
    iA, iB, iH, iF = sc["slots"]
    F = sc["w"]["fields"]
    pi8 = math.pi / 8

    def chk(b, kind, cond, what):
        if (f64 or kind not in F64_ONLY) and not cond:
            bad.append("arm %d kind %s: %s" % (b, kind, what))

    for b in range(B_ARMS):
        kind = sc["rk"][b]
        if kind is not None:
            a = _info_of(ref, b, iA)
            D, ratio, order = float(a["D"]), float(a["ratio"]), float(F[b, iA]["p"][5])
            if kind == "floor10":
                chk(b, kind, 0.9e-10 < D < 1.1e-10, "D = %g" % D)
            elif kind == "floor-":
                chk(b, kind, 0.998e-9 < D < 1e-9 and a["D"] < D_FLOOR, "D = %.6g" % D)
            elif kind == "floor+":
                chk(b, kind, 1e-9 < D < 1.002e-9 and a["D"] > D_FLOOR, "D = %.6g" % D)
            elif kind == "D1e-6":
                chk(b, kind, 0.99e-6 < D < 1.01e-6, "D = %g" % D)
            elif kind.startswith("cap"):
                if order > 0:
                    eps = float(kind[3] + "1e-" + kind[4])
                    edge = float(a["rs"]) * 1e6 ** (-1.0 / order)
                    chk(b, kind, a["clipped"] == (eps < 0) and abs(D / edge - 1 - eps) < 0.5 * abs(eps), "clipped %s, D / cap - 1 = %g" % (a["clipped"], D / edge - 1))
                else:
                    chk(b, kind, not a["clipped"], "clipped at order 0")
            elif kind.startswith("ratio"):
                side = float(a["ratio"] - 1)
                chk(b, kind, (side > 0) == (kind[5] == "+") and 0.5e-9 < abs(side) < 2e-9, "ratio - 1 = %g" % side)
            elif kind == "far50":
                chk(b, kind, ratio < 0.0205 and (order < 127 or float(a["m"]) < 1e-200), "ratio %g, m %g" % (ratio, float(a["m"])))
            elif kind == "rs0":
                chk(b, kind, a["rs"] == 0 and (a["m"] == 0) == (order > 0), "radius + safe = %g" % float(a["rs"]))
            elif kind == "force0":
                chk(b, kind, F[b, iA]["force"] == 0.0, "force")
            elif kind == "force+":
                chk(b, kind, F[b, iA]["force"] > 0.0, "force")
            elif kind == "D0":
                chk(b, kind, a["D"] == 0, "D = %g" % D)
            elif kind.startswith("cancel"):
                eps = 1e-3 if kind == "cancel3" else 1e-6
                bq = _info_of(ref, b, iB)
                ta, tb = float(F[b, iA]["force"]) * float(a["m"]), float(F[b, iB]["force"]) * float(bq["m"])
                res = abs(ta - tb) / abs(ta)   # (opposite directions)
                chk(b, kind, not a["clipped"] and not bq["clipped"] and 0.5 * eps < res < 2 * eps, "residual %g" % res)
            elif kind.startswith("goal"):
                g = _info_of(ref, b, 0)
                side = float(g["D"] / g["ds"] - 1)
                chk(b, kind, (side > 0) == (kind[4] == "+") and 0.5e-6 < abs(side) < 1.5e-6 and (g["s0"] < 1) == (side < 0), "D / ds - 1 = %g" % side)
        kind = sc["hk"][b]
        if kind is not None:
            a = _info_of(ref, b, iH)
            order, safe = float(F[b, iH]["p"][7]), float(F[b, iH]["p"][6])
            if kind == "n1e-13":
                chk(b, kind, a["off"], "not switched off")
                continue_h = False
            else:
                chk(b, kind, not a["off"], "switched off")
                continue_h = not a["off"]
            if continue_h:
                h = float(a["h"])
                if kind == "h-0.1":
                    chk(b, kind, -0.11 < h < -0.09 and (a["clipped"] or order == 0), "h = %g" % h)
                elif kind == "h1e-10":
                    chk(b, kind, 0.9e-10 < h < 1.1e-10, "h = %g" % h)
                elif kind == "hfloor-":
                    chk(b, kind, 0.998e-9 < h < 1e-9 and a["h"] < D_FLOOR, "h = %.6g" % h)
                elif kind == "hfloor+":
                    chk(b, kind, 1e-9 < h < 1.002e-9 and a["h"] > D_FLOOR, "h = %.6g" % h)
                elif kind.startswith("hcap"):
                    edge = safe * 1e6 ** (-1.0 / order)
                    eps = 1e-6 if kind[4] == "+" else -1e-6
                    chk(b, kind, a["clipped"] == (eps < 0) and abs(h / edge - 1 - eps) < 5e-7, "clipped %s, h / cap - 1 = %g" % (a["clipped"], h / edge - 1))
                elif kind == "hsafe":
                    chk(b, kind, abs(h / safe - 1) < 1e-6 and not a["clipped"], "h / safe = %g" % (h / safe))
                elif kind == "h50safe":
                    chk(b, kind, abs(h / safe - 50) < 1e-4, "h / safe = %g" % (h / safe))
                elif kind == "h0":
                    chk(b, kind, a["h"] == 0, "h = %g" % h)
                elif kind in ("n3", "n1e-3"):
                    chk(b, kind, abs(float(a["nn"]) / float(kind[1:]) - 1) < 1e-6, "|n| = %g" % float(a["nn"]))
        kind = sc["fk"][b]
        if kind is not None:
            a = _info_of(ref, b, iF)
            phi, P, along, dd = float(a["phi"]), float(a["P"]), float(a["along"]), float(a["dist"])
            cutA, cutD = float(F[b, iF]["p"][6]), float(F[b, iF]["p"][8])
            if kind.startswith("phi"):
                k, plus = int(kind[3]), kind[4] == "+"
                off = float(a["phi"] - k * _num(math.pi) / 8)   # (the double pi / 8: 1e-17 from the boundary, against offsets of 1e-9)
                # the octant of the angle: which of atan2_pos's reductions (steep, upper, x < 0) a correct evaluation takes
                chk(b, kind, (off > 0) == plus and 0.5e-9 < abs(off) < 2e-9 and int(phi / pi8) == (k if plus else k - 1) and not a["ga_clipped"],
                    "phi - k pi/8 = %g" % off)
            elif kind in ("cutang+6", "cutang-6"):
                side = phi / cutA - 1
                chk(b, kind, (side > 0) == (kind[6] == "+") and 0.5e-6 < abs(side) < 1.5e-6 and a["ga_clipped"] == (side > 0), "phi / cutAngle - 1 = %g" % side)
            elif kind in ("cutdist+6", "cutdist-6"):
                side = dd / cutD - 1
                chk(b, kind, (side > 0) == (kind[7] == "+") and 0.5e-6 < abs(side) < 1.5e-6 and a["gd_clipped"] == (side < 0), "|w| / cutDist - 1 = %g" % side)
            elif kind == "axis_front":
                chk(b, kind, P < 1e-9 and along > 0.09, "P = %g along = %g" % (P, along))
            elif kind == "axis_behind":
                chk(b, kind, P < 1e-9 and along < -0.09, "P = %g along = %g" % (P, along))
            elif kind == "apex":
                chk(b, kind, a["dist"] == 0 if sc["probe"] else dd < 1e-9, "|w| = %g" % dd)   # (the probe's pose is given: exactly 0)
            elif kind == "perp0":
                chk(b, kind, a["P"] == 0 and along > 0.1, "P = %g" % P)
            elif kind == "cutang0":
                chk(b, kind, cutA == 0.0 and a["ga_clipped"], "cutAngle = %g" % cutA)
    return bad


def kinds_of(sc, b):
    return "/".join(str(k) for k in (sc["rk"][b], sc["hk"][b], sc["fk"][b]) if k is not None)


def oracle_v6(oc, sc):
    """(v6, status) of the C oracle on a scene: cycle_batch for the cycle scenes, probe_field at the given poses for the probe scenes"""
    w, prm = sc["w"], sc["params"]
    if sc["probe"]:
        return oc.probe_field(prm, w["fields"], w["nfields"], sc["pose"]), np.zeros(B_ARMS, dtype=np.int32)
    out = oc.cycle_batch(sc["chain"], prm, w["q"], w["fields"], w["nfields"], want=("v6", "status"))
    return out["v6"], out["status"]


def oracle_scene(oc, sid, io_dtype):
    """(scene, reference, R): R the C oracle's worst err / E over the scene's held arms"""
    sc = make_scene(oc, sid, io_dtype)
    ref = scene_reference(sc)
    v6, _ = oracle_v6(oc, sc)
    return sc, ref, float(v6_ratio(v6, ref).max())
