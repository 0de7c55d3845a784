"""A high-precision restatement of the whole-arm avoidance command (include/vfik.h: vfik_link_avoid) on hp_links' back end -- 50 digits
with mpmath, numpy.longdouble where mpmath cannot be imported -- and the host's float64 NumPy forms of the same command.

A helper of the suite, not a conftest.py: tests/test_avoid_reference.py holds the host forms to the 50-digit one on the CPU,
tests/test_gpu_link_avoid.py the HIP kernel on the GPU, tests/avoid_reference.py uses the host form inside the oracle-stepped moves.

The command.  From a Chain, spheres (link_i, c_i, r_i), rows of q, rows pts (B, n_rep, 4) = (Q_j, R_j), gain, d0 and scale (B,), every input
taken as the exact double that its I/O-typed value widens to; the pair mask and the NaN-row rule are hp_clearance's:

    P_i   = X_link_i(q_b) c_i                      hp_links.link_frames: the public chain, link 0 the base, link n the flange
    s_ij  = sqrt(|P_i - Q_j|^2),   d_ij = s_ij - r_i - R_j,   a_ij = 1 - d_ij / d0
    ACTIVE iff a_ij > 0 and s_ij > 0
    F_i   = gain scale[b] sum_j a_ij (P_i - Q_j) / s_ij                     over the active pairs
    tau_k = sum over spheres with link_i > k of   z_k . ((P_i - o_k) x F_i)   (revolute k)   or   z_k . F_i   (prismatic k)
            z_k, o_k: third and fourth column of X_k
    a NaN in q[b]: zeros; no active pair: zeros.

`avoid` evaluates in 50 digits only the pairs whose float64 a_ij > -PREFILTER; the others contribute exactly 0 (float64 errs by 1e-13
here, so none of them can be active).

THE UNIT OF ERROR of tau_k, from reading avoid_kernel.  Write g = gain scale[b], R_ij = reach_i + |Q_j| + |R_j| + r_i (the unit of one
clearance, hp_clearance), lever_ik = |P_i - o_k| for link_i > k and 0 otherwise.  Then

    unit_k = n u |g| sum over the pairs with a_ij > -1e-9 and s_ij > 0 of   R_ij ( (1 / d0 + a+_ij / s_ij) lever_ik + a+_ij ),   a+ = max(a, 0)

  * the walk: P_i, z_k and o_k are link_kernel's frames, off by O(n) u reach; so d_ij is off by n u R_ij (hp_clearance's derivation), hence
    a_ij by n u R_ij / d0 -- the 1 / d0 sensitivity -- and the direction (P_i - Q_j) / s_ij by n u R_ij / s_ij, which a_ij scales: the
    a_ij / s_ij sensitivity.  A pair within that error of the edge a = 0 may be switched either way: the law is continuous there, the
    switch costs no more than the first term, which is why pairs down to a = -1e-9 carry it.
  * the kernel uses ONE computed F_i in T_F, T_N and both prefix sums, and z . (P x F) - (z x o) . F = z . ((P - o) x F) holds for any F: the
    error of F_i reaches tau_k times the LEVER |P_i - o_k|, not times |P_i| and |o_k| apiece.
  * what does not cancel is the rounding of the one-pass form itself: P_i x F_i, m_k = z_k x o_k, their dot products, the running sums and
    the final bracket each round at u (|P_i| + |o_k|) |F_i| <= u R_ij |g| a_ij per pair -- the last term, without a lever.  It is carried
    by EVERY sphere, also those with link_i <= k whose share of the totals is subtracted again as the prefix.
  * the output's own rounding is not in the unit: THE BAR is K_MARGIN units beyond the output's half ulp.
An arm without such a pair has unit 0: its row must be exactly zero."""
import numpy as np

import hp_clearance as hc
import hp_links as hl
import hp_reference as hp
from vfclik_amd.chain import Chain

U = hp.U
K_MARGIN = hp.K_MARGIN
PREFILTER = 1e-6
EDGE = 1e-9


def host_frames(chain, q):
    """(Z, O): (B, n, 3) each, the joint axis z_k and the origin o_k of X_k in float64 -- Chain.fk of the truncated chains, as
    hp_links.host_points"""
    q = np.asarray(q, dtype=np.float64)
    B, n = q.shape[0], chain.n
    Z, O = np.empty((B, n, 3)), np.empty((B, n, 3))
    for k in range(n):
        X = np.tile(np.vstack([chain.B[0], [0, 0, 0, 1]]), (B, 1, 1)) if k == 0 else hl.truncated(chain, k).fk(q[:, :k])
        Z[:, k], O[:, k] = X[:, :3, 2], X[:, :3, 3]
    return Z, O


def _pairs(chain, spheres, q, pts, first, count, mask, gain, d0, scale):
    """what the float64 forms share: own (B, L, 4), rows, use, diff, s, a, on (B, L, count), F (B, L, 3), g (B,), bad (B,)"""
    q = np.asarray(q, dtype=np.float64)
    pts = np.asarray(pts, dtype=np.float64)
    B, L = q.shape[0], len(spheres)
    rows, use = hc._considered(pts, first, count, mask, L)
    bad = np.isnan(q).any(axis=1)
    own = hl.host_points(chain, spheres, np.where(bad[:, None], 0.0, q))
    g = float(gain) * (np.ones(B) if scale is None else np.asarray(scale, dtype=np.float64))
    with np.errstate(invalid="ignore", divide="ignore"):
        diff = own[:, :, None, :3] - rows[:, None, :, :3]
        s = np.sqrt((diff * diff).sum(axis=3))
        a = 1.0 - (s - own[:, :, None, 3] - rows[:, None, :, 3]) / float(d0)
        on = use & (a > 0.0) & (s > 0.0)
        w = np.where(on, a / np.where(on, s, 1.0), 0.0)
    F = g[:, None, None] * (w[..., None] * np.where(on[..., None], diff, 0.0)).sum(axis=2)
    return dict(q=np.where(bad[:, None], 0.0, q), own=own, rows=rows, use=use, diff=diff, s=s, a=a, on=on, F=F, g=g, bad=bad)


def host_avoid(chain, spheres, q, pts, first=0, count=None, mask=None, gain=1.0, d0=0.1, scale=None, detail=False):
    """The host's float64 form, the law as it is written: every sphere's F_i through the Jacobian transpose of its own point.  Returns
    tau (B, n) float64, not rounded (with detail=True: also the dict of _pairs)."""
    pts = np.asarray(pts, dtype=np.float64)
    count = pts.shape[1] - first if count is None else count
    p = _pairs(chain, spheres, q, pts, first, count, mask, gain, d0, scale)
    Z, O = host_frames(chain, p["q"])
    links = np.array([s[0] for s in spheres])
    tau = np.zeros((p["q"].shape[0], chain.n))
    for k in range(chain.n):
        beyond = links > k
        if not beyond.any():
            continue
        P, F = p["own"][:, beyond, :3], p["F"][:, beyond]
        if chain.jtype[k] == 0:
            tau[:, k] = np.einsum("bj,bij->b", Z[:, k], np.cross(P - O[:, None, k], F))
        else:
            tau[:, k] = np.einsum("bj,bij->b", Z[:, k], F)
    tau[p["bad"] | ~p["on"].any(axis=(1, 2))] = 0.0
    return (tau, p) if detail else tau


def walk_avoid(chain, spheres, q, pts, first=0, count=None, mask=None, gain=1.0, d0=0.1, scale=None):
    """The kernel's one-pass form in float64 NumPy: totals T_F, T_N, and per joint z_k, m_k = z_k x o_k and the prefix bracket c_k.  The
    same F_i as host_avoid: what differs is the algebra behind them."""
    pts = np.asarray(pts, dtype=np.float64)
    count = pts.shape[1] - first if count is None else count
    p = _pairs(chain, spheres, q, pts, first, count, mask, gain, d0, scale)
    Z, O = host_frames(chain, p["q"])
    B, n = p["q"].shape[0], chain.n
    TF, TN = np.zeros((B, 3)), np.zeros((B, 3))
    M, Cb = np.empty((B, n, 3)), np.empty((B, n))
    for i in range(n + 1):
        for j, sp in enumerate(spheres):
            if sp[0] == i:
                TF = TF + p["F"][:, j]
                TN = TN + np.cross(p["own"][:, j, :3], p["F"][:, j])
        if i < n:
            M[:, i] = np.cross(Z[:, i], O[:, i])
            zf, zn, mf = (Z[:, i] * TF).sum(axis=1), (Z[:, i] * TN).sum(axis=1), (M[:, i] * TF).sum(axis=1)
            Cb[:, i] = zn - mf if chain.jtype[i] == 0 else zf
    tau = np.empty((B, n))
    for k in range(n):
        zf, zn, mf = (Z[:, k] * TF).sum(axis=1), (Z[:, k] * TN).sum(axis=1), (M[:, k] * TF).sum(axis=1)
        tau[:, k] = (zn - mf if chain.jtype[k] == 0 else zf) - Cb[:, k]
    tau[p["bad"] | ~p["on"].any(axis=(1, 2))] = 0.0
    return tau


def _sqrt(x):
    return x.sqrt() if hp.BACKEND == "mpmath" else np.sqrt(x)


def avoid(chain, spheres, q, pts, first=0, count=None, mask=None, gain=1.0, d0=0.1, scale=None):
    """The 50-digit form.  Returns a dict: hi, lo (B, n) with hi + lo the command; unit (B, n), 0 for an arm that must be exactly zero;
    active (B,): the arm has an active pair in 50 digits."""
    pts = np.asarray(pts, dtype=np.float64)
    count = pts.shape[1] - first if count is None else count
    _tau, p = host_avoid(chain, spheres, q, pts, first, count, mask, gain, d0, scale, detail=True)
    B, L, n = p["q"].shape[0], len(spheres), chain.n
    num = lambda x: hp._num(float(x))
    hi, lo, active = np.zeros((B, n)), np.zeros((B, n)), np.zeros(B, dtype=bool)
    with np.errstate(invalid="ignore"):
        cand = p["use"] & (p["a"] > -PREFILTER)
    D0 = num(d0)
    for b in range(B):
        if p["bad"][b] or not cand[b].any():
            continue
        frames = hl.link_frames(chain, p["q"][b])
        G = num(gain) * (num(1.0) if scale is None else num(np.asarray(scale, dtype=np.float64)[b]))
        force = []
        for i in np.flatnonzero(cand[b].any(axis=1)):
            link, c, r = spheres[i]
            P = hl._apply(frames[link], [num(x) for x in c])
            F = [num(0.0)] * 3
            for j in np.flatnonzero(cand[b, i]):
                Q = [num(x) for x in p["rows"][b, j, :3]]
                df = [P[t] - Q[t] for t in range(3)]
                s = _sqrt(df[0] * df[0] + df[1] * df[1] + df[2] * df[2])
                a = num(1.0) - (s - num(r) - num(p["rows"][b, j, 3])) / D0
                if a > 0 and s > 0:
                    active[b] = True
                    F = [F[t] + a * df[t] / s for t in range(3)]
            force.append((link, P, [G * f for f in F]))
        if not active[b]:
            continue
        for k in range(n):
            z = [frames[k][t][2] for t in range(3)]
            o = [frames[k][t][3] for t in range(3)]
            tau = num(0.0)
            for link, P, F in force:
                if link <= k:
                    continue
                if chain.jtype[k] == 0:
                    v = [P[t] - o[t] for t in range(3)]
                    x = [v[1] * F[2] - v[2] * F[1], v[2] * F[0] - v[0] * F[2], v[0] * F[1] - v[1] * F[0]]
                    tau = tau + z[0] * x[0] + z[1] * x[1] + z[2] * x[2]
                else:
                    tau = tau + z[0] * F[0] + z[1] * F[1] + z[2] * F[2]
            hi[b, k] = float(tau)
            lo[b, k] = float(tau - num(hi[b, k]))
    return dict(hi=hi, lo=lo, unit=unit(chain, spheres, p, d0), active=active)


def unit(chain, spheres, p, d0):
    """the error unit (B, n) of the module's docstring, from the float64 quantities of _pairs"""
    B, L, n = p["q"].shape[0], len(spheres), chain.n
    Z, O = host_frames(chain, p["q"])
    links = np.array([s[0] for s in spheres])
    with np.errstate(invalid="ignore", divide="ignore"):
        S = p["use"] & (p["a"] > -EDGE) & (p["s"] > 0.0)                                     # (B, L, count)
        ap = np.where(S, np.maximum(p["a"], 0.0), 0.0)
        R = np.where(S, hl.reach(chain, spheres)[None, :, None] + np.linalg.norm(p["rows"][:, None, :, :3], axis=3)
                     + np.abs(p["rows"][:, None, :, 3]) + p["own"][:, :, None, 3], 0.0)
        sens = np.where(S, 1.0 / float(d0) + ap / np.where(S, p["s"], 1.0), 0.0)
    lever = np.linalg.norm(p["own"][:, :, None, :3] - O[:, None, :, :], axis=3) * (links[None, :, None] > np.arange(n)[None, None, :])   # (B, L, n)
    u = (R * sens).sum(axis=2)[:, :, None] * lever + (R * ap).sum(axis=2)[:, :, None]
    u = n * U * np.abs(p["g"])[:, None] * u.sum(axis=1)
    u[p["bad"]] = 0.0
    return u


def bar(ref, io_dtype):
    """(B, n): K_MARGIN units beyond half an ulp of the output type at the reference"""
    return K_MARGIN * ref["unit"] + 0.5 * np.spacing(np.abs(ref["hi"]).astype(io_dtype)).astype(np.float64)


def error(got, ref):
    return np.abs((np.asarray(got, dtype=np.float64) - ref["hi"]) - ref["lo"])


def worst_units(got, ref, io_dtype):
    """the largest error, less the output's half ulp, in units -- over the elements with a unit"""
    e = np.maximum(error(got, ref) - 0.5 * np.spacing(np.abs(ref["hi"]).astype(io_dtype)).astype(np.float64), 0.0)
    has = ref["unit"] > 0
    return float((e[has] / ref["unit"][has]).max()) if has.any() else 0.0


# ---- the cases the host test and the GPU test share ---------------------------------------------------------------------------------
CASES = hc.CASES       # (batch, sphere list, count, first, rows): batches 1 / 65 / 203, counts 1 / 5 / 16 / 32, partner / own / static rows
GAIN = 0.75
S_MIN = 1e-3


def make_case(robot, io_dtype, B, kind, count, first, rows, place=None, seed=11):
    """hp_clearance.make_case (the rows outside the window sit AT the arm's first sphere with radius 1: read, they would push hard) with
    the law's parameters beside it: gain, scale -- random in [0.5, 1.5], I/O-typed, None in the partner cases -- and d0, chosen from the
    arms' float64 clearances so that at least a third of the arms have an active pair and at least one has none (a batch of one arm
    cannot have both: its arm has an active pair).  Asserts s_ij >= S_MIN for every considered pair: no pair near the one discontinuity
    of the law, so nothing is left out of the comparison."""
    c = hc.make_case(robot, io_dtype, B, kind, count, first, rows, place=place, seed=seed)
    clear, _pair, _d = hc.host_clearance(c["chain"], c["spheres"], c["q"], c["pts"], first, count, c["mask"])
    fin = np.sort(clear[np.isfinite(clear)])
    assert fin.size >= 1, "no arm with a pair"
    if B == 1:
        d0 = abs(float(fin[0])) + 0.0625
    else:
        d0 = None
        for k in range(max((B + 2) // 3, B // 2), B):          # k arms active, the others not
            hi_k = fin[k] if k < fin.size else fin[-1] + 1.0    # (arms without a pair at all are never active)
            mid = 0.5 * (fin[k - 1] + hi_k) if k - 1 < fin.size else None
            if mid is not None and mid > 1e-3 and hi_k - fin[k - 1] > 1e-6:
                d0 = float(mid)
                break
        assert d0 is not None, "no d0 leaves an arm without an active pair"
    c["gain"], c["d0"] = GAIN, d0
    c["scale"] = None if rows == "partner" else np.random.default_rng(seed + 7).uniform(0.5, 1.5, size=B).astype(io_dtype).astype(np.float64)
    p = _pairs(c["chain"], c["spheres"], c["q"], c["pts"], first, count, c["mask"], GAIN, d0, c["scale"])
    assert np.all(p["s"][p["use"] & ~p["bad"][:, None, None]] >= S_MIN)
    n_on = int(p["on"].any(axis=(1, 2)).sum())
    assert 3 * n_on >= B and (B == 1 or n_on < B), (n_on, B)
    return c


def call_args(c):
    """the case as keyword arguments of host_avoid / avoid / Engine.link_avoid_host's tail"""
    return dict(first=c["first"], count=c["count"], mask=c["mask"], gain=c["gain"], d0=c["d0"], scale=c["scale"])


_HOST = {}


def host_case(robot, io_dtype, case):
    """(case, 50-digit reference, host form) of a case of CASES on host-placed rows -- computed once"""
    key = (robot, np.dtype(io_dtype).name) + tuple(case)
    if key not in _HOST:
        c = make_case(robot, io_dtype, *case)
        _HOST[key] = (c, avoid(c["chain"], c["spheres"], c["q"], c["pts"], **call_args(c)),
                      host_avoid(c["chain"], c["spheres"], c["q"], c["pts"], **call_args(c)))
    return _HOST[key]


# ---- the edge cases --------------------------------------------------------------------------------------------------------------------
EDGE_ARMS = ("at_d0", "penetrating", "coincident", "nan_q", "scale_zero", "prismatic_tail", "no_rows", "general")
EDGE_D0 = 0.375


def edge_chain():
    """six joints, the last two prismatic (an all-prismatic tail), an identity base; every B[i] a quarter turn or none and a translation of
    binary fractions, so that at q = 0 every frame is exact in float32 already"""
    rx = np.array([[1.0, 0, 0], [0, 0, -1.0], [0, 1.0, 0]])
    ry = np.array([[0, 0, 1.0], [0, 1.0, 0], [-1.0, 0, 0]])
    eye = np.eye(3)
    parts = ((eye, (0, 0, 0)), (rx, (0, 0, 0.25)), (ry, (0.25, 0, 0)), (rx, (0, 0, 0.5)), (eye, (0, 0.25, 0)), (ry, (0, 0, 0.125)), (eye, (0.125, 0, 0)))
    B = [np.hstack([r, np.array(t, dtype=np.float64)[:, None]]) for r, t in parts]
    return Chain(B, [0, 0, 0, 0, 1, 1], [-2.5] * 4 + [-0.2] * 2, [2.5] * 4 + [0.3] * 2, name="edge6")


def edge_case(io_dtype, place=None):
    """One batch of len(EDGE_ARMS) arms on edge_chain(), three spheres -- link 0 at the base's origin, link 3, link n behind the prismatic
    tail -- and three rows per arm, d0 = EDGE_D0:
      at_d0           q = 0: row 0 sits 0.5 from sphere 1 along x, both radii 0.0625: d = 0.375 = d0 EXACTLY, a = 0, no push; row 1 sits
                      0.25 from it along y and pushes (the builder asserts both in the float64 form, which is exact at q = 0)
      penetrating     row 0 sits 0.03 from sphere 1: d < 0, a > 1
      coincident      row 0 at the very coordinates of sphere 0 (link 0, identity base, centre 0): s = 0 exactly, contributes nothing; the
                      other spheres meet that row at a distance: the row is finite
      nan_q           penetrating's rows and a NaN in q: zeros
      scale_zero      penetrating's rows and scale = 0: zeros
      prismatic_tail  row 0 sits close to sphere 2, on link n: the two prismatic joints are pushed along their axes
      no_rows         every row NaN: zeros
      general         three random rows"""
    chain = edge_chain()
    n, B = chain.n, len(EDGE_ARMS)
    spheres = [(0, (0.0, 0.0, 0.0), 0.0625), (3, (0.25, 0.0, 0.125), 0.0625), (n, (0.0, 0.125, 0.0), 0.03125)]
    rnd = lambda a: np.asarray(a, dtype=np.float64).astype(io_dtype).astype(np.float64)
    rng = np.random.default_rng(77)
    q = rnd(rng.uniform(0.8 * chain.q_lo, 0.8 * chain.q_hi, size=(B, n)))
    q[0] = 0.0
    q[EDGE_ARMS.index("nan_q")] = q[EDGE_ARMS.index("scale_zero")] = q[1]
    place = place or (lambda qq, src, x: hl.host_points(chain, spheres, qq, src, x).astype(io_dtype).astype(np.float64))
    own = place(q, None, None)
    pts = np.full((B, 3, 4), np.nan)
    pts[0, 0] = np.append(own[0, 1, :3] + (0.5, 0, 0), 0.0625)
    pts[0, 1] = np.append(own[0, 1, :3] + (0, 0.25, 0), 0.0625)
    for name in ("penetrating", "nan_q", "scale_zero"):
        pts[EDGE_ARMS.index(name), 0] = np.append(own[1, 1, :3] + (0.03, 0, 0), 0.0625)
    pts[2, 0] = (0.0, 0.0, 0.0, 0.0625)
    pts[2, 1] = np.append(own[2, 1, :3] + (0.125, 0, 0), 0.0625)   # (and a row that does push, so that the arm's command is not all zero)
    b = EDGE_ARMS.index("prismatic_tail")
    pts[b, 0] = np.append(own[b, 2, :3] + (0.05, 0.02, -0.01), 0.03125)
    b = EDGE_ARMS.index("general")
    pts[b] = np.concatenate([own[b, :, :3] + rng.uniform(-0.2, 0.2, size=(3, 3)), rng.uniform(0.02, 0.1, size=(3, 1))], axis=1)
    pts = rnd(pts)
    q[EDGE_ARMS.index("nan_q"), 2] = np.nan
    scale = np.ones(B)
    scale[EDGE_ARMS.index("scale_zero")] = 0.0
    scale[EDGE_ARMS.index("general")] = 0.5
    c = dict(chain=chain, spheres=spheres, q=q, pts=pts, first=0, count=3, mask=None, gain=GAIN, d0=EDGE_D0, scale=scale)
    p = _pairs(chain, spheres, q, pts, 0, 3, None, GAIN, EDGE_D0, scale)
    assert p["a"][0, 1, 0] == 0.0 and not p["on"][0, 1, 0] and p["on"][0, 1, 1], "at_d0: the pair is not exactly at d0"
    assert p["a"][1, 1, 0] > 1.0 and p["s"][2, 0, 0] == 0.0 and p["on"][2].any()
    assert p["on"][EDGE_ARMS.index("prismatic_tail"), 2, 0]
    return c
