"""A high-precision restatement of the link points (include/vfik.h: vfik_link_points) on hp_reference's back end -- 50 digits with mpmath,
numpy.longdouble with a 64-bit mantissa where mpmath cannot be imported -- and the host's float64 form of the same points.

A helper of the suite, not a conftest.py: tests/test_links_host.py holds Chain.fk to it on the CPU, tests/test_gpu_link_points.py the HIP
kernel on the GPU.

The reference.  From a Chain, spheres (link, centre, radius), rows of q, src_arm and xform, every input taken as the exact double that its
I/O-typed value widens to:

    X_0 = B[0],   X_i = X_{i-1} Jz(q_s[i-1]) B[i]        hp_reference's _frame, _mul and the joint step of its _fk_jac
    P   = X_link c        and with a transform     P <- R_b P + t_b,   xform[b] = [R_b | t_b] row-major 3 x 4

for s = src_arm[b] (None: b).  An arm whose source lies outside the batch, or whose source's q row holds a NaN, has NaN rows.  Results are
pairs of doubles (hi, lo) with hi + lo the high-precision value, as hp_reference returns them.

The unit of error of a coordinate is n u reach, u = 2^-53, reach = sum_i |p(B_i)| + |c| (+ |t_b| with a transform): every product of the
walk moves a point by at most that much, and there are O(n) of them.

`host_points` are the points a caller computes on the host today: Chain.fk of the chain TRUNCATED at the sphere's link (link 0: B[0] itself),
times c, through the transform, all in float64."""
import numpy as np

import hp_reference as hp
from vfclik_amd.chain import Chain

U = hp.U
K_MARGIN = hp.K_MARGIN


def link_frames(chain, q):
    """one arm: [X_0 .. X_n], 3 x 4 frames in the high-precision type"""
    X = hp._frame(chain.B[0])
    out = [X]
    for i in range(chain.n):
        X = [row[:] for row in X]
        qi = hp._num(float(q[i]))
        if chain.jtype[i] == 0:   # X Jz(q): columns 0 and 1 turn (hp_reference._fk_jac)
            c, s = hp._cos(qi), hp._sin(qi)
            for r in range(3):
                X[r][0], X[r][1] = X[r][0] * c + X[r][1] * s, X[r][1] * c - X[r][0] * s
        else:                     # a shift along z
            for r in range(3):
                X[r][3] = X[r][3] + X[r][2] * qi
        X = hp._mul(X, hp._frame(chain.B[i + 1]))
        out.append(X)
    return out


def _apply(X, p):
    return [X[r][0] * p[0] + X[r][1] * p[1] + X[r][2] * p[2] + X[r][3] for r in range(3)]


def link_points(chain, spheres, q, src_arm=None, xform=None):
    """(hi, lo): two float64 arrays (B, L, 3), NaN rows for an arm without a source or with a NaN in its source's q row"""
    q = np.asarray(q, dtype=np.float64)
    B, L = q.shape[0], len(spheres)
    hi, lo = np.full((B, L, 3), np.nan), np.full((B, L, 3), np.nan)
    frames = {}
    for b in range(B):
        s = b if src_arm is None else int(src_arm[b])
        if s < 0 or s >= B or np.isnan(q[s]).any():
            continue
        if s not in frames:
            frames[s] = link_frames(chain, q[s])
        T = None if xform is None else hp._frame(np.asarray(xform, dtype=np.float64).reshape(B, 3, 4)[b])
        for j, (link, c, _r) in enumerate(spheres):
            P = _apply(frames[s][link], [hp._num(float(x)) for x in c])
            if T is not None:
                P = _apply(T, P)
            for k in range(3):
                hi[b, j, k] = float(P[k])
                lo[b, j, k] = float(P[k] - hp._num(hi[b, j, k]))
    return hi, lo


def reach(chain, spheres, xform=None, B=None):
    """(B, L) or (L,): sum_i |p(B_i)| + |c| (+ |t_b|), the length scale of a sphere's coordinates"""
    links = sum(float(np.linalg.norm(chain.B[i][:, 3])) for i in range(chain.n + 1))
    r = np.array([links + float(np.linalg.norm(c)) for _l, c, _r in spheres])
    if xform is None:
        return r
    t = np.linalg.norm(np.asarray(xform, dtype=np.float64).reshape(-1, 3, 4)[:, :, 3], axis=1)
    return r[None, :] + t[:, None]


def error_units(got, ref, chain, spheres, xform=None):
    """|got - (hi + lo)| / (n u reach) per coordinate, (B, L, 3); NaN where the reference is NaN"""
    hi, lo = ref
    r = reach(chain, spheres, xform)
    r = r[None, :, None] if r.ndim == 1 else r[:, :, None]
    with np.errstate(invalid="ignore"):
        return np.abs((np.asarray(got, dtype=np.float64) - hi) - lo) / (chain.n * U * r)


def truncated(chain, link):
    """the chain's first `link` joints: its flange is X_link (link >= 1)"""
    return Chain(chain.B[: link + 1], chain.jtype[:link], chain.q_lo[:link], chain.q_hi[:link], name="%s[:%d]" % (chain.name, link))


def host_points(chain, spheres, q, src_arm=None, xform=None):
    """(B, L, 4) float64 = x y z radius: what a caller computes on the host today.  NaN rows (radius included) for an arm without a
    source or with a NaN in its source's q row."""
    q = np.asarray(q, dtype=np.float64)
    B, L = q.shape[0], len(spheres)
    src = np.arange(B) if src_arm is None else np.asarray(src_arm, dtype=np.int64)
    ok = (src >= 0) & (src < B)
    qs = q[np.where(ok, src, 0)]
    ok &= ~np.isnan(qs).any(axis=1)
    qs = np.where(ok[:, None], qs, 0.0)
    out = np.full((B, L, 4), np.nan)
    fk = {}
    for j, (link, c, r) in enumerate(spheres):
        if link not in fk:
            fk[link] = np.tile(np.vstack([chain.B[0], [0, 0, 0, 1]]), (B, 1, 1)) if link == 0 else truncated(chain, link).fk(qs[:, :link])
        P = fk[link][:, :3, :3] @ np.asarray(c, dtype=np.float64) + fk[link][:, :3, 3]
        if xform is not None:
            T = np.asarray(xform, dtype=np.float64).reshape(B, 3, 4)
            P = np.einsum("bij,bj->bi", T[:, :, :3], P) + T[:, :, 3]
        out[:, j, :3] = P
        out[:, j, 3] = r
    out[~ok] = np.nan
    return out


# ---- the cases the host test and the GPU test share ---------------------------------------------------------------------------------
ROBOTS = ("powercube6", "lwr", "lwr_dual14", "mixed10")
SPHERE_LISTS = ("one", "five", "all16")
SOURCES = ("self", "pair", "zero", "mix")
# (sphere list, sources, with a transform): every list, every kind of source and both transform settings at least once per chain and I/O type
CASES = (("one", "self", False), ("five", "pair", True), ("five", "mix", False), ("all16", "zero", False), ("all16", "mix", True))


def _rot(axis, angle):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def chain_of(robot):
    """the three robots of vfclik_amd.robots, and `mixed10`: ten joints, two of them prismatic, axes all over, a base that is no identity"""
    if robot != "mixed10":
        return hp.chain_of(robot)
    rng = np.random.default_rng(1010)
    segs, lo, hi = [], [], []
    for i in range(10):
        prismatic = i in (3, 7)
        tip = np.eye(4)
        tip[:3, :3] = _rot(rng.normal(size=3), rng.uniform(-1.5, 1.5))
        tip[:3, 3] = rng.uniform(-0.25, 0.25, size=3)
        segs.append((1 if prismatic else 0, rng.normal(size=3), tip))
        lo.append(-0.2 if prismatic else -2.5)
        hi.append(0.3 if prismatic else 2.5)
    base = np.eye(4)
    base[:3, :3] = _rot([1.0, -2.0, 0.5], 0.7)
    base[:3, 3] = [0.3, -0.1, 0.4]
    return Chain.from_segments(segs, lo, hi, base=base, name="mixed10")


def sphere_list(chain, kind):
    """one: a single sphere on link 0 with c != 0 (a constant point through the base frame); five: unsorted, two spheres on one link;
    all16: sixteen spheres, every link 0..n used, unsorted"""
    n = chain.n
    if kind == "one":
        return [(0, (0.1, -0.2, 0.3), 0.05)]
    rng = np.random.default_rng(16 + n)
    if kind == "five":
        links = [n, 2, 4, 2, 1]
    else:
        assert kind == "all16"
        links = list(range(n + 1)) + [int(x) for x in rng.integers(0, n + 1, size=16 - (n + 1))]
        links = [links[i] for i in rng.permutation(16)]
    return [(l, tuple(rng.uniform(-0.15, 0.15, size=3)), float(rng.uniform(0.03, 0.09))) for l in links]


def sources(kind, B):
    """self: NULL; pair: b ^ 1 (the last arm of an odd batch has a partner outside it); zero: arm 0 for everybody; mix: own, partner, -1 and
    B by turns"""
    b = np.arange(B, dtype=np.int32)
    if kind == "self":
        return None
    if kind == "pair":
        return b ^ 1
    if kind == "zero":
        return np.zeros(B, dtype=np.int32)
    assert kind == "mix"
    return np.select([b % 4 == 0, b % 4 == 1, b % 4 == 2], [b, np.minimum(b ^ 1, B - 1), -1], B).astype(np.int32)


def inputs(chain, B, io_dtype, seed=5):
    """(q (B, n), xform (B, 12)): joint angles in 0.8 of the limits and a rotation plus a translation per arm, rounded to the I/O type"""
    rng = np.random.default_rng(seed)
    q = rng.uniform(0.8 * chain.q_lo, 0.8 * chain.q_hi, size=(B, chain.n))
    x = np.zeros((B, 3, 4))
    for b in range(B):
        x[b, :, :3] = _rot(rng.normal(size=3), rng.uniform(-np.pi, np.pi))
        x[b, :, 3] = rng.uniform(-1.0, 1.0, size=3)
    rnd = lambda a: a.astype(io_dtype).astype(np.float64)
    return rnd(q), rnd(x.reshape(B, 12))


_HOST_RATIO = {}


def host_ratio(robot, kind, src_kind, with_xform, B, io_dtype):
    """R of a case: the host's worst error (host_points against the 50-digit points) in units, with the reference it was measured
    against -- computed once per case."""
    key = (robot, kind, src_kind, with_xform, B, np.dtype(io_dtype).name)
    if key not in _HOST_RATIO:
        chain = chain_of(robot)
        sp = sphere_list(chain, kind)
        q, x = inputs(chain, B, io_dtype)
        src = sources(src_kind, B)
        x = x if with_xform else None
        ref = link_points(chain, sp, q, src, x)
        host = host_points(chain, sp, q, src, x)
        assert np.array_equal(np.isnan(host[:, :, 0]), np.isnan(ref[0][:, :, 0]))
        _HOST_RATIO[key] = (float(np.nanmax(error_units(host[:, :, :3], ref, chain, sp, x))), ref)
    return _HOST_RATIO[key]
