"""A high-precision restatement of the link-sphere clearance (include/vfik.h: vfik_link_clearance) on hp_links' back end -- 50 digits with
mpmath, numpy.longdouble where mpmath cannot be imported -- and the host's float64 form of the same measurement.

A helper of the suite, not a conftest.py: tests/test_clearance_reference.py holds the host form to the 50-digit one on the CPU,
tests/test_gpu_link_clearance.py the HIP kernel on the GPU, tests/clearance_reference.py uses the host form inside the oracle-stepped moves.

The measurement.  From a Chain, spheres (link, centre, radius), rows of q and rows pts (B, n_rep, 4) = x y z radius, every input taken as
the exact double that its I/O-typed value widens to:

    P_i  = X_link_i(q_b) c_i                          hp_links.link_frames: the public chain, link 0 the base, link n the flange
    d_ij = sqrt(|P_i - Q_j|^2) - r_i - R_j            row j counted from `first`, j < count
    clear[b] = min d_ij,   pair[b] = i * 32 + j       over the pairs with bit j of mask[i] set (mask None: all) whose row holds no NaN;
                                                      ties take the smallest code; no pair: +inf and -1; a NaN in q[b]: NaN and -1

The unit of error of a clearance is  n u (reach_i + |Q_j| + R_j + r_i)  of the minimising pair, u = 2^-53, reach_i = hp_links.reach.
Derivation, from reading clear_kernel: P_i is link_kernel's walk, whose coordinates err by O(n) u reach_i (hp_links); Q_j, R_j and r_i are
exact; each coordinate difference rounds once, u (|P| + |Q|) <= u (reach_i + |Q_j|); the sum of three squares (two fmas) and the square
root keep a relative error of about 2 u on a length that is at most reach_i + |Q_j|; the two subtractions round once each on values below
reach_i + |Q_j| + r_i + R_j.  Every term is a small multiple of u times a summand of the unit, and there are fewer than n of them beside
the walk's own: no term is missing.

`clearance` does not evaluate all L x count pairs of an arm in 50 digits: a pair whose float64 d_ij lies more than PREFILTER above the
float64 minimum cannot be the minimum (float64 errs by 1e-13 here), so only the others are; `second`, the runner-up, takes the float64
value where it lies that far off."""
import numpy as np

import hp_links as hl
import hp_reference as hp

U = hp.U
K_MARGIN = hp.K_MARGIN
PREFILTER = 1e-6


def _sqrt(x):
    return x.sqrt() if hp.BACKEND == "mpmath" else np.sqrt(x)


def mask_matrix(mask, L, count):
    """(L, count) bool from L words (bit j of word i), None: every pair"""
    if mask is None:
        return np.ones((L, count), dtype=bool)
    m = np.asarray(mask, dtype=np.uint64)
    assert m.shape == (L,)
    return ((m[:, None] >> np.arange(count, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(bool)


def mask_words(matrix):
    """L uint32 words from an (L, count) bool matrix"""
    m = np.asarray(matrix, dtype=bool)
    return (m.astype(np.uint64) << np.arange(m.shape[1], dtype=np.uint64)[None, :]).sum(axis=1).astype(np.uint32)


def _considered(pts, first, count, mask, L):
    rows = np.asarray(pts, dtype=np.float64)[:, first:first + count]
    ok = ~np.isnan(rows).any(axis=2)                                   # (B, count)
    return rows, ok[:, None, :] & mask_matrix(mask, L, count)[None]    # (B, L, count)


def host_clearance(chain, spheres, q, pts, first=0, count=None, mask=None):
    """The host's float64 form: Chain.fk of the truncated chains (hp_links.host_points) and NumPy.  Returns (clear (B,) float64, not
    rounded; pair (B,) int32; d (B, L, count) with +inf where the pair is not considered, NaN rows for an arm with a NaN in q)."""
    q = np.asarray(q, dtype=np.float64)
    pts = np.asarray(pts, dtype=np.float64)
    B, L = q.shape[0], len(spheres)
    count = pts.shape[1] - first if count is None else count
    rows, use = _considered(pts, first, count, mask, L)
    own = hl.host_points(chain, spheres, q)                            # (B, L, 4), NaN rows for a NaN in q
    bad = np.isnan(q).any(axis=1)
    with np.errstate(invalid="ignore"):
        diff = own[:, :, None, :3] - rows[:, None, :, :3]
        d = np.sqrt((diff * diff).sum(axis=3)) - own[:, :, None, 3] - rows[:, None, :, 3]
    d = np.where(use, d, np.inf)
    flat = d.reshape(B, L * count)
    k = np.argmin(np.where(np.isnan(flat), np.inf, flat), axis=1)     # the first minimum in (i, j) order is the smallest code
    clear = flat[np.arange(B), k]
    pair = np.where(use.reshape(B, -1)[np.arange(B), k], (k // count) * 32 + k % count, -1)   # (nothing considered: k = 0, not in use)
    clear = np.where(bad, np.nan, clear)
    pair = np.where(bad, -1, pair).astype(np.int32)
    d[bad] = np.nan
    return clear, pair, d


def clearance(chain, spheres, q, pts, first=0, count=None, mask=None):
    """The 50-digit form.  Returns a dict of (B,) arrays: hi, lo (hi + lo the minimum; +inf / 0 without a pair, NaN for a NaN in q), pair
    (int32), second (the smallest d_ij of a pair whose d_ij differs from the minimum, +inf without one: what the kernel could mistake
    the minimum for), unit (the error unit of the minimising pair, NaN without one)."""
    q = np.asarray(q, dtype=np.float64)
    pts = np.asarray(pts, dtype=np.float64)
    B, L, n = q.shape[0], len(spheres), chain.n
    count = pts.shape[1] - first if count is None else count
    rows, use = _considered(pts, first, count, mask, L)
    _c64, _p64, d64 = host_clearance(chain, spheres, q, pts, first, count, mask)
    reach = hl.reach(chain, spheres)
    hi, lo = np.full(B, np.inf), np.zeros(B)
    pair, second, unit = np.full(B, -1, dtype=np.int32), np.full(B, np.inf), np.full(B, np.nan)
    for b in range(B):
        if np.isnan(q[b]).any():
            hi[b] = lo[b] = np.nan
            continue
        if not use[b].any():
            continue
        m64 = d64[b].min()
        cand = np.argwhere(use[b] & (d64[b] <= m64 + PREFILTER))
        frames = hl.link_frames(chain, q[b])
        vals = []
        for i, j in cand:
            link, c, r = spheres[i]
            P = hl._apply(frames[link], [hp._num(float(x)) for x in c])
            Q = [hp._num(float(x)) for x in rows[b, j, :3]]
            s = (P[0] - Q[0]) ** 2 + (P[1] - Q[1]) ** 2 + (P[2] - Q[2]) ** 2
            vals.append((_sqrt(s) - hp._num(float(r)) - hp._num(float(rows[b, j, 3])), int(i) * 32 + int(j), int(i), int(j)))
        best = min(vals, key=lambda v: (v[0], v[1]))
        hi[b] = float(best[0])
        lo[b] = float(best[0] - hp._num(hi[b]))
        pair[b] = best[1]
        others = [float(v[0]) for v in vals if v[0] != best[0]]
        far = d64[b][use[b] & (d64[b] > m64 + PREFILTER)]
        second[b] = min(others + ([float(far.min())] if far.size else []) + [np.inf])
        i, j = best[2], best[3]
        unit[b] = n * U * (reach[i] + float(np.linalg.norm(rows[b, j, :3])) + abs(float(rows[b, j, 3])) + float(spheres[i][2]))
    return dict(hi=hi, lo=lo, pair=pair, second=second, unit=unit)


def error_units(got, ref):
    """|got - (hi + lo)| / unit per arm, for the arms with a finite reference; NaN elsewhere"""
    with np.errstate(invalid="ignore"):
        e = np.abs((np.asarray(got, dtype=np.float64) - ref["hi"]) - ref["lo"]) / ref["unit"]
    return np.where(np.isfinite(ref["hi"]), e, np.nan)


# ---- the cases the host test and the GPU test share ---------------------------------------------------------------------------------
ROW_SOURCES = ("partner", "own", "static")
# (batch, sphere list, count, first, rows): every batch size, list, count, window start and source at least once per chain and I/O type
CASES = ((203, "all16", 32, 0, "partner"), (65, "five", 5, 3, "own"), (1, "one", 1, 0, "static"), (203, "five", 16, 3, "static"),
         (65, "all16", 16, 0, "own"), (203, "one", 5, 3, "partner"))
EXTRA_ROWS = 2   # n_rep = first + count + EXTRA_ROWS: rows the kernel must not look at lie on both sides of the window


def host_place(chain, spheres, io_dtype):
    """place(q, src_arm, xform) on the host: hp_links.host_points rounded to the I/O type (what tests without a GPU take for link_points)"""
    return lambda q, src, x: hl.host_points(chain, spheres, q, src, x).astype(io_dtype).astype(np.float64)


def make_case(robot, io_dtype, B, kind, count, first, rows, place=None, seed=11):
    """One case: dict(chain, spheres, q, pts (B, n_rep, 4) float64 of I/O-typed values, first, count, mask (L words or None)).
    place(q, src_arm, xform) -> (B, L, 4): where link spheres are, I/O-typed (the GPU test hands in the device's link_points).
    partner  the links of arm b ^ 1 through the case's transform (the last arm of an odd batch: NaN rows); rows beyond L are static spheres
    own      the arm's own links, the mask dropping pairs on the same or on adjacent links and keeping each unordered pair once (i < j:
             d_ij and d_ji are one distance, apart only by the rows' rounding); rows beyond L are static spheres, all bits set
    static   random spheres within the arm's reach of which every fifth row is NaN
    The rows outside the window hold spheres AT the arm's own first sphere, radius 1: reading one of them would make the clearance -1."""
    chain = hl.chain_of(robot)
    spheres = hl.sphere_list(chain, kind)
    L = len(spheres)
    q, x = hl.inputs(chain, B, io_dtype, seed=seed)
    place = place or host_place(chain, spheres, io_dtype)
    rng = np.random.default_rng(seed + 1000 * count + first)
    rnd = lambda a: np.asarray(a, dtype=np.float64).astype(io_dtype).astype(np.float64)
    n_rep = first + count + EXTRA_ROWS
    reach = float(hl.reach(chain, spheres).max())
    static = np.concatenate([rng.uniform(-0.6 * reach, 0.6 * reach, size=(B, count, 3)), rng.uniform(0.02, 0.1, size=(B, count, 1))], axis=2)
    own = place(q, None, None)
    pts = np.empty((B, n_rep, 4))
    pts[:, :, :3] = own[:, :1, :3]
    pts[:, :, 3] = 1.0
    win = rnd(static)
    mask = None
    if rows == "partner":
        src = (np.arange(B, dtype=np.int32) ^ 1)
        src[src >= B] = -1
        them = place(q, src, x)
        k = min(L, count)
        win[:, :k] = them[:, :k]
    elif rows == "own":
        k = min(L, count)
        win[:, :k] = own[:, :k]
        links = np.array([s[0] for s in spheres])
        keep = np.ones((L, count), dtype=bool)
        keep[:, :k] = (np.abs(links[:, None] - links[None, :k]) > 1) & (np.arange(L)[:, None] < np.arange(k)[None, :])
        mask = mask_words(keep)
    else:
        assert rows == "static"
        win[:, 4::5] = np.nan
    pts[:, first:first + count] = win
    return dict(chain=chain, spheres=spheres, q=q, pts=pts, first=first, count=count, mask=mask)


_HOST_RATIO = {}


def host_ratio(robot, io_dtype, case):
    """R of a case of CASES on host-placed rows: the host form's worst error in units, with the reference -- computed once per case."""
    key = (robot, np.dtype(io_dtype).name) + tuple(case)
    if key not in _HOST_RATIO:
        c = make_case(robot, io_dtype, *case)
        ref = clearance(c["chain"], c["spheres"], c["q"], c["pts"], c["first"], c["count"], c["mask"])
        clear, pair, _d = host_clearance(c["chain"], c["spheres"], c["q"], c["pts"], c["first"], c["count"], c["mask"])
        e = error_units(clear, ref)
        _HOST_RATIO[key] = (float(np.nanmax(e)) if np.isfinite(e).any() else 0.0, ref, clear, pair, c)
    return _HOST_RATIO[key]


def ambiguous(ref, bar):
    """the arms whose two smallest d_ij lie closer than twice `bar` (B,): left out of the pair comparison only"""
    with np.errstate(invalid="ignore"):
        return np.isfinite(ref["hi"]) & (ref["second"] - ref["hi"] < 2.0 * bar)
