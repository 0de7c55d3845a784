"""vfik_link_clearance on the GPU (include/vfik.h; clear_kernel, vfclik_amd/csrc/vfik_aux.hip) against the 50-digit clearance of
tests/hp_clearance.py, in both I/O types.

Chains: the four of hp_links.ROBOTS.  Per chain and I/O type the six cases of hp_clearance.CASES: batches of 1, 65 and 203 arms (one lane,
one lane past a wave, a tail past a block that is no multiple of 64); the sphere lists one, five and all16; count 1, 5, 16 and 32; first 0
and 3 with n_rep = first + count + 2, the rows outside the window holding spheres that would give a clearance of -1; rows from the three
sources -- the device's own link_points of the partner b ^ 1 through a transform, the arm's own links under a mask that drops same-link and
adjacent-link pairs, random static spheres of which every fifth row is NaN.

THE BAR on clear: K_MARGIN max(1, R) units + half an ulp of the output type; the unit is n u (reach_i + |Q_j| + R_j + r_i) of the minimising
pair (hp_clearance derives it from the kernel's operations), R the host's worst error in the same units (tests/test_clearance_reference.py
prints it: up to 0.15).  +inf and NaN agree exactly.  pair is exact, except for arms whose two smallest d_ij lie closer than twice that bar
in the reference: those are left out of the pair comparison only, and capped at 5 % on the reference's numbers.
Ties (one sphere entered twice, one row entered twice): the smaller code, exactly.  Edges: all rows NaN or masked -> +inf and -1; a NaN in q
-> NaN and -1.  The host form equals the device form bit for bit.

With VFIK_CLEARANCE_TABLE=<file> the measured worst ratios are also written there (the record kept in profiles/clearance_accuracy.txt)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hp_clearance as hc  # noqa: E402
import hp_links as hl  # noqa: E402

pytestmark = pytest.mark.gpu

AMBIGUOUS_CAP = 0.05


@pytest.fixture(scope="module")
def env():
    import __graft_entry__ as g
    g.build()
    import torch
    from vfclik_amd import engine

    class E:
        pass

    e = E()
    e.engine, e.torch = engine, torch
    e.dev = torch.device("cuda", 0)
    e.table = []
    yield e
    path = os.environ.get("VFIK_CLEARANCE_TABLE")
    if path and e.table:
        with open(path, "a") as f:
            f.write("".join(e.table))


def _dev(env, a, dtype):
    return env.torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(env.dev)


def _both_forms(env, eng, c):
    """(clear float64, pair int32) of the host form, after holding the device form to it bit for bit"""
    t = eng.io_dtype.type
    clear, pair = eng.link_clearance_host(c["q"], c["pts"], c["first"], c["count"], c["mask"])
    dc, dp = eng.link_clearance(_dev(env, c["q"], t), _dev(env, c["pts"], t), c["first"], c["count"], c["mask"])
    eng.sync()
    dc, dp = dc.cpu().numpy(), dp.cpu().numpy()
    assert dc.dtype == eng.io_dtype and np.array_equal(dc.astype(np.float64), clear, equal_nan=True) and np.array_equal(dp, pair)
    assert np.array_equal(clear.astype(t).astype(np.float64), clear, equal_nan=True)   # I/O-typed values, widened
    return clear, pair


@pytest.mark.parametrize("robot", hl.ROBOTS)
@pytest.mark.parametrize("io_dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_against_50_digits(env, robot, io_dtype):
    chain = hl.chain_of(robot)
    for case in hc.CASES:
        B, kind, count, first, rows = case
        spheres = hl.sphere_list(chain, kind)
        eng = env.engine.Engine(chain, B, io_dtype=io_dtype, max_slots=16)
        eng.set_link_spheres(spheres)
        c = hc.make_case(robot, io_dtype, *case, place=lambda q, src, x: eng.link_points_host(q, src, x))
        R = hc.host_ratio(robot, io_dtype, case)[0]
        ref = hc.clearance(chain, spheres, c["q"], c["pts"], first, count, c["mask"])
        clear, pair = _both_forms(env, eng, c)
        eng.close()
        fin = np.isfinite(ref["hi"])
        assert np.array_equal(np.isnan(clear), np.isnan(ref["hi"])) and np.array_equal(np.isposinf(clear), np.isposinf(ref["hi"]))
        half_ulp = 0.5 * np.spacing(np.abs(np.where(fin, ref["hi"], 1.0)).astype(io_dtype)).astype(np.float64)
        bar = hc.K_MARGIN * max(1.0, R) * ref["unit"] + half_ulp
        err = np.abs((clear - ref["hi"]) - ref["lo"])
        # the kernel's own share in units: what is left of the error after the output's rounding
        ratio = float(np.max(np.maximum(err[fin] - half_ulp[fin], 0.0) / ref["unit"][fin])) if fin.any() else 0.0
        amb = hc.ambiguous(ref, bar)
        line = "%-10s %-7s %-30s R = %.3f  worst %.3f units of n u (reach + |Q| + R + r); %d of %d arms with a pair, %d ambiguous\n" % (
            robot, np.dtype(io_dtype).name, case, R, ratio, fin.sum(), B, amb.sum())
        print(line, end="")
        env.table.append(line)
        assert amb.sum() <= AMBIGUOUS_CAP * max(fin.sum(), 1), (case, amb.sum())
        assert np.all(err[fin] <= bar[fin]), (case, float(np.max(err[fin] / bar[fin])))
        assert np.array_equal(pair[~amb], ref["pair"][~amb]), (case, np.flatnonzero(~amb & (pair != ref["pair"])))
        assert np.all(pair[~fin] == -1)


@pytest.mark.parametrize("io_dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_ties_take_the_smallest_code(env, io_dtype):
    """own sphere 1 entered again at caller index 3 -- the image sorts them next to each other, the kernel meets them in link order -- and
    row 0 entered again as row 2: both d_ij are the same double on the device, and the smaller code must win, exactly"""
    c = hc.make_case("lwr", io_dtype, 65, "five", 5, 0, "static")
    sp = list(c["spheres"])
    sp[3] = sp[1]
    c["spheres"] = sp
    c["pts"][:, 2] = c["pts"][:, 0]
    eng = env.engine.Engine(c["chain"], 65, io_dtype=io_dtype, max_slots=16)
    eng.set_link_spheres(sp)
    ref = hc.clearance(c["chain"], sp, c["q"], c["pts"], 0, 5, None)
    clear, pair = _both_forms(env, eng, c)
    own, row = ref["pair"] // 32, ref["pair"] % 32
    assert np.any(own == 1) and np.any(row == 0) and not np.any(own == 3) and not np.any(row == 2)   # the reference meets both ties
    bar = hc.K_MARGIN * ref["unit"] + 0.5 * np.spacing(np.abs(ref["hi"]).astype(io_dtype)).astype(np.float64)
    amb = hc.ambiguous(ref, bar)
    assert amb.sum() <= AMBIGUOUS_CAP * 65
    assert np.array_equal(pair[~amb], ref["pair"][~amb])
    assert not np.any(pair // 32 == 3) and not np.any(pair % 32 == 2)    # every arm, ambiguous or not: never the larger code of a tie
    eng.close()


@pytest.mark.parametrize("io_dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_edges(env, io_dtype):
    c = hc.make_case("mixed10", io_dtype, 65, "five", 5, 3, "static")
    L = len(c["spheres"])
    eng = env.engine.Engine(c["chain"], 65, io_dtype=io_dtype, max_slots=16)
    eng.set_link_spheres(c["spheres"])
    # every row of the window NaN (the rows outside still hold spheres): +inf, -1
    e = dict(c, pts=c["pts"].copy())
    e["pts"][:, 3:8] = np.nan
    clear, pair = _both_forms(env, eng, e)
    assert np.all(np.isposinf(clear)) and np.all(pair == -1)
    # every pair masked
    clear, pair = _both_forms(env, eng, dict(c, mask=np.zeros(L, dtype=np.uint32)))
    assert np.all(np.isposinf(clear)) and np.all(pair == -1)
    # a NaN in one element of a row takes that row out, the radius included
    e = dict(c, pts=c["pts"].copy())
    e["pts"][:, 3:8, 3] = np.nan
    e["pts"][:, 5, 3] = 0.05
    clear, pair = _both_forms(env, eng, e)
    assert np.all(pair % 32 == 2) and np.isfinite(clear).all()
    # a NaN anywhere in q: NaN, -1 -- for that arm alone
    e = dict(c, q=c["q"].copy())
    e["q"][7, c["chain"].n - 1] = np.nan
    e["q"][64, 0] = np.nan
    clear, pair = _both_forms(env, eng, e)
    want, wpair = _both_forms(env, eng, c)
    bad = np.isin(np.arange(65), (7, 64))
    assert np.isnan(clear[bad]).all() and np.all(pair[bad] == -1)
    assert np.array_equal(clear[~bad], want[~bad]) and np.array_equal(pair[~bad], wpair[~bad])
    eng.close()


def test_refusals(env):
    c = hc.make_case("lwr", np.float32, 65, "five", 5, 3, "static")
    eng = env.engine.Engine(c["chain"], 65, io_dtype=np.float32, max_slots=16)
    E = env.engine.VfikError
    with pytest.raises(E, match="no link spheres"):
        eng.link_clearance_host(c["q"], c["pts"], 3, 5)
    eng.set_link_spheres(c["spheres"])
    for first, count in ((3, 0), (3, 33), (-1, 5), (6, 5)):
        with pytest.raises(E):
            eng.link_clearance_host(c["q"], c["pts"], first, count)
    with pytest.raises(E, match="at or beyond count"):
        eng.link_clearance_host(c["q"], c["pts"], 3, 5, mask=np.array([1, 1, 1 << 5, 1, 1], dtype=np.uint32))
    t = env.torch
    q, pts = _dev(env, c["q"], np.float32), _dev(env, c["pts"], np.float32)
    odd = t.empty(pts.numel() + 2, dtype=t.float32, device=env.dev)[2:].view(pts.shape)   # 8 bytes off a 16-byte boundary
    odd.copy_(pts)
    with pytest.raises(E, match="16-byte"):
        eng.link_clearance(q, odd, 3, 5)
    out, pair = eng.link_clearance(q, pts, 3, 5)      # the same rows, aligned
    eng.sync()
    assert np.array_equal(out.cpu().numpy().astype(np.float64), eng.link_clearance_host(c["q"], c["pts"], 3, 5)[0])
    eng.close()
