"""The host's float64 clearance (hp_clearance.host_clearance: Chain.fk of the truncated chains and NumPy) against the 50-digit one
(hp_clearance.clearance) on the cases of tests/test_gpu_link_clearance.py, with host-placed rows: R, the host's worst error in units of
n u (reach_i + |Q_j| + R_j + r_i), printed per case and held under K_MARGIN -- the GPU test gives the device K_MARGIN max(1, R) of the
same units.  Also checked here, on the reference alone: the edge rules, the tie rule, and the cap on the arms whose closest pair is
ambiguous (the GPU test leaves those out of its pair comparison)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hp_clearance as hc  # noqa: E402
import hp_links as hl  # noqa: E402

AMBIGUOUS_CAP = 0.05


@pytest.mark.parametrize("robot", hl.ROBOTS)
@pytest.mark.parametrize("io_dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_host_clearance_against_50_digits(robot, io_dtype):
    worst = 0.0
    for case in hc.CASES:
        R, ref, clear, pair, c = hc.host_ratio(robot, io_dtype, case)
        bar = hc.K_MARGIN * max(1.0, R) * ref["unit"] + 0.5 * np.spacing(np.abs(ref["hi"]).astype(io_dtype)).astype(np.float64)
        amb = hc.ambiguous(ref, bar)
        fin = np.isfinite(ref["hi"])
        print("%-10s %-28s R = %.3f units; %d of %d arms have a pair, %d ambiguous" % (robot, case, R, fin.sum(), len(fin), amb.sum()))
        worst = max(worst, R)
        assert np.array_equal(np.isnan(clear), np.isnan(ref["hi"])) and np.array_equal(np.isinf(clear), np.isinf(ref["hi"]))
        assert np.array_equal(pair[~amb], ref["pair"][~amb])
        assert amb.sum() <= AMBIGUOUS_CAP * max(fin.sum(), 1), (case, amb.sum(), fin.sum())
        # the window: a row outside it sits at the arm's own first sphere with radius 1 -- reading it would give a clearance near -1
        assert np.nanmin(np.where(fin, ref["hi"], np.nan)) > -0.9 if fin.any() else True
    assert hl.hp.BACKEND in ("mpmath", "longdouble")
    assert worst < hc.K_MARGIN, worst


def _lwr_case(B=8, io_dtype=np.float64):
    return hc.make_case("lwr", io_dtype, B, "five", 5, 0, "static")


def test_edge_rules_of_the_reference():
    c = _lwr_case()
    L = len(c["spheres"])
    for fn in (lambda *a: hc.host_clearance(*a)[:2], lambda *a: (lambda r: (r["hi"], r["pair"]))(hc.clearance(*a))):
        # nothing considered: every row NaN, or every pair masked
        pts = np.full_like(c["pts"], np.nan)
        clear, pair = fn(c["chain"], c["spheres"], c["q"], pts, 0, 5, None)
        assert np.all(np.isposinf(clear)) and np.all(pair == -1)
        clear, pair = fn(c["chain"], c["spheres"], c["q"], c["pts"], 0, 5, np.zeros(L, dtype=np.uint32))
        assert np.all(np.isposinf(clear)) and np.all(pair == -1)
        # a NaN in q
        q = c["q"].copy()
        q[3, 2] = np.nan
        clear, pair = fn(c["chain"], c["spheres"], q, c["pts"], 0, 5, None)
        assert np.isnan(clear[3]) and pair[3] == -1 and np.isfinite(np.delete(clear, 3)).all()
        # a NaN anywhere in a row takes the row out: the radius too
        pts = c["pts"].copy()
        pts[:, :5, 3] = np.nan
        pts[:, 2, 3] = 0.05
        clear, pair = fn(c["chain"], c["spheres"], c["q"], pts, 0, 5, None)
        assert np.all(pair % 32 == 2)


def tie_case(io_dtype=np.float64, B=65):
    """own sphere 1 entered again at caller index 3 (same link, centre and radius), and row 0 entered again as row 2: the smaller code wins"""
    c = hc.make_case("lwr", io_dtype, B, "five", 5, 0, "static")
    sp = list(c["spheres"])
    sp[3] = sp[1]
    c["spheres"] = sp
    c["pts"][:, 2] = c["pts"][:, 0]
    return c


def test_ties_take_the_smallest_code():
    c = tie_case()
    ref = hc.clearance(c["chain"], c["spheres"], c["q"], c["pts"], 0, 5, None)
    clear, pair, d = hc.host_clearance(c["chain"], c["spheres"], c["q"], c["pts"], 0, 5, None)
    assert np.array_equal(pair, ref["pair"])
    own, row = pair // 32, pair % 32
    assert not np.any(own == 3) and not np.any(row == 2) and np.any(own == 1) and np.any(row == 0)
    assert np.array_equal(d[:, 1], d[:, 3]) and np.array_equal(d[:, :, 0], d[:, :, 2])


def test_mask_words_round_trip():
    rng = np.random.default_rng(3)
    m = rng.random((7, 32)) < 0.5
    assert np.array_equal(hc.mask_matrix(hc.mask_words(m), 7, 32), m)
    assert hc.mask_matrix(None, 3, 4).all()
