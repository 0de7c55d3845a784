"""tests/hp_blocks.py held on the CPU, before a GPU is asked anything:

  * the caps on its input sets, from the reference alone;
  * its error function against the host's numpy: 1/x and sqrt are correctly rounded (<= 0.5 ulp); sin, cos, arctan2 and power are recorded
    as R, the host libm's own error under the same function;
  * planted faults: a float64 numpy model of a block (fmas emulated by error-free transformations, close to exact) stays under the block's
    bar on the block's own input set, and the same model with ONE defect exceeds it -- the bars bite.  The defects: the Newton step left
    out (seed modelled at 5e-9) of rcp_1nr and rsqrt_1nr; one table entry off by 4 u; the third Cody-Waite part dropped; one
    multiplication of the power chain skipped; atan_kernel fed t = 0.45 without the reduction; the mixer sum fused.
    (For rcp_nr and the Goldschmidt pair ONE missing step from a 5e-9 seed leaves 0.2 - 0.4 u, which no bar made of roundings can see:
    their seed terms are e0^4.  That is what the one-step functions' e0-based bars are for.)
  * the table of tests/golden/kconst_images.npz, and of the host driver tests/c_host/kconst.cpp on this machine's libm, is the correctly
    rounded (sin, cos)(k pi/32);
  * the harness builds for gfx950 without a GPU and exports its entry point."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hp_blocks as hb  # noqa: E402
from test_kconst import answers, driver, golden  # noqa: E402,F401  (the fixtures of the kconst driver)

U = hb.U


# ---- caps ------------------------------------------------------------------------------------------------------------------------------
def test_caps_atan2_branches():
    count = np.bincount(hb.atan2_branches(), minlength=8)
    print("atan2_pos points per (steep, upper, x < 0):", count.tolist())
    assert count.min() >= 200, count


def test_caps_nearest_to_k_pi_2():
    names, sl, x = hb.sincos_sets()
    xs = x[sl["nearest to k pi/2"]]
    d = hb.distance_to_k_pi_2(xs)
    print("nearest to k pi/2: %d points, %d within 1e-13, smallest non-zero distance %.3e" % (len(xs), int((d < 1e-13).sum()), d[d > 0].min()))
    assert int((d < 1e-13).sum()) >= 50
    assert len(x) <= 40000 and hb.sincos_contract() == sl[hb.SINCOS_OUTSIDE].start


def test_caps_unfused_triples_tell_fused_from_unfused():
    twice, once, _ = hb.unfused_reference()
    differ = int((~hb.same_bits(twice, once)).sum())
    print("unfused triples: %d of %d round differently fused" % (differ, len(twice)))
    assert 4 * differ >= len(twice)


def test_caps_power_points_stay_in_range():
    assert hb.power_squares_in_range()
    x, n = hb.power_points()
    assert sorted(set(n.tolist())) == sorted(float(o) for o in hb.INT_ORDERS)
    assert all(np.all((x[n == o] >= (1e-3 if o <= 20 else 0.5)) & (x[n == o] <= (1e3 if o <= 20 else 2.0))) for o in hb.INT_ORDERS)
    waves = hb.power_waves()
    for name, (rows, idx) in waves.items():   # every composition holds every pair once
        assert sorted(idx[idx >= 0].tolist()) == list(range(len(x))), name
        assert np.array_equal(rows[idx >= 0][np.argsort(idx[idx >= 0])], np.stack([x, n], axis=1)), name


def test_k_times_head_is_exact_on_every_input():
    names, sl, x = hb.sincos_sets()
    n = hb.sincos_contract()
    ks = hb.tab_k(x[:n])
    assert np.abs(ks).max() >= 1e6 and hb.k_head_exact(ks)      # |x| up to 1e5 rad: k up to 1.02e6
    assert not hb.k_head_exact([2 ** 30 + 1])                   # the check can fail: a 31-bit odd k times the head is no double


# ---- the error function against the host ------------------------------------------------------------------------------------------------
def test_error_function_against_host_numpy():
    x = hb.root_sets()[2][:hb.root_asserted()]
    ref = hb.root_reference()
    for name, got in (("1/x", 1.0 / x), ("sqrt", np.sqrt(x))):
        a, ulp, rel = hb.errors(got, *ref["rcp" if name == "1/x" else "sqrt"])
        print("host %-7s worst %.3f ulp, %.3f u relative" % (name, ulp.max(), rel.max()))
        assert ulp.max() <= 0.5 and rel.max() <= 1.0
    # a value one ulp off is one ulp off, and the lo word counts
    hi, lo = ref["sqrt"]
    assert np.allclose(hb.errors(np.nextafter(hi, np.inf), hi, np.zeros_like(hi))[1], 1.0)
    assert np.all(hb.errors(hi, hi, lo)[1] <= 0.5) and hb.errors(hi, hi, lo)[1].max() > 0.45
    xs = hb.sincos_sets()[2][:hb.sincos_contract()]
    (sh, slo), (ch, clo) = hb.sincos_reference()
    n = len(xs)
    print("host sin     R = %.3f ulp, %.3f u absolute" % (hb.errors(np.sin(xs), sh[:n], slo[:n])[1].max(), hb.errors(np.sin(xs), sh[:n], slo[:n])[0].max()))
    print("host cos     R = %.3f ulp, %.3f u absolute" % (hb.errors(np.cos(xs), ch[:n], clo[:n])[1].max(), hb.errors(np.cos(xs), ch[:n], clo[:n])[0].max()))
    _, _, y, xx = hb.atan2_sets()
    print("host arctan2 R = %.3f ulp" % hb.errors(np.arctan2(y, xx), *hb.atan2_reference())[1].max())
    px, po = hb.pow_path_points()
    R = hb.errors(np.power(px, po), *hb.pow_path_reference())[1].max()
    print("host power   R = %.3f ulp" % R)
    assert R < 16.0     # a libm is no reference, but one that is 16 ulp off would make the pow() path's bar meaningless


# ---- float64 models of the blocks -------------------------------------------------------------------------------------------------------
def _two_prod(a, b):
    """a b = p + e exactly (Dekker / Veltkamp), away from overflow and underflow"""
    p = a * b
    ca, cb = a * 134217729.0, b * 134217729.0
    ah, bh = ca - (ca - a), cb - (cb - b)
    al, bl = a - ah, b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def fma(a, b, c):
    """a b + c with one rounding, to ~u^2: the product and the sum by error-free transformations"""
    a, b, c = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), np.asarray(c, dtype=np.float64))
    p, e = _two_prod(a, b)
    s = p + c
    bb = s - p
    return s + (((p - (s - bb)) + (c - bb)) + e)


def _scaled(x, even):
    """x = m 2^e with m in [0.5, 1) (even: m in [0.5, 2), e even): the blocks are exact in powers of two, the models run on m"""
    m, e = np.frexp(x)
    if even:
        odd = e % 2 != 0
        m, e = np.where(odd, 2.0 * m, m), np.where(odd, e - 1, e)
    return m, e


SEED_E0 = 5e-9


def model_rcp_1nr(x, steps=1):
    m, e = _scaled(np.abs(x), False)
    y = (1.0 / m) * (1.0 + SEED_E0 * np.where(np.arange(len(m)) % 2, -1.0, 1.0))
    for _ in range(steps):
        y = fma(y, fma(-m, y, 1.0), y)
    return np.sign(x) * np.ldexp(y, -e)


def model_rsqrt_1nr(x, steps=1):
    m, e = _scaled(x, True)
    y = (1.0 / np.sqrt(m)) * (1.0 + SEED_E0 * np.where(np.arange(len(m)) % 2, -1.0, 1.0))
    for _ in range(steps):
        y = fma(0.5 * y, fma(-(m * y), y, 1.0), y)
    return np.ldexp(y, -(e // 2))


def model_sincos_fast(x, parts=3):
    k = np.rint(x * 6.36619772367581382433e-01)
    r = x
    for p in (1.57079632673412561417e+00, 6.07710050630396597660e-11, 2.02226624879595063154e-21)[:parts]:
        r = fma(-k, p, r)
    z = r * r
    ps, pc = 1.58969099521155010221e-10, -1.13596475577881948265e-11
    for a, b in ((-2.50507602534068634195e-08, 2.08757232129817482790e-09), (2.75573137070700676789e-06, -2.75573143513906633035e-07),
                 (-1.98412698298579493134e-04, 2.48015872894767294178e-05), (8.33333333332248946124e-03, -1.38888888888741095749e-03),
                 (-1.66666666666666324348e-01, 4.16666666666666019037e-02)):
        ps, pc = fma(z, ps, a), fma(z, pc, b)
    sr = fma(z * r, ps, r)
    cr = fma(z * z, pc, fma(z, -0.5, 1.0))
    n = k.astype(np.int64)
    sv, cv = np.where(n & 1, cr, sr), np.where(n & 1, sr, cr)
    return np.where(n & 2, -sv, sv), np.where((n + 1) & 2, -cv, cv)


def model_sincos_tab(x, table):
    k = np.rint(x * hb.TAB_SCALE)
    S, C = table[k.astype(np.int64) & 63, 0], table[k.astype(np.int64) & 63, 1]
    r = fma(-k, 3.79818781656637e-12, fma(-k, hb.TAB_HEAD, x))
    z = r * r
    ps = fma(z, fma(z, -1.98412698412698412698e-04, 8.33333333333333333333e-03), -1.66666666666666666667e-01)
    pc = fma(z, fma(z, 2.48015873015873015873e-05, -1.38888888888888888889e-03), 4.16666666666666666667e-02)
    ps, pc = fma(z * r, ps, r), fma(z, fma(z, pc, -0.5), 1.0)
    return fma(C, ps, S * pc), fma(-S, ps, C * pc)


def model_powi(x, n, skip=False):
    """square and multiply, lowest bit first; skip: the multiplication of the lowest set bit is left out"""
    n = n.astype(np.int64)
    r, b = np.ones_like(x), x.copy()
    low = n & -n
    with np.errstate(over="ignore"):
        for k in range(7):
            use = (n & (1 << k)) != 0
            if skip:
                use = use & (low != (1 << k))
            r = np.where(use, r * b, r)
            b = b * b
    return r


def model_atan_kernel(t):
    z = t * t
    w = z * z
    s1 = z * (3.33333333333329318027e-01 + w * (1.42857142725034663711e-01 + w * (9.09088713343650656196e-02 +
              w * (6.66107313738753120669e-02 + w * (4.97687799461593236017e-02 + w * 1.62858201153657823623e-02)))))
    s2 = w * (-1.99999999998764832476e-01 + w * (-1.11111104054623557880e-01 + w * (-7.69187620504482999495e-02 +
              w * (-5.83357013379057348645e-02 + w * -3.65315727442169155270e-02))))
    return t - t * (s1 + s2)


# ---- planted faults ---------------------------------------------------------------------------------------------------------------------
def test_planted_fault_newton_step_left_out():
    x = hb.root_sets()[2][:hb.root_asserted()]
    ref = hb.root_reference()
    both = np.concatenate([x, -x])
    rcp = (np.concatenate([ref["rcp"][0], -ref["rcp"][0]]), np.concatenate([ref["rcp"][1], -ref["rcp"][1]]))
    e0 = hb.errors(model_rcp_1nr(both, steps=0), *rcp)[2].max() * U
    assert 4.9e-9 < e0 < 5.1e-9
    for name, model, r, bar in (("rcp_1nr", model_rcp_1nr, rcp, hb.bar_rcp_1nr(e0)), ("rsqrt_1nr", model_rsqrt_1nr, ref["rsqrt"], hb.bar_rsqrt_1nr(e0))):
        arg = both if name == "rcp_1nr" else x
        sound, faulty = hb.errors(model(arg), *r)[2].max(), hb.errors(model(arg, steps=0), *r)[2].max()
        print("%-9s bar %.3f u relative: sound model %.3f, without its Newton step %.3e" % (name, bar, sound, faulty))
        assert sound <= bar < faulty
    assert hb.bar_goldschmidt(e0) <= hb.GOLDSCHMIDT_CEILING_U and hb.bar_goldschmidt(1e-6) <= hb.GOLDSCHMIDT_CEILING_U


def test_planted_fault_table_entry_and_cody_waite_part():
    n = hb.sincos_contract()
    x = hb.sincos_sets()[2][:n]
    (sh, slo), (ch, clo) = hb.sincos_reference()

    def worst(sc):
        return max(hb.errors(sc[0], sh[:n], slo[:n])[0].max(), hb.errors(sc[1], ch[:n], clo[:n])[0].max())

    table = hb.table_reference()
    off = table.copy()
    off[5, 0] += 4.0 * U
    sound, faulty = worst(model_sincos_tab(x, table)), worst(model_sincos_tab(x, off))
    print("sincos_tab_n bar %.1f u absolute: sound model %.3f, one table entry off by 4 u %.3f" % (hb.BAR_SINCOS_TAB_ABS_U, sound, faulty))
    assert sound <= hb.BAR_SINCOS_TAB_ABS_U < faulty
    sound, faulty = worst(model_sincos_fast(x)), worst(model_sincos_fast(x, parts=2))
    print("sincos_fast  bar %.1f u absolute: sound model %.3f, third Cody-Waite part dropped %.3f" % (hb.BAR_SINCOS_FAST_ABS_U, sound, faulty))
    assert sound <= hb.BAR_SINCOS_FAST_ABS_U < faulty


def test_planted_fault_power_chain():
    x, n = hb.power_points()
    hi, lo = hb.power_reference()
    sound, faulty = hb.errors(model_powi(x, n), hi, lo)[2], hb.errors(model_powi(x, n, skip=True), hi, lo)[2]
    for o in hb.INT_ORDERS:
        m = n == o
        print("x^%-3d bar %3d u relative: sound model %.2f, one multiplication skipped %.3e" % (o, hb.bar_powi(o), sound[m].max(), faulty[m].max()))
        assert sound[m].max() <= hb.bar_powi(o)
        assert o == 0 or faulty[m].max() > hb.bar_powi(o)
    assert np.all(model_powi(x, n)[n == 0] == 1.0) and np.array_equal(model_powi(x, n)[n == 1], x[n == 1])


def test_planted_fault_atan_kernel_without_the_reduction():
    t = hb.atan_kernel_points()
    sound = hb.errors(model_atan_kernel(t), *hb.atan_kernel_reference())[1].max()
    tt = np.array([0.45, -0.45])
    faulty = hb.errors(model_atan_kernel(tt), np.arctan(tt), np.zeros(2))[1].max()   # libm's half ulp does not matter to this figure
    print("atan_kernel bar %.1f ulp: sound model %.3f on |t| <= tan(pi/8), at t = 0.45 %.3f" % (hb.BAR_ATAN_KERNEL_ULP, sound, faulty))
    assert sound <= hb.BAR_ATAN_KERNEL_ULP < faulty - 0.5


def test_planted_fault_mixer_sum_fused():
    t = hb.unfused_triples()
    twice, once, prod = hb.unfused_reference()
    assert np.all(hb.same_bits(t[:, 0] + t[:, 1] * t[:, 2], twice)) and np.all(hb.same_bits(t[:, 1] * t[:, 2], prod))   # numpy rounds twice
    assert not np.all(hb.same_bits(once, twice))


# ---- the table and the harness ----------------------------------------------------------------------------------------------------------
def test_table_is_the_correctly_rounded_sine_and_cosine(golden, answers):  # noqa: F811
    assert hb.table_is_correctly_rounded(hb.kconst_table())
    i = golden["names"].index("lwr")
    assert hb.table_is_correctly_rounded(hb.kconst_table(golden["images"][i]))
    assert hb.table_is_correctly_rounded(hb.kconst_table(answers[i]["image"]))      # kconst_fill on this machine's libm: the very bytes the kernels get
    for k, j in ((5, 0), (32, 0), (63, 1)):      # the check can fail: one ulp off an entry, or a zero entry beyond the long double pi's residue
        off = hb.kconst_table()
        off[k, j] = np.nextafter(off[k, j], np.inf) if off[k, j] != 0.0 and k != 32 else 4.0 * hb.TABLE_ZERO_RESIDUE
        assert not hb.table_is_correctly_rounded(off)


def test_harness_builds_for_gfx950_and_exports_its_entry():
    import __graft_entry__ as g
    g.build()
    assert os.path.exists(hb.HARNESS) and os.path.exists(hb.HARNESS + ".srchash")
    lib = ctypes.CDLL(hb.HARNESS)
    assert hasattr(lib, "vfik_blocks_run")
    with open(hb.HARNESS, "rb") as f:
        blob = f.read()
    assert b"gfx950" in blob and all(("k_" + name).encode() in blob for name in hb.BLOCKS)
    # a bad request is refused before anything touches a device (hipErrorInvalidValue = 1)
    one = np.ones(1)
    lib.vfik_blocks_run.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p]
    assert lib.vfik_blocks_run(len(hb.BLOCKS), one.ctypes.data, 1, one.ctypes.data, 1, None) == 1
    assert lib.vfik_blocks_run(hb.BLOCKS["atan2_pos"][0], one.ctypes.data, 1, one.ctypes.data, 1, None) == 1
