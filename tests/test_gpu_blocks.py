"""The float64 building blocks of vfclik_amd/csrc/vfik_device.h on the GPU, one at a time, against the 50-digit reference of tests/hp_blocks.py:
the header's own functions behind the trivial kernels of tests/device_blocks/blocks.hip (out[i] = f(in[i]); element i is lane i mod 64 of wave
i div 64).  One test per family -- reciprocals and roots, sine / cosine, powers, arctangent, unfused -- each asserting the derived bars and
the bit-for-bit identities that hp_blocks.py's docstring states and derives; no bar here comes from a measured figure.  The composite tests
(field, nullspace, observers, ...) see a block only at the arguments a robot scene generates and through the conditioning of everything
around it; here a polynomial coefficient with wrong trailing digits, a lost Newton step or a contracted mixer sum shows directly
(tests/test_blocks_reference.py plants exactly those faults in numpy models and shows that the bars catch them).

With VFIK_BLOCKS_TABLE=<file> each test appends its worst figures per block and input set (profiles/device_blocks_accuracy.txt)."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hp_blocks as hb  # noqa: E402
import hp_reference as hp  # noqa: E402

pytestmark = pytest.mark.gpu
U = hb.U


@pytest.fixture(scope="module")
def env():
    import __graft_entry__ as g
    g.build()
    hb.load_harness()

    class E:
        table = []

        def note(self, line):
            print(line)
            self.table.append(line)

        def figures(self, block, what, got, hi, lo, idx=None):
            """one line of the record: the worst absolute, ulp and relative error of `block` on the points `idx`"""
            idx = slice(None) if idx is None else idx
            a, ulp, rel = hb.errors(np.asarray(got)[idx], hi[idx], lo[idx])
            fin = np.isfinite(np.asarray(got)[idx])
            self.note("%-16s %-28s %6d points: abs %10.4g u   %8.4g ulp   rel %10.4g u%s" % (
                block, what, a.size, a[fin].max() if fin.any() else np.nan, ulp[fin].max() if fin.any() else np.nan,
                rel[fin].max() if fin.any() else np.nan, "" if fin.all() else "   (%d not finite)" % int((~fin).sum())))

    e = E()
    yield e
    path = os.environ.get("VFIK_BLOCKS_TABLE")
    if path and e.table:
        with open(path, "a") as f:
            f.write("\n".join(e.table) + "\n")


def _both(pair):
    return np.concatenate([pair[0], -pair[0]]), np.concatenate([pair[1], -pair[1]])


def test_reciprocals_and_roots(env):
    names, sl, x = hb.root_sets()
    n = hb.root_asserted()
    xa, ref = x[:n], hb.root_reference()
    both, rcp = np.concatenate([xa, -xa]), _both(ref["rcp"])
    raw_rcp, raw_rsq = hb.run("rcp_raw", both), hb.run("rsq_raw", xa)
    e0_rcp = float(hb.errors(raw_rcp, *rcp)[2].max()) * U
    e0_rsq = float(hb.errors(raw_rsq, *ref["rsqrt"])[2].max()) * U
    rms = [float(np.sqrt(np.mean((hb.errors(g, *r)[2] * U) ** 2))) for g, r in ((raw_rcp, rcp), (raw_rsq, ref["rsqrt"]))]
    env.note("seeds: v_rcp_f64 e0 = %.4g relative (rms %.3g), v_rsq_f64 e0 = %.4g relative (rms %.3g) -- recorded, not asserted" % (e0_rcp, rms[0], e0_rsq, rms[1]))
    bar_r1, bar_q1, bar_g = hb.bar_rcp_1nr(e0_rcp), hb.bar_rsqrt_1nr(e0_rsq), hb.bar_goldschmidt(e0_rsq)
    env.note("bars: rcp_nr %.1f ulp, rcp_1nr %.4f u, rsqrt_1nr %.4f u, sqrt_rsqrt / rsqrt_n %.4f u relative" % (hb.BAR_RCP_NR_ULP, bar_r1, bar_q1, bar_g))
    assert bar_g <= hb.GOLDSCHMIDT_CEILING_U
    full = {"rsqrt_1nr": hb.run("rsqrt_1nr", x), "sqrt_rsqrt": hb.run("sqrt_rsqrt", x), "rsqrt_n4": hb.run4("rsqrt_n4", x)}
    got = {"rcp_raw": (raw_rcp, rcp, True), "rsq_raw": (raw_rsq, ref["rsqrt"], False),
           "rcp_nr": (hb.run("rcp_nr", both), rcp, True), "rcp_1nr": (hb.run("rcp_1nr", both), rcp, True),
           "rsqrt_1nr": (full["rsqrt_1nr"][:n], ref["rsqrt"], False), "rsqrt_1nr_pos": (hb.run("rsqrt_1nr_pos", xa), ref["rsqrt"], False),
           "sqrt_rsqrt root": (full["sqrt_rsqrt"][:n, 0], ref["sqrt"], False), "sqrt_rsqrt inv": (full["sqrt_rsqrt"][:n, 1], ref["rsqrt"], False),
           "rsqrt_n<4>": (full["rsqrt_n4"][:n], ref["rsqrt"], False)}
    for block, (g, r, signed) in got.items():
        for name in hb.ROOT_ASSERTED:
            idx = np.arange(sl[name].start, sl[name].stop)
            env.figures(block, name + (" (both signs)" if signed else ""), g, r[0], r[1], np.concatenate([idx, n + idx]) if signed else idx)
    failures = []

    def hold(block, column, bar):
        g, r, _ = got[block]
        worst = float(hb.errors(g, *r)[column].max())
        if not (np.all(np.isfinite(g)) and worst <= bar):
            failures.append("%s: %.4f %s against a bar of %.4f" % (block, worst, ("u absolute", "ulp", "u relative")[column], bar))

    hold("rcp_nr", 1, hb.BAR_RCP_NR_ULP)
    hold("rcp_1nr", 2, bar_r1)
    hold("rsqrt_1nr", 2, bar_q1)
    hold("rsqrt_1nr_pos", 2, bar_q1)
    for block in ("sqrt_rsqrt root", "sqrt_rsqrt inv", "rsqrt_n<4>"):
        hold(block, 2, bar_g)
    assert not failures, "\n".join(failures)
    # semantics, exactly
    zero = int(np.flatnonzero(x == 0.0)[0])
    assert full["sqrt_rsqrt"][zero, 0] == 0.0 and not np.signbit(full["sqrt_rsqrt"][zero, 0])
    for block, v in (("sqrt_rsqrt inv", full["sqrt_rsqrt"][:, 1]), ("rsqrt_1nr", full["rsqrt_1nr"]), ("rsqrt_n<4>", full["rsqrt_n4"])):
        assert np.all(np.isfinite(v[n:]) & (v[n:] > 0.0)), block      # below the clamp, subnormals and 0: finite and positive
        env.note("%-16s below the clamp, subnormals and 0: %.4g .. %.4g; at 0: %.4g" % (block, v[n:].min(), v[n:].max(), v[zero]))
    assert np.all(np.isfinite(full["sqrt_rsqrt"][n:, 0]) & (full["sqrt_rsqrt"][n:, 0] >= 0.0))
    assert np.all(hb.same_bits(got["rsqrt_1nr"][0], got["rsqrt_1nr_pos"][0]))       # x >= 1e-300: the clamp changes nothing
    assert np.all(hb.same_bits(full["rsqrt_n4"], full["sqrt_rsqrt"][:, 1]))         # two texts of one algorithm, every input


def test_sine_and_cosine(env):
    names, sl, x = hb.sincos_sets()
    n = hb.sincos_contract()
    (sh, slo), (ch, clo) = hb.sincos_reference()
    table = hb.kconst_table()
    assert hb.table_is_correctly_rounded(table)
    one = hb.run("sincos_fast", x)
    got = {"sincos_fast": (one[:, 0], one[:, 1]), "sincos_fast_n<4>": hb.run4("sincos_fast_n4", x), "sincos_tab_n<4>": hb.run4("sincos_tab_n4", x, table)}
    for block, (s, c) in got.items():
        for name in names:
            env.figures(block + " sin", name, s, sh, slo, sl[name])
            env.figures(block + " cos", name, c, ch, clo, sl[name])
    failures = []
    for block, (s, c) in got.items():
        bar = hb.BAR_SINCOS_TAB_ABS_U if "tab" in block else hb.BAR_SINCOS_FAST_ABS_U
        for what, g, hi, lo in (("sin", s, sh, slo), ("cos", c, ch, clo)):
            a = hb.errors(g[:n], hi[:n], lo[:n])[0]
            i = int(np.argmax(a))
            if not (np.all(np.isfinite(g[:n])) and a[i] <= bar):
                failures.append("%s %s: %.4f u absolute at x = %r against a bar of %.1f" % (block, what, a[i], float(x[i]), bar))
    assert not failures, "\n".join(failures)
    # two texts of one algorithm: the same bits at every input, the out-of-contract set included
    assert np.all(hb.same_bits(got["sincos_fast"][0], got["sincos_fast_n<4>"][0])) and np.all(hb.same_bits(got["sincos_fast"][1], got["sincos_fast_n<4>"][1]))


def test_powers(env):
    x, n = hb.power_points()
    hi, lo = hb.power_reference()
    waves = hb.power_waves()
    by_pair = {}
    for name, (rows, idx) in waves.items():
        out = hb.run("pow_order", rows)
        v = np.empty(len(x))
        v[idx[idx >= 0]] = out[idx >= 0]
        by_pair[name] = v
    rows, idx = waves["uniform"]
    v = np.empty(len(x))
    v[idx] = hb.run("powi_uniform", rows)
    by_pair["powi_uniform"] = v
    failures = []
    for name, v in by_pair.items():
        rel = hb.errors(v, hi, lo)[2]
        for o in hb.INT_ORDERS:
            m = n == o
            env.figures("x^%d" % o, ("pow_order, %s wave" % name) if name != "powi_uniform" else name, v, hi, lo, m)
            if not (np.all(np.isfinite(v[m])) and rel[m].max() <= hb.bar_powi(o)):
                failures.append("%s, order %d: %.3f u relative against a bar of %d" % (name, o, rel[m].max(), hb.bar_powi(o)))
        if not (np.all(v[n == 0] == 1.0) and np.array_equal(v[n == 1], x[n == 1])):
            failures.append("%s: order 0 is not exactly 1, or order 1 not exactly x" % name)
    # path independence: a neighbour's order never changes mine
    for name in ("uniform", "mixed", "fractional"):
        same = hb.same_bits(by_pair[name], by_pair["powi_uniform"])
        if not np.all(same):
            i = int(np.flatnonzero(~same)[0])
            failures.append("pow_order in a %s wave differs from powi_uniform at %d points, first x = %r, order %d" % (name, int((~same).sum()), float(x[i]), int(n[i])))
    # the pow() path against the host libm's own error
    px, po = hb.pow_path_points()
    phi, plo = hb.pow_path_reference()
    got = hb.run("pow_order", np.stack([px, po], axis=1))
    host = hb.errors(np.power(px, po), phi, plo)[1]
    ulp = hb.errors(got, phi, plo)[1]
    for o in hb.POW_ORDERS:
        m = po == o
        R = float(host[m].max())
        bar = hp.K_MARGIN * max(1.0, R)
        env.figures("x^%g (pow)" % o, "host libm R = %.3f ulp, bar %.1f" % (R, bar), got, phi, plo, m)
        if not (np.all(np.isfinite(got[m])) and ulp[m].max() <= bar):
            failures.append("pow path, order %g: %.3f ulp against a bar of %.2f (host libm R = %.3f)" % (o, ulp[m].max(), bar, R))
    rec = hb.recorded_power_points()
    out = hb.run("pow_order", rec)
    for o in hb.RECORDED_ORDERS:
        m = (rec[:, 1] == o) | (np.isnan(rec[:, 1]) & np.isnan(o))
        env.note("x^%-14g recorded only, x in [0.5, 2]: %d finite, %d inf, %d NaN, %d zero" % (
            o, int(np.isfinite(out[m]).sum()), int(np.isinf(out[m]).sum()), int(np.isnan(out[m]).sum()), int((out[m] == 0.0).sum())))
    assert not failures, "\n".join(failures)


def test_arctangent(env):
    t = hb.atan_kernel_points()
    khi, klo = hb.atan_kernel_reference()
    got = hb.run("atan_kernel", t)
    env.figures("atan_kernel", "|t| <= tan(pi/8)", got, khi, klo)
    worst = float(hb.errors(got, khi, klo)[1].max())
    assert np.all(np.isfinite(got)) and worst <= hb.BAR_ATAN_KERNEL_ULP, worst
    names, sl, y, x = hb.atan2_sets()
    hi, lo = hb.atan2_reference()
    got = hb.run("atan2_pos", np.stack([y, x], axis=1))
    for name in names:
        env.figures("atan2_pos", name, got, hi, lo, sl[name])
    branch = hb.atan2_branches()
    ulp = hb.errors(got, hi, lo)[1]
    for b in range(8):
        env.figures("atan2_pos", "steep %d upper %d x < 0 %d" % (b >> 2, (b >> 1) & 1, b & 1), got, hi, lo, branch == b)
    i = int(np.argmax(ulp))
    assert np.all(np.isfinite(got)) and ulp[i] <= hb.BAR_ATAN2_ULP, (float(ulp[i]), float(y[i]), float(x[i]))
    # the exact cases
    ey, ex, eg = y[sl[hb.ATAN2_EXACT]], x[sl[hb.ATAN2_EXACT]], got[sl[hb.ATAN2_EXACT]]
    on_axis, up = ey == 0.0, ex == 0.0
    assert np.all(hb.same_bits(eg[on_axis & (ex >= 0.0)], np.zeros(int((on_axis & (ex >= 0.0)).sum()))))     # (0, 0) and (0, x > 0): +0
    assert np.all(hb.same_bits(eg[on_axis & (ex < 0.0)], np.full(int((on_axis & (ex < 0.0)).sum()), math.pi)))
    assert np.all(hb.same_bits(eg[up & ~on_axis], np.full(int((up & ~on_axis).sum()), math.pi / 2)))          # (y, +0) and (y, -0)
    assert int((on_axis & (ex < 0.0)).sum()) == 32 and int((up & ~on_axis).sum()) == 64 and np.signbit(ex[up & ~on_axis]).sum() == 32


def test_unfused(env):
    t = hb.unfused_triples()
    twice, once, prod = hb.unfused_reference()
    mac, mul = hb.run("mac_unfused", t), hb.run("mul_unfused", t[:, 1:])
    env.note("mac_unfused      %d triples, %d of them round differently fused: %d equal the two-rounding value, %d the fused one" % (
        len(t), int((~hb.same_bits(twice, once)).sum()), int(hb.same_bits(mac, twice).sum()), int(hb.same_bits(mac, once).sum())))
    env.note("mul_unfused      %d products: %d equal the rounded product" % (len(t), int(hb.same_bits(mul, prod).sum())))
    assert np.all(hb.same_bits(mac, twice))
    assert np.all(hb.same_bits(mul, prod))
