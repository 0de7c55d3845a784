"""The float64 device building blocks of vfclik_amd/csrc/vfik_device.h against a 50-digit reference: input sets, the error function, the
derived bars and the loader of the test-only harness (tests/device_blocks: libvfik_blocks.so, one trivial kernel out[i] = f(in[i]) per block).

A helper of the suite in the style of hp_reference.py, whose mpmath back end (50 digits; numpy.longdouble where mpmath is missing) it reuses.
tests/test_blocks_reference.py holds the helper itself on the CPU (the caps below, the error function against the host's libm, planted
faults that must exceed each bar); tests/test_gpu_blocks.py holds the kernels on the GPU.

THE UNIT.  u = 2^-53, the ulp of a value in [0.5, 1).  One rounding moves a value by at most half an ulp of its binade: at most 0.5 u
ABSOLUTE for a value below 1, and at most 1 u RELATIVE (half an ulp of a mantissa of 1.0; 0.5 u of a mantissa just under 2).  `errors`
returns the absolute error in u, the error in ulp of the reference value (np.spacing of its leading double) and the relative error in u,
from reference pairs (hi, lo), hi + lo = the 50-digit value to ~32 digits: no half ulp of a rounded reference is added.

THE BARS.  Derived, none measured on the code under test; e0 is the hardware seed's worst relative error, measured by the same test on the
same inputs (the seed is the hardware, not the code under test; an MI355X gave 4.2e-8 for v_rcp_f64 and 4.9e-8 for v_rsq_f64).

  rcp_nr            1 ulp of 1/x (BAR_RCP_NR_ULP), the header's claim.  One step takes a relative error e to e^2: from any seed within 1e-6
                    the first step leaves < 1e-12 + 1 u, the second (1e-12)^2; e = fma(-x, y, 1) is ~1e-16 and its own rounding ~1e-32.
                    What is left is the rounding of the last fma, half an ulp.
  rcp_1nr           relative e0^2 + 1.5 u (bar_rcp_1nr).  In exact arithmetic y (1 + e), e = 1 - x y, is (1 - e0^2) / x.  e is one fma of
                    magnitude <= e0: its rounding is <= u e0.  The last fma rounds once: <= 1 u relative.  0.5 u of margin.
  rsqrt_1nr(_pos)   relative 1.5 e0^2 + 2 u (bar_rsqrt_1nr).  With y = (1 + d) / sqrt(x): e = 1 - x y^2 = -2 d - d^2 and
                    y (1 + e / 2) = (1 - 1.5 d^2 - ...) / sqrt(x).  The product x y is rounded (<= 1 u relative) before the fma forms e
                    from it: e is off by <= 1 u absolute, its half reaches the result, 0.5 u.  0.5 y is exact.  The last fma: <= 1 u.
                    0.5 u of margin.
  sqrt_rsqrt,       relative 3.375 e0^4 + 2.5 u for the root and for the reciprocal root alike (bar_goldschmidt; the issue's ceiling is
  rsqrt_n           4 u).  g0 = fl(x y), h0 = y / 2 (exact); r = 0.5 - g h; g <- g + g r, h <- h + h r, twice; inv = 2 h (exact).  Write
                    g = sqrt(x) (1 + a), h = (1 + b) / (2 sqrt(x)): r = -(a + b) / 2 to first order and a step maps (a, b) to
                    ((a - b) / 2, (b - a) / 2) plus 1.5 ((a + b) / 2)^2 -- the COMMON error is squared away, the DIFFERENCE of the two
                    is only halved.  The seed's error is common: 1.5 e0^2 after one step, 1.5 (1.5 e0^2)^2 = 3.375 e0^4 after two.  The
                    roundings are not common.  Counted: the product g0 (<= 1 u relative, in g alone: difference 1 u, halved by the first
                    step and carried by the second as it is, since a = -b then: 0.5 u); the first step's two fmas, one in g and one in h
                    (difference <= 2 u, halved by the second step: 1 u); the last step's own fma of the result (1 u).  Both r are fmas of
                    magnitude <= 1e-8 and 1e-15, their roundings are below 1e-24.  0.5 + 1 + 1 = 2.5 u, no margin added.
  sincos_fast(_n)   absolute 2 u within |x| <= 1e5 (BAR_SINCOS_FAST_ABS_U): the reduction's last rounding, 0.5 u of r, times a derivative
                    <= 1; under 1 u for fdlibm's kernels on [-pi/4, pi/4] (they promise < 1 ulp GIVEN the reduction's tail, which this
                    code drops: that is the 0.5 u above); 0.5 u of margin.  A bit-exact CPU emulation gives 1.49.  The relative error in
                    ulp is recorded only (emulation: 1.67 at worst, 0.5 at the doubles nearest to k pi/2).
  sincos_tab_n      absolute 2.5 u within |x| <= 1e5 (BAR_SINCOS_TAB_ABS_U): the table entries S_k, C_k are rounded, 0.5 u times
                    |cos r| <= 1 plus 0.5 u times |sin r| <= 0.05; the product S cos r and the fma that adds C sin r round once each,
                    0.5 u each; the cosine polynomial 0.5 u (the sine's rounding is scaled by |r| <= 0.05 and the reduction's by the same
                    binade: inside the 0.475 u the sine terms leave unused).  Emulation: 1.74.  Relative: recorded only, unbounded near
                    the zeros by construction (the result is a difference of two rounded products there).
                    `k * head is exact for |x| < 1e5` is asserted on the host with exact integers (k_head_exact).
  integer powers    relative (n - 1) u (bar_powi), powi_uniform and both integer paths of pow_order.  First order: a product of two
                    factors with relative errors ea u and eb u has ea + eb + 1 (its own rounding, <= 1 u relative).  By induction
                    x^m carries <= m - 1: (a - 1) + (b - 1) + 1 = (a + b) - 1, whatever the order of the chain's multiplications.
                    (Emulation: 92 u at n = 127.)  n = 0 is exactly 1 and n = 1 exactly x: 1.0 * x is exact.
  pow() path        the library function is not ours to bound: R = the host libm's pow worst error in ulp against the same reference on
                    the same inputs, bar = hp_reference.K_MARGIN max(1, R) ulp (the rule of tests/test_gpu_far_angles.py).
  atan_kernel       1 ulp of the result on |t| <= tan(pi/8) (BAR_ATAN_KERNEL_ULP), the header's claim (fdlibm: < 1 ulp below 7/16).
  atan2_pos         4 ulp of the reference angle (BAR_ATAN2_ULP): t = num rcp_nr(den) carries 1.5 ulp (the reciprocal's 1, the product's
                    0.5) through a derivative <= 1 into a result that is no smaller than t's share of it; the kernel's own 1 ulp; up to
                    three additions of rounded constants (pi/4, pi/2, pi), 0.5 ulp each of a result that only grows from one to the next.
                    1.5 + 1 + 1.5 = 4.  (Emulation with rcp_nr at its bar: 2.96 ulp.)
  mac / mul_unfused equal, bit for bit, to the two-rounding value computed with exact rationals; a quarter of the triples at least round
                    differently when fused (cap), so a contracted build fails.

THE CAPS, asserted on the reference alone (tests/test_blocks_reference.py) before any measured figure is looked at: each of the eight
(steep, upper, x < 0) branch combinations of atan2_pos a correct evaluation takes holds >= 200 points; the nearest-to-k pi/2 set holds
>= 50 points with |x - k pi/2| < 1e-13; >= a quarter of the unfused triples differ fused / unfused; every point under a power bar has its
result and every square it uses in [1e-290, 1e290].

Every input set is seeded, at most 40 000 points a block, and cached at module level with its reference; the arrays are not to be written to."""
import ctypes
import functools
import math
import os
from fractions import Fraction

import numpy as np

import hp_reference as hp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = hp.U
_num = hp._num
if hp.BACKEND == "mpmath":
    import mpmath as _mpm
    _sqrt, _atan2, _power, _pi = _mpm.sqrt, _mpm.atan2, _mpm.power, _mpm.mp.pi

    def _sincos(x):
        c, s = _mpm.cos_sin(x)
        return s, c
else:
    _sqrt, _atan2, _power, _pi = np.sqrt, np.arctan2, np.power, np.longdouble("3.14159265358979323846264338327950288")

    def _sincos(x):
        return np.sin(x), np.cos(x)

BAR_RCP_NR_ULP = 1.0
BAR_SINCOS_FAST_ABS_U = 2.0
BAR_SINCOS_TAB_ABS_U = 2.5
BAR_ATAN_KERNEL_ULP = 1.0
BAR_ATAN2_ULP = 4.0
GOLDSCHMIDT_CEILING_U = 4.0
CLAMP = 1e-300
TAN_PI_8 = 0.41421356237309503      # the constant of atan2_pos
TAB_HEAD = 0.09817477042088285      # the 33-bit head of pi/32 of sincos_tab_n
TAB_SCALE = 10.185916357881302      # its 32/pi
INT_ORDERS = (0, 1, 2, 3, 5, 20, 31, 64, 127)
POW_ORDERS = (128.0, 3.5, 0.5, -1.0)
RECORDED_ORDERS = (2.0 ** 31, float("nan"))


def bar_rcp_1nr(e0):
    return e0 * e0 / U + 1.5


def bar_rsqrt_1nr(e0):
    return 1.5 * e0 * e0 / U + 2.0


def bar_goldschmidt(e0):
    return 3.375 * e0 ** 4 / U + 2.5


def bar_powi(n):
    return np.maximum(np.asarray(n, dtype=np.float64) - 1.0, 0.0)


# ---- the error function ----------------------------------------------------------------------------------------------------------------
def errors(got, hi, lo):
    """(absolute error in u, error in ulp of the reference value, relative error in u) per element; the reference is hi + lo.  A
    reference of exactly 0 has no ulp and no relative error: both are 0 where got is 0 too, else inf."""
    got, hi, lo = (np.asarray(a, dtype=np.float64) for a in (got, hi, lo))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        d = np.abs((got - hi) - lo)
        ulp = np.where(hi == 0.0, np.where(d == 0.0, 0.0, np.inf), d / np.spacing(np.abs(hi)))
        rel = np.where(hi == 0.0, np.where(d == 0.0, 0.0, np.inf), d / np.abs(hi + lo) / U)
        return d / U, ulp, rel


def _pairs(values):
    """(hi, lo) arrays of a list of high-precision values"""
    hi = np.array([float(v) for v in values], dtype=np.float64)
    lo = np.array([float(v - _num(h)) for v, h in zip(values, hi)], dtype=np.float64)
    return hi, lo


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


def _sets(d):
    """an ordered {name: array} -> (names, slices, one concatenated read-only array)"""
    names, sl, at = list(d), {}, 0
    for k in names:
        sl[k] = slice(at, at + len(d[k]))
        at += len(d[k])
    return names, sl, _frozen(np.concatenate([np.asarray(d[k], dtype=np.float64) for k in names]))


def _neighbours(x):
    x = np.asarray(x, dtype=np.float64)
    return np.concatenate([np.nextafter(x, -np.inf), x, np.nextafter(x, np.inf)])


def _log_uniform(rng, lo, hi, n):
    return 10.0 ** rng.uniform(math.log10(lo), math.log10(hi), n)


# ---- reciprocals and roots -------------------------------------------------------------------------------------------------------------
ROOT_ASSERTED = ("log-uniform", "powers of two", "above the clamp")
ROOT_SEMANTIC = ("below the clamp", "subnormals and 0")


@functools.lru_cache(maxsize=None)
def root_sets():
    """positive arguments (the reciprocals take both signs of the asserted sets): (names, slices, x)"""
    rng = np.random.default_rng(101)
    p2 = 2.0 ** np.arange(-996, 997, 7)
    above = np.concatenate([[CLAMP], CLAMP * (1.0 + _log_uniform(rng, 1e-16, 1.0, 63))])
    above[1] = np.nextafter(CLAMP, np.inf)
    below = np.concatenate([[np.nextafter(CLAMP, 0.0)], CLAMP * (1.0 - _log_uniform(rng, 1e-16, 0.9, 63))])
    sub = np.concatenate([[0.0, 5e-324, 2.2250738585072014e-308, np.nextafter(2.2250738585072014e-308, 0.0)], _log_uniform(rng, 1e-323, 2e-308, 60)])
    return _sets({"log-uniform": _log_uniform(rng, 1e-300, 1e300, 4096), "powers of two": _neighbours(p2)[_neighbours(p2) >= CLAMP],
                  "above the clamp": above, "below the clamp": below, "subnormals and 0": sub})


def root_asserted():
    """the slice of root_sets' x that is held to the bars (x >= 1e-300)"""
    names, sl, x = root_sets()
    n = sl[ROOT_ASSERTED[-1]].stop
    assert np.all(x[:n] >= CLAMP) and np.all(x[n:] < CLAMP)
    return n


@functools.lru_cache(maxsize=None)
def root_reference():
    """{rcp, rsqrt, sqrt: (hi, lo)} of the asserted arguments"""
    x = root_sets()[2][:root_asserted()]
    v = [_num(float(t)) for t in x]
    r = [_sqrt(t) for t in v]
    return {"rcp": _frozen(*_pairs([1 / t for t in v])), "rsqrt": _frozen(*_pairs([1 / t for t in r])), "sqrt": _frozen(*_pairs(r))}


# ---- sine / cosine ---------------------------------------------------------------------------------------------------------------------
SINCOS_OUTSIDE = "outside the contract"
K_PI_2_MAX = 63661


@functools.lru_cache(maxsize=None)
def sincos_sets():
    rng = np.random.default_rng(102)
    half_pi, node = _pi / 2, _pi / 32
    ks = np.arange(0, K_PI_2_MAX + 1, 29)
    near = np.array([float(half_pi * int(k)) * (1.0 if (k // 29) % 2 == 0 else -1.0) for k in ks])
    kk = np.arange(-700, 701)
    nodes = np.array([float(node * int(k)) for k in kk])
    ties = np.array([float(node * (2 * int(k) + 1) / 2) for k in kk])
    far = rng.uniform(9e4, 1e5, 3000) * rng.choice([-1.0, 1.0], 3000)
    return _sets({"uniform in +-pi": rng.uniform(-math.pi, math.pi, 3000), "uniform in +-64": rng.uniform(-64.0, 64.0, 3000),
                  "log-uniform 1e-300 .. 1e5": _log_uniform(rng, 1e-300, 1e5, 3000) * rng.choice([-1.0, 1.0], 3000),
                  "nearest to k pi/2": _neighbours(near), "nodes k pi/32": _neighbours(nodes), "ties (k + 1/2) pi/32": _neighbours(ties),
                  "9e4 .. 1e5": far, SINCOS_OUTSIDE: _log_uniform(rng, 1e5, 1e6, 2000) * rng.choice([-1.0, 1.0], 2000)})


def sincos_contract():
    """how many leading points of sincos_sets' x lie within |x| <= 1e5 (every set but the last)"""
    names, sl, x = sincos_sets()
    n = sl[SINCOS_OUTSIDE].start
    assert np.all(np.abs(x[:n]) <= 1e5) and np.all(np.abs(x[n:]) > 1e5)
    return n


@functools.lru_cache(maxsize=None)
def sincos_reference():
    """((s_hi, s_lo), (c_hi, c_lo)) at every point of sincos_sets"""
    sc = [_sincos(_num(float(t))) for t in sincos_sets()[2]]
    return _frozen(*_pairs([a for a, _ in sc])), _frozen(*_pairs([b for _, b in sc]))


def distance_to_k_pi_2(x):
    """|x - k pi/2| for the nearest k, at 50 digits"""
    half_pi = _pi / 2
    out = []
    for t in np.asarray(x, dtype=np.float64):
        v = _num(float(t))
        k = int(np.rint(t / (math.pi / 2)))
        out.append(float(abs(v - half_pi * k)))
    return np.array(out)


def tab_k(x):
    """k of sincos_tab_n: the fma x 32/pi + 1.5 2^52 is the EXACT sum rounded to an integer, ties to even"""
    c = Fraction(TAB_SCALE)
    out = []
    for t in np.asarray(x, dtype=np.float64):
        p = Fraction(float(t)) * c
        f = math.floor(p)
        r = p - f
        out.append(f + (1 if r > Fraction(1, 2) or (r == Fraction(1, 2) and f % 2 == 1) else 0))
    return np.array(out, dtype=np.int64)


def k_head_exact(ks):
    """k * head is a double: the integer mantissa of head times |k| has no more than 53 bits"""
    m, e = Fraction(TAB_HEAD).numerator, Fraction(TAB_HEAD).denominator
    assert e & (e - 1) == 0
    while m % 2 == 0:
        m //= 2
    return all((abs(int(k)) * m).bit_length() <= 53 for k in set(np.asarray(ks).tolist()))


def kconst_table(image=None):
    """the 64 x 2 doubles (sin, cos)(k pi/32) kconst_fill puts behind a chain's constants: the last KiB of an image (default: the LWR's of
    tests/golden/kconst_images.npz)"""
    if image is None:
        z = np.load(os.path.join(ROOT, "tests", "golden", "kconst_images.npz"))
        i = [str(n) for n in z["names"]].index("lwr")
        end = int(np.cumsum(z["lengths"])[i])
        image = z["images"][end - int(z["lengths"][i]):end]
    image = np.asarray(image, dtype=np.uint8)
    assert len(image) % 1024 == 0 and len(image) >= 2048
    return image[-1024:].copy().view("<f8").reshape(64, 2)


@functools.lru_cache(maxsize=None)
def table_reference():
    """the correctly rounded (sin, cos)(k pi/32), k = 0 .. 63; the four exact zeros (sin at k = 0, 32, cos at k = 16, 48) are 0"""
    t = np.array([[float(v) for v in _sincos(_pi * k / 32)] for k in range(64)])
    t[0, 0] = t[32, 0] = t[16, 1] = t[48, 1] = 0.0
    return _frozen(t)


TABLE_ZERO_RESIDUE = 2.0 ** -62


def table_is_correctly_rounded(table):
    """Every entry has the bits of the correctly rounded value -- but for the three zeros away from k = 0: kconst_fill takes sinl / cosl of
    k times the LONG DOUBLE pi / 32, whose own rounding (pi_L - pi = -5.0e-20) comes back as the value there, up to 48 / 32 of it times
    sinl's slope: at most 2^-62 = 2.2e-19 absolute, 0.002 u, against the 0.5 u the table's rounding has in sincos_tab_n's bar."""
    table = np.asarray(table, dtype=np.float64).reshape(64, 2)
    ref = table_reference()
    same = same_bits(table, ref)
    zeros = np.zeros((64, 2), dtype=bool)
    zeros[32, 0] = zeros[16, 1] = zeros[48, 1] = True
    return bool(np.all(same | (zeros & (np.abs(table) <= TABLE_ZERO_RESIDUE))) and np.all(same[~zeros]))


# ---- powers ----------------------------------------------------------------------------------------------------------------------------
N_PER_ORDER = 1024


def _power_x(rng, order, n):
    return _log_uniform(rng, 1e-3, 1e3, n) if abs(order) <= 20 else _log_uniform(rng, 0.5, 2.0, n)


@functools.lru_cache(maxsize=None)
def power_points():
    """(x, order) of the integer orders, N_PER_ORDER each, ordered so that pair j has order INT_ORDERS[j % 9]: (x [N], n [N])"""
    rng = np.random.default_rng(103)
    xs = {n: _power_x(rng, n, N_PER_ORDER) for n in INT_ORDERS}
    j = np.arange(N_PER_ORDER * len(INT_ORDERS))
    n = np.array(INT_ORDERS)[j % len(INT_ORDERS)]
    x = np.array([xs[int(o)][i // len(INT_ORDERS)] for i, o in zip(j, n)])
    return _frozen(x, n.astype(np.float64))


@functools.lru_cache(maxsize=None)
def power_reference():
    x, n = power_points()
    return _frozen(*_pairs([_num(float(a)) ** int(b) for a, b in zip(x, n)]))


def power_waves():
    """The three compositions of pow_order's input, each as (rows [M, 2], index [M] into power_points or -1 for a lane that is not one):
      uniform    every wave's 64 lanes share one order (pairs sorted by order; N_PER_ORDER is a multiple of 64)
      mixed      pair j in lane j mod 64: a wave cycles through all nine orders
      fractional 63 pairs in cycling order behind a lane 0 of order 3.5"""
    x, n = power_points()
    P = len(x)
    assert N_PER_ORDER % 64 == 0 and P % 64 == 0
    order = np.argsort(n, kind="stable")
    uni = (np.stack([x[order], n[order]], axis=1), order)
    mixed = (np.stack([x, n], axis=1), np.arange(P))
    waves = -(-P // 63)
    idx = np.full(waves * 64, -1, dtype=np.int64)
    rows = np.empty((waves * 64, 2))
    rows[:] = (1.5, 3.5)
    lanes = np.arange(waves * 64).reshape(waves, 64)[:, 1:].reshape(-1)[:P]
    idx[lanes] = np.arange(P)
    rows[lanes] = mixed[0]
    for w in range(waves):      # every wave of each composition is what its name says
        assert rows[64 * w, 1] == 3.5
    assert all(len(set(uni[0][64 * w:64 * w + 64, 1])) == 1 for w in range(P // 64))
    assert all(set(mixed[0][64 * w:64 * w + 64, 1]) == set(float(o) for o in INT_ORDERS) for w in range(P // 64))
    return {"uniform": uni, "mixed": mixed, "fractional": (rows, idx)}


def power_squares_in_range():
    """the cap: the result and every square b = x^(2^j) that order n's chain multiplies into it lie in [1e-290, 1e290]"""
    x, n = power_points()
    ref = power_reference()[0]
    ok = np.all((np.abs(ref) >= 1e-290) & (np.abs(ref) <= 1e290))
    lx = np.log10(x)
    for j in range(7):
        used = n.astype(np.int64) >= (1 << j)
        ok = ok and np.all(np.abs(lx[used]) * (1 << j) <= 290.0)
    return bool(ok)


@functools.lru_cache(maxsize=None)
def pow_path_points():
    """(x, order) of the pow() path: whole waves of one order each (every lane is fractional or out of the chain's range)"""
    rng = np.random.default_rng(104)
    x = np.concatenate([_power_x(rng, o, N_PER_ORDER) for o in POW_ORDERS])
    return _frozen(x, np.repeat(POW_ORDERS, N_PER_ORDER))


@functools.lru_cache(maxsize=None)
def pow_path_reference():
    x, o = pow_path_points()
    return _frozen(*_pairs([_power(_num(float(a)), _num(float(b))) for a, b in zip(x, o)]))


def recorded_power_points():
    """orders 2^31 and NaN, a wave each: recorded only"""
    rng = np.random.default_rng(105)
    return np.stack([np.tile(_log_uniform(rng, 0.5, 2.0, 64), 2), np.repeat(RECORDED_ORDERS, 64)], axis=1)


# ---- arctangent ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def atan_kernel_points():
    rng = np.random.default_rng(106)
    t = np.concatenate([rng.uniform(-TAN_PI_8, TAN_PI_8, 4000), _log_uniform(rng, 1e-300, TAN_PI_8, 1000) * rng.choice([-1.0, 1.0], 1000),
                        [0.0, TAN_PI_8, -TAN_PI_8, np.nextafter(TAN_PI_8, 0.0)]])
    return _frozen(t)


@functools.lru_cache(maxsize=None)
def atan_kernel_reference():
    zero = _num(0.0) + 1
    return _frozen(*_pairs([_atan2(_num(float(t)), zero) for t in atan_kernel_points()]))


ATAN2_EXACT = "exact cases"


@functools.lru_cache(maxsize=None)
def atan2_sets():
    """(names, slices, y, x): y >= 0 throughout"""
    rng = np.random.default_rng(107)
    th = rng.uniform(0.0, math.pi, 6000)
    rad = _log_uniform(rng, 1e-8, 1e3, 6000)
    centres = np.array([math.pi / 8, math.pi / 4, 3 * math.pi / 8, math.pi / 2, 5 * math.pi / 8, 3 * math.pi / 4, 7 * math.pi / 8, 0.0, math.pi])
    off = np.concatenate([s * m * 10.0 ** -np.arange(3, 17) for s in (-1.0, 1.0) for m in (1.0, 3.0)])
    tho = np.clip((centres[:, None, None] + off[None, :, None] + np.zeros((1, 1, 4))).reshape(-1), 0.0, None)
    rado = np.tile([1e-8, 1e-3, 1.0, 1e3], len(centres) * len(off))
    mags = _log_uniform(rng, 1e-8, 1e3, 32)
    ey = np.concatenate([[0.0], np.zeros(64), mags, mags, mags, mags])
    ex = np.concatenate([[0.0], mags, -mags, np.zeros(32), -np.zeros(32), mags, -mags])
    d = {"uniform": (np.abs(rad * np.sin(th)), rad * np.cos(th)), "around the branch angles": (np.abs(rado * np.sin(tho)), rado * np.cos(tho)),
         ATAN2_EXACT: (ey, ex)}
    names, sl, y = _sets({k: v[0] for k, v in d.items()})
    x = _frozen(np.concatenate([d[k][1] for k in names]))
    assert np.all(y >= 0.0)
    return names, sl, y, x


@functools.lru_cache(maxsize=None)
def atan2_reference():
    _, _, y, x = atan2_sets()
    return _frozen(*_pairs([_atan2(_num(float(a)), _num(float(b))) if (a != 0.0 or b != 0.0) else _num(0.0) for a, b in zip(y, x)]))


def atan2_branches():
    """per point the (steep, upper, x < 0) combination a correct evaluation takes, as 4 steep + 2 upper + neg; t at 50 digits"""
    _, _, y, x = atan2_sets()
    out = []
    for a, b in zip(y, x):
        ax = abs(b)
        steep = a > ax
        num, den = (ax, a) if steep else (a, ax)
        upper = den > 0.0 and _num(float(num)) / _num(float(den)) > _num(TAN_PI_8)
        out.append(4 * int(steep) + 2 * int(upper) + int(b < 0.0))
    return np.array(out)


# ---- unfused ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def unfused_triples():
    """(acc, x, w) [4096, 3] with acc ~ -x w: minus the rounded product, its neighbour, 2^-30 off it, and 2^-12 off it, in turn"""
    rng = np.random.default_rng(108)
    x, w = rng.uniform(-2.0, 2.0, 4096), rng.uniform(-2.0, 2.0, 4096)
    p = -(x * w)
    kind = np.arange(4096) % 4
    acc = np.where(kind == 0, p, np.where(kind == 1, np.nextafter(p, np.inf), np.where(kind == 2, p * (1.0 + 2.0 ** -30), p * (1.0 - 2.0 ** -12))))
    return _frozen(np.stack([acc, x, w], axis=1))


@functools.lru_cache(maxsize=None)
def unfused_reference():
    """(rounded twice, rounded once (fused), the rounded product), exact rationals rounded to nearest even by float()"""
    t = unfused_triples()
    twice = np.array([float(Fraction(a) + Fraction(float(Fraction(x) * Fraction(w)))) for a, x, w in t.tolist()])
    once = np.array([float(Fraction(a) + Fraction(x) * Fraction(w)) for a, x, w in t.tolist()])
    prod = np.array([float(Fraction(x) * Fraction(w)) for _, x, w in t.tolist()])
    return _frozen(twice, once, prod)


def same_bits(a, b):
    """element-wise equality of the bit patterns (distinguishes -0.0 from 0.0; a NaN equals itself)"""
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64) == np.ascontiguousarray(b, dtype=np.float64).view(np.uint64)


# ---- the harness -----------------------------------------------------------------------------------------------------------------------
# block name -> (id, input columns, output columns), the order of BLOCKS in tests/device_blocks/blocks.hip
BLOCKS = {name: (i, ic, oc) for i, (name, ic, oc) in enumerate((
    ("rcp_raw", 1, 1), ("rsq_raw", 1, 1), ("rcp_nr", 1, 1), ("rcp_1nr", 1, 1), ("rsqrt_1nr", 1, 1), ("rsqrt_1nr_pos", 1, 1),
    ("sqrt_rsqrt", 1, 2), ("rsqrt_n4", 4, 4), ("sincos_fast", 1, 2), ("sincos_fast_n4", 4, 8), ("sincos_tab_n4", 4, 8),
    ("powi_uniform", 2, 1), ("pow_order", 2, 1), ("atan_kernel", 1, 1), ("atan2_pos", 2, 1), ("mac_unfused", 3, 1), ("mul_unfused", 2, 1)))}
HARNESS = os.path.join(ROOT, "tests", "device_blocks", "libvfik_blocks.so")
_LIB = []


def load_harness():
    """libvfik_blocks.so as __graft_entry__.build() left it; a missing library is an error"""
    if not _LIB:
        lib = ctypes.CDLL(HARNESS)
        lib.vfik_blocks_run.restype = ctypes.c_int
        lib.vfik_blocks_run.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p]
        _LIB.append(lib)
    return _LIB[0]


def run(block, rows, table=None):
    """One launch: rows [M] or [M, input columns] -> [M, output columns] ([M] for one column).  Element i is lane i mod 64 of wave i div 64."""
    bid, ic, oc = BLOCKS[block]
    a = np.ascontiguousarray(rows, dtype=np.float64).reshape(-1, ic)
    out = np.full((len(a), oc), np.nan)
    tab = None if table is None else np.ascontiguousarray(table, dtype=np.float64)
    assert tab is None or tab.size == 128
    err = load_harness().vfik_blocks_run(bid, a.ctypes.data, ic, out.ctypes.data, len(a), None if tab is None else tab.ctypes.data)
    assert err == 0, "vfik_blocks_run(%s): HIP error %d" % (block, err)
    return out[:, 0] if oc == 1 else out


def run4(block, x, table=None):
    """the N = 4 forms on a flat argument list (padded with zeros to a multiple of four): [M] for rsqrt_n4, ([M], [M]) = (sin, cos) else"""
    x = np.asarray(x, dtype=np.float64)
    pad = np.concatenate([x, np.zeros(-len(x) % 4)]).reshape(-1, 4)
    out = run(block, pad, table)
    if out.shape[1] == 4:
        return out.reshape(-1)[:len(x)]
    return out[:, :4].reshape(-1)[:len(x)], out[:, 4:].reshape(-1)[:len(x)]
