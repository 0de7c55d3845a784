// vfik_device.h -- the float64 device building blocks every kernel of the library is made of: reciprocals, roots and the branch-free
// sincos, the rotation axis / angle, the goal attractor, the field slots (eval_slot and its reader of the quad planes), the nullspace module.
// No kernel and no host code; included INSIDE `namespace vfik { namespace {` by vfik_kernel.hip (the cycle kernels) and vfik_aux.hip
// (probe_kernel, track_kernel, monitor_kernel, mix_kernel), after vfik_kernel.h.
#pragma once

constexpr double EPS_LEN = 1e-12;  // lengths below this are zero (unit vector := 0)
constexpr double D_FLOOR = 1e-9;   // distance floor inside decay laws
constexpr double MAG_CAP = 1e6;    // cap of a repeller's magnitude

// ------------------------------------------------------------------------------------------------
// float64 building blocks.  On gfx950 one wave per SIMD issues a float64 FMA about every 5 cycles
// (8 when dependent), v_rcp/v_rsq_f64 take ~17-20, and the IEEE sequences the compiler emits for
// `a / b`, sqrt() and sincos() cost ~65, ~90-110 and ~370 cycles (tools/ubench_fp64.hip).  The
// control cycle needs none of their corner-case handling, so it uses Newton-refined reciprocals and
// a branch-free sincos that the scheduler can interleave across the independent joints.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ double rcp_nr(double x) {  // 1/x, ~1 ulp, x normal and non-zero
    double y = __builtin_amdgcn_rcp(x);
    double e = __builtin_fma(-x, y, 1.0);
    y = __builtin_fma(y, e, y);
    e = __builtin_fma(-x, y, 1.0);
    return __builtin_fma(y, e, y);
}

// The flange rotation from the tool pose, Rf = Rt Rtool^-1 (tl: rows 0..2 of the tool, row-major 3 x 4), where /pose_no_tool recomposes it.
// NOT Rt Rtool^T: a tool read from a float32 file or typed with four decimals is off a rotation by 5e-8 ... 1e-4, and the reference's frame
// product (KDL) assumes nothing of the nine numbers.  The inverse by cofactors, then row by row: a row of Rt dies as its row of Rf is formed,
// and the barriers keep the scheduler from interleaving the two phases (the long chains' variants have no registers for both at once).
// Good to a few ulp times the block's condition number -- the published frame is held to 1e-9.  A block without an inverse gives non-finite values.
__device__ __forceinline__ void flange_rotation(const double* Rt, const double* tl, double* Rf) {
    const double a = tl[0], b = tl[1], c = tl[2], d = tl[4], e = tl[5], f = tl[6], g = tl[8], h = tl[9], i = tl[10];
    double ti[9];
    ti[0] = __builtin_fma(e, i, -(f * h)); ti[3] = __builtin_fma(f, g, -(d * i)); ti[6] = __builtin_fma(d, h, -(e * g));
    const double r = rcp_nr(a * ti[0] + b * ti[3] + c * ti[6]);
    ti[1] = __builtin_fma(c, h, -(b * i)); ti[2] = __builtin_fma(b, f, -(c * e));
    ti[4] = __builtin_fma(a, i, -(c * g)); ti[5] = __builtin_fma(c, d, -(a * f));
    ti[7] = __builtin_fma(b, g, -(a * h)); ti[8] = __builtin_fma(a, e, -(b * d));
#pragma unroll
    for (int k = 0; k < 9; ++k) ti[k] *= r;
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const double x = Rt[3 * q], y = Rt[3 * q + 1], z = Rt[3 * q + 2];
#pragma unroll
        for (int k = 0; k < 3; ++k) Rf[3 * q + k] = x * ti[k] + y * ti[3 + k] + z * ti[6 + k];
        __builtin_amdgcn_sched_barrier(0);
    }
}

// 1/sqrt(x) from ONE Newton step on v_rsq_f64 (5 instructions): the decay repellers' 1 / D, which is raised to the decay order (up to 127).
// The step's error is measured directly by tools/ubench_rsqrt.hip (figures in DESIGN 6.2) and held by tests/test_gpu_blocks.py to
// 1.5 e0^2 + 2 u of the 50-digit value, e0 the worst error of v_rsq_f64 itself on the same arguments (profiles/device_blocks_accuracy.txt:
// e0 = 4.9e-8 over 1e-300 ... 1e300, the step leaves 32 u; rsqrt_1nr and rsqrt_1nr_pos agree bit for bit from 1e-300 up).  An error COMMON to the slots of one order is
// a common factor of their terms and leaves a normalised sum unchanged but for the goal's share; tests/test_gpu_field_edges.py bounds
// what the twist sees of it.  sqrt_rsqrt's two Goldschmidt steps (10 instructions) stay where the value itself is published.
// x = 0 gives a large finite value.
__device__ __forceinline__ double rsqrt_1nr(double x) {
    const double y = __builtin_amdgcn_rsq(fmax(x, 1e-300));
    const double e = __builtin_fma(-(x * y), y, 1.0);
    return __builtin_fma(0.5 * y, e, y);
}

__device__ __forceinline__ double rsqrt_1nr_pos(double x) {   // ... for x > 0 known to the caller (no clamp)
    const double y = __builtin_amdgcn_rsq(x);
    const double e = __builtin_fma(-(x * y), y, 1.0);
    return __builtin_fma(0.5 * y, e, y);
}

// 1/x from ONE Newton step on v_rcp_f64: the LDL^T pivots of the IK's normal matrix.  Measured on gfx950, not assumed: over all mantissas
// (tests/test_gpu_blocks.py, profiles/device_blocks_accuracy.txt) the raw v_rcp_f64 is off by up to 4.2e-8 relative, so one step leaves up to
// e0^2 = 1.8e-15 = 16 u -- NOT under the rounding of its own last fma, as this comment said while it took the seed's error for ~5e-9 (the
// figure of the conditioning sweep's build without the step: the joint velocities then miss the reference by 5e7 cond u); the test holds it
// to e0^2 + 1.5 u with e0 measured on the same arguments.  Against the 50-digit reference (tests/test_gpu_conditioning.py) the joint
// velocities are within 2.5 cond u at lambda = 0.1 and 2.1 cond u at lambda = 1e-2 and 1e-3 (cond up to 1.4e7, singular poses included),
// cond = (sigma_1^2 + lambda^2) / (sigma_6^2 + lambda^2), u = 2^-53; rcp_nr's second step gives 2.1 at every lambda, the C oracle's
// plain-double solve 0.5 - 1.5.  No bound on lambda or on cond enters: the test holds every lambda >= 0 it runs to 8 cond u.
__device__ __forceinline__ double rcp_1nr(double x) {
    const double y = __builtin_amdgcn_rcp(x);
    return __builtin_fma(y, __builtin_fma(-x, y, 1.0), y);
}

// sqrt(x) and 1/sqrt(x) together (Goldschmidt from v_rsq_f64).  x = 0 gives (0, large finite).
__device__ __forceinline__ void sqrt_rsqrt(double x, double& root, double& inv) {
    const double y = __builtin_amdgcn_rsq(fmax(x, 1e-300));
    double g = x * y, h = 0.5 * y;
    double r = __builtin_fma(-g, h, 0.5);
    g = __builtin_fma(g, r, g);
    h = __builtin_fma(h, r, h);
    r = __builtin_fma(-g, h, 0.5);
    g = __builtin_fma(g, r, g);
    h = __builtin_fma(h, r, h);
    root = g;
    inv = h + h;
}

// acc + x*w with the product and the sum rounded separately, as CPython evaluates
// `result[i] += v[i] * w` (command_mixer.py:81).  HIP's __dmul_rn/__dadd_rn are plain operators that
// the compiler may still fuse, so contraction is switched off for this statement block.
__device__ __forceinline__ double mac_unfused(double acc, double x, double w) {
#pragma clang fp contract(off)
    const double prod = x * w;
    return acc + prod;
}

__device__ __forceinline__ double mul_unfused(double x, double w) {
#pragma clang fp contract(off)
    return x * w;
}

// sin and cos: Cody-Waite reduction by pi/2 in three parts, then the classic minimax kernels on
// [-pi/4, pi/4] (coefficients of fdlibm's __kernel_sin / __kernel_cos).  Under 1.5 u ABSOLUTE (u = 2^-53) for |x| up to 1e5 rad, not "< 1 ulp":
// fdlibm's kernels keep that only when given the reduction's tail, which is dropped here, so the reduction's last rounding (0.5 u) adds to
// theirs; measured 1.52 u, held to 2 u by tests/test_gpu_blocks.py.  Relative: 0.5 ulp at the doubles nearest to k pi/2 (the three-part
// reduction keeps the small remainder exact), up to 1.6 ulp elsewhere (profiles/device_blocks_accuracy.txt).
// Joint angles live inside their limits (a few radians).  (The eight-lanes kernel's: not instantiated for the longer chains.)
[[maybe_unused]] __device__ __forceinline__ void sincos_fast(double x, double& s, double& c) {
    const double k = __builtin_rint(x * 6.36619772367581382433e-01);
    double r = __builtin_fma(-k, 1.57079632673412561417e+00, x);
    r = __builtin_fma(-k, 6.07710050630396597660e-11, r);
    r = __builtin_fma(-k, 2.02226624879595063154e-21, r);
    const double z = r * r;
    double ps = __builtin_fma(z, 1.58969099521155010221e-10, -2.50507602534068634195e-08);
    double pc = __builtin_fma(z, -1.13596475577881948265e-11, 2.08757232129817482790e-09);
    ps = __builtin_fma(z, ps, 2.75573137070700676789e-06);
    pc = __builtin_fma(z, pc, -2.75573143513906633035e-07);
    ps = __builtin_fma(z, ps, -1.98412698298579493134e-04);
    pc = __builtin_fma(z, pc, 2.48015872894767294178e-05);
    ps = __builtin_fma(z, ps, 8.33333333332248946124e-03);
    pc = __builtin_fma(z, pc, -1.38888888888741095749e-03);
    ps = __builtin_fma(z, ps, -1.66666666666666324348e-01);
    pc = __builtin_fma(z, pc, 4.16666666666666019037e-02);
    const double sr = __builtin_fma(z * r, ps, r);
    const double cr = __builtin_fma(z * z, pc, __builtin_fma(z, -0.5, 1.0));
    const int n = (int)k;
    const double sv = (n & 1) ? cr : sr, cv = (n & 1) ? sr : cr;
    s = (n & 2) ? -sv : sv;
    c = ((n + 1) & 2) ? -cv : cv;
}

// The same for N independent arguments, written operation by operation across the N (structure-of-
// arrays order): a lone wave issues a dependent float64 op every ~8 cycles but independent ones every
// ~5, and the scheduler mostly keeps source order, so the source is laid out interleaved.
template <int N>
__device__ __forceinline__ void sincos_fast_n(const double* x, double* s, double* c) {
    double k[N], r[N], z[N], ps[N], pc[N];
#pragma unroll
    for (int i = 0; i < N; ++i) k[i] = __builtin_rint(x[i] * 6.36619772367581382433e-01);
#pragma unroll
    for (int i = 0; i < N; ++i) r[i] = __builtin_fma(-k[i], 1.57079632673412561417e+00, x[i]);
#pragma unroll
    for (int i = 0; i < N; ++i) r[i] = __builtin_fma(-k[i], 6.07710050630396597660e-11, r[i]);
#pragma unroll
    for (int i = 0; i < N; ++i) r[i] = __builtin_fma(-k[i], 2.02226624879595063154e-21, r[i]);
#pragma unroll
    for (int i = 0; i < N; ++i) z[i] = r[i] * r[i];
#pragma unroll
    for (int i = 0; i < N; ++i) {
        ps[i] = __builtin_fma(z[i], 1.58969099521155010221e-10, -2.50507602534068634195e-08);
        pc[i] = __builtin_fma(z[i], -1.13596475577881948265e-11, 2.08757232129817482790e-09);
    }
#pragma unroll
    for (int i = 0; i < N; ++i) {
        ps[i] = __builtin_fma(z[i], ps[i], 2.75573137070700676789e-06);
        pc[i] = __builtin_fma(z[i], pc[i], -2.75573143513906633035e-07);
    }
#pragma unroll
    for (int i = 0; i < N; ++i) {
        ps[i] = __builtin_fma(z[i], ps[i], -1.98412698298579493134e-04);
        pc[i] = __builtin_fma(z[i], pc[i], 2.48015872894767294178e-05);
    }
#pragma unroll
    for (int i = 0; i < N; ++i) {
        ps[i] = __builtin_fma(z[i], ps[i], 8.33333333332248946124e-03);
        pc[i] = __builtin_fma(z[i], pc[i], -1.38888888888741095749e-03);
    }
#pragma unroll
    for (int i = 0; i < N; ++i) {
        ps[i] = __builtin_fma(z[i], ps[i], -1.66666666666666324348e-01);
        pc[i] = __builtin_fma(z[i], pc[i], 4.16666666666666019037e-02);
    }
    double zr[N], zz[N], hh[N];
#pragma unroll
    for (int i = 0; i < N; ++i) { zr[i] = z[i] * r[i]; zz[i] = z[i] * z[i]; hh[i] = __builtin_fma(z[i], -0.5, 1.0); }
#pragma unroll
    for (int i = 0; i < N; ++i) { ps[i] = __builtin_fma(zr[i], ps[i], r[i]); pc[i] = __builtin_fma(zz[i], pc[i], hh[i]); }
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const int n = (int)k[i];
        const double sv = (n & 1) ? pc[i] : ps[i], cv = (n & 1) ? ps[i] : pc[i];
        s[i] = (n & 2) ? -sv : sv;
        c[i] = ((n + 1) & 2) ? -cv : cv;
    }
}

// sin and cos of N independent arguments through a 64-entry table: x = k pi/32 + r, |r| <= pi/64, and
//   sin x = S_k cos r + C_k sin r,   cos x = C_k cos r - S_k sin r
// with (S_k, C_k) = (sin, cos)(k pi/32) read from the wave's LDS copy of the table (one 16-byte read per angle, index
// k mod 64) and Taylor polynomials that are exact to the last bit on so short an interval (r^9/9! < 1e-16 r,
// r^10/10! < 3e-20).  23 instructions an angle against 33 for the pi/2 reduction above, whose minimax kernels need
// six coefficients each and a sign / swap selection by quadrant; ~2 u ABSOLUTE, u = 2^-53 (the table entries are rounded; measured
// 1.8 u, held to 2.5 u by tests/test_gpu_blocks.py) and NO relative bound near the zeros of sin and cos, where the result is the difference
// of two rounded products (1e15 ulp at the double nearest to a zero; sincos_fast keeps 0.5 ulp there).  pi/32 is
// split into a 33-bit head, so that k * head is exact for |x| < 1e5 rad (asserted in tests/test_blocks_reference.py), and a tail.
template <int N>
__device__ __forceinline__ void sincos_tab_n(const double* x, const char* tab, double* s, double* c) {
    typedef double d2 __attribute__((ext_vector_type(2)));
    // k = rint(x 32/pi) by the magic-number addition: x 32/pi + 1.5 2^52 rounds to an integer, whose low bits are the low dword of
    // the sum (two's complement, |k| < 2^31) -- one fma and one and for the table index where rint, cvt_i32 and and were.
    constexpr double MAGIC = 6755399441055744.0;
    double k[N], r[N], z[N], ps[N], pc[N], S[N], C[N], km[N];
#pragma unroll
    for (int i = 0; i < N; ++i) km[i] = __builtin_fma(x[i], 10.185916357881302, MAGIC);
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const d2 t = *reinterpret_cast<const d2*>(tab + ((unsigned)__double2loint(km[i]) & 63u) * 16);
        S[i] = t.x; C[i] = t.y;
    }
#pragma unroll
    for (int i = 0; i < N; ++i) k[i] = km[i] - MAGIC;
#pragma unroll
    for (int i = 0; i < N; ++i) r[i] = __builtin_fma(-k[i], 0.09817477042088285, x[i]);
#pragma unroll
    for (int i = 0; i < N; ++i) r[i] = __builtin_fma(-k[i], 3.79818781656637e-12, r[i]);
#pragma unroll
    for (int i = 0; i < N; ++i) z[i] = r[i] * r[i];
#pragma unroll
    for (int i = 0; i < N; ++i) {
        ps[i] = __builtin_fma(z[i], -1.98412698412698412698e-04, 8.33333333333333333333e-03);
        pc[i] = __builtin_fma(z[i], 2.48015873015873015873e-05, -1.38888888888888888889e-03);
    }
#pragma unroll
    for (int i = 0; i < N; ++i) {
        ps[i] = __builtin_fma(z[i], ps[i], -1.66666666666666666667e-01);
        pc[i] = __builtin_fma(z[i], pc[i], 4.16666666666666666667e-02);
    }
    double zr[N];
#pragma unroll
    for (int i = 0; i < N; ++i) { zr[i] = z[i] * r[i]; pc[i] = __builtin_fma(z[i], pc[i], -0.5); }
#pragma unroll
    for (int i = 0; i < N; ++i) { ps[i] = __builtin_fma(zr[i], ps[i], r[i]); pc[i] = __builtin_fma(z[i], pc[i], 1.0); }  // sin r, cos r
#pragma unroll
    for (int i = 0; i < N; ++i) { s[i] = S[i] * pc[i]; c[i] = C[i] * pc[i]; }
#pragma unroll
    for (int i = 0; i < N; ++i) { s[i] = __builtin_fma(C[i], ps[i], s[i]); c[i] = __builtin_fma(-S[i], ps[i], c[i]); }
}

// N independent 1/sqrt(x), operation by operation (x = 0 gives a large finite value)
template <int N>
__device__ __forceinline__ void rsqrt_n(const double* x, double* inv) {
    double y[N], g[N], h[N], r[N];
#pragma unroll
    for (int i = 0; i < N; ++i) y[i] = __builtin_amdgcn_rsq(fmax(x[i], 1e-300));
#pragma unroll
    for (int i = 0; i < N; ++i) { g[i] = x[i] * y[i]; h[i] = 0.5 * y[i]; }
#pragma unroll
    for (int i = 0; i < N; ++i) r[i] = __builtin_fma(-g[i], h[i], 0.5);
#pragma unroll
    for (int i = 0; i < N; ++i) { g[i] = __builtin_fma(g[i], r[i], g[i]); h[i] = __builtin_fma(h[i], r[i], h[i]); }
#pragma unroll
    for (int i = 0; i < N; ++i) r[i] = __builtin_fma(-g[i], h[i], 0.5);
#pragma unroll
    for (int i = 0; i < N; ++i) inv[i] = 2.0 * __builtin_fma(h[i], r[i], h[i]);
}

// x^n, n a wave-uniform small non-negative integer: square-and-multiply with scalar control flow
__device__ __forceinline__ double powi_uniform(double x, int n) {
    double r = 1.0, b = x;
    while (n) {
        if (n & 1) r *= b;
        n >>= 1;
        if (n) b *= b;
    }
    return r;
}

// x^order for x > 0.  Decay orders are small integers in every message the reference sends
// (object_feeder:277,279,302; README.old:75 uses 20): multiply chain when we can, pow() otherwise.
__device__ __forceinline__ double pow_order(double x, double order) {
    const int n = (int)order;
    const bool isint = (double)n == order && n >= 0 && n < 128;
    if (__all(isint)) {
        const int n0 = __builtin_amdgcn_readfirstlane(n);
        if (__all(n == n0)) return powi_uniform(x, n0);
        double r = 1.0, b = x;
#pragma unroll
        for (int k = 0; k < 7; ++k) {
            r = (n & (1 << k)) ? r * b : r;
            b = b * b;
        }
        return r;
    }
    return isint ? powi_uniform(x, n) : pow(x, order);
}

// atan(t), |t| <= tan(pi/8): fdlibm's 11-coefficient kernel (s_atan.c, good to < 1 ulp for |t| < 7/16)
__device__ __forceinline__ double atan_kernel(double t) {
    const double z = t * t, w = z * z;
    const double s1 = z * (3.33333333333329318027e-01 + w * (1.42857142725034663711e-01 + w * (9.09088713343650656196e-02 +
                      w * (6.66107313738753120669e-02 + w * (4.97687799461593236017e-02 + w * 1.62858201153657823623e-02)))));
    const double s2 = w * (-1.99999999998764832476e-01 + w * (-1.11111104054623557880e-01 + w * (-7.69187620504482999495e-02 +
                      w * (-5.83357013379057348645e-02 + w * -3.65315727442169155270e-02))));
    return t - t * (s1 + s2);
}

// atan2(y, x) for y >= 0 (an angle in [0, pi]), branch-free: two reductions bring the argument of the
// arctangent below tan(pi/8), where atan_kernel (above) is good to < 1 ulp.
// ocml's atan2 costs a lone wave ~2 000 cycles (tools/stamps.py: the waves that needed it ended the kernel
// 0.4 us after the rest); this is ~45 instructions.
__device__ __forceinline__ double atan2_pos(double y, double x) {
    const double ax = fabs(x);
    const bool steep = y > ax;                         // angle from the nearer axis: t in [0, 1]
    const double num = steep ? ax : y, den = steep ? y : ax;
    double t = den > 0.0 ? num * rcp_nr(den) : 0.0;    // atan2(0, 0) = 0
    const bool upper = t > 0.41421356237309503;        // tan(pi/8): atan(t) = pi/4 + atan((t - 1) / (t + 1))
    const double tr = (t - 1.0) * rcp_nr(t + 1.0);
    t = upper ? tr : t;
    double a = atan_kernel(t);
    a = upper ? 0.78539816339744830962 + a : a;        // angle from the nearer axis, in [0, pi/4]
    a = steep ? 1.57079632679489661923 - a : a;        // angle from the x axis of (|x|, y)
    return x < 0.0 ? 3.14159265358979323846 - a : a;
}

// Unit rotation axis (base frame) and angle of the rotation taking R to G, i.e. of log(G R^T) =
// KDL diff(R, G).rot.  Branch-free main line; the half-turn neighbourhood (sin(theta) < 1e-4, cos < 0),
// where the antisymmetric part vanishes, is fixed up from the symmetric part under a wave-uniform
// test.  The angle itself is only needed below the slow-down angle: `need_theta` (wave-uniform) says
// whether any lane can be that close; otherwise theta is reported as pi (any value >= rot_slow does).
// A slow-down angle below pi/8 (cos_slow > cos(pi/8); the default is 0.3) makes that evaluation short: a lane inside the angle has
// s / c <= tan(rot_slow) < tan(pi/8), so neither reduction of atan2_pos can fire for it -- its second reciprocal, the selects and
// the three additions go, the lane's own operations stay as they were (bit for bit); a lane outside the angle keeps pi.  The waves
// that get here end the launch: one in eleven of a batch of random goals has such a lane, and every launch waits for its slowest wave.
// This takes s^2 + c^2 = 1, i.e. goal and tool rotations that ARE rotations (float32 rounding of the goal moves s / c by 1e-7).  A scaled
// or skewed goal matrix can have c > cos_slow with s / c above tan(pi/8): atan_kernel is then off its interval (still < 1 ulp up
// to 7/16, degrading beyond), where atan2_pos reduced any (s, c); the value feeds min(1, theta / rot_slow) alone.
// (SHORT = false: without that short evaluation -- the general field path's variants, which sit at their register limit)
template <bool SHORT>
__device__ __forceinline__ void rot_axis_angle(const double* R, const double* G, double cos_slow, double* axis, double& theta,
                                               bool& has_axis) {
    double E[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) E[3 * i + j] = G[3 * i] * R[3 * j] + G[3 * i + 1] * R[3 * j + 1] + G[3 * i + 2] * R[3 * j + 2];
    const double a0 = 0.5 * (E[7] - E[5]), a1 = 0.5 * (E[2] - E[6]), a2 = 0.5 * (E[3] - E[1]);
    const double c = 0.5 * (E[0] + E[4] + E[8] - 1.0);
    double s, sinv;
    sqrt_rsqrt(a0 * a0 + a1 * a1 + a2 * a2, s, sinv);
    axis[0] = a0 * sinv; axis[1] = a1 * sinv; axis[2] = a2 * sinv;
    has_axis = s >= EPS_LEN;
    theta = 3.14159265358979323846;
    if (__any(c > cos_slow)) {  // some lane is within the slow-down angle
        if (SHORT && cos_slow > 0.92387953251128674) {  // cos(pi/8): wave-uniform
            const double th = atan_kernel(s * rcp_nr(c));
            theta = c > cos_slow ? th : theta;
        } else {
            theta = atan2_pos(s, c);
        }
    }
    const bool half_turn = s < 1e-4 && c < 0.0;
    if (__any(half_turn)) {
        // theta near pi (4 arms in 65 536 random goals): the axis comes from the symmetric part,
        // (E + E^T)/2 - c I = (1 - c) a a^T, whose row with the largest diagonal element is parallel to a;
        // the sign from the (small) antisymmetric part.  Selects, one rsqrt: the waves that get here
        // used to end the kernel 0.3 us after the others through three divergent branches with divisions.
        const bool k0 = E[0] >= E[4] && E[0] >= E[8], k1 = !k0 && E[4] >= E[8];
        const double s01 = 0.5 * (E[1] + E[3]), s02 = 0.5 * (E[2] + E[6]), s12 = 0.5 * (E[5] + E[7]);
        double x = k0 ? E[0] - c : (k1 ? s01 : s02);
        double y = k0 ? s01 : (k1 ? E[4] - c : s12);
        double z = k0 ? s02 : (k1 ? s12 : E[8] - c);
        const double flip = (x * a0 + y * a1 + z * a2 < 0.0) ? -1.0 : 1.0;
        double nn, k;
        sqrt_rsqrt(x * x + y * y + z * z, nn, k);
        k *= flip;
        if (half_turn) {
            axis[0] = x * k; axis[1] = y * k; axis[2] = z * k;
            has_axis = true;
            // pi - atan(s / |c|), s / |c| < 1.0001e-4: atan(t) = t - t^3 / 3 to 2e-21, within an ulp of pi of atan2_pos(s, c)
            const double t = s * rcp_nr(-c);
            theta = 3.14159265358979323846 - t * __builtin_fma(t * t, -3.33333333333333333333e-01, 1.0);
        }
    }
}

// type 1, point attractor: G = goal rotation (9) + position (3); adds force*vector to tot, scales sc.
// `on` masks the whole contribution (goal block absent): selects instead of a branch.
// SHORT (the straight-line variants and the eight-lanes kernel): rot_axis_angle's short arctangent, and 1 / rot_slow from the caller
// (`rot_slow_inv`: the batch constant); without it the reciprocal is formed here and the argument is not read.
template <bool SHORT = true>
__device__ __forceinline__ void attractor(const double* R, const double* p, const double* GR, const double* Gp,
                                          double slow, double force, double rot_slow, double cos_slow, bool on,
                                          double* tot, double* sc, double* dist = nullptr, double rot_slow_inv = 0.0) {
    const double dx = Gp[0] - p[0], dy = Gp[1] - p[1], dz = Gp[2] - p[2];
    double D, Dinv;
    sqrt_rsqrt(dx * dx + dy * dy + dz * dz, D, Dinv);
    const double kt = (on && D > EPS_LEN) ? force * Dinv : 0.0;
    tot[0] += dx * kt; tot[1] += dy * kt; tot[2] += dz * kt;
    double ax[3], th;
    bool has_axis;
    rot_axis_angle<SHORT>(R, GR, cos_slow, ax, th, has_axis);
    const bool rot_on = on && has_axis && th > EPS_LEN;  // selects, not a multiply by 0: an absent goal's axis may be NaN
    tot[3] += rot_on ? ax[0] * force : 0.0; tot[4] += rot_on ? ax[1] * force : 0.0; tot[5] += rot_on ? ax[2] * force : 0.0;
    const double s0 = slow > 0.0 ? fmin(1.0, D * rcp_nr(slow)) : 1.0;
    const double s1 = rot_slow > 0.0 ? fmin(1.0, th * (SHORT ? rot_slow_inv : rcp_nr(rot_slow))) : 1.0;
    sc[0] *= on ? s0 : 1.0;
    sc[1] *= on ? s1 : 1.0;
    if (dist) { dist[0] = D; dist[1] = th; }
}

// Element e (0..7) of slot m of this lane's arm in the quad-plane layout (vfik_kernel.h): plane
// 2m + e/4, component e%4.  sq points at plane 0, component 0 of the lane's arm; Q = plane pitch in
// elements (4 * Bpad).
template <typename T>
__device__ __forceinline__ double slot_elem(const T* sq, long Q, int m, int e) {
    return (double)sq[(long)(2 * m + (e >> 2)) * Q + (e & 3)];
}

// One field slot of any type, read from memory (the general path: mixed primitive types in a wave,
// fractional decay orders, more slots than the prefetch window).
// `rd(m, e)` = element e of slot m: SlotGlobal reads the quad planes in memory, SlotLds the rows staged in LDS.
template <typename RD>
__device__ void eval_slot(const RD& rd, int m, const double* Rt, const double* pt, double rot_slow, double cos_slow,
                          double* tot, double* sc) {
    const int type = (int)rd(m, 7);
    if (type <= 0) return;
    const double p0 = rd(m, 0), p1 = rd(m, 1), p2 = rd(m, 2),
                 p3 = rd(m, 3), p4 = rd(m, 4), p5 = rd(m, 5),
                 force = rd(m, 6);
    if (type == VFIK_FIELD_REPELLER) {  // x y z radius safeDist order
        const double dx = p0 - pt[0], dy = p1 - pt[1], dz = p2 - pt[2];
        double D, Dinv;
        sqrt_rsqrt(dx * dx + dy * dy + dz * dz, D, Dinv);
        Dinv = D < D_FLOOR ? 1.0 / D_FLOOR : Dinv;
        const double mag = fmin(pow_order((p3 + p4) * Dinv, p5), MAG_CAP);
        const double k = force * mag * Dinv;
        tot[0] += dx * k; tot[1] += dy * k; tot[2] += dz * k;
    } else if (type == VFIK_FIELD_HEMISPHERE) {  // x y z nx ny nz | safeDist order
        const double safe = rd(m + 1, 0), order = rd(m + 1, 1);
        double nn, ninv;
        sqrt_rsqrt(p3 * p3 + p4 * p4 + p5 * p5, nn, ninv);
        if (nn > EPS_LEN) {
            const double h = ((pt[0] - p0) * p3 + (pt[1] - p1) * p4 + (pt[2] - p2) * p5) * ninv;
            const double mag = fmin(pow_order(safe * rcp_nr(fmax(h, D_FLOOR)), order), MAG_CAP);
            const double k = -force * mag * ninv;
            tot[0] += p3 * k; tot[1] += p4 * k; tot[2] += p5 * k;
        }
    } else if (type == VFIK_FIELD_FUNNEL) {  // x y z ax ay az | cutAngle angleOrder cutDist distOrder
        const double cutA = rd(m + 1, 0), ordA = rd(m + 1, 1),
                     cutD = rd(m + 1, 2), ordD = rd(m + 1, 3);
        double an, ainv;
        sqrt_rsqrt(p3 * p3 + p4 * p4 + p5 * p5, an, ainv);
        if (an > EPS_LEN) {
            const double ax = p3 * ainv, ay = p4 * ainv, az = p5 * ainv;
            const double wx = pt[0] - p0, wy = pt[1] - p1, wz = pt[2] - p2;
            const double along = wx * ax + wy * ay + wz * az;
            const double ex = wx - along * ax, ey = wy - along * ay, ez = wz - along * az;
            double P, Pinv, dist, dinv;
            sqrt_rsqrt(ex * ex + ey * ey + ez * ez, P, Pinv);
            sqrt_rsqrt(wx * wx + wy * wy + wz * wz, dist, dinv);
            Pinv = P < D_FLOOR ? 1.0 / D_FLOOR : Pinv;
            dinv = dist < D_FLOOR ? 1.0 / D_FLOOR : dinv;
            const double phi = atan2_pos(P, along);
            const double ga = cutA > 0.0 ? fmin(1.0, pow_order(phi * rcp_nr(cutA), ordA)) : 1.0;
            const double gd = fmin(1.0, pow_order(cutD * dinv, ordD));
            const double k = -force * ga * gd * Pinv;
            tot[0] += ex * k; tot[1] += ey * k; tot[2] += ez * k;
        }
    } else if (type == VFIK_FIELD_ATTRACTOR) {  // a second attractor: frame16 + slow over 3 slots
        double GR[9], Gp[3];
        GR[0] = p0; GR[1] = p1; GR[2] = p2; Gp[0] = p3; GR[3] = p4; GR[4] = p5;
        GR[5] = rd(m + 1, 0); Gp[1] = rd(m + 1, 1);
        GR[6] = rd(m + 1, 2); GR[7] = rd(m + 1, 3); GR[8] = rd(m + 1, 4);
        Gp[2] = rd(m + 1, 5);
        attractor<false>(Rt, pt, GR, Gp, rd(m + 2, 4), force, rot_slow, cos_slow, true, tot, sc);
    }
}


// ------------------------------------------------------------------------------------------------
// Nullspace module, chains of up to 7 joints (scripts/nullspace:75-117), shared by cycle_kernel and cycle_sub8_kernel.
// In: Jm = the Jacobian by columns (destroyed: its rows are orthonormalised in place), the arm's sign memory
// (lv_r = lastvec, sig_r = sig, has_vec: lastvec holds a vector), c0 = /control[0], jl_task + descent(z) = the
// joint-limit task's direction.  Out: qn = move_in_nullspace (+ the projected joint-limit task), before check_limits and
// the gain; status bits; returns true when the sign memory was advanced (a unique nullspace direction exists).
// Every decision is taken PER LANE (per arm): which path an arm takes never depends on the other arms of its wave, so
// its result does not depend on where in a batch it sits (wave-wide votes only decide whether a path is executed at all).
// ------------------------------------------------------------------------------------------------
// ZFIRST / ZLAST: the Jacobian's first column is (x, y, 0, 0, 0, 1) / its last column (0, 0, 0, z) -- structural zeros of the chain's DH
// pattern (cycle_body: jzero).  The Gram-Schmidt pass tracks which entries are still exactly zero (a compile-time table once the loops are
// unrolled) and skips their terms: the last column's linear part stays zero to the end, the first column's zeros fill in at the first
// two steps -- 44 of the module's ~550 operations.
template <int NJ, bool ZFIRST = false, bool ZLAST = false, typename ZF>
__device__ __forceinline__ bool nullspace_core(double (&Jm)[NJ][6], double* lv_r, int& sig_r, bool& has_vec, double c0, bool jl_task,
                                               ZF&& descent, double* qn, int& status) {
    // Orthonormal basis (rows) of the row space of J by modified Gram-Schmidt, in place in Jm:
    // afterwards I - Q^T Q is restrict(I6, J) = I - pinv(J) J (nullspace:75-79).
    // One pass: loss of orthogonality ~ eps * cond(J), far below the 1e-6 bar wherever J is usable.
    // Right-looking order: once row s is normalised, the projections of ALL later rows onto it are
    // independent chains (5, 4, ... of them) that a lone wave can interleave; row by row (left-looking) the
    // same operations are one serial chain of 7-term dot products (dependent float64 ops issue every ~8
    // cycles, independent ones every ~5).  Same arithmetic, same order per row: same results.
    bool Z[NJ][6];   // entry (column i, row r) of J is still structurally zero
#pragma unroll
    for (int i = 0; i < NJ; ++i)
#pragma unroll
        for (int r = 0; r < 6; ++r) Z[i][r] = (ZFIRST && i == 0 && (r == 2 || r == 3 || r == 4)) || (ZLAST && i == NJ - 1 && r < 3);
    int rank = 0;
    double n0[6];  // squared norms of the rows of J: the rank test's yardstick
#pragma unroll
    for (int r = 0; r < 6; ++r) n0[r] = 0.0;
#pragma unroll
    for (int i = 0; i < NJ; ++i)
#pragma unroll
        for (int r = 0; r < 6; ++r)
            if (!Z[i][r]) n0[r] = __builtin_fma(Jm[i][r], Jm[i][r], n0[r]);
#pragma unroll
    for (int s = 0; s < 6; ++s) {
        double n1 = 0.0;
        if (s == 0) {
            n1 = n0[0];  // nothing has been projected out of the first row
        } else {
#pragma unroll
            for (int i = 0; i < NJ; ++i)
                if (!Z[i][s]) n1 += Jm[i][s] * Jm[i][s];
        }
        const bool keep = n1 > 1e-24 * n0[s] && n0[s] > 0.0;
        double n1r, n1i;
        sqrt_rsqrt(n1, n1r, n1i);
        const double inv = keep ? n1i : 0.0;
        rank += keep ? 1 : 0;
#pragma unroll
        for (int i = 0; i < NJ; ++i)
            if (!Z[i][s]) Jm[i][s] *= inv;
        double c[6];
#pragma unroll
        for (int r = s + 1; r < 6; ++r) c[r] = 0.0;
#pragma unroll
        for (int i = 0; i < NJ; ++i)
#pragma unroll
            for (int r = s + 1; r < 6; ++r)
                if (!Z[i][s] && !Z[i][r]) c[r] += Jm[i][s] * Jm[i][r];
#pragma unroll
        for (int i = 0; i < NJ; ++i)
#pragma unroll
            for (int r = s + 1; r < 6; ++r) {
                if (Z[i][s]) continue;                 // nothing of row s in this column
                if (Z[i][r]) { Jm[i][r] = -(c[r] * Jm[i][s]); Z[i][r] = false; }
                else Jm[i][r] -= c[r] * Jm[i][s];
            }
    }
    const int nullity = NJ - rank;
    bool advanced = false;
    if (nullity == 1) {
        double u[NJ];
        // u <- (I - Q^T Q) u: all six coefficients first (independent dot products), then the update (classical
        // Gram-Schmidt against an orthonormal Q); returns the largest |coefficient| = how much of u was row space
        auto project = [&](double* x) {
            double c[6];
#pragma unroll
            for (int r = 0; r < 6; ++r) c[r] = 0.0;
#pragma unroll
            for (int i = 0; i < NJ; ++i)
#pragma unroll
                for (int r = 0; r < 6; ++r)
                    if (!Z[i][r]) c[r] += Jm[i][r] * x[i];
#pragma unroll
            for (int r = 0; r < 6; ++r)
#pragma unroll
                for (int i = 0; i < NJ; ++i)
                    if (!Z[i][r]) x[i] -= c[r] * Jm[i][r];
            double cm = fabs(c[0]);
#pragma unroll
            for (int r = 1; r < 6; ++r) cm = fmax(cm, fabs(c[r]));
            return cm;
        };
        auto norm2 = [&](const double* x) {
            double n = 0.0;
#pragma unroll
            for (int i = 0; i < NJ; ++i) n += x[i] * x[i];
            return n;
        };
        double nn = 0.0;
        // Warm start: the nullspace direction turns little between two control cycles, so last cycle's vector
        // (the sign memory, nullspace:92,104) is projected instead of a unit vector: no search for the best
        // unit vector, and ONE projection suffices when it removes little (its residual row-space part is
        // ~ eps cond(J) times what was removed).  An arm without a usable previous vector (first cycle, a
        // jump that leaves less than half of it) takes the cold path below.
        bool warm = false;
        if (__any(has_vec)) {  // (a stored vector is a unit vector)
#pragma unroll
            for (int i = 0; i < NJ; ++i) u[i] = lv_r[i];
            const double cm = project(u);
            nn = norm2(u);
            warm = has_vec && nn > 0.25;
            const bool again = warm && cm > 1e-2;  // a real move: project once more, as the cold path does
            if (__any(again)) {
                double u2[NJ];
#pragma unroll
                for (int i = 0; i < NJ; ++i) u2[i] = u[i];
                project(u2);
                const double nn2 = norm2(u2);
#pragma unroll
                for (int i = 0; i < NJ; ++i) u[i] = again ? u2[i] : u[i];
                nn = again ? nn2 : nn;
            }
        }
        if (__any(!warm)) {
            // cold: the normalised column of the projector with the largest diagonal, projected twice
            double dg[NJ], uc[NJ];
            double best = -1.0;
            int ib = 0;
#pragma unroll
            for (int i = 0; i < NJ; ++i) dg[i] = 1.0;
#pragma unroll
            for (int r = 0; r < 6; ++r)
#pragma unroll
                for (int i = 0; i < NJ; ++i) dg[i] -= Jm[i][r] * Jm[i][r];
#pragma unroll
            for (int i = 0; i < NJ; ++i)
                if (dg[i] > best) { best = dg[i]; ib = i; }
#pragma unroll
            for (int i = 0; i < NJ; ++i) uc[i] = (i == ib) ? 1.0 : 0.0;
            project(uc);  // twice: the second pass squares the residual
            project(uc);
            const double nnc = norm2(uc);
#pragma unroll
            for (int i = 0; i < NJ; ++i) u[i] = warm ? u[i] : uc[i];
            nn = warm ? nn : nnc;
        }
        double nrm, ninv;
        sqrt_rsqrt(nn, nrm, ninv);
        // All three sign decisions are taken on the un-normalised u and applied with the normalisation, in one
        // multiplication per joint.  (1) The raw vector v as LAPACK's SVD leaves it: the first component that is
        // not negligible (|v_i| > 1e-9 of the unit vector) is negative (oracle + golden).
        const double thr = 1e-9 * nrm;
        bool found = false, negate = false;  // negate: v = -u / |u|
#pragma unroll
        for (int i = 0; i < NJ; ++i)
            if (!found && fabs(u[i]) > thr) { found = true; negate = u[i] > 0.0; }
        // (2) sign continuity against the previous cycle (nullspace:101-105): sig flips when sig v is farther from
        // lastvec than -sig v; |sig v - l|^2 - |sig v + l|^2 = -4 sig (v . l), so only the sign of v . l counts
        double dot = 0.0;
#pragma unroll
        for (int i = 0; i < NJ; ++i) dot += u[i] * lv_r[i];
        int sig = sig_r;
        const double vl = negate ? -dot : dot;
        if ((sig < 0 ? -vl : vl) < 0.0) sig = -sig;
        sig_r = sig;
        has_vec = true;
        const double k = (negate != (sig < 0)) ? -ninv : ninv;
#pragma unroll
        for (int i = 0; i < NJ; ++i) {
            u[i] *= k;
            lv_r[i] = u[i];
            qn[i] = u[i] * c0;  // move_in_nullspace (nullspace:113-117): min(n, 4, 1) = 1 row
        }
        advanced = true;
    } else if (nullity >= 2) {
        status |= VFIK_ST_NULL_AMBIGUOUS;  // SVD basis not unique: /control cannot be honoured
    }
    if (jl_task) {
        double z[NJ];
        descent(z);
        double c[6];
#pragma unroll
        for (int r = 0; r < 6; ++r) c[r] = 0.0;
#pragma unroll
        for (int i = 0; i < NJ; ++i)
#pragma unroll
            for (int r = 0; r < 6; ++r) c[r] += Jm[i][r] * z[i];
#pragma unroll
        for (int r = 0; r < 6; ++r)
#pragma unroll
            for (int i = 0; i < NJ; ++i) z[i] -= c[r] * Jm[i][r];
#pragma unroll
        for (int i = 0; i < NJ; ++i) qn[i] += z[i];
    }
    return advanced;
}

// slot reader for eval_slot: the quad planes in global memory (vfik_kernel.hip has the one of a wave's LDS region, SlotLds)
template <typename T> struct SlotGlobal {
    const T* sq; long Q;  // plane 0, component 0 of this lane's arm; plane pitch in elements
    __device__ __forceinline__ double operator()(int m, int e) const { return slot_elem(sq, Q, m, e); }
};
