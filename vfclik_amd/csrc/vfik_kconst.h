// vfik_kconst.h -- a chain's batch-shared device constants and how the host derives them: KConst<NJ>, the image's layout (KTab, the
// VFIK_KCONST_*_OFF patch points), the DH patterns the lean kernels are built for, and kconst_fill: vfik_chain + vfik_params + the shared
// tool -> the image, the `plain` code and the pattern decision.  Pure host code on the C++ standard library and include/vfik_types.h: no
// HIP symbol, so tests/c_host/kconst.cpp holds it on the CPU (tests/test_kconst.py).  The device code reads KConst through vfik_kernel.h,
// which includes this header; vfik_abi.cpp uploads the image (upload_kconst).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstring>

#include <stdint.h>

#include "../../include/vfik_types.h"

// joint counts the library is built for (one fully unrolled kernel each)
#ifndef VFIK_NJ_LIST
#define VFIK_NJ_LIST X(6) X(7) X(10) X(14)
#endif

namespace vfik {

// Batch-shared constants: chain geometry, limits and parameters.  They live in DEVICE memory (one
// copy per handle, rewritten only by vfik_set_chain / vfik_set_params) and are read through the
// scalar cache; the kernarg block stays small.  Measured: with the 2.3 KB of constants inside the
// kernarg segment every batch of s_loads was a long-latency fetch in the middle of the kinematics.
template <int NJ>
struct KConst {
    // ---- kinematics block: copied into LDS by every wave (one or two 1-KiB requests) and read from
    // there as vector operands.  As scalar (SGPR) operands the ~90 doubles did not fit the 100 SGPRs:
    // the compiler hoisted every s_load to the top and spilled to VGPR lanes (v_writelane/readlane).
    // Chain in Denavit-Hartenberg form, derived on the host from the z-normal form of vfik_chain
    // (kconst_fill_t below): T_ee = base * prod_i [ Screw_z(q_i) Tx(a_i) Rx(alpha_i) ] * Screw_z(tail)
    double base[12];  // B[0], row-major 3x4
    // c = crev*cos(q+off) + cprs, s = crev*sin(q+off) + sprs, displacement = qd*q + d: revolute joints have
    // (crev, cprs, sprs, qd) = (1, 0, 0, 0), prismatic ones (0, cos off, sin off, 1) -- arithmetic blends
    struct DH { double off, crev, cprs, sprs, qd, d, a, ca, sa, pad; } dh[NJ];   // dh[0].pad: the batch's uniform repeller FORCE (below)
    // dh[1].pad: 1 / rot_slow (0: no rotational slow-down), which every wave formed with rcp_nr until round 5.  In a pad, so that no member moves:
    // as a member of its own behind cos_slow it moved every later member by 8 bytes, and a 14-joint general variant then spilled 52 B per lane.
    // (That rot_slow lies in (0, pi/8) -- the short arctangent of rot_axis_angle -- the kernels read off cos_slow > cos(pi/8).)
    double tail_c, tail_s, tail_e;  // trailing z-screw of the last fixed transform
    // safe distance of every decay repeller of the batch when they all share one (and one force, dh[0].pad): the uniform repeller
    // image of the straight-line path then carries (x y z radius) per slot only (vfik_scene.h: pack_fields, plan_scene)
    double rep_safe;
    // ---- everything else: read through the scalar cache.  Ordered by use on the lean paths: the first members share the 1-KiB
    // rows that every wave copies to LDS for the kinematics block, so the L2 has them by the time the scalar loads ask -- with
    // one handle after another (inputs from HBM) the first use of lambda2 / rot_slow cost the wave an HBM round trip (round 3).
    double speed, lambda2, rot_slow, null_gain, lookahead, max_vel;
    double cos_slow;  // cos(rot_slow): rotation angles with a smaller cosine need no atan2 (scalar = 1)
    double jp_kp, jp_delta;  // joint P controller (joint_p_controller:55-57)
    double jl_gain;          // gain of the joint-limit task (jl_k is jl_gain / half^2 of the STATIC limits; per-cycle limits use this)
    double mix_w[VFIK_MIX_CHANNELS];
    // shared tool frame (rows 0..2 of the 4x4; per-arm tools are a device array).  In the rows every wave copies to LDS: with the inputs
    // cold a scalar load from the tail of the block is an HBM round trip of its own (measured on a flag there: C3 +7 %, profiles/r04_ab_tool.txt)
    double tool[12];
    double wy[6];    // the batch's IK weights (/weight, vf:295-309), in the copied rows for the same reason
    double wq[NJ];
    double q_lo[NJ];
    double q_hi[NJ];
    double q_mid[NJ];     // (lo + hi) / 2
    double inv_half[NJ];  // 2 / (hi - lo)
    double jl_k[NJ];      // jl_gain / half^2
    unsigned prismatic_mask;
    unsigned pad0;
    static constexpr int KIN_BYTES = (12 + 10 * NJ + 4 + 10 + VFIK_MIX_CHANNELS + 12 + 6 + NJ) * 8;  // through wq: the block every wave copies to LDS
    static constexpr int KIN_ROWS = (KIN_BYTES + 1023) / 1024;  // 1-KiB LDS rows / requests
};
// The device image of the constants is KConst<NJ> padded to a multiple of 1 KiB, then the 1-KiB sin / cos table
// ((sin, cos)(k pi/32), k = 0..63) that every wave copies to LDS with the kinematics block.
// where the host patches the uniform repeller pair into the device image (vfik_abi.cpp: write_uniform_pair)
#define VFIK_KCONST_REP_FORCE_OFF ((12 + 9) * 8)
#define VFIK_KCONST_ROT_SLOW_INV_OFF ((12 + 10 + 9) * 8)   // dh[1].pad: 1 / rot_slow
#define VFIK_KCONST_REP_SAFE_OFF(nj) ((12 + 10 * (nj) + 3) * 8)
static_assert(offsetof(KConst<7>, rep_safe) == VFIK_KCONST_REP_SAFE_OFF(7) && offsetof(KConst<14>, rep_safe) == VFIK_KCONST_REP_SAFE_OFF(14), "KConst::rep_safe");
static_assert(offsetof(KConst<7>, dh) + offsetof(KConst<7>::DH, pad) == VFIK_KCONST_REP_FORCE_OFF, "KConst::dh[0].pad");
static_assert(offsetof(KConst<7>, dh) + sizeof(KConst<7>::DH) + offsetof(KConst<7>::DH, pad) == VFIK_KCONST_ROT_SLOW_INV_OFF && offsetof(KConst<14>, dh) == offsetof(KConst<7>, dh), "KConst::dh[1].pad");
static_assert(offsetof(KConst<7>, wq) + 7 * 8 == KConst<7>::KIN_BYTES && offsetof(KConst<14>, wq) + 14 * 8 == KConst<14>::KIN_BYTES, "KConst::wq closes the LDS-copied block");
static_assert(KConst<7>::KIN_BYTES <= 1024 && KConst<6>::KIN_BYTES <= 1024 && KConst<10>::KIN_BYTES <= 2048 && KConst<14>::KIN_BYTES <= 2048, "the copied block keeps its row count");
template <int NJ> struct KTab { static constexpr int OFFSET = ((int)sizeof(KConst<NJ>) + 1023) / 1024 * 1024; };

// DH patterns the lean kernels are built for (cycle_body, DHP): per joint count, bit i of
//   SWAP: link i has a = 0 and alpha = +pi/2 EXACTLY as the kernel sees it (ca == 0, sa == 1: the host snaps |ca| < 1e-15),
//   NONE: a = 0 and alpha = 0 (ca == 1, sa == 0),     D0: the link's z-offset d is 0.
// Pattern 1 per joint count: the KUKA LWR 4+ (vfclik's default robot), two of them in series (BASELINE's C5), the 6-joint arm of
// robots.py.  A chain qualifies when its own masks contain the pattern's (kconst_fill_t collects them, dh_pattern_of decides).
//   OFF0 / OFFPI: the joint's angle offset in the DH form is an even / odd multiple of pi (the joint angle itself enters the
//   sin / cos, an odd multiple negates both),     BASE_I: the base frame B[0] is the identity (joint 1 starts from unit vectors).
template <int NJ, int DHP> struct DhPattern { static constexpr unsigned SWAP = 0, NONE = 0, D0 = 0, OFF0 = 0, OFFPI = 0; static constexpr bool BASE_I = false; };
template <> struct DhPattern<7, 1> { static constexpr unsigned SWAP = 0x3Fu, NONE = 0x40u, D0 = 0x2Au, OFF0 = 0x15u, OFFPI = 0x6Au; static constexpr bool BASE_I = true; };
template <> struct DhPattern<14, 1> {
    static constexpr unsigned SWAP = 0x1FBFu, NONE = 0x2040u, D0 = 0x152Au, OFF0 = 0xA95u, OFFPI = 0x356Au;
    static constexpr bool BASE_I = true;
};
template <> struct DhPattern<6, 1> { static constexpr unsigned SWAP = 0x1Du, NONE = 0x20u, D0 = 0x16u, OFF0 = 0x27u, OFFPI = 0x18u; static constexpr bool BASE_I = true; };
// A pattern whose LAST link keeps its frame (NONE) must give that link a z-offset (D0 clear): the last joint's angle reaches the position through
// that offset alone (cycle_body: J_LAST_AXIAL; the eight-lanes kernel likewise) -- with d = 0 a NaN last angle would be a finite command again.
template <int NJ> constexpr bool dh_last_axial_has_offset() {
    return !((DhPattern<NJ, 1>::NONE >> (NJ - 1)) & 1u) || !((DhPattern<NJ, 1>::D0 >> (NJ - 1)) & 1u);
}
static_assert(dh_last_axial_has_offset<6>() && dh_last_axial_has_offset<7>() && dh_last_axial_has_offset<14>(), "DhPattern: an axial last link needs d != 0");
// the pattern id of a chain with these masks (0: none built for it)
inline int dh_pattern_of(int nj, unsigned swap, unsigned none, unsigned d0, unsigned off0, unsigned offpi, bool base_identity) {
    unsigned ps = 0, pn = 0, pd = 0, p0 = 0, ppi = 0;
    bool pb = false;
    switch (nj) {
#define X(n) case n: ps = DhPattern<n, 1>::SWAP; pn = DhPattern<n, 1>::NONE; pd = DhPattern<n, 1>::D0; p0 = DhPattern<n, 1>::OFF0; ppi = DhPattern<n, 1>::OFFPI; pb = DhPattern<n, 1>::BASE_I; break;
        VFIK_NJ_LIST
#undef X
        default: break;
    }
    if (ps == 0) return 0;
    // the chain's zeros must CONTAIN the pattern's (more zeros are fine: they are multiplied out); its pi offsets must be the pattern's
    return ((swap & ps) == ps && (none & pn) == pn && (d0 & pd) == pd && (off0 & p0) == p0 && (offpi & ppi) == ppi && (!pb || base_identity)) ? 1 : 0;
}

inline bool has_dh_pattern(int nj) {
    switch (nj) {
#define X(n) case n: return DhPattern<n, 1>::SWAP != 0;
        VFIK_NJ_LIST
#undef X
        default: return false;
    }
}

// Whether a shared tool (rows 0..2 of the 4 x 4, row-major 3 x 4) can ride on the PLAIN kernels' TOOLC variants, which rebuild the lever arm
// p_ee - p_tip = -Rt (Rtool^-1 t) and /pose_no_tool from the tool pose: its 3 x 3 block must be invertible to working accuracy --
// max |Rtool Rtool^T - I| <= VFIK_TOOL_MAX_DEFECT (include/vfik.h states the rule); a block with a larger defect, a singular or a non-finite
// one is not a plain + tool handle (kconst_fill then reports plain = 0: the general variants, which keep the flange frame).
// c3 = Rtool^-1 t by cofactors in long double (zeros when the answer is no).  Host code.
inline bool tool_block_serves_plain(const double* tool12, double* c3) {
    const long double a = tool12[0], b = tool12[1], c = tool12[2], d = tool12[4], e = tool12[5], f = tool12[6], g = tool12[8], h = tool12[9], i = tool12[10];
    const long double t[3] = {tool12[3], tool12[7], tool12[11]};
    const long double co[9] = {e * i - f * h, c * h - b * i, b * f - c * e, f * g - d * i, a * i - c * g, c * d - a * f, d * h - e * g, b * g - a * h, a * e - b * d};
    const long double det = a * co[0] + b * co[3] + c * co[6];
    long double defect = 0.0L;
    bool finite = true;
    for (int r = 0; r < 3; ++r)
        for (int k = 0; k < 3; ++k) {
            long double s = r == k ? -1.0L : 0.0L;
            for (int m = 0; m < 3; ++m) s += (long double)tool12[4 * r + m] * (long double)tool12[4 * k + m];
            s = s < 0.0L ? -s : s;
            finite = finite && s == s;
            defect = s > defect ? s : defect;
        }
    const bool ok = finite && defect <= (long double)VFIK_TOOL_MAX_DEFECT && det != 0.0L;
    for (int j = 0; j < 3; ++j) c3[j] = ok ? (double)((co[3 * j] * t[0] + co[3 * j + 1] * t[1] + co[3 * j + 2] * t[2]) / det) : 0.0;
    return ok;
}

// cos(rot_slow) as the attractor compares it: rotation angles with a smaller cosine need no atan2 (scalar = 1); -2: always evaluate the angle
inline double cos_slow_of(double rot_slowdown) { return rot_slowdown > 0.0 && rot_slowdown < 3.14159265358979323846 ? std::cos(rot_slowdown) : -2.0; }

namespace kconst_detail {
// ------------------------------------------------------------------------------------------------
// z-normal form -> DH form.  Every fixed transform factors as
//     B = Rz(theta) Tz(d) Tx(a) Rx(alpha) Rz(phi) Tz(e)          (ZXZ Euler angles + common normal)
// and the z-screws commute with the joint motions on either side, so the trailing (phi, e) of B[i]
// joins the leading (theta, d) of B[i+1] and the variable of joint i+1.  B[0] stays general.
// ------------------------------------------------------------------------------------------------
struct Screws { double theta, d, a, alpha, phi, e; };

inline Screws dh_factor(const double* B) {
    const double R00 = B[0], R10 = B[4], R02 = B[2], R12 = B[6], R20 = B[8], R21 = B[9], R22 = B[10];
    const double tx = B[3], ty = B[7], tz = B[11];
    Screws s{};
    const double sa = std::sqrt(R02 * R02 + R12 * R12);
    s.alpha = std::atan2(sa, R22);
    if (sa > 1e-12) {
        s.theta = std::atan2(R02, -R12);
        s.phi = std::atan2(R20, R21);
        const double ct = std::cos(s.theta), st = std::sin(s.theta);
        const double ux = ct * tx + st * ty, uy = -st * tx + ct * ty;
        s.a = ux;
        s.e = -uy / sa;
        s.d = tz - s.e * R22;
    } else {  // consecutive axes parallel (alpha = 0) or anti-parallel (alpha = pi)
        s.theta = (tx * tx + ty * ty > 1e-24) ? std::atan2(ty, tx) : 0.0;
        s.a = std::sqrt(tx * tx + ty * ty);
        s.e = 0.0;
        s.d = tz;
        const double g = std::atan2(R10, R00);
        s.phi = R22 > 0.0 ? g - s.theta : s.theta - g;
    }
    return s;
}

inline void mat_mul(const double* A, const double* B, double* C) {  // 3x4 row-major frames
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) C[4 * i + j] = A[4 * i] * B[j] + A[4 * i + 1] * B[4 + j] + A[4 * i + 2] * B[8 + j];
        C[4 * i + 3] = A[4 * i] * B[3] + A[4 * i + 1] * B[7] + A[4 * i + 2] * B[11] + A[4 * i + 3];
    }
}

inline double dh_recompose_error(const Screws& s, const double* B) {
    auto rz = [](double t, double d, double* M) { const double c = std::cos(t), sn = std::sin(t); const double m[12] = {c, -sn, 0, 0, sn, c, 0, 0, 0, 0, 1, d}; memcpy(M, m, sizeof m); };
    auto rx = [](double al, double a, double* M) { const double c = std::cos(al), sn = std::sin(al); const double m[12] = {1, 0, 0, a, 0, c, -sn, 0, 0, sn, c, 0}; memcpy(M, m, sizeof m); };
    double A[12], X[12], C[12], T1[12], T2[12];
    rz(s.theta, s.d, A); rx(s.alpha, s.a, X); rz(s.phi, s.e, C);
    mat_mul(A, X, T1); mat_mul(T1, C, T2);
    double err = 0.0;
    for (int k = 0; k < 12; ++k) err = std::fmax(err, std::fabs(T2[k] - B[k]));
    return err;
}
}  // namespace kconst_detail

template <int NJ>
double kconst_fill_t(void* dst, const vfik_chain& ch, const vfik_params& p, const double* tool12, int* plain, int* dhp) {
    KConst<NJ>& c = *static_cast<KConst<NJ>*>(dst);
    memset(&c, 0, sizeof c);
    memcpy(c.base, ch.B[0], sizeof c.base);
    double phi_prev = 0.0, e_prev = 0.0, worst = 0.0;
    unsigned m_swap = 0, m_none = 0, m_d0 = 0, m_off0 = 0, m_offpi = 0;   // the chain's DH pattern (DhPattern)
    for (int i = 0; i < NJ; ++i) {
        const kconst_detail::Screws s = kconst_detail::dh_factor(ch.B[i + 1]);
        worst = std::fmax(worst, kconst_detail::dh_recompose_error(s, ch.B[i + 1]));
        const double off = phi_prev + s.theta;
        const bool pris = ch.jtype[i] == 1;
        c.dh[i].off = off;
        c.dh[i].crev = pris ? 0.0 : 1.0;
        c.dh[i].cprs = pris ? std::cos(off) : 0.0;
        c.dh[i].sprs = pris ? std::sin(off) : 0.0;
        c.dh[i].qd = pris ? 1.0 : 0.0;
        c.dh[i].d = e_prev + s.d;
        c.dh[i].a = s.a;
        c.dh[i].ca = std::cos(s.alpha);
        c.dh[i].sa = std::sin(s.alpha);
        // exact zeros and ones where the geometry has them (cos(pi/2) is 6e-17 in floating point): the DH pattern masks below -- and
        // the kernel variants that assume them -- rest on EXACT values; the snap moves a frame by less than 1e-15
        if (std::fabs(c.dh[i].a) < 1e-15) c.dh[i].a = 0.0;
        if (std::fabs(c.dh[i].d) < 1e-15) c.dh[i].d = 0.0;
        if (std::fabs(c.dh[i].ca) < 1e-15 && c.dh[i].sa > 0.0) { c.dh[i].ca = 0.0; c.dh[i].sa = 1.0; }
        if (std::fabs(c.dh[i].sa) < 1e-15 && c.dh[i].ca > 0.0) { c.dh[i].sa = 0.0; c.dh[i].ca = 1.0; }
        if (!pris && c.dh[i].a == 0.0 && c.dh[i].ca == 0.0 && c.dh[i].sa == 1.0) m_swap |= 1u << i;
        if (!pris && c.dh[i].a == 0.0 && c.dh[i].ca == 1.0 && c.dh[i].sa == 0.0) m_none |= 1u << i;
        if (!pris && c.dh[i].d == 0.0) m_d0 |= 1u << i;
        {   // an offset that is a multiple of pi: snapped to it, so that the pattern's "no offset" / "negate" is exact for this chain
            const double kpi = off / 3.14159265358979323846;
            const double kr = std::nearbyint(kpi);
            if (!pris && std::fabs(kpi - kr) < 1e-12) {
                c.dh[i].off = kr * 3.14159265358979323846;
                if (((long)kr) % 2 == 0) m_off0 |= 1u << i; else m_offpi |= 1u << i;
            }
        }
        phi_prev = s.phi;
        e_prev = s.e;
        const double half = 0.5 * (ch.q_hi[i] - ch.q_lo[i]);
        c.q_lo[i] = ch.q_lo[i];
        c.q_hi[i] = ch.q_hi[i];
        c.q_mid[i] = 0.5 * (ch.q_lo[i] + ch.q_hi[i]);
        c.inv_half[i] = 1.0 / half;
        c.jl_k[i] = p.jl_gain / (half * half);
        c.wq[i] = p.wq[i];
        if (ch.jtype[i] == 1) c.prismatic_mask |= 1u << i;
    }
    c.tail_c = std::cos(phi_prev);
    c.tail_s = std::sin(phi_prev);
    c.tail_e = e_prev;
    for (int i = 0; i < 6; ++i) c.wy[i] = p.wy[i];
    for (int i = 0; i < VFIK_MIX_CHANNELS; ++i) c.mix_w[i] = p.mix_w[i];
    for (int k = 0; k < 12; ++k) c.tool[k] = tool12[k];
    // The shared tool on the PLAIN kernels (TOOLC): they keep no flange value through the field and rebuild the lever arm p_ee - p_tip =
    // -Rt (Rtool^-1 t) and /pose_no_tool from the tool pose.  c3 = Rtool^-1 t is formed here, in long double by cofactors, and rides in
    // dh[2..4].pad (no member moves); the block must be invertible to working accuracy for that -- the rule of include/vfik.h:
    // max |Rtool Rtool^T - I| <= VFIK_TOOL_MAX_DEFECT, else the handle takes the general variants, which keep the flange frame itself
    // (tool_block_serves_plain).
    static_assert(NJ >= 5, "KConst::dh[2..4].pad");
    double c3[3];
    const bool tool_block_ok = tool_block_serves_plain(tool12, c3);
    for (int j = 0; j < 3; ++j) c.dh[2 + j].pad = c3[j];
    c.speed = p.speed_scale;
    c.lambda2 = p.lambda * p.lambda;
    c.rot_slow = p.rot_slowdown;
    c.cos_slow = cos_slow_of(p.rot_slowdown);
    // (the kernels' rcp_nr(rot_slow) of old is this value: its last Newton step rounds (1 - e^2) / rot_slow with e < 2^-48 once)
    c.dh[1].pad = p.rot_slowdown > 0.0 ? 1.0 / p.rot_slowdown : 0.0;   // (KConst: 1 / rot_slow)
    c.null_gain = p.null_gain;
    c.lookahead = p.lookahead;
    c.max_vel = p.max_vel;
    c.jp_kp = p.jp_kp;
    c.jp_delta = p.jp_delta;
    c.jl_gain = p.jl_gain;
    // PLAIN variant of the kernel: revolute joints only, no trailing screw.  *plain: 0 general variants; else 1 + (the batch's shared tool
    // is not the identity ? 1 : 0) + (its IK weights are not all one ? 2 : 0): the lean float32 kernels and the eight-lanes kernel have
    // variants that apply a shared tool and shared weights themselves (cycle_body: TOOLC, WTSC), every other launch of such a handle takes
    // the general variants (plan_cycle).
    bool pl = c.prismatic_mask == 0 && c.tail_c == 1.0 && c.tail_s == 0.0 && c.tail_e == 0.0 && tool_block_ok;
    static const double ident[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    bool tool_ident = true;
    for (int k = 0; k < 12; ++k) tool_ident = tool_ident && tool12[k] == ident[k];
    bool unit_w = true;
    for (int i = 0; i < 6; ++i) unit_w = unit_w && p.wy[i] == 1.0;
    for (int i = 0; i < NJ; ++i) unit_w = unit_w && p.wq[i] == 1.0;
    *plain = pl ? 1 + (tool_ident ? 0 : 1) + (unit_w ? 0 : 2) : 0;
    bool base_i = true;
    {
        static const double ident[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
        for (int k = 0; k < 12; ++k) base_i = base_i && c.base[k] == ident[k];
    }
    if (dhp) *dhp = pl ? dh_pattern_of(NJ, m_swap, m_none, m_d0, m_off0, m_offpi, base_i) : 0;
    // (sin, cos)(k pi/32), k = 0 .. 63, for sincos_tab_n
    double* tab = reinterpret_cast<double*>(static_cast<char*>(dst) + KTab<NJ>::OFFSET);
    for (int k = 0; k < 64; ++k) {
        const long double a = (long double)k * 3.14159265358979323846264338327950288L / 32.0L;
        tab[2 * k] = (double)sinl(a);
        tab[2 * k + 1] = (double)cosl(a);
    }
    return worst;
}

// the joint counts the library is built for, bit n = n joints
inline uint32_t supported_joints_mask() {
    uint32_t m = 0;
#define X(n) m |= 1u << n;
    VFIK_NJ_LIST
#undef X
    return m;
}

// size of the device image of KConst<nj> for the host (0 if nj is not built)
inline size_t kconst_bytes(int nj) {  // the constants, padded to 1 KiB, and the sin / cos table behind them
    switch (nj) {
#define X(n) case n: return KTab<n>::OFFSET + 1024;
        VFIK_NJ_LIST
#undef X
        default: return 0;
    }
}

// fill a host image of KConst<nj> at dst; returns the largest recomposition error of the DH conversion (the caller refuses a chain above
// 1e-9), 1e300 for a joint count that is not built
inline double kconst_fill(int nj, void* dst, const vfik_chain& chain, const vfik_params& p, const double* tool12, int* plain, int* dhp = nullptr) {
    switch (nj) {
#define X(n) case n: return kconst_fill_t<n>(dst, chain, p, tool12, plain, dhp);
        VFIK_NJ_LIST
#undef X
        default: return 1e300;
    }
}

}  // namespace vfik
