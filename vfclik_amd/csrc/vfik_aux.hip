// vfik_aux.hip -- the library's small kernels beside the control cycle, and every type-erased launcher vfik_abi.cpp calls:
//   mix_kernel, track_kernel, monitor_kernel, probe_kernel      the mixer's sum alone, the tracking estimator, the distance monitor, the field probe
//   move_kernel, move_scene_kernel                              goals, obstacles, funnels, hemispheres and attractors that move
//   check_kernel, script_kernel (+ the _stall_ builds)          the check after each block of a timed move (vfik_check_body.inc, twice)
//   link_kernel                                                 sphere centres on the links of a source arm: the other arm as an obstacle
//   clear_kernel                                                the room between an arm's own link spheres and other spheres; the wait rule
//   launch_cycle                                                a launch's plan (vfik_kernel.h: plan_cycle) -> the entry point of the object that holds
//                                                               its kernel (vfik_kernel.hip, compiled per joint count, I/O type, nullspace module)
// Compiled once (csrc/Makefile: vfik_dispatch.o).  The float64 building blocks are vfik_device.h, shared with the cycle kernels.
#include "vfik_kernel.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <type_traits>

namespace vfik {
// the per-part entry points of vfik_kernel.hip
#define X(n)                                                                                                      \
    hipError_t launch_cycle_nj##n##_t32_ns0(const KArgs& kargs, const CyclePlan& plan, hipStream_t stream);      \
    hipError_t launch_cycle_nj##n##_t32_ns1(const KArgs& kargs, const CyclePlan& plan, hipStream_t stream);      \
    hipError_t launch_cycle_nj##n##_t64_ns0(const KArgs& kargs, const CyclePlan& plan, hipStream_t stream);      \
    hipError_t launch_cycle_nj##n##_t64_ns1(const KArgs& kargs, const CyclePlan& plan, hipStream_t stream);
VFIK_NJ_LIST
#undef X

namespace {
#include "vfik_device.h"

// CommandMixer.read's weighted sum alone (command_mixer.py:78-82): out = sum_k cmd[k] * w[k], left to
// right from 0.0, multiply and add rounded separately (what CPython does).
template <typename T>
__global__ void __launch_bounds__(256) mix_kernel(const T* cmds, const double* w, int K, long count, long chan_stride, T* out) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    double acc = 0.0;
    for (int k = 0; k < K; ++k) acc = mac_unfused(acc, (double)cmds[k * chan_stride + i], w[k]);
    out[i] = (T)acc;
}

// ------------------------------------------------------------------------------------------------
// Tracking-error estimator of scripts/vf (vf:349-428), batched, as its own small kernel (a diagnostic:
// it never feeds qdot).  Per arm it keeps the previous tool frame, the last 4 commanded twists and a
// frame counter; from the 6th frame on (frame_list longer than 5, vf:354) it compares the twist
// MEASURED between the two latest frames, scaled by the assumed 150 Hz robot loop (vf:408-411), with
// the twist COMMANDED check_delay = 4 cycles earlier (vf:363): direction angles, corrected magnitudes,
// |difference| and arm_tracking = difference < 0.10.  state: [38][B] doubles (12 frame, 24 commands,
// count, -).  out: [B][8] = vel_diff_angle, rot_diff_angle, ext_vel_mag_corr, ext_rot_mag_corr,
// cmd_vel_mag_corr, cmd_rot_mag_corr, ext_int_diff, arm_tracking (vf:418-427); zeros until the 6th frame.
// ------------------------------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(256) track_kernel(const T* pose, const T* v6, double* st, T* out, const int* active, int B) {
    const int arm = blockIdx.x * blockDim.x + threadIdx.x;
    if (arm >= B) return;
    if (active && !active[arm]) return;  // inside vf's `if qInBottle` (vf:312-313,349): no fresh q, no new frame
    const long Bs = B;
    double F[12], P[12], cmd[4][6];
#pragma unroll
    for (int k = 0; k < 12; ++k) { F[k] = (double)pose[(long)arm * 16 + k]; P[k] = st[k * Bs + arm]; }
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int k = 0; k < 6; ++k) cmd[j][k] = st[(12 + 6 * j + k) * Bs + arm];
    const double cnt = st[36 * Bs + arm];  // frames seen before this one
    // cmd_buffer.append(...); keep the last 4 (vf:350-352): after the shift cmd[0] is the oldest
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int k = 0; k < 6; ++k) cmd[j][k] = cmd[j + 1][k];
#pragma unroll
    for (int k = 0; k < 6; ++k) cmd[3][k] = (double)v6[(long)arm * 6 + k];
    double res[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (cnt >= 5.0) {  // len(frame_list) > frame_list_size (vf:354)
        // ext_diff = PyKDL.diff(previous frame, this frame): vel = dp, rot = log(R_b R_a^T) in the base frame
        double ev[3] = {F[3] - P[3], F[7] - P[7], F[11] - P[11]};
        double Ra[9], Rb[9], ax[3], th;
        bool has_axis;
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) { Ra[3 * r + c] = P[4 * r + c]; Rb[3 * r + c] = F[4 * r + c]; }
        rot_axis_angle<false>(Ra, Rb, -2.0, ax, th, has_axis);
        const double ext_vel_mag = sqrt(ev[0] * ev[0] + ev[1] * ev[1] + ev[2] * ev[2]);
        const double ext_rot_mag = has_axis ? th : 0.0;
        // the command issued check_delay = 4 cycles ago is the oldest entry of the full buffer (vf:363)
        const double* c = cmd[0];
        const double cmd_vel_mag = sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
        const double cmd_rot_mag = sqrt(c[3] * c[3] + c[4] * c[4] + c[5] * c[5]);
        double eu[3] = {1, 0, 0}, cu[3] = {1, 0, 0}, er[3] = {1, 0, 0}, cr[3] = {1, 0, 0};  // vf:365-374,390-399
        if (ext_vel_mag > 0.0) for (int k = 0; k < 3; ++k) eu[k] = ev[k] / ext_vel_mag;
        if (cmd_vel_mag > 0.0) for (int k = 0; k < 3; ++k) cu[k] = c[k] / cmd_vel_mag;
        if (ext_rot_mag > 0.0) for (int k = 0; k < 3; ++k) er[k] = ax[k];
        if (cmd_rot_mag > 0.0) for (int k = 0; k < 3; ++k) cr[k] = c[3 + k] / cmd_rot_mag;
        const double vd = fmin(1.0, fmax(-1.0, cu[0] * eu[0] + cu[1] * eu[1] + cu[2] * eu[2]));
        const double rd = fmin(1.0, fmax(-1.0, cr[0] * er[0] + cr[1] * er[1] + cr[2] * er[2]));
        res[0] = fabs(acos(vd));
        res[1] = fabs(acos(rd));
        res[2] = ext_vel_mag * 150.0;   // loop_freq (vf:408)
        res[3] = ext_rot_mag * 150.0;
        res[4] = cmd_vel_mag;
        res[5] = cmd_rot_mag / 5.0;     // vf:412
        res[6] = fabs((res[4] + res[5]) - (res[2] + res[3]));
        res[7] = res[6] < 0.10 ? 1.0 : 0.0;  // tracking_th (vf:409,416)
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) out[(long)arm * 8 + k] = (T)res[k];
#pragma unroll
    for (int k = 0; k < 12; ++k) st[k * Bs + arm] = F[k];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int k = 0; k < 6; ++k) st[(12 + 6 * j + k) * Bs + arm] = cmd[j][k];
    st[36 * Bs + arm] = cnt + 1.0;
}

// ------------------------------------------------------------------------------------------------
// Distance monitor of scripts/monitor_distance (monitor_distance:76-84,148-167), batched: for every arm
// and every object frame it was told about (/dmonitor/objectsIn: the goal is object 0, obstacles
// follow), the xyz distance between the tool pose and the object and the rotation angle between their
// orientations, in DEGREES (orientLength = |diff(current, final).rot| * 180/pi).  One thread per
// (arm, object); pose [B][16], frames [B][O][16], out [B][O][2].  A diagnostic: it never feeds qdot.
// ------------------------------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(256) monitor_kernel(const T* pose, const T* frames, int O, long count, T* out, const int* active) {
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count) return;
    const long arm = t / O;
    if (active && !active[arm]) return;  // no fresh q, no new pose (monitor_distance:138-147 acts on a pose that ARRIVED): the rows stay
    double P[12], F[12];
    const T* pp = pose + arm * 16;
    const T* fp = frames + t * 16;
#pragma unroll
    for (int k = 0; k < 12; ++k) { P[k] = (double)pp[k]; F[k] = (double)fp[k]; }
    const double dx = P[3] - F[3], dy = P[7] - F[7], dz = P[11] - F[11];
    // relative rotation E = R_cur^T R_obj; its angle is what |diff().rot| measures
    double E[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) E[3 * i + j] = P[i] * F[j] + P[4 + i] * F[4 + j] + P[8 + i] * F[8 + j];
    const double a0 = 0.5 * (E[7] - E[5]), a1 = 0.5 * (E[2] - E[6]), a2 = 0.5 * (E[3] - E[1]);
    const double c = 0.5 * (E[0] + E[4] + E[8] - 1.0);
    const double sn = sqrt(a0 * a0 + a1 * a1 + a2 * a2);
    out[2 * t] = (T)sqrt(dx * dx + dy * dy + dz * dz);
    // (atan2_pos answers 0 for a pair that holds a NaN -- its compares fail and the quotient is taken for 0 / 0: a pose that is not finite has
    // no angle, and a monitor that reported 0 degrees for it would call a poisoned arm aligned)
    const double both = sn + c;
    out[2 * t + 1] = (T)((both == both ? atan2_pos(sn, c) : both) * 57.295779513082320877);
}

// ------------------------------------------------------------------------------------------------
// Field probe of scripts/vf (vf:469-503, "for visualizing"): the arm's total field evaluated at a pose that
// is handed in (/pose_in) instead of the forward kinematics: v6 = speedScale * scalars * normCart(sum)
// (vf:491-494 = vf:344-347 at another frame).  One thread per arm; goal block and slots are read straight
// from the quad planes through the general per-slot path.  pose [B][16], out [B][6].
// ------------------------------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(256) probe_kernel(const T* pose, const T* goal, const T* slots, int B, long Bp, int slots_used,
                                                    double rot_slow, double cos_slow, T* out) {
    const int arm = blockIdx.x * blockDim.x + threadIdx.x;
    if (arm >= B) return;
    double Rt[9], pt[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) Rt[3 * r + c] = (double)pose[(long)arm * 16 + 4 * r + c];
        pt[r] = (double)pose[(long)arm * 16 + 4 * r + 3];
    }
    const long Qp = Bp * 4;
    double gq[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) gq[k] = (double)goal[(long)(k >> 2) * Qp + (long)arm * 4 + (k & 3)];
    double tot[6] = {0, 0, 0, 0, 0, 0}, sc[2] = {1.0, 1.0};
    double GR[9], Gp[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) GR[3 * r + c] = gq[4 * r + c];
        Gp[r] = gq[4 * r + 3];
    }
    attractor<false>(Rt, pt, GR, Gp, gq[13], gq[14], rot_slow, cos_slow, gq[12] != 0.0, tot, sc, nullptr);
    const T* sq = slots + (long)arm * 4;
    const SlotGlobal<T> rg{sq, Qp};
    for (int m = 0; m < slots_used; ++m) eval_slot(rg, m, Rt, pt, rot_slow, cos_slow, tot, sc);
    double nt, nti, nr, nri;
    sqrt_rsqrt(tot[0] * tot[0] + tot[1] * tot[1] + tot[2] * tot[2], nt, nti);
    sqrt_rsqrt(tot[3] * tot[3] + tot[4] * tot[4] + tot[5] * tot[5], nr, nri);
    const double speed = gq[15];
    const double kt = nt > EPS_LEN ? speed * sc[0] * nti : 0.0;
    const double kr = nr > EPS_LEN ? speed * sc[1] * nri : 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        out[(long)arm * 6 + k] = (T)(tot[k] * kt);
        out[(long)arm * 6 + 3 + k] = (T)(tot[3 + k] * kr);
    }
}

// ------------------------------------------------------------------------------------------------
// vfik_move_fields (ABI 6): goals and obstacles that move (object_feeder:214-354 re-sends an object's primitives with new coordinates
// whenever its pose changes: the goal frame, object_feeder:229-241; x y z radius of the point obstacles and the near-goal repeller,
// object_feeder:317-334).  One thread per (arm, primitive): lanes run over arms -- aligned to the planes' 64-quad rows, so that every
// plane write of a wave is one contiguous 1 KiB (2 KiB at float64 I/O) -- and blockIdx.y over the primitives: the goal frame when
// one is given, then decay repeller k of the caller's rows.  Every image a later launch may read gets the new numbers:
//   goal block   rows 0..2 of the frame (plane 3 -- present, slow-down, force, speedScale -- stays),
//   uniform      plane k + 1: the whole quad (x y z radius),
//   compact      (x0 y0 z0 r0 | s0 f0 x1 y1 | z1 r1 s1 f1): the even slot's first quad; the odd slot's two half quads (s f stay),
//   general      first plane of the slot repmap names (p0..p3 = x y z radius; p4 p5 force type stay).
// Rows from the arm's repeller count on find MOVE_NONE in the map and write nothing: an unused slot keeps its -inf radius / zero force.
// Plain vector stores, no LDS, no loop, no register array.  VEC: the caller's arrays are 16-byte aligned (whole-quad loads).
// ------------------------------------------------------------------------------------------------
template <typename T> struct alignas(16) MoveQuad { T v[4]; };
template <typename T> struct alignas(2 * sizeof(T)) MovePair { T v[2]; };

template <typename T, bool VEC>
__device__ __forceinline__ MoveQuad<T> move_load(const T* src) {
    if (VEC) return *reinterpret_cast<const MoveQuad<T>*>(src);
    MoveQuad<T> r;
#pragma unroll
    for (int e = 0; e < 4; ++e) r.v[e] = src[e];
    return r;
}

// the goal frame of one arm: rows 0..2 into the goal block's first three planes
template <typename T, bool VEC>
__device__ __forceinline__ void move_goal_row(const MoveArgs& m, int arm, long j) {
    const long Qp = m.Bpad;  // quads per plane
    MoveQuad<T>* const g = static_cast<MoveQuad<T>*>(m.goal) + arm;
    if (g[3 * Qp].v[0] == (T)0) return;   // no goal block: the row is ignored
    const T* src = static_cast<const T*>(m.goal16) + j * 16;
    const MoveQuad<T> r0 = move_load<T, VEC>(src), r1 = move_load<T, VEC>(src + 4), r2 = move_load<T, VEC>(src + 8);
    if (r0.v[0] != r0.v[0]) return;       // NaN: this goal stays
    g[0] = r0;
    g[Qp] = r1;
    g[2 * Qp] = r2;
}

// decay repeller k of one arm: x y z radius into the uniform, the compact and the general image
template <typename T, bool VEC>
__device__ __forceinline__ void move_rep_row(const MoveArgs& m, int arm, long j, int k) {
    const long Qp = m.Bpad;
    if (k >= m.n_rep || k >= m.S) return;
    const unsigned gs = m.repmap[((long)(k >> 3) * m.Bpad + arm) * 8 + (k & 7)];
    if (gs >= (unsigned)m.S) return;              // MOVE_NONE: the arm has no k-th decay repeller
    const MoveQuad<T> r = move_load<T, VEC>(static_cast<const T*>(m.rep4) + (j * m.n_rep + k) * 4);
    if (r.v[0] != r.v[0]) return;                 // NaN: this repeller stays
    static_cast<MoveQuad<T>*>(m.slots_uni)[(long)(k + 1) * Qp + arm] = r;
    static_cast<MoveQuad<T>*>(m.slots)[(long)(2 * gs) * Qp + arm] = r;
    MoveQuad<T>* const f = static_cast<MoveQuad<T>*>(m.slots_fast) + (long)(3 * (k >> 1)) * Qp + arm;
    if (!(k & 1)) {
        f[0] = r;
    } else {
        MovePair<T> lo, hi;
        lo.v[0] = r.v[0]; lo.v[1] = r.v[1]; hi.v[0] = r.v[2]; hi.v[1] = r.v[3];
        reinterpret_cast<MovePair<T>*>(f + Qp)[1] = lo;
        reinterpret_cast<MovePair<T>*>(f + 2 * Qp)[0] = hi;
    }
}

template <typename T, bool VEC>
__global__ void __launch_bounds__(256) move_kernel(const MoveArgs m) {
    const int arm = (m.first_arm & ~63) + (int)(blockIdx.x * 256 + threadIdx.x);
    if (arm < m.first_arm || arm >= m.first_arm + m.n_arms) return;
    const long j = arm - m.first_arm;
    if (m.active && !m.active[j]) return;
    int k = (int)blockIdx.y;
    if (m.goal16) {
        if (k == 0) {
            move_goal_row<T, VEC>(m, arm, j);
            return;
        }
        --k;
    }
    move_rep_row<T, VEC>(m, arm, j, k);
}

// ------------------------------------------------------------------------------------------------
// vfik_move_scene: the rest of what the object feeder re-sends for an object that moves -- the approach funnel of `set goalAndNormal`
// (object_feeder:248-303), the surface of `set ObstacleH` (object_feeder:335-354) -- and attractors behind the goal block.  The same
// thread mapping as move_kernel; blockIdx.y runs over the goal frame, the caller's repeller rows, then its funnel, hemisphere and attractor
// rows (the class of a block is uniform: scalar branches).  Goal and repellers: move_kernel's stores.  The new classes live in the general
// image (and the aux block), whose slots keep p0..p5 | force type in two planes:
//   funnel / hemisphere k, general slot gs   plane 2 gs <- the quad x y z ax; plane 2 gs + 1 <- its FIRST pair ay az (force, type stay);
//                                            k = 0 also aux planes 0, 1 (funnel) or 3, 4 (hemisphere), laid out alike (cutAngle
//                                            angleOrder / safe order in the second pair stay);
//   attractor k, general slot gs             planes 2 gs, 2 gs + 1 (pair), 2 gs + 2, 2 gs + 3 (pair) <- p0..p11; slot gs + 2 (frame row 3,
//                                            slow-down distance) stays.
// A wave's pair stores cover the first 8 of every 16 bytes of one contiguous 1-KiB row (2 KiB at float64 I/O): every 128-byte line of the row
// is touched by ONE instruction -- byte-masked in L2, no line split between instructions -- as move_kernel's odd compact-image slots already are.
// Rows of six are 8-byte aligned at float32: pair loads (VEC: the caller's 6-rows are pair aligned, its 4- and 16-rows quad aligned).
// ------------------------------------------------------------------------------------------------
template <typename T, bool VEC>
__device__ __forceinline__ MovePair<T> move_load_pair(const T* src) {
    if (VEC) return *reinterpret_cast<const MovePair<T>*>(src);
    MovePair<T> r;
    r.v[0] = src[0]; r.v[1] = src[1];
    return r;
}

__device__ __forceinline__ unsigned scene_slot(const SceneMoveArgs& s, int cls, int arm, int k) {
    return s.scenemap[((long)(cls * s.map_planes + (k >> 3)) * s.m.Bpad + arm) * 8 + (k & 7)];
}

// funnel / hemisphere k of one arm: six scalars into the slot's first quad and the first pair of its second
template <typename T, bool VEC>
__device__ __forceinline__ void move_six_row(const SceneMoveArgs& s, int arm, int cls, const T* src, int k, int aux_plane) {
    const long Qp = s.m.Bpad;
    if (k >= s.m.S) return;
    const unsigned gs = scene_slot(s, cls, arm, k);
    if (gs + 1 >= (unsigned)s.m.S) return;        // MOVE_NONE: the arm has no k-th primitive of this class (a real one owns slots gs, gs + 1)
    const MovePair<T> a = move_load_pair<T, VEC>(src), b = move_load_pair<T, VEC>(src + 2), c = move_load_pair<T, VEC>(src + 4);
    if (a.v[0] != a.v[0]) return;                 // NaN: this primitive stays
    MoveQuad<T> q;
    q.v[0] = a.v[0]; q.v[1] = a.v[1]; q.v[2] = b.v[0]; q.v[3] = b.v[1];
    MoveQuad<T>* const g = static_cast<MoveQuad<T>*>(s.m.slots) + (long)(2 * gs) * Qp + arm;
    g[0] = q;
    reinterpret_cast<MovePair<T>*>(g + Qp)[0] = c;
    if (k == 0) {   // the arm's first funnel / hemisphere: the straight-line path reads it from the aux block
        MoveQuad<T>* const x = static_cast<MoveQuad<T>*>(s.aux) + (long)aux_plane * Qp + arm;
        x[0] = q;
        reinterpret_cast<MovePair<T>*>(x + Qp)[0] = c;
    }
}

// attractor k behind the goal block: rows 0..2 of its frame, p0..p11 of the general image's three slots
template <typename T, bool VEC>
__device__ __forceinline__ void move_att_row(const SceneMoveArgs& s, int arm, const T* src, int k) {
    const long Qp = s.m.Bpad;
    if (k >= s.m.S) return;
    const unsigned gs = scene_slot(s, SCENE_ATT, arm, k);
    if (gs + 2 >= (unsigned)s.m.S) return;        // MOVE_NONE (a real one owns slots gs .. gs + 2)
    const MoveQuad<T> r0 = move_load<T, VEC>(src), r1 = move_load<T, VEC>(src + 4), r2 = move_load<T, VEC>(src + 8);
    if (r0.v[0] != r0.v[0]) return;               // NaN: this attractor stays
    MoveQuad<T> q;
    MovePair<T> p45, p1011;
    p45.v[0] = r1.v[0]; p45.v[1] = r1.v[1];
    q.v[0] = r1.v[2]; q.v[1] = r1.v[3]; q.v[2] = r2.v[0]; q.v[3] = r2.v[1];
    p1011.v[0] = r2.v[2]; p1011.v[1] = r2.v[3];
    MoveQuad<T>* const g = static_cast<MoveQuad<T>*>(s.m.slots) + (long)(2 * gs) * Qp + arm;
    g[0] = r0;
    reinterpret_cast<MovePair<T>*>(g + Qp)[0] = p45;
    g[2 * Qp] = q;
    reinterpret_cast<MovePair<T>*>(g + 3 * Qp)[0] = p1011;
}

template <typename T, bool VEC>
__global__ void __launch_bounds__(256) move_scene_kernel(const SceneMoveArgs s) {
    const MoveArgs& m = s.m;
    const int arm = (m.first_arm & ~63) + (int)(blockIdx.x * 256 + threadIdx.x);
    if (arm < m.first_arm || arm >= m.first_arm + m.n_arms) return;
    const long j = arm - m.first_arm;
    if (m.active && !m.active[j]) return;
    int k = (int)blockIdx.y;
    if (m.goal16) {
        if (k == 0) {
            move_goal_row<T, VEC>(m, arm, j);
            return;
        }
        --k;
    }
    if (m.rep4) {
        if (k < m.n_rep) {
            move_rep_row<T, VEC>(m, arm, j, k);
            return;
        }
        k -= m.n_rep;
    }
    if (s.fun6) {
        if (k < s.n_fun) {
            move_six_row<T, VEC>(s, arm, SCENE_FUN, static_cast<const T*>(s.fun6) + (j * s.n_fun + k) * 6, k, 0);
            return;
        }
        k -= s.n_fun;
    }
    if (s.hem6) {
        if (k < s.n_hem) {
            move_six_row<T, VEC>(s, arm, SCENE_HEM, static_cast<const T*>(s.hem6) + (j * s.n_hem + k) * 6, k, 3);
            return;
        }
        k -= s.n_hem;
    }
    if (s.att16 && k < s.n_att) move_att_row<T, VEC>(s, arm, static_cast<const T*>(s.att16) + (j * s.n_att + k) * 16, k);
}

// ------------------------------------------------------------------------------------------------
// The check after block k of a timed move -- `stride` control cycles that ran under gate[] and left the integrated joint angles in q_now: one
// thread per arm, one kernel for two RULES (JOINT) and two TARGETS (LIST).
// The Cartesian rule (vfik_goto, vfik_follow): the arrival check of the reference's "send a goal, then wait until the arm is there" calls
//   (handlers.py:346-440: gotoFrame reads the object-0 entry of /dmonitor/distOut until pos_dist < goal_precision[0] and
//   orient_dist * pi / 180 < goal_precision[1], handlers.py:374-381) on the goal_dist row the block left in `dist`.  Both compares STRICT, in
//   double (NaN never arrives), and only while the arm is under way.  An arm without a goal block never arrives: its goal_dist is measured
//   against the zero frame of an empty block (a tool near the origin would pass), so the block's `present` flag decides.
// The joint rule (vfik_goto_js, vfik_follow_js): the wait of the reference's joint-space motion call, HandleJController.set_ref_js(js, wait,
//   goal_precision) (handlers.py:544-576), which sends js to /jpctrl/ref and reads /bridge/encoders until
//       ((js - goal_precision) <= q) * ((js + goal_precision) >= q)).all()
//   and returns (result, js - q).  `ref` is the arm's row of the reference as the caller sent it (not the clamped value the controller keeps), q the
//   row the block integrated.  Both edges are computed as written, in double on the io-typed values, both compares non-strict; NaN in q or in
//   the row fails a compare, so it never arrives -- a row that starts with NaN (an arm without a controller) included.  diff = (T)(ref - q) for
//   every arm that ran the block, also after it arrived or finished its list.  The precisions come by value and are indexed by the uniform
//   loop counter alone: scalar loads from the kernel arguments.
// One goal: arrived[b] = (k + 1) * stride - 1 at the arm's first successful check, the 0-based cycle whose tool pose / joint angles were measured.
// A list (vfik_follow: a user of the reference sends a LIST of gotoFrame calls -- approach, grasp, lift, place -- each the moment the previous
//   one returned true, handlers.py:346-387; vfik_follow_js: a script of set_ref_js calls -- home posture, pre-grasp posture, ...), way[B][W][16]
//   or [B][W][n]: an arm found at item next[b] gets reached[b][next] = (k + 1) * stride - 1 and next + 1, and -- if its list goes on -- the
//   following item as its target.  A frame goes into its goal block: move_goal_row's three quad stores (lanes run over arms: a wave's stores to a
//   plane lie in one 1 KiB row; plane 3 -- present, slow-down, force, speedScale -- stays), loaded as whole quads by the arriving lanes alone.  A
//   posture goes into its row of `ref`, the reference row of the HANDLE that every block reads as io->q_ref, copied element by element from
//   wayq, so the rule reads the posture as the caller sent it.  At most one item per check: the distance to the new goal exists only after the
//   next block (gotoFrame drops its first read for the same reason, handlers.py:365-384), and the controller has not moved towards the new
//   posture yet.
//     precision    via_prec while an item follows, prec at the arm's last one (joint: and past it, last = next >= len - 1);
//     way_now[b]   the item this check was made against: min(next, len - 1) on entry.
//   One goal is a list of one item here: len = 1, next = arrived >= 0.
// For every form:
//   the arm did not run (gate[b] == 0): the cycle kernel stored nothing for it -- its q row and, in a trace, its distance and item-index rows
//     repeat, it keeps its diff;
//   next block's gate: the caller's && len > 0 && !(hold && next == len) -- with `hold` not once the arm arrived or finished its list;
//   pending[k]: the arms that take part and have next < len -- a wave ballot, one atomic add per wave.
// k < 0 (uniform): one goal: arrived = -1; a list: reached = -1, next = 0, len = leading rows of way[b] that do not start with NaN; the gate; and
// item 0 into the goal block of every arm that takes part and has one, or into the arm's row of `ref` -- NaN for an arm that does not take part:
// no controller, the io->q_ref convention.
// Rows of n elements per lane, as the cycle kernel's q_out store; no LDS, no scratch, no register array.
// The stall rule (vfik_set_stall_rule; StallArgs, vfik_kernel.h) is a compile-time switch of the body: check_stall_kernel and
// script_stall_kernel carry it, check_kernel and script_kernel are the device code they were without it.
// ------------------------------------------------------------------------------------------------
// a quad as ONE value (a struct copy through MoveQuad would stay a 16 / 32-byte private object here: the frame's three loads come before the
// stores they may alias); 16-byte aligned for either I/O type, which is what way16 and the planes guarantee
template <typename T> struct FollowQuad { typedef T type __attribute__((ext_vector_type(4), aligned(16))); };

template <typename T>
__device__ __forceinline__ void follow_goal_store(T* goal, int b, long Qp, const T* frame) {
    typedef typename FollowQuad<T>::type Quad;
    const Quad* const src = reinterpret_cast<const Quad*>(frame);
    Quad* const g = reinterpret_cast<Quad*>(goal) + b;
    const Quad r0 = src[0], r1 = src[1], r2 = src[2];
    g[0] = r0;
    g[Qp] = r1;
    g[2 * Qp] = r2;
}

// The stall rule's helpers (StallArgs, vfik_kernel.h).  NaN is never progress: every compare is strict, and the joint measure keeps a NaN.
__device__ __forceinline__ void stall_reset(const StallArgs& st, int b) {
    st.best[2 * (long)b] = __builtin_inf();
    st.best[2 * (long)b + 1] = __builtin_inf();
    st.count[b] = 0;
}
__device__ __forceinline__ double stall_max(double e, double v) { return (v > e || v != v) ? v : e; }
// one evaluation for an arm that ran, is under way and did not arrive: true when this check declares it stalled
__device__ __forceinline__ bool stall_step(const StallArgs& st, int b, bool joint, double m0, double m1, int cycle) {
    double* const best = st.best + 2 * (long)b;
    const double b0 = best[0], b1 = joint ? 0.0 : best[1];
    const int c = st.count[b];
    const bool p0 = m0 < b0 - (joint ? st.eps_js : st.eps_pos), p1 = !joint && m1 < b1 - st.eps_rot;
    if (p0 || p1) {
        best[0] = m0 < b0 ? m0 : b0;
        if (!joint) best[1] = m1 < b1 ? m1 : b1;
        st.count[b] = 0;
        return false;
    }
    st.count[b] = c + 1;
    if (c + 1 != st.patience) return false;
    st.stalled[b] = cycle;
    return true;
}

// check_kernel and script_kernel, then check_stall_kernel and script_stall_kernel: one text, compiled without and with the stall rule
#define VFIK_STALL 0
#include "vfik_check_body.inc"
#undef VFIK_STALL
#define VFIK_STALL 1
#include "vfik_check_body.inc"
#undef VFIK_STALL

// ------------------------------------------------------------------------------------------------
// vfik_link_points: the other arm as an obstacle.  The reference runs one process set per arm (old/system_start.sh.old:60,237) and an arm
// learns where its neighbour is only as `set ObstacleP` objects that somebody re-sends whenever they move (object_feeder:317-334).  Here one
// lane per arm b walks the chain of the arm's SOURCE s = src_arm[b] (NULL: b itself) once, in float64, in the frames of the public chain
// (LinkArgs, vfik_kernel.h; LinkImage, vfik_links.h):
//     X_0 = B[0],   X_i = X_{i-1} Jz(q_s[i-1]) B[i]
// and when the walk stands at link i it emits every sphere of that link -- the image holds them sorted by link, the loop over them and the
// one over the joints have uniform bounds, the image is read at uniform addresses, jtype is a uniform branch -- as (R_b (X_i c) + t_b, radius)
// into the caller's row first_rep + perm of rep4[b].  The running frame is twelve named doubles: no frame array, no register array indexed at
// run time, no scratch.  sin and cos: sincos_fast (vfik_device.h), whose contract covers joint ranges.  A row is one 16-byte store (float32)
// or two (float64).  The image is a kernel argument of its own, __restrict__: beside the kernel's vector stores that is what lets the compiler
// read it with scalar loads.
// A source outside [0, B) -- no index of the caller's is used unchecked -- writes L rows of NaN without reading q; so does a q row that holds
// a NaN anywhere (a first pass over the row: the spheres of link 0 are emitted before the joints are read).
// ------------------------------------------------------------------------------------------------
struct LinkFrame { double r00, r01, r02, p0, r10, r11, r12, p1, r20, r21, r22, p2; };

// X <- X Jz(q): a rotation about, or a shift along, the frame's own z
__device__ __forceinline__ void link_joint(LinkFrame& X, int jtype, double q) {
    if (jtype == 0) {
        double s, c;
        sincos_fast(q, s, c);
        const double a0 = X.r00, a1 = X.r10, a2 = X.r20;
        X.r00 = __builtin_fma(X.r01, s, a0 * c); X.r01 = __builtin_fma(-a0, s, X.r01 * c);
        X.r10 = __builtin_fma(X.r11, s, a1 * c); X.r11 = __builtin_fma(-a1, s, X.r11 * c);
        X.r20 = __builtin_fma(X.r21, s, a2 * c); X.r21 = __builtin_fma(-a2, s, X.r21 * c);
    } else {
        X.p0 = __builtin_fma(X.r02, q, X.p0);
        X.p1 = __builtin_fma(X.r12, q, X.p1);
        X.p2 = __builtin_fma(X.r22, q, X.p2);
    }
}

// one row of X <- X [Rb | pb]
__device__ __forceinline__ void link_fixed_row(double& r0, double& r1, double& r2, double& p, const double* __restrict__ b) {
    const double a0 = r0, a1 = r1, a2 = r2;
    r0 = __builtin_fma(a2, b[8], __builtin_fma(a1, b[4], a0 * b[0]));
    r1 = __builtin_fma(a2, b[9], __builtin_fma(a1, b[5], a0 * b[1]));
    r2 = __builtin_fma(a2, b[10], __builtin_fma(a1, b[6], a0 * b[2]));
    p = __builtin_fma(a2, b[11], __builtin_fma(a1, b[7], __builtin_fma(a0, b[3], p)));
}

template <typename T>
__global__ void __launch_bounds__(256) link_kernel(const LinkImage* __restrict__ im, const LinkArgs a) {
    typedef typename FollowQuad<T>::type Quad;
    const int b = (int)(blockIdx.x * 256 + threadIdx.x);
    if (b >= a.B) return;
    const int n = im->n, L = im->L;
    const int s = a.src_arm ? a.src_arm[b] : b;
    bool bad = s < 0 || s >= a.B;
    const T* const qs = static_cast<const T*>(a.q) + (long)(bad ? 0 : s) * n;
    if (!bad)
        for (int i = 0; i < n; ++i) {
            const T v = qs[i];
            bad = bad || v != v;
        }
    // where the source's base stands as seen from this arm's base: taken as given, rotation or not
    double t00 = 1, t01 = 0, t02 = 0, t03 = 0, t10 = 0, t11 = 1, t12 = 0, t13 = 0, t20 = 0, t21 = 0, t22 = 1, t23 = 0;
    if (a.xform12) {
        const T* const x = static_cast<const T*>(a.xform12) + (long)b * 12;
        t00 = (double)x[0]; t01 = (double)x[1]; t02 = (double)x[2]; t03 = (double)x[3];
        t10 = (double)x[4]; t11 = (double)x[5]; t12 = (double)x[6]; t13 = (double)x[7];
        t20 = (double)x[8]; t21 = (double)x[9]; t22 = (double)x[10]; t23 = (double)x[11];
    }
    Quad* const out = static_cast<Quad*>(a.rep4) + (long)b * a.n_rep + a.first_rep;
    Quad* const trj = a.traj ? static_cast<Quad*>(a.traj) + (long)b * L : nullptr;
    const T nan = (T)__builtin_nan("");
    LinkFrame X = {im->B[0][0], im->B[0][1], im->B[0][2], im->B[0][3], im->B[0][4], im->B[0][5],
                   im->B[0][6], im->B[0][7], im->B[0][8], im->B[0][9], im->B[0][10], im->B[0][11]};
    int j = 0;
    for (int i = 0;; ++i) {
        for (; j < L && im->link[j] == i; ++j) {
            const double cx = im->c[j][0], cy = im->c[j][1], cz = im->c[j][2];
            double px = __builtin_fma(X.r02, cz, __builtin_fma(X.r01, cy, __builtin_fma(X.r00, cx, X.p0)));
            double py = __builtin_fma(X.r12, cz, __builtin_fma(X.r11, cy, __builtin_fma(X.r10, cx, X.p1)));
            double pz = __builtin_fma(X.r22, cz, __builtin_fma(X.r21, cy, __builtin_fma(X.r20, cx, X.p2)));
            if (a.xform12) {
                const double ux = px, uy = py, uz = pz;
                px = __builtin_fma(t02, uz, __builtin_fma(t01, uy, __builtin_fma(t00, ux, t03)));
                py = __builtin_fma(t12, uz, __builtin_fma(t11, uy, __builtin_fma(t10, ux, t13)));
                pz = __builtin_fma(t22, uz, __builtin_fma(t21, uy, __builtin_fma(t20, ux, t23)));
            }
            Quad v;
            v.x = bad ? nan : (T)px; v.y = bad ? nan : (T)py; v.z = bad ? nan : (T)pz; v.w = bad ? nan : (T)im->c[j][3];
            const int row = im->perm[j];
            out[row] = v;
            if (trj) trj[row] = v;
        }
        if (i >= n) break;
        link_joint(X, im->jtype[i], bad ? 0.0 : (double)qs[i]);
        const double* __restrict__ const Bn = im->B[i + 1];
        link_fixed_row(X.r00, X.r01, X.r02, X.p0, Bn);
        link_fixed_row(X.r10, X.r11, X.r12, X.p1, Bn);
        link_fixed_row(X.r20, X.r21, X.r22, X.p2, Bn);
    }
}

// ------------------------------------------------------------------------------------------------
// vfik_link_clearance: the room between an arm's own link spheres and a set of other spheres (ClearArgs, vfik_kernel.h).  link_kernel's walk
// with another thing done at every sphere: one lane per arm b walks its OWN chain from q[b] -- link_joint, link_fixed_row, twelve named
// doubles, the image read at uniform addresses -- and when the walk stands at a link, every sphere of that link meets the arm's `count` rows
// of pts4: the distance from the coordinate differences in float64, less both radii.  The running minimum is one double and one code; the
// pair mask comes by value in the image's sorted order and is indexed by the uniform sphere counter alone (a scalar load from the kernel
// arguments), so a masked pair costs a scalar branch and no load.  The kernel visits own spheres in LINK order, not the caller's: a tie is
// settled by a compare on the code.  No register array indexed at run time, no scratch.
// The rows: an arm's `count` rows are wanted once per own sphere, up to 16 times, and lie at a per-lane stride of n_rep quads in memory.  They
// are read from there ONCE and staged in LDS -- 16-byte units, unit u of lane t at [u * 64 + t]: a wave's ds_read_b128 covers 1 KiB of
// consecutive banks, no conflict -- in blocks of ONE wave: count KiB of dynamic LDS at float32, twice that at float64, 64 KiB at the most, so
// a CU's 160 KiB hold two workgroups (float64, count 32) or more -- at count 8 and under as many as there are wave slots.  Every lane reads back only what it wrote: no barrier.  Against
// re-reading the rows through the cache this is 19 % (float32) to 28 % (float64) faster at L = count = 8 and 2 to 4 % slower at 3
// (profiles/clearance_cost.txt).
// With a gate (the wait rule of the timed moves) the lane then decides whether its arm waits through the block that follows.
// ------------------------------------------------------------------------------------------------
typedef unsigned int ClearU4 __attribute__((ext_vector_type(4)));
typedef float ClearF4 __attribute__((ext_vector_type(4)));
typedef double ClearD2 __attribute__((ext_vector_type(2)));

// a staged row, its 16-byte units 64 apart, widened exactly
__device__ __forceinline__ void clear_row(const ClearU4* p, float, double& x, double& y, double& z, double& w) {
    const ClearF4 f = (ClearF4)p[0];
    x = (double)f.x; y = (double)f.y; z = (double)f.z; w = (double)f.w;
}
__device__ __forceinline__ void clear_row(const ClearU4* p, double, double& x, double& y, double& z, double& w) {
    const ClearD2 a = (ClearD2)p[0], b = (ClearD2)p[64];
    x = a.x; y = a.y; z = b.x; w = b.y;
}

template <typename T>
__global__ void __launch_bounds__(64) clear_kernel(const LinkImage* __restrict__ im, const ClearArgs a) {
    constexpr int U = (int)(4 * sizeof(T) / 16);   // 16-byte units per row
    extern __shared__ ClearU4 clear_lds[];
    const int b = (int)(blockIdx.x * 64 + threadIdx.x);
    if (b >= a.B) return;
    const int n = im->n, L = im->L, count = a.count;
    const T* const qs = static_cast<const T*>(a.q) + (long)b * n;
    bool bad = false;
    for (int i = 0; i < n; ++i) {
        const T v = qs[i];
        bad = bad || v != v;
    }
    const ClearU4* const rows = static_cast<const ClearU4*>(a.pts4) + ((long)b * a.n_rep + a.first) * U;
    for (int u = 0; u < count * U; ++u) clear_lds[u * 64 + threadIdx.x] = rows[u];
    double best = __builtin_inf();
    int code = -1;
    LinkFrame X = {im->B[0][0], im->B[0][1], im->B[0][2], im->B[0][3], im->B[0][4], im->B[0][5],
                   im->B[0][6], im->B[0][7], im->B[0][8], im->B[0][9], im->B[0][10], im->B[0][11]};
    int j = 0;
    for (int i = 0;; ++i) {
        for (; j < L && im->link[j] == i; ++j) {
            const unsigned m = a.mask[j];
            if (m == 0u) continue;
            const double cx = im->c[j][0], cy = im->c[j][1], cz = im->c[j][2], ri = im->c[j][3];
            const double px = __builtin_fma(X.r02, cz, __builtin_fma(X.r01, cy, __builtin_fma(X.r00, cx, X.p0)));
            const double py = __builtin_fma(X.r12, cz, __builtin_fma(X.r11, cy, __builtin_fma(X.r10, cx, X.p1)));
            const double pz = __builtin_fma(X.r22, cz, __builtin_fma(X.r21, cy, __builtin_fma(X.r20, cx, X.p2)));
            const int own = im->perm[j] * 32;
            for (int r = 0; r < count; ++r) {
                if (!((m >> r) & 1u)) continue;
                double x, y, z, R;
                clear_row(clear_lds + r * U * 64 + threadIdx.x, T(), x, y, z, R);
                const double dx = px - x, dy = py - y, dz = pz - z;
                const double d = (sqrt(__builtin_fma(dz, dz, __builtin_fma(dy, dy, dx * dx))) - ri) - R;
                const bool row_ok = x == x && y == y && z == z && R == R;   // a NaN row is "leave as it is": no obstacle
                const int c = own + r;
                const bool take = row_ok && (code < 0 || d < best || (d == best && c < code));
                best = take ? d : best;
                code = take ? c : code;
            }
        }
        if (i >= n) break;
        link_joint(X, im->jtype[i], bad ? 0.0 : (double)qs[i]);
        const double* __restrict__ const Bn = im->B[i + 1];
        link_fixed_row(X.r00, X.r01, X.r02, X.p0, Bn);
        link_fixed_row(X.r10, X.r11, X.r12, X.p1, Bn);
        link_fixed_row(X.r20, X.r21, X.r22, X.p2, Bn);
    }
    const T out = bad ? (T)__builtin_nan("") : (T)best;
    if (bad) code = -1;
    if (a.clear) static_cast<T*>(a.clear)[b] = out;
    if (a.pair) a.pair[b] = code;
    if (a.gate) {   // the wait rule: strict, on the io-typed value, so NaN and +inf never wait
        const bool wait = a.gate[b] == 1 && (!a.yields || a.yields[b] != 0) && (double)out < a.min_clearance;
        if (wait) a.gate[b] = 0;
        if (a.waited) a.waited[b] = (a.first_block ? 0 : a.waited[b]) + (wait ? 1 : 0);
    }
}

// ------------------------------------------------------------------------------------------------
// vfik_link_avoid: link spheres that push their own joints (AvoidArgs, vfik_kernel.h).  clear_kernel's walk once more -- one lane per arm, one
// wave a block, link_joint, link_fixed_row, twelve named doubles, the image at uniform addresses, the mask by value in the image's order --
// and at every own sphere P_i a repulsive velocity from the rows it is close to,
//     F_i = g_b sum_j a_ij (P_i - Q_j) / s_ij,   a_ij = 1 - (s_ij - r_i - R_j) / d0 > 0,  s_ij > 0      (strict: a NaN row, a NaN radius never push)
// which the Jacobian transpose of that point turns into a joint command: tau_k = sum over the spheres beyond joint k of z_k . ((P_i - o_k) x F_i),
// prismatic z_k . F_i.  ONE forward walk: with  z . ((P - o) x F) = z . (P x F) - (z x o) . F,  T_F = sum F_i, T_N = sum P_i x F_i and the same
// sums over the spheres up to link k,
//     revolute  tau_k = (z_k . T_N - m_k . T_F) - c_k,  c_k = z_k . Pre_N(k) - m_k . Pre_F(k),  m_k = z_k x o_k;    prismatic  tau_k = z_k . T_F - z_k . Pre_F(k)
// When the walk stands at link k it has emitted exactly the spheres of links <= k, so the running totals ARE the prefix sums: it keeps z_k,
// m_k, c_k -- seven doubles a joint -- and a loop over the joints finishes once the totals are known.  Those doubles go to LDS, double s of
// lane t at [s * 64 + t]: a wave's ds_write_b64 / ds_read_b64 covers 512 consecutive bytes, no bank conflict, a lane reads only what it
// wrote, no barrier.  No register array indexed at run time, no scratch.  n x 3.5 KiB; behind them the arm's rows, staged as clear_kernel
// stages them where both fit into 64 KiB, else (a.stage == 0, uniform) read through the cache at every sphere (launch_avoid).
// A NaN in q[b]: a row of zeros (one NaN command would poison qdot_out through a zero mixer weight); no active pair: zeros, +0 each.  Every
// arm b < B is written on every call, each destination once.
// Resources (tools/resusage.py): 104 VGPRs and 73 SGPRs in either I/O type, no scratch, no static LDS; dynamic LDS as launch_avoid says.
// ------------------------------------------------------------------------------------------------
// a row at its place in memory, its 16-byte units side by side, widened exactly
__device__ __forceinline__ void avoid_row_mem(const ClearU4* p, float, double& x, double& y, double& z, double& w) {
    clear_row(p, 0.0f, x, y, z, w);
}
__device__ __forceinline__ void avoid_row_mem(const ClearU4* p, double, double& x, double& y, double& z, double& w) {
    const ClearD2 a = (ClearD2)p[0], b = (ClearD2)p[1];
    x = a.x; y = a.y; z = b.x; w = b.y;
}

template <typename T>
__global__ void __launch_bounds__(64) avoid_kernel(const LinkImage* __restrict__ im, const AvoidArgs a) {
    constexpr int U = (int)(4 * sizeof(T) / 16);   // 16-byte units per row
    extern __shared__ ClearU4 avoid_lds[];
    const int b = (int)(blockIdx.x * 64 + threadIdx.x);
    if (b >= a.B) return;
    const int n = im->n, L = im->L, count = a.count;
    double* const jl = reinterpret_cast<double*>(avoid_lds) + threadIdx.x;   // the joints' doubles: 7 n slots of 64
    ClearU4* const rl = avoid_lds + n * (7 * 64 * 8 / 16) + threadIdx.x;     // the staged rows behind them
    const T* const qs = static_cast<const T*>(a.q) + (long)b * n;
    bool bad = false;
    for (int i = 0; i < n; ++i) {
        const T v = qs[i];
        bad = bad || v != v;
    }
    const ClearU4* const rows = static_cast<const ClearU4*>(a.pts4) + ((long)b * a.n_rep + a.first) * U;
    const bool stage = a.stage != 0;
    if (stage)
        for (int u = 0; u < count * U; ++u) rl[u * 64] = rows[u];
    const double g = a.gain * (a.scale ? (double)static_cast<const T*>(a.scale)[b] : 1.0), d0 = a.d0;
    double tfx = 0, tfy = 0, tfz = 0, tnx = 0, tny = 0, tnz = 0;
    bool any = false;
    LinkFrame X = {im->B[0][0], im->B[0][1], im->B[0][2], im->B[0][3], im->B[0][4], im->B[0][5],
                   im->B[0][6], im->B[0][7], im->B[0][8], im->B[0][9], im->B[0][10], im->B[0][11]};
    int j = 0;
    for (int i = 0;; ++i) {
        for (; j < L && im->link[j] == i; ++j) {
            const unsigned m = a.mask[j];
            if (m == 0u) continue;
            const double cx = im->c[j][0], cy = im->c[j][1], cz = im->c[j][2], ri = im->c[j][3];
            const double px = __builtin_fma(X.r02, cz, __builtin_fma(X.r01, cy, __builtin_fma(X.r00, cx, X.p0)));
            const double py = __builtin_fma(X.r12, cz, __builtin_fma(X.r11, cy, __builtin_fma(X.r10, cx, X.p1)));
            const double pz = __builtin_fma(X.r22, cz, __builtin_fma(X.r21, cy, __builtin_fma(X.r20, cx, X.p2)));
            double fx = 0, fy = 0, fz = 0;
            for (int r = 0; r < count; ++r) {
                if (!((m >> r) & 1u)) continue;
                double x, y, z, R;
                if (stage) clear_row(rl + r * U * 64, T(), x, y, z, R);
                else avoid_row_mem(rows + r * U, T(), x, y, z, R);
                const double dx = px - x, dy = py - y, dz = pz - z;
                const double s = sqrt(__builtin_fma(dz, dz, __builtin_fma(dy, dy, dx * dx)));
                const double act = 1.0 - ((s - ri) - R) / d0;
                const bool on = act > 0.0 && s > 0.0;   // (a NaN anywhere in the row makes act NaN: no obstacle)
                const double w = on ? act / s : 0.0;
                fx = __builtin_fma(w, on ? dx : 0.0, fx);
                fy = __builtin_fma(w, on ? dy : 0.0, fy);
                fz = __builtin_fma(w, on ? dz : 0.0, fz);
                any = any || on;
            }
            fx *= g; fy *= g; fz *= g;
            tfx += fx; tfy += fy; tfz += fz;
            tnx += py * fz - pz * fy;
            tny += pz * fx - px * fz;
            tnz += px * fy - py * fx;
        }
        if (i >= n) break;
        {   // joint i turns about / shifts along z of X_i through its origin; the totals so far are the sums over the links <= i
            const double zx = X.r02, zy = X.r12, zz = X.r22;
            const double mx = zy * X.p2 - zz * X.p1, my = zz * X.p0 - zx * X.p2, mz = zx * X.p1 - zy * X.p0;
            const double zf = __builtin_fma(zz, tfz, __builtin_fma(zy, tfy, zx * tfx));
            const double zn = __builtin_fma(zz, tnz, __builtin_fma(zy, tny, zx * tnx));
            const double mf = __builtin_fma(mz, tfz, __builtin_fma(my, tfy, mx * tfx));
            double* const s = jl + i * (7 * 64);
            s[0] = zx; s[64] = zy; s[128] = zz; s[192] = mx; s[256] = my; s[320] = mz;
            s[384] = im->jtype[i] == 0 ? zn - mf : zf;
        }
        link_joint(X, im->jtype[i], bad ? 0.0 : (double)qs[i]);
        const double* __restrict__ const Bn = im->B[i + 1];
        link_fixed_row(X.r00, X.r01, X.r02, X.p0, Bn);
        link_fixed_row(X.r10, X.r11, X.r12, X.p1, Bn);
        link_fixed_row(X.r20, X.r21, X.r22, X.p2, Bn);
    }
    const bool zero = bad || !any;
    T* const out = a.out ? static_cast<T*>(a.out) + (long)b * n : nullptr;
    T* const chan = a.chan_out ? static_cast<T*>(a.chan_out) + (long)b * n : nullptr;
    T* const trj = a.traj ? static_cast<T*>(a.traj) + (long)b * n : nullptr;
    for (int k = 0; k < n; ++k) {
        const double* const s = jl + k * (7 * 64);
        const double zx = s[0], zy = s[64], zz = s[128], mx = s[192], my = s[256], mz = s[320], c = s[384];
        const double zf = __builtin_fma(zz, tfz, __builtin_fma(zy, tfy, zx * tfx));
        const double zn = __builtin_fma(zz, tnz, __builtin_fma(zy, tny, zx * tnx));
        const double mf = __builtin_fma(mz, tfz, __builtin_fma(my, tfy, mx * tfx));
        const double tau = (im->jtype[k] == 0 ? zn - mf : zf) - c;
        const T v = zero ? (T)0 : (T)tau;
        if (out) out[k] = v;
        if (chan) chan[k] = v;
        if (trj) trj[k] = v;
    }
}

}  // namespace

// Dynamic LDS of avoid_kernel: the joints' doubles, n x 7 x 64 x 8 bytes = n x 3.5 KiB (56 KiB at 16 joints), and behind them the arm's rows as
// clear_kernel stages them, count KiB at float32, twice that at float64 -- WHERE BOTH FIT INTO 64 KiB.  Where they do not (16 joints and more
// than 8 rows of float32 or 4 of float64, say) the rows stay where they are and every own sphere reads them through the cache: a.stage = 0.
hipError_t launch_avoid(int io_dtype, int n, AvoidArgs a, hipStream_t stream) {
    const dim3 grid((unsigned)((a.B + 63) / 64)), blk(64);
    const size_t joints = (size_t)n * 7 * 64 * 8, rows = (size_t)a.count * (io_dtype == 32 ? 1024 : 2048);
    a.stage = joints + rows <= 65536 ? 1 : 0;
    const size_t lds = joints + (a.stage ? rows : 0);
    if (io_dtype == 32) hipLaunchKernelGGL(avoid_kernel<float>, grid, blk, lds, stream, a.img, a);
    else hipLaunchKernelGGL(avoid_kernel<double>, grid, blk, lds, stream, a.img, a);
    return hipGetLastError();
}

hipError_t launch_clear(int io_dtype, const ClearArgs& a, hipStream_t stream) {
    const dim3 grid((unsigned)((a.B + 63) / 64)), blk(64);   // one wave a block; the arm's rows: count x 16 bytes (float64: 32) a lane of LDS
    if (io_dtype == 32) hipLaunchKernelGGL(clear_kernel<float>, grid, blk, (size_t)a.count * 1024, stream, a.img, a);
    else hipLaunchKernelGGL(clear_kernel<double>, grid, blk, (size_t)a.count * 2048, stream, a.img, a);
    return hipGetLastError();
}

hipError_t launch_link(int io_dtype, const LinkArgs& a, hipStream_t stream) {
    const dim3 grid((unsigned)((a.B + 255) / 256)), blk(256);
    if (io_dtype == 32) hipLaunchKernelGGL(link_kernel<float>, grid, blk, 0, stream, a.img, a);
    else hipLaunchKernelGGL(link_kernel<double>, grid, blk, 0, stream, a.img, a);
    return hipGetLastError();
}

hipError_t launch_cycle(int io_dtype, int nj, const KArgs& kargs, int block, hipStream_t stream, CyclePlan* plan_out) {
    const bool ns = kargs.flags & VFIK_F_NULLSPACE;
    const CyclePlan plan = plan_cycle(kargs, nj, io_dtype, ns, block);
    if (plan_out) *plan_out = plan;
    switch (nj) {
#define X(n)                                                                                                                        \
    case n:                                                                                                                         \
        return io_dtype == 32 ? (ns ? launch_cycle_nj##n##_t32_ns1(kargs, plan, stream) : launch_cycle_nj##n##_t32_ns0(kargs, plan, stream))  \
                              : (ns ? launch_cycle_nj##n##_t64_ns1(kargs, plan, stream) : launch_cycle_nj##n##_t64_ns0(kargs, plan, stream));
        VFIK_NJ_LIST
#undef X
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_mix(int io_dtype, const void* cmds, const double* w_dev, int K, long count, long chan_stride,
                      void* out, hipStream_t stream) {
    const int block = 256;
    const dim3 grid((unsigned)((count + block - 1) / block)), blk(block);
    if (io_dtype == 32)
        hipLaunchKernelGGL(mix_kernel<float>, grid, blk, 0, stream, static_cast<const float*>(cmds), w_dev, K, count,
                           chan_stride, static_cast<float*>(out));
    else
        hipLaunchKernelGGL(mix_kernel<double>, grid, blk, 0, stream, static_cast<const double*>(cmds), w_dev, K, count,
                           chan_stride, static_cast<double*>(out));
    return hipGetLastError();
}

hipError_t launch_probe(int io_dtype, const void* pose, const void* goal, const void* slots, int B, long Bp, int slots_used,
                        double rot_slow, double cos_slow, void* out, hipStream_t stream) {
    const int block = 64;
    const dim3 grid((B + block - 1) / block), blk(block);
    if (io_dtype == 32)
        hipLaunchKernelGGL(probe_kernel<float>, grid, blk, 0, stream, static_cast<const float*>(pose), static_cast<const float*>(goal),
                           static_cast<const float*>(slots), B, Bp, slots_used, rot_slow, cos_slow, static_cast<float*>(out));
    else
        hipLaunchKernelGGL(probe_kernel<double>, grid, blk, 0, stream, static_cast<const double*>(pose), static_cast<const double*>(goal),
                           static_cast<const double*>(slots), B, Bp, slots_used, rot_slow, cos_slow, static_cast<double*>(out));
    return hipGetLastError();
}

hipError_t launch_monitor(int io_dtype, const void* pose, const void* frames, int O, long count, void* out, hipStream_t stream, const int* active) {
    const int block = 256;
    const dim3 grid((unsigned)((count + block - 1) / block)), blk(block);
    if (io_dtype == 32)
        hipLaunchKernelGGL(monitor_kernel<float>, grid, blk, 0, stream, static_cast<const float*>(pose),
                           static_cast<const float*>(frames), O, count, static_cast<float*>(out), active);
    else
        hipLaunchKernelGGL(monitor_kernel<double>, grid, blk, 0, stream, static_cast<const double*>(pose),
                           static_cast<const double*>(frames), O, count, static_cast<double*>(out), active);
    return hipGetLastError();
}

hipError_t launch_move(int io_dtype, const MoveArgs& m, hipStream_t stream) {
    const int lanes = (m.first_arm & 63) + m.n_arms;
    const dim3 grid((unsigned)((lanes + 255) / 256), (unsigned)((m.goal16 ? 1 : 0) + (m.rep4 ? m.n_rep : 0))), blk(256);
    const bool vec = (((uintptr_t)m.goal16 | (uintptr_t)m.rep4) & 15u) == 0;
    if (io_dtype == 32) {
        if (vec) hipLaunchKernelGGL((move_kernel<float, true>), grid, blk, 0, stream, m);
        else hipLaunchKernelGGL((move_kernel<float, false>), grid, blk, 0, stream, m);
    } else {
        if (vec) hipLaunchKernelGGL((move_kernel<double, true>), grid, blk, 0, stream, m);
        else hipLaunchKernelGGL((move_kernel<double, false>), grid, blk, 0, stream, m);
    }
    return hipGetLastError();
}

hipError_t launch_move_scene(int io_dtype, const SceneMoveArgs& s, hipStream_t stream) {
    const MoveArgs& m = s.m;
    const int lanes = (m.first_arm & 63) + m.n_arms;
    const int rows = (m.goal16 ? 1 : 0) + (m.rep4 ? m.n_rep : 0) + (s.fun6 ? s.n_fun : 0) + (s.hem6 ? s.n_hem : 0) + (s.att16 ? s.n_att : 0);
    if (rows < 1) return hipSuccess;
    const dim3 grid((unsigned)((lanes + 255) / 256), (unsigned)rows), blk(256);
    const size_t pair = io_dtype == 32 ? 8 : 16;
    const bool vec = (((uintptr_t)m.goal16 | (uintptr_t)m.rep4 | (uintptr_t)s.att16) & 15u) == 0 && (((uintptr_t)s.fun6 | (uintptr_t)s.hem6) & (pair - 1)) == 0;
    if (io_dtype == 32) {
        if (vec) hipLaunchKernelGGL((move_scene_kernel<float, true>), grid, blk, 0, stream, s);
        else hipLaunchKernelGGL((move_scene_kernel<float, false>), grid, blk, 0, stream, s);
    } else {
        if (vec) hipLaunchKernelGGL((move_scene_kernel<double, true>), grid, blk, 0, stream, s);
        else hipLaunchKernelGGL((move_scene_kernel<double, false>), grid, blk, 0, stream, s);
    }
    return hipGetLastError();
}

hipError_t launch_track(int io_dtype, const void* pose, const void* v6, double* state, void* out, const int* active, int B, hipStream_t stream) {
    const int block = 256;
    const dim3 grid((B + block - 1) / block), blk(block);
    if (io_dtype == 32)
        hipLaunchKernelGGL(track_kernel<float>, grid, blk, 0, stream, static_cast<const float*>(pose), static_cast<const float*>(v6),
                           state, static_cast<float*>(out), active, B);
    else
        hipLaunchKernelGGL(track_kernel<double>, grid, blk, 0, stream, static_cast<const double*>(pose),
                           static_cast<const double*>(v6), state, static_cast<double*>(out), active, B);
    return hipGetLastError();
}

hipError_t launch_check(int io_dtype, bool joint, bool list, const CheckArgs& g, hipStream_t stream, const StallArgs* st) {
    const dim3 grid((unsigned)((g.B + 255) / 256)), blk(256);
    auto launch = [&](auto t) {
        typedef decltype(t) T;
        if (st) {   // the handle has a stall rule
            if (joint) {
                if (list) hipLaunchKernelGGL((check_stall_kernel<T, true, true>), grid, blk, 0, stream, g, *st);
                else hipLaunchKernelGGL((check_stall_kernel<T, true, false>), grid, blk, 0, stream, g, *st);
            } else {
                if (list) hipLaunchKernelGGL((check_stall_kernel<T, false, true>), grid, blk, 0, stream, g, *st);
                else hipLaunchKernelGGL((check_stall_kernel<T, false, false>), grid, blk, 0, stream, g, *st);
            }
        } else if (joint) {
            if (list) hipLaunchKernelGGL((check_kernel<T, true, true>), grid, blk, 0, stream, g);
            else hipLaunchKernelGGL((check_kernel<T, true, false>), grid, blk, 0, stream, g);
        } else {
            if (list) hipLaunchKernelGGL((check_kernel<T, false, true>), grid, blk, 0, stream, g);
            else hipLaunchKernelGGL((check_kernel<T, false, false>), grid, blk, 0, stream, g);
        }
    };
    if (io_dtype == 32) launch(0.0f);
    else launch(0.0);
    return hipGetLastError();
}

hipError_t launch_script(int io_dtype, const ScriptArgs& s, hipStream_t stream, const StallArgs* st) {
    const dim3 grid((unsigned)((s.c.B + 255) / 256)), blk(256);
    if (st) {   // the handle has a stall rule
        if (io_dtype == 32) hipLaunchKernelGGL(script_stall_kernel<float>, grid, blk, 0, stream, s, *st);
        else hipLaunchKernelGGL(script_stall_kernel<double>, grid, blk, 0, stream, s, *st);
    } else if (io_dtype == 32) hipLaunchKernelGGL(script_kernel<float>, grid, blk, 0, stream, s);
    else hipLaunchKernelGGL(script_kernel<double>, grid, blk, 0, stream, s);
    return hipGetLastError();
}
}  // namespace vfik
