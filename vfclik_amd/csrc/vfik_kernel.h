// vfik_kernel.h -- kernel argument blocks, the launch plan and the type-erased launchers shared by vfik_kernel.hip, vfik_aux.hip (device) and
// vfik_abi.cpp (host).  The chain's constants (KConst, kconst_fill, the DH patterns) are vfik_kconst.h, plain host code, included here.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdio>
#include <string>

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/vfik_types.h"
#include "vfik_kconst.h"
#include "vfik_links.h"

namespace vfik {

// Device data layout (DESIGN.md "Data layout in HBM").  T = io dtype (float | double), B = batch,
// Bpad = B rounded up to 64.  A "quad" is T[4] (16 or 32 bytes); a quad PLANE is Bpad quads, one per
// arm, so that the 64 lanes of a wave read 1 KiB (2 KiB) of contiguous memory with one (two)
// 16-byte-per-lane request(s).
//   q, qdot_*, qdist      [B][n]      batch-major (the reference's bottles: n doubles per arm)
//   pose, pose_nt         [B][16]
//   goal                  4 planes    frame rows 0,1,2 | (present, slow-down, force, speedScale of the arm)
//   funnel                3 planes    the arm's funnel attractor (object_feeder:262-279: the approach cone of a goal with a normal), if it is
//                                     the only non-repeller entry of the set: (x y z ax | ay az cutAngle angleOrder | cutDist distOrder force present)
//   hemisphere            3 planes    likewise the arm's ONE hemisphere repeller (object_feeder:344-353): (x y z nx | ny nz safeDist order | force present - -)
//   slots_fast            3 ceil(S/2) planes  decay repellers only, two slots in three quads: (x0 y0 z0 r0 | s0 f0 x1 y1 | z1 r1 s1 f1);
//                                     what the straight-line field path reads (24 instead of 32 bytes a slot at float I/O)
//   orders                ceil(S/16) planes of 16 BYTES per arm (whatever T): byte m % 16 of plane m / 16 = integer decay order of compact-image
//                                     slot m (< 128; unused slots carry 5): read by the MIXO kernel variants when the batch's orders differ
//   slots                 2S planes   slot m = planes 2m, 2m+1 = (p0 p1 p2 p3 | p4 p5 force type);
//                                     type -1 = continuation of the previous slot (p6..p11 / p12..p16),
//                                     type 0 = empty
//   tool (per-arm only)   3 planes    frame rows 0,1,2 (a shared tool lives in KConst)
//   mixw (per-arm only)   2 planes    mixer weights w0..w3 | w4 w5 - -  (shared weights live in KConst)
//   lastvec               [(n + 4) / 4][Bpad] quads of FLOAT: the unique basis vector of the last cycle (n values), then
//                                     sig as +-1 / +-2 (nullspace:91-92; vfik_kernel.hip); chains of up to 7 joints only
//   ext                   [4][B][n]   last commands of mixer channels 2..5
// (Batch-shared constants -- chain geometry, limits and parameters -- are KConst<NJ>: vfik_kconst.h.)

// Per-wave LDS region of the cycle kernel (vfik_kernel.hip, cycle_body), by I/O type T.
template <typename T> struct Stage {
    // Slots staged at a time (prefetch window / chunk size).  float64 I/O stages 4: with 8 the region is 56 KB
    // and only three of a CU's four SIMDs get a wave (160 KB LDS) -- the launch then runs in two rounds
    // (measured 15.3 us instead of ~8 for the C3 batch).
    static constexpr int PRE = sizeof(T) == 8 ? 4 : 8;
    static constexpr int Q16 = (int)sizeof(T) / 4;           // 16-B pieces per quad
    static constexpr int QBYTES = 4 * (int)sizeof(T);        // bytes of one quad
    static constexpr int QSTEP = Q16 * 1024;                 // LDS bytes of one staged quad (a 1-KiB row per 16 bytes per lane)
    static constexpr int QPCF = 3 * PRE / 2;                 // quads of one chunk of the compact repeller image
    // Region of one wave, in the order [goal 4 | slot quads 0 .. QPCF-1 | q | kinematics | table] -- that much is all a LEAN
    // launch on the straight-line path touches (`lean_bytes`: 19.75 KB for 7 joints with float I/O, eight waves per CU) --
    // then [slot quads QPCF .. 2 PRE - 1 | tool 3 | mixer weights 2] for the general path and the optional per-arm inputs.
    static constexpr int GOAL_OFF = 0, SLOT_OFF = 4 * QSTEP, Q_OFF = (4 + QPCF) * QSTEP;
    // q is batch-major ([B][n]): a lane's n values are contiguous and travel as 16-byte pieces plus a
    // remainder of one to three 4-byte pieces (a 12-byte LDS-DMA did not land lane-linear on gfx950)
    __host__ __device__ static constexpr int qbytes(int nj) { return nj * (int)sizeof(T); }
    __host__ __device__ static constexpr int q16(int nj) { return qbytes(nj) / 16; }
    __host__ __device__ static constexpr int qrem(int nj) { return qbytes(nj) % 16; }
    __host__ __device__ static constexpr int qregion(int nj) { return q16(nj) * 1024 + qrem(nj) * 64; }
    __host__ __device__ static constexpr int kin_rows(int nj) { return ((12 + 10 * nj + 4 + 10 + VFIK_MIX_CHANNELS + 12 + 6 + nj) * 8 + 1023) / 1024; }  // = KConst<nj>::KIN_ROWS
    __host__ __device__ static constexpr int kin_off(int nj) { return Q_OFF + qregion(nj); }
    __host__ __device__ static constexpr int tab_off(int nj) { return kin_off(nj) + kin_rows(nj) * 1024; }  // sin / cos table, 1 KiB
    __host__ __device__ static constexpr int lean_bytes(int nj) { return tab_off(nj) + 1024; }
    __host__ __device__ static constexpr int slot_off(int idx, int nj) {  // slot quad idx of the staged chunk
        return idx < QPCF ? SLOT_OFF + idx * QSTEP : lean_bytes(nj) + (idx - QPCF) * QSTEP;
    }
    __host__ __device__ static constexpr int tool_off(int nj) { return lean_bytes(nj) + (2 * PRE - QPCF) * QSTEP; }
    __host__ __device__ static constexpr int mixw_off(int nj) { return tool_off(nj) + 3 * QSTEP; }
    __host__ __device__ static constexpr int bytes(int nj) { return mixw_off(nj) + 2 * QSTEP; }
};

// Chains longer than this have no registers left for loop-carried state: their rollout is a sequence of
// single-cycle launches that integrate q on the way out (vfik_abi.cpp), not the ROLL kernel variant.
#define VFIK_ROLL_MAX_NJ 7
// Chains of VFIK_HEAVY_MIN_NJ joints or more: the non-lean single-cycle variants are an object of their own (-DVFIK_HEAVY_PART, Makefile)
#ifndef VFIK_HEAVY_MIN_NJ
#define VFIK_HEAVY_MIN_NJ 12
#endif

struct KArgs {
    int B;
    int Bpad;         // B rounded up to 64: pitch of the quad planes
    int slots_used;
    int fast_order;   // >= 0: every used slot of every arm is a decay repeller (or empty) with this integer
                      // decay order (what object_feeder sends for point obstacles); -1: general path
    unsigned flags;
    int tool_stride;  // 0: one tool for the batch (KConst::tool); else per-arm tool quads ([3][Bpad])
    int plain;        // 0: the general variants; else the PLAIN kernels (vfik_kernel.hip), 1 + (the batch's shared tool is not the identity ? 1 : 0) + (its IK weights are not all one ? 2 : 0)
    int block;        // threads per block of the launch (read from here: blockDim.x costs its own scalar load)
    const void* q;
    const void* goal;
    const void* slots;
    const void* slots_fast;  // compact repeller image of the straight-line path: 3 quad planes per pair of slots (vfik_scene.h, pack_fields)
    const void* tool;
    const void* null_control;
    const void* ext;
    const void* mixw;  // per-arm mixer weights, 2 quad planes, or NULL (KConst::mix_w for every arm)
    const double* wts;    // per-arm IK weights [6 + n][Bpad] (wy rows, then wq rows), or NULL (KConst::wy / wq)
    const void* q_ref;    // [B][n] joint P controller reference (mixer channel 2), or NULL
    const void* q_cmded;  // [B][n] LWR echo of the commanded position (bridge:199-203 command form), or NULL
    float* lastvec;
    void* qdot_vf;
    void* qdot_null;
    void* qdot_out;
    void* pose;
    void* pose_nt;
    void* v6;
    void* qdist;
    void* goal_dist;  // [B][2] distance / rotation angle (degrees) to the goal block, or NULL
    int* status;
    unsigned long long* stamps;  // diagnostic builds only (-DVFIK_STAMPS): [waves][8] s_memtime values
    const void* kc;              // KConst<n> in device memory
    // closed-loop rollout (ROLL kernel variant): n_cycles control cycles per launch, q += dt * qdot_out
    void* q_out;                 // [B][n] joint angles after the last cycle, or NULL
    double dt;
    int n_cycles;                // 0: ordinary single-cycle launch
    int clamp;                   // keep q inside [q_lo, q_hi] after each integration step
    int status_or;               // OR the status bits into what a.status already holds (cycle 2.. of a stepped rollout)
    // ABI 3
    const int* active;           // [B] fresh-q gate (vf:312-313, nullspace:162-163): 0 = the arm stores nothing this launch; NULL = all
    const void* q_lo;            // [B][n] this cycle's joint limits per arm (nullspace:167, joint_p_controller:80), or NULL:
    const void* q_hi;            //        the chain's static limits of KConst
    void* q_ref_out;             // [B][n] the joint controller's reference after its clamp (joint_p_controller:121), or NULL
    int sub8_max_batch;          // batches up to this size take the eight-lanes-per-arm kernel when the launch is lean (0: never)
    int sub8_max_batch_ns;       // ... with the nullspace module, qdot_out / status only
    int sub8_max_batch_full;     // ... when the launch asks for more than qdot_out (the rows the per-arm processes publish every cycle)
    int n_simd;                  // SIMDs of the device (4 per CU): launches of at most that many waves are one wave per SIMD
    const void* funnel;          // aux block, 6 quad planes: funnel (x y z ax | ay az cutAngle angleOrder | cutDist distOrder force present) and
                                 // hemisphere (x y z nx | ny nz safeDist order | force present - -), or unused
    int slots_used_fast;         // slots of the COMPACT repeller image in use (an arm's funnel is not a slot there)
    int has_funnel;              // some arm's field set has a funnel attractor or a hemisphere repeller (straight-line path: the FUN kernel variants)
    const void* arena;           // the handle's state arena [goal | kconst | lastvec | slots_fast | slots] (arena_layout), or NULL
    int uni;                     // 1: every decay repeller of the batch shares one safe distance and one force (KConst::rep_safe, dh[0].pad): lean launches read the uniform image
    int uni_planes;              // quad planes of the compact image = offset of the uniform image behind slots_fast
    int waves2;                  // 1: lean straight-line float launches of more than n_simd waves take the two-waves-per-SIMD build (VFIK_TWO_WAVES=0: never)
    int one5;                    // 1: the uniform image holds ONE chunk of order-5 repellers and owns planes 1 ... PRE (vfik_set_fields): the lean float launches of
                                 // chains of up to 7 joints take cycle_kernel_s's one-chunk body (in what was padding: sizeof(KArgs) is unchanged)
    // round 4: decay repellers whose INTEGER orders differ (README.old:75 documents order 20 beside the feeder's 5, object_feeder:302)
    const void* orders;          // order planes: 16 bytes per arm and plane = the decay orders of 16 slots of the compact image, one byte each
    int mixed;                   // 1: the batch's repellers do not share one order -- the straight-line path reads `orders` (MIXO kernel variants)
    int dhp;                     // DH pattern of the chain the lean kernels may assume (DhPattern; 0: none) -- only with `plain`
};

// The per-handle device state a LEAN launch reads lives in ONE allocation with offsets that follow from (io type, joints, Bpad):
//   [goal: 4 quad planes | aux (funnel 3, hemisphere 3): 6 quad planes | kconst: KCONST_SLOT(nj) bytes | lastvec: (nj + 4) / 4 planes of 16 B | slots_fast ... | slots_uni ... | slots ...]
// so that such a launch's kernarg is one base pointer + the io pointers (KLean, 56 bytes) instead of the 340-byte KArgs: what a
// launch costs the HOST grows with its kernarg (tools/ubench_launch: 32-64 B 2.8 us, 336 B 3.9 us on a slow host), and at a
// 5-us launch period the enqueue loop is never far from being the bottleneck.
#define VFIK_KCONST_SLOT(kconst_bytes) ((((kconst_bytes) + 2048) + 255) / 256 * 256)
struct KLean {
    const void* base;            // the arena
    const void* q;
    void* qdot_out;
    int* status;
    int B, Bpad, slots_used, fast_order;   // (slots_used: of the compact image)
    unsigned flags;
    int block;
};
// KLean::fast_order of a uniform-image launch: the decay order (< 128) in bits 0-6, the image's offset in quad planes from bit 8 on, and
// bit 7: take the one-chunk order-5 body (cycle_kernel_s; the launcher sets it from KArgs::one5)
constexpr int ONE5_BIT = 128;
static_assert(sizeof(KArgs) == 352 && sizeof(KLean) == 56, "KArgs / KLean: the kernarg sizes the launch costs were measured with");

// ------------------------------------------------------------------------------------------------
// The launch plan of a control cycle: which kernel variant a launch takes, with which template arguments, grid, block and LDS.
// Plain host code (no HIP call): vfik_kernel.hip's launcher maps a plan to its instantiation, tests/c_host/launch_plan.cpp prints it.
// ------------------------------------------------------------------------------------------------
enum class CycleFamily {
    Refused,          // a rollout the kernels do not run in-kernel (rollout_in_kernel): the caller steps it (vfik_abi.cpp: launch_cycles)
    Sub8,             // eight lanes per arm (cycle_sub8_kernel): small batches of the outputs the per-arm processes publish
    Lean,             // q -> qdot_out on the straight-line field path (cycle_kernel_s, LEAN 1)
    LeanTwoWaves,     // ... beyond one wave per SIMD: two waves per SIMD (WAVES 2)
    PublishingLean,   // no per-arm option, the published rows at run time (cycle_kernel_x, LEAN 3)
    Mixo,             // decay orders that differ, lean or publishing-lean (cycle_kernel_m)
    Rollout,          // in-kernel rollout (ROLL, LEAN 0)
    RolloutLean,      // in-kernel rollout of a lean launch (ROLL, LEAN 1)
    SteppedCycle,     // one cycle of a host-stepped rollout of a long chain: lean, q integrated on the way out (LEAN 2)
    GeneralLean,      // q -> qdot_out on the general field path (LEAN 1, FASTF 0)
    Full,             // every other launch (LEAN 0); `heavy`: the long chains' object of its own
};

// the flag sets of the nullspace module in vfclik's default process set (nullspace + mixer; C5 adds the joint-limit task): the CF variants
constexpr int CF_NSMIX = VFIK_F_NULLSPACE | VFIK_F_MIXER, CF_NSJLMIX = CF_NSMIX | VFIK_F_JOINT_LIMIT_TASK;

struct CyclePlan {
    CycleFamily family;
    // the kernel's template arguments as compiled (cycle_kernel_s / _x / _m; Sub8: dhp alone)
    bool plain, roll, fastf;
    int lean;        // 0 general, 1 lean, 2 a stepped rollout's cycle, 3 publishing lean
    int cf;          // the flag set as a compile-time constant, or -1
    bool fun;
    int waves;
    bool uni, mixo;
    int dhp;         // DH-pattern bits the variant is built with (bit 0 pattern, bit 1 shared tool, bit 2 shared IK weights)
    bool heavy;      // Full of a long chain: launch_heavy_nj<n>
    unsigned grid, block;
    size_t lds;
    // kernel arguments the plan rewrites
    int fast_order;  // -1: the general field path; UNI: the uniform image's offset in the upper bits
    int slots_used;  // the straight-line path counts the slots of the compact image
};

// Whether an n_cycles > 0 launch runs as ONE in-kernel rollout (ROLL variants: PLAIN chains of up to 7 joints without shared options); else the
// caller steps it cycle by cycle -- with a tool, IK weights or prismatic joints the loop-carried state no longer fits the registers.
inline bool rollout_in_kernel(int nj, int plain) { return nj <= VFIK_ROLL_MAX_NJ && plain == 1; }

// ---- what a launch asks for (KArgs), as the plan reads it
// no per-arm option: tool, mixer weights, IK weights, extra mixer channels, joint controller, LWR command form, per-cycle limits
inline bool no_per_arm_option(const KArgs& a) {
    return !a.tool_stride && !a.mixw && !a.wts && !a.ext && !a.q_ref && !a.q_cmded && !a.q_lo && !a.q_ref_out;
}
inline bool single_cycle(const KArgs& a) { return !a.q_out && a.n_cycles == 0; }
// without the nullspace module a lean variant assumes no feature flag
inline bool lean_flags(const KArgs& a, bool ns) { return ns || a.flags == 0; }
// the rows the per-arm processes publish every cycle
inline bool publishes_rows(const KArgs& a) { return a.qdot_vf || a.qdot_null || a.pose || a.pose_nt || a.qdist; }
// nothing but q -> qdot_out (and status): no other input or output, whatever the field path (q_out may be a stepped rollout's)
inline bool qdot_out_only(const KArgs& a, bool ns) {
    return lean_flags(a, ns) && no_per_arm_option(a) && !publishes_rows(a) && !a.null_control && !a.v6 && !a.goal_dist && !a.active;
}
// the lean and publishing-lean single-cycle launches: the only ones with FUN and MIXO variants
inline bool lean_single(const KArgs& a, bool ns) { return lean_flags(a, ns) && no_per_arm_option(a) && single_cycle(a); }
// the launches the eight-lanes kernel serves (before the batch-size cap)
inline bool sub8_served(const KArgs& a, bool ns) {
    return no_per_arm_option(a) && single_cycle(a) && !a.active && !a.v6 && !a.goal_dist && a.qdot_out && (ns || (a.flags == 0 && !a.null_control));
}

namespace plan_detail {
struct Sizes { size_t bytes, lean, tool, qstep; };
inline Sizes sizes(int io_bits, int nj) {
    if (io_bits == 32) return {(size_t)Stage<float>::bytes(nj), (size_t)Stage<float>::lean_bytes(nj), (size_t)Stage<float>::tool_off(nj), (size_t)Stage<float>::QSTEP};
    return {(size_t)Stage<double>::bytes(nj), (size_t)Stage<double>::lean_bytes(nj), (size_t)Stage<double>::tool_off(nj), (size_t)Stage<double>::QSTEP};
}

// The route of a plain (pl) or general launch.  `shared`: the PLAIN kernels with the batch's shared tool / IK weights in dhp's bits 1-2 --
// only the eight-lanes kernel and the lean / publishing-lean float32 straight-line variants have those; false when none serves the launch.
inline bool route(const KArgs& a, int nj, int io_bits, bool ns, bool pl, int dhp, bool shared, CyclePlan& p) {
    const bool f32 = io_bits == 32;
    const Sizes s = sizes(io_bits, nj);
    // FASTF: the straight-line repeller path.  A funnel block (FUN) or decay orders that differ (MIXO) keep it only for the lean and
    // publishing-lean single-cycle launches of PLAIN chains; every other launch of such a batch takes the general path.
    bool fastf = a.fast_order >= 0, fun = false, mixo = false;
    if (fastf && a.has_funnel) {
        if (pl && lean_single(a, ns)) fun = true;
        else fastf = false;
    }
    if (fastf && a.mixed) {
        if (pl && lean_single(a, ns)) mixo = true;
        else fastf = fun = false;
    }
    p.plain = pl;
    p.fastf = fastf;
    p.fun = fun;
    p.fast_order = fastf ? a.fast_order : -1;
    p.slots_used = fastf ? a.slots_used_fast : a.slots_used;
    // the uniform repeller image (UNI): the lean single-cycle straight-line variants, when every decay repeller shares one safe distance and force
    const bool uni = fastf && !fun && !mixo && a.uni;
    const bool lean = pl && qdot_out_only(a, ns) && fastf;
    const size_t waves = p.block / 64;
    const size_t lds_full = p.lds;
    // LEAN launches touch only the head of the region: they ask for no more while the launch is at most one wave per SIMD; beyond, the
    // full size keeps it in rounds of one wave per SIMD (two waves per SIMD compete for the same HBM time; profiles/r02_batch_scaling.txt)
    const size_t lds_lean = (long)p.grid * (long)waves <= (long)a.n_simd ? waves * s.lean : lds_full;
    const size_t lds_fun = std::max(lds_lean, waves * (s.lean + 6 * s.qstep));   // + the aux block's six rows per wave
    // the DH pattern a cycle_kernel variant is built with: the lean straight-line variants but
    // the two-waves one on the compact image (it spilled with the pattern); float64 I/O: the pattern alone, for the 7-joint chain
    auto use = [&](CycleFamily f, bool roll, int lean_v, size_t lds) {
        p.family = f;
        p.roll = roll;
        p.lean = lean_v;
        p.lds = lds;
        const bool built = fastf && (roll ? lean_v == 1 : lean_v != 0) && !(p.waves == 2 && !p.uni);
        p.dhp = built ? (f32 ? dhp : (nj == 7 ? (dhp & 1) : 0)) : 0;
        return true;
    };
    // the nullspace module's two flag sets of the default process set, as compile-time constants (chains of up to 7 joints)
    const int cf = (!shared && ns && nj <= 7 && (a.flags == (unsigned)CF_NSMIX || a.flags == (unsigned)CF_NSJLMIX)) ? (int)a.flags : -1;
    if (pl && a.n_cycles > 0 && nj <= VFIK_ROLL_MAX_NJ)
        return lean ? use(CycleFamily::RolloutLean, true, 1, lds_lean) : use(CycleFamily::Rollout, true, 0, lds_full);
    // small batches: eight lanes per arm, where the same-box A/B wins (profiles/r03_latency_small_*.txt): launches that publish the rows at
    // every size up to sub8_max_batch_full; qdot_out alone, with or without the nullspace module, up to its own cap
    if (pl && nj <= (ns ? 7 : 8) && fastf && !fun && !mixo && sub8_served(a, ns) &&
        a.B <= (publishes_rows(a) ? a.sub8_max_batch_full : (ns ? a.sub8_max_batch_ns : a.sub8_max_batch))) {
        p.family = CycleFamily::Sub8;
        p.dhp = dhp;
        p.grid = (unsigned)((a.B + 7) / 8);
        p.block = 64;
        p.lds = 8 * 1024;
        return true;
    }
    if (shared && !f32) return false;
    if (mixo) {   // one wave per block; beyond one wave per SIMD the full region (rounds, as above); + one row for the order bytes
        p.mixo = true;
        p.grid = (unsigned)((a.B + 63) / 64);
        p.block = 64;
        size_t lds = (long)p.grid <= (long)a.n_simd ? s.lean : s.bytes;
        if (fun) lds = std::max(lds, s.lean + 6 * s.qstep);
        return use(CycleFamily::Mixo, false, qdot_out_only(a, ns) ? 1 : 3, lds + 1024);
    }
    if (lean && !a.q_out) {
        if (fun) return use(CycleFamily::Lean, false, 1, lds_fun);
        // beyond one wave per SIMD: the two-waves-per-SIMD build (float I/O, up to 7 joints; with the nullspace module on the uniform image only --
        // the compact-image variants of that build spilled)
        if (!shared && f32 && nj <= 7 && a.waves2 && (long)p.grid * (long)waves > (long)a.n_simd && (!ns || uni)) {
            p.waves = 2;
            p.uni = uni;
            p.cf = cf;
            return use(CycleFamily::LeanTwoWaves, false, 1, waves * s.lean);
        }
        p.uni = uni;
        p.cf = cf;
        return use(CycleFamily::Lean, false, 1, lds_lean);
    }
    if (!shared && nj > VFIK_ROLL_MAX_NJ && lean) return use(CycleFamily::SteppedCycle, false, 2, lds_lean);   // (q_out: a stepped rollout's cycle)
    if (pl && fastf && lean_single(a, ns)) {
        if (fun) return use(CycleFamily::PublishingLean, false, 3, lds_fun);
        p.uni = uni;
        p.cf = cf;
        return use(CycleFamily::PublishingLean, false, 3, lds_lean);
    }
    if (shared) return false;
    if (pl && qdot_out_only(a, ns) && !fastf && !a.q_out) return use(CycleFamily::GeneralLean, false, 1, lds_full);
    p.heavy = nj >= VFIK_HEAVY_MIN_NJ;
    return use(CycleFamily::Full, false, 0, lds_full);
}
}  // namespace plan_detail

// The plan of one launch of the cycle kernel: nj joints, io_bits 32 / 64, ns = the launch's flags carry VFIK_F_NULLSPACE, block = the
// handle's threads per block.  The decisions are taken in this order, the first that applies wins.
inline CyclePlan plan_cycle(const KArgs& a, int nj, int io_bits, bool ns, int block) {
    CyclePlan p{};
    p.family = CycleFamily::Refused;
    p.cf = -1;
    p.waves = 1;
    // A full region that does not fit the CU four times (float64 I/O from 10 joints on: 42-44 KB) would leave one SIMD of every CU idle: such
    // launches go as one wave per block, each block asking for the part of the region its options use -- the rows of a per-arm tool and of
    // per-arm mixer weights are the region's tail (profiles/r04_heavy_variants.txt).  (VFIK_BLOCK: a block's waves must fit the CU's 160 KB.)
    const plan_detail::Sizes s = plan_detail::sizes(io_bits, nj);
    if (4 * s.bytes > 160u * 1024u) {
        block = 64;
        p.lds = (a.tool_stride || a.mixw) ? s.bytes : s.tool;
    } else {
        while (block > 64 && (size_t)(block / 64) * s.bytes > 160u * 1024u) block -= 64;
        p.lds = (size_t)(block / 64) * s.bytes;
    }
    p.block = (unsigned)block;
    p.grid = (unsigned)((a.B + block - 1) / block);
    if (a.n_cycles > 0 && !rollout_in_kernel(nj, a.plain)) return p;
    const int dhp = (a.plain && a.dhp == 1 && has_dh_pattern(nj)) ? 1 : 0;   // (the chain matches the pattern built for its joint count)
    if (a.plain >= 2 && dhp == (has_dh_pattern(nj) ? 1 : 0)) {
        // The batch's shared tool (a.plain - 1 bit 0) and / or IK weights other than one (bit 1, chains of up to 7 joints) on the PLAIN kernels;
        // a launch none of their variants serves, or a chain off its pattern, takes the general variants
        const int opt = a.plain - 1, bits = opt == 1 ? 2 : (nj <= 7 && opt == 2) ? 4 : (nj <= 7 && opt == 3) ? 6 : 0;
        CyclePlan q = p;
        if (bits && plan_detail::route(a, nj, io_bits, ns, true, dhp | bits, true, q)) return q;
    }
    plan_detail::route(a, nj, io_bits, ns, a.plain == 1, a.plain == 1 ? dhp : 0, false, p);
    return p;
}

// The demangled name of the instantiation a plan takes, namespace and parameter list stripped (template arguments in the order the kernels
// declare them; " [heavy]": the long chains' object of their own).  Host code: tests/c_host/launch_plan.cpp prints it, vfik_launched_kernels
// reports it -- neither is on the enqueue path.
inline std::string cycle_kernel_name(const CyclePlan& p, int nj, int io_bits, bool ns) {
    const char* t = io_bits == 32 ? "float" : "double";
    auto b = [](bool v) { return v ? "true" : "false"; };
    char s[256];
    switch (p.family) {
        case CycleFamily::Refused: return "refused";
        case CycleFamily::Sub8:
            std::snprintf(s, sizeof s, "cycle_sub8_kernel%s<%s, %d, %s, %d>", ns ? "" : "_x", t, nj, b(ns), p.dhp);
            return s;
        case CycleFamily::Mixo:
            std::snprintf(s, sizeof s, "cycle_kernel_m<%s, %d, %s, %d, %s, %d>", t, nj, b(ns), p.lean, b(p.fun), p.dhp);
            return s;
        case CycleFamily::Lean:
        case CycleFamily::LeanTwoWaves:
            std::snprintf(s, sizeof s, "cycle_kernel_s<%s, %d, %s, true, false, true, 1, %d, false, %s, %d, %s, %d>", t, nj, b(ns), p.cf, b(p.fun), p.waves,
                          b(p.uni), p.dhp);
            return s;
        default:
            std::snprintf(s, sizeof s, "cycle_kernel_x<%s, %d, %s, %s, %s, %s, %d, %d, false, %s, %d, %s, false, %d>%s", t, nj, b(ns), b(p.plain), b(p.roll), b(p.fastf),
                          p.lean, p.cf, b(p.fun), p.waves, b(p.uni), p.dhp, p.heavy ? " [heavy]" : "");
            return s;
    }
}

// Type-erased launchers (implemented in vfik_aux.hip).  kargs points to a KArgs<nj>.
// *plan (may be NULL) receives the launch's plan -- which instantiation it took (cycle_kernel_name), the eight-lanes-per-arm kernel among them
hipError_t launch_cycle(int io_dtype, int nj, const KArgs& kargs, int block, hipStream_t stream, CyclePlan* plan = nullptr);
hipError_t launch_probe(int io_dtype, const void* pose, const void* goal, const void* slots, int B, long Bp, int slots_used,
                        double rot_slow, double cos_slow, void* out, hipStream_t stream);
// vfik_move_fields (ABI 6): new coordinates for the goal frames and the decay repellers of arms [first_arm, first_arm + n_arms), written into
// every image vfik_set_fields packed.  repmap: per arm one 16-bit entry per compact-image slot, 16 bytes (8 slots) per arm and plane like the
// order planes -- entry k = the GENERAL slot of the arm's k-th decay repeller (it differs from k behind a funnel, hemisphere or further
// attractor), MOVE_NONE from the arm's repeller count on.
constexpr unsigned short MOVE_NONE = 0xFFFFu;
struct MoveArgs {
    void* goal;                 // 4 quad planes
    void* slots;                // 2 S quad planes
    void* slots_fast;           // compact image
    void* slots_uni;            // uniform image (slot m in plane m + 1)
    const unsigned short* repmap;
    const void* goal16;         // [n_arms][16] or NULL
    const void* rep4;           // [n_arms][n_rep][4] or NULL
    const int* active;          // [n_arms] or NULL
    int first_arm, n_arms, n_rep, S;
    long Bpad;
};
hipError_t launch_move(int io_dtype, const MoveArgs& m, hipStream_t stream);
// vfik_move_scene: the same, and new coordinates for funnels, hemispheres and the attractors behind the goal block.  scenemap: THREE maps
// of repmap's layout one after the other -- class c (SCENE_FUN, SCENE_HEM, SCENE_ATT) owns planes [c * map_planes, (c + 1) * map_planes),
// map_planes = (max(1, S) + 7) / 8 of 16 bytes (8 entries) per arm -- so entry k of class c of arm b is
//   scenemap[((c * map_planes + (k >> 3)) * Bpad + b) * 8 + (k & 7)]
// = the GENERAL slot of the arm's k-th funnel / hemisphere / attractor after the goal block in ascending-id order (the first of a funnel's or a
// hemisphere's two slots, of an attractor's three), MOVE_NONE from the arm's count of that class on.  aux: the 6 quad planes behind the goal
// block (funnel 0..2, hemisphere 3..5), which hold the arm's FIRST funnel and FIRST hemisphere: row k = 0 goes there too.
enum { SCENE_FUN = 0, SCENE_HEM = 1, SCENE_ATT = 2 };
struct SceneMoveArgs {
    MoveArgs m;
    void* aux;                  // 6 quad planes
    const unsigned short* scenemap;
    const void* fun6;           // [n_arms][n_fun][6] or NULL
    const void* hem6;           // [n_arms][n_hem][6] or NULL
    const void* att16;          // [n_arms][n_att][16] or NULL
    int n_fun, n_hem, n_att, map_planes;
};
hipError_t launch_move_scene(int io_dtype, const SceneMoveArgs& s, hipStream_t stream);
// The check that runs after block k of a timed move (check_kernel<T, JOINT, LIST>, vfik_aux.hip), for all four forms: vfik_goto (Cartesian
// rule, one goal), vfik_follow (Cartesian rule, a LIST of goal frames), vfik_goto_js (joint rule, io->q_ref) and vfik_follow_js (joint rule, a LIST
// of postures).  A list form's check that finds an arm at item next[b] notes the cycle in reached[b][next], advances next[b] and sends the arm
// to the following item: its frame into the arm's goal block (move_goal_row's stores), or its posture into the arm's row of `ref`.
// k < 0: the pass in front of block 0 and nothing else -- one goal: arrived[b] = -1, gate[b] = the caller's gate; a list: reached = -1, next = 0,
// len[b] = the arm's list length (leading rows of way[b] whose first element is not NaN), gate[b] = the caller's gate && len > 0, and item 0 into
// the goal blocks of those arms, or into `ref` (there NaN for an arm kept out).
// What every launch reads comes first (the dispatch object is compiled with kernel-argument preload); a member of the other rule or target is
// not read.
struct CheckArgs {
    int* gate;                  // [B] the handle's gate: what block k ran under on entry, what block k + 1 runs under on exit
    const int* active;          // [B] the caller's gate, or NULL = every arm
    int* pending;               // &pending[k]: zeroed on the stream in front of the call
    int B, n, W, k, stride, hold;   // W: items per list
    long Bpad;
    const void* q_prev;         // [B][n] the q row block k read
    void* q_now;                // [B][n] the q row block k wrote
    // What one form reads lies together, so that the Cartesian one-goal check finds its arguments in the first 120 bytes, as before the four
    // checks had one struct, and the joint one's in one run up to `diff`: one goal, the Cartesian rule, the precisions, the joint rule's rows, then a
    // list's members and its via precisions.
    int* arrived;               // one goal: [B] cycle index of the arm's first successful check, -1 = not yet
    // the Cartesian rule
    void* dist;                 // [B][2] goal_dist of block k (metres, degrees)
    const void* dist_prev;      // [B][2] the trace's row k - 1, or NULL (no trace, or k = 0): what an arm that did not run repeats
    void* goal;                 // the goal block's 4 quad planes: plane 3, component 0 is its `present` flag; a list writes planes 0..2
    // joint: goal_precision per joint, entries at or beyond n are not read; Cartesian: [0] metres, [1] radians
    double prec[VFIK_MAX_JOINTS];       // one goal, and at an arm's last item
    // the joint rule
    void* ref;                  // [B][n] one goal: io->q_ref as the caller sent it (read only), a row that starts with NaN never arrives;
                                //        a list: the handle's reference row, the posture the arm is under way to, min(next, len - 1)
    void* diff;                 // [B][n] ref - q of every arm that ran block k, or NULL
    // a list
    int* reached;               // [B][W] cycle index of the check that found the arm at item w, -1 = not yet
    int* next;                  // [B] items reached so far = the index of the one under way
    int* len;                   // [B] list lengths, a buffer of the handle: written by the k < 0 pass, read by every check
    const void* way;            // Cartesian: way16 [B][W][16], the goal frames in order, 16-byte aligned; joint: wayq [B][W][n], the postures
    int* way_now;               // [B] row k of way_traj -- the item this check was made against -- or NULL
    const int* way_prev;        // [B] row k - 1 of way_traj, or NULL (no trace, or k = 0)
    double via_prec[VFIK_MAX_JOINTS];   // a list: at every item before an arm's last
};
// The stall rule of a handle (vfik_set_stall_rule), evaluated inside the check by the STALL builds (check_stall_kernel, script_stall_kernel) for
// every arm that ran its block, is under way and did not arrive at this check.  The measure, in double on the io-typed values: the Cartesian
// rule's (d, a) as the arrival rule forms them (NaN for an arm without a goal block), or the joint rule's e = max |ref - q| over the joints whose
// precision in force is finite (best[b][0] alone).  Progress: d < best_d - eps_pos || a < best_a - eps_rot, or e < best_e - eps_js, all strict;
// then best = the componentwise minimum and count = 0, else ++count, and count == patience writes stalled[b] = (k + 1) * stride - 1.  A stalled
// arm meets no rule again, is not counted in pending[k] and, with `stop`, has gate 0.  k < 0: best = +inf, count = 0, stalled = -1; the check
// that advances an arm resets its best and count.  A second kernel argument, so that CheckArgs and ScriptArgs -- and with them the device
// code of the builds without the rule -- keep their layout.  The arm's own lane reads and writes its state; no LDS, no scratch, no atomic.
struct StallArgs {
    double* best;               // [B][2]
    int* count;                 // [B]
    int* stalled;               // [B] cycle index of the check that declared the arm stalled, -1 = not stalled
    int patience, stop;
    double eps_pos, eps_rot, eps_js;
};
// st == NULL: the builds without the rule
hipError_t launch_check(int io_dtype, bool joint, bool list, const CheckArgs& g, hipStream_t stream, const StallArgs* st = nullptr);
// The check of a motion script (vfik_script; script_kernel<T>, vfik_aux.hip): vfik_follow's state machine over a list whose items are goal
// frames or postures, kind[b][w] telling which.  `c` is read as a Cartesian list's check reads it -- way = way16, prec / via_prec = the distance
// pair, ref = the handle's reference row, diff -- and the rest is the script's own: what the joint rule and the switch of controller need.
// An arm found at step next[b] is sent to the following one: a frame into its goal block, a posture into its row of `ref`, and the mixer quad of
// that step's kind into plane 0 of its row of `mixw`, which the script's blocks read as KArgs::mixw.  k < 0: the pass in front of block 0 also
// fills plane 1 (w4 w5 max_vel) from the arm's row of `bridge`, or from `bridge_u` where the handle has no per-arm bridge state.
struct ScriptArgs {
    CheckArgs c;
    const int* kind;            // [B][W] VFIK_STEP_FRAME, VFIK_STEP_POSTURE; anything else ends the arm's script
    const void* wayq;           // [B][W][n] read at posture steps alone
    void* mixw;                 // the script's 2 quad planes [2][Bpad]: w0..w3 | w4 w5 max_vel -
    const void* bridge;         // the handle's per-arm planes (vfik_set_mixer_weights, vfik_set_max_vel), or NULL
    double bridge_u[4];         // w4, w5, max_vel, 0 of every arm without them
    double mix[2][4];           // w0..w3 under way to a frame [0], to a posture [1]
    double js_prec[VFIK_MAX_JOINTS], js_via_prec[VFIK_MAX_JOINTS];   // the joint rule's band: at an arm's last step, at those before it
};
hipError_t launch_script(int io_dtype, const ScriptArgs& s, hipStream_t stream, const StallArgs* st = nullptr);
// vfik_link_points (link_kernel<T>, vfik_aux.hip): the centres of the handle's link spheres for every arm, from the joint angles of the arm's
// SOURCE arm, in the shape vfik_move_fields takes as rep4.  One lane per arm b: s = src_arm ? src_arm[b] : b; a source outside [0, B) or a NaN in
// q[s] gives L rows of NaN and q is not read for an out-of-range source.  The chain of `img` (vfik_links.h: LinkImage, device memory, read at
// uniform addresses) is walked once in float64; sphere j of the caller's list goes into row first_rep + j of rep4[b][n_rep][4] as
// (R_b P + t_b, radius) -- xform12[b] = [R_b | t_b] row-major 3x4, or NULL -- and, when `traj` is given, into row j of traj[b][L][4] too (the
// trace of a coupled timed move).  Rows outside first_rep .. first_rep + L - 1 are not written.  rep4 and traj are 16-byte aligned.
struct LinkArgs {
    const LinkImage* img;
    const void* q;              // [B][n]
    const int* src_arm;         // [B] or NULL
    const void* xform12;        // [B][12] or NULL
    void* rep4;                 // [B][n_rep][4]
    void* traj;                 // [B][L][4] or NULL
    int B, n_rep, first_rep;
};
hipError_t launch_link(int io_dtype, const LinkArgs& a, hipStream_t stream);
// vfik_link_clearance and the wait rule of the timed moves (clear_kernel<T>, vfik_aux.hip): how much room is left between an arm's own link
// spheres and `count` rows of pts4[b][n_rep][4] (x y z radius, from row `first`).  One lane per arm b walks the chain of `img` once from q[b],
// as link_kernel does, and when the walk stands at a link compares every sphere of that link with the arm's rows:
//     d = sqrt(|P - Q|^2) - r_own - R_row    in float64;    clear[b] = (T) min d;    pair[b] = own * 32 + row (own: the CALLER's index)
// over the pairs whose bit `row` of mask[own's sorted position] is set and whose row holds no NaN; ties take the smallest code.  No pair:
// +inf and -1; a NaN in q[b]: NaN and -1.  clear and pair may be NULL.
// The wait rule (gate != NULL; vfik_set_wait_rule): an arm with gate[b] == 1 and yields[b] != 0 (yields NULL: every arm) whose (double)(T)
// clearance is < min_clearance gets gate[b] = 0 and counts in waited[b] -- stored when `first_block`, else added.
struct ClearArgs {
    const LinkImage* img;
    const void* q;              // [B][n]
    const void* pts4;           // [B][n_rep][4], 16-byte aligned
    void* clear;                // [B] io dtype or NULL
    int* pair;                  // [B] or NULL
    int B, n_rep, first, count;
    uint32_t mask[VFIK_MAX_LINK_SPHERES];   // the image's sorted order (vfik_links.h: clear_mask)
    int* gate;                  // [B] or NULL: no rule
    const int* yields;          // [B] or NULL
    int* waited;                // [B] or NULL
    double min_clearance;
    int first_block;
};
hipError_t launch_clear(int io_dtype, const ClearArgs& a, hipStream_t stream);
// vfik_link_avoid and the avoid rule of the timed moves (avoid_kernel<T>, vfik_aux.hip): every own link sphere is pushed away from the rows
// it is close to, and the push goes through the Jacobian transpose of the sphere's point into a joint command.  The walk, the rows, the mask
// and the NaN-row rule are ClearArgs'; with s = sqrt(|P - Q|^2) in float64:
//     a = 1 - (s - r_own - R_row) / d0,  active iff a > 0 and s > 0;    F_own = gain * scale[b] * sum a (P - Q) / s
//     tau_k = sum over own spheres on links > k of  z_k . ((P - o_k) x F)  (revolute)  or  z_k . F  (prismatic);    row[b][k] = (T) tau_k
// A NaN in q[b] or no active pair: a row of zeros.  The row of every arm b < B goes to each of out, chan_out and traj that is given.
struct AvoidArgs {
    const LinkImage* img;
    const void* q;              // [B][n]
    const void* pts4;           // [B][n_rep][4], 16-byte aligned
    const void* scale;          // [B] io dtype or NULL (all ones)
    void* out;                  // [B][n] io dtype or NULL
    void* chan_out;             // [B][n]: the handle's rows of one ext channel, or NULL
    void* traj;                 // [B][n]: a trace row, or NULL
    int B, n_rep, first, count;
    uint32_t mask[VFIK_MAX_LINK_SPHERES];   // the image's sorted order (vfik_links.h: clear_mask)
    double gain, d0;
    int stage;                  // set by launch_avoid: the rows are staged in LDS behind the joints' doubles
};
hipError_t launch_avoid(int io_dtype, int n, AvoidArgs a, hipStream_t stream);
hipError_t launch_monitor(int io_dtype, const void* pose, const void* frames, int O, long count, void* out, hipStream_t stream, const int* active = nullptr);
hipError_t launch_track(int io_dtype, const void* pose, const void* v6, double* state, void* out, const int* active, int B, hipStream_t stream);
hipError_t launch_mix(int io_dtype, const void* cmds, const double* w_dev, int K, long count, long chan_stride,
                      void* out, hipStream_t stream);

}  // namespace vfik
