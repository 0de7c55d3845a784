// vfik_abi.cpp -- host side of the C-ABI declared in include/vfik.h: handle, device state, field
// packing, launches.  Compiled by hipcc into libvfik_hip.so together with vfik_kernel.hip (the cycle kernels) and
// vfik_aux.hip (the auxiliary kernels, the launchers); the chain's constants come from vfik_kconst.h.
// There is no CPU execution path in this file: every compute entry point launches a HIP kernel.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <limits>
#include <vector>

#include "../../include/vfik.h"
#include "vfik_io_layout.h"
#include "vfik_kernel.h"
#include "vfik_scene.h"

namespace {

thread_local std::string g_err;

int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess) return fail(VFIK_E_HIP, "%s: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

}  // namespace

struct vfik_handle {
    int device = 0, io_dtype = 32, n = 0, max_slots = 0, B = 0, Bpad = 0, block = 64;
    // eight-lanes-per-arm kernel for lean launches of batches up to this size (vfik_set_small_batch_kernel,
    // VFIK_SUB8_MAX_BATCH).  Measured crossover (tools/ab_mapping.py, float64 I/O, goal + 4 repellers): 3-7 % faster than
    // one lane per arm up to 4 096 arms, equal at 8 192, 1.4x / 2.0x / 2.8x SLOWER at 16 384 / 32 768 / 65 536.
    // Round 4 re-decided the first two (profiles/r04_latency_small_*.txt): the lane-per-arm lean kernels lost a sixth of their instructions and
    // enter through 56 bytes of scalar arguments, the eight-lanes kernel through the 360-byte block -- back to back it is the host's enqueue that
    // sets its pace (3.5 against 4.9-6.1 us per lean launch at every size), and with one synchronisation per cycle the two are within 3 %.
    int sub8_max_batch = 0;          // q -> qdot_out without the module: one lane per arm at every size (4096 until round 3)
    int sub8_max_batch_ns = 0;       // with the nullspace module and qdot_out only: likewise (32 until round 3)
    int sub8_max_batch_full = 4096;  // launches that publish the per-cycle rows: -4 ... -10 % at every size either way (vfik_set_small_batch_kernel sets all three)
    long sub8_launches = 0;  // how many launches took it (introspection for tests / A/B)
    // the distinct cycle-kernel instantiations launched since the last vfik_launched_kernels (plans only: names are formatted when asked)
    static constexpr int LAUNCHED_MAX = 16;
    struct Launched { vfik::CyclePlan p; bool ns; } launched[LAUNCHED_MAX];
    int launched_n = 0;
    bool launched_lost = false;   // more distinct kernels than the record holds
    long epoch = 0;          // moves with every call that can change what a launch bakes in (vfik_launch_epoch)
    int n_simd = 1024;       // 4 per CU of this device
    // Batches beyond one wave per SIMD take the lean kernels compiled for two waves per SIMD (cycle_kernel WAVES = 2; float I/O, chains of up to 7
    // joints): 131 072 arms 10.4 -> 9.1 us, 524 288 38.4 -> 33.4 (profiles/r03_batch_scaling.txt).  VFIK_TWO_WAVES=0 keeps the rounds of one wave per SIMD.
    int waves2 = 1;
    size_t esz = 4;
    hipStream_t stream = nullptr;
    bool own_stream = true;
    vfik_chain chain{};
    bool chain_set = false;
    vfik_params params{};
    // device state
    void* d_arena = nullptr;   // [goal | kconst | lastvec | slots_fast | slots]: d_goal, d_kconst, d_lastvec, d_slots_fast, d_slots point into it
    void* d_goal = nullptr;    // 4 quad planes
    void* d_funnel = nullptr;  // aux block, 6 quad planes: the arm's funnel attractor (3) and hemisphere repeller (3) on the straight-line path (vfik_kernel.h)
    void* d_slots = nullptr;   // 2*S quad planes
    void* d_slots_uni = nullptr;   // uniform repeller image: ONE quad plane per slot (x y z radius); read when every decay repeller of the batch shares safe distance and force
    // the field sets as vfik_set_fields left them (vfik_scene.h): every arm's summary, and what the batch's launches take for it
    std::vector<vfik::ArmScene> arms;
    vfik::ScenePlan scene;
    vfik::SceneKnobs knobs;
    double uni_safe = 0.0, uni_force = 0.0;   // the uniform repeller pair as the device constants hold it (KConst::rep_safe, dh[0].pad)
    void* d_slots_fast = nullptr;  // compact repeller image for the straight-line path: 3 quad planes per PAIR of slots
    void* d_orders = nullptr;      // order planes: 16 bytes per arm and plane, one byte per compact-image slot (vfik_kernel.h); read when the scene is `mixed`
    unsigned short* d_repmap = nullptr;   // vfik_move_fields: general slot of the arm's k-th decay repeller, 8 entries (16 bytes) per arm and plane (vfik_kernel.h: MoveArgs)
    unsigned short* d_scenemap = nullptr; // vfik_move_scene: the same for its k-th funnel, hemisphere and attractor behind the goal block, three maps in a row (vfik_kernel.h: SceneMoveArgs)
    bool fields_set = false;       // some vfik_set_fields call succeeded: there are images to move
    struct DevBuf { void* p = nullptr; size_t bytes = 0; };   // a device buffer grown on demand (reserve)
    DevBuf move_stage;             // vfik_move_fields_host / vfik_move_scene_host: the rounded rows on the device
    void* d_tool = nullptr;    // 3 quad planes (per-arm tools only)
    double tool_shared[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    int tool_per_arm = 0;
    void* d_ext = nullptr;     // [4][B][n], allocated on first use
    float* d_lastvec = nullptr;  // nullspace sign memory, [(n + 4) / 4][Bpad][4] floats (vfik_kernel.h)
    double* d_mixw = nullptr;  // [16]
    unsigned long long* d_stamps = nullptr;  // diagnostic build only
    void* d_rollq[2] = {nullptr, nullptr};  // q ping-pong of the stepped rollout (long chains)
    // vfik_goto, each allocated at the first call that needs it: the gate its blocks run under, pending[] when the caller keeps none, a
    // goal_dist row when the caller names none, the blocks' q pair without q_traj (not d_rollq: a stepped block's own intermediate cycles
    // ping-pong there, and its first would write the row it reads), the device side of vfik_goto_host
    int* d_goto_gate = nullptr;
    DevBuf goto_pending;
    void* d_goto_dist = nullptr;
    void* d_gotoq[2] = {nullptr, nullptr};
    DevBuf goto_stage;
    int* d_follow_len = nullptr;   // vfik_follow (which runs on vfik_goto's buffers): every arm's path length
    void* d_js_ref = nullptr;      // vfik_follow_js, vfik_script: the reference row [B][n] their blocks read as io->q_ref (nobody else reads it)
    void* d_script_mixw = nullptr; // vfik_script: the 2 quad planes its blocks read as the per-arm mixer weights (d_mixw_arm's layout; nobody else reads them)
    // vfik_set_stall_rule: the rule the checks of every timed move evaluate (stall_on), its per-arm state best[B][2] and count[B], and
    // stalled[B] where the caller names no array of its own
    bool stall_on = false;
    vfik_stall_rule stall{};
    double* d_stall_best = nullptr;
    int* d_stall_count = nullptr;
    int* d_stall_own = nullptr;
    // vfik_set_link_spheres: the caller's list (n_links of them) and its device image (vfik_links.h), which link_kernel reads; the staging of
    // vfik_link_points_host.  vfik_set_coupling: the coupling every block of a timed move applies (couple_on) and the handle's rep4 buffer
    // [B][first_rep + n_links][4], NaN outside the rows link_kernel writes
    int n_links = 0;
    vfik_link_sphere links[VFIK_MAX_LINK_SPHERES] = {};
    void* d_link_img = nullptr;
    DevBuf link_stage;
    bool couple_on = false;
    vfik_coupling couple{};
    DevBuf couple_rep;
    // vfik_link_clearance: the image as the host keeps it (the mask is permuted by its perm[]); vfik_set_wait_rule: the rule every block of a
    // timed move under a coupling applies (wait_on), its mask in the image's order, and waited[B] where the caller names no array of its own
    vfik::LinkImage link_img{};
    bool wait_on = false;
    vfik_wait_rule wait{};
    uint32_t wait_mask[VFIK_MAX_LINK_SPHERES] = {};
    int* d_wait_own = nullptr;
    // vfik_set_avoid_rule: the push every block of a timed move under a coupling writes into one ext channel (avoid_on), its mask in the image's order
    bool avoid_on = false;
    vfik_avoid_rule avoid{};
    uint32_t avoid_mask[VFIK_MAX_LINK_SPHERES] = {};
    double* d_wts = nullptr;    // per-arm IK weights [6 + n][Bpad], allocated by vfik_set_arm_weights
    // equal rows of a whole-batch vfik_set_arm_weights: the batch's IK weights from then on, kept apart from the caller's vfik_params (whose
    // wy / wq a later vfik_set_params compares against) until a vfik_set_params changes wy or wq
    bool wts_promoted = false;
    double shared_wy[6] = {1, 1, 1, 1, 1, 1};
    double shared_wq[VFIK_MAX_JOINTS] = {1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1};
    void* d_qalign = nullptr;   // 16-byte-aligned copy of a vfik_step q that is not (launch_cycles), allocated at the first such call
    // every arm's bridge state (mixer weights, limiter speed) equal: the launch reads them from the batch constants like a handle that
    // never had per-arm bridge state (a.mixw stays NULL, so the lean / publishing-lean variants keep serving it) -- what a port-level caller
    // produces when every arm's handler sends the same /bridge/weight (handlers.py:189-204,481-497)
    bool bridge_uniform = false;
    double bridge_u[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // ... the common row, as the per-arm image holds it (rounded to the I/O type)
    double* d_track = nullptr;  // tracking-error history [38][B], allocated on first use
    void* d_mixw_arm = nullptr;  // per-arm mixer weights (2 quad planes), allocated on first use
    void* d_kconst = nullptr;  // vfik::KConst<n>: chain + parameters, read through the scalar cache
    // observers fused into the cycle call (ABI 4): object frames of the distance monitor [B][n_objects][16] in the io
    // dtype, and the cycle's pose / field twist when the caller did not ask for them itself
    void* d_objects = nullptr;
    int n_objects = 0;
    vfik::IoDims io_dims() const { return {(size_t)n, esz, (size_t)n_objects}; }   // what the sizes of vfik_io's members depend on (vfik_io_layout.h)
    void* d_obs_pose = nullptr;
    void* d_obs_v6 = nullptr;
    size_t dev_bytes = 0;
    // host bookkeeping
    std::vector<double> bridge_host;  // [B][8] mirror of d_mixw_arm: mixer weights 0..5, max_vel 6
    int plain = 0;  // the chain allows the PLAIN kernel variants: 1 + (shared tool ? 1 : 0) + (shared IK weights other than one ? 2 : 0); 0: the general variants
    int dhp = 0;    // ... and the chain matches a DH pattern the lean kernels are built for (vfik_kconst.h: DhPattern)
    int dhp_allowed = 1;   // VFIK_DH_PATTERN=0: always the general DH form (tests, A/B)
    bool speed_set = false;
    // vfik_step_host / vfik_rollout_host: one device arena + one pinned host arena for every member of the call
    void* arena_dev = nullptr;
    void* arena_host = nullptr;
    void* arena_host_dev = nullptr;   // the device's address of the pinned host arena (zero-copy calls)
    size_t arena_bytes = 0;
    size_t zero_copy_max = (size_t)64 << 10;   // calls of at most this many bytes: the kernel reads / writes the pinned arena itself (VFIK_ZERO_COPY_MAX)
    DevBuf sc[vfik::N_STAGED];  // ... and per-member device buffers for calls of few large members (not part of vfik_device_bytes, like the arenas)
    // pipelined host path (vfik_submit_host / vfik_wait): up to PIPE submissions in flight, each slot with
    // its own device staging buffers and events; s_in / s_out are the side streams
    static constexpr int PIPE = 3;
    struct PipeSlot {
        DevBuf sc[vfik::N_STAGED];
        hipEvent_t ev_in = nullptr, ev_k = nullptr, ev_out = nullptr;
        long ticket = -1;  // submission living in this slot, -1 = free
    };
    PipeSlot pipe[PIPE];
    hipStream_t s_in = nullptr, s_out = nullptr;
    long next_ticket = 0;
};

namespace {

// counted: the allocation is part of vfik_device_bytes
int dev_alloc(vfik_handle* h, void** p, size_t bytes, bool zero, bool counted = true) {
    HIP_TRY(hipMalloc(p, bytes));
    if (counted) h->dev_bytes += bytes;
    if (zero) HIP_TRY(hipMemsetAsync(*p, 0, bytes, h->stream));
    return VFIK_OK;
}

// Grow-on-demand device buffer: at least `bytes`, the old content lost.  counted: the buffer is part of vfik_device_bytes; sync: work on the
// handle's stream may still use the old buffer.
int reserve(vfik_handle* h, vfik_handle::DevBuf& b, size_t bytes, bool counted, bool sync) {
    if (bytes <= b.bytes) return VFIK_OK;
    if (sync) HIP_TRY(hipStreamSynchronize(h->stream));
    if (b.p) { (void)hipFree(b.p); if (counted) h->dev_bytes -= b.bytes; }
    b = {};
    if (dev_alloc(h, &b.p, bytes, false, counted)) return VFIK_E_HIP;
    b.bytes = bytes;
    return VFIK_OK;
}

// Buffers of the handle are allocated at the first call that needs them, never while `stream` is being captured (the allocation would be part
// of the captured work or fail it): the caller's message tells which call to make outside the capture first.
int refuse_capture(hipStream_t stream, const char* msg) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(stream, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone) return fail(VFIK_E_STATE, "%s", msg);
    (void)hipGetLastError();
    return VFIK_OK;
}

int check_arms(const vfik_handle* h, int first_arm, int n_arms) {
    if (first_arm < 0 || n_arms < 1 || first_arm + n_arms > h->B) return fail(VFIK_E_ARG, "arm range [%d, %d) outside batch %d", first_arm, first_arm + n_arms, h->B);
    return VFIK_OK;
}

// A setter rewrites device state that kernels of the pipelined host path may still be reading on the
// side streams: let those drain first (the handle's own stream is synchronised by the setters themselves).
// (every vfik_set_* / vfik_reset_state call passes through here: the launch epoch moves with them, vfik_launch_epoch)
// (vfik_move_fields drains them too, without moving the epoch: it changes nothing a launch bakes in)
int drain_side_streams(vfik_handle* h) {
    if (h->s_in) HIP_TRY(hipStreamSynchronize(h->s_in));
    if (h->s_out) HIP_TRY(hipStreamSynchronize(h->s_out));
    return VFIK_OK;
}

int quiesce(vfik_handle* h) {
    ++h->epoch;
    return drain_side_streams(h);
}

// true when the GPU can dereference p: device memory, or pinned / registered host memory
bool gpu_visible(const void* p) {
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) != hipSuccess) {
        (void)hipGetLastError();  // pageable memory: not an error of ours
        return false;
    }
    return at.type == hipMemoryTypeHost || at.type == hipMemoryTypeDevice || at.type == hipMemoryTypeManaged;
}

// ... rounded to the handle's I/O type
void put_io(const vfik_handle* h, std::vector<char>& buf, size_t idx, double v) {
    if (h->io_dtype == 32) vfik::put<float>(buf, idx, v); else vfik::put<double>(buf, idx, v);
}

void fill_kargs(const vfik_handle* h, const vfik_io* io, vfik::KArgs& a) {
    std::memset(&a, 0, sizeof a);
    a.B = h->B;
    a.Bpad = h->Bpad;
    a.slots_used = h->scene.slots_used;
    a.fast_order = h->scene.fast_order;
    a.flags = h->params.flags;
    a.tool_stride = h->tool_per_arm ? h->Bpad : 0;
    a.plain = (h->plain && !h->tool_per_arm && !h->d_wts) ? h->plain : 0;   // (1 ... 4: the PLAIN kernels, with the batch's shared tool / shared IK weights as vfik_kernel.h says)
    a.wts = h->d_wts;
    a.q = io->q;
    a.goal = h->d_goal;
    a.slots = h->d_slots;
    a.slots_fast = h->d_slots_fast;
    a.tool = h->d_tool;
    a.null_control = io->null_control;
    a.ext = h->d_ext;
    a.mixw = h->bridge_uniform ? nullptr : h->d_mixw_arm;
    a.q_ref = io->q_ref;
    a.q_cmded = io->q_cmded;
    a.lastvec = h->d_lastvec;
    a.qdot_vf = io->qdot_vf;
    a.qdot_null = io->qdot_null;
    a.qdot_out = io->qdot_out;
    a.pose = io->pose;
    a.pose_nt = io->pose_nt;
    a.v6 = io->v6;
    a.qdist = io->qdist;
    a.status = io->status;
    a.goal_dist = io->goal_dist;
    a.active = io->active;
    a.q_lo = io->q_lo;
    a.q_hi = io->q_hi;
    a.q_ref_out = io->q_ref ? io->q_ref_out : nullptr;
    a.sub8_max_batch = h->sub8_max_batch;
    a.sub8_max_batch_full = h->sub8_max_batch_full;
    a.sub8_max_batch_ns = h->sub8_max_batch_ns;
    a.n_simd = h->n_simd;
    a.arena = h->d_arena;
    a.funnel = h->d_funnel;
    a.slots_used_fast = h->scene.slots_used_fast;
    a.has_funnel = h->scene.any_funnel;
    a.waves2 = h->waves2;
    a.one5 = h->scene.one_chunk();
    a.uni = h->scene.uniform(h->knobs);
    a.uni_planes = vfik::image_shape(vfik::IMG_COMPACT, h->max_slots, h->io_dtype).planes;
    a.stamps = h->d_stamps;
    a.kc = h->d_kconst;
    a.orders = h->d_orders;
    a.mixed = h->scene.mixed_orders();
    a.dhp = a.plain ? h->dhp : 0;
}

// rewrite the device copy of the batch constants (chain + parameters); rare, synchronous
int upload_kconst(vfik_handle* h) {
    if (!h->chain_set) return VFIK_OK;
    std::vector<char> img(vfik::kconst_bytes(h->n));
    int plain = 0, dhp = 0;
    vfik_params kp = h->params;
    if (h->bridge_uniform) {   // (the arms' common bridge state stands in for the batch-wide values)
        for (int k = 0; k < VFIK_MIX_CHANNELS; ++k) kp.mix_w[k] = h->bridge_u[k];
        kp.max_vel = h->bridge_u[6];
    }
    if (h->wts_promoted) {   // (the arms' common IK weights stand in for the caller's)
        for (int k = 0; k < 6; ++k) kp.wy[k] = h->shared_wy[k];
        for (int k = 0; k < h->n; ++k) kp.wq[k] = h->shared_wq[k];
    }
    const double err = vfik::kconst_fill(h->n, img.data(), h->chain, kp, h->tool_shared, &plain, &dhp);
    if (!(err < 1e-9)) return fail(VFIK_E_ARG, "chain: a fixed transform is not a rigid motion (DH recomposition error %.3e)", err);
    std::memcpy(img.data() + VFIK_KCONST_REP_SAFE_OFF(h->n), &h->uni_safe, sizeof(double));   // the batch's uniform repeller pair (vfik_set_fields)
    std::memcpy(img.data() + VFIK_KCONST_REP_FORCE_OFF, &h->uni_force, sizeof(double));
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipMemcpyAsync(h->d_kconst, img.data(), img.size(), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->plain = plain;
    h->dhp = h->dhp_allowed ? dhp : 0;
    return VFIK_OK;
}

int check_handle(const vfik_handle* h) {
    if (!h) return fail(VFIK_E_ARG, "null handle");
    return VFIK_OK;
}

}  // namespace

extern "C" {

int vfik_abi_version(void) { return VFIK_ABI_VERSION; }

void vfik_struct_sizes(size_t out[4]) {
    out[0] = sizeof(vfik_field); out[1] = sizeof(vfik_chain); out[2] = sizeof(vfik_params); out[3] = sizeof(vfik_io);
}

const char* vfik_last_error(void) { return g_err.c_str(); }

int vfik_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

uint32_t vfik_supported_joints(void) { return vfik::supported_joints_mask(); }

vfik_handle* vfik_create(int device, int io_dtype, int n_joints, int max_slots, int batch) {
    if (io_dtype != 32 && io_dtype != 64) { fail(VFIK_E_ARG, "io_dtype must be 32 or 64, got %d", io_dtype); return nullptr; }
    if (n_joints < 1 || n_joints > VFIK_MAX_JOINTS || !((vfik::supported_joints_mask() >> n_joints) & 1u)) {
        fail(VFIK_E_UNSUPPORTED, "no kernel built for %d joints (mask 0x%x)", n_joints, vfik::supported_joints_mask());
        return nullptr;
    }
    if (batch < 1 || max_slots < 0 || max_slots > 4096) { fail(VFIK_E_ARG, "bad batch %d / max_slots %d", batch, max_slots); return nullptr; }
    int ndev = vfik_device_count();
    if (device < 0 || device >= ndev) {
        fail(VFIK_E_HIP, "device %d not available (%d HIP devices visible); this library has no CPU path", device, ndev);
        return nullptr;
    }
    vfik_handle* h = new vfik_handle();
    h->device = device; h->io_dtype = io_dtype; h->n = n_joints; h->max_slots = max_slots; h->B = batch;
    h->esz = io_dtype == 32 ? 4 : 8;
    if (const char* e = std::getenv("VFIK_BLOCK")) {
        int b = std::atoi(e);
        if (b == 64 || b == 128 || b == 192 || b == 256) h->block = b;  // tuning knob; LDS per block = waves x 27-56 KB
    }
    if (const char* e = std::getenv("VFIK_SUB8_MAX_BATCH")) h->sub8_max_batch = h->sub8_max_batch_full = h->sub8_max_batch_ns = std::max(0, std::atoi(e));
    if (const char* e = std::getenv("VFIK_TWO_WAVES")) h->waves2 = std::atoi(e) != 0;
    h->knobs.io_dtype = io_dtype; h->knobs.n = n_joints;
    if (const char* e = std::getenv("VFIK_UNIFORM_IMAGE")) h->knobs.uni_allowed = std::atoi(e) != 0;
    if (const char* e = std::getenv("VFIK_ONE_CHUNK")) h->knobs.one_chunk_allowed = std::atoi(e) != 0;
    if (const char* e = std::getenv("VFIK_MIXED_ORDERS")) h->knobs.mixed_allowed = std::atoi(e) != 0;
    if (const char* e = std::getenv("VFIK_DH_PATTERN")) h->dhp_allowed = std::atoi(e) != 0;
    if (const char* e = std::getenv("VFIK_ZERO_COPY_MAX")) h->zero_copy_max = (size_t)std::max(0L, std::atol(e));
    auto bail = [&](const char* what) { if (g_err.empty()) fail(VFIK_E_HIP, "%s failed", what); vfik_destroy(h); return (vfik_handle*)nullptr; };
    if (hipSetDevice(device) != hipSuccess) return bail("hipSetDevice");
    if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) return bail("hipStreamCreate");
    {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0) h->n_simd = 4 * cus;
    }
    const size_t B = batch;
    h->Bpad = (batch + 63) / 64 * 64;
    // (the images' sizes: vfik_scene.h, image_shape)
    auto image_sz = [&](vfik::Image img) { return vfik::image_bytes(img, max_slots, io_dtype, (size_t)h->Bpad); };
    {   // the state a lean launch reads, in one allocation whose layout the kernel can derive (vfik_kernel.h: arena layout)
        const size_t sz_goal = image_sz(vfik::IMG_GOAL) + image_sz(vfik::IMG_AUX);   // goal block + aux block (funnel, hemisphere)
        const size_t sz_kc = VFIK_KCONST_SLOT(vfik::kconst_bytes(n_joints));   // (+ slack inside: the kinematics block is copied in whole 1-KiB rows)
        const size_t sz_lv = (size_t)((n_joints + 4) / 4) * h->Bpad * 4 * sizeof(float);
        const size_t sz_sf = image_sz(vfik::IMG_COMPACT);
        const size_t sz_su = image_sz(vfik::IMG_UNI);   // (never fewer planes than one chunk's: the one-chunk body reads them all)
        const size_t sz_sl = image_sz(vfik::IMG_SLOTS);
        const size_t sz_or = image_sz(vfik::IMG_ORDERS);   // (zeros: order 0, force 0)
        if (dev_alloc(h, &h->d_arena, sz_goal + sz_kc + sz_lv + sz_sf + sz_su + sz_sl + sz_or, true)) return bail("alloc state arena");
        char* a0 = static_cast<char*>(h->d_arena);
        h->d_goal = a0;
        h->d_funnel = a0 + image_sz(vfik::IMG_GOAL);
        h->d_kconst = a0 + sz_goal;
        h->d_lastvec = reinterpret_cast<float*>(a0 + sz_goal + sz_kc);
        h->d_slots_fast = a0 + sz_goal + sz_kc + sz_lv;
        h->d_slots_uni = a0 + sz_goal + sz_kc + sz_lv + sz_sf;   // (kernel side: slots_fast + uni_planes quad planes)
        h->d_slots = a0 + sz_goal + sz_kc + sz_lv + sz_sf + sz_su;
        h->d_orders = a0 + sz_goal + sz_kc + sz_lv + sz_sf + sz_su + sz_sl;
    }
    {   // vfik_move_fields' map, every entry MOVE_NONE until field sets arrive
        const size_t sz_map = image_sz(vfik::IMG_REPMAP), sz_smap = image_sz(vfik::IMG_SCENEMAPS);
        if (dev_alloc(h, (void**)&h->d_repmap, sz_map, false)) return bail("alloc repeller map");
        if (hipMemsetAsync(h->d_repmap, 0xFF, sz_map, h->stream) != hipSuccess) return bail("init repeller map");
        if (dev_alloc(h, (void**)&h->d_scenemap, sz_smap, false)) return bail("alloc scene maps");
        if (hipMemsetAsync(h->d_scenemap, 0xFF, sz_smap, h->stream) != hipSuccess) return bail("init scene maps");
    }
    {   // the uniform image starts out with every slot unused (radius -inf), like the zeros (force 0) of the other two images
        std::vector<char> plane((size_t)h->Bpad * 4 * h->esz, 0);
        for (int b = 0; b < h->Bpad; ++b) put_io(h, plane, (size_t)b * 4 + 3, -std::numeric_limits<double>::infinity());
        // (plane 0 stays like this for good: the slot every out-of-range quad reads; so do the planes past max_slots, which no call writes)
        for (int sidx = 0; sidx < vfik::image_shape(vfik::IMG_UNI, max_slots, io_dtype).planes; ++sidx)
            if (hipMemcpyAsync(static_cast<char*>(h->d_slots_uni) + (size_t)sidx * plane.size(), plane.data(), plane.size(), hipMemcpyHostToDevice, h->stream) != hipSuccess)
                return bail("init uniform image");
        if (hipStreamSynchronize(h->stream) != hipSuccess) return bail("init uniform image");
    }
    if (dev_alloc(h, (void**)&h->d_mixw, 16 * sizeof(double), true)) return bail("alloc mixw");
    h->arms.assign(B, vfik::ArmScene{});
#ifdef VFIK_STAMPS
    if (dev_alloc(h, (void**)&h->d_stamps, ((B + 63) / 64) * 10 * sizeof(unsigned long long), true)) return bail("alloc stamps");
#endif
    // defaults: identity tool (vf:154), sig = 1 (nullspace:91), reference default parameters
    if (vfik_reset_state(h) != VFIK_OK) return bail("reset_state");
    vfik_params p{};
    p.speed_scale = 1.0; p.lambda = 0.1; p.rot_slowdown = 0.3; p.null_gain = 0.5; p.lookahead = 0.3;
    p.jl_gain = 0.5; p.max_vel = 1.0; p.jp_kp = 1.5; p.jp_delta = 0.087;
    for (double& w : p.wy) w = 1.0;
    for (double& w : p.wq) w = 1.0;
    p.mix_w[0] = p.mix_w[1] = 1.0;
    h->params = p;
    {
        std::vector<double> all(B, p.speed_scale);
        if (vfik_set_speed_scale(h, 0, batch, all.data()) != VFIK_OK) return bail("speed scale");
        h->speed_set = true;
    }
    if (hipStreamSynchronize(h->stream) != hipSuccess) return bail("sync");
    return h;
}

void vfik_destroy(vfik_handle* h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    void* ptrs[] = {h->d_arena, h->d_tool, h->d_ext, h->d_mixw, h->d_stamps, h->d_mixw_arm, h->d_track, h->d_wts, h->d_rollq[0], h->d_rollq[1], h->d_objects, h->d_obs_pose, h->d_obs_v6,
                    h->d_qalign, h->d_repmap, h->d_scenemap, h->move_stage.p, h->d_goto_gate, h->goto_pending.p, h->d_goto_dist, h->d_gotoq[0], h->d_gotoq[1],
                    h->goto_stage.p, h->d_follow_len, h->d_js_ref, h->d_script_mixw, h->d_stall_best, h->d_stall_count, h->d_stall_own,
                    h->d_link_img, h->link_stage.p, h->couple_rep.p, h->d_wait_own};
    for (void* p : ptrs) if (p) (void)hipFree(p);
    if (h->arena_dev) (void)hipFree(h->arena_dev);
    if (h->arena_host) (void)hipHostFree(h->arena_host);
    for (auto& sc : h->sc) if (sc.p) (void)hipFree(sc.p);
    for (auto& ps : h->pipe) {
        if (ps.ev_out) (void)hipEventSynchronize(ps.ev_out);
        for (auto& s : ps.sc) if (s.p) (void)hipFree(s.p);
        for (hipEvent_t e : {ps.ev_in, ps.ev_k, ps.ev_out}) if (e) (void)hipEventDestroy(e);
    }
    if (h->s_in) (void)hipStreamDestroy(h->s_in);
    if (h->s_out) (void)hipStreamDestroy(h->s_out);
    if (h->own_stream && h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
}

int vfik_set_stream(vfik_handle* h, void* hip_stream) {
    if (check_handle(h)) return VFIK_E_ARG;
    if (quiesce(h) != VFIK_OK) return VFIK_E_HIP;
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (h->own_stream && h->stream) HIP_TRY(hipStreamDestroy(h->stream));
    // the caller's stream is used as given; NULL is HIP's default (null) stream of the device,
    // which is what torch.cuda.current_stream().cuda_stream is unless the caller switched streams
    h->stream = static_cast<hipStream_t>(hip_stream);
    h->own_stream = false;
    return VFIK_OK;
}

int vfik_set_chain(vfik_handle* h, const vfik_chain* c) {
    if (check_handle(h)) return VFIK_E_ARG;
    if (quiesce(h) != VFIK_OK) return VFIK_E_HIP;
    if (!c) return fail(VFIK_E_ARG, "null chain");
    if (c->n != h->n) return fail(VFIK_E_ARG, "chain has %d joints, handle was created for %d", c->n, h->n);
    for (int i = 0; i < c->n; ++i) {
        if (c->jtype[i] != 0 && c->jtype[i] != 1) return fail(VFIK_E_ARG, "joint %d: unknown type %d", i, c->jtype[i]);
        if (!(c->q_hi[i] > c->q_lo[i])) return fail(VFIK_E_ARG, "joint %d: q_hi must exceed q_lo", i);
    }
    for (int i = 0; i <= c->n; ++i)
        for (int k = 0; k < 12; ++k)
            if (!std::isfinite(c->B[i][k])) return fail(VFIK_E_ARG, "chain transform %d has a non-finite entry", i);
    const vfik_chain saved = h->chain;
    const bool was_set = h->chain_set;
    h->chain = *c;
    h->chain_set = true;
    const int rc = upload_kconst(h);
    if (rc != VFIK_OK) { h->chain = saved; h->chain_set = was_set; }
    else { h->n_links = 0; h->couple_on = false; h->wait_on = false; h->avoid_on = false; }   // (the link spheres were those of the old chain's frames)
    return rc;
}

static int upload_bridge_state(vfik_handle* h, int first_arm, int n_arms);

int vfik_set_params(vfik_handle* h, const vfik_params* p) {
    if (check_handle(h)) return VFIK_E_ARG;
    if (quiesce(h) != VFIK_OK) return VFIK_E_HIP;
    if (!p) return fail(VFIK_E_ARG, "null params");
    if (!(p->lambda >= 0.0) || !(p->speed_scale >= 0.0) || !(p->max_vel >= 0.0) || !std::isfinite(p->lambda))
        return fail(VFIK_E_ARG, "lambda, speed_scale and max_vel must be finite and >= 0");
    if ((p->flags & VFIK_F_JOINT_LIMIT_TASK) && !(p->flags & VFIK_F_NULLSPACE))
        return fail(VFIK_E_ARG, "VFIK_F_JOINT_LIMIT_TASK needs VFIK_F_NULLSPACE");
    const bool speed_changed = !h->speed_set || p->speed_scale != h->params.speed_scale;
    // (against what the caller passed last: weights promoted from equal per-arm rows are not the caller's, vfik_set_arm_weights)
    bool weights_changed = false;
    for (int k = 0; k < 6; ++k) weights_changed = weights_changed || p->wy[k] != h->params.wy[k];
    for (int k = 0; k < h->n; ++k) weights_changed = weights_changed || p->wq[k] != h->params.wq[k];
    const bool maxvel_changed = p->max_vel != h->params.max_vel;
    bool mixw_changed = false;
    for (int k = 0; k < VFIK_MIX_CHANNELS; ++k) mixw_changed = mixw_changed || p->mix_w[k] != h->params.mix_w[k];
    h->params = *p;
    if ((maxvel_changed || mixw_changed) && h->d_mixw_arm) {
        // vfik_params.max_vel / mix_w are batch-wide: a CHANGED value is written to every arm, like speed_scale
        // (with per-arm bridge state the kernel reads nothing else)
        HIP_TRY(hipSetDevice(h->device));
        for (int b = 0; b < h->B; ++b) {
            if (maxvel_changed) h->bridge_host[(size_t)b * 8 + 6] = p->max_vel;
            for (int k = 0; mixw_changed && k < VFIK_MIX_CHANNELS; ++k) h->bridge_host[(size_t)b * 8 + k] = p->mix_w[k];
        }
        const int rc = upload_bridge_state(h, 0, h->B);
        if (rc != VFIK_OK) return rc;
    }
    if (weights_changed) h->wts_promoted = false;
    if (weights_changed && h->d_wts) {  // new batch-wide IK weights replace every arm's own
        HIP_TRY(hipSetDevice(h->device));
        HIP_TRY(hipStreamSynchronize(h->stream));
        (void)hipFree(h->d_wts);
        h->d_wts = nullptr;
    }
    if (speed_changed) {  // vfik_params.speed_scale is the batch-wide /max_vel value: written to every arm
        std::vector<double> all(h->B, p->speed_scale);
        const int rc = vfik_set_speed_scale(h, 0, h->B, all.data());
        if (rc != VFIK_OK) return rc;
        h->speed_set = true;
    }
    return upload_kconst(h);
}

// device image of the per-arm IK weights: [6 + n][Bpad] doubles, every arm starting from the batch's
static int ensure_arm_weights(vfik_handle* h) {
    if (h->d_wts) return VFIK_OK;
    const size_t Bp = h->Bpad, rows = 6 + h->n;
    std::vector<double> img(rows * Bp, 1.0);
    for (size_t r = 0; r < rows; ++r) {
        const double* wy = h->wts_promoted ? h->shared_wy : h->params.wy;
        const double* wq = h->wts_promoted ? h->shared_wq : h->params.wq;
        const double v = r < 6 ? wy[r] : wq[r - 6];
        for (size_t b = 0; b < Bp; ++b) img[r * Bp + b] = v;
    }
    if (dev_alloc(h, (void**)&h->d_wts, img.size() * sizeof(double), false)) return VFIK_E_HIP;
    HIP_TRY(hipMemcpyAsync(h->d_wts, img.data(), img.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return VFIK_OK;
}

int vfik_set_arm_weights(vfik_handle* h, int first_arm, int n_arms, const double* wy, const double* wq) {
    if (check_handle(h)) return VFIK_E_ARG;
    if (quiesce(h) != VFIK_OK) return VFIK_E_HIP;
    if (check_arms(h, first_arm, n_arms)) return VFIK_E_ARG;
    if (!wy && !wq) return fail(VFIK_E_ARG, "vfik_set_arm_weights: give wy, wq or both");
    for (int j = 0; j < n_arms; ++j) {
        for (int k = 0; wy && k < 6; ++k)
            if (!std::isfinite(wy[(size_t)j * 6 + k])) return fail(VFIK_E_ARG, "arm %d: task weight %d is not finite", first_arm + j, k);
        for (int k = 0; wq && k < h->n; ++k)
            if (!std::isfinite(wq[(size_t)j * h->n + k])) return fail(VFIK_E_ARG, "arm %d: joint weight %d is not finite", first_arm + j, k);
    }
    HIP_TRY(hipSetDevice(h->device));
    if (first_arm == 0 && n_arms == h->B && wy && wq) {
        // The whole batch, and every arm with the same weights (a port-level caller forwards each arm's /weight bottle): these ARE batch-wide
        // weights -- stored as such, the arms' own dropped, so that the launches stay on the kernels built for plain chains (WTSC) instead
        // of the general variants.  Stored beside the caller's vfik_params, not in them: a later vfik_set_params that leaves wy / wq as the
        // caller last passed them must not write those back over these.
        bool same = true;
        for (int j = 1; j < n_arms && same; ++j)
            same = std::memcmp(wy + (size_t)j * 6, wy, 6 * sizeof(double)) == 0 && std::memcmp(wq + (size_t)j * h->n, wq, h->n * sizeof(double)) == 0;
        if (same) {
            for (int k = 0; k < 6; ++k) h->shared_wy[k] = wy[k];
            for (int k = 0; k < h->n; ++k) h->shared_wq[k] = wq[k];
            h->wts_promoted = true;
            if (h->d_wts) {
                HIP_TRY(hipStreamSynchronize(h->stream));
                (void)hipFree(h->d_wts);
                h->d_wts = nullptr;
            }
            return upload_kconst(h);
        }
    }
    if (ensure_arm_weights(h) != VFIK_OK) return VFIK_E_HIP;
    const size_t Bp = h->Bpad;
    std::vector<double> row(n_arms);
    for (int r = 0; r < 6 + h->n; ++r) {
        const double* src = r < 6 ? wy : wq;
        if (!src) continue;
        const int stride = r < 6 ? 6 : h->n, col = r < 6 ? r : r - 6;
        for (int j = 0; j < n_arms; ++j) row[j] = src[(size_t)j * stride + col];
        HIP_TRY(hipMemcpyAsync(h->d_wts + (size_t)r * Bp + first_arm, row.data(), n_arms * sizeof(double), hipMemcpyHostToDevice, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));  // `row` is reused
    }
    return VFIK_OK;
}

int vfik_set_tool(vfik_handle* h, const double* tool16, int per_arm) {
    if (check_handle(h)) return VFIK_E_ARG;
    if (quiesce(h) != VFIK_OK) return VFIK_E_HIP;
    if (!tool16) return fail(VFIK_E_ARG, "null tool");
    HIP_TRY(hipSetDevice(h->device));
    if (!per_arm) {  // one sticky tool frame for the batch: lives with the other shared constants
        for (int k = 0; k < 12; ++k) h->tool_shared[k] = tool16[k];
        h->tool_per_arm = 0;
        return upload_kconst(h);
    }
    const size_t B = h->B, Bp = h->Bpad;
    {   // every arm with the same frame (a port-level caller forwards each arm's /tool bottle, and a fleet of one robot type carries one
        // hand): that is the batch's shared tool, with the values as the per-arm image would hold them (rounded to the I/O type) -- the
        // launch stays on the PLAIN kernels (vfik_kernel.hip, TOOLC) instead of the general variants, 6.9 against 10.6 us for C3N
        bool same = true;
        for (size_t b = 1; b < B && same; ++b) same = std::memcmp(tool16 + b * 16, tool16, 12 * sizeof(double)) == 0;
        if (same) {
            for (int k = 0; k < 12; ++k) h->tool_shared[k] = h->io_dtype == 32 ? (double)(float)tool16[k] : tool16[k];
            h->tool_per_arm = 0;
            return upload_kconst(h);
        }
    }
    std::vector<char> buf(3 * Bp * 4 * h->esz, 0);
    for (size_t b = 0; b < B; ++b)
        for (int k = 0; k < 12; ++k) {  // rows 0..2 of the 4x4 -> 3 quad planes
            const double v = tool16[b * 16 + k];
            const size_t idx = ((size_t)(k >> 2) * Bp + b) * 4 + (k & 3);
            put_io(h, buf, idx, v);
        }
    if (!h->d_tool && dev_alloc(h, &h->d_tool, buf.size(), false)) return VFIK_E_HIP;
    HIP_TRY(hipMemcpyAsync(h->d_tool, buf.data(), buf.size(), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->tool_per_arm = 1;
    return VFIK_OK;
}

int vfik_set_fields(vfik_handle* h, int first_arm, int n_arms, const vfik_field* fields, int max_fields,
                    const int32_t* counts) {
    if (check_handle(h)) return VFIK_E_ARG;
    if (quiesce(h) != VFIK_OK) return VFIK_E_HIP;
    if (!fields || !counts) return fail(VFIK_E_ARG, "null fields / counts");
    if (check_arms(h, first_arm, n_arms)) return VFIK_E_ARG;
    if (max_fields < 0) return fail(VFIK_E_ARG, "negative max_fields");
    // validate everything before touching device state
    for (int j = 0; j < n_arms; ++j) {
        if (counts[j] < 0 || counts[j] > max_fields) return fail(VFIK_E_ARG, "arm %d: count %d outside [0, %d]", first_arm + j, counts[j], max_fields);
        const vfik_field* f = fields + (size_t)j * max_fields;
        int bad = 0;
        const int need = vfik::slots_needed(f, counts[j], &bad);
        if (need < 0) return fail(VFIK_E_ARG, "arm %d field %d: unknown type %d", first_arm + j, f[bad].id, f[bad].type);
        if (need > h->max_slots) return fail(VFIK_E_ARG, "arm %d needs %d slots, handle capacity is %d", first_arm + j, need, h->max_slots);
    }
    HIP_TRY(hipSetDevice(h->device));
    // pack (vfik_scene.h): the staging images of the call's arms and what each arm's set holds
    vfik::FieldImages im;
    std::vector<vfik::ArmScene> packed(n_arms);
    const int S = h->max_slots;
    if (h->io_dtype == 32) vfik::pack_fields<float>(fields, max_fields, counts, n_arms, S, im, packed.data());
    else vfik::pack_fields<double>(fields, max_fields, counts, n_arms, S, im, packed.data());
    auto planes = [&](vfik::Image img) { return (size_t)vfik::staged_planes(img, S, h->io_dtype); };
    const size_t qb = 4 * h->esz, w = (size_t)n_arms * qb, pitch = (size_t)h->Bpad * qb;
    const size_t gp = planes(vfik::IMG_GOAL) - 1;   // the goal block's last plane is copied apart
    char* dg = static_cast<char*>(h->d_goal) + (size_t)first_arm * qb;
    HIP_TRY(hipMemcpy2DAsync(dg, pitch, im.goal.data(), w, w, gp, hipMemcpyHostToDevice, h->stream));
    // plane 3 = (present, slow-down, force, speedScale): the 4th component belongs to vfik_set_speed_scale
    HIP_TRY(hipMemcpy2DAsync(dg + gp * pitch, qb, im.goal.data() + gp * w, qb, 3 * h->esz, n_arms, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpy2DAsync(static_cast<char*>(h->d_funnel) + (size_t)first_arm * qb, pitch, im.aux.data(), w, w, planes(vfik::IMG_AUX), hipMemcpyHostToDevice, h->stream));
    if (S > 0) {
        const size_t w16 = (size_t)n_arms * 16, pitch16 = (size_t)h->Bpad * 16;   // order planes and maps: 16 bytes per arm and plane
        char* ds = static_cast<char*>(h->d_slots) + (size_t)first_arm * qb;
        HIP_TRY(hipMemcpy2DAsync(ds, pitch, im.slots.data(), w, w, planes(vfik::IMG_SLOTS), hipMemcpyHostToDevice, h->stream));
        char* df = static_cast<char*>(h->d_slots_fast) + (size_t)first_arm * qb;
        HIP_TRY(hipMemcpy2DAsync(df, pitch, im.compact.data(), w, w, planes(vfik::IMG_COMPACT), hipMemcpyHostToDevice, h->stream));
        char* du = static_cast<char*>(h->d_slots_uni) + pitch + (size_t)first_arm * qb;   // (slot m in plane m + 1)
        HIP_TRY(hipMemcpy2DAsync(du, pitch, im.uni.data(), w, w, planes(vfik::IMG_UNI), hipMemcpyHostToDevice, h->stream));
        char* dor = static_cast<char*>(h->d_orders) + (size_t)first_arm * 16;
        HIP_TRY(hipMemcpy2DAsync(dor, pitch16, im.orders.data(), w16, w16, planes(vfik::IMG_ORDERS), hipMemcpyHostToDevice, h->stream));
        char* dm = reinterpret_cast<char*>(h->d_repmap) + (size_t)first_arm * 16;
        HIP_TRY(hipMemcpy2DAsync(dm, pitch16, im.repmap.data(), w16, w16, planes(vfik::IMG_REPMAP), hipMemcpyHostToDevice, h->stream));
        char* dsm = reinterpret_cast<char*>(h->d_scenemap) + (size_t)first_arm * 16;   // (the three maps' planes follow each other on both sides)
        HIP_TRY(hipMemcpy2DAsync(dsm, pitch16, im.scenemaps.data(), w16, w16, planes(vfik::IMG_SCENEMAPS), hipMemcpyHostToDevice, h->stream));
    }
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->fields_set = true;
    std::copy(packed.begin(), packed.end(), h->arms.begin() + first_arm);
    // what the batch's launches take from now on: decided over ALL arms (vfik_scene.h: plan_scene)
    h->scene = vfik::plan_scene(h->arms.data(), h->B, h->knobs);
    // a uniform pair other than the one in the device constants: there it goes
    if (h->scene.uni_ok && h->scene.have_pair && (h->scene.safe != h->uni_safe || h->scene.force != h->uni_force)) {
        h->uni_safe = h->scene.safe; h->uni_force = h->scene.force;
        if (h->chain_set) {  // (a chain set later writes the pair with the rest of the constants: upload_kconst)
            char* kc = static_cast<char*>(h->d_kconst);
            HIP_TRY(hipMemcpyAsync(kc + VFIK_KCONST_REP_SAFE_OFF(h->n), &h->uni_safe, sizeof(double), hipMemcpyHostToDevice, h->stream));
            HIP_TRY(hipMemcpyAsync(kc + VFIK_KCONST_REP_FORCE_OFF, &h->uni_force, sizeof(double), hipMemcpyHostToDevice, h->stream));
            HIP_TRY(hipStreamSynchronize(h->stream));
        }
    }
    return VFIK_OK;
}

// the checks the two forms of vfik_move_fields share
static int move_check(vfik_handle* h, int first_arm, int n_arms, const void* goal16, const void* rep4, int n_rep) {
    if (check_arms(h, first_arm, n_arms)) return VFIK_E_ARG;
    if (!goal16 && !rep4) return fail(VFIK_E_ARG, "vfik_move_fields: give goal16, rep4 or both");
    if (n_rep < 0 || n_rep > h->max_slots) return fail(VFIK_E_ARG, "n_rep %d outside [0, %d]", n_rep, h->max_slots);
    if (!h->fields_set) return fail(VFIK_E_STATE, "vfik_move_fields before any vfik_set_fields: there is nothing to move");
    return VFIK_OK;
}

// the images of the handle and the rows to write into them (an array with no rows is no array)
static vfik::MoveArgs move_args(const vfik_handle* h, int first_arm, int n_arms, const void* goal16, const void* rep4, int n_rep, const int32_t* active) {
    vfik::MoveArgs m{};
    m.goal = h->d_goal;
    m.slots = h->d_slots;
    m.slots_fast = h->d_slots_fast;
    m.slots_uni = h->d_slots_uni;
    m.repmap = h->d_repmap;
    m.goal16 = goal16;
    m.rep4 = n_rep > 0 ? rep4 : nullptr;
    m.active = active;
    m.first_arm = first_arm;
    m.n_arms = n_arms;
    m.n_rep = n_rep;
    m.S = h->max_slots;
    m.Bpad = h->Bpad;
    return m;
}

static int move_launch(vfik_handle* h, int first_arm, int n_arms, const void* goal16, const void* rep4, int n_rep, const int32_t* active) {
    const vfik::MoveArgs m = move_args(h, first_arm, n_arms, goal16, rep4, n_rep, active);
    if (!m.goal16 && !m.rep4) return VFIK_OK;   // (rep4 with no rows: nothing to write)
    hipError_t e = vfik::launch_move(h->io_dtype, m, h->stream);
    if (e != hipSuccess) return fail(VFIK_E_HIP, "move launch: %s", hipGetErrorString(e));
    return VFIK_OK;
}

int vfik_move_fields(vfik_handle* h, int first_arm, int n_arms, const void* goal16, const void* rep4, int n_rep, const int32_t* active) {
    if (check_handle(h)) return VFIK_E_ARG;
    if (drain_side_streams(h) != VFIK_OK) return VFIK_E_HIP;
    const int rc = move_check(h, first_arm, n_arms, goal16, rep4, n_rep);
    if (rc != VFIK_OK) return rc;
    HIP_TRY(hipSetDevice(h->device));
    return move_launch(h, first_arm, n_arms, goal16, rep4, n_rep, active);
}

int vfik_move_fields_host(vfik_handle* h, int first_arm, int n_arms, const double* goal16, const double* rep4, int n_rep) {
    if (check_handle(h)) return VFIK_E_ARG;
    if (drain_side_streams(h) != VFIK_OK) return VFIK_E_HIP;
    const int rc = move_check(h, first_arm, n_arms, goal16, rep4, n_rep);
    if (rc != VFIK_OK) return rc;
    HIP_TRY(hipSetDevice(h->device));
    if (n_rep == 0) rep4 = nullptr;
    const size_t ng = goal16 ? (size_t)n_arms * 16 : 0, nr = rep4 ? (size_t)n_arms * n_rep * 4 : 0;
    if (ng + nr == 0) return VFIK_OK;
    std::vector<char> buf((ng + nr) * h->esz);   // rounded as vfik_set_fields rounds p[] (NaN stays NaN)
    for (size_t k = 0; k < ng + nr; ++k) {
        const double v = k < ng ? goal16[k] : rep4[k - ng];
        put_io(h, buf, k, v);
    }
    if (reserve(h, h->move_stage, buf.size(), true, true) != VFIK_OK) return VFIK_E_HIP;
    char* d = static_cast<char*>(h->move_stage.p);
    HIP_TRY(hipMemcpyAsync(d, buf.data(), buf.size(), hipMemcpyHostToDevice, h->stream));
    const int rl = move_launch(h, first_arm, n_arms, goal16 ? d : nullptr, rep4 ? d + ng * h->esz : nullptr, n_rep, nullptr);
    if (rl != VFIK_OK) return rl;
    HIP_TRY(hipStreamSynchronize(h->stream));   // `buf` and the stage are reused
    return VFIK_OK;
}

// ---- link spheres: the other arm as an obstacle (link_kernel, vfik_aux.hip; the image and the checks of the list: vfik_links.h) ----
size_t vfik_link_sphere_size(void) { return sizeof(vfik_link_sphere); }

int vfik_set_link_spheres(vfik_handle* h, const vfik_link_sphere* s, int L) {
    if (check_handle(h)) return VFIK_E_ARG;
    if (quiesce(h) != VFIK_OK) return VFIK_E_HIP;
    if (!s) L = 0;
    if (!h->chain_set) return fail(VFIK_E_STATE, "vfik_set_link_spheres before vfik_set_chain: the spheres sit on the chain's links");
    char msg[160];
    if (vfik::links_check(h->chain, s, L, msg, sizeof msg)) return fail(VFIK_E_ARG, "%s", msg);
    HIP_TRY(hipSetDevice(h->device));
    if (refuse_capture(h->stream, "vfik_set_link_spheres uploads the handle's link image: call it before capturing the stream")) return VFIK_E_STATE;
    if (!h->d_link_img && dev_alloc(h, &h->d_link_img, sizeof(vfik::LinkImage), false)) return VFIK_E_HIP;
    vfik::LinkImage img;
    vfik::links_fill(h->chain, s, L, &img);
    HIP_TRY(hipStreamSynchronize(h->stream));   // (an earlier vfik_link_points may still read the old image)
    HIP_TRY(hipMemcpyAsync(h->d_link_img, &img, sizeof img, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->link_img = img;
    for (int j = 0; j < L; ++j) h->links[j] = s[j];
    h->n_links = L;
    h->couple_on = false;   // (its buffer has the old list's rows)
    h->wait_on = false;     // (the rule reads that buffer)
    h->avoid_on = false;    // (likewise)
    return VFIK_OK;
}

// the checks the two forms of vfik_link_points share
static int link_check(vfik_handle* h, const void* q, const void* rep4, int n_rep, int first_rep) {
    if (!q || !rep4) return fail(VFIK_E_ARG, "vfik_link_points: q and rep4 are required");
    if (first_rep < 0 || first_rep + h->n_links > n_rep) return fail(VFIK_E_ARG, "rows [%d, %d) outside the %d rows of rep4", first_rep, first_rep + h->n_links, n_rep);
    if (n_rep > h->max_slots) return fail(VFIK_E_ARG, "n_rep %d outside [0, %d]", n_rep, h->max_slots);
    if (h->n_links < 1) return fail(VFIK_E_STATE, "vfik_link_points before vfik_set_link_spheres: there is nothing to place");
    return VFIK_OK;
}

static int link_launch(vfik_handle* h, const void* q, const int32_t* src_arm, const void* xform12, void* rep4, void* traj, int n_rep, int first_rep) {
    vfik::LinkArgs a{};
    a.img = static_cast<const vfik::LinkImage*>(h->d_link_img);
    a.q = q; a.src_arm = src_arm; a.xform12 = xform12; a.rep4 = rep4; a.traj = traj;
    a.B = h->B; a.n_rep = n_rep; a.first_rep = first_rep;
    const hipError_t e = vfik::launch_link(h->io_dtype, a, h->stream);
    if (e != hipSuccess) return fail(VFIK_E_HIP, "link launch: %s", hipGetErrorString(e));
    return VFIK_OK;
}

int vfik_link_points(vfik_handle* h, const void* q, const int32_t* src_arm, const void* xform12, void* rep4, int n_rep, int first_rep) {
    if (check_handle(h)) return VFIK_E_ARG;
    if (drain_side_streams(h) != VFIK_OK) return VFIK_E_HIP;
    const int rc = link_check(h, q, rep4, n_rep, first_rep);
    if (rc != VFIK_OK) return rc;
    if (reinterpret_cast<uintptr_t>(rep4) % 16) return fail(VFIK_E_ARG, "rep4 must be 16-byte aligned: the kernel stores its rows in 16-byte pieces");
    HIP_TRY(hipSetDevice(h->device));
    return link_launch(h, q, src_arm, xform12, rep4, nullptr, n_rep, first_rep);
}

int vfik_link_points_host(vfik_handle* h, const double* q, const int32_t* src_arm, const double* xform12, double* rep4, int n_rep, int first_rep) {
    if (check_handle(h)) return VFIK_E_ARG;
    if (drain_side_streams(h) != VFIK_OK) return VFIK_E_HIP;
    const int rc = link_check(h, q, rep4, n_rep, first_rep);
    if (rc != VFIK_OK) return rc;
    HIP_TRY(hipSetDevice(h->device));
    // one stage: q | xform12 | the L rows per arm (16-byte aligned) | src_arm
    const size_t B = (size_t)h->B, L = (size_t)h->n_links;
    const size_t nq = B * h->n, nx = xform12 ? B * 12 : 0;
    const size_t out_off = ((nq + nx) * h->esz + 15) / 16 * 16, out_bytes = B * L * 4 * h->esz, src_off = out_off + out_bytes;
    std::vector<char> buf(src_off + (src_arm ? B * sizeof(int32_t) : 0));
    for (size_t k = 0; k < nq + nx; ++k) put_io(h, buf, k, k < nq ? q[k] : xform12[k - nq]);
    if (src_arm) std::memcpy(buf.data() + src_off, src_arm, B * sizeof(int32_t));
    if (reserve(h, h->link_stage, buf.size(), true, true) != VFIK_OK) return VFIK_E_HIP;
    char* d = static_cast<char*>(h->link_stage.p);
    HIP_TRY(hipMemcpyAsync(d, buf.data(), buf.size(), hipMemcpyHostToDevice, h->stream));
    const int rl = link_launch(h, d, src_arm ? reinterpret_cast<const int32_t*>(d + src_off) : nullptr, xform12 ? d + nq * h->esz : nullptr,
                               d + out_off, nullptr, (int)L, 0);
    if (rl != VFIK_OK) return rl;
    HIP_TRY(hipMemcpyAsync(buf.data() + out_off, d + out_off, out_bytes, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    for (size_t b = 0; b < B; ++b)
        for (size_t k = 0; k < L * 4; ++k) {
            const char* src = buf.data() + out_off + (b * L * 4 + k) * h->esz;
            double v;
            if (h->io_dtype == 32) { float f; std::memcpy(&f, src, sizeof f); v = f; } else std::memcpy(&v, src, sizeof v);
            rep4[(b * (size_t)n_rep + (size_t)first_rep) * 4 + k] = v;
        }
    return VFIK_OK;
}

size_t vfik_coupling_size(void) { return sizeof(vfik_coupling); }

int vfik_set_coupling(vfik_handle* h, const vfik_coupling* c) {
    if (check_handle(h)) return VFIK_E_ARG;
    if (!c) { h->couple_on = false; h->wait_on = false; h->avoid_on = false; return VFIK_OK; }
    if (h->n_links < 1) return fail(VFIK_E_STATE, "vfik_set_coupling before vfik_set_link_spheres: there is nothing to couple");
    if (c->reserved != 0) return fail(VFIK_E_ARG, "coupling: reserved must be 0");
    if (c->first_rep < 0 || c->first_rep + h->n_links > h->max_slots)
        return fail(VFIK_E_ARG, "coupling: repellers [%d, %d) outside the %d slots of the handle", c->first_rep, c->first_rep + h->n_links, h->max_slots);
    if (c->src_arm && (!gpu_visible(c->src_arm) || reinterpret_cast<uintptr_t>(c->src_arm) % sizeof(int32_t)))
        return fail(VFIK_E_ARG, "coupling: src_arm must be an int32-aligned DEVICE pointer (NULL: every arm its own source)");
    if (c->xform12 && (!gpu_visible(c->xform12) || reinterpret_cast<uintptr_t>(c->xform12) % h->esz))
        return fail(VFIK_E_ARG, "coupling: xform12 must be a DEVICE pointer aligned to the I/O type");
    if (c->link_traj && (!gpu_visible(c->link_traj) || reinterpret_cast<uintptr_t>(c->link_traj) % 16))
        return fail(VFIK_E_ARG, "coupling: link_traj must be a 16-byte aligned DEVICE pointer");
    HIP_TRY(hipSetDevice(h->device));
    if (refuse_capture(h->stream, "vfik_set_coupling allocates the handle's repeller rows: call it before capturing the stream")) return VFIK_E_STATE;
    if (drain_side_streams(h) != VFIK_OK) return VFIK_E_HIP;
    const size_t bytes = (size_t)h->B * (size_t)(c->first_rep + h->n_links) * 4 * h->esz;
    if (reserve(h, h->couple_rep, bytes, true, true) != VFIK_OK) return VFIK_E_HIP;
    HIP_TRY(hipMemsetAsync(h->couple_rep.p, 0xFF, h->couple_rep.bytes, h->stream));   // (all bits set is a NaN of either I/O type: "leave as it is")
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->couple = *c;
    h->couple_on = true;
    return VFIK_OK;
}

// ---- link-sphere clearance (clear_kernel, vfik_aux.hip; the checks and the mask's permutation: vfik_links.h) ----
// what the two forms of vfik_link_clearance share: the checks, then the mask in the image's order into the kernel's arguments
static int clear_args(vfik_handle* h, const void* q, const void* pts4, int n_rep, int first, int count, const uint32_t* mask, void* clear,
                      vfik::ClearArgs& a) {
    char msg[160];
    const int rc = vfik::clear_check(h->n_links, q, pts4, clear, n_rep, first, count, mask, msg, sizeof msg);
    if (rc != 0) return fail(rc, "vfik_link_clearance: %s", msg);
    a = vfik::ClearArgs{};
    a.img = static_cast<const vfik::LinkImage*>(h->d_link_img);
    a.B = h->B; a.n_rep = n_rep; a.first = first; a.count = count;
    vfik::clear_mask(h->link_img, mask, count, a.mask);
    return VFIK_OK;
}

static int clear_launch(vfik_handle* h, const vfik::ClearArgs& a) {
    const hipError_t e = vfik::launch_clear(h->io_dtype, a, h->stream);
    if (e != hipSuccess) return fail(VFIK_E_HIP, "clearance launch: %s", hipGetErrorString(e));
    return VFIK_OK;
}

int vfik_link_clearance(vfik_handle* h, const void* q, const void* pts4, int n_rep, int first, int count, const uint32_t* mask, void* clear,
                        int32_t* pair) {
    if (check_handle(h)) return VFIK_E_ARG;
    if (drain_side_streams(h) != VFIK_OK) return VFIK_E_HIP;
    vfik::ClearArgs a;
    const int rc = clear_args(h, q, pts4, n_rep, first, count, mask, clear, a);
    if (rc != VFIK_OK) return rc;
    HIP_TRY(hipSetDevice(h->device));
    a.q = q; a.pts4 = pts4; a.clear = clear; a.pair = pair;
    return clear_launch(h, a);
}

int vfik_link_clearance_host(vfik_handle* h, const double* q, const double* pts4, int n_rep, int first, int count, const uint32_t* mask,
                             double* clear, int32_t* pair) {
    if (check_handle(h)) return VFIK_E_ARG;
    if (drain_side_streams(h) != VFIK_OK) return VFIK_E_HIP;
    vfik::ClearArgs a;
    alignas(16) static const char aligned_stand_in = 0;   // (the caller's pts4 is copied: its alignment is not the kernel's concern)
    const int rc = clear_args(h, q, pts4 ? &aligned_stand_in : nullptr, n_rep, first, count, mask, clear, a);
    if (rc != VFIK_OK) return rc;
    HIP_TRY(hipSetDevice(h->device));
    if (refuse_capture(h->stream, "vfik_link_clearance_host copies and synchronises: not while the stream is being captured")) return VFIK_E_STATE;
    // one stage: q | the rows (16-byte aligned) | clear | pair
    const size_t B = (size_t)h->B, nq = B * h->n, np = B * (size_t)n_rep * 4;
    const size_t pts_off = (nq * h->esz + 15) / 16 * 16, clear_off = pts_off + np * h->esz, pair_off = (clear_off + B * h->esz + 15) / 16 * 16;
    std::vector<char> buf(pair_off + B * sizeof(int32_t));
    for (size_t k = 0; k < nq; ++k) put_io(h, buf, k, q[k]);
    for (size_t k = 0; k < np; ++k) put_io(h, buf, pts_off / h->esz + k, pts4[k]);
    if (reserve(h, h->link_stage, buf.size(), true, true) != VFIK_OK) return VFIK_E_HIP;
    char* const d = static_cast<char*>(h->link_stage.p);
    HIP_TRY(hipMemcpyAsync(d, buf.data(), clear_off, hipMemcpyHostToDevice, h->stream));
    a.q = d; a.pts4 = d + pts_off; a.clear = d + clear_off; a.pair = reinterpret_cast<int32_t*>(d + pair_off);
    const int rl = clear_launch(h, a);
    if (rl != VFIK_OK) return rl;
    HIP_TRY(hipMemcpyAsync(buf.data() + clear_off, d + clear_off, buf.size() - clear_off, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    for (size_t b = 0; b < B; ++b) {
        const char* src = buf.data() + clear_off + b * h->esz;
        if (h->io_dtype == 32) { float f; std::memcpy(&f, src, sizeof f); clear[b] = f; } else std::memcpy(&clear[b], src, sizeof(double));
    }
    if (pair) std::memcpy(pair, buf.data() + pair_off, B * sizeof(int32_t));
    return VFIK_OK;
}

// ---- arms that wait for room: the rule every block of a timed move under a coupling applies (wait_block) ----
size_t vfik_wait_rule_size(void) { return sizeof(vfik_wait_rule); }

int vfik_set_wait_rule(vfik_handle* h, const vfik_wait_rule* r) {
    if (check_handle(h)) return VFIK_E_ARG;
    if (!r) { h->wait_on = false; return VFIK_OK; }
    if (!h->couple_on) return fail(VFIK_E_STATE, "vfik_set_wait_rule before vfik_set_coupling: the rule measures against the coupling's rows");
    if (!std::isfinite(r->min_clearance)) return fail(VFIK_E_ARG, "wait rule: min_clearance must be finite");
    if (r->reserved != 0) return fail(VFIK_E_ARG, "wait rule: reserved must be 0");
    const int L = h->n_links;
    bool any = false;
    for (int i = 0; i < VFIK_MAX_LINK_SPHERES; ++i) any = any || r->mask[i] != 0;
    for (int i = 0; i < VFIK_MAX_LINK_SPHERES; ++i)
        if ((i >= L && r->mask[i] != 0) || (r->mask[i] >> L) != 0)
            return fail(VFIK_E_ARG, "wait rule: mask[%d] = 0x%08x names a sphere at or beyond the %d of the handle", i, (unsigned)r->mask[i], L);
    const struct { const char* name; const void* p; } ints[] = {{"yields", r->yields}, {"pair_traj", r->pair_traj}, {"waited", r->waited}};
    for (const auto& x : ints)
        if (x.p && (!gpu_visible(x.p) || reinterpret_cast<uintptr_t>(x.p) % sizeof(int32_t)))
            return fail(VFIK_E_ARG, "wait rule: %s must be an int32-aligned DEVICE pointer", x.name);
    if (r->clear_traj && (!gpu_visible(r->clear_traj) || reinterpret_cast<uintptr_t>(r->clear_traj) % h->esz))
        return fail(VFIK_E_ARG, "wait rule: clear_traj must be a DEVICE pointer aligned to the I/O type");
    HIP_TRY(hipSetDevice(h->device));
    if (refuse_capture(h->stream, "vfik_set_wait_rule allocates the handle's waited[B]: call it before capturing the stream")) return VFIK_E_STATE;
    if (drain_side_streams(h) != VFIK_OK) return VFIK_E_HIP;
    if (!h->d_wait_own) {
        if (dev_alloc(h, (void**)&h->d_wait_own, (size_t)h->B * sizeof(int32_t), false)) return VFIK_E_HIP;
        HIP_TRY(hipMemsetAsync(h->d_wait_own, 0, (size_t)h->B * sizeof(int32_t), h->stream));   // (nobody waited before the first timed move)
    }
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->wait = *r;
    vfik::clear_mask(h->link_img, any ? r->mask : nullptr, L, h->wait_mask);
    h->wait_on = true;
    return VFIK_OK;
}

int vfik_waited_host(vfik_handle* h, int32_t* out) {
    if (check_handle(h)) return VFIK_E_ARG;
    if (!out) return fail(VFIK_E_ARG, "vfik_waited_host: out[B] is required");
    if (!h->wait_on) return fail(VFIK_E_STATE, "vfik_waited_host: the handle has no wait rule (vfik_set_wait_rule)");
    HIP_TRY(hipSetDevice(h->device));
    if (refuse_capture(h->stream, "vfik_waited_host copies to the host and synchronises: not while the stream is being captured")) return VFIK_E_STATE;
    HIP_TRY(hipMemcpyAsync(out, h->wait.waited ? h->wait.waited : h->d_wait_own, (size_t)h->B * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return VFIK_OK;
}

// ---- whole-arm avoidance (avoid_kernel, vfik_aux.hip; the checks: vfik_links.h) ----
static size_t ext_chan_bytes(const vfik_handle* h) { return (size_t)h->B * h->n * h->esz; }
static void* ext_chan(const vfik_handle* h, int channel) { return static_cast<char*>(h->d_ext) + ext_chan_bytes(h) * (channel - 2); }

// what the two forms of vfik_link_avoid share: the checks, then the mask in the image's order and the law into the kernel's arguments
static int avoid_args(vfik_handle* h, const void* q, const void* pts4, int n_rep, int first, int count, const uint32_t* mask, double gain, double d0,
                      const void* out, int channel, vfik::AvoidArgs& a) {
    char msg[160];
    const int rc = vfik::avoid_check(h->n_links, q, pts4, out, n_rep, first, count, mask, gain, d0, channel, h->d_ext != nullptr, msg, sizeof msg);
    if (rc != 0) return fail(rc, "vfik_link_avoid: %s", msg);
    a = vfik::AvoidArgs{};
    a.img = static_cast<const vfik::LinkImage*>(h->d_link_img);
    a.B = h->B; a.n_rep = n_rep; a.first = first; a.count = count;
    a.gain = gain; a.d0 = d0;
    vfik::clear_mask(h->link_img, mask, count, a.mask);
    return VFIK_OK;
}

static int avoid_launch(vfik_handle* h, const vfik::AvoidArgs& a) {
    const hipError_t e = vfik::launch_avoid(h->io_dtype, h->n, a, h->stream);
    if (e != hipSuccess) return fail(VFIK_E_HIP, "avoid launch: %s", hipGetErrorString(e));
    return VFIK_OK;
}

int vfik_link_avoid(vfik_handle* h, const void* q, const void* pts4, int n_rep, int first, int count, const uint32_t* mask, double gain, double d0,
                    const void* scale, void* out, int channel) {
    if (check_handle(h)) return VFIK_E_ARG;
    if (drain_side_streams(h) != VFIK_OK) return VFIK_E_HIP;
    vfik::AvoidArgs a;
    const int rc = avoid_args(h, q, pts4, n_rep, first, count, mask, gain, d0, out, channel, a);
    if (rc != VFIK_OK) return rc;
    HIP_TRY(hipSetDevice(h->device));
    a.q = q; a.pts4 = pts4; a.scale = scale; a.out = out;
    if (channel >= 0) a.chan_out = ext_chan(h, channel);
    return avoid_launch(h, a);
}

int vfik_link_avoid_host(vfik_handle* h, const double* q, const double* pts4, int n_rep, int first, int count, const uint32_t* mask, double gain,
                         double d0, const double* scale, double* out) {
    if (check_handle(h)) return VFIK_E_ARG;
    if (drain_side_streams(h) != VFIK_OK) return VFIK_E_HIP;
    vfik::AvoidArgs a;
    alignas(16) static const char aligned_stand_in = 0;   // (the caller's pts4 is copied: its alignment is not the kernel's concern)
    const int rc = avoid_args(h, q, pts4 ? &aligned_stand_in : nullptr, n_rep, first, count, mask, gain, d0, out, -1, a);
    if (rc != VFIK_OK) return rc;
    HIP_TRY(hipSetDevice(h->device));
    if (refuse_capture(h->stream, "vfik_link_avoid_host copies and synchronises: not while the stream is being captured")) return VFIK_E_STATE;
    // one stage: q | the rows (16-byte aligned) | scale | out
    const size_t B = (size_t)h->B, nq = B * h->n, np = B * (size_t)n_rep * 4;
    const size_t pts_off = (nq * h->esz + 15) / 16 * 16, scale_off = pts_off + np * h->esz, out_off = (scale_off + B * h->esz + 15) / 16 * 16;
    std::vector<char> buf(out_off + nq * h->esz);
    for (size_t k = 0; k < nq; ++k) put_io(h, buf, k, q[k]);
    for (size_t k = 0; k < np; ++k) put_io(h, buf, pts_off / h->esz + k, pts4[k]);
    for (size_t k = 0; scale && k < B; ++k) put_io(h, buf, scale_off / h->esz + k, scale[k]);
    if (reserve(h, h->link_stage, buf.size(), true, true) != VFIK_OK) return VFIK_E_HIP;
    char* const d = static_cast<char*>(h->link_stage.p);
    HIP_TRY(hipMemcpyAsync(d, buf.data(), out_off, hipMemcpyHostToDevice, h->stream));
    a.q = d; a.pts4 = d + pts_off; a.scale = scale ? d + scale_off : nullptr; a.out = d + out_off;
    const int rl = avoid_launch(h, a);
    if (rl != VFIK_OK) return rl;
    HIP_TRY(hipMemcpyAsync(buf.data() + out_off, d + out_off, nq * h->esz, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    for (size_t k = 0; k < nq; ++k) {
        const char* src = buf.data() + out_off + k * h->esz;
        if (h->io_dtype == 32) { float f; std::memcpy(&f, src, sizeof f); out[k] = f; } else std::memcpy(&out[k], src, sizeof(double));
    }
    return VFIK_OK;
}

// ---- the avoid rule: the push every block of a timed move under a coupling writes into one ext channel (avoid_block) ----
size_t vfik_avoid_rule_size(void) { return sizeof(vfik_avoid_rule); }

int vfik_set_avoid_rule(vfik_handle* h, const vfik_avoid_rule* r) {
    if (check_handle(h)) return VFIK_E_ARG;
    if (quiesce(h) != VFIK_OK) return VFIK_E_HIP;
    if (!r) { h->avoid_on = false; return VFIK_OK; }
    if (!h->couple_on) return fail(VFIK_E_STATE, "vfik_set_avoid_rule before vfik_set_coupling: the rule pushes away from the coupling's rows");
    char msg[160];
    const int L = h->n_links;
    if (vfik::avoid_rule_check(L, r->gain, r->d0, r->channel, r->reserved, r->mask, msg, sizeof msg) != 0) return fail(VFIK_E_ARG, "avoid rule: %s", msg);
    if (r->scale && (!gpu_visible(r->scale) || reinterpret_cast<uintptr_t>(r->scale) % h->esz))
        return fail(VFIK_E_ARG, "avoid rule: scale must be a DEVICE pointer aligned to the I/O type");
    if (r->avoid_traj && (!gpu_visible(r->avoid_traj) || reinterpret_cast<uintptr_t>(r->avoid_traj) % h->esz))
        return fail(VFIK_E_ARG, "avoid rule: avoid_traj must be a DEVICE pointer aligned to the I/O type");
    HIP_TRY(hipSetDevice(h->device));
    if (refuse_capture(h->stream, "vfik_set_avoid_rule may allocate the handle's ext buffer and zeroes its channel: call it before capturing the stream")) return VFIK_E_STATE;
    if (!h->d_ext && dev_alloc(h, &h->d_ext, ext_chan_bytes(h) * (VFIK_MIX_CHANNELS - 2), true)) return VFIK_E_HIP;
    HIP_TRY(hipMemsetAsync(ext_chan(h, r->channel), 0, ext_chan_bytes(h), h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    bool any = false;
    for (int i = 0; i < VFIK_MAX_LINK_SPHERES; ++i) any = any || r->mask[i] != 0;
    h->avoid = *r;
    vfik::clear_mask(h->link_img, any ? r->mask : nullptr, L, h->avoid_mask);
    h->avoid_on = true;
    return VFIK_OK;
}

size_t vfik_scene_move_size(void) { return sizeof(vfik_scene_move); }

// the checks the two forms of vfik_move_scene share
static int scene_check(vfik_handle* h, int first_arm, int n_arms, const vfik_scene_move* mv) {
    if (!mv) return fail(VFIK_E_ARG, "vfik_move_scene: null vfik_scene_move");
    if (check_arms(h, first_arm, n_arms)) return VFIK_E_ARG;
    if (!mv->goal16 && !mv->rep4 && !mv->fun6 && !mv->hem6 && !mv->att16) return fail(VFIK_E_ARG, "vfik_move_scene: give at least one of goal16, rep4, fun6, hem6, att16");
    const struct { const char* name; int v; } counts[] = {{"n_rep", mv->n_rep}, {"n_fun", mv->n_fun}, {"n_hem", mv->n_hem}, {"n_att", mv->n_att}};
    for (const auto& c : counts)
        if (c.v < 0 || c.v > h->max_slots) return fail(VFIK_E_ARG, "%s %d outside [0, %d]", c.name, c.v, h->max_slots);
    if (!h->fields_set) return fail(VFIK_E_STATE, "vfik_move_scene before any vfik_set_fields: there is nothing to move");
    return VFIK_OK;
}

// (an array with no rows is no array; a move of goal and repellers alone is vfik_move_fields' launch)
static int scene_launch(vfik_handle* h, int first_arm, int n_arms, const vfik_scene_move& mv) {
    const void* rep4 = mv.n_rep > 0 ? mv.rep4 : nullptr;
    vfik::SceneMoveArgs s{};
    s.fun6 = mv.n_fun > 0 ? mv.fun6 : nullptr;
    s.hem6 = mv.n_hem > 0 ? mv.hem6 : nullptr;
    s.att16 = mv.n_att > 0 ? mv.att16 : nullptr;
    if (!s.fun6 && !s.hem6 && !s.att16) return move_launch(h, first_arm, n_arms, mv.goal16, rep4, rep4 ? mv.n_rep : 0, mv.active);
    s.m = move_args(h, first_arm, n_arms, mv.goal16, rep4, rep4 ? mv.n_rep : 0, mv.active);
    s.aux = h->d_funnel;
    s.scenemap = h->d_scenemap;
    s.n_fun = s.fun6 ? mv.n_fun : 0;
    s.n_hem = s.hem6 ? mv.n_hem : 0;
    s.n_att = s.att16 ? mv.n_att : 0;
    s.map_planes = vfik::image_shape(vfik::IMG_REPMAP, h->max_slots, h->io_dtype).planes;
    hipError_t e = vfik::launch_move_scene(h->io_dtype, s, h->stream);
    if (e != hipSuccess) return fail(VFIK_E_HIP, "scene move launch: %s", hipGetErrorString(e));
    return VFIK_OK;
}

int vfik_move_scene(vfik_handle* h, int first_arm, int n_arms, const vfik_scene_move* mv) {
    if (check_handle(h)) return VFIK_E_ARG;
    if (drain_side_streams(h) != VFIK_OK) return VFIK_E_HIP;
    const int rc = scene_check(h, first_arm, n_arms, mv);
    if (rc != VFIK_OK) return rc;
    HIP_TRY(hipSetDevice(h->device));
    return scene_launch(h, first_arm, n_arms, *mv);
}

int vfik_move_scene_host(vfik_handle* h, int first_arm, int n_arms, const vfik_scene_move* mv) {
    if (check_handle(h)) return VFIK_E_ARG;
    if (drain_side_streams(h) != VFIK_OK) return VFIK_E_HIP;
    const int rc = scene_check(h, first_arm, n_arms, mv);
    if (rc != VFIK_OK) return rc;
    if (mv->active) return fail(VFIK_E_ARG, "vfik_move_scene_host takes no active mask: give NaN rows");
    HIP_TRY(hipSetDevice(h->device));
    // the rows of 4 and 16 first: every part of the stage then starts as aligned as its loads want (rows of six: pairs)
    const double* src[5] = {static_cast<const double*>(mv->goal16), static_cast<const double*>(mv->rep4), static_cast<const double*>(mv->att16),
                            static_cast<const double*>(mv->fun6), static_cast<const double*>(mv->hem6)};
    const size_t per_arm[5] = {16, (size_t)mv->n_rep * 4, (size_t)mv->n_att * 16, (size_t)mv->n_fun * 6, (size_t)mv->n_hem * 6};
    size_t off[6] = {0, 0, 0, 0, 0, 0};
    for (int c = 0; c < 5; ++c) {
        if (per_arm[c] == 0) src[c] = nullptr;
        off[c + 1] = off[c] + (src[c] ? (size_t)n_arms * per_arm[c] : 0);
    }
    if (off[5] == 0) return VFIK_OK;
    std::vector<char> buf(off[5] * h->esz);   // rounded as vfik_set_fields rounds p[] (NaN stays NaN)
    for (int c = 0; c < 5; ++c)
        for (size_t k = off[c]; k < off[c + 1]; ++k) {
            const double v = src[c][k - off[c]];
            put_io(h, buf, k, v);
        }
    if (reserve(h, h->move_stage, buf.size(), true, true) != VFIK_OK) return VFIK_E_HIP;
    char* d = static_cast<char*>(h->move_stage.p);
    HIP_TRY(hipMemcpyAsync(d, buf.data(), buf.size(), hipMemcpyHostToDevice, h->stream));
    vfik_scene_move dv = *mv;
    dv.goal16 = src[0] ? d + off[0] * h->esz : nullptr;
    dv.rep4 = src[1] ? d + off[1] * h->esz : nullptr;
    dv.att16 = src[2] ? d + off[2] * h->esz : nullptr;
    dv.fun6 = src[3] ? d + off[3] * h->esz : nullptr;
    dv.hem6 = src[4] ? d + off[4] * h->esz : nullptr;
    const int rl = scene_launch(h, first_arm, n_arms, dv);
    if (rl != VFIK_OK) return rl;
    HIP_TRY(hipStreamSynchronize(h->stream));   // `buf` and the stage are reused
    return VFIK_OK;
}

int vfik_set_speed_scale(vfik_handle* h, int first_arm, int n_arms, const double* values) {
    if (check_handle(h)) return VFIK_E_ARG;
    if (quiesce(h) != VFIK_OK) return VFIK_E_HIP;
    if (!values) return fail(VFIK_E_ARG, "null values");
    if (check_arms(h, first_arm, n_arms)) return VFIK_E_ARG;
    for (int j = 0; j < n_arms; ++j)
        if (!(values[j] >= 0.0) || !std::isfinite(values[j])) return fail(VFIK_E_ARG, "arm %d: speedScale must be finite and >= 0", first_arm + j);
    HIP_TRY(hipSetDevice(h->device));
    std::vector<char> buf((size_t)n_arms * h->esz);
    for (int j = 0; j < n_arms; ++j) put_io(h, buf, j, values[j]);
    const size_t qb = 4 * h->esz;
    char* dst = static_cast<char*>(h->d_goal) + 3 * (size_t)h->Bpad * qb + (size_t)first_arm * qb + 3 * h->esz;
    HIP_TRY(hipMemcpy2DAsync(dst, qb, buf.data(), h->esz, h->esz, n_arms, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return VFIK_OK;
}

// Per-arm bridge state on the device: 2 quad planes [w0 w1 w2 w3 | w4 w5 max_vel -], mirrored on the host so
// that the two setters below can rewrite an arm's quads without reading them back.
static int upload_bridge_state(vfik_handle* h, int first_arm, int n_arms);
static int ensure_bridge_state(vfik_handle* h) {
    if (h->d_mixw_arm) return VFIK_OK;
    const size_t plane = (size_t)h->Bpad * 4 * h->esz;
    if (dev_alloc(h, &h->d_mixw_arm, 2 * plane, true)) return VFIK_E_HIP;
    h->bridge_host.assign((size_t)h->B * 8, 0.0);
    for (int b = 0; b < h->B; ++b) {  // every arm starts from the batch-wide values
        for (int k = 0; k < VFIK_MIX_CHANNELS; ++k) h->bridge_host[(size_t)b * 8 + k] = h->params.mix_w[k];
        h->bridge_host[(size_t)b * 8 + 6] = h->params.max_vel;
    }
    return upload_bridge_state(h, 0, h->B);
}

static int upload_bridge_state(vfik_handle* h, int first_arm, int n_arms) {
    const size_t qb = 4 * h->esz, plane = (size_t)h->Bpad * qb;
    std::vector<char> buf(2 * (size_t)n_arms * qb, 0);
    for (int j = 0; j < n_arms; ++j)
        for (int k = 0; k < 8; ++k) {
            const size_t idx = ((size_t)(k >> 2) * n_arms + j) * 4 + (k & 3);
            const double v = h->bridge_host[(size_t)(first_arm + j) * 8 + k];
            put_io(h, buf, idx, v);
        }
    char* dst = static_cast<char*>(h->d_mixw_arm) + (size_t)first_arm * qb;
    HIP_TRY(hipMemcpy2DAsync(dst, plane, buf.data(), (size_t)n_arms * qb, (size_t)n_arms * qb, 2, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    // all arms alike?  (O(B) per call; the callers are setters, not the cycle)
    const bool was = h->bridge_uniform;
    bool same = true;
    for (int b = 1; b < h->B && same; ++b) same = std::memcmp(&h->bridge_host[(size_t)b * 8], &h->bridge_host[0], 7 * sizeof(double)) == 0;
    h->bridge_uniform = same;
    if (same)
        for (int k = 0; k < 7; ++k) h->bridge_u[k] = h->io_dtype == 32 ? (double)(float)h->bridge_host[k] : h->bridge_host[k];
    if (same || was) return upload_kconst(h);
    return VFIK_OK;
}

int vfik_set_mixer_weights(vfik_handle* h, int first_arm, int n_arms, const double* w) {
    if (check_handle(h)) return VFIK_E_ARG;
    if (quiesce(h) != VFIK_OK) return VFIK_E_HIP;
    HIP_TRY(hipSetDevice(h->device));
    if (!w) {  // every arm's mixer weights back to the batch-wide vfik_params.mix_w; per-arm limiter speeds stay
        if (!h->d_mixw_arm) return VFIK_OK;
        for (int b = 0; b < h->B; ++b)
            for (int k = 0; k < VFIK_MIX_CHANNELS; ++k) h->bridge_host[(size_t)b * 8 + k] = h->params.mix_w[k];
        return upload_bridge_state(h, 0, h->B);
    }
    if (check_arms(h, first_arm, n_arms)) return VFIK_E_ARG;
    if (ensure_bridge_state(h) != VFIK_OK) return VFIK_E_HIP;
    for (int j = 0; j < n_arms; ++j)
        for (int k = 0; k < VFIK_MIX_CHANNELS; ++k) h->bridge_host[(size_t)(first_arm + j) * 8 + k] = w[(size_t)j * VFIK_MIX_CHANNELS + k];
    return upload_bridge_state(h, first_arm, n_arms);
}

int vfik_set_max_vel(vfik_handle* h, int first_arm, int n_arms, const double* values) {
    if (check_handle(h)) return VFIK_E_ARG;
    if (quiesce(h) != VFIK_OK) return VFIK_E_HIP;
    if (!values) return fail(VFIK_E_ARG, "null values");
    if (check_arms(h, first_arm, n_arms)) return VFIK_E_ARG;
    for (int j = 0; j < n_arms; ++j)
        if (!(values[j] >= 0.0)) return fail(VFIK_E_ARG, "arm %d: max_vel %g must be >= 0", first_arm + j, values[j]);   // (+inf: no limit, as vfik_params.max_vel)
    HIP_TRY(hipSetDevice(h->device));
    if (ensure_bridge_state(h) != VFIK_OK) return VFIK_E_HIP;
    for (int j = 0; j < n_arms; ++j) h->bridge_host[(size_t)(first_arm + j) * 8 + 6] = values[j];
    return upload_bridge_state(h, first_arm, n_arms);
}

int vfik_set_ext_cmd(vfik_handle* h, int channel, const void* cmd_host) {
    if (check_handle(h)) return VFIK_E_ARG;
    if (quiesce(h) != VFIK_OK) return VFIK_E_HIP;
    if (channel < 2 || channel >= VFIK_MIX_CHANNELS) return fail(VFIK_E_ARG, "channel %d: only 2..%d are external", channel, VFIK_MIX_CHANNELS - 1);
    if (h->avoid_on && channel == h->avoid.channel)
        return fail(VFIK_E_STATE, "vfik_set_ext_cmd: channel %d is written by the handle's avoid rule (vfik_set_avoid_rule)", channel);
    HIP_TRY(hipSetDevice(h->device));
    const size_t chan = (size_t)h->B * h->n * h->esz;
    if (!h->d_ext) {
        if (!cmd_host) return VFIK_OK;  // zeroing a channel that was never set
        if (dev_alloc(h, &h->d_ext, chan * (VFIK_MIX_CHANNELS - 2), true)) return VFIK_E_HIP;
    }
    char* dst = static_cast<char*>(h->d_ext) + chan * (channel - 2);
    if (cmd_host) HIP_TRY(hipMemcpyAsync(dst, cmd_host, chan, hipMemcpyHostToDevice, h->stream));
    else HIP_TRY(hipMemsetAsync(dst, 0, chan, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return VFIK_OK;
}

int vfik_reset_state(vfik_handle* h) {
    if (check_handle(h)) return VFIK_E_ARG;
    if (quiesce(h) != VFIK_OK) return VFIK_E_HIP;
    HIP_TRY(hipSetDevice(h->device));
    // lastvec = 0, sig = +1 (element n of every arm's state)
    const size_t planes = (size_t)(h->n + 4) / 4, Bp = h->Bpad;
    std::vector<float> img(planes * Bp * 4, 0.0f);
    for (size_t b = 0; b < Bp; ++b) img[((size_t)(h->n / 4) * Bp + b) * 4 + (h->n & 3)] = 1.0f;
    HIP_TRY(hipMemcpyAsync(h->d_lastvec, img.data(), img.size() * sizeof(float), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return VFIK_OK;
}

// the kernel a launch took, into the handle's record (vfik_launched_kernels) when it is not there yet: a few compares, no string, no allocation
static void note_launch(vfik_handle* h, const vfik::CyclePlan& p, unsigned flags) {
    const bool ns = flags & VFIK_F_NULLSPACE;
    for (int i = 0; i < h->launched_n; ++i) {
        const vfik::CyclePlan& r = h->launched[i].p;
        if (h->launched[i].ns == ns && r.family == p.family && r.plain == p.plain && r.roll == p.roll && r.fastf == p.fastf && r.lean == p.lean && r.cf == p.cf &&
            r.fun == p.fun && r.waves == p.waves && r.uni == p.uni && r.mixo == p.mixo && r.dhp == p.dhp && r.heavy == p.heavy)
            return;
    }
    if (h->launched_n == vfik_handle::LAUNCHED_MAX) { h->launched_lost = true; return; }
    h->launched[h->launched_n].p = p;
    h->launched[h->launched_n].ns = ns;
    ++h->launched_n;
}

// status_or: the launch ORs its status bits into what io->status holds (block 2.. of a goto), as cycle 2.. of a stepped rollout does
// mixw: per-arm mixer planes that stand in for the handle's (a script's own, vfik_script), or NULL
static int launch_cycles(vfik_handle* h, const vfik_io* io, int n_cycles, double dt, int clamp, void* q_out, hipStream_t stream, int status_or = 0,
                         const void* mixw = nullptr) {
    if (check_handle(h)) return VFIK_E_ARG;
    if (!io || !io->q) return fail(VFIK_E_ARG, "a control cycle needs io->q");
    if (!h->chain_set) return fail(VFIK_E_STATE, "vfik_set_chain has not been called");
    if (n_cycles > 0 && io->q_cmded) return fail(VFIK_E_ARG, "io->q_cmded (LWR position command form) is for vfik_step only");
    if (!io->q_lo != !io->q_hi) return fail(VFIK_E_ARG, "io->q_lo and io->q_hi come together (both or neither)");
    HIP_TRY(hipSetDevice(h->device));
    vfik::KArgs a;
    fill_kargs(h, io, a);
    if (mixw) a.mixw = mixw;
    if (reinterpret_cast<uintptr_t>(io->q) % 16) {
        // The kernels fetch q in 16-byte pieces up to its length rounded up to 16 bytes (vfik_kernel.hip, QBLK): from a q that is not 16-byte
        // aligned the last piece could reach into the next page.  Such a q is staged through an aligned buffer of the handle.
        const size_t qbytes = (size_t)h->B * h->n * h->esz;
        if (!h->d_qalign) {
            if (refuse_capture(stream, "io->q is not 16-byte aligned: its staging buffer is allocated at the first such call -- make one before capturing the stream")) return VFIK_E_STATE;
            if (dev_alloc(h, &h->d_qalign, (qbytes + 15) / 16 * 16, false)) return VFIK_E_HIP;
        }
        HIP_TRY(hipMemcpyAsync(h->d_qalign, io->q, qbytes, hipMemcpyDefault, stream));
        a.q = h->d_qalign;
    }
    a.dt = dt;
    a.clamp = clamp ? 1 : 0;
    if (n_cycles > 0 && (io->track_error || io->obj_dist))
        return fail(VFIK_E_ARG, "io->track_error / io->obj_dist are per control cycle: vfik_step only, not a rollout");
    if (n_cycles > 0 && !vfik::rollout_in_kernel(h->n, a.plain)) {
        // Long chains, and (round 4) chains with a tool, IK weights or prismatic joints, whose in-kernel loop spilled 12-268 B per
        // lane: the rollout is n_cycles single-cycle launches, each integrating q on its way out
        // (q ping-pongs between two device buffers; the caller's io->q is never written).  The kernel has
        // no registers left for loop-carried state at these sizes -- the in-kernel loop spills and is
        // slower than this (C5: 22 us per cycle against 17.4 us).  Outputs are those of the last cycle,
        // status bits accumulate, the nullspace state advances launch by launch.
        const size_t qbytes = (size_t)h->B * h->n * h->esz;
        for (int k = 0; k < 2; ++k)
            if (!h->d_rollq[k] && dev_alloc(h, &h->d_rollq[k], qbytes, false)) return VFIK_E_HIP;
        a.n_cycles = 0;
        const void* q_in = a.q;
        for (int c = 0; c < n_cycles; ++c) {
            const bool last = c == n_cycles - 1;
            vfik::KArgs k = a;
            k.q = q_in;
            k.q_out = (last && q_out) ? q_out : h->d_rollq[c & 1];
            k.status_or = c > 0 || status_or;
            if (!last) {  // intermediate cycles produce no outputs but the status bits
                k.qdot_vf = k.qdot_null = k.qdot_out = k.pose = k.pose_nt = k.v6 = k.qdist = k.goal_dist = k.q_ref_out = nullptr;
            }
            vfik::CyclePlan plan;
            hipError_t e = vfik::launch_cycle(h->io_dtype, h->n, k, h->block, stream, &plan);
            note_launch(h, plan, k.flags);
            if (e != hipSuccess) return fail(VFIK_E_HIP, "kernel launch: %s", hipGetErrorString(e));
            q_in = k.q_out;
        }
        return VFIK_OK;
    }
    a.n_cycles = n_cycles;
    a.q_out = q_out;
    a.status_or = status_or ? 1 : 0;
    // observers of the cycle (ABI 4): they read the cycle's own pose / twist on the device
    const bool want_track = io->track_error != nullptr, want_dist = io->obj_dist != nullptr;
    if (want_track || want_dist) {
        if (want_dist && (!h->d_objects || h->n_objects < 1)) return fail(VFIK_E_STATE, "io->obj_dist needs vfik_set_objects");
        // the observers' buffers are allocated at the first request: never under stream capture (an allocation there would be part of
        // the captured work or fail it) -- a caller that captures vfik_step with observers makes one such call outside the capture first
        if (((!a.pose && !h->d_obs_pose) || (want_track && ((!a.v6 && !h->d_obs_v6) || !h->d_track))) &&
            refuse_capture(stream, "io->track_error / io->obj_dist: the observers' device buffers are allocated at the first request -- make one such vfik_step call before capturing the stream"))
            return VFIK_E_STATE;
        if (!a.pose) {
            if (!h->d_obs_pose && dev_alloc(h, &h->d_obs_pose, (size_t)h->B * 16 * h->esz, true)) return VFIK_E_HIP;
            a.pose = h->d_obs_pose;
        }
        if (want_track && !a.v6) {
            if (!h->d_obs_v6 && dev_alloc(h, &h->d_obs_v6, (size_t)h->B * 6 * h->esz, true)) return VFIK_E_HIP;
            a.v6 = h->d_obs_v6;
        }
        if (want_track && !h->d_track && dev_alloc(h, (void**)&h->d_track, (size_t)38 * h->B * sizeof(double), true)) return VFIK_E_HIP;
    }
    vfik::CyclePlan plan;
    hipError_t e = vfik::launch_cycle(h->io_dtype, h->n, a, h->block, stream, &plan);
    h->sub8_launches += plan.family == vfik::CycleFamily::Sub8;
    note_launch(h, plan, a.flags);
    if (e != hipSuccess) return fail(VFIK_E_HIP, "kernel launch: %s", hipGetErrorString(e));
    if (want_track) {
        e = vfik::launch_track(h->io_dtype, a.pose, a.v6, h->d_track, io->track_error, io->active, h->B, stream);
        if (e != hipSuccess) return fail(VFIK_E_HIP, "track launch: %s", hipGetErrorString(e));
    }
    if (want_dist) {
        e = vfik::launch_monitor(h->io_dtype, a.pose, h->d_objects, h->n_objects, (long)h->B * h->n_objects, io->obj_dist, stream, io->active);
        if (e != hipSuccess) return fail(VFIK_E_HIP, "monitor launch: %s", hipGetErrorString(e));
    }
    return VFIK_OK;
}

int vfik_step(vfik_handle* h, const vfik_io* io) { return launch_cycles(h, io, 0, 0.0, 0, nullptr, h ? h->stream : nullptr); }

int vfik_rollout(vfik_handle* h, const vfik_io* io, int n_cycles, double dt, int clamp_to_limits, void* q_out) {
    if (n_cycles < 1 || n_cycles > 1000000) return fail(VFIK_E_ARG, "n_cycles %d outside [1, 1e6]", n_cycles);
    if (!std::isfinite(dt)) return fail(VFIK_E_ARG, "dt must be finite");
    return launch_cycles(h, io, n_cycles, dt, clamp_to_limits, q_out, h ? h->stream : nullptr);
}

int vfik_sync(vfik_handle* h) {
    if (check_handle(h)) return VFIK_E_ARG;
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return VFIK_OK;
}

// ---- host-pointer forms: the staging of a call's members (vfik_io_layout.h) between the caller's arrays and the device ----
namespace {
using vfik::IoStaging;

// every member in a device buffer of its own, grown on demand (sc[vfik::N_STAGED]); only the inputs: the outputs stay where they point
int map_buffers(vfik_handle* h, IoStaging& st, vfik_handle::DevBuf* sc, bool inputs_only, const char* what) {
    for (int i = 0; i < vfik::N_STAGED; ++i) {
        IoStaging::Member& m = st.m[i];
        if (!m.present || (inputs_only && !m.input)) continue;
        if (reserve(h, sc[i], m.bytes, false, false)) return fail(VFIK_E_HIP, "%s allocation failed", what);
        m.dev = sc[i].p;
    }
    return VFIK_OK;
}

// The three copies of a staged call, one hipMemcpyAsync per member.  Gated arms store nothing: under a gate (io->active) the caller's
// output rows go in before the launch, so that theirs come back as they went in -- the outputs that every arm writes excepted
// (IoStaging::Member::gated).
int copy_members(IoStaging& st, IoStaging::Which which, hipStream_t stream) {
    return st.each(which, [&](IoStaging::Member& m) {
        if (which == IoStaging::OUTPUTS) HIP_TRY(hipMemcpyAsync(m.host, m.dev, m.bytes, hipMemcpyDeviceToHost, stream));
        else HIP_TRY(hipMemcpyAsync(m.dev, m.host, m.bytes, hipMemcpyHostToDevice, stream));
        return (int)VFIK_OK;
    });
}
}  // namespace

// Host-pointer form, calls whose bytes are small against their member count: ONE copy in, the launches, ONE copy out, one synchronisation.  Inputs and
// outputs live in one device arena and one pinned host arena (same layout, every member 256-byte aligned); the caller's arrays are packed into /
// unpacked from the pinned arena on the host.  (Until round 3 every member was its own hipMemcpyAsync: with the eleven
// outputs the port-level host layer asks for that was 197 us per call for ONE arm, ~15 us per copy, against 34 us for
// qdot_out alone.)
static int cycles_host(vfik_handle* h, const vfik_io* io, int n_cycles, double dt, int clamp, void* q_out_host) {
    if (check_handle(h)) return VFIK_E_ARG;
    if (!io || !io->q) return fail(VFIK_E_ARG, "a control cycle needs io->q");
    HIP_TRY(hipSetDevice(h->device));
    IoStaging st(*io, h->B, h->io_dims());
    st.add(vfik::X_Q_OUT, q_out_host, (size_t)h->B * h->n * h->esz, true);   // (a gated arm's q is not integrated)
    st.layout();
    const size_t total = st.total, in_bytes = st.in_bytes;
    auto launch = [&]() {
        const vfik_io d = st.device_io();
        return n_cycles > 0 ? vfik_rollout(h, &d, n_cycles, dt, clamp, st.extra(vfik::X_Q_OUT).dev) : vfik_step(h, &d);
    };
    // The arena saves ~15 us per member beyond two and costs a host memcpy of every byte (~38 GB/s): measured 197 -> 40 us for
    // one arm with 13 members, 306 -> 190 us for 4 096 arms (2 MB), but 142 -> 236 us for a C3 step (q and qdot_out, 3.6 MB).
    if (total > ((size_t)256 << 10) && total > (size_t)std::max(0, st.members - 2) * ((size_t)512 << 10)) {
        // Few large members: the copies are bandwidth, not count -- every member straight between the caller's array and its
        // own device buffer.
        int rc = map_buffers(h, st, h->sc, false, "scratch");
        if (rc == VFIK_OK) rc = copy_members(st, IoStaging::INPUTS, h->stream);
        if (rc == VFIK_OK && io->active) rc = copy_members(st, IoStaging::GATED_OUTPUTS, h->stream);
        if (rc == VFIK_OK) rc = launch();
        if (rc == VFIK_OK) rc = copy_members(st, IoStaging::OUTPUTS, h->stream);
        if (rc != VFIK_OK) return rc;
        HIP_TRY(hipStreamSynchronize(h->stream));
        return VFIK_OK;
    }
    if (h->arena_bytes < total) {
        HIP_TRY(hipStreamSynchronize(h->stream));
        if (h->arena_dev) (void)hipFree(h->arena_dev);
        if (h->arena_host) (void)hipHostFree(h->arena_host);
        h->arena_dev = h->arena_host = nullptr;
        h->arena_bytes = 0;
        const size_t cap = total + total / 4 + 4096;
        if (hipMalloc(&h->arena_dev, cap) != hipSuccess || hipHostMalloc(&h->arena_host, cap, hipHostMallocMapped) != hipSuccess)
            return fail(VFIK_E_HIP, "arena allocation of %zu bytes failed", cap);
        if (hipHostGetDevicePointer(&h->arena_host_dev, h->arena_host, 0) != hipSuccess) { (void)hipGetLastError(); h->arena_host_dev = nullptr; }
        h->arena_bytes = cap;
    }
    char* const hostA = static_cast<char*>(h->arena_host);
    // A handful of arms (what vfclik itself runs: one arm per process set): no copy at all -- the kernels read the inputs from, and write
    // the outputs to, the pinned arena over the bus.  Two copy submissions and their DMA round trips cost such a call more than the
    // kernel's few PCIe transactions (ccb_rate: one arm, qdot_out only 23 -> 17 us; profiles/r03_ccb_rate.txt).
    const bool zero_copy = total <= h->zero_copy_max && h->arena_host_dev;
    char* const devA = zero_copy ? static_cast<char*>(h->arena_host_dev) : static_cast<char*>(h->arena_dev);
    st.map(devA);
    auto pack = [&](IoStaging::Member& m) { std::memcpy(hostA + m.off, m.host, m.bytes); return 0; };
    st.each(IoStaging::INPUTS, pack);
    size_t h2d = in_bytes;   // without a gate the input prefix alone goes to the device, with one the whole arena
    if (io->active && total > in_bytes) { st.each(IoStaging::GATED_OUTPUTS, pack); h2d = total; }
    if (!zero_copy) HIP_TRY(hipMemcpyAsync(devA, hostA, h2d, hipMemcpyHostToDevice, h->stream));
    const int rc = launch();
    if (rc != VFIK_OK) return rc;
    if (!zero_copy && total > in_bytes) HIP_TRY(hipMemcpyAsync(hostA + in_bytes, devA + in_bytes, total - in_bytes, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    st.each(IoStaging::OUTPUTS, [&](IoStaging::Member& m) { std::memcpy(m.host, hostA + m.off, m.bytes); return 0; });
    return VFIK_OK;
}

int vfik_step_host(vfik_handle* h, const vfik_io* io) { return cycles_host(h, io, 0, 0.0, 0, nullptr); }

int vfik_rollout_host(vfik_handle* h, const vfik_io* io, int n_cycles, double dt, int clamp_to_limits, void* q_out) {
    if (n_cycles < 1) return fail(VFIK_E_ARG, "n_cycles must be >= 1");
    return cycles_host(h, io, n_cycles, dt, clamp_to_limits, q_out);
}

// ---- timed moves: batched goto (handlers.py:346-440), waypoint lists (a script of gotoFrame calls, handlers.py:346-387), joint-space goto and
// posture lists (set_ref_js, handlers.py:544-576).  Every form is blocks of `stride` cycles through launch_cycles, as vfik_rollout runs them, one
// check kernel after each block, the handle's gate, pending[k], ping-pong q rows and optional traces: ONE vfik::TimedMove (vfik_io_layout.h) that each
// form's check fills from its own options, one run loop on it. ----
size_t vfik_goto_opts_size(void) { return sizeof(vfik_goto_opts); }
size_t vfik_follow_opts_size(void) { return sizeof(vfik_follow_opts); }
size_t vfik_goto_js_opts_size(void) { return sizeof(vfik_goto_js_opts); }
size_t vfik_follow_js_opts_size(void) { return sizeof(vfik_follow_js_opts); }
size_t vfik_script_opts_size(void) { return sizeof(vfik_script_opts); }

namespace {
using vfik::TimedMove;

// the members every form's options carry under the same names
extern "C++" {
template <typename O>
TimedMove timed_of(const vfik_io* io, const O* o, bool joint, bool list) {
    TimedMove m{};
    m.io = io;
    m.joint = joint;
    m.list = list;
    m.n_cycles = o->n_cycles; m.stride = o->stride; m.dt = o->dt;
    m.clamp = o->clamp_to_limits; m.hold = o->hold;
    m.x[vfik::X_PENDING] = o->pending; m.x[vfik::X_Q_OUT] = o->q_out; m.x[vfik::X_Q_TRAJ] = o->q_traj;
    return m;
}
}

// what every form refuses, before anything is enqueued
int timed_check(vfik_handle* h, TimedMove& m) {
    const vfik_io* io = m.io;
    if (!io || !io->q) return fail(VFIK_E_ARG, "a goto needs io->q");
    if (m.stride < 1) return fail(VFIK_E_ARG, "stride %d: at least one cycle between two checks", m.stride);
    if (m.n_cycles < 1 || m.n_cycles > 1000000) return fail(VFIK_E_ARG, "n_cycles %d outside [1, 1e6]", m.n_cycles);
    if (m.n_cycles % m.stride) return fail(VFIK_E_ARG, "n_cycles %d is no multiple of stride %d", m.n_cycles, m.stride);
    if (!std::isfinite(m.dt)) return fail(VFIK_E_ARG, "dt must be finite");
    if (!m.joint && (!(m.prec[0] >= 0.0) || !(m.prec[1] >= 0.0)))
        return fail(VFIK_E_ARG, "goal precision (%g m, %g rad) must not be negative or NaN", m.prec[0], m.prec[1]);
    if (io->q_cmded) return fail(VFIK_E_ARG, "io->q_cmded (LWR position command form) is for vfik_step only");
    if (io->track_error || io->obj_dist) return fail(VFIK_E_ARG, "io->track_error / io->obj_dist are per control cycle: vfik_step only, not a goto");
    if (!io->q_lo != !io->q_hi) return fail(VFIK_E_ARG, "io->q_lo and io->q_hi come together (both or neither)");
    if (!h->chain_set) return fail(VFIK_E_STATE, "vfik_set_chain has not been called");
    if (h->couple_on && !h->fields_set) return fail(VFIK_E_STATE, "a timed move under a coupling before any vfik_set_fields: there are no repellers to move");
    if (h->avoid_on && !(h->params.flags & VFIK_F_MIXER))
        return fail(VFIK_E_STATE, "a timed move under an avoid rule: the push enters through mixer channel %d, and the handle's params lack VFIK_F_MIXER", (int)h->avoid.channel);
    m.n_checks = m.n_cycles / m.stride;
    m.gated = m.hold || io->active || m.list || (h->stall_on && h->stall.stop) || h->wait_on;   // (a stalled arm that stops, and one that waits, are gated like a held one)
    return VFIK_OK;
}

int goto_check(vfik_handle* h, const vfik_io* io, const vfik_goto_opts* o, TimedMove& m) {
    if (check_handle(h)) return VFIK_E_ARG;
    if (!io || !io->q) return fail(VFIK_E_ARG, "a goto needs io->q");
    if (!o || !o->arrived) return fail(VFIK_E_ARG, "vfik_goto: the options and their arrived[B] are required");
    m = timed_of(io, o, false, false);
    m.prec[0] = o->pos_prec; m.prec[1] = o->rot_prec;
    m.x[vfik::X_ARRIVED] = o->arrived; m.x[vfik::X_DIST_TRAJ] = o->dist_traj;
    return timed_check(h, m);
}

int follow_check(vfik_handle* h, const vfik_io* io, const vfik_follow_opts* o, TimedMove& m) {
    if (check_handle(h)) return VFIK_E_ARG;
    if (!o || !o->way16 || !o->reached || !o->next) return fail(VFIK_E_ARG, "vfik_follow: the options, their way16[B][W][16], reached[B][W] and next[B] are required");
    if (o->n_way < 1) return fail(VFIK_E_ARG, "n_way %d: a path has at least one waypoint", o->n_way);
    if (reinterpret_cast<uintptr_t>(o->way16) % 16) return fail(VFIK_E_ARG, "way16 must be 16-byte aligned: the kernel loads its rows in 16-byte pieces");
    if (!(o->via_pos_prec >= 0.0) || !(o->via_rot_prec >= 0.0))
        return fail(VFIK_E_ARG, "via precision (%g m, %g rad) must not be negative or NaN", o->via_pos_prec, o->via_rot_prec);
    m = timed_of(io, o, false, true);
    m.n_way = o->n_way;
    m.prec[0] = o->pos_prec; m.prec[1] = o->rot_prec; m.via_prec[0] = o->via_pos_prec; m.via_prec[1] = o->via_rot_prec;
    m.x[vfik::X_WAY16] = const_cast<void*>(o->way16); m.x[vfik::X_REACHED] = o->reached; m.x[vfik::X_NEXT] = o->next;
    m.x[vfik::X_DIST_TRAJ] = o->dist_traj; m.x[vfik::X_WAY_TRAJ] = o->way_traj;
    return timed_check(h, m);
}

// prec[n] of a joint form, given and none of it negative or NaN, into the move
int js_prec(const vfik_handle* h, const double* prec, const char* form, const char* what, double* into) {
    if (!prec) return fail(VFIK_E_ARG, "%s: prec[n], the goal precision per joint, is required", form);
    for (int i = 0; i < h->n; ++i) {
        if (!(prec[i] >= 0.0)) return fail(VFIK_E_ARG, "%s[%d] = %g: a goal precision must not be negative or NaN", what, i, prec[i]);
        into[i] = prec[i];
    }
    return VFIK_OK;
}

int goto_js_check(vfik_handle* h, const vfik_io* io, const vfik_goto_js_opts* o, TimedMove& m) {
    if (check_handle(h)) return VFIK_E_ARG;
    if (!o || !o->arrived) return fail(VFIK_E_ARG, "vfik_goto_js: the options and their arrived[B] are required");
    m = timed_of(io, o, true, false);
    m.x[vfik::X_ARRIVED] = o->arrived; m.x[vfik::X_DIFF] = o->diff;
    const int rc = timed_check(h, m);
    if (rc != VFIK_OK) return rc;
    if (!io->q_ref) return fail(VFIK_E_ARG, "vfik_goto_js needs io->q_ref, the joint reference of every arm");
    return js_prec(h, o->prec, "vfik_goto_js", "prec", m.prec);
}

int follow_js_check(vfik_handle* h, const vfik_io* io, const vfik_follow_js_opts* o, TimedMove& m) {
    if (check_handle(h)) return VFIK_E_ARG;
    if (!o || !o->wayq || !o->reached || !o->next) return fail(VFIK_E_ARG, "vfik_follow_js: the options, their wayq[B][W][n], reached[B][W] and next[B] are required");
    if (o->n_way < 1) return fail(VFIK_E_ARG, "n_way %d: a list has at least one posture", o->n_way);
    if (reinterpret_cast<uintptr_t>(o->wayq) % h->esz) return fail(VFIK_E_ARG, "wayq must be aligned to its element type");
    m = timed_of(io, o, true, true);
    m.n_way = o->n_way;
    m.x[vfik::X_WAYQ] = const_cast<void*>(o->wayq); m.x[vfik::X_REACHED] = o->reached; m.x[vfik::X_NEXT] = o->next;
    m.x[vfik::X_DIFF] = o->diff; m.x[vfik::X_WAY_TRAJ] = o->way_traj;
    const int rc = timed_check(h, m);
    if (rc != VFIK_OK) return rc;
    if (io->q_ref) return fail(VFIK_E_ARG, "vfik_follow_js supplies io->q_ref itself (the handle's reference row): leave it NULL");
    if (js_prec(h, o->prec, "vfik_follow_js", "prec", m.prec) != VFIK_OK) return VFIK_E_ARG;
    return js_prec(h, o->via_prec ? o->via_prec : o->prec, "vfik_follow_js", "via_prec", m.via_prec);
}

// a motion script: a waypoint list's move (its blocks, distance row and traces) with the joint rule's members beside it
int script_check(vfik_handle* h, const vfik_io* io, const vfik_script_opts* o, TimedMove& m) {
    if (check_handle(h)) return VFIK_E_ARG;
    if (!o || !o->kind || !o->way16 || !o->wayq || !o->reached || !o->next)
        return fail(VFIK_E_ARG, "vfik_script: the options, their kind[B][W], way16[B][W][16], wayq[B][W][n], reached[B][W] and next[B] are required");
    if (o->n_way < 1) return fail(VFIK_E_ARG, "n_way %d: a script has at least one step", o->n_way);
    if (reinterpret_cast<uintptr_t>(o->way16) % 16) return fail(VFIK_E_ARG, "way16 must be 16-byte aligned: the kernel loads its rows in 16-byte pieces");
    if (reinterpret_cast<uintptr_t>(o->wayq) % h->esz) return fail(VFIK_E_ARG, "wayq must be aligned to its element type");
    if (reinterpret_cast<uintptr_t>(o->kind) % sizeof(int32_t)) return fail(VFIK_E_ARG, "kind must be aligned to int32");
    if (!(o->via_pos_prec >= 0.0) || !(o->via_rot_prec >= 0.0))
        return fail(VFIK_E_ARG, "via precision (%g m, %g rad) must not be negative or NaN", o->via_pos_prec, o->via_rot_prec);
    for (int k = 0; k < 4; ++k)
        if (!std::isfinite(o->mix_frame[k]) || !std::isfinite(o->mix_posture[k]))
            return fail(VFIK_E_ARG, "mix_frame[%d] = %g, mix_posture[%d] = %g: a mixer weight must be finite", k, o->mix_frame[k], k, o->mix_posture[k]);
    m = timed_of(io, o, false, true);
    m.script = true;
    m.n_way = o->n_way;
    m.prec[0] = o->pos_prec; m.prec[1] = o->rot_prec; m.via_prec[0] = o->via_pos_prec; m.via_prec[1] = o->via_rot_prec;
    for (int k = 0; k < 4; ++k) { m.mix[0][k] = o->mix_frame[k]; m.mix[1][k] = o->mix_posture[k]; }
    m.x[vfik::X_KIND] = const_cast<int32_t*>(o->kind);
    m.x[vfik::X_WAY16] = const_cast<void*>(o->way16); m.x[vfik::X_WAYQ] = const_cast<void*>(o->wayq);
    m.x[vfik::X_REACHED] = o->reached; m.x[vfik::X_NEXT] = o->next;
    m.x[vfik::X_DIST_TRAJ] = o->dist_traj; m.x[vfik::X_WAY_TRAJ] = o->way_traj; m.x[vfik::X_DIFF] = o->diff;
    const int rc = timed_check(h, m);
    if (rc != VFIK_OK) return rc;
    if (io->q_ref) return fail(VFIK_E_ARG, "vfik_script supplies io->q_ref itself (the handle's reference row): leave it NULL");
    if (js_prec(h, o->prec, "vfik_script", "prec", m.js_prec) != VFIK_OK) return VFIK_E_ARG;
    if (js_prec(h, o->via_prec ? o->via_prec : o->prec, "vfik_script", "via_prec", m.js_via_prec) != VFIK_OK) return VFIK_E_ARG;
    if (!(h->params.flags & VFIK_F_MIXER)) return fail(VFIK_E_STATE, "vfik_script switches controllers through the mixer: the handle's params lack VFIK_F_MIXER");
    return VFIK_OK;
}

vfik::TimedDims timed_dims(const vfik_handle* h, const TimedMove& m) { return {(size_t)h->B, (size_t)h->n, h->esz, (size_t)m.n_way, (size_t)m.n_checks}; }

// the handle's buffers this move needs (first call: never under stream capture) and pending[] zeroed
int timed_reserve(vfik_handle* h, TimedMove& m) {
    const vfik_io* io = m.io;
    const size_t qrow = (size_t)h->B * h->n * h->esz, pend = (size_t)m.n_checks * sizeof(int);
    const bool need_pending = !m.x[vfik::X_PENDING] && h->goto_pending.bytes < pend;
    const bool need_dist = !m.joint && !m.x[vfik::X_DIST_TRAJ] && !io->goal_dist && !h->d_goto_dist;
    const bool need_q = !m.x[vfik::X_Q_TRAJ] && !h->d_gotoq[0];
    // a block reads io->q or a row of q_traj: one that is not 16-byte aligned goes through launch_cycles' staging buffer
    const bool odd_q = reinterpret_cast<uintptr_t>(io->q) % 16 ||
                       (m.x[vfik::X_Q_TRAJ] && m.n_checks > 1 && (reinterpret_cast<uintptr_t>(m.x[vfik::X_Q_TRAJ]) % 16 || qrow % 16));
    const bool need_ref = ((m.joint && m.list) || m.script) && !h->d_js_ref;   // the row a posture list's or a script's blocks read as io->q_ref
    const bool need_mixw = m.script && !h->d_script_mixw;                      // the planes a script's blocks read as the per-arm mixer weights
    if (!h->d_goto_gate || need_pending || need_dist || need_q || (odd_q && !h->d_qalign) || (m.list && !h->d_follow_len) || need_ref || need_mixw) {
        if (refuse_capture(h->stream, "vfik_goto / vfik_follow: the handle's device buffers (gate, pending, distance row, q rows) are allocated at the first request -- make one such call before capturing the stream"))
            return VFIK_E_STATE;
        if (m.list && !h->d_follow_len && dev_alloc(h, (void**)&h->d_follow_len, (size_t)h->B * sizeof(int), false)) return VFIK_E_HIP;
        if (need_ref && dev_alloc(h, &h->d_js_ref, (qrow + 15) / 16 * 16, false)) return VFIK_E_HIP;
        if (need_mixw && dev_alloc(h, &h->d_script_mixw, 2 * (size_t)h->Bpad * 4 * h->esz, true)) return VFIK_E_HIP;
        if (!h->d_goto_gate && dev_alloc(h, (void**)&h->d_goto_gate, (size_t)h->B * sizeof(int), false)) return VFIK_E_HIP;
        // (synchronised: an earlier goto may still count into the smaller array)
        if (need_pending && reserve(h, h->goto_pending, pend, true, true)) return VFIK_E_HIP;
        if (need_dist && dev_alloc(h, &h->d_goto_dist, (size_t)h->B * 2 * h->esz, false)) return VFIK_E_HIP;
        for (int k = 0; need_q && k < 2; ++k)
            if (!h->d_gotoq[k] && dev_alloc(h, &h->d_gotoq[k], (qrow + 15) / 16 * 16, false)) return VFIK_E_HIP;
        if (odd_q && !h->d_qalign && dev_alloc(h, &h->d_qalign, (qrow + 15) / 16 * 16, false)) return VFIK_E_HIP;
    }
    if (!m.x[vfik::X_PENDING]) m.x[vfik::X_PENDING] = h->goto_pending.p;
    HIP_TRY(hipMemsetAsync(m.x[vfik::X_PENDING], 0, pend, h->stream));
    return VFIK_OK;
}

// the check after block k; k < 0 (w == NULL): the pass in front of block 0, which sets the gate and the arms' state
int timed_launch_check(vfik_handle* h, const TimedMove& m, int k, const vfik::BlockRows* w) {
    vfik::CheckArgs g{};
    g.gate = h->d_goto_gate;
    g.active = m.io->active;
    g.B = h->B; g.n = h->n; g.W = m.n_way; g.k = k; g.stride = m.stride; g.hold = m.hold ? 1 : 0;
    g.Bpad = h->Bpad;
    if (w) {
        g.pending = static_cast<int32_t*>(m.x[vfik::X_PENDING]) + k;
        g.q_prev = w->q_prev; g.q_now = w->q_now;
        g.dist = w->dist; g.dist_prev = w->dist_prev;
        g.way_now = w->way_now; g.way_prev = w->way_prev;
    }
    g.arrived = static_cast<int32_t*>(m.x[vfik::X_ARRIVED]);
    g.reached = static_cast<int32_t*>(m.x[vfik::X_REACHED]);
    g.next = static_cast<int32_t*>(m.x[vfik::X_NEXT]);
    g.len = h->d_follow_len;
    g.way = m.x[m.joint ? vfik::X_WAYQ : vfik::X_WAY16];
    g.goal = h->d_goal;
    g.ref = m.list ? h->d_js_ref : const_cast<void*>(m.io->q_ref);
    g.diff = m.x[vfik::X_DIFF];
    std::memcpy(g.prec, m.prec, sizeof g.prec);   // (all of both: the Cartesian pair sits in [0], [1] whatever n is)
    std::memcpy(g.via_prec, m.via_prec, sizeof g.via_prec);
    // the handle's stall rule: the STALL builds of the same checks, the rule and its state as their second argument
    vfik::StallArgs sa{};
    const vfik::StallArgs* st = nullptr;
    if (h->stall_on) {
        sa.best = h->d_stall_best; sa.count = h->d_stall_count;
        sa.stalled = h->stall.stalled ? h->stall.stalled : h->d_stall_own;
        sa.patience = h->stall.patience; sa.stop = h->stall.stop;
        sa.eps_pos = h->stall.eps_pos; sa.eps_rot = h->stall.eps_rot; sa.eps_js = h->stall.eps_js;
        st = &sa;
    }
    if (m.script) {
        vfik::ScriptArgs s{};
        s.c = g;
        s.kind = static_cast<const int*>(m.x[vfik::X_KIND]);
        s.wayq = m.x[vfik::X_WAYQ];
        s.mixw = h->d_script_mixw;
        s.bridge = h->d_mixw_arm;
        s.bridge_u[0] = h->params.mix_w[4]; s.bridge_u[1] = h->params.mix_w[5]; s.bridge_u[2] = h->params.max_vel;
        std::memcpy(s.mix, m.mix, sizeof s.mix);
        std::memcpy(s.js_prec, m.js_prec, sizeof s.js_prec);
        std::memcpy(s.js_via_prec, m.js_via_prec, sizeof s.js_via_prec);
        const hipError_t es = vfik::launch_script(h->io_dtype, s, h->stream, st);
        return es != hipSuccess ? fail(VFIK_E_HIP, "script launch: %s", hipGetErrorString(es)) : (int)VFIK_OK;
    }
    hipError_t e = vfik::launch_check(h->io_dtype, m.joint, m.list, g, h->stream, st);
    if (e != hipSuccess) {
        static const char* const name[2][2] = {{"arrive", "follow"}, {"arrive_js", "follow_js"}};
        return fail(VFIK_E_HIP, "%s launch: %s", name[m.joint][m.list], hipGetErrorString(e));
    }
    return VFIK_OK;
}

int timed_begin(vfik_handle* h, TimedMove& m) {
    const int rc = timed_reserve(h, m);
    return rc != VFIK_OK ? rc : timed_launch_check(h, m, -1, nullptr);
}

// The handle's coupling (vfik_set_coupling) in front of block k's cycles: the link spheres of every arm's source at the block's input row into
// the handle's rows, then the launch vfik_move_fields makes for them (move_launch: the tickets were drained when the move began).
int couple_block(vfik_handle* h, int k, const void* q_prev) {
    const int L = h->n_links, n_rep = h->couple.first_rep + L;
    char* const traj = static_cast<char*>(h->couple.link_traj);
    const int rc = link_launch(h, q_prev, h->couple.src_arm, h->couple.xform12, h->couple_rep.p,
                               traj ? traj + (size_t)k * h->B * L * 4 * h->esz : nullptr, n_rep, h->couple.first_rep);
    return rc != VFIK_OK ? rc : move_launch(h, 0, h->B, nullptr, h->couple_rep.p, n_rep, nullptr);
}

// The handle's wait rule (vfik_set_wait_rule) behind the coupling's two launches: every arm's clearance at the block's input row against the
// partner's rows as just placed, into row k of the rule's traces, and the gate of this block cleared for the arms that yield and lack room.
int wait_block(vfik_handle* h, int k, const void* q_prev) {
    const int L = h->n_links;
    vfik::ClearArgs a{};
    a.img = static_cast<const vfik::LinkImage*>(h->d_link_img);
    a.q = q_prev; a.pts4 = h->couple_rep.p;
    a.B = h->B; a.n_rep = h->couple.first_rep + L; a.first = h->couple.first_rep; a.count = L;
    std::memcpy(a.mask, h->wait_mask, sizeof a.mask);
    if (h->wait.clear_traj) a.clear = static_cast<char*>(h->wait.clear_traj) + (size_t)k * h->B * h->esz;
    if (h->wait.pair_traj) a.pair = h->wait.pair_traj + (size_t)k * h->B;
    a.gate = h->d_goto_gate; a.yields = h->wait.yields;
    a.waited = h->wait.waited ? h->wait.waited : h->d_wait_own;
    a.min_clearance = h->wait.min_clearance;
    a.first_block = k == 0;
    return clear_launch(h, a);
}

// The handle's avoid rule (vfik_set_avoid_rule) behind the coupling's launches and the wait rule's: every arm's push at the block's input row
// away from the partner's rows as just placed, into the rule's ext channel -- where the block's cycles read it -- and row k of its trace.
int avoid_block(vfik_handle* h, int k, const void* q_prev) {
    const int L = h->n_links;
    vfik::AvoidArgs a{};
    a.img = static_cast<const vfik::LinkImage*>(h->d_link_img);
    a.q = q_prev; a.pts4 = h->couple_rep.p; a.scale = h->avoid.scale;
    a.B = h->B; a.n_rep = h->couple.first_rep + L; a.first = h->couple.first_rep; a.count = L;
    a.gain = h->avoid.gain; a.d0 = h->avoid.d0;
    std::memcpy(a.mask, h->avoid_mask, sizeof a.mask);
    a.chan_out = ext_chan(h, h->avoid.channel);
    if (h->avoid.avoid_traj) a.traj = static_cast<char*>(h->avoid.avoid_traj) + (size_t)k * ext_chan_bytes(h);
    return avoid_launch(h, a);
}

// block k -- `stride` cycles through launch_cycles, as vfik_rollout runs them -- and its check
int timed_block(vfik_handle* h, const TimedMove& m, int k) {
    const vfik::BlockRows w = vfik::block_rows(m, timed_dims(h, m), k, h->d_gotoq, h->d_goto_dist);
    vfik_io b = *m.io;
    b.q = w.q_prev;
    b.goal_dist = w.dist;
    if ((m.joint && m.list) || m.script) b.q_ref = h->d_js_ref;
    b.active = m.gated ? h->d_goto_gate : nullptr;   // (the gate is all ones from start to end: the launch without one stores the same rows)
    if (h->couple_on) {
        int rl = couple_block(h, k, w.q_prev);
        if (rl == VFIK_OK && h->wait_on) rl = wait_block(h, k, w.q_prev);
        if (rl == VFIK_OK && h->avoid_on) rl = avoid_block(h, k, w.q_prev);
        if (rl != VFIK_OK) return rl;
    }
    const int rc = launch_cycles(h, &b, m.stride, m.dt, m.clamp, w.q_now, h->stream, k > 0, m.script ? h->d_script_mixw : nullptr);
    return rc != VFIK_OK ? rc : timed_launch_check(h, m, k, &w);
}

// q_out: the row the last executed block wrote; io->goal_dist beside a trace: the trace's last row
int timed_end(vfik_handle* h, const TimedMove& m, int checks_run) {
    if (checks_run < 1) return VFIK_OK;
    // (a velocity push must not outlive the move: the avoid rule's channel back to zero, behind the last block on the stream)
    if (h->avoid_on && h->couple_on) HIP_TRY(hipMemsetAsync(ext_chan(h, h->avoid.channel), 0, ext_chan_bytes(h), h->stream));
    const vfik::TimedDims d = timed_dims(h, m);
    const vfik::BlockRows w = vfik::block_rows(m, d, checks_run - 1, h->d_gotoq, h->d_goto_dist);
    if (m.x[vfik::X_Q_OUT]) HIP_TRY(hipMemcpyAsync(m.x[vfik::X_Q_OUT], w.q_now, vfik::extra_bytes(vfik::X_Q_OUT, d, 1), hipMemcpyDeviceToDevice, h->stream));
    if (m.x[vfik::X_DIST_TRAJ] && m.io->goal_dist)
        HIP_TRY(hipMemcpyAsync(m.io->goal_dist, w.dist, vfik::extra_bytes(vfik::X_DIST_TRAJ, d, 1), hipMemcpyDeviceToDevice, h->stream));
    return VFIK_OK;
}

// the device-pointer forms, after their check
int timed_run(vfik_handle* h, TimedMove& m) {
    if (drain_side_streams(h) != VFIK_OK) return VFIK_E_HIP;
    HIP_TRY(hipSetDevice(h->device));
    int rc = timed_begin(h, m);
    for (int k = 0; rc == VFIK_OK && k < m.n_checks; ++k) rc = timed_block(h, m, k);
    return rc != VFIK_OK ? rc : timed_end(h, m, m.n_checks);
}

// an arm whose list has no item (NaN in the first element of its first row, of row_len elements) is kept out like a gated one
bool any_arm_kept_out(const vfik_handle* h, const void* way, size_t row_len) {
    for (size_t b = 0; b < (size_t)h->B; ++b)
        if (h->esz == 4 ? std::isnan(static_cast<const float*>(way)[b * row_len]) : std::isnan(static_cast<const double*>(way)[b * row_len])) return true;
    return false;
}

// the early exit of the host forms: pending[done - 1] read back after every poll_checks checks
int poll_pending(vfik_handle* h, const TimedMove& m, int done, int32_t* left) {
    HIP_TRY(hipMemcpyAsync(left, static_cast<int32_t*>(m.x[vfik::X_PENDING]) + (done - 1), sizeof *left, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return VFIK_OK;
}

// a script's arm whose first step is of no kind has no script: kept out in the same way
bool any_arm_without_script(const vfik_handle* h, const int32_t* kind, size_t W) {
    for (size_t b = 0; b < (size_t)h->B; ++b)
        if (kind[b * W] != VFIK_STEP_FRAME && kind[b * W] != VFIK_STEP_POSTURE) return true;
    return false;
}

// The host-pointer forms, after their check: every member of io and of the options in ONE device buffer of the handle (grown on demand, members
// 256-byte aligned), copied in before the first block and out after the last one executed.  A list is copied in with the inputs (way16's
// alignment rule holds for the caller's array too, although the kernel reads the staged copy).  Under a gate the caller's rows of the gated
// outputs go in before the blocks (vfik_io_layout.h: IO_EXTRAS).
int timed_run_host(vfik_handle* h, TimedMove& m, int poll_checks, int* checks_run) {
    if (poll_checks < 0) return fail(VFIK_E_ARG, "poll_checks %d: 0 (never) or a positive count of checks", poll_checks);
    if (drain_side_streams(h) != VFIK_OK) return VFIK_E_HIP;
    HIP_TRY(hipSetDevice(h->device));
    const vfik::TimedDims d = timed_dims(h, m);
    IoStaging st(*m.io, h->B, h->io_dims());
    vfik::timed_stage(st, m, d);
    st.layout();
    if (reserve(h, h->goto_stage, st.total, true, true)) return VFIK_E_HIP;
    st.map(h->goto_stage.p);
    int rc = copy_members(st, IoStaging::INPUTS, h->stream);
    if (rc != VFIK_OK) return rc;
    const bool kept_out = m.io->active || h->wait_on || (m.script ? any_arm_without_script(h, static_cast<const int32_t*>(m.x[vfik::X_KIND]), d.W)
                                                    : m.list && any_arm_kept_out(h, m.x[m.joint ? vfik::X_WAYQ : vfik::X_WAY16], d.W * (m.joint ? d.n : 16)));
    if (kept_out && (rc = copy_members(st, IoStaging::GATED_OUTPUTS, h->stream)) != VFIK_OK) return rc;
    if (m.script && !kept_out) {   // an arm that meets no posture step keeps its diff row, under no gate at all
        const IoStaging::Member& df = st.extra(vfik::X_DIFF);
        if (df.present && df.host) HIP_TRY(hipMemcpyAsync(df.dev, df.host, df.bytes, hipMemcpyHostToDevice, h->stream));
    }
    const vfik_io dev_io = st.device_io();
    m.io = &dev_io;
    vfik::timed_rewire(st, m);
    if ((rc = timed_begin(h, m)) != VFIK_OK) return rc;
    int done = 0;
    while (done < m.n_checks) {
        if ((rc = timed_block(h, m, done)) != VFIK_OK) return rc;
        ++done;
        if (poll_checks > 0 && done % poll_checks == 0 && done < m.n_checks) {
            int32_t left = -1;
            if ((rc = poll_pending(h, m, done, &left)) != VFIK_OK) return rc;
            if (left == 0) break;   // every arm that takes part and the caller lets run is there, or at its last item
        }
    }
    if ((rc = timed_end(h, m, done)) != VFIK_OK) return rc;
    IoStaging back = st;   // what goes back: of pending and the traces the checks that ran (st keeps the sizes its layout was made of)
    vfik::timed_cut(back, d, done);
    if ((rc = copy_members(back, IoStaging::OUTPUTS, h->stream)) != VFIK_OK) return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (checks_run) *checks_run = done;
    return VFIK_OK;
}
}  // namespace

int vfik_goto(vfik_handle* h, const vfik_io* io, const vfik_goto_opts* o) {
    TimedMove m;
    const int rc = goto_check(h, io, o, m);
    return rc != VFIK_OK ? rc : timed_run(h, m);
}
int vfik_goto_host(vfik_handle* h, const vfik_io* io, const vfik_goto_opts* o, int poll_checks, int* checks_run) {
    TimedMove m;
    const int rc = goto_check(h, io, o, m);
    return rc != VFIK_OK ? rc : timed_run_host(h, m, poll_checks, checks_run);
}
int vfik_follow(vfik_handle* h, const vfik_io* io, const vfik_follow_opts* o) {
    TimedMove m;
    const int rc = follow_check(h, io, o, m);
    return rc != VFIK_OK ? rc : timed_run(h, m);
}
int vfik_follow_host(vfik_handle* h, const vfik_io* io, const vfik_follow_opts* o, int poll_checks, int* checks_run) {
    TimedMove m;
    const int rc = follow_check(h, io, o, m);
    return rc != VFIK_OK ? rc : timed_run_host(h, m, poll_checks, checks_run);
}
int vfik_goto_js(vfik_handle* h, const vfik_io* io, const vfik_goto_js_opts* o) {
    TimedMove m;
    const int rc = goto_js_check(h, io, o, m);
    return rc != VFIK_OK ? rc : timed_run(h, m);
}
int vfik_goto_js_host(vfik_handle* h, const vfik_io* io, const vfik_goto_js_opts* o, int poll_checks, int* checks_run) {
    TimedMove m;
    const int rc = goto_js_check(h, io, o, m);
    return rc != VFIK_OK ? rc : timed_run_host(h, m, poll_checks, checks_run);
}
int vfik_follow_js(vfik_handle* h, const vfik_io* io, const vfik_follow_js_opts* o) {
    TimedMove m;
    const int rc = follow_js_check(h, io, o, m);
    return rc != VFIK_OK ? rc : timed_run(h, m);
}
int vfik_follow_js_host(vfik_handle* h, const vfik_io* io, const vfik_follow_js_opts* o, int poll_checks, int* checks_run) {
    TimedMove m;
    const int rc = follow_js_check(h, io, o, m);
    return rc != VFIK_OK ? rc : timed_run_host(h, m, poll_checks, checks_run);
}
int vfik_script(vfik_handle* h, const vfik_io* io, const vfik_script_opts* o) {
    TimedMove m;
    const int rc = script_check(h, io, o, m);
    return rc != VFIK_OK ? rc : timed_run(h, m);
}
int vfik_script_host(vfik_handle* h, const vfik_io* io, const vfik_script_opts* o, int poll_checks, int* checks_run) {
    TimedMove m;
    const int rc = script_check(h, io, o, m);
    return rc != VFIK_OK ? rc : timed_run_host(h, m, poll_checks, checks_run);
}

// ---- the stall rule of the timed moves: state of the handle that their checks alone read (timed_launch_check) ----
size_t vfik_stall_rule_size(void) { return sizeof(vfik_stall_rule); }

int vfik_set_stall_rule(vfik_handle* h, const vfik_stall_rule* r) {
    if (check_handle(h)) return VFIK_E_ARG;
    if (!r) { h->stall_on = false; return VFIK_OK; }
    if (r->patience < 1) return fail(VFIK_E_ARG, "stall rule: patience %d, at least one check without progress", r->patience);
    if (r->stop != 0 && r->stop != 1) return fail(VFIK_E_ARG, "stall rule: stop %d is neither 0 nor 1", r->stop);
    if (!std::isfinite(r->eps_pos) || !std::isfinite(r->eps_rot) || !std::isfinite(r->eps_js) || r->eps_pos < 0.0 || r->eps_rot < 0.0 || r->eps_js < 0.0)
        return fail(VFIK_E_ARG, "stall rule: eps (%g m, %g rad, joints %g) must be finite and not negative", r->eps_pos, r->eps_rot, r->eps_js);
    if (r->stalled && (!gpu_visible(r->stalled) || reinterpret_cast<uintptr_t>(r->stalled) % sizeof(int32_t)))
        return fail(VFIK_E_ARG, "stall rule: stalled must be an int32-aligned DEVICE pointer (NULL: the handle's own array)");
    HIP_TRY(hipSetDevice(h->device));
    if (refuse_capture(h->stream, "vfik_set_stall_rule allocates the handle's stall state: call it before capturing the stream")) return VFIK_E_STATE;
    if (drain_side_streams(h) != VFIK_OK) return VFIK_E_HIP;
    const size_t B = (size_t)h->B;
    if (!h->d_stall_best && dev_alloc(h, (void**)&h->d_stall_best, B * 2 * sizeof(double), true)) return VFIK_E_HIP;
    if (!h->d_stall_count && dev_alloc(h, (void**)&h->d_stall_count, B * sizeof(int32_t), true)) return VFIK_E_HIP;
    if (!h->d_stall_own) {   // (-1 in every byte: no arm stalled before the first timed move)
        if (dev_alloc(h, (void**)&h->d_stall_own, B * sizeof(int32_t), false)) return VFIK_E_HIP;
        HIP_TRY(hipMemsetAsync(h->d_stall_own, 0xFF, B * sizeof(int32_t), h->stream));
    }
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->stall = *r;
    h->stall_on = true;
    return VFIK_OK;
}

int vfik_stalled_host(vfik_handle* h, int32_t* out) {
    if (check_handle(h)) return VFIK_E_ARG;
    if (!out) return fail(VFIK_E_ARG, "vfik_stalled_host: out[B] is required");
    if (!h->stall_on) return fail(VFIK_E_STATE, "vfik_stalled_host: the handle has no stall rule (vfik_set_stall_rule)");
    HIP_TRY(hipSetDevice(h->device));
    if (refuse_capture(h->stream, "vfik_stalled_host copies to the host and synchronises: not while the stream is being captured")) return VFIK_E_STATE;
    HIP_TRY(hipMemcpyAsync(out, h->stall.stalled ? h->stall.stalled : h->d_stall_own, (size_t)h->B * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return VFIK_OK;
}

// ---- pipelined host path -------------------------------------------------------------------------
void* vfik_host_alloc(vfik_handle* h, size_t bytes) {
    if (!h || bytes == 0) { fail(VFIK_E_ARG, "vfik_host_alloc: bad arguments"); return nullptr; }
    void* p = nullptr;
    if (hipSetDevice(h->device) != hipSuccess || hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) {
        fail(VFIK_E_HIP, "hipHostMalloc(%zu) failed", bytes);
        return nullptr;
    }
    return p;
}

int vfik_host_free(vfik_handle* h, void* p) {
    if (check_handle(h)) return VFIK_E_ARG;
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipHostFree(p));
    return VFIK_OK;
}

int vfik_wait(vfik_handle* h, long ticket) {
    if (check_handle(h)) return VFIK_E_ARG;
    if (ticket < 0 || ticket >= h->next_ticket) return fail(VFIK_E_ARG, "vfik_wait: unknown ticket %ld", ticket);
    auto& ps = h->pipe[ticket % vfik_handle::PIPE];
    if (ps.ticket != ticket) return VFIK_OK;  // already waited for (or its slot was recycled, which waits)
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipEventSynchronize(ps.ev_out));
    ps.ticket = -1;
    return VFIK_OK;
}

int vfik_submit_host(vfik_handle* h, const vfik_io* io, long* ticket) {
    if (check_handle(h)) return VFIK_E_ARG;
    if (!io || !io->q || !ticket) return fail(VFIK_E_ARG, "vfik_submit_host needs io->q and a ticket");
    if (!h->chain_set) return fail(VFIK_E_STATE, "vfik_set_chain has not been called");
    HIP_TRY(hipSetDevice(h->device));
    if (!h->s_in) {  // non-blocking: no implicit ordering against the NULL stream a caller may have chosen
        HIP_TRY(hipStreamCreateWithFlags(&h->s_in, hipStreamNonBlocking));
        HIP_TRY(hipStreamCreateWithFlags(&h->s_out, hipStreamNonBlocking));
    }
    auto& ps = h->pipe[h->next_ticket % vfik_handle::PIPE];
    if (!ps.ev_in) {
        HIP_TRY(hipEventCreateWithFlags(&ps.ev_in, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&ps.ev_k, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&ps.ev_out, hipEventDisableTiming));
    }
    if (ps.ticket >= 0) {  // the slot's previous submission must have left the device before its buffers are reused
        HIP_TRY(hipEventSynchronize(ps.ev_out));
        ps.ticket = -1;
    }
    IoStaging st(*io, h->B, h->io_dims());
    // Zero-copy: when every buffer is pinned (device-visible) host memory the kernel writes qdot across
    // PCIe itself, and reads q the same way when nothing else is in flight (lowest latency: 83 us per C3
    // step, 1.8 MB each way).  While an earlier submission is still running, the inputs go through the
    // copy engine instead, which overlaps that kernel: 56 us per step at 2-3 in flight, against 66 us for
    // reads by the kernel and 95 us for the three-stream staging below.
    bool direct = true;
    for (const IoStaging::Member& m : st.m) direct = direct && (!m.present || gpu_visible(m.host));
    if (direct) {
        bool busy = false;
        for (auto& o : h->pipe)
            if (o.ticket >= 0 && hipEventQuery(o.ev_out) == hipErrorNotReady) busy = true;
        (void)hipGetLastError();
        vfik_io d = *io;
        if (busy) {   // the inputs alone are staged; the outputs stay the caller's pinned arrays
            int rc = map_buffers(h, st, ps.sc, true, "staging");
            if (rc == VFIK_OK) rc = copy_members(st, IoStaging::INPUTS, h->s_in);
            if (rc != VFIK_OK) return rc;
            d = st.device_io(io);
            HIP_TRY(hipEventRecord(ps.ev_in, h->s_in));
            HIP_TRY(hipStreamWaitEvent(h->stream, ps.ev_in, 0));
        }
        const int rc = launch_cycles(h, &d, 0, 0.0, 0, nullptr, h->stream);
        if (rc != VFIK_OK) return rc;
        HIP_TRY(hipEventRecord(ps.ev_out, h->stream));
        ps.ticket = h->next_ticket;
        *ticket = h->next_ticket++;
        return VFIK_OK;
    }
    int rc = map_buffers(h, st, ps.sc, false, "staging");
    if (rc == VFIK_OK) rc = copy_members(st, IoStaging::INPUTS, h->s_in);
    if (rc == VFIK_OK && io->active) rc = copy_members(st, IoStaging::GATED_OUTPUTS, h->s_in);
    if (rc != VFIK_OK) return rc;
    HIP_TRY(hipEventRecord(ps.ev_in, h->s_in));
    HIP_TRY(hipStreamWaitEvent(h->stream, ps.ev_in, 0));
    const vfik_io d = st.device_io();
    if ((rc = vfik_step(h, &d)) != VFIK_OK) return rc;
    HIP_TRY(hipEventRecord(ps.ev_k, h->stream));
    HIP_TRY(hipStreamWaitEvent(h->s_out, ps.ev_k, 0));
    if ((rc = copy_members(st, IoStaging::OUTPUTS, h->s_out)) != VFIK_OK) return rc;
    HIP_TRY(hipEventRecord(ps.ev_out, h->s_out));
    ps.ticket = h->next_ticket;
    *ticket = h->next_ticket++;
    return VFIK_OK;
}

int vfik_track_reset(vfik_handle* h) {
    if (check_handle(h)) return VFIK_E_ARG;
    HIP_TRY(hipSetDevice(h->device));
    if (h->d_track) HIP_TRY(hipMemsetAsync(h->d_track, 0, (size_t)38 * h->B * sizeof(double), h->stream));
    return VFIK_OK;
}

int vfik_track_error(vfik_handle* h, const void* pose, const void* v6, void* out, const int32_t* active) {
    if (check_handle(h)) return VFIK_E_ARG;
    if (!pose || !v6 || !out) return fail(VFIK_E_ARG, "vfik_track_error: pose, v6 and out are required");
    HIP_TRY(hipSetDevice(h->device));
    if (!h->d_track && dev_alloc(h, (void**)&h->d_track, (size_t)38 * h->B * sizeof(double), true)) return VFIK_E_HIP;
    hipError_t e = vfik::launch_track(h->io_dtype, pose, v6, h->d_track, out, active, h->B, h->stream);
    if (e != hipSuccess) return fail(VFIK_E_HIP, "track launch: %s", hipGetErrorString(e));
    return VFIK_OK;
}

int vfik_probe_field(vfik_handle* h, const void* pose, void* v6) {
    if (check_handle(h)) return VFIK_E_ARG;
    if (!pose || !v6) return fail(VFIK_E_ARG, "vfik_probe_field: pose and v6 are required");
    HIP_TRY(hipSetDevice(h->device));
    const double rs = h->params.rot_slowdown;
    hipError_t e = vfik::launch_probe(h->io_dtype, pose, h->d_goal, h->d_slots, h->B, h->Bpad, h->scene.slots_used, rs, vfik::cos_slow_of(rs), v6, h->stream);
    if (e != hipSuccess) return fail(VFIK_E_HIP, "probe launch: %s", hipGetErrorString(e));
    return VFIK_OK;
}

int vfik_object_distances(vfik_handle* h, const void* pose, const void* frames, int max_objects, void* out) {
    if (check_handle(h)) return VFIK_E_ARG;
    if (!pose || !frames || !out) return fail(VFIK_E_ARG, "vfik_object_distances: pose, frames and out are required");
    if (max_objects < 1 || max_objects > 4096) return fail(VFIK_E_ARG, "max_objects %d outside [1, 4096]", max_objects);
    HIP_TRY(hipSetDevice(h->device));
    hipError_t e = vfik::launch_monitor(h->io_dtype, pose, frames, max_objects, (long)h->B * max_objects, out, h->stream);
    if (e != hipSuccess) return fail(VFIK_E_HIP, "monitor launch: %s", hipGetErrorString(e));
    return VFIK_OK;
}

int vfik_set_objects(vfik_handle* h, int first_arm, int n_arms, const double* frames, int n_objects) {
    if (check_handle(h)) return VFIK_E_ARG;
    if (quiesce(h) != VFIK_OK) return VFIK_E_HIP;
    if (!frames) return fail(VFIK_E_ARG, "null frames");
    if (n_objects < 1 || n_objects > 4096) return fail(VFIK_E_ARG, "n_objects %d outside [1, 4096]", n_objects);
    if (check_arms(h, first_arm, n_arms)) return VFIK_E_ARG;
    if (n_objects != h->n_objects && (first_arm != 0 || n_arms != h->B))
        return fail(VFIK_E_ARG, "n_objects changes from %d to %d: the call must cover every arm", h->n_objects, n_objects);
    const size_t count = (size_t)n_arms * n_objects * 16;
    for (size_t k = 0; k < count; ++k)
        if (!std::isfinite(frames[k])) return fail(VFIK_E_ARG, "object frame entry %zu is not finite", k);
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (n_objects != h->n_objects) {
        if (h->d_objects) { (void)hipFree(h->d_objects); h->d_objects = nullptr; h->n_objects = 0; }
        if (dev_alloc(h, &h->d_objects, (size_t)h->B * n_objects * 16 * h->esz, true)) return VFIK_E_HIP;
        h->n_objects = n_objects;
    }
    std::vector<char> buf(count * h->esz);
    for (size_t k = 0; k < count; ++k) put_io(h, buf, k, frames[k]);
    char* dst = static_cast<char*>(h->d_objects) + (size_t)first_arm * n_objects * 16 * h->esz;
    HIP_TRY(hipMemcpyAsync(dst, buf.data(), buf.size(), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return VFIK_OK;
}

int vfik_mix(vfik_handle* h, const void* cmds, const double* weights, int K, void* out) {
    if (check_handle(h)) return VFIK_E_ARG;
    if (!cmds || !weights || !out || K < 1 || K > 16) return fail(VFIK_E_ARG, "vfik_mix: bad arguments (K=%d)", K);
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipMemcpyAsync(h->d_mixw, weights, K * sizeof(double), hipMemcpyHostToDevice, h->stream));
    const long count = (long)h->B * h->n;
    hipError_t e = vfik::launch_mix(h->io_dtype, cmds, h->d_mixw, K, count, count, out, h->stream);
    if (e != hipSuccess) return fail(VFIK_E_HIP, "mix launch: %s", hipGetErrorString(e));
    return VFIK_OK;
}

void* vfik_dev_alloc(vfik_handle* h, size_t bytes) {
    if (!h || bytes == 0) { fail(VFIK_E_ARG, "vfik_dev_alloc: bad arguments"); return nullptr; }
    void* p = nullptr;
    if (hipSetDevice(h->device) != hipSuccess || hipMalloc(&p, bytes) != hipSuccess) { fail(VFIK_E_HIP, "hipMalloc(%zu) failed", bytes); return nullptr; }
    return p;
}

int vfik_dev_free(vfik_handle* h, void* p) {
    if (check_handle(h)) return VFIK_E_ARG;
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipFree(p));
    return VFIK_OK;
}

int vfik_memcpy_h2d(vfik_handle* h, void* dst, const void* src, size_t bytes) {
    if (check_handle(h)) return VFIK_E_ARG;
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return VFIK_OK;
}

int vfik_memcpy_d2h(vfik_handle* h, void* dst, const void* src, size_t bytes) {
    if (check_handle(h)) return VFIK_E_ARG;
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return VFIK_OK;
}

int vfik_time_steps(vfik_handle* h, const vfik_io* io, int warmup, int steps, float* ms_total) {
    if (check_handle(h)) return VFIK_E_ARG;
    if (!ms_total || steps < 1 || warmup < 0) return fail(VFIK_E_ARG, "vfik_time_steps: bad arguments");
    HIP_TRY(hipSetDevice(h->device));
    for (int i = 0; i < warmup; ++i) {
        int rc = vfik_step(h, io);
        if (rc != VFIK_OK) return rc;
    }
    hipEvent_t t0, t1;
    HIP_TRY(hipEventCreate(&t0));
    HIP_TRY(hipEventCreate(&t1));
    HIP_TRY(hipEventRecord(t0, h->stream));
    for (int i = 0; i < steps; ++i) {
        int rc = vfik_step(h, io);
        if (rc != VFIK_OK) { (void)hipEventDestroy(t0); (void)hipEventDestroy(t1); return rc; }
    }
    HIP_TRY(hipEventRecord(t1, h->stream));
    HIP_TRY(hipEventSynchronize(t1));
    HIP_TRY(hipEventElapsedTime(ms_total, t0, t1));
    (void)hipEventDestroy(t0);
    (void)hipEventDestroy(t1);
    return VFIK_OK;
}

#ifdef VFIK_STAMPS
// diagnostic build: copy the per-wave section stamps ([waves][8]) to the host
int vfik_debug_read_stamps(vfik_handle* h, unsigned long long* dst) {
    if (check_handle(h)) return VFIK_E_ARG;
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipMemcpy(dst, h->d_stamps, (size_t)((h->B + 63) / 64) * 10 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return VFIK_OK;
}
#endif

int vfik_slots_in_use(vfik_handle* h) { return h ? h->scene.slots_used : VFIK_E_ARG; }

int vfik_field_path(vfik_handle* h) { return h ? h->scene.field_path() : VFIK_E_ARG; }

long vfik_launch_epoch(vfik_handle* h) { return h ? h->epoch : (long)VFIK_E_ARG; }

int vfik_dh_pattern(vfik_handle* h) { return h ? ((h->plain && !h->tool_per_arm && !h->d_wts) ? h->dhp : 0) : VFIK_E_ARG; }

int vfik_mixed_orders(vfik_handle* h) { return h ? h->scene.mixed_orders() : VFIK_E_ARG; }

int vfik_uniform_repellers(vfik_handle* h) { return h ? h->scene.uniform(h->knobs) : VFIK_E_ARG; }

int vfik_one_chunk(vfik_handle* h) { return h ? h->scene.one_chunk() : VFIK_E_ARG; }

int vfik_set_small_batch_kernel(vfik_handle* h, int max_batch) {
    if (check_handle(h)) return VFIK_E_ARG;
    if (max_batch < 0) return fail(VFIK_E_ARG, "max_batch must be >= 0");
    ++h->epoch;
    h->sub8_max_batch = max_batch;
    h->sub8_max_batch_full = max_batch;
    h->sub8_max_batch_ns = max_batch;
    return VFIK_OK;
}

long vfik_small_batch_launches(vfik_handle* h) { return h ? h->sub8_launches : -1; }

int vfik_launched_kernels(vfik_handle* h, char* buf, int len) {
    if (check_handle(h)) return VFIK_E_ARG;
    if (h->launched_lost) return fail(VFIK_E_STATE, "more than %d distinct cycle kernels launched since the last vfik_launched_kernels", vfik_handle::LAUNCHED_MAX);
    std::string all;
    for (int i = 0; i < h->launched_n; ++i) {
        all += vfik::cycle_kernel_name(h->launched[i].p, h->n, h->io_dtype, h->launched[i].ns);
        all += '\n';
    }
    if (!buf) return (int)all.size();
    if (len < (int)all.size() + 1) return fail(VFIK_E_ARG, "vfik_launched_kernels: %d bytes needed", (int)all.size() + 1);
    std::memcpy(buf, all.c_str(), all.size() + 1);
    h->launched_n = 0;
    return (int)all.size();
}

size_t vfik_device_bytes(vfik_handle* h) { return h ? h->dev_bytes : 0; }

}  // extern "C"
