// vfik_io_layout.h -- the ONE description of vfik_io for the host-pointer call forms (vfik_step_host, vfik_rollout_host, vfik_goto_host,
// vfik_follow_host, vfik_goto_js_host, vfik_follow_js_host, vfik_script_host, vfik_submit_host): which member is an input, how many bytes it has, and where it lies in a staging buffer.  Pure arithmetic, no HIP:
// vfik_abi.cpp does the copies, tests/c_host/io_layout.cpp checks the layout on the CPU.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>

#include "../../include/vfik.h"

namespace vfik {

struct IoDims { size_t n, esz, n_objects; };   // joints, bytes of an element of the I/O type, object frames of vfik_set_objects

// bytes of ONE arm's row
inline size_t row_joints(const IoDims& d) { return d.n * d.esz; }
inline size_t row_4(const IoDims& d) { return VFIK_NULL_CONTROLS * d.esz; }
inline size_t row_16(const IoDims& d) { return 16 * d.esz; }
inline size_t row_6(const IoDims& d) { return 6 * d.esz; }
inline size_t row_2(const IoDims& d) { return 2 * d.esz; }
inline size_t row_8(const IoDims& d) { return 8 * d.esz; }
inline size_t row_i32(const IoDims&) { return sizeof(int32_t); }
inline size_t row_objects(const IoDims& d) { return (d.n_objects > 0 ? d.n_objects : 1) * 2 * d.esz; }   // (sized before any vfik_set_objects too)

constexpr size_t IO_ALWAYS = ~(size_t)0;
struct IoMember {
    size_t field;                         // offsetof(vfik_io, member): every member is one pointer
    bool input;
    size_t (*row_bytes)(const IoDims&);
    size_t only_with;                     // staged only when this other member is given (IO_ALWAYS: whenever the caller gives it)
};

// A member of include/vfik.h's vfik_io is staged by the host forms once it has its entry here (and its field in vfclik_amd/engine.py's IO).
// Inputs first: they are one contiguous prefix of a staging buffer.
#define VFIK_IO_FIELD(m) offsetof(vfik_io, m)
constexpr IoMember IO_MEMBERS[] = {
    {VFIK_IO_FIELD(q), true, row_joints, IO_ALWAYS},
    {VFIK_IO_FIELD(null_control), true, row_4, IO_ALWAYS},
    {VFIK_IO_FIELD(q_ref), true, row_joints, IO_ALWAYS},
    {VFIK_IO_FIELD(q_cmded), true, row_joints, IO_ALWAYS},
    {VFIK_IO_FIELD(active), true, row_i32, IO_ALWAYS},
    {VFIK_IO_FIELD(q_lo), true, row_joints, IO_ALWAYS},
    {VFIK_IO_FIELD(q_hi), true, row_joints, IO_ALWAYS},
    {VFIK_IO_FIELD(qdot_vf), false, row_joints, IO_ALWAYS},
    {VFIK_IO_FIELD(qdot_null), false, row_joints, IO_ALWAYS},
    {VFIK_IO_FIELD(qdot_out), false, row_joints, IO_ALWAYS},
    {VFIK_IO_FIELD(pose), false, row_16, IO_ALWAYS},
    {VFIK_IO_FIELD(pose_nt), false, row_16, IO_ALWAYS},
    {VFIK_IO_FIELD(v6), false, row_6, IO_ALWAYS},
    {VFIK_IO_FIELD(qdist), false, row_joints, IO_ALWAYS},
    {VFIK_IO_FIELD(status), false, row_i32, IO_ALWAYS},
    {VFIK_IO_FIELD(goal_dist), false, row_2, IO_ALWAYS},
    {VFIK_IO_FIELD(q_ref_out), false, row_joints, VFIK_IO_FIELD(q_ref)},   // the kernel writes it only with a joint controller (fill_kargs)
    {VFIK_IO_FIELD(track_error), false, row_8, IO_ALWAYS},
    {VFIK_IO_FIELD(obj_dist), false, row_objects, IO_ALWAYS},
};
#undef VFIK_IO_FIELD
constexpr int N_IO = sizeof IO_MEMBERS / sizeof IO_MEMBERS[0];
static_assert(N_IO * sizeof(void*) == sizeof(vfik_io), "vfik_io has a member without an entry in IO_MEMBERS (or one that is no pointer)");
constexpr bool io_inputs_first() {
    for (int i = 1; i < N_IO; ++i)
        if (IO_MEMBERS[i].input && !IO_MEMBERS[i - 1].input) return false;
    return true;
}
static_assert(io_inputs_first(), "IO_MEMBERS: the inputs come first");

// what a call form stages beside vfik_io's members, behind io's: outputs, but for way16 and wayq -- inputs that a form copies in with the
// inputs of io, outside their contiguous prefix (in_bytes)
enum IoExtra {
    X_Q_OUT,       // [B][n]            vfik_rollout_host's and vfik_goto_host's q_out
    X_ARRIVED,     // [B] int32         the rest: vfik_goto_opts
    X_PENDING,     // [n_checks] int32
    X_Q_TRAJ,      // [n_checks][B][n]
    X_DIST_TRAJ,   // [n_checks][B][2]
    X_WAY16,       // [B][W][16]        input; the rest: vfik_follow_opts
    X_REACHED,     // [B][W] int32
    X_NEXT,        // [B] int32
    X_WAY_TRAJ,    // [n_checks][B] int32
    X_DIFF,        // [B][n]            vfik_goto_js_opts' and vfik_follow_js_opts' diff
    X_WAYQ,        // [B][W][n]         input, as X_WAY16: vfik_follow_js_opts
    X_KIND,        // [B][W] int32      input: vfik_script_opts' kind -- a script stages way16, wayq and kind
    N_IO_EXTRA
};
constexpr int N_STAGED = N_IO + N_IO_EXTRA;

inline void* io_get(const vfik_io& io, size_t field) {
    void* p;
    std::memcpy(&p, reinterpret_cast<const char*>(&io) + field, sizeof p);
    return p;
}
inline void io_set(vfik_io& io, size_t field, void* p) { std::memcpy(reinterpret_cast<char*>(&io) + field, &p, sizeof p); }

// One call's members: where the caller has them (host), where the kernels see them (dev), and their place in a staging buffer.
struct IoStaging {
    struct Member {
        void* host = nullptr;     // the caller's array (inputs are only read); NULL with `present`: staged, copied nowhere
        void* dev = nullptr;
        size_t bytes = 0, off = 0;
        bool present = false, input = false;
        bool gated = false;       // an output that arms can leave unwritten under the gate: the caller's rows go in before the launch
    };
    enum Which { INPUTS, GATED_OUTPUTS, OUTPUTS };
    static constexpr size_t ALIGN = 256;

    Member m[N_STAGED];
    size_t in_bytes = 0, total = 0;   // the input prefix; all of it
    int members = 0;

    // io's members as the caller gave them; layout() once the extras are in
    IoStaging(const vfik_io& io, size_t B, const IoDims& d) {
        for (int i = 0; i < N_IO; ++i) {
            const IoMember& t = IO_MEMBERS[i];
            Member& x = m[i];
            x.host = io_get(io, t.field);
            if (t.only_with != IO_ALWAYS && !io_get(io, t.only_with)) x.host = nullptr;
            x.present = x.host != nullptr;
            x.input = t.input;
            x.gated = !t.input;
            x.bytes = B * t.row_bytes(d);
        }
    }
    // always: staged without an array of the caller's, too
    void add(IoExtra which, void* host, size_t bytes, bool gated, bool always = false, bool input = false) {
        Member& x = m[N_IO + which];
        x.host = host;
        x.present = host != nullptr || always;
        x.bytes = bytes;
        x.gated = gated;
        x.input = input;
    }
    Member& extra(IoExtra which) { return m[N_IO + which]; }

    // every present member at the next multiple of ALIGN, in order: io's inputs are a prefix, absent members take no room
    void layout() {
        auto up = [](size_t b) { return (b + ALIGN - 1) & ~(ALIGN - 1); };
        total = in_bytes = 0;
        members = 0;
        for (Member& x : m) {
            x.off = total;
            if (!x.present) continue;
            total += up(x.bytes);
            if (x.input && &x < m + N_IO) in_bytes = total;
            ++members;
        }
    }
    // the members in one buffer, as layout() placed them
    void map(void* base) {
        for (Member& x : m) x.dev = x.present ? static_cast<char*>(base) + x.off : nullptr;
    }
    // what a launch on the staged members gets for the caller's io (the extras: extra(...).dev); outputs_from: only the inputs are staged,
    // the outputs stay where this io has them
    vfik_io device_io(const vfik_io* outputs_from = nullptr) const {
        vfik_io d = outputs_from ? *outputs_from : vfik_io{};
        for (int i = 0; i < N_IO; ++i)
            if (!outputs_from || m[i].input) io_set(d, IO_MEMBERS[i].field, m[i].dev);
        return d;
    }
    // f(Member&) -> 0 or an error that ends the walk: over the inputs, the outputs that go in under a gate, or all outputs that have
    // somewhere to go
    template <typename F>
    int each(Which w, F f) {
        for (Member& x : m) {
            if (!x.present || !x.host) continue;
            if (w == INPUTS ? !x.input : (x.input || (w == GATED_OUTPUTS && !x.gated))) continue;
            if (int rc = f(x)) return rc;
        }
        return 0;
    }
};

// ---- timed moves: vfik_goto, vfik_follow, vfik_goto_js, vfik_follow_js, vfik_script and their host forms ----
// ONE description of a move between its checks and its last block.  The forms differ on two axes: the rule is the Cartesian distance pair or
// the per-joint band (joint), the target one goal or a list with reached, next and len (list).  A script (vfik_script) is a Cartesian list
// (joint false, list true: its blocks' distance row, its traces) whose items are of either kind: `script` adds the joint rule's members.
struct TimedMove {
    const vfik_io* io;
    bool joint, list;
    int n_cycles, stride, clamp, hold, n_way, n_checks;
    double dt;
    void* x[N_IO_EXTRA];   // the options' arrays, each under its IoExtra (device pointers; NULL: not given, or not one of this form's)
    // joint: goal_precision per joint; Cartesian: [0] metres, [1] radians.  via_prec: a list's, at every item but an arm's last
    double prec[VFIK_MAX_JOINTS], via_prec[VFIK_MAX_JOINTS];
    bool gated;            // the blocks run under the handle's gate (hold, the caller gates, or a list -- an arm without one is kept out)
    // a script: prec / via_prec hold the Cartesian pair of its frame steps, these the rest
    bool script;
    double js_prec[VFIK_MAX_JOINTS], js_via_prec[VFIK_MAX_JOINTS];   // the per-joint band of its posture steps
    double mix[2][4];      // mixer weights of channels 0..3 while an arm is under way to a frame [0] or to a posture [1]
};

struct TimedDims { size_t B, n, esz, W, n_checks; };   // arms, joints, bytes of an I/O element, items per list, checks

// What the host forms do with each IoExtra (IO_EXTRAS[X] describes TimedMove::x[X]).  row: the bytes of the whole array, or of ONE check's row of
// a per-check trace -- which has n_checks of them and goes back cut to the checks that ran.  gated: an output that arms can leave unwritten
// under the gate; always: staged without an array of the caller's too; input: copied in with io's inputs.
struct IoExtraInfo {
    size_t (*row)(const TimedDims&);
    bool gated, always, input, per_check;
};
constexpr IoExtraInfo IO_EXTRAS[N_IO_EXTRA] = {
    /* X_Q_OUT     */ {[](const TimedDims& d) { return d.B * d.n * d.esz; }, false, false, false, false},   // written for every arm at the end
    /* X_ARRIVED   */ {[](const TimedDims& d) { return d.B * sizeof(int32_t); }, false, false, false, false},
    /* X_PENDING   */ {[](const TimedDims&) { return sizeof(int32_t); }, false, true, false, true},         // the early exit reads it
    /* X_Q_TRAJ    */ {[](const TimedDims& d) { return d.B * d.n * d.esz; }, false, false, false, true},    // a gated arm's rows repeat its start
    /* X_DIST_TRAJ */ {[](const TimedDims& d) { return d.B * 2 * d.esz; }, true, false, false, true},
    /* X_WAY16     */ {[](const TimedDims& d) { return d.B * d.W * 16 * d.esz; }, false, false, true, false},
    /* X_REACHED   */ {[](const TimedDims& d) { return d.B * d.W * sizeof(int32_t); }, false, false, false, false},   // reached and next: written
    /* X_NEXT      */ {[](const TimedDims& d) { return d.B * sizeof(int32_t); }, false, false, false, false},         // for every arm in front of block 0
    /* X_WAY_TRAJ  */ {[](const TimedDims& d) { return d.B * sizeof(int32_t); }, true, false, false, true},
    /* X_DIFF      */ {[](const TimedDims& d) { return d.B * d.n * d.esz; }, true, false, false, false},    // a gated arm keeps its row
    /* X_WAYQ      */ {[](const TimedDims& d) { return d.B * d.W * d.n * d.esz; }, false, false, true, false},
    /* X_KIND      */ {[](const TimedDims& d) { return d.B * d.W * sizeof(int32_t); }, false, false, true, false},
};
inline size_t extra_bytes(IoExtra x, const TimedDims& d, size_t checks) { return IO_EXTRAS[x].row(d) * (IO_EXTRAS[x].per_check ? checks : 1); }

// the extras a form stages, as bits 1 << IoExtra
constexpr unsigned timed_extras(bool joint, bool list) {
    return 1u << X_Q_OUT | 1u << X_PENDING | 1u << X_Q_TRAJ | 1u << (joint ? X_DIFF : X_DIST_TRAJ) |
           (list ? 1u << X_REACHED | 1u << X_NEXT | 1u << X_WAY_TRAJ | 1u << (joint ? X_WAYQ : X_WAY16) : 1u << X_ARRIVED);
}
// ... and a move's: a script stages a waypoint list's and, for its posture steps, diff, wayq and kind
constexpr unsigned timed_extras(const TimedMove& m) {
    return timed_extras(m.joint, m.list) | (m.script ? 1u << X_DIFF | 1u << X_WAYQ | 1u << X_KIND : 0u);
}

// The move's extras into a staging and its arrays rewired to their staged addresses (between the two: layout() and map()); the sizes of what
// goes back after `done` checks.
inline void timed_stage(IoStaging& st, const TimedMove& m, const TimedDims& d) {
    for (int x = 0; x < N_IO_EXTRA; ++x)
        if (timed_extras(m) >> x & 1)
            st.add((IoExtra)x, m.x[x], extra_bytes((IoExtra)x, d, d.n_checks), IO_EXTRAS[x].gated, IO_EXTRAS[x].always, IO_EXTRAS[x].input);
}
inline void timed_rewire(IoStaging& st, TimedMove& m) {
    for (int x = 0; x < N_IO_EXTRA; ++x) m.x[x] = st.extra((IoExtra)x).dev;
}
inline void timed_cut(IoStaging& back, const TimedDims& d, size_t done) {
    for (int x = 0; x < N_IO_EXTRA; ++x)
        if (IO_EXTRAS[x].per_check) back.extra((IoExtra)x).bytes = extra_bytes((IoExtra)x, d, done);
}

// the rows of block k: the q it reads and writes, its goal_dist, and the trace's rows in front of it (NULL: no trace, or k = 0)
struct BlockRows {
    const void* q_prev;
    void* q_now;
    void* dist;
    const void* dist_prev;
    int32_t* way_now;
    const int32_t* way_prev;
};
// q: the trace's rows, or the handle's pair by turns (pingpong); block 0 reads io->q.  dist: the trace's row, or io->goal_dist, or the handle's
// row (handle_dist) -- a joint form has no distance row: its blocks' goal_dist is the caller's business.
inline BlockRows block_rows(const TimedMove& m, const TimedDims& d, int k, void* const pingpong[2], void* handle_dist) {
    auto row = [&](IoExtra x, int i) { return m.x[x] && i >= 0 ? static_cast<char*>(m.x[x]) + (size_t)i * IO_EXTRAS[x].row(d) : nullptr; };
    auto q_row = [&](int i) { return m.x[X_Q_TRAJ] ? (void*)row(X_Q_TRAJ, i) : pingpong[i & 1]; };
    BlockRows w;
    w.q_prev = k == 0 ? m.io->q : q_row(k - 1);
    w.q_now = q_row(k);
    w.dist = m.x[X_DIST_TRAJ] ? row(X_DIST_TRAJ, k) : (m.io->goal_dist || m.joint ? m.io->goal_dist : handle_dist);
    w.dist_prev = row(X_DIST_TRAJ, k - 1);
    w.way_now = reinterpret_cast<int32_t*>(row(X_WAY_TRAJ, k));
    w.way_prev = reinterpret_cast<const int32_t*>(row(X_WAY_TRAJ, k - 1));
    return w;
}

}  // namespace vfik
