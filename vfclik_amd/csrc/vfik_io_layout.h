// vfik_io_layout.h -- the ONE description of vfik_io for the host-pointer call forms (vfik_step_host, vfik_rollout_host, vfik_goto_host,
// vfik_follow_host, vfik_goto_js_host, vfik_follow_js_host, vfik_submit_host): which member is an input, how many bytes it has, and where it lies in a staging buffer.  Pure arithmetic, no HIP:
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

}  // namespace vfik
