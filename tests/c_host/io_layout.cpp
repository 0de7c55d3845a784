// The staging layout of the host-pointer call forms (vfclik_amd/csrc/vfik_io_layout.h), checked on the CPU: no HIP, no library.
// And of the timed moves (vfik_goto, vfik_follow, vfik_goto_js, vfik_follow_js): the table of what their host forms stage and the rows of a block.
// tests/test_io_layout.py builds this with AddressSanitizer + UBSan and runs it as a process of its own.
#include <cstdio>
#include <vector>

#include "../../vfclik_amd/csrc/vfik_io_layout.h"

using vfik::IoStaging;

static int failures = 0;
#define CHECK(cond, ...)                                       \
    do {                                                       \
        if (!(cond)) {                                         \
            ++failures;                                        \
            std::printf("FAIL %s:%d  %s  ", __FILE__, __LINE__, #cond); \
            std::printf(__VA_ARGS__);                          \
            std::printf("\n");                                 \
        }                                                      \
    } while (0)

enum Subset { Q_AND_QDOT_OUT, EVERYTHING, EVERYTHING_AND_GOTO };

static size_t up(size_t b) { return (b + 255) / 256 * 256; }

static void check_case(size_t n, size_t esz, size_t B, Subset sub) {
    // the caller's arrays: distinct non-null addresses, never dereferenced by the layout
    static char arrays[vfik::N_STAGED];
    vfik_io io{};
    if (sub == Q_AND_QDOT_OUT) {
        io.q = &arrays[0];
        io.qdot_out = &arrays[1];
    } else {
        for (int i = 0; i < vfik::N_IO; ++i) vfik::io_set(io, vfik::IO_MEMBERS[i].field, &arrays[i]);
    }
    const size_t n_objects = sub == Q_AND_QDOT_OUT ? 0 : 2, n_checks = 5;
    const vfik::IoDims dims{n, esz, n_objects};
    IoStaging st(io, B, dims);
    if (sub == EVERYTHING_AND_GOTO) {
        st.add(vfik::X_Q_OUT, &arrays[vfik::N_IO + 0], B * n * esz, false);
        st.add(vfik::X_ARRIVED, &arrays[vfik::N_IO + 1], B * sizeof(int32_t), false);
        st.add(vfik::X_PENDING, nullptr, n_checks * sizeof(int32_t), false, true);   // staged without an array of the caller's
        st.add(vfik::X_Q_TRAJ, &arrays[vfik::N_IO + 3], n_checks * B * n * esz, false);
        st.add(vfik::X_DIST_TRAJ, &arrays[vfik::N_IO + 4], n_checks * B * 2 * esz, true);
    }
    st.layout();
    const int want_members = sub == Q_AND_QDOT_OUT ? 2 : vfik::N_IO + (sub == EVERYTHING_AND_GOTO ? 5 : 0);
    CHECK(st.members == want_members, "n=%zu esz=%zu B=%zu subset %d: %d members", n, esz, B, (int)sub, st.members);

    // the sizes, spelled out here a second time on purpose: [B][n], [B][4], [B][16], [B][6], [B][2], [B][8], int32 [B], [B][max(objects, 1)][2]
    const size_t Bn = B * n * esz;
    const size_t want_bytes[vfik::N_IO] = {Bn, B * 4 * esz, Bn, Bn, B * 4, Bn, Bn,
                                           Bn, Bn, Bn, B * 16 * esz, B * 16 * esz, B * 6 * esz, Bn, B * 4, B * 2 * esz, Bn, B * 8 * esz,
                                           B * (n_objects ? n_objects : 1) * 2 * esz};
    for (int i = 0; i < vfik::N_IO; ++i) CHECK(st.m[i].bytes == want_bytes[i], "member %d: %zu bytes, expected %zu", i, st.m[i].bytes, want_bytes[i]);

    size_t sum = 0, end_prev = 0, inputs_end = 0;
    bool seen_output = false;
    for (int i = 0; i < vfik::N_STAGED; ++i) {
        const IoStaging::Member& m = st.m[i];
        if (!m.present) continue;   // absent: takes no room -- `sum` and the no-gap check below would show it
        CHECK(m.off % 256 == 0, "member %d at offset %zu", i, m.off);
        CHECK(m.off == end_prev, "member %d at %zu, the one before ends at %zu (overlap or gap)", i, m.off, end_prev);
        CHECK(m.off + m.bytes <= st.total, "member %d ends at %zu, total %zu", i, m.off + m.bytes, st.total);
        end_prev = m.off + up(m.bytes);
        sum += up(m.bytes);
        if (m.input) {
            CHECK(!seen_output, "input %d behind an output", i);
            inputs_end = end_prev;
        } else {
            seen_output = true;
        }
    }
    CHECK(st.total == sum, "total %zu, sum of the rounded sizes %zu", st.total, sum);
    CHECK(st.in_bytes == inputs_end, "input prefix %zu, the inputs end at %zu", st.in_bytes, inputs_end);
    for (int i = 0; i < vfik::N_STAGED; ++i)   // no two present members overlap, pair by pair
        for (int j = i + 1; j < vfik::N_STAGED; ++j) {
            const IoStaging::Member &a = st.m[i], &b = st.m[j];
            if (a.present && b.present) CHECK(a.off + a.bytes <= b.off || b.off + b.bytes <= a.off, "members %d and %d overlap", i, j);
        }

    // mapped into a buffer of `total` bytes, every member lies inside it, and the device io names exactly the present members
    std::vector<char> buf(st.total + 1);
    st.map(buf.data());
    const vfik_io d = st.device_io();
    for (int i = 0; i < vfik::N_STAGED; ++i) {
        const IoStaging::Member& m = st.m[i];
        CHECK((m.dev != nullptr) == m.present, "member %d: device address %p, present %d", i, m.dev, (int)m.present);
        if (m.present) {
            CHECK(static_cast<char*>(m.dev) + m.bytes <= buf.data() + st.total, "member %d leaves the buffer", i);
            static_cast<char*>(m.dev)[0] = 1;                 // (the sanitizers watch these two)
            if (m.bytes) static_cast<char*>(m.dev)[m.bytes - 1] = 1;
        }
        if (i < vfik::N_IO) CHECK(vfik::io_get(d, vfik::IO_MEMBERS[i].field) == m.dev, "member %d of the device io", i);
    }
    // q_ref_out goes with q_ref
    vfik_io no_ref = io;
    no_ref.q_ref = nullptr;
    no_ref.q_ref_out = &arrays[2];
    IoStaging st2(no_ref, B, dims);
    st2.layout();
    for (int i = 0; i < vfik::N_IO; ++i)
        if (vfik::IO_MEMBERS[i].field == offsetof(vfik_io, q_ref_out)) CHECK(!st2.m[i].present, "q_ref_out staged without q_ref");
    // the busy direct form: inputs staged, outputs as the caller has them
    const vfik_io half = st.device_io(&io);
    CHECK(half.q == d.q && half.qdot_out == io.qdot_out && half.status == io.status, "device_io(outputs_from)");
    // the walks: inputs, outputs under a gate (q_out and q_traj of a goto are not), outputs
    int n_in = 0, n_gated = 0, n_out = 0;
    st.each(IoStaging::INPUTS, [&](IoStaging::Member& m) { n_in += m.input; return 0; });
    st.each(IoStaging::GATED_OUTPUTS, [&](IoStaging::Member& m) { n_gated += !m.input; return 0; });
    st.each(IoStaging::OUTPUTS, [&](IoStaging::Member& m) { n_out += !m.input; return 0; });
    const int want_in = sub == Q_AND_QDOT_OUT ? 1 : 7, want_out = sub == Q_AND_QDOT_OUT ? 1 : 12;
    CHECK(n_in == want_in, "%d inputs walked", n_in);
    CHECK(n_gated == want_out + (sub == EVERYTHING_AND_GOTO ? 1 : 0), "%d gated outputs walked", n_gated);   // + the distance trace
    CHECK(n_out == want_out + (sub == EVERYTHING_AND_GOTO ? 4 : 0), "%d outputs walked", n_out);           // + all but pending (no array)
}

// ---- the timed moves: the table of extras (IO_EXTRAS, timed_extras) and the rows of a block (block_rows) ----
enum Form { GOTO, FOLLOW, GOTO_JS, FOLLOW_JS };
static const char* const FORM_NAME[] = {"goto", "follow", "goto_js", "follow_js"};

static void check_move(Form form, size_t n, size_t esz, size_t B, size_t W, size_t n_checks, bool all) {
    using namespace vfik;
    const bool joint = form == GOTO_JS || form == FOLLOW_JS, list = form == FOLLOW || form == FOLLOW_JS;
    char tag[96];
    std::snprintf(tag, sizeof tag, "%s n=%zu esz=%zu B=%zu W=%zu checks=%zu %s", FORM_NAME[form], n, esz, B, W, n_checks, all ? "all" : "required");
    static char arrays[N_STAGED];
    vfik_io io{};
    io.q = &arrays[0];
    io.qdot_out = &arrays[1];
    const TimedDims d{B, n, esz, W, n_checks};
    const size_t Bn = B * n * esz, i32 = sizeof(int32_t);

    // what the form stages, spelled out here a second time on purpose: the rows of st.add that each host form had of its own
    struct Row { IoExtra x; size_t bytes; bool gated, always, input, required; };
    std::vector<Row> rows = {{X_Q_OUT, Bn, false, false, false, false}, {X_PENDING, n_checks * i32, false, true, false, false},
                             {X_Q_TRAJ, n_checks * Bn, false, false, false, false}};
    if (!joint) rows.push_back({X_DIST_TRAJ, n_checks * B * 2 * esz, true, false, false, false});
    if (joint) rows.push_back({X_DIFF, Bn, true, false, false, false});
    if (!list) rows.push_back({X_ARRIVED, B * i32, false, false, false, true});
    if (list) {
        rows.push_back({X_REACHED, B * W * i32, false, false, false, true});
        rows.push_back({X_NEXT, B * i32, false, false, false, true});
        rows.push_back({X_WAY_TRAJ, n_checks * B * i32, true, false, false, false});
        if (joint) rows.push_back({X_WAYQ, B * W * n * esz, false, false, true, true});
        else rows.push_back({X_WAY16, B * W * 16 * esz, false, false, true, true});
    }
    CHECK(rows.size() == (list ? 8u : 5u), "%s", tag);

    // every array of the options given -- also those of the other forms, which must not be staged -- or only the required ones
    TimedMove m{};
    m.io = &io;
    m.joint = joint;
    m.list = list;
    m.n_way = (int)W;
    m.n_checks = (int)n_checks;
    IoStaging want(io, B, IoDims{n, esz, 0});
    for (int x = 0; x < N_IO_EXTRA; ++x)
        if (all) m.x[x] = &arrays[N_IO + x];
    m.x[X_PENDING] = nullptr;   // (the table stages it without an array of the caller's)
    for (const Row& r : rows) {
        if (r.required) m.x[r.x] = &arrays[N_IO + r.x];
        want.add(r.x, m.x[r.x], r.bytes, r.gated, r.always, r.input);
    }
    want.layout();
    IoStaging st(io, B, IoDims{n, esz, 0});
    timed_stage(st, m, d);
    st.layout();
    CHECK(st.total == want.total && st.in_bytes == want.in_bytes && st.members == want.members, "%s: total %zu / %zu, members %d / %d", tag, st.total,
          want.total, st.members, want.members);
    unsigned staged = 0, form_set = 0;
    for (const Row& r : rows) form_set |= 1u << r.x;
    CHECK(timed_extras(joint, list) == form_set, "%s: the form's extras %#x, expected %#x", tag, timed_extras(joint, list), form_set);
    for (int x = 0; x < N_IO_EXTRA; ++x) {
        const IoStaging::Member &a = st.extra((IoExtra)x), &b = want.extra((IoExtra)x);
        CHECK(a.present == b.present && a.host == b.host && a.bytes == b.bytes && a.off == b.off && a.gated == b.gated && a.input == b.input,
              "%s: extra %d: present %d / %d, %zu / %zu bytes at %zu / %zu", tag, x, (int)a.present, (int)b.present, a.bytes, b.bytes, a.off, b.off);
        if (a.present) staged |= 1u << x;
        if (a.present) CHECK(a.input == (x == X_WAY16 || x == X_WAYQ), "%s: extra %d input %d", tag, x, (int)a.input);
    }
    CHECK(all ? staged == form_set : (staged & ~form_set) == 0, "%s: staged %#x, the form's %#x", tag, staged, form_set);
    CHECK(st.extra(X_PENDING).present && !st.extra(X_PENDING).host, "%s: pending is staged without an array of the caller's", tag);
    int n_out = 0, n_host_out = 0;
    st.each(IoStaging::OUTPUTS, [&](IoStaging::Member& x) { n_out += &x >= st.m + N_IO; return 0; });
    for (const Row& r : rows) n_host_out += m.x[r.x] && !r.input;
    CHECK(n_out == n_host_out, "%s: %d outputs among the extras go back, %d have an array", tag, n_out, n_host_out);

    // an early end after `done` checks: `done` rows of every trace go back, everything else whole
    std::vector<char> buf(st.total + 1);
    st.map(buf.data());
    const size_t done = n_checks / 2;   // 0 of 1, 2 of 5
    IoStaging back = st;
    timed_cut(back, d, done);
    for (int x = 0; x < N_IO_EXTRA; ++x) {
        size_t want_bytes = st.extra((IoExtra)x).bytes;
        if (x == X_PENDING) want_bytes = done * i32;
        if (x == X_Q_TRAJ) want_bytes = done * Bn;
        if (x == X_DIST_TRAJ) want_bytes = done * B * 2 * esz;
        if (x == X_WAY_TRAJ) want_bytes = done * B * i32;
        if (st.extra((IoExtra)x).present) CHECK(back.extra((IoExtra)x).bytes == want_bytes, "%s: extra %d goes back with %zu bytes, expected %zu", tag, x, back.extra((IoExtra)x).bytes, want_bytes);
        CHECK(back.extra((IoExtra)x).off == st.extra((IoExtra)x).off && back.extra((IoExtra)x).dev == st.extra((IoExtra)x).dev, "%s: extra %d moved", tag, x);
    }
    for (int i = 0; i < N_IO; ++i) CHECK(back.m[i].bytes == st.m[i].bytes, "%s: member %d of io cut", tag, i);
    TimedMove wired = m;
    timed_rewire(st, wired);
    for (int x = 0; x < N_IO_EXTRA; ++x) CHECK(wired.x[x] == st.extra((IoExtra)x).dev, "%s: extra %d not rewired to its staged address", tag, x);

    // the rows of a block, against traces of exactly their size (the sanitizers watch the first and last byte of every row)
    std::vector<char> q_traj(n_checks * Bn), dist_traj(n_checks * B * 2 * esz), way_traj(n_checks * B * i32), pp0(Bn), pp1(Bn), hdist(B * 2 * esz),
        gdist(B * 2 * esz);
    void* const pingpong[2] = {pp0.data(), pp1.data()};
    auto touch = [](const void* p, size_t bytes) {
        if (!p || !bytes) return;
        char* c = static_cast<char*>(const_cast<void*>(p));
        c[0] = 1;
        c[bytes - 1] = 1;
    };
    for (int mask = 0; mask < 16; ++mask) {
        const bool with_q = mask & 1, with_dist = (mask & 2) && !joint, with_way = (mask & 4) && list, with_gdist = mask & 8;
        TimedMove r{};
        r.io = &io;
        r.joint = joint;
        r.list = list;
        r.x[X_Q_TRAJ] = with_q ? q_traj.data() : nullptr;
        r.x[X_DIST_TRAJ] = with_dist ? dist_traj.data() : nullptr;
        r.x[X_WAY_TRAJ] = with_way ? way_traj.data() : nullptr;
        io.goal_dist = with_gdist ? gdist.data() : nullptr;
        const void* q_before = nullptr;
        for (size_t k : {(size_t)0, (size_t)1, (size_t)2, n_checks - 1}) {
            if (k >= n_checks) continue;
            const BlockRows w = block_rows(r, d, (int)k, pingpong, hdist.data());
            char t2[160];
            std::snprintf(t2, sizeof t2, "%s traces %d k=%zu", tag, mask, k);
            touch(w.q_prev == io.q ? nullptr : w.q_prev, Bn);
            touch(w.q_now, Bn);
            touch(w.dist, B * 2 * esz);
            touch(w.dist_prev, B * 2 * esz);
            touch(w.way_now, B * i32);
            touch(w.way_prev, B * i32);
            if (k == 0) CHECK(w.q_prev == io.q, "%s: block 0 reads io->q", t2);
            if (with_q) {
                CHECK(w.q_now == q_traj.data() + k * Bn, "%s: q_now", t2);
                if (k > 0) CHECK(w.q_prev == q_traj.data() + (k - 1) * Bn, "%s: q_prev", t2);
            } else {
                CHECK(w.q_now == pingpong[k & 1], "%s: q_now is not the handle's row %zu", t2, k & 1);
                if (k > 0) CHECK(w.q_prev == pingpong[(k - 1) & 1] && w.q_prev != w.q_now, "%s: the q rows do not alternate", t2);
                if (k == 1) CHECK(w.q_prev == q_before, "%s: block 1 does not read what block 0 wrote", t2);
            }
            q_before = w.q_now;
            if (with_dist) {
                CHECK(w.dist == dist_traj.data() + k * B * 2 * esz, "%s: dist", t2);
                CHECK(w.dist_prev == (k > 0 ? dist_traj.data() + (k - 1) * B * 2 * esz : nullptr), "%s: dist_prev", t2);
            } else {
                CHECK(w.dist_prev == nullptr, "%s: dist_prev without a trace", t2);
                if (joint) CHECK(w.dist == io.goal_dist && w.dist != hdist.data(), "%s: a joint form's goal_dist is the caller's", t2);
                else CHECK(w.dist == (with_gdist ? (void*)gdist.data() : (void*)hdist.data()), "%s: dist", t2);
            }
            if (with_way) {
                CHECK((char*)w.way_now == way_traj.data() + k * B * i32, "%s: way_now", t2);
                CHECK((const char*)w.way_prev == (k > 0 ? way_traj.data() + (k - 1) * B * i32 : nullptr), "%s: way_prev", t2);
            } else {
                CHECK(w.way_now == nullptr && w.way_prev == nullptr, "%s: way rows without a trace", t2);
            }
        }
    }
}

int main() {
    int cases = 0;
    for (size_t n : {6, 7, 16})
        for (size_t esz : {4, 8})
            for (size_t B : {1, 37, 700})
                for (Subset s : {Q_AND_QDOT_OUT, EVERYTHING, EVERYTHING_AND_GOTO}) {
                    check_case(n, esz, B, s);
                    ++cases;
                }
    if (failures) {
        std::printf("io_layout: %d failures\n", failures);
        return 1;
    }
    std::printf("io_layout OK (%d cases)\n", cases);
    int moves = 0;
    for (Form f : {GOTO, FOLLOW, GOTO_JS, FOLLOW_JS})
        for (size_t n : {6, 7, 16})
            for (size_t esz : {4, 8})
                for (size_t B : {1, 37, 700})
                    for (size_t W : {1, 3})
                        for (size_t n_checks : {1, 5})
                            for (bool all : {true, false}) {
                                check_move(f, n, esz, B, W, n_checks, all);
                                ++moves;
                            }
    if (failures) {
        std::printf("timed moves: %d failures\n", failures);
        return 1;
    }
    std::printf("timed moves OK (%d cases)\n", moves);
    return 0;
}
