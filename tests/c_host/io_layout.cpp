// The staging layout of the host-pointer call forms (vfclik_amd/csrc/vfik_io_layout.h), checked on the CPU: no HIP, no library.
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
    return 0;
}
