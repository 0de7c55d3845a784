// Prints the kernel each launch description takes under the launch plan (vfik_kernel.h: plan_cycle), with its grid, block and LDS bytes:
// one line of `key=value` pairs per launch on stdin (KArgs members; pointers: 1 = given), one line per launch on stdout.  Host code only, no GPU:
// built and run by tests/test_launch_plan.py.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "../../vfclik_amd/csrc/vfik_kernel.h"

// The KUKA LWR 4+ in z-normal form (vfclik_amd/robots.py: (a, alpha, d) = (0, +-pi/2 | 0, d) per link): B[0] the identity, B[i] = Tz(d_i) Rx(alpha_i)
static vfik_chain lwr_chain() {
    static const double quarter[7] = {1, -1, -1, 1, 1, -1, 0}, d[7] = {0.310, 0.0, 0.400, 0.0, 0.390, 0.0, 0.078};
    vfik_chain c;
    std::memset(&c, 0, sizeof c);
    c.n = 7;
    c.B[0][0] = c.B[0][5] = c.B[0][10] = 1.0;
    for (int i = 0; i < 7; ++i) {
        const double al = quarter[i] * 1.57079632679489661923, ca = std::cos(al), sa = std::sin(al);
        const double B[12] = {1, 0, 0, 0, 0, ca, -sa, 0, 0, sa, ca, d[i]};
        std::memcpy(c.B[i + 1], B, sizeof B);
        c.q_lo[i] = -2.0; c.q_hi[i] = 2.0;
    }
    return c;
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::map<std::string, long> kv;
        std::istringstream in(line);
        std::string tok;
        while (in >> tok) {
            const size_t eq = tok.find('=');
            kv[tok.substr(0, eq)] = std::strtol(tok.c_str() + eq + 1, nullptr, 0);
        }
        auto get = [&](const char* k, long d) { auto it = kv.find(k); return it == kv.end() ? d : it->second; };
        auto ptr = [&](const char* k) { return get(k, 0) ? reinterpret_cast<void*>(0x1000) : nullptr; };
        vfik::KArgs a;
        std::memset(&a, 0, sizeof a);
        const int nj = (int)get("nj", 7), io = (int)get("io", 32), block = (int)get("block", 256);
        a.B = (int)get("B", 4096);
        a.Bpad = (a.B + 63) / 64 * 64;
        a.flags = (unsigned)get("flags", 0);
        a.fast_order = (int)get("fast_order", 5);
        a.slots_used = (int)get("slots_used", 6);
        a.slots_used_fast = (int)get("slots_used_fast", 4);
        a.tool_stride = get("tool", 0) ? a.Bpad : 0;
        a.plain = (int)get("plain", 1);
        a.dhp = (int)get("dhp", 0);
        // The rule for a shared tool's 3 x 3 block (include/vfik.h, vfik_set_tool): tool_shear_e6 = s gives the identity with entry (0, 1) =
        // s / 1e6, a block whose max |R R^T - I| is that entry; tool_flat = 1 zeroes the block's last column (no inverse).  `plain` and `dhp` are
        // then what kconst_fill answers for the LWR with that tool, as a handle takes them: 2 and 1, or 0 and 0 for a block the rule refuses.
        if (kv.count("tool_shear_e6") || kv.count("tool_flat")) {
            double tool12[12] = {1, 0, 0, 0.02, 0, 1, 0, -0.01, 0, 0, 1, 0.2};
            tool12[1] = (double)get("tool_shear_e6", 0) / 1e6;
            if (get("tool_flat", 0)) tool12[2] = tool12[6] = tool12[10] = 0.0;
            const vfik_chain lwr = lwr_chain();
            vfik_params par;
            std::memset(&par, 0, sizeof par);
            par.speed_scale = 1.0; par.lambda = 0.1;
            for (double& w : par.wy) w = 1.0;
            for (double& w : par.wq) w = 1.0;
            std::vector<char> image(vfik::kconst_bytes(lwr.n));
            vfik::kconst_fill(lwr.n, image.data(), lwr, par, tool12, &a.plain, &a.dhp);
        }
        a.mixw = ptr("mixw");
        a.wts = static_cast<const double*>(ptr("wts"));
        a.ext = ptr("ext");
        a.q_ref = ptr("q_ref");
        a.q_cmded = ptr("q_cmded");
        a.q_lo = ptr("q_lo");
        a.q_hi = a.q_lo;
        a.q_ref_out = ptr("q_ref_out");
        a.null_control = ptr("null_control");
        a.qdot_vf = ptr("qdot_vf");
        a.qdot_null = ptr("qdot_null");
        a.qdot_out = get("qdot_out", 1) ? reinterpret_cast<void*>(0x1000) : nullptr;
        a.pose = ptr("pose");
        a.pose_nt = ptr("pose_nt");
        a.v6 = ptr("v6");
        a.qdist = ptr("qdist");
        a.goal_dist = ptr("goal_dist");
        a.active = static_cast<const int*>(ptr("active"));
        a.q_out = ptr("q_out");
        a.n_cycles = (int)get("n_cycles", 0);
        a.sub8_max_batch = (int)get("sub8", 0);
        a.sub8_max_batch_ns = (int)get("sub8_ns", 0);
        a.sub8_max_batch_full = (int)get("sub8_full", 4096);
        a.n_simd = (int)get("n_simd", 1024);
        a.has_funnel = (int)get("funnel", 0);
        a.mixed = (int)get("mixed", 0);
        a.uni = (int)get("uni", 0);
        a.waves2 = (int)get("waves2", 0);
        const bool ns = a.flags & VFIK_F_NULLSPACE;
        const vfik::CyclePlan p = vfik::plan_cycle(a, nj, io, ns, block);
        std::printf("%s grid=%u block=%u lds=%zu\n", vfik::cycle_kernel_name(p, nj, io, ns).c_str(), p.grid, p.block, p.lds);
    }
    return 0;
}
