// The argument checks of the whole-arm avoidance (vfclik_amd/csrc/vfik_links.h: avoid_check, avoid_rule_check) on the CPU: host code only, no
// GPU, no HIP header, no library -- built and run by tests/test_avoid_host.py, once plain and once with -fsanitize=address,undefined.  One
// request per line on stdin, of one of two kinds:
//   call L= q=<0|1> pts=<address, decimal> out=<0|1> n_rep= first= count= mask=<L uint32 as hex, or `null`> gain= d0= channel= ext=<0|1>
//   rule L= gain= d0= channel= reserved= mask=<16 uint32 as hex>
// q and out say whether the pointer is given; pts is the address itself (only NULL and the alignment are looked at); ext: the handle has an
// ext buffer; gain and d0 as strtod reads them (nan, inf).  A call's mask is copied into a heap block of exactly L words, so that a read
// past the caller's list is a finding of the sanitizer.  One answer per line:   rc=<0|-1|-4> msg=<the reason, empty for 0>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>

#include "../../vfclik_amd/csrc/vfik_links.h"

namespace {

bool unhex(const std::string& s, void* out, size_t bytes) {
    if (s.size() != 2 * bytes) return false;
    unsigned char* p = static_cast<unsigned char*>(out);
    for (size_t i = 0; i < bytes; ++i) p[i] = (unsigned char)std::strtol(s.substr(2 * i, 2).c_str(), nullptr, 16);
    return true;
}

}  // namespace

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        std::string kind, tok, msk = "null";
        in >> kind;
        int L = 0, n_rep = 0, first = 0, count = 0, has_q = 0, has_out = 0, channel = -1, ext = 0, reserved = 0;
        unsigned long long pts = 0;
        double gain = 0.0, d0 = 0.0;
        while (in >> tok) {
            const size_t eq = tok.find('=');
            const std::string k = tok.substr(0, eq), v = tok.substr(eq + 1);
            if (k == "L") L = std::atoi(v.c_str());
            else if (k == "q") has_q = std::atoi(v.c_str());
            else if (k == "pts") pts = std::strtoull(v.c_str(), nullptr, 10);
            else if (k == "out") has_out = std::atoi(v.c_str());
            else if (k == "n_rep") n_rep = std::atoi(v.c_str());
            else if (k == "first") first = std::atoi(v.c_str());
            else if (k == "count") count = std::atoi(v.c_str());
            else if (k == "mask") msk = v;
            else if (k == "gain") gain = std::strtod(v.c_str(), nullptr);
            else if (k == "d0") d0 = std::strtod(v.c_str(), nullptr);
            else if (k == "channel") channel = std::atoi(v.c_str());
            else if (k == "ext") ext = std::atoi(v.c_str());
            else if (k == "reserved") reserved = std::atoi(v.c_str());
            else {
                std::fprintf(stderr, "avoid: unknown key %s\n", k.c_str());
                return 2;
            }
        }
        char msg[160] = "";
        static const char some = 0;
        int rc;
        if (kind == "call") {
            uint32_t* mask = nullptr;
            const int words = L > 0 && L <= VFIK_MAX_LINK_SPHERES ? L : 0;
            if (msk != "null") {
                mask = static_cast<uint32_t*>(std::malloc(words ? words * sizeof(uint32_t) : 1));
                if (!unhex(msk, mask, words * sizeof(uint32_t))) {
                    std::fprintf(stderr, "avoid: mask= is not L words\n");
                    return 2;
                }
            }
            rc = vfik::avoid_check(L, has_q ? &some : nullptr, reinterpret_cast<const void*>((uintptr_t)pts), has_out ? &some : nullptr, n_rep, first,
                                   count, mask, gain, d0, channel, ext != 0, msg, sizeof msg);
            std::free(mask);
        } else if (kind == "rule") {
            uint32_t mask[VFIK_MAX_LINK_SPHERES];
            if (!unhex(msk, mask, sizeof mask)) {
                std::fprintf(stderr, "avoid: a rule's mask= is sixteen words\n");
                return 2;
            }
            rc = vfik::avoid_rule_check(L, gain, d0, channel, reserved, mask, msg, sizeof msg);
        } else {
            std::fprintf(stderr, "avoid: a request is a `call` or a `rule`\n");
            return 2;
        }
        std::printf("rc=%d msg=%s\n", rc, rc == 0 ? "" : msg);
    }
    return 0;
}
