// The scene side of vfik_set_fields (vfclik_amd/csrc/vfik_scene.h) on the CPU: host code only, no GPU, no library -- built and run by
// tests/test_scene_plan.py.  One request per line on stdin, `key=value` pairs; arrays (vfik_field records, int32 counts) travel as hex bytes.
//   scene_plan plan    io= nj= B= S= uni= mixed= one= then one or more  set=<first_arm>,<n_arms>,<max_fields>,<counts>,<fields>
//                      -> what a handle with these knobs decides after each call (" | " between them), up to a call vfik_set_fields would refuse
//   scene_plan pack    io= S= n_arms= max_fields= counts= fields=   -> every staging image as hex, then the arms' summaries
//   scene_plan planes  io= S=                                       -> every image's planes and bytes per arm and plane
//   scene_plan slots   fields=                                      -> slots_needed of one arm
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../vfclik_amd/csrc/vfik_scene.h"

namespace {

std::vector<unsigned char> unhex(const std::string& s) {
    std::vector<unsigned char> out(s.size() / 2);
    for (size_t i = 0; i < out.size(); ++i) out[i] = (unsigned char)std::strtol(s.substr(2 * i, 2).c_str(), nullptr, 16);
    return out;
}

template <typename V>
void hex_line(const char* name, const V& v) {
    const unsigned char* p = reinterpret_cast<const unsigned char*>(v.data());
    std::printf("%s ", name);
    for (size_t i = 0; i < v.size() * sizeof(v[0]); ++i) std::printf("%02x", p[i]);
    std::printf("\n");
}

struct FieldSets {   // the arguments of one vfik_set_fields call
    int first_arm = 0, n_arms = 0, max_fields = 0;
    std::vector<int32_t> counts;
    std::vector<vfik_field> fields;
    void take(const std::string& counts_hex, const std::string& fields_hex) {
        const std::vector<unsigned char> c = unhex(counts_hex), f = unhex(fields_hex);
        counts.resize(c.size() / sizeof(int32_t));
        std::memcpy(counts.data(), c.data(), counts.size() * sizeof(int32_t));
        fields.resize(f.size() / sizeof(vfik_field) + 1);   // (+ 1: data() of an empty call is still a pointer)
        std::memcpy(fields.data(), f.data(), f.size());
    }
};

void pack(int io, const FieldSets& c, int S, vfik::FieldImages& im, vfik::ArmScene* arms) {
    if (io == 32) vfik::pack_fields<float>(c.fields.data(), c.max_fields, c.counts.data(), c.n_arms, S, im, arms);
    else vfik::pack_fields<double>(c.fields.data(), c.max_fields, c.counts.data(), c.n_arms, S, im, arms);
}

}  // namespace

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        std::string tok, fields_hex, counts_hex;
        int io = 32, nj = 7, B = 1, S = 16, n_arms = 1, max_fields = 0;
        vfik::SceneKnobs knobs;
        std::vector<FieldSets> calls;
        while (in >> tok) {
            const size_t eq = tok.find('=');
            const std::string k = tok.substr(0, eq), v = tok.substr(eq + 1);
            if (k == "io") io = std::atoi(v.c_str());
            else if (k == "nj") nj = std::atoi(v.c_str());
            else if (k == "B") B = std::atoi(v.c_str());
            else if (k == "S") S = std::atoi(v.c_str());
            else if (k == "n_arms") n_arms = std::atoi(v.c_str());
            else if (k == "max_fields") max_fields = std::atoi(v.c_str());
            else if (k == "uni") knobs.uni_allowed = std::atoi(v.c_str());
            else if (k == "mixed") knobs.mixed_allowed = std::atoi(v.c_str());
            else if (k == "one") knobs.one_chunk_allowed = std::atoi(v.c_str());
            else if (k == "counts") counts_hex = v;
            else if (k == "fields") fields_hex = v;
            else if (k == "set") {
                std::istringstream parts(v);
                std::string p[5];
                for (std::string& s : p) std::getline(parts, s, ',');
                FieldSets c;
                c.first_arm = std::atoi(p[0].c_str()); c.n_arms = std::atoi(p[1].c_str()); c.max_fields = std::atoi(p[2].c_str());
                c.take(p[3], p[4]);
                calls.push_back(c);
            }
        }
        knobs.io_dtype = io; knobs.n = nj;
        if (mode == "plan") {
            // a handle as vfik_create leaves it, then vfik_set_fields' host side call by call: validate, pack, store the arms, plan
            std::vector<vfik::ArmScene> arms(B);
            for (size_t ci = 0; ci < calls.size(); ++ci) {
                const FieldSets& c = calls[ci];
                bool refused = false;
                for (int j = 0; j < c.n_arms; ++j) {
                    const int need = vfik::slots_needed(c.fields.data() + (size_t)j * c.max_fields, c.counts[j]);
                    if (need < 0 || need > S) refused = true;
                }
                if (refused) { std::printf("%scall %zu refused", ci ? " | " : "", ci); break; }
                vfik::FieldImages im;
                pack(io, c, S, im, arms.data() + c.first_arm);
                const vfik::ScenePlan plan = vfik::plan_scene(arms.data(), B, knobs);
                std::printf("%sslots_used=%d slots_used_fast=%d any_funnel=%d fast_order=%d mixed=%d uni_ok=%d one5=%d", ci ? " | " : "", plan.slots_used,
                            plan.slots_used_fast, plan.any_funnel, plan.fast_order, plan.mixed, plan.uni_ok, plan.one5);
                if (plan.uni_ok && plan.have_pair) std::printf(" pair=%.17g,%.17g", plan.safe, plan.force);
                else std::printf(" pair=none");
                std::printf(" field_path=%d mixed_orders=%d uniform=%d one_chunk=%d", plan.field_path(), plan.mixed_orders(), plan.uniform(knobs), plan.one_chunk());
            }
            std::printf("\n");
        } else if (mode == "pack") {
            FieldSets c;
            c.n_arms = n_arms; c.max_fields = max_fields;
            c.take(counts_hex, fields_hex);
            vfik::FieldImages im;
            std::vector<vfik::ArmScene> arms(n_arms);
            pack(io, c, S, im, arms.data());
            hex_line("goal", im.goal); hex_line("aux", im.aux); hex_line("slots", im.slots); hex_line("compact", im.compact);
            hex_line("uni", im.uni); hex_line("orders", im.orders); hex_line("repmap", im.repmap); hex_line("scenemaps", im.scenemaps);
            std::printf("arms");
            for (const vfik::ArmScene& a : arms)
                std::printf(" %d,%d,%d,%d,%.17g,%.17g,%d,%d", a.slots, a.compact_slots, a.has_aux ? 1 : 0, (int)a.pair, a.safe, a.force, (int)a.orders, a.order);
            std::printf("\n");
        } else if (mode == "planes") {
            static const char* names[vfik::N_IMAGES] = {"goal", "aux", "slots", "compact", "uni", "orders", "repmap", "scenemaps"};
            for (int img = 0; img < vfik::N_IMAGES; ++img) {
                const vfik::ImageShape s = vfik::image_shape((vfik::Image)img, S, io);
                std::printf("%s=%d,%d,%zu ", names[img], s.planes, vfik::staged_planes((vfik::Image)img, S, io), s.arm_bytes);
            }
            std::printf("\n");
        } else if (mode == "slots") {
            FieldSets c;
            c.take("", fields_hex);
            int bad = -1;
            const int need = vfik::slots_needed(c.fields.data(), (int)c.fields.size() - 1, &bad);
            std::printf("need=%d bad=%d\n", need, bad);
        } else {
            std::fprintf(stderr, "usage: scene_plan plan|pack|planes|slots < requests\n");
            return 2;
        }
    }
    return 0;
}
