// vfik_scene.h -- the scene side of vfik_set_fields as pure host code: the images a field set is packed into (the ONE table of their plane
// counts), the packing itself, what it learns about each arm (ArmScene), and the batch's field-path decision (plan_scene).  No HIP call and
// no handle: vfik_abi.cpp allocates, copies and uploads by it, tests/c_host/scene_plan.cpp drives it on the CPU (tests/test_scene_plan.py).
// What it decides is the input of the launch plan (vfik_kernel.h: plan_cycle): fast_order, uni, mixed, one5, has_funnel, slots_used_fast.
#pragma once

#include <algorithm>
#include <cstddef>
#include <limits>
#include <vector>

#include "../../include/vfik.h"
#include "vfik_kernel.h"

namespace vfik {

// number of device slots a field of this type occupies (goal block excluded)
inline int slots_of(int type) {
    switch (type) {
        case VFIK_FIELD_NULL: return 0;
        case VFIK_FIELD_REPELLER: return 1;
        case VFIK_FIELD_HEMISPHERE: return 2;
        case VFIK_FIELD_FUNNEL: return 2;
        case VFIK_FIELD_ATTRACTOR: return 3;
        default: return -1;
    }
}

// THE goal rule: the first attractor of a walk over an arm's fields is its goal block and takes no slot; every other primitive takes slots_of(type)
inline bool takes_goal_block(const vfik_field& fd, bool& have_goal) {
    if (fd.type != VFIK_FIELD_ATTRACTOR || have_goal) return false;
    have_goal = true;
    return true;
}

// Slots the arm's field set needs, or -1 with *bad = the index of the first field of an unknown type.  (Which attractor the walk meets first
// does not matter to the count.)
inline int slots_needed(const vfik_field* f, int count, int* bad = nullptr) {
    int need = 0;
    bool goal = false;
    for (int k = 0; k < count; ++k) {
        const int ns = slots_of(f[k].type);
        if (ns < 0) { if (bad) *bad = k; return -1; }
        if (takes_goal_block(f[k], goal)) continue;
        need += ns;
    }
    return need;
}

// ---- the images vfik_set_fields writes, said once ----
// Quad-plane images hold one quad (4 scalars of the I/O type) per arm and plane; the order planes and the maps 16 bytes per arm and plane.
enum Image {
    IMG_GOAL,       // goal block
    IMG_AUX,        // funnel planes 0..2, hemisphere planes 3..5 (straight-line path)
    IMG_SLOTS,      // general image: 2 quads per slot (>= 1 slot: the prefetch reads slot 0)
    IMG_COMPACT,    // compact repeller image: 3 quads per PAIR of slots
    IMG_UNI,        // uniform repeller image: the empty plane 0, then one quad per slot
    IMG_ORDERS,     // order planes: one byte per compact-image slot, 16 a plane
    IMG_REPMAP,     // vfik_move_fields' map: one unsigned short per compact-image slot, 8 a plane
    IMG_SCENEMAPS,  // vfik_move_scene's maps: three of repmap's layout in a row (SCENE_FUN, SCENE_HEM, SCENE_ATT)
    N_IMAGES
};
struct ImageShape { int planes; size_t arm_bytes; };   // planes on the device; bytes per arm and plane

inline ImageShape image_shape(Image img, int max_slots, int io_dtype) {
    const int S1 = std::max(1, max_slots);
    const size_t quad = 4 * (size_t)(io_dtype == 32 ? 4 : 8);
    switch (img) {
        case IMG_GOAL: return {4, quad};
        case IMG_AUX: return {6, quad};
        case IMG_SLOTS: return {2 * S1, quad};
        case IMG_COMPACT: return {3 * ((S1 + 1) / 2), quad};
        // ... and at least one chunk's worth of the I/O type (Stage<T>::PRE), because the one-chunk body of the lean launches requests planes
        // 1 ... PRE without looking at the slots in use
        case IMG_UNI: return {std::max(S1, io_dtype == 32 ? Stage<float>::PRE : Stage<double>::PRE) + 1, quad};
        case IMG_ORDERS: return {(S1 + 15) / 16, 16};
        case IMG_REPMAP: return {(S1 + 7) / 8, 16};
        case IMG_SCENEMAPS: return {3 * ((S1 + 7) / 8), 16};
        default: return {0, 0};
    }
}
// Planes of an image that a vfik_set_fields call stages and copies.  They are the device's, but for the uniform image: its staging holds the
// slots alone -- slot m lives in device plane m + 1, and the planes past max_slots belong to vfik_create.
inline int staged_planes(Image img, int max_slots, int io_dtype) {
    return img == IMG_UNI ? std::max(1, max_slots) : image_shape(img, max_slots, io_dtype).planes;
}
inline size_t image_bytes(Image img, int max_slots, int io_dtype, size_t arms) {
    const ImageShape s = image_shape(img, max_slots, io_dtype);
    return (size_t)s.planes * arms * s.arm_bytes;
}

// The staging images of one vfik_set_fields call: staged_planes(img) planes of n_arms arms each (plane P, arm j, component c of a quad ->
// (P * n_arms + j) * 4 + c).
struct FieldImages {
    std::vector<char> goal, aux, slots, compact, uni;
    std::vector<unsigned char> orders;
    std::vector<unsigned short> repmap, scenemaps;
};

// What packing learns about one arm -- all plan_scene needs to know of it.  (The default is an arm without fields: vfik_create's.)
enum class ArmOrders {
    NONE,     // no decay repeller
    ONE,      // every slot is a decay repeller of the integer order `order` (beside at most one funnel and one hemisphere with integer orders)
    DIFFER,   // ... of integer orders that differ
    GENERAL   // anything else: the general field path
};
enum class ArmPair { NONE, ONE, MIXED };   // no decay repeller; all of them share one (safe, force); they do not
struct ArmScene {
    int slots = 0;          // general slots used
    int compact_slots = 0;  // slots of the compact repeller image used (repellers only: the funnel is not one)
    bool has_aux = false;   // a funnel or a hemisphere
    ArmPair pair = ArmPair::NONE;
    double safe = 0.0, force = 0.0;   // ... the pair (ArmPair::ONE), rounded to the I/O type
    ArmOrders orders = ArmOrders::NONE;
    int order = 0;          // ... the order (ArmOrders::ONE)
};

// an order the straight-line path can take: an integer in [0, 128)
inline bool small_int_order(double o) { return o >= 0.0 && o < 128.0 && (double)(int)o == o; }

template <typename T>
inline void put(std::vector<char>& buf, size_t idx, double v) {
    reinterpret_cast<T*>(buf.data())[idx] = static_cast<T>(v);
}

// Pack the field sets of n_arms arms into the staging images and summarise each arm.
// The walk is in ascending id.  The arm's class (ArmOrders) does not depend on the walk's order: a second attractor, funnel or hemisphere makes
// the arm GENERAL whichever of the two comes first, every order is tested on its own, and the repellers' orders differ when they are not all equal.
template <typename T>
void pack_fields(const vfik_field* fields, int max_fields, const int32_t* counts, int n_arms, int S, FieldImages& im, ArmScene* arms) {
    const int io = sizeof(T) == 4 ? 32 : 64;
    auto quads = [&](Image img) { return (size_t)staged_planes(img, S, io) * n_arms * 4 * sizeof(T); };
    im.aux.assign(quads(IMG_AUX), 0);
    im.goal.assign(quads(IMG_GOAL), 0);
    im.slots.assign(quads(IMG_SLOTS), 0);
    // compact image: a decay repeller needs 6 of its slot's 8 scalars (x y z radius safe | force; the decay order is
    // one number for the batch on the straight-line path and the type is known), so two slots share three quads:
    // (x0 y0 z0 r0 | s0 f0 x1 y1 | z1 r1 s1 f1).  Slots of another type leave zeros (force 0): they force the general path.
    im.compact.assign(quads(IMG_COMPACT), 0);
    // uniform image: when every decay repeller of the BATCH has the same safe distance and force (what the object feeder sends:
    // 0.001 and -10, object_feeder:301-302,323,331) a slot is one quad (x y z radius) and the pair lives in the constants
    im.uni.assign(quads(IMG_UNI), 0);
    // (the force being the batch's, a slot an arm does not use cannot carry force 0 as in the other images: its radius is -inf)
    for (size_t q4 = 0; q4 < im.uni.size() / (4 * sizeof(T)); ++q4) put<T>(im.uni, q4 * 4 + 3, -std::numeric_limits<double>::infinity());
    // order planes: byte (m % 16) of plane (m / 16) = the integer decay order of compact-image slot m; slots an arm does not use
    // repeat the order of its last repeller (5 -- what the feeder sends, object_feeder:302,333 -- for an arm without any)
    const size_t order_planes = (size_t)staged_planes(IMG_ORDERS, S, io);
    im.orders.assign(order_planes * n_arms * 16, 5);
    // vfik_move_fields' map: entry (m % 8) of plane (m / 8) = the general slot of compact-image slot m, MOVE_NONE behind the arm's last repeller
    const size_t map_planes = (size_t)staged_planes(IMG_REPMAP, S, io);
    im.repmap.assign(map_planes * n_arms * 8, MOVE_NONE);
    // vfik_move_scene's maps, three of that layout in a row: entry k of class c (funnel, hemisphere, attractor behind the goal block) = the
    // general slot of the arm's k-th primitive of that class, MOVE_NONE from the arm's count on
    im.scenemaps.assign(3 * map_planes * n_arms * 8, MOVE_NONE);
    std::vector<int> order;
    for (int j = 0; j < n_arms; ++j) {
        auto sm = [&](int cls, int k) -> unsigned short& { return im.scenemaps[((cls * map_planes + (size_t)(k >> 3)) * n_arms + j) * 8 + (k & 7)]; };
        auto ord = [&](int ms) -> unsigned char& { return im.orders[((size_t)(ms >> 4) * n_arms + j) * 16 + (ms & 15)]; };
        const vfik_field* f = fields + (size_t)j * max_fields;
        order.resize(counts[j]);
        for (int k = 0; k < counts[j]; ++k) order[k] = k;
        std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return f[a].id < f[b].id; });
        bool have_goal = false, have_funnel = false, have_hemi = false;
        ArmScene arm;
        int m = 0, mr = 0;  // general slots used; compact-image slots used (repellers only, packed densely)
        int n_fun = 0, n_hem = 0, n_att = 0;   // funnels, hemispheres, attractors behind the goal block seen so far
        auto gq = [&](int e) { return ((size_t)(e >> 2) * n_arms + j) * 4 + (e & 3); };
        for (int k : order) {
            const vfik_field& fd = f[k];
            if (fd.type == VFIK_FIELD_NULL) continue;
            if (takes_goal_block(fd, have_goal)) {
                for (int e = 0; e < 12; ++e) put<T>(im.goal, gq(e), fd.p[e]);
                put<T>(im.goal, gq(12), 1.0);  // "goal present"
                put<T>(im.goal, gq(13), fd.p[16]);
                put<T>(im.goal, gq(14), fd.force);
                continue;
            }
            const int ns = slots_of(fd.type);
            auto at = [&](int slot, int e) { return ((size_t)(2 * (m + slot) + (e >> 2)) * n_arms + j) * 4 + (e & 3); };
            for (int e = 0; e < 6; ++e) put<T>(im.slots, at(0, e), fd.p[e]);
            put<T>(im.slots, at(0, 6), fd.force);
            put<T>(im.slots, at(0, 7), (double)fd.type);
            if (fd.type == VFIK_FIELD_FUNNEL) sm(SCENE_FUN, n_fun++) = (unsigned short)m;
            if (fd.type == VFIK_FIELD_HEMISPHERE) sm(SCENE_HEM, n_hem++) = (unsigned short)m;
            if (fd.type == VFIK_FIELD_ATTRACTOR) sm(SCENE_ATT, n_att++) = (unsigned short)m;
            if (fd.type == VFIK_FIELD_FUNNEL && !have_funnel) {
                // the straight-line path's funnel block (used only when this funnel is the arm's one non-repeller entry): one funnel attractor
                // with small integer decay orders (object_feeder:277,279 sends 10 and 2) is evaluated from its own block
                have_funnel = true;
                const double blk[12] = {fd.p[0], fd.p[1], fd.p[2], fd.p[3], fd.p[4], fd.p[5], fd.p[6], fd.p[7], fd.p[8], fd.p[9], fd.force, 1.0};
                for (int e = 0; e < 12; ++e) put<T>(im.aux, ((size_t)(e >> 2) * n_arms + j) * 4 + (e & 3), blk[e]);
                if (!small_int_order(fd.p[7]) || !small_int_order(fd.p[9])) arm.orders = ArmOrders::GENERAL;
            } else if (fd.type == VFIK_FIELD_HEMISPHERE && !have_hemi) {
                // ... and the hemisphere block (object_feeder:344-353, ObstacleH: a surface with its normal): x y z nx | ny nz safe order | force present
                // -- one hemisphere repeller with a small integer decay order (object_feeder:353 sends 5)
                have_hemi = true;
                const double blk[12] = {fd.p[0], fd.p[1], fd.p[2], fd.p[3], fd.p[4], fd.p[5], fd.p[6], fd.p[7], fd.force, 1.0, 0.0, 0.0};
                for (int e = 0; e < 12; ++e) put<T>(im.aux, ((size_t)(3 + (e >> 2)) * n_arms + j) * 4 + (e & 3), blk[e]);
                if (!small_int_order(fd.p[7])) arm.orders = ArmOrders::GENERAL;
            } else if (fd.type != VFIK_FIELD_REPELLER) {
                arm.orders = ArmOrders::GENERAL;   // a further attractor, funnel or hemisphere
            }
            if (fd.type == VFIK_FIELD_REPELLER) {
                for (int e = 0; e < 4; ++e) put<T>(im.uni, ((size_t)mr * n_arms + j) * 4 + e, fd.p[e]);
                // (compared as the device will see them: rounded to the I/O type)
                const double sv = (double)static_cast<T>(fd.p[4]), fv = (double)static_cast<T>(fd.force);
                if (arm.pair == ArmPair::NONE) { arm.pair = ArmPair::ONE; arm.safe = sv; arm.force = fv; }
                else if (arm.safe != sv || arm.force != fv) arm.pair = ArmPair::MIXED;
                // (the uniform image's kernel clamps radius + safe at 0 -- how it disarms unused slots: a repeller with a NEGATIVE sum
                // keeps the arm, hence the batch, on the compact image)
                if ((double)static_cast<T>(fd.p[3]) + sv < 0.0) arm.pair = ArmPair::MIXED;
                // (non-integer or large orders send the batch to the general path: the byte is not read then)
                const bool small = small_int_order(fd.p[5]);
                const int o = small ? (int)fd.p[5] : 0;
                ord(mr) = (unsigned char)o;
                if (!small) arm.orders = ArmOrders::GENERAL;
                else if (arm.orders == ArmOrders::NONE) { arm.orders = ArmOrders::ONE; arm.order = o; }
                else if (arm.orders == ArmOrders::ONE && o != arm.order) arm.orders = ArmOrders::DIFFER;
                im.repmap[((size_t)(mr >> 3) * n_arms + j) * 8 + (mr & 7)] = (unsigned short)m;
                const int pair = mr >> 1, half = mr & 1;
                ++mr;
                for (int i = 0; i < 6; ++i) {
                    const int e = 6 * half + i;  // position in the pair's 12 scalars
                    put<T>(im.compact, ((size_t)(3 * pair + (e >> 2)) * n_arms + j) * 4 + (e & 3), i < 5 ? fd.p[i] : fd.force);
                }
            }
            for (int c = 1; c < ns; ++c) {
                for (int e = 0; e < 6; ++e) {
                    const int pi = 6 * c + e;
                    put<T>(im.slots, at(c, e), pi < VFIK_MAX_PARAMS ? fd.p[pi] : 0.0);
                }
                put<T>(im.slots, at(c, 7), -1.0);
            }
            m += ns;
        }
        // the slots behind the last repeller repeat ITS order: a partly filled chunk adds no distinct order of its own
        for (int ms = mr; mr > 0 && ms < (int)order_planes * 16; ++ms) ord(ms) = ord(mr - 1);
        arm.slots = m;
        arm.compact_slots = mr;
        arm.has_aux = have_funnel || have_hemi;
        arms[j] = arm;
    }
}

// ---- the batch's decision ----
struct SceneKnobs {
    int uni_allowed = 1;        // VFIK_UNIFORM_IMAGE=0: always the compact image (tests, A/B)
    int mixed_allowed = 1;      // VFIK_MIXED_ORDERS=0: differing integer orders take the general path, as until round 3 (tests, A/B)
    int one_chunk_allowed = 1;  // VFIK_ONE_CHUNK=0: never the one-chunk order-5 body of the lean launches (tests, A/B)
    int io_dtype = 32, n = 0;   // the handle's I/O type and joint count
};

struct ScenePlan {
    int slots_used = 0;
    int slots_used_fast = 0;   // slots of the compact repeller image in use
    int any_funnel = 0;        // some arm has an aux block
    int fast_order = 0;        // >= 0: the straight-line path, with this order unless `mixed`; -1: the general path
    int mixed = 0;             // the batch's decay repellers have integer orders that differ (between slots or between arms): the order planes are read
    int uni_ok = 0;            // the batch's decay repellers share one pair (the one in the device constants: KConst::rep_safe, dh[0].pad)
    int one5 = 0;              // the uniform image holds one chunk of order-5 repellers: cycle_kernel_s's one-chunk body
    bool have_pair = false;    // with uni_ok: there is such a pair (some arm has a decay repeller) ...
    double safe = 0.0, force = 0.0;   // ... this one
    // what introspection reports and a launch is given (the general path has none of the three)
    int field_path() const { return fast_order < 0 ? 0 : (any_funnel ? 2 : 1); }
    int mixed_orders() const { return (fast_order >= 0 && mixed) ? 1 : 0; }
    int uniform(const SceneKnobs& k) const { return (fast_order >= 0 && uni_ok && k.uni_allowed) ? 1 : 0; }
    int one_chunk() const { return (fast_order >= 0 && one5) ? 1 : 0; }
};

// ALL arms of the handle, not those of one call: a partial vfik_set_fields changes the batch's answer.
inline ScenePlan plan_scene(const ArmScene* arms, int B, const SceneKnobs& knobs) {
    ScenePlan p;
    for (int b = 0; b < B; ++b) {
        p.slots_used = std::max(p.slots_used, arms[b].slots);
        p.slots_used_fast = std::max(p.slots_used_fast, arms[b].compact_slots);
        p.any_funnel |= arms[b].has_aux ? 1 : 0;
    }
    // One integer order for every decay repeller of the batch: the straight-line path with that order as a launch constant.  Integer
    // orders that differ -- within an arm (DIFFER) or between arms: the straight-line path still, reading the order planes (`mixed`).
    int fo = -1;
    bool general = false, mixed = false;
    for (int b = 0; b < B; ++b) {
        const ArmScene& a = arms[b];
        if (a.orders == ArmOrders::GENERAL) { general = true; break; }
        if (a.orders == ArmOrders::DIFFER || (a.orders == ArmOrders::ONE && fo >= 0 && a.order != fo)) mixed = true;
        if (a.orders == ArmOrders::ONE) fo = a.order;
    }
    if (!knobs.mixed_allowed && mixed) general = true;
    p.mixed = (!general && mixed) ? 1 : 0;
    p.fast_order = general ? -1 : (fo < 0 ? 5 : fo);   // (no repeller anywhere: any order >= 1 will do -- see the uniform image below)
    // one (safe distance, force) for every decay repeller of the batch?  Then the pair goes into the device constants and the lean
    // launches read the uniform image.
    // (not with decay order 0: the uniform image disarms an unused slot through its magnitude, ((radius + safe) / D)^order = 0^order,
    // which is 1 for order 0)
    bool uni_ok = !general && p.fast_order != 0;
    for (int b = 0; b < B && uni_ok; ++b) {
        const ArmScene& a = arms[b];
        if (a.pair == ArmPair::NONE) continue;
        if (a.pair == ArmPair::MIXED) { uni_ok = false; break; }
        if (!p.have_pair) { p.have_pair = true; p.safe = a.safe; p.force = a.force; }
        else if (a.safe != p.safe || a.force != p.force) uni_ok = false;
    }
    p.uni_ok = uni_ok ? 1 : 0;
    // One chunk of order-5 repellers on the uniform image (what the feeder sends: object_feeder:302,333): the lean float launches of chains
    // of up to 7 joints take the body compiled for exactly that (cycle_kernel_s, ONE5).  It reads planes 1 ... PRE of the image whatever
    // the slots in use: the image owns them (image_shape: IMG_UNI), and every plane at or beyond an arm's count is empty -- vfik_set_fields'
    // copy rewrites all max_slots planes of the arms it names (pack_fields: radius -inf past the arm's last repeller), the planes beyond
    // max_slots keep the -inf of vfik_create, and vfik_move_fields writes the rows of existing repellers alone.
    p.one5 = (knobs.one_chunk_allowed && uni_ok && knobs.uni_allowed && p.fast_order == 5 && knobs.io_dtype == 32 && knobs.n <= 7 &&
              p.slots_used_fast <= Stage<float>::PRE) ? 1 : 0;
    return p;
}

}  // namespace vfik
