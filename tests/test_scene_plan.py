"""The scene side of vfik_set_fields as pure host code (vfclik_amd/csrc/vfik_scene.h), on the CPU: tests/c_host/scene_plan.cpp -- built with
hipcc as host code, no GPU, no library -- packs field sets and prints what the batch's launches take for them.

THE DECISION TABLE (ROWS): a handle's knobs, one or more vfik_set_fields calls, and plan_scene's answer after each call, every branch of it.
The expected values were written down from the comments of plan_scene and pack_fields, row by row, and then held against the driver; each row
says in its name which comment it stands for, and MIXED says what those comments do not justify.  tests/test_gpu_scene_plan.py runs the rows marked `gpu` through real handles.

THE IMAGES: tests/golden/scene_images.npz holds two dozen seeded field sets (at most 5 arms, max_slots 0 ... 8, at most 10 fields an arm, every
field type, shuffled and repeated ids, NULL fields, arms without fields) and, for both I/O types, every staging image and per-arm result that
the pack_fields of commit cdee413 made of them -- the last commit that had the function inside vfik_abi.cpp.  tests/golden/make_scene_images.py
wrote it: it compiles that commit's vfik_abi.cpp into a driver of its own and calls the function there.  The comparison is byte for byte.
One exception, at max_slots 0 only: the general slots' staging image, which no call copies then, was one empty plane and is now two (the
table's number, which is also the device's) -- both are held to be all zeros.

THE PLANE TABLE and slots_needed: stated below."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELD = np.dtype([("id", "<i4"), ("type", "<i4"), ("force", "<f8"), ("p", "<f8", (17,))])   # vfik_field (vfclik_amd/_abi.py: FIELD_DTYPE)
NULL, ATTRACTOR, REPELLER, HEMISPHERE, FUNNEL = 0, 1, 2, 4, 5
IMAGES = ("goal", "aux", "slots", "compact", "uni", "orders", "repmap", "scenemaps")


def field(type_, id_, force, *p):
    return (id_, type_, force, tuple(p) + (0.0,) * (17 - len(p)))


def goal(id_=1):
    return field(ATTRACTOR, id_, 1.0, 1, 0, 0, 0.5, 0, 1, 0, 0.1, 0, 0, 1, 0.4, 0, 0, 0, 1, 0.05)


def rep(id_, safe=0.001, order=5.0, force=-10.0, radius=0.05):
    """a point obstacle as the feeder sends it (object_feeder:326-333): x y z radius safeDist order"""
    return field(REPELLER, id_, force, 0.3 + 0.01 * id_, -0.2, 0.4, radius, safe, order)


def funnel(id_, angle_order=10.0, dist_order=2.0):
    return field(FUNNEL, id_, 1.0, 0.5, 0.1, 0.4, 0, 0, 1, 0.5, angle_order, 0.3, dist_order)


def hemi(id_, order=5.0):
    return field(HEMISPHERE, id_, -10.0, 0.5, 0.1, 0.0, 0, 0, 1, 0.001, order)


def records(arms, max_fields=None):
    """(fields[n_arms][max_fields], counts[n_arms]) of lists of fields"""
    max_fields = max_fields or max([len(a) for a in arms] + [1])
    f = np.zeros((len(arms), max_fields), dtype=FIELD)
    for j, a in enumerate(arms):
        for k, fd in enumerate(a):
            f[j, k] = fd
    return f, np.array([len(a) for a in arms], dtype=np.int32)


def feeder(n, **kw):
    """goal + n point obstacles with the feeder's pair (0.001, -10) and order 5"""
    return [goal()] + [rep(4 + k, **kw) for k in range(n)]


def plan(slots, order, path, mixed=0, uni=1, one=0, pair="none", fast=None, aux=None, uni_ok=None):
    """the driver's line.  slots: slots_used (and slots_used_fast unless `fast`); order: fast_order; path: field_path; uni: what a launch is
    given (uni_ok: what the scene allows, where a knob makes them differ); one: the one-chunk body; pair: the batch's (safe, force)"""
    fast = slots if fast is None else fast
    aux = (1 if path == 2 else 0) if aux is None else aux
    uni_ok = uni if uni_ok is None else uni_ok
    return ("slots_used=%d slots_used_fast=%d any_funnel=%d fast_order=%s mixed=%d uni_ok=%d one5=%s pair=%s field_path=%d mixed_orders=%d uniform=%d one_chunk=%s"
            % (slots, fast, aux, order, mixed, uni_ok, one, pair, path, mixed, uni, one))


F32 = "0.0010000000474974513,-10"   # the feeder's pair as float32 I/O holds it
F64 = "0.001,-10"
GENERAL = dict(order=-1, path=0, uni=0)
# NOT PINNED ("*") on the rows whose orders differ: fast_order and the one-chunk bit.  The order planes are read there and a launch uses neither --
# the launch plan gives a MIXO launch no uniform image, hence no one-chunk body -- and the comments of plan_scene justify no value: fast_order
# is the order of the last arm that has ONE order, or the default 5 when the orders differ inside every arm that has repellers, and with that 5
# one5, hence vfik_one_chunk, can say 1 for a batch none of whose launches takes the body.  A finding of this table, left as it is.
MIXED = dict(order="*", one="*", mixed=1)
SAFE_A, SAFE_B = 0.001, 0.001 + 1e-12   # two safe distances that are one float32

# (name, knobs of the handle, calls [(first_arm, [arm's fields, ...]), ...], {io: [the plan after each call]}, gpu)
# knobs: nj (7), B (1), S (16), uni / mixed / one = VFIK_UNIFORM_IMAGE / VFIK_MIXED_ORDERS / VFIK_ONE_CHUNK (1)
ROWS = [
    # -- basic scenes --
    ("1 no field at all: `fo < 0 ? 5`, straight-line, uniform without a pair", {}, [(0, [[]])],
     {32: [plan(0, 5, 1, one=1)], 64: [plan(0, 5, 1)]}, True),
    ("2 goal only: the same", {}, [(0, [[goal()]])],
     {32: [plan(0, 5, 1, one=1)], 64: [plan(0, 5, 1)]}, True),
    ("3 the feeder's scene, goal + 8 obstacles: one chunk of order 5", {}, [(0, [feeder(8)])],
     {32: [plan(8, 5, 1, one=1, pair=F32)]}, True),
    ("3 ... at 6 joints", {"nj": 6}, [(0, [feeder(8)])],
     {32: [plan(8, 5, 1, one=1, pair=F32)]}, False),
    ("4 ... with 9 obstacles: more than Stage<float>::PRE", {}, [(0, [feeder(9)])],
     {32: [plan(9, 5, 1, pair=F32)]}, True),
    ("5 ... at float64: the one-chunk body is float32's", {}, [(0, [feeder(8)])],
     {64: [plan(8, 5, 1, pair=F64)]}, True),
    ("6 ... at 10 joints: chains of up to 7", {"nj": 10}, [(0, [feeder(8)])],
     {32: [plan(8, 5, 1, pair=F32)]}, False),
    ("7 ... with VFIK_ONE_CHUNK=0", {"one": 0}, [(0, [feeder(8)])],
     {32: [plan(8, 5, 1, pair=F32)]}, True),
    ("8 ... with VFIK_UNIFORM_IMAGE=0: the scene allows the image, no launch reads it", {"uni": 0}, [(0, [feeder(8)])],
     {32: [plan(8, 5, 1, uni=0, uni_ok=1, pair=F32)]}, True),
    ("9 order 4 everywhere", {}, [(0, [feeder(3, order=4.0)])],
     {32: [plan(3, 4, 1, pair=F32)], 64: [plan(3, 4, 1, pair=F64)]}, True),
    ("10 orders that differ inside one arm: the order planes", {}, [(0, [[goal(), rep(4), rep(5, order=20.0)]])],
     {32: [plan(2, path=1, pair=F32, **MIXED)], 64: [plan(2, path=1, pair=F64, **MIXED)]}, True),
    ("11 orders that differ between two arms", {"B": 2}, [(0, [feeder(2), feeder(2, order=4.0)])],
     {32: [plan(2, path=1, pair=F32, **MIXED)]}, False),
    ("11 ... with an arm without repellers between them", {"B": 3}, [(0, [feeder(2), [goal()], feeder(1, order=4.0)])],
     {32: [plan(2, path=1, pair=F32, **MIXED)]}, False),
    ("12 row 10 with VFIK_MIXED_ORDERS=0: general", {"mixed": 0}, [(0, [[goal(), rep(4), rep(5, order=20.0)]])],
     {32: [plan(2, **GENERAL)]}, True),
    ("12 row 11 with VFIK_MIXED_ORDERS=0: general", {"B": 2, "mixed": 0}, [(0, [feeder(2), feeder(2, order=4.0)])],
     {32: [plan(2, **GENERAL)]}, False),
    ("13 a non-integer order", {}, [(0, [[goal(), rep(4), rep(5, order=2.5)]])],
     {32: [plan(2, **GENERAL)], 64: [plan(2, **GENERAL)]}, True),
    ("14 order 128: the byte holds [0, 128)", {}, [(0, [[goal(), rep(4, order=128.0)]])],
     {32: [plan(1, **GENERAL)]}, False),
    ("14 ... and 127 is an order", {}, [(0, [[goal(), rep(4, order=127.0)]])],
     {32: [plan(1, 127, 1, pair=F32)]}, False),
    ("15 a negative order", {}, [(0, [[goal(), rep(4, order=-1.0)]])],
     {32: [plan(1, **GENERAL)]}, False),
    ("16 order 0 everywhere: straight-line, `not with decay order 0`", {}, [(0, [feeder(2, order=0.0)])],
     {32: [plan(2, 0, 1, uni=0)], 64: [plan(2, 0, 1, uni=0)]}, True),
    # -- the pair --
    ("17 two arms whose pairs differ", {"B": 2}, [(0, [feeder(2), feeder(2, force=-5.0)])],
     {32: [plan(2, 5, 1, uni=0)]}, False),
    ("18 one arm whose own repellers differ in safe distance", {}, [(0, [[goal(), rep(4), rep(5, safe=0.002)]])],
     {32: [plan(2, 5, 1, uni=0)], 64: [plan(2, 5, 1, uni=0)]}, True),
    ("19 a repeller with radius + safe < 0: the uniform kernel clamps that sum", {}, [(0, [[goal(), rep(4, safe=-0.1), rep(5, safe=-0.1)]])],
     {32: [plan(2, 5, 1, uni=0)]}, False),
    ("20 two safe distances that round to one float32: compared as the device sees them", {}, [(0, [[goal(), rep(4, safe=SAFE_A), rep(5, safe=SAFE_B)]])],
     {32: [plan(2, 5, 1, one=1, pair=F32)]}, False),
    ("21 the same two at float64", {}, [(0, [[goal(), rep(4, safe=SAFE_A), rep(5, safe=SAFE_B)]])],
     {64: [plan(2, 5, 1, uni=0)]}, False),
    ("21 ... in two arms", {"B": 2}, [(0, [[goal(), rep(4, safe=SAFE_A)], [goal(), rep(4, safe=SAFE_B)]])],
     {32: [plan(1, 5, 1, one=1, pair=F32)], 64: [plan(1, 5, 1, uni=0)]}, False),
    # -- scene classes --
    ("22 one funnel with integer orders: the aux block", {}, [(0, [[goal(), funnel(2), rep(4)]])],
     {32: [plan(3, 5, 2, fast=1, one=1, pair=F32)]}, False),
    ("23 a funnel with a non-integer order", {}, [(0, [[goal(), funnel(2, dist_order=0.5), rep(4)]])],
     {32: [plan(3, fast=1, aux=1, **GENERAL)]}, False),
    ("24 a second funnel", {}, [(0, [[goal(), funnel(2), funnel(3), rep(4)]])],
     {32: [plan(5, fast=1, aux=1, **GENERAL)]}, False),
    ("25 one hemisphere", {}, [(0, [[goal(), hemi(3), rep(4)]])],
     {32: [plan(3, 5, 2, fast=1, one=1, pair=F32)], 64: [plan(3, 5, 2, fast=1, pair=F64)]}, True),
    ("25 ... with a non-integer order", {}, [(0, [[goal(), hemi(3, order=1.5), rep(4)]])],
     {32: [plan(3, fast=1, aux=1, **GENERAL)]}, False),
    ("25 ... a funnel and a hemisphere, orders that differ", {}, [(0, [[goal(), funnel(2), hemi(3), rep(4), rep(5, order=4.0)]])],
     {32: [plan(6, path=2, fast=2, pair=F32, **MIXED)]}, False),
    ("26 a second attractor behind the goal", {}, [(0, [[goal(), goal(2), rep(4)]])],
     {32: [plan(4, fast=1, **GENERAL)]}, False),
    ("27 a funnel in front of the repellers: general slots count it, compact slots do not", {"B": 2}, [(0, [[goal(), funnel(2), rep(4), rep(5)], feeder(3)])],
     {32: [plan(4, 5, 2, fast=3, one=1, pair=F32)], 64: [plan(4, 5, 2, fast=3, pair=F64)]}, True),
    # -- sequences: a partial call changes the batch's answer --
    ("28-29 whole batch uniform; one arm re-set with another pair: off; re-set with the batch's pair: on again", {"B": 3},
     [(0, [feeder(8)] * 3), (1, [feeder(8, force=-5.0)]), (1, [feeder(4)])],
     {32: [plan(8, 5, 1, one=1, pair=F32), plan(8, 5, 1, uni=0), plan(8, 5, 1, one=1, pair=F32)],
      64: [plan(8, 5, 1, pair=F64), plan(8, 5, 1, uni=0), plan(8, 5, 1, pair=F64)]}, True),
    ("30 whole batch order 5; one arm re-set with no repeller: unchanged", {"B": 3},
     [(0, [feeder(8)] * 3), (2, [[goal()]])],
     {32: [plan(8, 5, 1, one=1, pair=F32)] * 2, 64: [plan(8, 5, 1, pair=F64)] * 2}, True),
    ("30 ... the only arm with repellers re-set without: the default order again, no pair", {"B": 2},
     [(0, [feeder(2, order=4.0), [goal()]]), (0, [[goal()]])],
     {32: [plan(2, 4, 1, pair=F32), plan(0, 5, 1, one=1)]}, False),
]


def request(knobs, io, calls):
    k = dict(nj=7, B=1, S=16, uni=1, mixed=1, one=1)
    k.update(knobs)
    sets = []
    for first, arms in calls:
        f, counts = records(arms)
        sets.append("set=%d,%d,%d,%s,%s" % (first, len(arms), f.shape[1], counts.tobytes().hex(), f.tobytes().hex()))
    return "io=%d %s %s" % (io, " ".join("%s=%d" % kv for kv in k.items()), " ".join(sets))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path_factory.mktemp("scene_plan") / "scene_plan")
    subprocess.check_call([hipcc, "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "c_host", "scene_plan.cpp"), "-o", exe])
    return exe


def ask(driver, mode, requests):
    r = subprocess.run([driver, mode], input="\n".join(requests) + "\n", capture_output=True, text=True, timeout=60, check=True)
    return r.stdout.splitlines()


def test_every_row_of_the_decision_table(driver):
    cases = [(name, io, request(knobs, io, calls), " | ".join(want)) for name, knobs, calls, wants, _ in ROWS for io, want in sorted(wants.items())]
    got = ask(driver, "plan", [c[2] for c in cases])
    assert len(got) == len(cases)
    same = lambda want, g: len(want.split()) == len(g.split()) and all(w == t or w.endswith("=*") and t.startswith(w[:-1]) for w, t in zip(want.split(), g.split()))
    diff = ["%s (float%d)\n    want %s\n    got  %s" % (name, io, want, g) for (name, io, _, want), g in zip(cases, got) if not same(want, g)]
    assert not diff, "\n".join(diff)


def test_the_table_reaches_every_branch():
    """every value of every member of the plan, and every row the issue of this table names"""
    lines = [w for *_, wants, _ in ROWS for want in wants.values() for w in want]
    for frag in ("fast_order=-1", "fast_order=0", "fast_order=4", "fast_order=5", "fast_order=127", "mixed=1", "uni_ok=0", "uni_ok=1 one5=0", "one5=1", "pair=none", "any_funnel=1",
                 "field_path=0", "field_path=1", "field_path=2", "uni_ok=1 one5=0 pair=%s field_path=1 mixed_orders=0 uniform=0" % F32):
        assert any(frag in ln for ln in lines), frag
    numbers = {name.split()[0] for name, *_ in ROWS}
    assert numbers >= {str(n) for n in range(1, 28)} | {"28-29", "30"}
    assert sum(1 for *_, gpu in ROWS if gpu) >= 12


def test_the_images_are_the_parents_byte_for_byte(driver):
    z = np.load(os.path.join(ROOT, "tests", "golden", "scene_images.npz"))
    shapes, fields, counts = z["shapes"], z["fields"], z["counts"]
    assert len(shapes) >= 24 and shapes[:, 1].max() <= 5 and shapes[:, 0].max() <= 8 and shapes[:, 2].max() <= 10
    assert set(fields["type"].tolist()) == {NULL, ATTRACTOR, REPELLER, HEMISPHERE, FUNNEL} and 0 in counts.tolist()
    reqs, at_f, at_c = [], 0, 0
    for S, n_arms, max_fields in shapes:
        f, c = fields[at_f:at_f + n_arms * max_fields], counts[at_c:at_c + n_arms]
        at_f, at_c = at_f + n_arms * max_fields, at_c + n_arms
        reqs.append("S=%d n_arms=%d max_fields=%d counts=%s fields=%s" % (S, n_arms, max_fields, c.tobytes().hex(), f.tobytes().hex()))
    for io in (32, 64):
        got = ask(driver, "pack", ["io=%d %s" % (io, r) for r in reqs])
        assert len(got) == 9 * len(shapes)
        blob, lengths, arms = z["images%d" % io].tobytes(), z["lengths%d" % io], z["arms%d" % io]
        at, at_a = 0, 0
        for i, (S, n_arms, _) in enumerate(shapes):
            for k, name in enumerate(IMAGES):
                want = blob[at:at + lengths[i, k]]
                at += lengths[i, k]
                tag, _, hexed = got[9 * i + k].partition(" ")
                assert tag == name
                if name == "slots" and S == 0:   # (never copied at max_slots 0: see the module's docstring)
                    assert not any(want) and not any(bytes.fromhex(hexed)) and len(hexed) // 2 == 2 * len(want)
                    continue
                assert bytes.fromhex(hexed) == want, "scene %d float%d: image %s" % (i, io, name)
            # the arms' results, value for value: slots, compact slots, aux, pair state, safe, force; then the order class against classify_arm's
            # code of old (-1 no repeller, n >= 0 that integer order, -3 integer orders that differ, -2 general)
            tag, _, rest = got[9 * i + 8].partition(" ")
            assert tag == "arms"
            new = [[float(v) for v in a.split(",")] for a in rest.split()]
            assert len(new) == n_arms
            for a, old in zip(new, arms[at_a:at_a + n_arms]):
                assert a[:6] == old[:6].tolist(), "scene %d float%d" % (i, io)
                assert {0: -1, 1: a[7], 2: -3, 3: -2}[int(a[6])] == old[6], "scene %d float%d" % (i, io)
            at_a += n_arms
        assert at == len(blob) and at_a == len(arms)


def test_the_plane_table(driver):
    """Planes of each image for max_slots S, with S1 = max(1, S) (an image is never empty: the prefetch reads slot 0): goal 4, aux 6, general 2 S1,
    compact 3 ceil(S1 / 2), uniform 1 + max(S1, PRE) with PRE = 8 for float32 and 4 for float64 (of which a call stages the S1 slot planes), order
    planes ceil(S1 / 16), repeller map ceil(S1 / 8), scene maps 3 ceil(S1 / 8); a quad per arm and plane in the first five, 16 bytes in the others."""
    cases = [(io, S) for io in (32, 64) for S in (0, 1, 2, 7, 8, 15, 16, 17)]
    got = ask(driver, "planes", ["io=%d S=%d" % c for c in cases])
    for (io, S), line in zip(cases, got):
        S1, quad, pre = max(1, S), 4 * io // 8, 8 if io == 32 else 4
        want = {"goal": (4, 4, quad), "aux": (6, 6, quad), "slots": (2 * S1, 2 * S1, quad), "compact": (3 * -(-S1 // 2), 3 * -(-S1 // 2), quad),
                "uni": (1 + max(S1, pre), S1, quad), "orders": (-(-S1 // 16), -(-S1 // 16), 16), "repmap": (-(-S1 // 8), -(-S1 // 8), 16),
                "scenemaps": (3 * -(-S1 // 8), 3 * -(-S1 // 8), 16)}
        assert {k: tuple(int(x) for x in v.split(",")) for k, v in (t.split("=") for t in line.split())} == want, (io, S)


def test_slots_needed_refuses_what_set_fields_refuses(driver):
    """the goal rule: the first attractor is free, every other primitive takes slots_of(type); an unknown type is named by its index"""
    def need(arm):
        f, _ = records([arm])
        return ask(driver, "slots", ["fields=%s" % f[0, :len(arm)].tobytes().hex()])[0]
    assert need([]) == "need=0 bad=-1"
    assert need([goal(), field(NULL, 0, 0.0)]) == "need=0 bad=-1"
    assert need(feeder(16)) == "need=16 bad=-1"
    assert need(feeder(17)) == "need=17 bad=-1"                              # one more than a handle of 16 slots has: vfik_set_fields refuses
    assert need([rep(4), goal(9), goal(1), funnel(2), hemi(3)]) == "need=8 bad=-1"   # 1 + 0 + 3 + 2 + 2: the FIRST attractor, whatever its id
    assert need([goal(), rep(4), field(3, 7, 1.0), field(9, 8, 1.0)]) == "need=-1 bad=2"
    # ... and the plan mode, which validates as vfik_set_fields does, stops at such a call
    f17 = request({}, 32, [(0, [feeder(2)]), (0, [feeder(17)])])
    bad = request({}, 32, [(0, [[goal(), field(3, 7, 1.0)]])])
    got = ask(driver, "plan", [f17, bad])
    assert got[0].startswith("slots_used=2 ") and got[0].endswith(" | call 1 refused") and got[1] == "call 0 refused"
