"""tests/guard_arena.py on CPU tensors: every kind of stray store it is for is reported at the right region, side and offset, a
stand-in kernel that reads behind its input is caught by the nan-against-huge comparison, the layout is what the module promises, and
the coverage table names exactly the functions include/vfik.h declares.

The stated limit: a store that writes exactly the bytes already there cannot be seen (test_a_store_of_the_same_bytes_is_the_limit)."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guard_arena as ga  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, N = 205, 7     # 205 arms x 7 floats: 5740 bytes, a 12-byte tail behind the last whole 16-byte piece


def _arena(fill="nan", skew=0, seed=3):
    a = ga.Arena("cpu", seed, fill=fill)
    a.carve("q", (B, N), np.float32, "in", skew)
    a.carve("qdot_out", (B, N), np.float32, "out", skew)
    a.carve("pose", (B, 16), np.float64, "out", skew)
    a.carve("status", (B,), np.int32, "out", skew)
    a.put("q", np.random.default_rng(seed).uniform(-1, 1, (B, N)))
    return a


def _poke(a, name, offset, data):
    """Store bytes at ``offset`` from the region's start, as a kernel that got an address wrong would."""
    import torch
    r = a.regions[name]
    d = np.frombuffer(bytes(data), dtype=np.uint8).copy()
    a.buf[r.start + offset:r.start + offset + len(d)] = torch.from_numpy(d)


def _other(a, name, offset, n):
    """n bytes that all differ from what the arena holds there"""
    r = a.regions[name]
    now = a.buf[r.start + offset:r.start + offset + n].numpy()
    return (now ^ 0x5A).tobytes()


def test_untouched_arena_is_intact():
    for skew in (0, 1):
        a = _arena(skew=skew)
        a.regions["qdot_out"].view[:] = 1.5    # a well-behaved kernel: every output written, nothing else
        a.regions["pose"].view[:] = -2.0
        a.regions["status"].view[:] = 7
        assert a.damaged() == []


def test_four_bytes_right_behind_the_end():
    a = _arena()
    n = a.regions["qdot_out"].nbytes
    _poke(a, "qdot_out", n, _other(a, "qdot_out", n, 4))
    assert a.damaged() == [{"region": "qdot_out", "side": "behind", "first": 0, "last": 3, "count": 4}]


def test_a_16_byte_store_over_the_12_byte_tail():
    a = _arena()
    n = a.regions["qdot_out"].nbytes
    assert n == 5740 and n % 16 == 12
    _poke(a, "qdot_out", n - 12, _other(a, "qdot_out", n - 12, 16))    # the last piece of the array, requested whole
    assert a.damaged() == [{"region": "qdot_out", "side": "behind", "first": 0, "last": 3, "count": 4}]


def test_one_element_in_front_of_the_start():
    for name, size in (("qdot_out", 4), ("pose", 8), ("status", 4)):
        a = _arena(skew=1)
        _poke(a, name, -size, _other(a, name, -size, size))
        assert a.damaged() == [{"region": name, "side": "front", "first": -size, "last": -1, "count": size}]


def test_a_tile_one_wave_further_on():
    a = _arena()
    r = a.regions["status"]
    at = (B // 64 + 1) * 64 * 4       # the wave behind the batch's last, partial one: rows 256..511 of int32
    assert at >= r.nbytes
    _poke(a, "status", at, _other(a, "status", at, 1024))
    assert a.damaged() == [{"region": "status", "side": "behind", "first": at - r.nbytes, "last": at - r.nbytes + 1023, "count": 1024}]
    # and the largest tile there is, 64 rows of 16 doubles, one wave too far at the end of a full last wave: still inside the band
    a = ga.Arena("cpu", 5)
    a.carve("pose", (192, 16), np.float64, "out")
    n = a.regions["pose"].nbytes
    _poke(a, "pose", n, _other(a, "pose", n, ga.TILE_BYTES))
    assert a.damaged() == [{"region": "pose", "side": "behind", "first": 0, "last": ga.TILE_BYTES - 1, "count": ga.TILE_BYTES}]
    assert ga.TILE_BYTES < ga.BAND


def test_zeros_in_the_middle_of_a_band():
    for fill in ("nan", "huge"):
        a = _arena(fill=fill)
        n = a.regions["q"].nbytes
        _poke(a, "q", n + 8000, bytes(64))          # behind an input: the band is all 0xFF or all 0x7F
        assert a.damaged() == [{"region": "q", "side": "behind", "first": 8000, "last": 8063, "count": 64}]
    a = _arena()
    _poke(a, "pose", -8192, bytes(4096))            # in front of an output: the fill has a zero byte once in 256
    (rec,) = a.damaged()
    assert (rec["region"], rec["side"]) == ("pose", "front")
    assert -8192 <= rec["first"] <= -8192 + 8 and -4096 - 8 <= rec["last"] <= -4097 and 4096 * 0.98 < rec["count"] <= 4096


def test_a_copy_of_another_band():
    import torch
    a = _arena()
    src, dst = a.regions["qdot_out"], a.regions["pose"]
    a.buf[dst.back[0]:dst.back[1]] = a.buf[src.back[0]:src.back[1]].clone()
    (rec,) = a.damaged()
    assert (rec["region"], rec["side"]) == ("pose", "behind")
    assert rec["first"] <= 8 and rec["last"] >= ga.BAND - 8 and rec["count"] > ga.BAND * 0.98
    # and the same fill at another seed is another fill
    b = ga.Arena("cpu", 4)
    b.carve("q", (B, N), np.float32, "out")
    assert not torch.equal(a.buf[:1024], b.buf[:1024])


def test_a_store_into_an_input_is_reported():
    a = _arena()
    _poke(a, "q", 28, _other(a, "q", 28, 4))
    assert a.damaged() == [{"region": "q", "side": "inside", "first": 28, "last": 31, "count": 4}]


def test_a_store_of_the_same_bytes_is_the_limit():
    a = _arena()
    r = a.regions["qdot_out"]
    _poke(a, "qdot_out", r.nbytes, a.buf[r.end:r.end + 16].numpy().tobytes())
    assert a.damaged() == []


def _reads_behind(q, out):
    """A stand-in kernel: out[b] = sum of row b of q, and -- the bug -- the last arm's sum runs one element over q's end."""
    import torch
    flat = torch.as_strided(q, (q.numel() + 1,), (1,))
    out[:] = q.sum(dim=1)
    out[-1] += flat[q.numel()]


def test_a_read_behind_the_input_differs_between_nan_and_huge():
    got = {}
    for fill in ("nan", "huge"):
        a = ga.Arena("cpu", 9, fill=fill)
        q = a.carve("q", (B, N), np.float32, "in")
        out = a.carve("out", (B,), np.float32, "out")
        a.put("q", np.random.default_rng(1).uniform(-1, 1, (B, N)))
        _reads_behind(q, out)
        assert a.damaged() == []             # (a read damages nothing: only the comparison can see it)
        got[fill] = a.bytes_of("out")
    assert not np.array_equal(got["nan"], got["huge"])
    assert np.array_equal(got["nan"][:-4], got["huge"][:-4])
    # the honest kernel is equal under both fills, and equal to a run on arrays of their own
    res = []
    for fill in ("nan", "huge", None):
        a = ga.Arena("cpu", 9, fill=fill or "nan")
        q = a.carve("q", (B, N), np.float32, "in")
        out = a.carve("out", (B,), np.float32, "out")
        a.put("q", np.random.default_rng(1).uniform(-1, 1, (B, N)))
        if fill is None:
            q, out = a.plain_copy("q"), a.plain_copy("out")
            assert np.array_equal(ga.raw_bytes(out), a.initial_bytes("out"))
        out[:] = q.sum(dim=1)
        res.append(ga.raw_bytes(out) if fill is None else a.bytes_of("out"))
    assert np.array_equal(res[0], res[1]) and np.array_equal(res[0], res[2])


def test_fills_are_what_the_module_says():
    for fill, byte in (("nan", 0xFF), ("huge", 0x7F)):
        a = _arena(fill=fill)
        r = a.regions["q"]
        band = a.buf[r.back[0]:r.back[1]].numpy()
        assert (band == byte).all() and (a.buf[r.front[0]:r.front[1]].numpy() == byte).all()
        f32, f64, i32 = band[:16].view(np.float32), band[:16].view(np.float64), band[:16].view(np.int32)
        if fill == "nan":
            assert np.isnan(f32).all() and np.isnan(f64).all() and (i32 == -1).all()
        else:
            assert np.allclose(f32, 3.39e38, rtol=1e-2) and np.allclose(f64, 1.38e306, rtol=1e-2) and (i32 == 0x7F7F7F7F).all()
    # output regions and their bands: the position-dependent fill, the same under both
    a, b = _arena("nan"), _arena("huge")
    for name in ("qdot_out", "pose", "status"):
        r = a.regions[name]
        assert np.array_equal(a.buf[r.front[0]:r.back[1]].numpy(), b.buf[r.front[0]:r.back[1]].numpy())
        assert np.array_equal(a.bytes_of(name), np.frombuffer(np.random.default_rng(3).bytes(a.capacity), np.uint8)[r.start:r.end])


@pytest.mark.parametrize("skew", (0, 1))
def test_layout(skew):
    a = _arena(skew=skew)
    spans = []
    for r in a.regions.values():
        assert r.front == (r.start - ga.BAND, r.start) and r.back == (r.end, r.end + ga.BAND)
        assert 0 <= r.front[0] and r.back[1] <= a.capacity == a.buf.numel()
        assert r.view.is_contiguous() and tuple(r.view.shape) == r.shape and r.view.element_size() == r.dtype.itemsize
        assert r.view.data_ptr() == a.buf.data_ptr() + r.start
        assert r.view.data_ptr() % 16 == skew * r.dtype.itemsize and r.view.data_ptr() % r.dtype.itemsize == 0
        spans.append((r.front[0], r.back[1]))
    for (a0, a1), (b0, b1) in zip(spans, spans[1:]):
        assert a1 <= b0, "bands of two regions overlap"
    assert a.band_bytes() == 4 * 2 * ga.BAND + a.regions["q"].nbytes
    # the comparison run's array: allocated on its own, aligned, the same bytes
    p = a.plain_copy("pose")
    assert p.data_ptr() % 16 == 0 and not a.buf.data_ptr() <= p.data_ptr() < a.buf.data_ptr() + a.capacity
    assert tuple(p.shape) == a.regions["pose"].shape and np.array_equal(ga.raw_bytes(p), a.initial_bytes("pose"))
    # both skews start from the same arrays, at places that do not depend on the skew of the regions in front
    b = _arena(skew=0)
    for name, r in a.regions.items():
        assert r.start - b.regions[name].start == skew * r.dtype.itemsize and np.array_equal(a.initial_bytes(name), b.initial_bytes(name))


def test_skew_on_a_16_byte_argument_is_refused():
    a = ga.Arena("cpu", 0)
    for arg in ("way16", "rep4", "pts4", "link_traj"):
        with pytest.raises(ValueError, match="16-byte aligned"):
            a.carve(arg, (4, 3, 16), np.float32, "in", skew=1)
        with pytest.raises(ValueError, match="16-byte aligned"):
            a.carve("x_" + arg, (4, 3, 4), np.float64, "out", skew=1, arg=arg)
        a.carve(arg, (4, 3, 16), np.float32, "in", skew=0)
    assert sorted(ga.ALIGN16) == ["link_traj", "pts4", "rep4", "way16"]
    with pytest.raises(ValueError, match="full"):
        ga.Arena("cpu", 0, capacity=40000).carve("big", (10000,), np.float32, "out")


def test_align16_is_what_the_header_says():
    """Every argument the header wants 16-byte aligned is in ALIGN16, and nothing else is."""
    hdr = open(os.path.join(ROOT, "include", "vfik.h")).read()
    named = set(re.findall(r"\b(\w+\d) not 16-byte aligned", hdr))
    assert named == {"way16", "rep4", "pts4"}, named
    assert named | {"link_traj"} == set(ga.ALIGN16)


def test_coverage_table_names_exactly_the_headers_functions():
    hdr = open(os.path.join(ROOT, "include", "vfik.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    names = set(re.findall(r"\b(vfik_[a-z0-9_]+)\s*\(", hdr))       # (the expression of tests/test_abi_symbols.py)
    assert len(names) >= 20
    both = set(ga.GUARDED) & set(ga.EXEMPT)
    assert not both, "in GUARDED and in EXEMPT: %s" % sorted(both)
    table = set(ga.GUARDED) | set(ga.EXEMPT)
    assert names - table == set(), "entry points without a guard case or a reason: %s" % sorted(names - table)
    assert table - names == set(), "not in include/vfik.h: %s" % sorted(table - names)
    for k, why in ga.EXEMPT.items():
        assert isinstance(why, str) and len(why) > 20 and "\n" not in why, k
    # every guard case is a test of tests/test_gpu_extents.py
    src = open(os.path.join(ROOT, "tests", "test_gpu_extents.py")).read()
    for k, cases in ga.GUARDED.items():
        assert cases, k
        for c in cases:
            assert re.search(r"^def %s\(" % re.escape(c), src, flags=re.M), "%s: no test %s in tests/test_gpu_extents.py" % (k, c)
    # every device form is guarded: a function with a _host twin takes device pointers
    for n in names:
        if n.endswith("_host") and n[:-5] in names and n[:-5] not in ("vfik_stalled", "vfik_waited"):
            assert n[:-5] in ga.GUARDED, n[:-5]
