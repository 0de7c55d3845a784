"""vfik_link_avoid on the GPU (include/vfik.h; avoid_kernel, vfclik_amd/csrc/vfik_aux.hip) against the 50-digit command of tests/hp_avoid.py,
in both I/O types.

Chains: the four of hp_links.ROBOTS.  Per chain and I/O type the six shared cases of hp_avoid.CASES -- batches of 1, 65 and 203 arms, counts
1, 5, 16 and 32, rows from the device's own link_points of the partner, the arm's own links under a mask, static spheres with every fifth
row NaN, rows outside the window that would push hard if read, d0 so that about half of the arms have an active pair -- and the edge batch
of hp_avoid.edge_case.  With 14 and 10 joints, 16 and 32 rows the kernel leaves the rows in memory; elsewhere it stages them.

THE BAR: hp_avoid.K_MARGIN units beyond half an ulp of the output type; the unit is hp_avoid's (the walk's n u reach through the 1 / d0 and
a / s sensitivities of each active pair and the lever |P_i - o_k|).  Where the unit is 0 -- no active pair, a NaN in q -- the row is exactly
zero.  The host form equals the device form bit for bit.

With VFIK_AVOID_TABLE=<file> the measured worst ratios are also written there (the record kept in profiles/avoid_accuracy.txt)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hp_avoid as ha  # noqa: E402
import hp_links as hl  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import __graft_entry__ as g
    g.build()
    import torch
    from vfclik_amd import _abi, engine, synth

    class E:
        pass

    e = E()
    e.engine, e.torch, e.abi, e.synth = engine, torch, _abi, synth
    e.dev = torch.device("cuda", 0)
    e.table = []
    yield e
    path = os.environ.get("VFIK_AVOID_TABLE")
    if path and e.table:
        with open(path, "a") as f:
            f.write("".join(e.table))


def _dev(env, a, dtype):
    return env.torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(env.dev)


def _both_forms(env, eng, c):
    """the command (B, n) float64 of the host form, after holding the device form to it bit for bit"""
    t = eng.io_dtype.type
    kw = ha.call_args(c)
    host = eng.link_avoid_host(c["q"], c["pts"], **kw)
    dkw = dict(kw, scale=None if kw["scale"] is None else _dev(env, kw["scale"], t))
    out = eng.link_avoid(_dev(env, c["q"], t), _dev(env, c["pts"], t), **dkw)
    eng.sync()
    out = out.cpu().numpy()
    assert out.dtype == eng.io_dtype and out.shape == host.shape and np.array_equal(out.astype(np.float64), host)
    assert np.array_equal(host.astype(t).astype(np.float64), host)   # I/O-typed values, widened
    return host


def _hold(got, ref, io_dtype, what):
    assert np.isfinite(got).all(), what
    assert np.all(got[ref["unit"] == 0] == 0), what                   # arms without a pair, arms with a NaN in q: zeros
    err, bar = ha.error(got, ref), ha.bar(ref, io_dtype)
    assert np.all(err <= bar), (what, float((err / bar).max()))


@pytest.mark.parametrize("robot", hl.ROBOTS)
@pytest.mark.parametrize("io_dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_against_50_digits(env, robot, io_dtype):
    chain = hl.chain_of(robot)
    for case in ha.CASES:
        B, kind, count, first, rows = case
        spheres = hl.sphere_list(chain, kind)
        eng = env.engine.Engine(chain, B, io_dtype=io_dtype, max_slots=16)
        eng.set_link_spheres(spheres)
        c = ha.make_case(robot, io_dtype, *case, place=lambda q, src, x: eng.link_points_host(q, src, x))
        ref = ha.avoid(chain, spheres, c["q"], c["pts"], **ha.call_args(c))
        got = _both_forms(env, eng, c)
        eng.close()
        line = "%-10s %-7s %-30s d0 = %.4f  %3d of %3d arms active; worst %.3f units\n" % (
            robot, np.dtype(io_dtype).name, case, c["d0"], ref["active"].sum(), B, ha.worst_units(got, ref, io_dtype))
        print(line, end="")
        env.table.append(line)
        assert 3 * ref["active"].sum() >= B and (B == 1 or not ref["active"].all())
        assert np.all(got[~ref["active"] & (ref["unit"] == 0).all(axis=1)] == 0)
        _hold(got, ref, io_dtype, case)


@pytest.mark.parametrize("io_dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_edges(env, io_dtype):
    chain = ha.edge_chain()
    eng = env.engine.Engine(chain, len(ha.EDGE_ARMS), io_dtype=io_dtype, max_slots=16)
    c = ha.edge_case(io_dtype)
    eng.set_link_spheres(c["spheres"])
    c = ha.edge_case(io_dtype, place=lambda q, src, x: eng.link_points_host(q, src, x))
    ref = ha.avoid(chain, c["spheres"], c["q"], c["pts"], **ha.call_args(c))
    got = _both_forms(env, eng, c)
    line = "%-10s %-7s %-30s d0 = %.4f  %3d of %3d arms active; worst %.3f units\n" % (
        "edge6", np.dtype(io_dtype).name, "edges", c["d0"], ref["active"].sum(), len(ha.EDGE_ARMS), ha.worst_units(got, ref, io_dtype))
    print(line, end="")
    env.table.append(line)
    _hold(got, ref, io_dtype, "edges")
    arm = ha.EDGE_ARMS.index
    for name in ("nan_q", "scale_zero", "no_rows"):
        assert np.all(got[arm(name)] == 0), name
    for name in ("at_d0", "penetrating", "coincident", "prismatic_tail", "general"):
        assert np.any(got[arm(name)] != 0), name
    assert np.all(got[arm("prismatic_tail"), 4:] != 0)
    # a sphere on link 0 moves no joint: with that sphere alone every row is zero
    only0 = dict(c, mask=np.array([7, 0, 0], dtype=np.uint32))
    assert np.all(_both_forms(env, eng, only0) == 0)
    eng.close()


@pytest.mark.parametrize("io_dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_channel_then_step_equals_set_ext_cmd(env, io_dtype):
    """[link_avoid(channel = 4); step] against [set_ext_cmd(4, out); step], bit for bit -- and the channel does reach qdot_out"""
    case = (65, "five", 5, 3, "static")
    c = ha.make_case("lwr", io_dtype, *case)
    chain, B, t = c["chain"], 65, np.dtype(io_dtype).type
    params = env.abi.default_params(flags=env.abi.F_NULLSPACE | env.abi.F_MIXER, mix_w=[1.0, 1.0, 0.0, 0.0, 1.0, 0.0])
    w = env.synth.make_workload(chain, B, 2, seed=4, io_dtype=io_dtype)
    eng = env.engine.Engine(chain, B, io_dtype=io_dtype, max_slots=8, params=params)
    eng.set_fields(w["fields"], w["nfields"])
    eng.set_link_spheres(c["spheres"])
    kw = ha.call_args(c)
    kw["scale"] = _dev(env, kw["scale"], t)
    q, pts = _dev(env, c["q"], t), _dev(env, c["pts"], t)

    def step():
        eng.reset_state()                                              # (the nullspace module keeps state from cycle to cycle)
        return eng.step_host(c["q"], want=("qdot_out",))["qdot_out"]   # (step_host synchronises the engine's stream)

    with pytest.raises(env.engine.VfikError, match="ext buffer"):      # nothing allocated the ext buffer yet
        eng.link_avoid(q, pts, channel=4, **kw)
    eng.set_ext_cmd(4, np.zeros((B, chain.n)))                         # allocates it, all zero
    zero = step()
    out = eng.link_avoid(q, pts, channel=4, **kw)
    pushed = step()
    cmd = out.cpu().numpy()
    assert np.any(cmd != 0) and not np.array_equal(pushed, zero)
    again = eng.link_avoid(q, pts, out=None, channel=3, **kw)          # another channel, weight 0: the same command, qdot_out as it was
    assert np.array_equal(step(), pushed)
    assert np.array_equal(again.cpu().numpy(), cmd)
    eng.set_ext_cmd(3, None)
    eng.set_ext_cmd(4, None)
    assert np.array_equal(step(), zero)
    eng.set_ext_cmd(4, cmd)
    assert np.array_equal(step(), pushed)
    eng.close()


def test_refusals(env):
    c = ha.make_case("lwr", np.float32, 65, "five", 5, 3, "static")
    eng = env.engine.Engine(c["chain"], 65, io_dtype=np.float32, max_slots=16)
    E = env.engine.VfikError
    kw = dict(first=3, count=5, gain=1.0, d0=0.1)
    with pytest.raises(E, match="no link spheres"):
        eng.link_avoid_host(c["q"], c["pts"], **kw)
    eng.set_link_spheres(c["spheres"])
    for first, count in ((3, 0), (3, 33), (-1, 5), (6, 5)):
        with pytest.raises(E):
            eng.link_avoid_host(c["q"], c["pts"], **dict(kw, first=first, count=count))
    for bad in (dict(d0=0.0), dict(d0=-0.1), dict(d0=np.inf), dict(d0=np.nan), dict(gain=np.inf), dict(gain=np.nan)):
        with pytest.raises(E):
            eng.link_avoid_host(c["q"], c["pts"], **dict(kw, **bad))
    with pytest.raises(E, match="at or beyond count"):
        eng.link_avoid_host(c["q"], c["pts"], mask=np.array([1, 1, 1 << 5, 1, 1], dtype=np.uint32), **kw)
    t = env.torch
    q, pts = _dev(env, c["q"], np.float32), _dev(env, c["pts"], np.float32)
    odd = t.empty(pts.numel() + 2, dtype=t.float32, device=env.dev)[2:].view(pts.shape)   # 8 bytes off a 16-byte boundary
    odd.copy_(pts)
    with pytest.raises(E, match="16-byte"):
        eng.link_avoid(q, odd, **kw)
    with pytest.raises(E, match="joint controller"):
        eng.link_avoid(q, pts, channel=2, **kw)
    for channel in (0, 1, 6, -2):
        with pytest.raises(E):
            eng.link_avoid(q, pts, channel=channel, **kw)
    with pytest.raises(E, match="ext buffer"):
        eng.link_avoid(q, pts, channel=5, **kw)
    assert eng.lib.vfik_link_avoid(eng.h, q.data_ptr(), pts.data_ptr(), pts.shape[1], 3, 5, None, 1.0, 0.1, None, None, -1) == -1   # no destination
    out = eng.link_avoid(q, pts, **kw)                     # the same rows, aligned
    eng.sync()
    assert np.array_equal(out.cpu().numpy().astype(np.float64), eng.link_avoid_host(c["q"], c["pts"], **kw))
    eng.close()


def test_replays_under_graph_capture(env):
    """a plain call allocates nothing and is valid under capture: one chain on one stream, no parallel branch"""
    torch = env.torch
    c = ha.make_case("lwr", np.float64, 65, "five", 5, 3, "static")
    eng = env.engine.Engine(c["chain"], 65, io_dtype=np.float64, max_slots=16)
    eng.set_link_spheres(c["spheres"])
    kw = dict(ha.call_args(c), scale=None)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        eng.use_stream(s.cuda_stream)
        q, pts = _dev(env, c["q"], np.float64), _dev(env, c["pts"], np.float64)
        out = torch.zeros(65, c["chain"].n, dtype=torch.float64, device=env.dev)
        eng.link_avoid(q, pts, out=out, **kw)
        torch.cuda.synchronize()
        direct = out.clone()
        assert bool((direct != 0).any())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            eng.link_avoid(q, pts, out=out, **kw)
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, direct)
        q.copy_(_dev(env, np.roll(c["q"], 1, axis=0), np.float64))     # the replay reads the arrays as they are now
        graph.replay()
        torch.cuda.synchronize()
        assert not torch.equal(out, direct)
    eng.close()
