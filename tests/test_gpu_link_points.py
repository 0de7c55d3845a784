"""vfik_link_points on the GPU (include/vfik.h; link_kernel, vfclik_amd/csrc/vfik_aux.hip) against the 50-digit link points of
tests/hp_links.py, in both I/O types.

Chains: powercube6, lwr, lwr_dual14 and hp_links' `mixed10` (ten joints, two prismatic, a base that is no identity, from KDL-style segments).
Per chain and I/O type the five cases of hp_links.CASES -- one sphere on link 0 with c != 0; five unsorted spheres, two on one link; sixteen
with every link used, n included; sources NULL, b ^ 1, all zeros, and a mix with -1 and B; without and with a per-arm rotation plus translation
rounded to the I/O type -- at B = 203 (three waves and a part), written with n_rep = L + 3 and first_rep = 2 into a buffer prefilled with a
sentinel: the five rows outside stay bit-identical.

THE BAR, per coordinate: K_MARGIN max(1, R) n u reach + half an ulp of the output type at the coordinate's magnitude; reach = sum |p(B_i)| + |c|
(+ |t_b| with a transform), u = 2^-53, R the host's worst error in the same units on the same inputs (hp_links.host_ratio; tests/test_links_host.py
prints it: up to 0.26).  The device gets the suite's K_MARGIN = 8 over the host because its sin / cos and its order of operations differ; a
wrong frame is off by centimetres, twelve orders above this.  The radius is the sphere's rounded to the type, exactly; an arm whose source is
outside the batch has NaN rows; the host form equals the device form bit for bit.

With VFIK_LINK_TABLE=<file> the measured worst ratios are also written there (the record kept in profiles/link_points_accuracy.txt)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import coupled_reference as cr  # noqa: E402
import hp_links as hl  # noqa: E402

pytestmark = pytest.mark.gpu

B0 = 203
SENTINEL = -777.25   # exact in both I/O types


@pytest.fixture(scope="module")
def env():
    import __graft_entry__ as g
    g.build()
    import torch
    from vfclik_amd import _abi, engine, robots

    class E:
        pass

    e = E()
    e.abi, e.engine, e.robots, e.torch = _abi, engine, robots, torch
    e.dev = torch.device("cuda", 0)
    e.table = []
    yield e
    path = os.environ.get("VFIK_LINK_TABLE")
    if path and e.table:
        with open(path, "a") as f:
            f.write("".join(e.table))


def _dev(env, a, dtype):
    return env.torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(env.dev)


def _points(env, eng, q, src, xform, n_rep, first_rep):
    """the device form on a sentinel-filled buffer -> (n_arms, n_rep, 4) of the engine's dtype"""
    t = eng.io_dtype.type
    out = env.torch.full((eng.batch, n_rep, 4), SENTINEL, dtype=getattr(env.torch, eng.io_dtype.name), device=env.dev)
    eng.link_points(_dev(env, q, t), None if src is None else _dev(env, src, np.int32), None if xform is None else _dev(env, xform, t),
                    out=out, first_rep=first_rep)
    eng.sync()
    return out.cpu().numpy()


def _check_case(env, eng, chain, robot, kind, src_kind, with_xform, B, io_dtype):
    sp = hl.sphere_list(chain, kind)
    L = len(sp)
    q, x = hl.inputs(chain, B, io_dtype)
    x = x if with_xform else None
    src = hl.sources(src_kind, B)
    R, ref = hl.host_ratio(robot, kind, src_kind, with_xform, B, io_dtype)
    eng.set_link_spheres(sp)
    got = _points(env, eng, q, src, x, L + 3, 2)
    # the five rows outside: untouched
    assert np.all(got[:, :2] == io_dtype(SENTINEL)) and np.all(got[:, 2 + L:] == io_dtype(SENTINEL))
    rows = got[:, 2:2 + L]
    gone = np.isnan(ref[0][:, :, 0])
    s = np.arange(B) if src is None else src
    assert np.array_equal(gone[:, 0], (s < 0) | (s >= B))
    assert np.isnan(rows[gone]).all() and not np.isnan(rows[~gone]).any()
    # the radius: the sphere's, rounded to the type
    rad = np.array([r for _l, _c, r in sp]).astype(io_dtype)
    assert np.array_equal(rows[~gone[:, 0], :, 3], np.tile(rad, (np.count_nonzero(~gone[:, 0]), 1)))
    # the bar
    units = hl.error_units(rows[:, :, :3], ref, chain, sp, x)
    reach = hl.reach(chain, sp, x)
    reach = reach[None, :, None] if reach.ndim == 1 else reach[:, :, None]
    err = units * (chain.n * hl.U * reach)
    half_ulp = 0.5 * np.spacing(np.abs(ref[0]).astype(io_dtype)).astype(np.float64)
    bar = hl.K_MARGIN * max(1.0, R) * chain.n * hl.U * reach + half_ulp
    ok = np.broadcast_to(~gone[:, :, None], err.shape)
    worst_units = float(np.nanmax(np.where(ok, (err - half_ulp) / (chain.n * hl.U * reach), -np.inf)))
    line = "%-10s %-7s %-5s %-4s xform %d  B %3d  host R %.3f  device %.3f units beyond half an ulp of the output (allowed %.0f), worst error %.3e m, worst error / bar %.3f\n" % (
        robot, np.dtype(io_dtype).name, kind, src_kind, with_xform, B, R, max(worst_units, 0.0), hl.K_MARGIN * max(1.0, R),
        float(np.nanmax(np.where(ok, err, 0.0))), float(np.nanmax(np.where(ok, err / bar, 0.0))))
    print(line, end="")
    env.table.append(line)
    assert np.all(err[ok] <= bar[ok]), line
    # the host form: the same bits, and only its own rows
    host = np.full((B, L + 3, 4), SENTINEL)
    back = eng.link_points_host(q, src, x, out=host, first_rep=2)
    assert back is host and np.all(host[:, :2] == SENTINEL) and np.all(host[:, 2 + L:] == SENTINEL)
    assert np.array_equal(host[:, 2:2 + L], rows.astype(np.float64), equal_nan=True)
    return rows


@pytest.mark.parametrize("io_dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("robot", hl.ROBOTS)
def test_against_50_digits(env, robot, io_dtype):
    chain = hl.chain_of(robot)
    eng = env.engine.Engine(chain, B0, io_dtype=io_dtype, max_slots=19)
    for kind, src_kind, with_xform in hl.CASES:
        _check_case(env, eng, chain, robot, kind, src_kind, with_xform, B0, io_dtype)
    eng.close()


@pytest.mark.parametrize("B", [1, 64])
def test_one_arm_and_one_wave(env, B):
    chain = hl.chain_of("lwr")
    for io_dtype in (np.float32, np.float64):
        eng = env.engine.Engine(chain, B, io_dtype=io_dtype, max_slots=19)
        _check_case(env, eng, chain, "lwr", "five", "zero", True, B, io_dtype)
        _check_case(env, eng, chain, "lwr", "all16", "self", False, B, io_dtype)
        if B > 1:
            _check_case(env, eng, chain, "lwr", "five", "mix", False, B, io_dtype)
        eng.close()


@pytest.mark.parametrize("io_dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_nan_row(env, io_dtype):
    """arm 70's q row holds a NaN at joint 3: the rows of everybody whose source it is -- arm 71 under b ^ 1, spheres of links 0..3 included --
    start with NaN; nobody else's rows change by a bit"""
    chain = hl.chain_of("lwr")
    sp = hl.sphere_list(chain, "all16")
    q, x = hl.inputs(chain, B0, io_dtype)
    src = hl.sources("pair", B0)
    eng = env.engine.Engine(chain, B0, io_dtype=io_dtype, max_slots=19)
    eng.set_link_spheres(sp)
    clean = _points(env, eng, q, src, x, 16, 0)
    qn = q.copy()
    qn[70, 3] = np.nan
    got = _points(env, eng, qn, src, x, 16, 0)
    assert np.isnan(got[71]).all()
    others = np.arange(B0) != 71
    assert np.array_equal(got[others], clean[others], equal_nan=True) and not np.isnan(got[70]).any()
    own = _points(env, eng, qn, None, None, 16, 0)      # its own source: arm 70 alone
    assert np.isnan(own[70]).all() and not np.isnan(own[np.arange(B0) != 70]).any()
    eng.close()


@pytest.mark.parametrize("io_dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_composition_with_move_fields(env, io_dtype):
    """[link_points; move_fields(repellers = its output); step] returns the bits of an engine that got the same rows through set_fields, and
    nothing a launch decides at enqueue time moves"""
    chain = env.robots.lwr()
    c = cr.pair_case(chain, B0, io_dtype)
    w, L, fr = c["w"], len(c["spheres"]), c["first_rep"]
    params = env.abi.default_params(flags=env.abi.F_NULLSPACE | env.abi.F_MIXER)
    eng = env.engine.Engine(chain, B0, io_dtype=io_dtype, max_slots=8, params=params)
    eng.set_fields(w["fields"], w["nfields"])
    eng.set_link_spheres(c["spheres"])
    t = io_dtype
    qd = _dev(env, c["q0"], t)
    before = (eng.field_path, eng.uniform_repellers, eng.slots_in_use, eng.launch_epoch)
    out = eng.link_points(qd, _dev(env, c["src_arm"], np.int32), _dev(env, c["xform"], t), first_rep=fr)
    assert tuple(out.shape) == (B0, fr + L, 4)
    eng.move_fields(repellers=out)
    assert (eng.field_path, eng.uniform_repellers, eng.slots_in_use, eng.launch_epoch) == before
    got = eng.step_host(c["q0"], want=("qdot_out", "qdot_vf", "pose"))
    rows = out.cpu().numpy().astype(np.float64)
    assert np.isnan(rows[:, :fr]).all()                  # the rows in front: "leave as it is"
    f2 = w["fields"].copy()
    slots = cr.repeller_slots(f2, w["nfields"])
    for b in range(B0):
        for j in range(L):
            if not np.isnan(rows[b, fr + j, 0]):
                f2["p"][b, slots[b][fr + j], 0:4] = rows[b, fr + j]
    assert np.count_nonzero(f2["p"] != w["fields"]["p"]) >= 3 * 3 * (B0 - 1)
    ref = env.engine.Engine(chain, B0, io_dtype=io_dtype, max_slots=8, params=params)
    ref.set_fields(f2, w["nfields"])
    want = ref.step_host(c["q0"], want=("qdot_out", "qdot_vf", "pose"))
    for k in ("qdot_out", "qdot_vf", "pose"):
        assert np.array_equal(got[k], want[k]), k
    # ... and it is not the scene the engine started with
    eng0 = env.engine.Engine(chain, B0, io_dtype=io_dtype, max_slots=8, params=params)
    eng0.set_fields(w["fields"], w["nfields"])
    assert not np.array_equal(eng0.step_host(c["q0"], want=("qdot_vf",))["qdot_vf"][:B0 - 1], got["qdot_vf"][:B0 - 1])
    for e in (eng, ref, eng0):
        e.close()


def test_argument_errors(env):
    chain = env.robots.lwr()
    E = env.engine.VfikError
    eng = env.engine.Engine(chain, 8, io_dtype=np.float32, max_slots=6)
    q = _dev(env, np.zeros((8, 7)), np.float32)
    out = env.torch.zeros((8, 6, 4), dtype=env.torch.float32, device=env.dev)
    with pytest.raises(E, match="vfik_set_link_spheres"):      # VFIK_E_STATE: no spheres
        eng.link_points(q, out=out)
    with pytest.raises(E, match="vfik_set_link_spheres"):
        eng.set_coupling(src_arm=np.zeros(8, dtype=np.int32))
    for bad in ([(8, (0, 0, 0), 0.1)], [(-1, (0, 0, 0), 0.1)], [(1, (np.nan, 0, 0), 0.1)], [(1, (0, 0, 0), -0.1)], [(1, (0, 0, 0), np.inf)],
                [(1, (0, 0, 0), 0.1)] * 17):
        with pytest.raises(E):
            eng.set_link_spheres(bad)
    eng.set_link_spheres([(3, (0.1, 0, 0), 0.05), (7, (0, 0, 0.1), 0.06)])
    for kw in (dict(first_rep=-1), dict(first_rep=5), dict(n_rep=7)):          # rows outside rep4; n_rep > max_slots
        with pytest.raises(E):
            eng.link_points(q.data_ptr(), out=out.data_ptr(), **dict(dict(n_rep=6, first_rep=0), **kw))
    with pytest.raises(E, match="16-byte"):
        eng.link_points(q.data_ptr(), out=out.data_ptr() + 4, n_rep=4)
    with pytest.raises(E):
        eng.link_points(0, out=out.data_ptr(), n_rep=6)
    with pytest.raises(E):
        eng.set_coupling(src_arm=np.zeros(8, dtype=np.int32), first_rep=5)    # first_rep + L > max_slots
    with pytest.raises(ValueError):
        eng.set_coupling(first_rep=3)                                          # nothing to couple with: not a silent "off"
    with pytest.raises(ValueError):
        eng.set_coupling(src_arm=np.zeros(8, dtype=np.int32), link_traj=out, trace_checks=4)
    eng.link_points(q, out=out, first_rep=4)                                    # the last two rows: accepted
    eng.sync()
    assert np.all(out.cpu().numpy()[:, :4] == 0) and np.all(out.cpu().numpy()[:, 4:, 3] == np.float32([0.05, 0.06]))
    eng.set_link_spheres(None)                                                  # none again
    with pytest.raises(E, match="vfik_set_link_spheres"):
        eng.link_points(q, out=out)
    eng.close()
