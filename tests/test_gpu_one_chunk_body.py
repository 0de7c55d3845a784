"""The one-chunk order-5 body of the uniform-image lean kernels (cycle_kernel_s behind one entry branch: vfik_kernel.hip, ONE5).

The host decides in vfik_set_fields (Engine.one_chunk reports it): uniform image in use, decay order 5, at most 8 repellers on any arm,
float32 I/O, a chain of up to 7 joints, and not VFIK_ONE_CHUNK=0.  The body then reads planes 1 ... 8 of the uniform image whatever the
slots in use -- so the image must own them (a handle created with max_slots < 8) and every plane at or beyond an arm's count must be
empty (a smaller field set after a larger one).

Every case in which the body runs is held to the C oracle at test_gpu_parity's float32 bar and to a second engine created under
VFIK_ONE_CHUNK=0 (the other body of the same kernel) within 1 float32 ulp with identical status: the two bodies are the same source
expressions.  Batches: 1 arm and 130 arms (two full waves and a two-arm tail: a partial wave and the `arm >= B` exit)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_variants as kv  # noqa: E402
from test_gpu_parity import TOL32  # noqa: E402  (the float32 bar every parity test of the suite uses)

pytestmark = pytest.mark.gpu

LEAN = ("qdot_out", "status")
EXACT = []   # (case, largest ulp difference between the two bodies): printed by the last test of the file


@pytest.fixture(scope="module")
def env():
    import __graft_entry__ as g
    g.build()
    import torch
    from oracle import oracle_c
    from vfclik_amd import _abi, engine, robots, synth
    lib = engine.load_library()
    assert lib.vfik_device_count() >= 1, "no HIP device: the gpu tests need an MI355X"

    class E:
        pass

    e = E()
    e.oc, e.abi, e.engine, e.robots, e.synth, e.torch = oracle_c, _abi, engine, robots, synth, torch
    return e


def _scene(env, chain, B, S, seed, nobs=None):
    """Goal + obstacles as the feeder sends them; per-arm counts drawn from 0 ... S with an arm at 0 and an arm at S (one arm: S)."""
    nobs = max(S, 1) if nobs is None else nobs
    w = env.synth.make_workload(chain, B, nobs, seed=seed, io_dtype=np.float32)
    counts = np.random.default_rng(seed + 1).integers(0, S + 1, B)
    counts[-1] = S
    if B > 1:
        counts[0] = 0
        counts[B // 2] = S
    w["nfields"] = (1 + counts).astype(np.int32)
    return w


def _engine(env, monkeypatch, chain, B, params, max_slots=8, one_chunk=True, dt=np.float32):
    if not one_chunk:
        monkeypatch.setenv("VFIK_ONE_CHUNK", "0")
    eng = env.engine.Engine(chain, B, io_dtype=dt, max_slots=max_slots, params=params)
    if not one_chunk:
        monkeypatch.delenv("VFIK_ONE_CHUNK")
    return eng


def _ulps(a, b):
    """largest distance between two float32 arrays in units in the last place (0 = the same bits, but for the sign of zero)"""
    def key(x):
        i = np.ascontiguousarray(x, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    assert np.all(np.isfinite(a)) and np.all(np.isfinite(b))
    return int(np.abs(key(a) - key(b)).max())


def _vs_oracle(got, ref):
    assert np.array_equal(got["status"], ref["status"])
    err = float(np.abs(got["qdot_out"].astype(np.float64) - ref["qdot_out"]).max())
    assert np.all(np.isfinite(got["qdot_out"])) and err < TOL32, "qdot_out: max err %.3e" % err


def _lean_uniform(eng, nj=7):
    """the launches since the last call: the uniform-image lean kernel at one wave per SIMD, nothing else"""
    launched = [kv.parse(k) for k in eng.launched_kernels()]
    assert launched
    for v in launched:
        assert v.kernel == "cycle_kernel_s" and v.args["UNI"] and v.args["WAVES"] == 1 and v.args["NJ"] == nj, v.name


def _both_bodies(env, monkeypatch, case, chain, params, w, max_slots=8, tool=None, prepare=None):
    """Step `w` on a handle that takes the one-chunk body and on one created under VFIK_ONE_CHUNK=0; the first against the oracle,
    the two against each other.  `prepare(eng)` runs after set_fields on both.  Returns the one-chunk handle's result."""
    B = w["q"].shape[0]
    out = []
    for one in (True, False):
        eng = _engine(env, monkeypatch, chain, B, params, max_slots=max_slots, one_chunk=one)
        eng.set_fields(w["fields"], w["nfields"])
        if tool is not None:
            eng.set_tool(tool)
        if prepare is not None:
            prepare(eng)
        assert eng.uniform_repellers and eng.one_chunk == one, (case, one)
        out.append(eng.step_host(w["q"], want=LEAN))
        _lean_uniform(eng, chain.n)
        eng.close()
    d = _ulps(out[0]["qdot_out"], out[1]["qdot_out"])
    print("%s: one-chunk body against the generic body: %d ulp" % (case, d))
    EXACT.append((case, d))
    assert d <= 1, (case, d)
    assert np.array_equal(out[0]["status"], out[1]["status"]), case
    return out[0]


@pytest.mark.parametrize("flags", [0, 1 | 4])
@pytest.mark.parametrize("S", [0, 1, 7, 8])
@pytest.mark.parametrize("B", [1, 130])
def test_one_chunk_body_against_oracle_and_generic_body(env, monkeypatch, B, S, flags):
    chain = env.robots.lwr()
    params = env.abi.default_params(flags=flags)
    w = _scene(env, chain, B, S, seed=100 + 10 * S + B)
    got = _both_bodies(env, monkeypatch, "B%d S%d flags%d" % (B, S, flags), chain, params, w)
    _vs_oracle(got, env.oc.cycle_batch(chain, params, w["q"], w["fields"], w["nfields"], want=LEAN))


def test_shared_tool(env, monkeypatch):
    chain = env.robots.lwr()
    params = env.abi.default_params()
    w = _scene(env, chain, 130, 8, seed=7)
    tool = np.eye(4)
    tool[:3, 3] = [0.02, -0.01, 0.2]
    c, s = np.cos(0.3), np.sin(0.3)
    tool[:3, :3] = [[c, -s, 0], [s, c, 0], [0, 0, 1]]
    tool = tool.reshape(16)
    got = _both_bodies(env, monkeypatch, "shared tool", chain, params, w, tool=tool)
    _vs_oracle(got, env.oc.cycle_batch(chain, params, w["q"], w["fields"], w["nfields"], tool=tool, want=LEAN))


def test_six_joint_chain(env, monkeypatch):
    chain = env.robots.powercube6()
    params = env.abi.default_params()
    w = _scene(env, chain, 130, 8, seed=8)
    got = _both_bodies(env, monkeypatch, "powercube6", chain, params, w)
    _vs_oracle(got, env.oc.cycle_batch(chain, params, w["q"], w["fields"], w["nfields"], want=LEAN))


def test_handle_with_fewer_slots_than_a_chunk(env, monkeypatch):
    """max_slots = 3: the body still requests planes 1 ... 8, which the image owns and keeps empty."""
    chain = env.robots.lwr()
    params = env.abi.default_params()
    for B in (1, 130):
        w = _scene(env, chain, B, 3, seed=9 + B)
        got = _both_bodies(env, monkeypatch, "max_slots 3, B%d" % B, chain, params, w, max_slots=3)
        _vs_oracle(got, env.oc.cycle_batch(chain, params, w["q"], w["fields"], w["nfields"], want=LEAN))
    # ... and a handle without any slot
    w = _scene(env, chain, 130, 0, seed=12)
    got = _both_bodies(env, monkeypatch, "max_slots 0", chain, params, w, max_slots=0)
    _vs_oracle(got, env.oc.cycle_batch(chain, params, w["q"], w["fields"], w["nfields"], want=LEAN))


@pytest.mark.parametrize("flags", [0, 1 | 4])
def test_smaller_field_set_after_a_larger_one(env, monkeypatch, flags):
    """8 obstacles, a step, then 2: the planes of the six that left must read as empty -- byte for byte a fresh handle given the 2."""
    chain = env.robots.lwr()
    params = env.abi.default_params(flags=flags)
    B = 130
    w8 = env.synth.make_workload(chain, B, 8, seed=13, io_dtype=np.float32)
    w2 = {k: (v.copy() if hasattr(v, "copy") else v) for k, v in w8.items()}
    w2["nfields"] = np.full(B, 3, dtype=np.int32)
    a = _engine(env, monkeypatch, chain, B, params)
    a.set_fields(w8["fields"], w8["nfields"])
    assert a.one_chunk and a.slots_in_use == 8
    _vs_oracle(a.step_host(w8["q"], want=LEAN), env.oc.cycle_batch(chain, params, w8["q"], w8["fields"], w8["nfields"], want=LEAN))
    a.set_fields(w2["fields"], w2["nfields"])
    a.reset_state()
    assert a.one_chunk and a.slots_in_use == 2
    ga = a.step_host(w2["q"], want=LEAN)
    _lean_uniform(a)
    b = _engine(env, monkeypatch, chain, B, params)
    b.set_fields(w2["fields"], w2["nfields"])
    assert b.one_chunk
    gb = b.step_host(w2["q"], want=LEAN)
    assert ga["qdot_out"].tobytes() == gb["qdot_out"].tobytes() and np.array_equal(ga["status"], gb["status"])
    _vs_oracle(ga, env.oc.cycle_batch(chain, params, w2["q"], w2["fields"], w2["nfields"], want=LEAN))
    a.close()
    b.close()


def test_move_fields_of_every_repeller(env, monkeypatch):
    chain = env.robots.lwr()
    params = env.abi.default_params()
    B = 130
    w = _scene(env, chain, B, 8, seed=14)
    rng = np.random.default_rng(15)
    rows = np.ascontiguousarray(w["fields"]["p"][:, 1:9, :4]).astype(np.float32)
    rows[:, :, :3] += rng.uniform(-0.05, 0.05, (B, 8, 3)).astype(np.float32)
    moved = {k: (v.copy() if hasattr(v, "copy") else v) for k, v in w.items()}
    moved["fields"]["p"][:, 1:9, :4] = rows.astype(np.float64)
    dev = env.torch.from_numpy(rows).cuda()
    env.torch.cuda.synchronize()
    got = _both_bodies(env, monkeypatch, "move_fields", chain, params, w, prepare=lambda eng: eng.move_fields(repellers=dev))
    _vs_oracle(got, env.oc.cycle_batch(chain, params, w["q"], moved["fields"], moved["nfields"], want=LEAN))


@pytest.mark.parametrize("case", ["order 4", "9 obstacles", "16 obstacles", "pair differs", "VFIK_ONE_CHUNK=0", "float64 I/O"])
@pytest.mark.parametrize("B", [1, 130])
def test_scenes_that_stay_on_the_generic_body(env, monkeypatch, case, B):
    chain = env.robots.lwr()
    params = env.abi.default_params()
    nobs = {"9 obstacles": 9, "16 obstacles": 16}.get(case, 8)
    dt = np.float64 if case == "float64 I/O" else np.float32
    w = env.synth.make_workload(chain, B, nobs, seed=16 + B, io_dtype=dt)
    if case == "order 4":
        w["fields"]["p"][:, 1:, 5] = 4.0
    if case == "pair differs":   # one arm's third repeller with another safe distance: the compact image for the batch
        w["fields"]["p"][B // 2, 3, 4] = np.float64(np.float32(0.004))
    eng = _engine(env, monkeypatch, chain, B, params, max_slots=16, one_chunk=case != "VFIK_ONE_CHUNK=0", dt=dt)
    eng.set_fields(w["fields"], w["nfields"])
    assert eng.field_path == 1 and not eng.one_chunk
    assert eng.uniform_repellers == (case != "pair differs")
    got = eng.step_host(w["q"], want=LEAN)
    ref = env.oc.cycle_batch(chain, params, w["q"], w["fields"], w["nfields"], want=LEAN)
    if dt == np.float32:
        _vs_oracle(got, ref)
    else:
        assert np.array_equal(got["status"], ref["status"]) and np.abs(got["qdot_out"] - ref["qdot_out"]).max() < 1e-9
    # ... and back to the feeder's scene on the same handle: the decision follows the field sets
    if case in ("order 4", "9 obstacles", "16 obstacles", "pair differs"):
        w8 = env.synth.make_workload(chain, B, 8, seed=18 + B, io_dtype=np.float32)
        eng.set_fields(w8["fields"], w8["nfields"])
        assert eng.one_chunk
        _vs_oracle(eng.step_host(w8["q"], want=LEAN), env.oc.cycle_batch(chain, params, w8["q"], w8["fields"], w8["nfields"], want=LEAN))
    eng.close()


def test_zz_report_whether_the_bodies_agree_bit_for_bit():
    """Not a check of its own (every case above asserts <= 1 ulp): one line for the record."""
    if EXACT:
        print("one-chunk body against generic body, largest difference over %d cases: %d ulp" % (len(EXACT), max(d for _, d in EXACT)))
