"""Two inputs of a cycle that the kernels' parity tests did not vary: IK weights promoted from equal per-arm rows, across a later
vfik_set_params that does not touch them; and a device q that is not 16-byte aligned (the lean kernels fetch q in 16-byte pieces)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROWS = ("qdot_vf", "qdot_null", "qdot_out", "pose", "pose_nt", "qdist", "status")


@pytest.fixture(scope="module")
def env():
    import __graft_entry__ as g
    g.build()
    from oracle import oracle_c
    from vfclik_amd import _abi, engine, robots, synth

    class E:
        pass

    e = E()
    e.oc, e.abi, e.engine, e.robots, e.synth = oracle_c, _abi, engine, robots, synth
    return e


def _check(got, ref, keys, tol):
    for k in keys:
        if k == "status":
            assert np.array_equal(got[k], ref[k])
            continue
        err = np.abs(np.asarray(got[k], dtype=np.float64) - ref[k]).max()
        assert np.all(np.isfinite(got[k])) and err < tol, "%s: %.3e" % (k, err)


@pytest.mark.parametrize("B,dt,tol", [(1, np.float32, 1e-6), (1, np.float64, 1e-9), (6000, np.float32, 1e-6), (6000, np.float64, 1e-9)])
def test_promoted_arm_weights_survive_an_unrelated_set_params(env, B, dt, tol):
    """Equal per-arm IK weights for the whole batch are the batch's weights (vfik_set_arm_weights).  A later vfik_set_params that leaves
    wy / wq as the caller last passed them -- here the unit weights of the handle's creation, with another speed scale -- keeps them."""
    f = env.abi
    chain = env.robots.lwr()
    w = env.synth.make_workload(chain, B, 8, seed=71, io_dtype=dt)
    wy = [1.0, 1.0, 1.0, 0.5, 0.5, 0.25]
    wq = [1.0, 0.25, 1.0, 0.5, 1.0, 0.25, 1.0]
    flags = f.F_NULLSPACE | f.F_MIXER
    eng = env.engine.Engine(chain, B, io_dtype=dt, max_slots=8, params=f.default_params(flags=flags))
    eng.set_fields(w["fields"], w["nfields"])
    eng.set_arm_weights(wy=np.tile(wy, (B, 1)), wq=np.tile(wq, (B, 1)))
    eng.set_params(speed_scale=0.3)
    got = eng.step_host(w["q"], want=ROWS)
    eng.close()
    ref = env.oc.cycle_batch(chain, f.default_params(flags=flags, speed_scale=0.3, wy=wy, wq=wq + [1.0] * 9), w["q"], w["fields"], w["nfields"])
    unit = env.oc.cycle_batch(chain, f.default_params(flags=flags, speed_scale=0.3), w["q"], w["fields"], w["nfields"])
    assert np.abs(ref["qdot_out"] - unit["qdot_out"]).max() > 1e-3   # (the weights act)
    _check(got, ref, ROWS, tol)


def test_set_params_that_changes_the_weights_replaces_promoted_ones(env):
    """... while a vfik_set_params that CHANGES wy / wq is batch-wide again: its weights replace the promoted ones."""
    f = env.abi
    chain = env.robots.lwr()
    B = 300
    w = env.synth.make_workload(chain, B, 8, seed=72, io_dtype=np.float64)
    eng = env.engine.Engine(chain, B, io_dtype=np.float64, max_slots=8, params=f.default_params(flags=5))
    eng.set_fields(w["fields"], w["nfields"])
    eng.set_arm_weights(wy=np.tile([1.0, 1.0, 1.0, 0.5, 0.5, 0.25], (B, 1)), wq=np.tile([1.0, 0.25, 1.0, 0.5, 1.0, 0.25, 1.0], (B, 1)))
    wq2 = [0.5, 1.0, 0.5, 1.0, 0.3, 1.0, 0.5]
    eng.set_params(wq=wq2 + [1.0] * 9)
    got = eng.step_host(w["q"], want=ROWS)
    eng.close()
    ref = env.oc.cycle_batch(chain, f.default_params(flags=5, wq=wq2 + [1.0] * 9), w["q"], w["fields"], w["nfields"])
    _check(got, ref, ROWS, 1e-9)


@pytest.mark.parametrize("robot", ["powercube6", "lwr", "lwr_dual14"])
@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("family", ["lean", "publishing", "mixo"])
def test_q_at_an_offset_of_one_element(env, robot, dt, family):
    """vfik_step with q a device view one element past a 16-byte boundary, B % 4 != 0 (q's length is no multiple of 16 bytes): the
    results of an aligned q to the bit, and the oracle's -- for each family that fetches q in 16-byte pieces."""
    import torch
    chain = env.robots.by_name(robot)
    n, B = chain.n, 64 * 3 + 13
    tdt = torch.float32 if dt == np.float32 else torch.float64
    w = env.synth.make_workload(chain, B, 5, seed=73, io_dtype=dt)
    if family == "mixo":
        w["fields"]["p"][:, 1:3, 5] = 20.0   # integer orders that differ
    want = ("qdot_out", "status") if family == "lean" else ROWS
    params = env.abi.default_params(flags=5)
    eng = env.engine.Engine(chain, B, io_dtype=dt, max_slots=8, params=params)
    eng.set_fields(w["fields"], w["nfields"])
    eng.set_small_batch_kernel(0)
    eng.use_stream(torch.cuda.current_stream().cuda_stream)
    assert eng.mixed_orders == (family == "mixo")
    base = torch.zeros(B * n + 1, dtype=tdt, device="cuda")
    base[1:] = torch.from_numpy(w["q"].reshape(-1).astype(dt)).cuda()
    q_off = base[1:].view(B, n)
    q_al = q_off.clone()
    assert q_off.storage_offset() == 1 and q_off.data_ptr() % 16 != 0 and q_al.data_ptr() % 16 == 0
    outs = []
    for q in (q_off, q_al):
        o = {k: torch.zeros(B, 16 if k.startswith("pose") else n, dtype=tdt, device="cuda") for k in want if k != "status"}
        o["status"] = torch.zeros(B, dtype=torch.int32, device="cuda")
        eng.step(eng.make_io(q, **o))
        torch.cuda.synchronize()
        outs.append({k: v.cpu().numpy() for k, v in o.items()})
    (name,) = eng.launched_kernels()
    eng.close()
    assert name.startswith({"lean": "cycle_kernel_s<", "publishing": "cycle_kernel_x<", "mixo": "cycle_kernel_m<"}[family]), name
    if family == "publishing":
        assert name.split(", ")[6] == "3", name   # (LEAN 3)
    for k in want:
        assert np.array_equal(outs[0][k], outs[1][k]), k
    ref = env.oc.cycle_batch(chain, params, w["q"], w["fields"], w["nfields"], want=want)
    _check(outs[0], ref, want, 1e-6 if dt == np.float32 else 1e-9)
