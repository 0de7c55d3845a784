"""Engine.set_params with a new lambda and a new rot_slowdown on a handle that has already stepped.

Both are batch constants with derived values packed beside them -- lambda^2, cos(rot_slowdown) and 1 / rot_slowdown (KConst::dh[1].pad, read by
the straight-line variants of chains of up to 9 joints) -- so a handle whose parameters change must end up with exactly the constants a
fresh handle gets.  64 arms of the LWR, a third of them inside the NEW slow-down angle of 0.2 rad (built like the INSIDE / DEEP lanes of
tests/test_gpu_goal_rare_paths.py: the goal is the oracle's own tool pose turned by a chosen angle), where 1 / rot_slowdown scales the twist.

The first engine is created at (lambda 0.1, rot_slowdown 0.3), stepped, then moved to (1e-2, 0.2); the second is created at (1e-2, 0.2).
Their outputs are byte-equal, on the lean, the publishing and the eight-lanes kernels, and both are within the bar of
tests/test_gpu_conditioning.py of the high-precision reference (tests/hp_reference.py)."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hp_reference as hp  # noqa: E402
import kernel_variants as kv  # noqa: E402

B = 64
OLD, NEW = dict(rot_slowdown=0.3, **{"lambda": 0.1}), dict(rot_slowdown=0.2, **{"lambda": 1e-2})


def _rodrigues(u, th):
    K = np.array([[0.0, -u[2], u[1]], [u[2], 0.0, -u[0]], [-u[1], u[0], 0.0]])
    return np.eye(3) + math.sin(th) * K + (1.0 - math.cos(th)) * (K @ K)


def _scene(oc, io_dtype):
    """(chain, workload, inside): arms 0, 3, 6, ... have their goal 0.2 - 1e-3 rad (even ones) or deep inside 0.2 rad of the tool pose"""
    from vfclik_amd import _abi, robots, synth
    chain = robots.lwr()
    w = synth.make_workload(chain, B, 2, seed=11, io_dtype=io_dtype)
    pose = oc.cycle_batch(chain, _abi.default_params(), w["q"], w["fields"], w["nfields"], want=("pose",))["pose"].reshape(B, 4, 4)
    rng = np.random.default_rng(12)
    inside = np.arange(B) % 3 == 0
    for b in np.nonzero(inside)[0]:
        u = rng.normal(size=3)
        u /= np.linalg.norm(u)
        G = np.eye(4)
        G[:3, :3] = _rodrigues(u, NEW["rot_slowdown"] - 1e-3 if b % 2 == 0 else rng.uniform(1e-3, 0.1)) @ pose[b, :3, :3]
        G[:3, 3] = pose[b, :3, 3] + rng.uniform(-0.3, 0.3, 3)
        w["fields"]["p"][b, 0, :16] = G.reshape(16).astype(io_dtype).astype(np.float64)
    return chain, w, inside


@pytest.mark.gpu
@pytest.mark.parametrize("io_dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_set_params_equals_a_fresh_engine(io_dtype):
    import __graft_entry__ as g
    g.build()
    from oracle import oracle_c as oc
    from vfclik_amd import _abi as abi, engine
    oc.build()
    chain, w, inside = _scene(oc, io_dtype)
    p_new = abi.default_params(**NEW)
    want_o = ("qdot_vf", "qdot_out", "pose", "v6", "status")
    orc = oc.cycle_batch(chain, p_new, w["q"], w["fields"], w["nfields"], want=want_o)
    orc_old = oc.cycle_batch(chain, abi.default_params(**OLD), w["q"], w["fields"], w["nfields"], want=want_o)
    # the inside arms turn slower than one unit of speed_scale under the new angle, and the new parameters move every arm's result
    wn = np.linalg.norm(orc["v6"][:, 3:], axis=1)
    assert np.all(wn[inside] < 0.999) and np.all(np.abs(wn[~inside] - 1.0) < 1e-12)
    assert np.all(np.abs(orc["qdot_vf"] - orc_old["qdot_vf"]).max(axis=1) > 1e-4)
    assert np.all(orc["status"] == 0)
    ref = hp.reference(("lwr", np.dtype(io_dtype).name, "set_params"), chain, w["q"], orc["v6"], NEW["lambda"], *hp.weights("unit", 7), "unit")
    R = float(hp.ratio(orc["qdot_vf"], ref)[0].max())
    kinds, eps = np.where(inside, 1, 0), np.zeros(B)     # (printed as `kind`: 1 = inside the slow-down angle)
    failures = []
    for small, want in ((0, ("qdot_out", "status")), (0, ("qdot_out", "qdot_vf", "pose", "status")), (4096, ("qdot_out", "status"))):
        outs = []
        for moved in (True, False):
            eng = engine.Engine(chain, B, io_dtype=io_dtype, max_slots=4, params=abi.default_params(**(OLD if moved else NEW)))
            try:
                eng.set_small_batch_kernel(small)
                eng.set_fields(w["fields"], w["nfields"])
                if moved:
                    first = eng.step_host(w["q"], want=want)
                    assert np.abs(first["qdot_out"].astype(np.float64) - orc_old["qdot_out"]).max() < hp.S_BAR[io_dtype]
                    eng.set_params(**NEW)
                eng.launched_kernels()
                outs.append(eng.step_host(w["q"], want=want))
                names = [kv.parse(n) for n in eng.launched_kernels()]
                assert names and all(v.kernel == ("cycle_sub8_kernel_x" if small else "cycle_kernel_s" if len(want) == 2 else "cycle_kernel_x")
                                     and v.args["NJ"] == 7 for v in names), names
            finally:
                eng.close()
        for k in want:
            assert outs[0][k].tobytes() == outs[1][k].tobytes(), "%s after set_params differs from a fresh engine's (cap %d)" % (k, small)
        got = outs[0]
        assert np.array_equal(got["status"], orc["status"])
        for k in want[:-1]:
            if k == "pose":
                assert hp.error(got[k], ref, "pose").max() <= hp.S_BAR[io_dtype]
            else:
                hp.check_qdot(got[k], ref, io_dtype, R, "cap %d %s" % (small, k), kinds, eps, failures)
    assert not failures, "\n".join(failures)
