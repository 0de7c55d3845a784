"""The two CPU oracles against the 50-digit field reference (tests/hp_field.py) on the edge scenes of the field sweep.

Every field test before this one compared a kernel with the C oracle at 1e-9 / 1e-6 on random scenes: order 5, obstacles decimetres away,
nothing near a floor, a cap or a kink -- and the oracle is itself plain double arithmetic with libm's pow.  Here the oracle is held to a
reference first, on scenes built for the field's decision edges (hp_field's docstring lists them), with a bar that scales with the
conditioning the reference itself reports; tests/test_gpu_field_edges.py then holds the HIP kernels to the same reference.

Bar per arm: |v6 - reference| <= max(S, 8 E), S = 1e-9 / 1e-6 (the suite's), 8 = hp_reference.K_MARGIN,
E = u (kappa_pose + kappa_rel + (4 + kappa_sum) max|v6|).  kappa_rel and the 1 / sin(theta) weight of an attractor's axis are this
work's additions to the kappa of the issue: without the first the C oracle is 1e4 E off on the probe scenes' on-axis funnel arms, without
the second 15 E off on two regular goals at theta = 3.13 (hp_field's docstring derives both from the reference's own sensitivities).

Measured (this file's print, both I/O types): the C oracle's worst ratio err / E is 1.0 (order 0), 0.87, 0.82, 0.82, 0.76, 0.99 (order
127) on scene 1, 1.27 on the powercube6, 0.8 on scenes 2 to 5, 1.68 on scene 6 (float32), 0.85 on scene 7, 0.42 and 1.89 on the probe
scenes; the NumPy restatement's stays below 2.5.  No arm of any scene is finite-only: after normCart even the arms inside the 1e-9 floor
keep 8 E below 1e-5 of max|v6| (the 1e15 of the floor multiplies a term that dominates the sum, and the sum is normalised)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hp_field as hf  # noqa: E402
import hp_reference as hp  # noqa: E402

IO = [np.float32, np.float64]


def _numpy_v6(sc):
    """the NumPy restatement, arm by arm"""
    from oracle import vfik_numpy as vn
    from vfclik_amd import _abi
    w, chain = sc["w"], sc["chain"]
    pd = _abi.params_to_dict(sc["params"])
    out = np.zeros((hf.B_ARMS, 6))
    for b in range(hf.B_ARMS):
        fd = {int(f["id"]): [float(f["force"]), int(f["type"]), f["p"][:_abi.FIELD_NPARAMS[int(f["type"])]].tolist()]
              for f in w["fields"][b][:w["nfields"][b]]}
        if sc["probe"]:
            VF, SF = vn.build_total_field(fd, vn.vectorFieldLibrary(pd["rot_slowdown"]))
            pose = sc["pose"][b].tolist()
            vec, s = VF.getVector(pose), SF.getScalar(pose)
            out[b, :3], out[b, 3:] = pd["speed_scale"] * s[0] * vec[:3], pd["speed_scale"] * s[1] * vec[3:]
        else:
            arm = vn.ArmCycle(chain.B, chain.jtype, chain.q_lo, chain.q_hi, pd)
            arm.set_fields(fd)
            out[b] = arm.cycle(w["q"][b].tolist())["v6"]
    return out


@pytest.mark.parametrize("io_dtype", IO, ids=["f32", "f64"])
@pytest.mark.parametrize("sid", hf.SCENES)
def test_oracles_against_the_reference(oracle_c, sid, io_dtype):
    sc, ref, R = hf.oracle_scene(oracle_c, sid, io_dtype)
    w = sc["w"]
    # the inputs are what the I/O type holds
    assert np.array_equal(w["fields"]["p"], w["fields"]["p"].astype(io_dtype).astype(np.float64))
    assert np.array_equal(w["fields"]["force"], w["fields"]["force"].astype(io_dtype).astype(np.float64))
    # every constructed arm meets the condition its kind names (from the reference's own quantities)
    bad = hf.kind_failures(sc, ref)
    assert not bad, "%d arms miss their kind's condition:\n" % len(bad) + "\n".join(bad[:20])
    held = ~ref["finite_only"]
    bar = np.maximum(hp.S_BAR[io_dtype], hp.K_MARGIN * ref["E"])    # (the oracles return doubles: no half ulp of a float32 store)
    v6c, status = hf.oracle_v6(oracle_c, sc)
    v6n = _numpy_v6(sc)
    assert np.all(status == 0)
    for name, v6 in (("C oracle", v6c), ("NumPy restatement", v6n)):
        assert np.all(np.isfinite(v6)), name
        err = hf.v6_error(v6, ref).max(axis=1)
        rat = np.where(held, err / ref["E"], 0.0)
        b = int(np.argmax(rat))
        print("%-9s %s %-17s worst err / E %.3f (arm %d %s: err %.2e, kappa_pose %.2e kappa_rel %.2e kappa_sum %.2e)"
              % (sid, np.dtype(io_dtype).name, name, rat[b], b, hf.kinds_of(sc, b), err[b], ref["kappa_pose"][b], ref["kappa_rel"][b],
                 ref["kappa_sum"][b]))
        over = held & (err > bar)
        assert not over.any(), "%s: %d arms over max(S, 8 E), worst ratio %.2f on arm %d (%s)" % (name, int(over.sum()), rat[b], b, hf.kinds_of(sc, b))
    # the scene is as hard as it claims, and not harder than can be held
    print("%-9s %s max kappa_sum %.3e, max kappa_pose %.3e, max kappa_rel %.3e, finite-only arms %d"
          % (sid, np.dtype(io_dtype).name, ref["kappa_sum"].max(), ref["kappa_pose"].max(), ref["kappa_rel"].max(), int((~held).sum())))
    if sid in hf.CODE_PATH_SCENES or sid == "P-rep":   # (P-aux has no repeller to cancel: the probe kernel's cancellation is P-rep's)
        assert ref["kappa_sum"].max() >= 1e3
    assert (~held).sum() <= hf.B_ARMS // 8
    for kinds in (sc["rk"], sc["hk"], sc["fk"]):
        for k in set(kinds) - {None}:
            assert any(held[b] for b in range(hf.B_ARMS) if kinds[b] == k), "kind %s has no held arm" % k
    assert np.abs(ref["v6"]).max() > 0.05


@pytest.mark.parametrize("sid", ["1-o5", "2-o5", "6", "P-rep", "P-aux"])
def test_every_group_of_eight_mixes_the_kinds(oracle_c, sid):
    """From a built scene: any eight consecutive arms hold eight different kinds of each primitive under test, and every wave holds every
    kind.  (Six in the uniform scenes, where the two force kinds are regular arms like the regular kind itself, seven for the hemisphere, whose index is shifted at a seam
    so that a funnel kind meets every hemisphere kind; scene 6's repellers are not under test.)"""
    sc = hf.make_scene(oracle_c, sid, np.float64)
    for name, kinds, least in (("rk", sc["rk"], 6 if sc["uniform"] else 8), ("hk", sc["hk"], 7), ("fk", sc["fk"], 8)):
        if kinds[0] is None or (sid == "6" and name == "rk"):
            continue
        for s0 in range(hf.B_ARMS - 7):
            assert len(set(kinds[s0:s0 + 8])) >= least, (name, s0, kinds[s0:s0 + 8])
        for wv in range(3):
            assert set(kinds[64 * wv:64 * wv + 64]) == set(kinds), (name, wv)
