"""Finite but far-out joint angles: the published pose of the chains that take each sine / cosine path -- the LDS table (6 and 7 joints), the
table-free pi/2 reduction (14 joints) and the eight-lanes kernel's -- at |q| of about 10, 1e3 and 1e5 rad, against the 50-digit kinematics
of tests/hp_reference.py.  vfik_device.h claims less than 1 ulp (sincos_fast) and about 2 ulp (sincos_tab_n) "for |x| up to ~1e5 rad";
angles beyond that are outside the contract (include/vfik.h, io->q).

The bar is the oracle's: the C oracle (libm) is measured against the same reference at the same q, R = its worst error in the units of
poison_reference.far_units (u per joint for a rotation entry, u x reach per joint for the position), and the kernel is allowed the suite's
margin over it, K = 8 max(1, R) units (hp_reference.K_MARGIN, as tests/test_gpu_field_edges.py).  R comes from the oracle and never from the
kernel, and there is no absolute floor under the bar.

Two launch forms per chain, and which instantiation ran is asserted from its name (tests/kernel_variants.py):
  pattern   the launch without per-arm options takes the kernel built for the chain's DH pattern (template argument D, bit 0) where the
            library has one -- float32 I/O: all three chains; float64 I/O: the 7-joint chain.  It takes the joint angle as it is
            (vfik_kernel.hip: ang[i] = q[i]) and is held to K units at every scale.
  general   the launch with per-arm limits (four times the angles: no limit logic is in the way; no flag is set) takes a general variant
            (D = 0), and the eight-lanes kernel takes no option: both ADD the link's DH angle offset to the joint angle in double.  The sum
            is rounded: a joint whose offset is not zero carries up to half an ulp of it, (|q_i| + |off_i|) 2^-53 rad, which no sine / cosine
            can undo.  Their bar is K units plus that term for the joints that do add an offset (poison_reference.far_angle_term, the
            offsets read from the recorded device constants: pi or 2 pi on four of the LWR's seven joints, two of the 6-joint arm's): a
            rotation entry moves by at most the angle's error, the position by at most reach times it.  At |q| ~ 10 the term is under one
            unit of a 7-joint chain's K.
A float32 row is allowed the half ulp of its store, which is far above every bar here: at float32 I/O the test shows that nothing gross
happens, no more.

With VFIK_POISON_TABLE=<file> the figures are also written there (profiles/poison_isolation.txt)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hp_reference as hp  # noqa: E402
import kernel_variants as kv  # noqa: E402
import poison_reference as pr  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import __graft_entry__ as g
    g.build()
    from oracle import oracle_c
    from vfclik_amd import _abi, engine, synth

    class E:
        pass

    e = E()
    e.oc, e.abi, e.engine, e.synth = oracle_c, _abi, engine, synth
    e.table = []
    yield e
    path = os.environ.get("VFIK_POISON_TABLE")
    if path and e.table:
        with open(path, "a") as f:
            f.write("\n".join(e.table) + "\n")


CASES = [(c, io) for c in pr.FAR_CHAINS for io in (32, 64)]


def _d_bit(name):
    v = kv.parse(name)
    return v.args["D"] & 1


@pytest.mark.parametrize("name,io", CASES, ids=["%s-f%d" % (c.replace(" ", "-"), io) for c, io in CASES])
def test_pose_at_far_out_angles(env, name, io):
    dt = np.float32 if io == 32 else np.float64
    sub8 = name.endswith("eight-lanes")
    offsets = pr.far_offsets(name)
    failures = []
    for scale in pr.FAR_SCALES:
        chain, q = pr.far_case(name, scale, dt)
        assert np.abs(q).min() >= 0.49 * scale and np.abs(q).max() <= 1.01 * scale
        B = len(q)
        w = env.synth.make_workload(chain, B, 1, seed=3, io_dtype=dt)
        params = env.abi.default_params()
        ref = pr.far_reference(name, scale, dt, chain, q)
        E_R, E_p = pr.far_units(chain)
        reach = E_p / E_R
        o_rot, o_pos = pr.far_errors(env.oc.cycle_batch(chain, params, q, w["fields"], w["nfields"], want=("pose",))["pose"], ref, np.float64)
        R = max(float(o_rot.max()) / E_R, float(o_pos.max()) / E_p)
        K = hp.K_MARGIN * max(1.0, R)
        term = pr.far_angle_term(q, offsets)
        forms = [("eight-lanes", True)] if sub8 else [("pattern", False), ("general", True)]
        for form, adds in forms:
            eng = env.engine.Engine(chain, B, io_dtype=dt, max_slots=8, params=params)
            try:
                eng.set_fields(w["fields"], w["nfields"])
                eng.set_small_batch_kernel(B if sub8 else 0)
                eng.launched_kernels()
                lim = dict(q_lo=np.full_like(q, -4.0 * scale), q_hi=np.full_like(q, 4.0 * scale)) if form == "general" else {}
                got = eng.step_host(q, want=("qdot_out", "pose", "status"), **lim)
                launched = sorted(eng.launched_kernels())
            finally:
                eng.close()
            assert len(launched) == 1, launched
            if sub8:
                assert launched[0].startswith("cycle_sub8"), launched
            elif form == "general":
                assert not launched[0].startswith("cycle_sub8") and _d_bit(launched[0]) == 0, launched
            else:
                assert not launched[0].startswith("cycle_sub8")
                if _d_bit(launched[0]) == 0:      # no pattern variant for this chain and I/O type: this launch adds the offsets too
                    assert io == 64 and chain.n != 7, launched
                    adds = True
            assert np.isfinite(got["pose"]).all() and not pr.nan_bit(got["status"]).any()
            e_rot, e_pos = pr.far_errors(got["pose"], ref, dt)
            extra = term if adds else 0.0
            over = max(float((e_rot / (K * E_R + extra)).max()), float((e_pos / (K * E_p + reach * extra)).max()))
            units = max(float(e_rot.max()) / E_R, float(e_pos.max()) / E_p)
            line = "far angles %-16s float%d |q| ~ %-6g %-11s %s: oracle R = %5.2f, kernel %9.2f units (%.1e), bar K = %.0f units%s: error / bar %.3f%s" % (
                name, io, scale, form, launched[0].split("<")[0] + (" D=%d" % _d_bit(launched[0]) if not sub8 else ""), R, units,
                max(float(e_rot.max()), float(e_pos.max())), K, " + the offsets' term (up to %.1e rad)" % float(np.max(extra)) if adds else "", over,
                "" if over <= 1.0 else " -- FAILS")
            print(line)
            env.table.append(line)
            if not over <= 1.0:
                failures.append(line)
    assert not failures, "\n".join(failures)
