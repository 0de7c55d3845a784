"""Every cycle-kernel instantiation the library ships, run once against the CPU oracle.

The variants are read from the built library (tests/kernel_variants.py), never from a list written here: a variant added to the
build without a recipe below fails its group.  A recipe maps a variant's template arguments to an engine configuration -- chain,
I/O type, flag set, shared tool and IK weights, field set, batch size, what the launch asks for -- and the test asserts that the
launch took exactly that variant (Engine.launched_kernels) and that every output it wrote equals the oracle's: qdot_out and status,
the published rows, the integrated q of a rollout, and for the nullspace module a second cycle that reads the sign memory back.
Each feature a recipe turns on (tool, weights, aux block, differing orders, nullspace module, joint-limit task, repellers) must move
the oracle's result by 1e-3 somewhere in the batch, or the case could not catch a bug in it.

One test per object the library is compiled in: joint count x I/O type x nullspace module or not."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_variants as kv  # noqa: E402

pytestmark = pytest.mark.gpu

GROUPS = [(n, t, ns) for n in (6, 7, 10, 14) for t in (32, 64) for ns in (False, True)]
ROWS = ("qdot_vf", "qdot_null", "qdot_out", "pose", "pose_nt", "qdist", "status")
LEAN = ("qdot_out", "status")
B_SMALL = 64 * 3 + 13           # a partial last wave, not a multiple of 8 either (the eight-lanes kernel's blocks)
B_BIG = 65536 + 64 * 2 + 37     # beyond one wave per SIMD (256 CUs): the two-waves launches
ROLL_K, ROLL_DT = 6, 0.01
FEATURE_MIN = 1e-3


@pytest.fixture(scope="module")
def env():
    import __graft_entry__ as g
    g.build()
    from oracle import oracle_c
    from vfclik_amd import _abi, chain, engine, robots, synth

    class E:
        pass

    e = E()
    e.oc, e.abi, e.chain, e.engine, e.robots, e.synth = oracle_c, _abi, chain, engine, robots, synth
    e.variants = kv.by_group()
    return e


# ---- chains ----------------------------------------------------------------------------------------------------------
def _chain(env, nj, pattern):
    """The chain of a joint count, on its DH pattern (vfik_kernel.h: DhPattern) or with one link off it (an a-offset)."""
    R, Chain = env.robots, env.chain.Chain
    lwr_dh, lwr_lim = list(R._LWR_DH), R._LWR_LIM
    off = list(lwr_dh)
    off[2] = (0.05, -math.pi / 2, 0.4, 0.0)
    if nj == 7:
        return R.lwr() if pattern else Chain.from_dh(off, -lwr_lim, lwr_lim, name="lwr_off")
    if nj == 14:
        return R.lwr_dual14() if pattern else Chain.from_dh(off, -lwr_lim, lwr_lim).concat(R.lwr(), name="dual14_off")
    if nj == 6:
        if pattern:
            return R.powercube6()
        dh = [(0.02, math.pi / 2, 0.30, 0.0), (0.35, 0.0, 0.0, 0.0), (0.0, math.pi / 2, 0.0, 0.0), (0.0, -math.pi / 2, 0.30, 0.0),
              (0.0, math.pi / 2, 0.0, 0.0), (0.0, 0.0, 0.10, 0.0)]
        lim = np.array([170, 120, 150, 170, 120, 170], dtype=float) * math.pi / 180
        return Chain.from_dh(dh, -lim, lim, name="powercube6_off")
    assert nj == 10 and not pattern   # (no pattern is built for 10 joints)
    return kv.chain10(R, Chain)


def _tool(i=0):
    t = np.eye(4)
    t[:3, 3] = [0.02, -0.01 + 0.001 * (i % 7), 0.2]
    c, s = np.cos(0.3), np.sin(0.3)
    t[:3, :3] = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]]) @ np.array([[1, 0, 0], [0, np.cos(0.2), -np.sin(0.2)], [0, np.sin(0.2), np.cos(0.2)]])
    return t.reshape(16)


# ---- the recipe: template arguments -> configuration ----------------------------------------------------------------
class Recipe:
    """What a variant needs.  `key` is the handle's configuration (variants with the same key share one handle); the rest is what the
    launch asks for: outputs, the eight-lanes cap, per-arm limits, a rollout.  `b_small` / `b_big`: the batch of a one-wave-per-SIMD and of
    a two-waves variant (tests/test_gpu_extents.py also runs a batch whose last wave is full)."""

    def __init__(self, v, b_small=B_SMALL, b_big=B_BIG):
        a = v.args
        sub8 = v.kernel.startswith("cycle_sub8")
        self.v = v
        self.nj, self.t = a["NJ"], np.float32 if a["T"] == "float" else np.float64
        self.ns = a["NS"]
        d = a["D"]
        self.pattern, self.shared_tool, self.shared_wts = bool(d & 1), bool(d & 2), bool(d & 4)
        self.mixo = v.kernel == "cycle_kernel_m"
        cf = a.get("CF", -1)
        if sub8 or self.mixo:
            cf = 7
        # the nullspace module: a compiled-in flag set, or NULLSPACE | JOINT_LIMIT_TASK | MIXER | LIMITER (not one of them: CF = -1)
        self.flags = (cf if cf != -1 else 15) if self.ns else 0
        self.plain = a.get("PL", True)
        self.per_arm_tool = not self.plain     # (tools that differ between arms: the general variants)
        self.fastf = a.get("FASTF", True)
        self.fun = a.get("FUN", False)
        self.uni = a.get("UNI", False)
        self.big = a.get("WAVES", 1) == 2
        self.B = b_big if self.big else b_small
        lean = 3 if sub8 else a["LEAN"]
        self.roll = a.get("ROLL", False) or lean == 2
        self.cap = self.B if sub8 else 0
        # per-arm q_lo / q_hi: a run-time option that keeps a launch of a PLAIN chain off the lean and publishing-lean variants
        self.limits = lean == 0 and self.plain and not self.roll
        if lean == 1:
            self.want = ("qdot_out",) if self.roll else LEAN
        elif lean == 2:
            self.want = ("qdot_out",)
        elif lean == 3:
            self.want = ROWS
        else:
            self.want = ("qdot_out", "pose") if self.roll and self.fastf else ("qdot_out",) if self.roll else ROWS
        if not self.fastf:
            self.fields = "general"
        elif self.mixo:
            self.fields = "mixo_fun" if self.fun else "mixo"
        elif self.fun:
            self.fields = "fun"
        else:
            self.fields = "uni" if (self.uni or sub8) else "pairs"
        # /control into the null space (nullspace:137-176): what makes the module act where the flag set has no joint-limit task.  A lean
        # launch takes none: there the module's output is its sign memory, read back by a second, publishing cycle that takes /control.
        # (Honoured where the null space is one-dimensional only -- include/vfik.h, vfik_io.null_control: chains of up to 7 joints.)
        self.ctrl = self.ns and self.nj <= 7 and lean != 1 and not self.roll
        self.readback = self.ns and self.nj <= 7 and lean == 1 and not self.roll and not (self.flags & 2)
        self.key = (self.pattern, self.plain, self.shared_tool, self.shared_wts, self.flags, self.fields, self.B)

    def __repr__(self):
        return "Recipe(pattern=%s plain=%s tool=%s weights=%s flags=%d fields=%s B=%d want=%s cap=%d limits=%s roll=%s)" % (
            self.pattern, self.plain, self.shared_tool, self.shared_wts, self.flags, self.fields, self.B, ",".join(self.want),
            self.cap, self.limits, self.roll)


def _fields(env, chain, B, kind, dt, seed):
    w = env.synth.make_workload(chain, B, 5, seed=seed, io_dtype=dt, max_fields=8)
    F, nf = w["fields"], w["nfields"]

    def cast(x):
        return float(dt(x))
    F["p"][:, 1, 3] = cast(0.25)   # one wide obstacle: the repellers act on many arms
    if kind == "pairs":       # two (safe distance, force) pairs: the compact image
        F["force"][:, 3] = -20.0
    elif kind == "general":   # a fractional decay order: the general field path
        F["p"][:, 2, 5] = 4.5
    if kind in ("mixo", "mixo_fun"):   # integer orders that differ
        F["p"][:, 1:3, 5] = 2.0
    if kind in ("fun", "mixo_fun"):   # the aux block: a funnel at the goal and a hemisphere repeller behind it
        F["id"][:, 6], F["type"][:, 6], F["force"][:, 6] = 2, env.abi.FIELD_FUNNEL, 30.0
        F["p"][:, 6, 0:3] = F["p"][:, 0, [3, 7, 11]]
        F["p"][:, 6, 3:6] = F["p"][:, 0, [2, 6, 10]]
        F["p"][:, 6, 6:10] = [cast(0.15), 10.0, cast(0.15), 2.0]
        F["id"][:, 7], F["type"][:, 7], F["force"][:, 7] = 3, env.abi.FIELD_HEMISPHERE, -10.0
        F["p"][:, 7, 0:3] = F["p"][:, 0, [3, 7, 11]] - 0.1 * F["p"][:, 0, [2, 6, 10]]
        F["p"][:, 7, 3:6] = F["p"][:, 0, [2, 6, 10]]
        F["p"][:, 7, 6:8] = [cast(0.05), 5.0]
        for k in (6, 7):
            F["p"][:, k, :8] = F["p"][:, k, :8].astype(dt).astype(np.float64)
        nf[:] = 8
    else:
        nf[:] = 6
    return w


class Handle:
    """One engine and the inputs of one configuration, with the oracle's view of them."""

    def __init__(self, env, r, seed):
        self.env = env
        self.chain = _chain(env, r.nj, r.pattern)
        n, B, dt = r.nj, r.B, r.t
        rng = np.random.default_rng(seed)
        self.w = _fields(env, self.chain, B, r.fields, dt, seed)
        wts = {}
        if r.shared_wts:
            wts = dict(wy=[1.0, 1.0, 1.0, 0.3, 0.3, 0.1], wq=list(rng.uniform(0.2, 1.0, n)) + [1.0] * (16 - n))
        self.params = env.abi.default_params(flags=r.flags, **wts)
        self.tool = None
        if r.shared_tool:
            self.tool = _tool()
        elif r.per_arm_tool:
            self.tool = np.stack([_tool(i) for i in range(B)])
            self.tool[:, 3] += rng.uniform(-0.01, 0.01, B)
            self.tool = self.tool.astype(dt).astype(np.float64)
        lo, hi = self.chain.q_lo, self.chain.q_hi
        self.q_lo = (np.tile(0.9 * lo, (B, 1)) + rng.uniform(0.0, 0.1, (B, n))).astype(dt).astype(np.float64)
        self.q_hi = (np.tile(0.9 * hi, (B, 1)) - rng.uniform(0.0, 0.1, (B, n))).astype(dt).astype(np.float64)
        self.ctrl = rng.uniform(-1, 1, (B, 4)).astype(dt).astype(np.float64)
        self.q2 = np.clip(self.w["q"] + rng.normal(0, 0.05, (B, n)), 0.85 * lo, 0.85 * hi).astype(dt).astype(np.float64)
        self.eng = env.engine.Engine(self.chain, B, io_dtype=dt, max_slots=10, params=self.params)
        self.eng.set_fields(self.w["fields"], self.w["nfields"])
        if self.tool is not None:
            self.eng.set_tool(self.tool, per_arm=self.tool.ndim == 2)
        # the handle is what its recipe says: field path, uniform image, differing orders
        assert self.eng.field_path == (0 if r.fields == "general" else 2 if r.fields in ("fun", "mixo_fun") else 1), r
        assert self.eng.uniform_repellers == (r.fields not in ("pairs", "general")), r
        assert self.eng.mixed_orders == (r.fields in ("mixo", "mixo_fun")), r
        # the oracle's sample: every arm of a small batch; of a big one the first and the last (partial) wave and 1 000 more
        if B > 4096:
            last = (B - 1) // 64 * 64
            self.idx = np.unique(np.concatenate([np.arange(64), np.arange(last, B), rng.choice(np.arange(64, last), 1000, replace=False)]))
        else:
            self.idx = np.arange(B)

    def oracle(self, q, want, params=None, fields=None, nfields=None, tool="same", states=None, limits=False, ctrl=False):
        """The oracle on the sample; q is the whole batch's."""
        i = self.idx
        F = self.w["fields"] if fields is None else fields
        nf = self.w["nfields"] if nfields is None else nfields
        t = self.tool if isinstance(tool, str) else tool
        if t is not None and t.ndim == 2:
            t = t[i]
        kw = dict(q_lo=self.q_lo[i], q_hi=self.q_hi[i]) if limits else {}
        if ctrl:
            kw["null_control"] = self.ctrl[i]
        return self.env.oc.cycle_batch(self.chain, params or self.params, q[i], F[i], nf[i], tool=t, states=states,
                                       want=tuple(k for k in want if k != "q"), **kw)

    def close(self):
        self.eng.close()


def _cmp(got, ref, keys, tol, idx, what):
    """the differences, as strings"""
    bad = []
    for k in keys:
        g = np.asarray(got[k])[idx]
        if k == "status":
            if not np.array_equal(g, ref[k]):
                bad.append("%s: status differs on %d arms" % (what, int((g != ref[k]).sum())))
            continue
        err = np.abs(g.astype(np.float64) - ref[k])
        if not (np.all(np.isfinite(g)) and err.max() < tol):
            bad.append("%s: %s max|hip - oracle| = %.3e" % (what, k, float(np.nan_to_num(err, nan=np.inf).max())))
    return bad


def _with_flags(abi, params, flags):
    p = abi.Params.from_buffer_copy(params)
    p.flags = flags
    return p


def _features(h, r):
    """Each feature the recipe turns on must change the oracle's qdot_out by FEATURE_MIN somewhere in the (sampled) batch."""
    abi = h.env.abi
    q = h.w["q"]
    ctrl = r.ctrl or r.readback
    base = h.oracle(q, ("qdot_out",), limits=r.limits, ctrl=ctrl)["qdot_out"]
    offs = []
    if h.tool is not None:
        offs.append(("the tool", dict(tool=None)))
    if r.shared_wts:
        offs.append(("the IK weights", dict(params=_with_flags(abi, abi.default_params(), r.flags))))
    # (a 6-joint arm has no null space: the module's output is zero there by construction -- compared all the same)
    if r.ns and r.nj > 6:
        offs.append(("the nullspace module", dict(params=_with_flags(abi, h.params, 0))))
    if r.flags & abi.F_JOINT_LIMIT_TASK and r.nj > 6:
        offs.append(("the joint-limit task", dict(params=_with_flags(abi, h.params, r.flags & ~abi.F_JOINT_LIMIT_TASK))))
    F = h.w["fields"]
    rep = F.copy()
    rep["force"][rep["type"] == abi.FIELD_REPELLER] = 0.0
    offs.append(("the repellers", dict(fields=rep)))
    if r.fields in ("fun", "mixo_fun"):
        nf = h.w["nfields"].copy()
        nf[:] = 6
        offs.append(("the funnel and the hemisphere", dict(nfields=nf)))
    if r.fields in ("mixo", "mixo_fun"):
        same = F.copy()
        same["p"][:, 1:6, 5] = 5.0
        offs.append(("the differing orders", dict(fields=same)))
    bad = []
    for name, kw in offs:
        d = float(np.abs(h.oracle(q, ("qdot_out",), limits=r.limits, ctrl=ctrl, **kw)["qdot_out"] - base).max())
        if not d >= FEATURE_MIN:
            bad.append("%s contributes %.1e < %.0e" % (name, d, FEATURE_MIN))
    return bad


def _run(h, r):
    """The variant's launch(es) on the handle: (the kernels launched, the differences from the oracle)."""
    eng, env = h.eng, h.env
    tol = 1e-6 if r.t == np.float32 else 1e-9
    eng.set_small_batch_kernel(r.cap)
    eng.reset_state()
    eng.launched_kernels()   # (clears the record)
    states = env.oc.new_states(len(h.idx), r.nj) if r.ns else None
    lim = dict(q_lo=h.q_lo, q_hi=h.q_hi) if r.limits else {}
    bad = []
    if r.roll:   # the oracle stepped cycle by cycle on its own state
        got = eng.rollout_host(h.w["q"], ROLL_K, ROLL_DT, want=r.want, **lim)
        launched = eng.launched_kernels()
        q = h.w["q"].copy()
        for _ in range(ROLL_K):
            ref = h.oracle(q, r.want, states=states, limits=r.limits)
            q[h.idx] = q[h.idx] + ROLL_DT * ref["qdot_out"]
            if r.t == np.float32:
                q = q.astype(np.float32).astype(np.float64)
        bad += _cmp(got, {"q": q[h.idx]}, ("q",), 2e-5 if r.t == np.float32 else 1e-9, h.idx, "rollout")
    else:
        launched = set()
        for cycle, q in enumerate((h.w["q"], h.q2) if r.ns else (h.w["q"],)):
            want, ctrl = (ROWS, True) if (cycle and r.readback) else (r.want, r.ctrl)
            got = eng.step_host(q, null_control=h.ctrl if ctrl else None, want=want, **lim)
            launched |= eng.launched_kernels()
            ref = h.oracle(q, want, states=states, limits=r.limits, ctrl=ctrl)
            bad += _cmp(got, ref, want, tol, h.idx, "cycle %d" % (cycle + 1))
    return launched, bad + _features(h, r)


@pytest.mark.parametrize("nj,io,ns", GROUPS, ids=["nj%d-f%d-%s" % (n, t, "ns" if ns else "plain") for n, t, ns in GROUPS])
def test_every_built_variant_matches_the_oracle(env, nj, io, ns):
    variants = env.variants.get((nj, io, ns), [])
    assert variants, "the library has no cycle kernel for %d joints, float%d I/O, nullspace %s" % (nj, io, ns)
    failures, handles, ok = [], {}, 0
    try:
        for v in variants:
            try:
                r = Recipe(v)
            except Exception as e:   # (a) no recipe
                failures.append("%s: no recipe (%s: %s)" % (v.name, type(e).__name__, e))
                continue
            h = handles.get(r.key)
            if h is None:
                h = handles[r.key] = Handle(env, r, seed=1000 + 17 * len(handles))
            launched, bad = _run(h, r)
            if v.name not in launched:   # (b) another kernel took the launch
                failures.append("%s: not launched by %r, which took %s" % (v.name, r, sorted(launched)))
            elif bad:                    # (c) not the oracle's numbers
                failures.append("%s: %s" % (v.name, "; ".join(bad)))
            else:
                ok += 1
            if r.big:   # (a big handle serves one variant)
                handles.pop(r.key).close()
    finally:
        for h in handles.values():
            h.close()
    print("nj=%d float%d %s: %d of %d variants launched and matched" % (nj, io, "ns" if ns else "plain", ok, len(variants)))
    assert not failures, "%d of %d variants:\n" % (len(failures), len(variants)) + "\n".join(failures)
