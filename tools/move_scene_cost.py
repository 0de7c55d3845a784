#!/usr/bin/env python
"""What a goalAndNormal target that moves costs (vfik_move_scene), measured on one box in one session:

 (a) wall clock of Engine.set_fields for the batch -- what a moving goalAndNormal target costs without vfik_move_scene, because a funnel
     with new coordinates was a change of structure: 65 536 arms, 7 joints, goal + approach funnel + near-goal repeller + 8 obstacles
     (field path 2), float32 I/O;
 (b) HIP-event period of 200 x [move_scene], 200 x [step] and 200 x [move_scene; step], for a move of goal + funnel + near-goal repeller
     (what the feeder re-sends for the target, object_feeder:248-303) and for a move of everything (the 8 obstacles too), warm (one handle)
     and cold (handles launched round-robin, more than the 256 MiB Infinity Cache touched between two uses of one); the host's enqueue
     cost per iteration beside each period, because it may bound it; the bytes a move reads and writes and the rate they imply;
 (c) with --parent-root DIR (a built checkout of the parent commit): tools/move_cost.py on the parent and on this build, each in a process
     of its own -- the cost of the OLD call, vfik_move_fields (goal + 8 repellers, C3), and of [move; step]; Engine.set_fields of that
     batch on both (it now packs and uploads three more slot maps).  THE BAR: this build's medians of the two periods are not above the
     parent's by more than the spread (max - min) of the parent's own repetitions; the tool exits non-zero otherwise.

Every figure with its median and spread, into profiles/move_scene_cost.txt (--out)."""
import argparse
import ctypes as C
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(HERE, "profiles", "move_scene_cost.txt"))
ap.add_argument("--parent-root", default=None, help="a built checkout of the parent commit: part (c)")
ap.add_argument("--cold-sets", type=int, default=8)
args = ap.parse_args()
sys.path.insert(0, HERE)
import torch  # noqa: E402

from vfclik_amd import _abi, engine, robots, synth  # noqa: E402

chain = robots.lwr()
L = []


def say(s=""):
    print(s, flush=True)
    L.append(s)


def stats(xs):
    xs = np.sort(np.asarray(xs, dtype=np.float64))
    return "median %9.2f  min %9.2f  p10 %9.2f  p90 %9.2f  max %9.2f  (n = %d)" % (
        np.median(xs), xs[0], xs[int(0.1 * (len(xs) - 1))], xs[int(round(0.9 * (len(xs) - 1)))], xs[-1], len(xs))


def workload(B, nobs, seed):
    """goalAndNormal + obstacles as the feeder numbers them: goal 1, funnel 2 (force 30), near-goal repeller 3, obstacles 4..."""
    w = synth.make_workload(chain, B, nobs, seed=seed, io_dtype=np.float32, max_fields=nobs + 3)
    F = w["fields"]
    i = 1 + nobs
    F["id"][:, i], F["type"][:, i], F["force"][:, i] = 2, 5, 30.0
    F["p"][:, i, 0:3] = F["p"][:, 0, [3, 7, 11]]
    F["p"][:, i, 3:6] = F["p"][:, 0, [2, 6, 10]]
    F["p"][:, i, 6:10] = [0.15, 10.0, 0.15, 2.0]
    F["id"][:, i + 1], F["type"][:, i + 1], F["force"][:, i + 1] = 3, 2, -10.0
    F["p"][:, i + 1, 0:3] = F["p"][:, 0, [3, 7, 11]] - 0.05 * F["p"][:, 0, [2, 6, 10]]
    F["p"][:, i + 1, 3:6] = [0.2, 0.001, 5.0]
    w["nfields"][:] = nobs + 3
    return w


B, NOBS, K, R, ESZ = 65536, 8, 200, 15, 4
SLOTS = 2 + 1 + NOBS
say("move_scene_cost -- tools/move_scene_cost.py; device: %s; ABI %d" % (torch.cuda.get_device_name(0), _abi.ABI_VERSION))
say("times in microseconds; medians with min / p10 / p90 / max over the repetitions named")
say("scene: %d arms, 7 joints, float32 I/O, goal + approach funnel + near-goal repeller + %d obstacles (set goalAndNormal + %d x set ObstacleP)"
    % (B, NOBS, NOBS))
say()

# ---- (a) ------------------------------------------------------------------------------------------------------------------------
say("(a) Engine.set_fields of the batch, wall clock (host sort + pack + copies + synchronisations): a moving goalAndNormal target on the parent")
w = workload(B, NOBS, 1)
eng = engine.Engine(chain, B, io_dtype=np.float32, max_slots=SLOTS)
eng.set_fields(w["fields"], w["nfields"])
assert eng.field_path == 2, eng.field_path
ts = []
for _ in range(9):
    t0 = time.perf_counter()
    eng.set_fields(w["fields"], w["nfields"])
    ts.append((time.perf_counter() - t0) * 1e6)
set_med = float(np.median(ts))
say("    %6d arms: %s" % (B, stats(ts)))
eng.close()
say()

# ---- (b) ------------------------------------------------------------------------------------------------------------------------
# per arm: rows read + one 16-bit map entry per repeller / funnel row + the goal's `present` quad; written: goal rows 0-2 (48 B), per
# repeller the uniform quad, the compact slot and the general quad (48 B), per funnel quad + pair in the general image and the aux block (48 B)
BYTES = {
    "target": (B * ((16 + 4 + 6) * ESZ + 2 * 2 + 4 * ESZ), B * (12 + 12 + 12) * ESZ),
    "everything": (B * ((16 + (1 + NOBS) * 4 + 6) * ESZ + (2 + NOBS) * 2 + 4 * ESZ), B * (12 + (1 + NOBS) * 12 + 12) * ESZ),
}
say("(b) HIP-event period of %d back-to-back iterations on one stream, %d repetitions" % (K, R))
say("    target     = goal + funnel + near-goal repeller: reads %.1f MB, writes %.1f MB" % (BYTES["target"][0] / 1e6, BYTES["target"][1] / 1e6))
say("    everything = target + the %d obstacles:          reads %.1f MB, writes %.1f MB" % (NOBS, BYTES["everything"][0] / 1e6, BYTES["everything"][1] / 1e6))
stream = torch.cuda.current_stream().cuda_stream
sets = []
for k in range(args.cold_sets):
    w = workload(B, NOBS, 1 + k)
    eng = engine.Engine(chain, B, io_dtype=np.float32, max_slots=SLOTS)
    eng.set_fields(w["fields"], w["nfields"])
    assert eng.field_path == 2
    eng.use_stream(stream)
    q = torch.from_numpy(w["q"].astype(np.float32)).cuda()
    out = torch.zeros(B, 7, dtype=torch.float32, device="cuda")
    P = w["fields"]["p"]
    goal = torch.from_numpy(np.ascontiguousarray(P[:, 0, :16]).astype(np.float32)).cuda()
    fun = torch.from_numpy(np.ascontiguousarray(P[:, 1 + NOBS:2 + NOBS, :6]).astype(np.float32)).cuda()
    # ascending id: the near-goal repeller (3) is decay repeller 0, the obstacles (4 ...) follow
    rep = torch.from_numpy(np.ascontiguousarray(np.concatenate([P[:, 2 + NOBS:3 + NOBS, :4], P[:, 1:1 + NOBS, :4]], axis=1)).astype(np.float32)).cuda()
    step = eng.stepper(eng.make_io(q, qdot_out=out))
    calls = {}
    for name, n_rep in (("target", 1), ("everything", 1 + NOBS)):
        mv = _abi.SceneMove()
        mv.goal16, mv.rep4, mv.fun6, mv.n_rep, mv.n_fun = goal.data_ptr(), rep.data_ptr(), fun.data_ptr(), n_rep, 1
        if name == "target":     # rows of ONE repeller per arm: a tensor of its own
            rep1 = rep[:, :1].contiguous()
            mv.rep4 = rep1.data_ptr()
            calls["keep"] = rep1

        def move(fn=eng.lib.vfik_move_scene, h=eng.h, mv=mv):
            if fn(h, 0, B, C.byref(mv)):
                raise RuntimeError("vfik_move_scene failed")
        calls[name] = move
    sets.append((eng, step, calls, (q, out, goal, fun, rep)))
torch.cuda.synchronize()
res = {}
for state, use in (("warm", sets[:1]), ("cold", sets)):
    for what in ("step", "target", "target+step", "everything", "everything+step"):
        per, enq = [], []
        for r in range(R + 2):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            t0 = time.perf_counter()
            for i in range(K):
                _, step, calls, _ = use[i % len(use)]
                if what != "step":
                    calls[what.split("+")[0]]()
                if what.endswith("step"):
                    step()
            t1 = time.perf_counter()
            e1.record()
            torch.cuda.synchronize()
            if r >= 2:               # two untimed repetitions warm every shape up
                per.append(e0.elapsed_time(e1) * 1e3 / K)
                enq.append((t1 - t0) * 1e6 / K)
        res[state, what] = (float(np.median(per)), float(np.median(enq)))
        say("    %s  [%-15s]  period  %s" % (state, what, stats(per)))
        say("    %s  [%-15s]  enqueue %s" % (state, what, stats(enq)))
    for name in ("target", "everything"):
        t, e = res[state, name]
        rd, wr = BYTES[name]
        say("    %s: move_scene of %s alone, %.2f us per launch: %.1f MB in %.2f us = %.2f TB/s (vfik_move_fields: 4.8 TB/s warm, profiles/move_fields_cost.txt)%s" % (
            state, name, t, (rd + wr) / 1e6, t, (rd + wr) / t / 1e6, "  (the enqueue, %.2f us, bounds this period)" % e if e > 0.9 * t else ""))
    say("    %s: [move_scene(target); step] %.2f us against [step] %.2f us; through set_fields: %.0f us + step = %.0fx that period" % (
        state, res[state, "target+step"][0], res[state, "step"][0], set_med, (set_med + res[state, "step"][0]) / res[state, "target+step"][0]))
for eng, *_ in sets:
    eng.close()
del sets
say()

# ---- (c) ------------------------------------------------------------------------------------------------------------------------
say("(c) the OLD call on the parent and on this build: tools/move_cost.py part (b), C3 (goal + 8 repellers, 65 536 arms, float32 I/O)")
failed = False
if args.parent_root is None:
    say("    not measured (no --parent-root)")
else:
    got = {}
    for label, root in (("parent", args.parent_root), ("this build", HERE)):
        with tempfile.TemporaryDirectory() as tmp:
            r = subprocess.run([sys.executable, os.path.join(HERE, "tools", "move_cost.py"), "--root", root, "--out", os.path.join(tmp, "cost.txt")],
                               stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
        lines = [s for s in r.stdout.splitlines() if re.match(r"\s+C3  (warm|cold)\s+\[(move|move\+step|step)\s*\]\s+period", s)]
        sets = [s for s in r.stdout.splitlines() if re.match(r"\s+\d+ arms: median", s)]     # its part (a): set_fields now packs three more maps
        if r.returncode != 0 or len(lines) != 6:
            say("  %s: FAILED (exit %d): %s" % (label, r.returncode, r.stderr.strip().splitlines()[-1] if r.stderr.strip() else ""))
            failed = True
            continue
        say("  %s:" % label)
        for s in sets:
            say("    Engine.set_fields, goal + 8 obstacles, %s" % s.strip())
        for s in lines:
            say(s)
            m = re.match(r"\s+C3  (\w+)\s+\[([a-z+]+)\s*\]\s+period\s+median\s+([\d.]+)\s+min\s+([\d.]+).*max\s+([\d.]+)", s)
            got[label, m.group(1), m.group(2)] = tuple(float(m.group(i)) for i in (3, 4, 5))
    say("  THE BAR: this build's median is not above the parent's by more than the parent's own spread (max - min)")
    for state in ("warm", "cold"):
        for what in ("move", "move+step"):
            if ("parent", state, what) not in got or ("this build", state, what) not in got:
                continue
            pm, plo, phi = got["parent", state, what]
            tm = got["this build", state, what][0]
            ok = tm <= pm + (phi - plo)
            failed |= not ok
            say("    C3 %s [%-9s]: parent %.2f (spread %.2f), this build %.2f : %s" % (state, what, pm, phi - plo, tm, "PASS" if ok else "FAIL"))

os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(L) + "\n")
sys.exit(1 if failed else 0)
