#!/usr/bin/env python
"""What a scene that moves costs (ABI 6, vfik_move_fields), measured on one box with one build:

 (a) wall clock of Engine.set_fields (host sort + pack + six copies + two synchronisations; unchanged by ABI 6: the baseline) for the
     whole C3 batch (65 536 arms, 7 joints, goal + 8 obstacles, float32 I/O) and for 4 096 arms;
 (b) HIP-event period of 200 x [move_fields; step] against 200 x [step], and of 200 x [move_fields] alone, for C3 and C3N (nullspace +
     mixer), warm (one handle, cache-resident) and cold (handles launched round-robin, more than the 256 MiB Infinity Cache touched
     between two uses of one); the host's enqueue cost per iteration is reported beside each period, because it may bound it;
 (c) ControlCycleBatch.cycle() for 64 and 4 096 arms with every arm's goal re-sent on /vectorField/param each cycle -- on this build
     and, with --parent-root DIR (a built checkout of the parent commit), on the parent, each in a process of its own.

Every figure with its median and spread, into profiles/move_fields_cost.txt (--out).  THE BAR: (b)'s [move; step] period is below (a) +
one step; the tool exits non-zero when it is not."""
import argparse
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(HERE, "profiles", "move_fields_cost.txt"))
ap.add_argument("--root", default=HERE, help="import vfclik_amd from this tree (the child processes of part (c))")
ap.add_argument("--parent-root", default=None, help="a built checkout of the parent commit: part (c) is run there as well")
ap.add_argument("--ccb-child", action="store_true", help="part (c) only, lines on stdout")
ap.add_argument("--cold-sets", type=int, default=8)
args = ap.parse_args()
sys.path.insert(0, args.root)
from vfclik_amd import _abi, engine, ports as yarp, robots, synth  # noqa: E402
from vfclik_amd.vf_module import ControlCycleBatch  # noqa: E402

chain = robots.lwr()


def stats(xs):
    xs = np.sort(np.asarray(xs, dtype=np.float64))
    return "median %9.2f  min %9.2f  p10 %9.2f  p90 %9.2f  max %9.2f  (n = %d)" % (
        np.median(xs), xs[0], xs[int(0.1 * (len(xs) - 1))], xs[int(round(0.9 * (len(xs) - 1)))], xs[-1], len(xs))


# ---- (c) ------------------------------------------------------------------------------------------------------------------------
def ccb_lines():
    out = []
    for B in (64, 4096):
        bases = ["/%d/lwr/right" % i for i in range(B)]
        cb = ControlCycleBatch(chain, bases, io_dtype=np.float64, max_fields=8)
        rng = np.random.default_rng(1)
        q = rng.uniform(0.5 * chain.q_lo, 0.5 * chain.q_hi, (B, 7))
        goal = chain.fk(rng.uniform(0.5 * chain.q_lo, 0.5 * chain.q_hi, (B, 7))).reshape(B, 16)
        par = []
        for base in bases:
            p = yarp.BufferedPortBottle()
            p.open(base + "/test/param")
            yarp.Network.connect(base + "/test/param", base + "/vectorField/param")
            par.append(p)

        def send(step):
            for a in range(B):           # the feeder's goal bottle (object_feeder:229-241): add 1 1.0 1 (frame, slow-down)
                b = par[a].prepare(); b.clear(); b.addString("add"); b.addInt(1); b.addDouble(1.0); b.addInt(1)
                lst = b.addList()
                row = goal[a].copy()
                row[3] += 1e-4 * step
                for v in list(row) + [0.05]:
                    lst.addDouble(float(v))
                par[a].writeStrict()
                if step == 0:            # four obstacles that stand still
                    for k in range(4):
                        b = par[a].prepare(); b.clear(); b.addString("add"); b.addInt(4 + k); b.addDouble(-10.0); b.addInt(2)
                        lst = b.addList()
                        for v in (0.3 + 0.1 * k, -0.2, 0.4, 0.05, 0.001, 5.0):
                            lst.addDouble(float(v))
                        par[a].writeStrict()
        reps = 40 if B <= 64 else 12
        ts = []
        for step in range(reps + 2):
            send(step)
            cb.write_encoders(q)
            t0 = time.perf_counter()
            got = cb.cycle()
            t1 = time.perf_counter()
            assert got.all()
            if step >= 2:
                ts.append((t1 - t0) * 1e6)
        out.append("    %5d arms, every goal re-sent each cycle: cycle() us  %s" % (B, stats(ts)))
        cb.close()
    return out


if args.ccb_child:
    print("\n".join(ccb_lines()), flush=True)
    sys.exit(0)

import torch  # noqa: E402

L = []


def say(s=""):
    print(s, flush=True)
    L.append(s)


say("move_fields_cost -- tools/move_cost.py; device: %s; ABI %d" % (torch.cuda.get_device_name(0), _abi.ABI_VERSION))
say("times in microseconds; medians with min / p10 / p90 / max over the repetitions named")
say()

# ---- (a) ------------------------------------------------------------------------------------------------------------------------
say("(a) Engine.set_fields, wall clock (host pack + copies + synchronisations), goal + 8 obstacles, float32 I/O")
set_med = {}
for B in (65536, 4096):
    w = synth.make_workload(chain, B, 8, seed=1, io_dtype=np.float32)
    eng = engine.Engine(chain, B, io_dtype=np.float32, max_slots=8)
    eng.set_fields(w["fields"], w["nfields"])
    ts = []
    for _ in range(9):
        t0 = time.perf_counter()
        eng.set_fields(w["fields"], w["nfields"])
        ts.append((time.perf_counter() - t0) * 1e6)
    set_med[B] = float(np.median(ts))
    say("    %6d arms: %s" % (B, stats(ts)))
    eng.close()
say()

# ---- (b) ------------------------------------------------------------------------------------------------------------------------
B, NOBS, K, R = 65536, 8, 200, 15
ESZ = 4
rd = B * (16 + NOBS * 4) * ESZ + B * NOBS * 2 + B * 4 * ESZ          # the caller's rows + the 16-bit slot map + the goal's `present` quad
wr = B * (12 + NOBS * (4 + 4 + 4)) * ESZ                                # goal rows 0-2; per repeller: uniform quad, compact slot, general quad
say("(b) HIP-event period of %d back-to-back iterations on one stream, %d repetitions; 65 536 arms, goal + 8 obstacles, float32 I/O" % (K, R))
say("    a move of this batch reads %.1f MB (rows, slot map, goal flags) and writes %.1f MB (goal block, uniform, compact and general images)"
    % (rd / 1e6, wr / 1e6))
stream = torch.cuda.current_stream().cuda_stream
worst_ratio = 0.0
bar_lines = []
for wl, flags in (("C3", 0), ("C3N", 1 | 4)):
    sets = []
    for k in range(args.cold_sets):
        w = synth.make_workload(chain, B, NOBS, seed=1 + k, io_dtype=np.float32)
        eng = engine.Engine(chain, B, io_dtype=np.float32, max_slots=NOBS, params=_abi.default_params(flags=flags))
        eng.set_fields(w["fields"], w["nfields"])
        eng.use_stream(stream)
        q = torch.from_numpy(w["q"].astype(np.float32)).cuda()
        out = torch.zeros(B, 7, dtype=torch.float32, device="cuda")
        goal = torch.from_numpy(np.ascontiguousarray(w["fields"]["p"][:, 0, :16]).astype(np.float32)).cuda()
        rep = torch.from_numpy(np.ascontiguousarray(w["fields"]["p"][:, 1:1 + NOBS, :4]).astype(np.float32)).cuda()
        io = eng.make_io(q, qdot_out=out)
        step = eng.stepper(io)
        mv, h = eng.lib.vfik_move_fields, eng.h
        gp, rp = C.c_void_p(goal.data_ptr()), C.c_void_p(rep.data_ptr())

        def move(mv=mv, h=h, gp=gp, rp=rp):
            if mv(h, 0, B, gp, rp, NOBS, None):
                raise RuntimeError("vfik_move_fields failed")
        sets.append((eng, step, move, (q, out, goal, rep, io)))
    torch.cuda.synchronize()
    for state, use in (("warm", sets[:1]), ("cold", sets)):
        res = {}
        for what in ("step", "move", "move+step"):
            per, enq = [], []
            for r in range(R + 2):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                t0 = time.perf_counter()
                for i in range(K):
                    _, step, move, _ = use[i % len(use)]
                    if what != "step":
                        move()
                    if what != "move":
                        step()
                t1 = time.perf_counter()
                e1.record()
                torch.cuda.synchronize()
                if r >= 2:               # two untimed repetitions warm every shape up
                    per.append(e0.elapsed_time(e1) * 1e3 / K)
                    enq.append((t1 - t0) * 1e6 / K)
            res[what] = (float(np.median(per)), float(np.median(enq)))
            say("    %-3s %s  [%-9s]  period  %s" % (wl, state, what, stats(per)))
            say("    %-3s %s  [%-9s]  enqueue %s" % (wl, state, what, stats(enq)))
        t_move = res["move"][0]
        say("    %-3s %s: the move alone, %.2f us per launch: %.1f MB in %.2f us = %.2f TB/s = %.0f %% of 8 TB/s%s" % (
            wl, state, t_move, (rd + wr) / 1e6, t_move, (rd + wr) / t_move / 1e6, 100.0 * (rd + wr) / t_move / 1e6 / 8.0,
            "  (the enqueue, %.2f us, bounds this period)" % res["move"][1] if res["move"][1] > 0.9 * t_move else ""))
        bar = set_med[B] + res["step"][0]
        ok = res["move+step"][0] < bar
        worst_ratio = max(worst_ratio, res["move+step"][0] / bar)
        bar_lines.append("    %-3s %s: [move; step] %.2f us  <  set_fields %.0f us + step %.2f us = %.0f us : %s (%.0fx below)" % (
            wl, state, res["move+step"][0], set_med[B], res["step"][0], bar, "PASS" if ok else "FAIL", bar / res["move+step"][0]))
    for eng, *_ in sets:
        eng.close()
    del sets
say()
say("THE BAR: the [move; step] period is below set_fields + one step")
for s in bar_lines:
    say(s)
say()

# ---- (c) ------------------------------------------------------------------------------------------------------------------------
say("(c) ControlCycleBatch.cycle(), float64 I/O, goal + 4 obstacles per arm, EVERY arm's goal re-sent on /vectorField/param each cycle")
say("    (the time of cycle() alone: port polling, FieldSets.flush, one fused launch, one synchronisation; writing the bottles is not in it)")
for label, root in (("this build", HERE), ("parent", args.parent_root)):
    if root is None:
        say("  %s: not measured (no --parent-root)" % label)
        continue
    r = subprocess.run([sys.executable, os.path.join(HERE, "tools", "move_cost.py"), "--ccb-child", "--root", root],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    say("  %s:" % label)
    if r.returncode != 0:
        say("    FAILED (exit %d): %s" % (r.returncode, r.stderr.strip().splitlines()[-1] if r.stderr.strip() else ""))
    for line in r.stdout.rstrip("\n").splitlines():
        say(line)

os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(L) + "\n")
sys.exit(0 if worst_ratio < 1.0 else 1)
