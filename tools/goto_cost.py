#!/usr/bin/env python
"""What the arrival check of a batched goto costs (vfik_goto), measured on one box in one session, on C3's batch: 65 536 arms, 7 joints,
goal + 8 obstacles, float32 I/O, 200 control cycles:

 (a) vfik_rollout of 200 cycles asking qdot_out only: the cycles alone, one launch;
 (b) the same cycles as 200 / s vfik_rollout calls of s cycles that also ask goal_dist and q_out (q ping-pongs between two device
     rows), s in {1, 4, 10, 50}: what a caller enqueued before vfik_goto existed, minus the host round trip -- THE YARDSTICK;
 (c) vfik_goto at the same strides, hold off and on, without and with the traces (q_traj, dist_traj);
     cost of a check = ((c) - (b)) / n_checks;
 (d) Engine.goto_host on the near-goal workload of tests/test_gpu_goto.py (every arm starts 0.02-0.25 rad from its goal) with a time-out
     of 2000 cycles: poll 8 against no poll, wall clock;
 the floor: one small dependent load -> store launch over as many lanes (tools/ubench_launch, 1024 workgroups of 64), in the same session.
 THE BAR: a check without traces costs at most 2 x that floor (the x 2: the wave atomic and the two extra row streams); with q_traj and
 dist_traj, plus the bytes of their rows at the rate profiles/move_fields_cost.txt reached (4.81 TB/s warm).
 (e) with --parent-root DIR (a built checkout of the parent commit): bench.py --gpus 1 --steps 200 --warmup 20 on the parent and on this
     build, alternating, each in a process of its own.  The cycle kernels are untouched: this build's median must lie inside the parent's
     own run-to-run spread.

HIP-event periods, every figure with median and spread; into profiles/goto_cost.txt (--out).  Exit status 1 when a bar is missed."""
import argparse
import ctypes as C
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(HERE, "profiles", "goto_cost.txt"))
ap.add_argument("--parent-root", default=None, help="a built checkout of the parent commit: part (e)")
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--bench-reps", type=int, default=4)
args = ap.parse_args()
sys.path.insert(0, HERE)
import torch  # noqa: E402

from vfclik_amd import _abi, engine, robots, synth  # noqa: E402

chain = robots.lwr()
L = []
failed = False


def say(s=""):
    print(s, flush=True)
    L.append(s)


def stats(xs):
    xs = np.sort(np.asarray(xs, dtype=np.float64))
    return "median %10.2f  min %10.2f  max %10.2f  (n = %d)" % (np.median(xs), xs[0], xs[-1], len(xs))


B, NOBS, K, R = 65536, 8, 200, args.reps
DT, PREC = 0.01, (0.01, 0.05)
STRIDES = (1, 4, 10, 50)
say("goto_cost -- tools/goto_cost.py; device: %s; ABI %d" % (torch.cuda.get_device_name(0), _abi.ABI_VERSION))
say("times in microseconds for the WHOLE sequence of %d control cycles unless a line says otherwise; HIP events around the sequence on one" % K)
say("stream, the host's enqueue time beside it (it may bound the period); %d repetitions after 2 untimed ones" % R)
say("batch: %d arms, 7 joints, float32 I/O, goal + %d obstacles (C3), flags 0, clamp on, dt %.2f, precision (%.2f m, %.2f rad)" % (B, NOBS, DT, PREC[0], PREC[1]))
say()

# ---- the floor ------------------------------------------------------------------------------------------------------------------
floor = None
ub = os.path.join(HERE, "tools", "ubench_launch")
if os.path.exists(ub):
    r = subprocess.run([ub], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    for ln in r.stdout.splitlines():
        m = re.match(r"\s*1024\s+([\d.]+)\s+([\d.]+)\s+([\d.]+)", ln)
        if m:
            floor = float(m.group(2))
            say("the floor (tools/ubench_launch, 1024 workgroups of 64 lanes, back-to-back period): empty %.2f, load+store %.2f, const+load+store %.2f us"
                % (float(m.group(1)), floor, float(m.group(3))))
if floor is None:
    say("the floor: tools/ubench_launch is not built (make -C tools ubench_launch): NOT measured, the bar below is not judged")
say()

stream = torch.cuda.current_stream().cuda_stream
w = synth.make_workload(chain, B, NOBS, seed=1, io_dtype=np.float32)
eng = engine.Engine(chain, B, io_dtype=np.float32, max_slots=8, params=_abi.default_params(max_vel=0.7))
eng.set_fields(w["fields"], w["nfields"])
eng.use_stream(stream)
dev = torch.device("cuda", 0)
q0 = torch.from_numpy(w["q"].astype(np.float32)).to(dev)
qdot = torch.zeros(B, 7, device=dev)
gdist = torch.zeros(B, 2, device=dev)
qpp = [torch.zeros(B, 7, device=dev), torch.zeros(B, 7, device=dev)]
arrived = torch.zeros(B, dtype=torch.int32, device=dev)
pending = torch.zeros(K, dtype=torch.int32, device=dev)
q_traj = torch.zeros(K, B, 7, device=dev)
d_traj = torch.zeros(K, B, 2, device=dev)


def timed(fn):
    per, enq = [], []
    for r in range(R + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        t0 = time.perf_counter()
        fn()
        t1 = time.perf_counter()
        e1.record()
        torch.cuda.synchronize()
        if r >= 2:
            per.append(e0.elapsed_time(e1) * 1e3)
            enq.append((t1 - t0) * 1e6)
    return per, enq


def report(label, per, enq):
    say("    %-44s period  %s" % (label, stats(per)))
    say("    %-44s enqueue %s" % ("", stats(enq)))
    return float(np.median(per))


say("(a) vfik_rollout of %d cycles, qdot_out only (one launch)" % K)
io_a = eng.make_io(q0, qdot_out=qdot)
t_a = report("rollout(200)", *timed(lambda: eng.rollout(io_a, K, DT, clamp=True)))
say("    = %.2f us per cycle" % (t_a / K))
say()

say("(b) THE YARDSTICK: %d / s vfik_rollout calls of s cycles, each asking qdot_out, goal_dist and q_out" % K)
t_b = {}
for s in STRIDES:
    ios = [eng.make_io(q0 if k == 0 else qpp[(k - 1) & 1], qdot_out=qdot, goal_dist=gdist) for k in range(3)]

    def run_b(s=s, ios=ios):
        for k in range(K // s):
            eng.rollout(ios[0] if k == 0 else ios[1 + ((k - 1) & 1)], s, DT, q_out=qpp[k & 1], clamp=True)
    t_b[s] = report("s = %2d: %3d x rollout(%d)" % (s, K // s, s), *timed(run_b))
say()

say("(c) vfik_goto, n_cycles %d; cost of a check = ((c) - (b)) / n_checks" % K)
io_c = eng.make_io(q0, qdot_out=qdot)
check = {}
for traces in (False, True):
    for hold in (False, True):
        for s in STRIDES:
            n = K // s
            kw = dict(arrived=arrived, pending=pending[:n])
            if traces:
                kw.update(q_traj=q_traj[:n], dist_traj=d_traj[:n])
            label = "s = %2d, hold %s, %s" % (s, "on " if hold else "off", "q_traj + dist_traj" if traces else "no trace")
            t = report(label, *timed(lambda: eng.goto(io_c, K, DT, PREC, stride=s, hold=hold, clamp=True, **kw)))
            check[traces, hold, s] = (t - t_b[s]) / n
            say("    %-44s a check costs (%.2f - %.2f) / %d = %.2f us" % ("", t, t_b[s], n, check[traces, hold, s]))
torch.cuda.synchronize()
say("    arms that arrived in these %d cycles from C3's random starts: %d of %d" % (K, int((arrived >= 0).sum()), B))
say()
row_us = (B * 7 * 4 + B * 2 * 4) / 4.81e6   # bytes of a q row and a distance row at 4.81 TB/s, in us
say("THE BAR: a check costs at most 2 x the floor; with the traces, plus %.2f us (a q row and a distance row, %.2f MB, at 4.81 TB/s)" % (row_us, (B * 9 * 4) / 1e6))
if floor is not None:
    for (traces, hold, s), c in sorted(check.items()):
        bar = 2 * floor + (row_us if traces else 0.0)
        ok = c <= bar
        failed |= not ok
        say("    s = %2d, hold %s, %-18s: %6.2f us per check, bar %.2f us : %s" % (s, "on " if hold else "off", "q_traj + dist_traj" if traces else "no trace", c, bar,
                                                                                 "PASS" if ok else "MISSED"))
if failed:
    say("    What the excess is made of is NOT measured here.  A check is one launch of check_kernel<T, 0, 0>: a kernel boundary, 2.4 MB of rows and, while")
    say("    most arms are under way, one atomic add per wave -- 1024 waves adding to ONE word, pending[k].  Adds of every wave of the chip to a")
    say("    single address are the first suspect (same-address atomics serialise); a per-block sum in front of the atomic is the experiment to make.")
say()
eng.close()
del q_traj, d_traj

# ---- (d) ------------------------------------------------------------------------------------------------------------------------
say("(d) Engine.goto_host, near-goal workload (tests/test_gpu_goto.py: start 0.02-0.25 rad from the goal), time-out 2000 cycles, stride 4, hold on:")
say("    wall clock of the call in MILLISECONDS, host arrays in and out (q, arrived, pending, qdot_out)")
Bd = 65536
wd = synth.make_workload(chain, Bd, NOBS, seed=53, io_dtype=np.float32)
rng = np.random.default_rng(7)
qg = rng.uniform(0.7 * chain.q_lo, 0.7 * chain.q_hi, size=(Bd, 7))
sd = rng.uniform(0.02, 0.25, size=(Bd, 1))
qs = (qg + sd * rng.uniform(-1.0, 1.0, size=(Bd, 7))).astype(np.float32)
wd["fields"]["p"][:, 0, :16] = chain.fk(qg).reshape(Bd, 16).astype(np.float32)
eng = engine.Engine(chain, Bd, io_dtype=np.float32, max_slots=8, params=_abi.default_params(max_vel=0.7))
eng.set_fields(wd["fields"], wd["nfields"])
for poll in (0, 8):
    ts, ran, left = [], None, None
    for r in range(5):
        t0 = time.perf_counter()
        got = eng.goto_host(qs, 2000, DT, PREC, stride=4, hold=True, clamp=True, poll=poll)
        ts.append((time.perf_counter() - t0) * 1e3)
        ran, left = got["checks_run"], int(got["pending"][-1])
    say("    poll %d: %s ms; checks run %d of 500, arms still under way at the end %d, arrived %d of %d"
        % (poll, stats(ts[1:]), ran, left, int((got["arrived"] >= 0).sum()), Bd))
if left:
    say("    %d arms of this workload are not there after 2000 cycles: pending never reaches 0, so no poll can end this goto early -- the" % left)
    say("    difference between the two lines is what 62 polls (a 4-byte copy and a synchronisation each) cost.  The early exit itself is")
    say("    shown by tests/test_gpu_goto.py::test_early_exit on a batch of arms that all arrive.")
eng.close()
say()

# ---- (e) ------------------------------------------------------------------------------------------------------------------------
say("(e) bench.py --gpus 1 --steps 200 --warmup 20, parent and this build alternating, a process each: ms_per_step")
if args.parent_root is None:
    say("    not measured (no --parent-root)")
else:
    vals = {"parent": [], "this build": []}
    for r in range(args.bench_reps):
        for label, root in (("parent", args.parent_root), ("this build", HERE)):
            p = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "200", "--warmup", "20"], cwd=root, stdout=subprocess.PIPE,
                               stderr=subprocess.PIPE, text=True, timeout=600)
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
            if p.returncode != 0 or not line:
                say("    %s: FAILED (exit %d)" % (label, p.returncode))
                failed = True
                continue
            vals[label].append(json.loads(line[-1])["ms_per_step"] * 1e3)
    for label, v in vals.items():
        if v:
            say("    %-10s us per step: %s   runs: %s" % (label, stats(v), " ".join("%.3f" % x for x in v)))
    if vals["parent"] and vals["this build"]:
        pm, spread = float(np.median(vals["parent"])), max(vals["parent"]) - min(vals["parent"])
        tm = float(np.median(vals["this build"]))
        ok = tm <= pm + spread
        failed |= not ok
        say("    THE BAR: this build's median %.3f is not above the parent's %.3f by more than the parent's own spread %.3f : %s" % (tm, pm, spread, "PASS" if ok else "MISSED"))

os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(L) + "\n")
sys.exit(1 if failed else 0)
