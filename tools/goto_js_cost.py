#!/usr/bin/env python
"""What a check of vfik_goto_js costs over a check of vfik_goto, and a check of vfik_follow_js over one of vfik_goto_js, measured on one
box in one session, on C3's batch under joint control: 65 536 arms, 7 joints, goal + 8 obstacles, float32 I/O, mixer weights
[0, 0, 1, 0, 0, 0] with VFIK_F_MIXER, 200 control cycles, strides 4 / 10 / 50.

vfik_goto is existing code and the yardstick.  Every call gets the same options, hold off and an all-ones io->active, so that all run
every block under the handle's gate on every arm; io names goal_dist in all of them (a joint block asks the cycle kernel for it only then)
and the reference the controller reads is the same array -- the caller's io->q_ref for vfik_goto and vfik_goto_js, copied into the handle's
row by vfik_follow_js.  The cycle launches are then the same kernels on the same arms, and the difference of two periods, divided by the
number of checks, is what one check kernel costs over the other:

 (a) goto_js over goto      check_kernel<T, 1, 0> reads two q-sized rows per arm (the reference and the integrated angles: 2 x 28 B) where
                            check_kernel<T, 0, 0> reads the distance pair and the goal block's `present` flag (12 B);
 (b) follow_js over goto_js check_kernel<T, 1, 1> reads next and the list length where check_kernel<T, 1, 0> reads arrived (8 against 4 B per arm)
                            and, per posture reached, copies a row (2 x 28 B) and writes reached / next (8 B).  The goto_js heads for
                            posture 0 of the W = 4 postures per arm.

Two scenes, since a check kernel's waves add into pending[k] only where they find an arm under way (profiles/follow_cost.txt):

 far    postures at q0 +- 0.5 rad on every joint, jp_kp 0.5: after 200 cycles 0.18 rad are left, so NO arm arrives in any of the three calls
        (under joint control the tool does not head for the Cartesian goal either) and every wave of every check adds: like against like;
 near   postures at q0 + 0.04 w U(-1, 1), w = 1..4, jp_kp 8: every arm is at posture 0 after a few checks, so goto_js' waves stop adding
        while goto's (nobody at the Cartesian goal) and follow_js' (arms under way until their LAST posture) go on.

Series alternate: --series of each, every one a median of --reps HIP-event periods after 2 untimed runs.  Reported: the medians, the
spread of goto's own medians over its series, the differences per check and the extra bytes at the 4.81 TB/s
profiles/move_fields_cost.txt reached.  The expectation is that each difference lies inside goto's own spread plus the time of the
extra bytes; the figure is reported with that spread next to it whichever way it falls, and anything beyond is listed as a finding.

 (e) with --parent-root DIR (a built checkout of the parent commit): bench.py --gpus 1 --steps 200 --warmup 20 on the parent and on this
     build, alternating, each in a process of its own: both medians and the parent's spread.

Into profiles/goto_js_cost.txt (--out)."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(HERE, "profiles", "goto_js_cost.txt"))
ap.add_argument("--parent-root", default=None, help="a built checkout of the parent commit: part (e)")
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--series", type=int, default=3)
ap.add_argument("--bench-reps", type=int, default=4)
args = ap.parse_args()
sys.path.insert(0, HERE)
import torch  # noqa: E402

from vfclik_amd import _abi, engine, robots, synth  # noqa: E402

chain = robots.lwr()
L = []


def say(s=""):
    print(s, flush=True)
    L.append(s)


B, NOBS, K, W, R, N = 65536, 8, 200, 4, args.reps, 7
DT, PREC = 0.01, (0.01, 0.05)
PREC_JS = 0.004 + 0.002 * np.arange(N)
STRIDES = (4, 10, 50)
RATE = 4.81e6   # bytes per microsecond
say("goto_js_cost -- tools/goto_js_cost.py; device: %s; ABI %d" % (torch.cuda.get_device_name(0), _abi.ABI_VERSION))
say("times in microseconds for the WHOLE sequence of %d control cycles unless a line says otherwise; HIP events around the sequence on one" % K)
say("stream; %d series of goto, goto_js and follow_js, alternating, each a median of %d periods after 2 untimed runs" % (args.series, R))
say("batch: %d arms, 7 joints, float32 I/O, goal + %d obstacles (C3), joint control (mixer [0 0 1 0 0 0], F_MIXER), W = %d," % (B, NOBS, W))
say("clamp on, dt %.2f, goto precision (%.2f m, %.2f rad), joint precision 0.004 + 0.002 i rad (via: 3 x), hold off, io->active all ones," % (DT, PREC[0], PREC[1]))
say("io->goal_dist and qdot_out named in every call, no trace, no diff, pending given")
say()

stream = torch.cuda.current_stream().cuda_stream
w = synth.make_workload(chain, B, NOBS, seed=1, io_dtype=np.float32)
params = _abi.default_params(flags=_abi.F_MIXER, mix_w=[0, 0, 1, 0, 0, 0], max_vel=0.7)
eng = engine.Engine(chain, B, io_dtype=np.float32, max_slots=8, params=params)
eng.set_fields(w["fields"], w["nfields"])
eng.use_stream(stream)
dev = torch.device("cuda", 0)
rng = np.random.default_rng(3)
near = w["q"][:, None, :] + 0.04 * np.arange(1, W + 1)[None, :, None] * rng.uniform(-1.0, 1.0, size=(B, W, N))
far = w["q"][:, None, :] + 0.5 * rng.choice([-1.0, 1.0], size=(B, W, N))
q0 = torch.from_numpy(w["q"].astype(np.float32)).to(dev)
qdot = torch.zeros(B, N, device=dev)
gdist = torch.zeros(B, 2, device=dev)
ones = torch.ones(B, dtype=torch.int32, device=dev)
arrived = torch.zeros(B, dtype=torch.int32, device=dev)
arrived_js = torch.zeros(B, dtype=torch.int32, device=dev)
reached = torch.zeros(B, W, dtype=torch.int32, device=dev)
nxt = torch.zeros(B, dtype=torch.int32, device=dev)
pending = torch.zeros(K, dtype=torch.int32, device=dev)
io_own = eng.make_io(q0, qdot_out=qdot, goal_dist=gdist, active=ones)


def median_period(fn):
    per = []
    for r in range(R + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if r >= 2:
            per.append(e0.elapsed_time(e1) * 1e3)
    return float(np.median(per))


findings = []
for scene, kp, way in (("far", 0.5, far), ("near", 8.0, near)):
    eng.set_params(jp_kp=kp)
    wayq = torch.from_numpy(way.astype(np.float32)).to(dev)
    q_ref = wayq[:, 0].contiguous()
    io_ref = eng.make_io(q0, q_ref=q_ref, qdot_out=qdot, goal_dist=gdist, active=ones)
    say("scene %s (jp_kp %g)" % (scene, kp))
    for s in STRIDES:
        n = K // s
        kw = dict(stride=s, hold=False, clamp=True, pending=pending[:n])

        def goto():
            eng.goto(io_ref, K, DT, PREC, arrived=arrived, **kw)

        def goto_js():
            eng.goto_js(io_ref, K, DT, PREC_JS, arrived=arrived_js, **kw)

        def follow_js():
            eng.follow_js(io_own, wayq, K, DT, PREC_JS, via_precision=3 * PREC_JS, reached=reached, next=nxt, **kw)
        g, j, f = [], [], []
        for _ in range(args.series):
            g.append(median_period(goto))
            j.append(median_period(goto_js))
            f.append(median_period(follow_js))
        torch.cuda.synchronize()
        hits, there_js, there = int((reached >= 0).sum()), int((arrived_js >= 0).sum()), int((arrived >= 0).sum())
        gm, jm, fm, spread = float(np.median(g)), float(np.median(j)), float(np.median(f)), max(g) - min(g)
        say("s = %2d: goto      medians %s  -> %9.2f, spread of its medians %.2f (arms it found at the Cartesian goal: %d)" % (s, " ".join("%9.2f" % x for x in g), gm, spread, there))
        say("        goto_js   medians %s  -> %9.2f (arms at posture 0: %d)" % (" ".join("%9.2f" % x for x in j), jm, there_js))
        say("        follow_js medians %s  -> %9.2f (postures reached: %d)" % (" ".join("%9.2f" % x for x in f), fm, hits))
        for label, diff, extra in (("(a) goto_js over goto", jm - gm, (2 * 4 * N - 12) * B * n),
                                   ("(b) follow_js over goto_js", fm - jm, 4 * B * n + (2 * 4 * N + 8) * hits)):
            bytes_us = extra / RATE
            beyond = diff - spread - bytes_us
            say("        %-27s %+9.2f us = %+.3f us per check (%d checks); extra bytes %.2f MB = %.2f us at 4.81 TB/s; goto's spread %.2f; beyond both: %s"
                % (label, diff, diff / n, n, extra / 1e6, bytes_us, spread, "nothing" if beyond <= 0 else "%.2f us = %.3f us per check" % (beyond, beyond / n)))
            if beyond > 0:
                findings.append("scene %s, s = %d, %s: %.3f us per check beyond goto's spread and the extra bytes" % (scene, s, label, beyond / n))
    say()
say("FINDINGS" if findings else "FINDINGS: none -- every difference lies inside goto's own spread plus the time of the extra bytes")
for x in findings:
    say("    " + x)
if findings:
    say("    Scene far compares like with like (every wave of every check adds into pending[k]); in scene near the calls differ in who is")
    say("    still under way, and a difference there goes with the waves that add, as in profiles/follow_cost.txt's scene near: goto_js' arms")
    say("    are all at posture 0 after a few checks, goto's and follow_js' stay under way.  What else an excess is made of is not measured here.")
say()
eng.close()

say("(e) bench.py --gpus 1 --steps 200 --warmup 20, parent and this build alternating, a process each: us per step")
if args.parent_root is None:
    say("    not measured (no --parent-root)")
else:
    vals = {"parent": [], "this build": []}
    runs = [(label, root) for r in range(args.bench_reps) for label, root in (("parent", args.parent_root), ("this build", HERE))]
    for label, root in runs:
        p = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "200", "--warmup", "20"], cwd=root, stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, text=True, timeout=600)
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
        if p.returncode != 0 or not line:
            say("    %s: FAILED (exit %d); nothing further is started" % (label, p.returncode))
            break
        vals[label].append(json.loads(line[-1])["ms_per_step"] * 1e3)
    for label, v in vals.items():
        if v:
            say("    %-10s median %.3f  min %.3f  max %.3f   runs: %s" % (label, np.median(v), min(v), max(v), " ".join("%.3f" % x for x in v)))
    if vals["parent"] and vals["this build"]:
        pm, spread, tm = float(np.median(vals["parent"])), max(vals["parent"]) - min(vals["parent"]), float(np.median(vals["this build"]))
        say("    this build's median %.3f against the parent's %.3f; the parent's own spread %.3f : %s" % (tm, pm, spread, "inside" if tm <= pm + spread else "ABOVE"))

os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(L) + "\n")
