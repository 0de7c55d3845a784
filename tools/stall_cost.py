#!/usr/bin/env python
"""What the stall rule of the timed moves costs and what it buys (vfik_set_stall_rule), measured on one box in one session:

 (a) rule off, against the parent: vfik_goto on C3's batch (65 536 arms, 7 joints, goal + 8 obstacles, float32 I/O), 200 control cycles,
     strides 4 / 10 / 50, hold on, no trace -- this build against a checkout of the parent commit with its library built
     (--parent-root DIR; tools/build_rev.sh builds the library).  tools/isa_diff.py says the device code is the same, so the difference is
     expected inside the parent's own spread.
 (b) rule on, where nobody stalls (patience above the number of checks), against rule off in the same session: the excess per check over
     the bytes of the rule's state -- 44 B per arm and check (best 16 in and out, count 4 in and out, stalled 4 in) at the 4.81 TB/s
     profiles/move_fields_cost.txt records -- plus the spread of the rule-off series.
 (c) the benefit: tests/test_gpu_stall.py's goto scene (every eighth arm's goal three times as far from the base) at 65 536 arms, float64
     I/O, Engine.goto_host with a time-out of 4000 cycles, stride 4, poll 8: wall clock and checks_run without and with the rule.
 (d) with --parent-root: bench.py --gpus 1 --steps 200 --warmup 20 on the parent and on this build, alternating, a process each.

(a) and (b): THREE alternating series (parent, this build rule off, this build rule on), each figure the median of 9 HIP-event periods
after 2 untimed ones, every series a process of its own; nothing else of ours runs on the GPU meanwhile.  No bar is fixed in advance: the
figures are stated, and a miss of the expectation is stated plainly.  Into profiles/stall_cost.txt (--out).  The first process of ours
that fails (a series, part (c), a bench.py run: any exit status but 0, or no result line) ends the tool: nothing further is started on
the GPU, what was collected so far is written, exit status 1."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(HERE, "profiles", "stall_cost.txt"))
ap.add_argument("--parent-root", default=None, help="a checkout of the parent commit with its library built: parts (a) and (d)")
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--series", type=int, default=3)
ap.add_argument("--bench-reps", type=int, default=3)
ap.add_argument("--worker", default=None, help="internal: the package root to measure, one series, JSON on stdout")
ap.add_argument("--rule", type=int, default=0, help="internal: the worker sets a rule under which nobody stalls")
args = ap.parse_args()

B, NOBS, K, DT, PREC, STRIDES = 65536, 8, 200, 0.01, (0.01, 0.05), (4, 10, 50)

if args.worker:   # ---- one series: the median period of vfik_goto at every stride, in microseconds
    sys.path.insert(0, args.worker)
    import torch
    from vfclik_amd import _abi, engine, robots, synth
    chain = robots.lwr()
    w = synth.make_workload(chain, B, NOBS, seed=1, io_dtype=np.float32)
    eng = engine.Engine(chain, B, io_dtype=np.float32, max_slots=8, params=_abi.default_params(max_vel=0.7))
    eng.set_fields(w["fields"], w["nfields"])
    eng.use_stream(torch.cuda.current_stream().cuda_stream)
    if args.rule:
        eng.set_stall_rule(K + 1, eps=(1e-3, 1e-2), stop=True)
    dev = torch.device("cuda", 0)
    q0 = torch.from_numpy(w["q"].astype(np.float32)).to(dev)
    io = eng.make_io(q0, qdot_out=torch.zeros(B, 7, device=dev))
    arrived = torch.zeros(B, dtype=torch.int32, device=dev)
    pending = torch.zeros(K, dtype=torch.int32, device=dev)
    out = {}
    for s in STRIDES:
        per = []
        for r in range(args.reps + 2):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            eng.goto(io, K, DT, PREC, stride=s, hold=True, clamp=True, arrived=arrived, pending=pending[:K // s])
            e1.record()
            torch.cuda.synchronize()
            if r >= 2:
                per.append(e0.elapsed_time(e1) * 1e3)
        out[str(s)] = [float(np.median(per)), float(min(per)), float(max(per))]
    eng.close()
    print("RESULT " + json.dumps(out))
    sys.exit(0)

sys.path.insert(0, HERE)
import torch  # noqa: E402

from vfclik_amd import _abi, engine, robots, synth  # noqa: E402

L = []


def say(s=""):
    print(s, flush=True)
    L.append(s)


def finish(code):
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(L) + "\n")
    sys.exit(code)


def stop(what, code):
    """A process of ours failed on the GPU -- whatever the cause, nothing further is started there: what was collected is written, exit 1."""
    say("    %s FAILED (exit %s); nothing further is started on the GPU" % (what, code))
    finish(1)


def series(root, rule):
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", root, "--rule", str(rule), "--reps", str(args.reps)],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
    if p.returncode != 0 or not line:
        say("    " + " | ".join(p.stderr.strip().splitlines()[-2:]))
        stop("a series (%s, rule %s)" % (root, "on" if rule else "off"), p.returncode)
    return json.loads(line[-1][7:])


say("stall_cost -- tools/stall_cost.py; device: %s; ABI %d" % (torch.cuda.get_device_name(0), _abi.ABI_VERSION))
say("(a), (b): vfik_goto, %d arms, 7 joints, float32 I/O, goal + %d obstacles (C3), %d cycles, hold on, no trace; microseconds for the whole" % (B, NOBS, K))
say("sequence; %d alternating series, each the median of %d HIP-event periods (min .. max beside it) in a process of its own" % (args.series, args.reps))
say()
kinds = ([("parent", args.parent_root, 0)] if args.parent_root else []) + [("rule off", HERE, 0), ("rule on", HERE, 1)]
res = {k: [] for k, _, _ in kinds}
for i in range(args.series):
    for k, root, rule in kinds:
        r = series(root, rule)   # (a failed series ends the tool)
        res[k].append(r)
        say("    series %d  %-8s  %s" % (i + 1, k, "   ".join("s = %2s: %9.2f (%9.2f .. %9.2f)" % (s, *r[str(s)]) for s in STRIDES)))
say()


def med(k, s):
    return float(np.median([r[str(s)][0] for r in res[k]]))


def spread(k, s):
    v = [r[str(s)][0] for r in res[k]]
    return max(v) - min(v)


say("(a) rule off against the parent: median over the series' medians, the parent's own spread over its series")
if args.parent_root and res["parent"] and res["rule off"]:
    for s in STRIDES:
        d, sp = med("rule off", s) - med("parent", s), spread("parent", s)
        say("    s = %2d: parent %9.2f  this build %9.2f  difference %+7.2f us (%+.2f %%), parent's spread %.2f us : %s"
            % (s, med("parent", s), med("rule off", s), d, 100 * d / med("parent", s), sp, "inside" if abs(d) <= sp else "OUTSIDE the parent's spread"))
else:
    say("    not measured (no --parent-root)")
say()
say("(b) rule on (nobody stalls) against rule off: excess per check, against 44 B per arm at 4.81 TB/s = %.2f us plus the rule-off spread per check" % (B * 44 / 4.81e6))
if res["rule on"] and res["rule off"]:
    for s in STRIDES:
        n = K // s
        ex, bound = (med("rule on", s) - med("rule off", s)) / n, B * 44 / 4.81e6 + spread("rule off", s) / n
        say("    s = %2d: rule off %9.2f  rule on %9.2f  excess per check (%d checks) %+6.2f us, bytes + spread %.2f us : %s"
            % (s, med("rule off", s), med("rule on", s), n, ex, bound, "within" if ex <= bound else "MISSED"))
say()

# ---- (c) ------------------------------------------------------------------------------------------------------------------------------
say("(c) the benefit: Engine.goto_host, %d lwr arms, float64 I/O, nullspace + joint-limit task, every eighth arm's goal out of reach, time-out 4000" % B)
say("    cycles, stride 4, hold on, poll 8; wall clock of the call in MILLISECONDS (host arrays in and out), rule: patience 5, eps (1e-3, 1e-2), stop")
chain = robots.lwr()
w = synth.make_workload(chain, B, 3, seed=53, io_dtype=np.float64)
rng = np.random.default_rng(7)
qg = rng.uniform(0.7 * chain.q_lo, 0.7 * chain.q_hi, size=(B, 7))
q0 = qg + rng.uniform(0.02, 0.25, size=(B, 1)) * rng.uniform(-1.0, 1.0, size=(B, 7))
goal = chain.fk(qg).reshape(B, 16)
goal[3::8, 3::4] *= [3.0, 3.0, 3.0, 1.0]
w["fields"]["p"][:, 0, :16] = goal
eng = engine.Engine(chain, B, io_dtype=np.float64, max_slots=8, params=_abi.default_params(flags=5, max_vel=0.7))
eng.set_fields(w["fields"], w["nfields"])
for rule in (False, True):
    ts = []
    try:
        eng.set_stall_rule(5 if rule else None, eps=(1e-3, 1e-2), stop=True)
        for r in range(4):
            eng.reset_state()
            t0 = time.perf_counter()
            got = eng.goto_host(q0, 4000, DT, PREC, stride=4, hold=True, clamp=True, poll=8)
            ts.append((time.perf_counter() - t0) * 1e3)
    except engine.VfikError as e:
        stop("part (c), %s the rule: %s" % ("with" if rule else "without", e), "a library error")
    say("    %-12s wall %8.1f ms (median of 3 after 1; %.1f .. %.1f), checks_run %4d of 1000, arrived %d, stalled %d, still under way %d"
        % ("with the rule" if rule else "without", float(np.median(ts[1:])), min(ts[1:]), max(ts[1:]), got["checks_run"],
           int((got["arrived"] >= 0).sum()), int((got["stalled"] >= 0).sum()) if rule else 0, int(got["pending"][-1])))
eng.close()
say()

# ---- (d) ------------------------------------------------------------------------------------------------------------------------------
say("(d) bench.py --gpus 1 --steps 200 --warmup 20, parent and this build alternating, a process each: microseconds per step")
if args.parent_root is None:
    say("    not measured (no --parent-root)")
else:
    vals = {"parent": [], "this build": []}
    for label, root in [lr for r in range(args.bench_reps) for lr in (("parent", args.parent_root), ("this build", HERE))]:
        p = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "200", "--warmup", "20"], cwd=root, stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, text=True, timeout=600)
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
        if p.returncode != 0 or not line:
            stop("bench.py of %s" % label, p.returncode)
        vals[label].append(json.loads(line[-1])["ms_per_step"] * 1e3)
    for label, v in vals.items():
        if v:
            say("    %-10s median %.3f  runs: %s" % (label, float(np.median(v)), " ".join("%.3f" % x for x in v)))
    if vals["parent"] and vals["this build"]:
        pm, sp, tm = float(np.median(vals["parent"])), max(vals["parent"]) - min(vals["parent"]), float(np.median(vals["this build"]))
        say("    this build's median %.3f against the parent's %.3f, the parent's own spread %.3f : %s"
            % (tm, pm, sp, "inside" if tm <= pm + sp else "ABOVE the parent's spread"))

finish(0)
