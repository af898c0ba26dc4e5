"""A/B: Trainer steps at C3 size (4x4 grid x 1024 envs = 16,384 agents, fp16,
one stream, fused env step) with n_step 1 and with n_step 3 (the staging ring
and one k_replay_nstep_commit launch per step on top of the same env step and
learn).  Both trainers live in one process; after a warm-up that takes each
past its first learns, rounds of N steps alternate between them, each timed
with a host clock around work that ends in a device synchronise.  Prints one
JSON line: ms per step of every round, each arm's mean, the one-step arm's own
spread (a difference within it is no difference), the ratio, the commit launch
timed alone (device events around N launches), and the box's HBM copy rate
from bench.py's streaming probe.  This describes a cost; it gates nothing.
usage: python tools/ab_nstep.py [--steps N] [--rounds R] [--envs E] [--grid RxC]
       [--n_step K] [--warmup W] [--precision fp16|bf16|fp32] [--other-first]
       [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dmdqn_amd.agent import AgentConfig  # noqa: E402
from dmdqn_amd.env import EnvConfig  # noqa: E402
from dmdqn_amd.trainer import Trainer  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--envs", type=int, default=1024)
ap.add_argument("--grid", default="4x4")
ap.add_argument("--n_step", type=int, default=3)
ap.add_argument("--warmup", type=int, default=160, help="steps before the first round (> 130)")
ap.add_argument("--precision", default="fp16")
ap.add_argument("--other-first", action="store_true",
                help="build and time the n-step arm before the one-step arm (a control)")
ap.add_argument("--out", default=None)
args = ap.parse_args()
rows, cols = (int(x) for x in args.grid.split("x"))


def build(n_step):
    return Trainer(EnvConfig(rows=rows, cols=cols, num_envs=args.envs, seed=0),
                   AgentConfig(precision=args.precision, seed=0, n_step=n_step), overlap="none")


other = f"n{args.n_step}"
# two trainers differ in their memory as well as their launches, and where two
# working sets of this size land shows in the step time (DESIGN section 6,
# "Measured: the sweep path"): --other-first swaps the build order as a control
arms = ({other: build(args.n_step), "n1": build(1)} if args.other_first
        else {"n1": build(1), other: build(args.n_step)})
for tr in arms.values():
    for _ in range(args.warmup):
        tr.step()
    tr.synchronize()
    assert tr.agent.learn_launches > 0, "warm up past the first learn"
ms = {k: [] for k in arms}
for _ in range(args.rounds):
    for name, tr in arms.items():
        tr.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            tr.step()
        tr.synchronize()
        ms[name].append((time.perf_counter() - t0) * 1e3 / args.steps)
# the commit launch alone: the same window committed again and again into the
# slot the next commit writes (no advance), device events around N launches
ag = arms[other].agent
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
total = ag.ring.total
for i in range(args.steps + 10):
    if i == 10:
        e0.record()
    ag.ring.commit_nstep(ag.stage, ag.stage.next_slot, ag.cfg.gamma, ag.nstep_gamma_a)
    ag.ring.total = total
e1.record()
torch.cuda.synchronize()
commit_us = e0.elapsed_time(e1) * 1e3 / args.steps
res = {"agents": args.envs * rows * cols, "precision": args.precision, "steps": args.steps,
       "rounds": args.rounds, "n_step": args.n_step, "order": list(arms),
       "commit_us_per_launch": round(commit_us, 3),
       "ms_per_step": {k: [round(x, 5) for x in v] for k, v in ms.items()},
       "mean_ms": {k: round(float(np.mean(v)), 5) for k, v in ms.items()},
       "n1_spread_ms": round(float(max(ms["n1"]) - min(ms["n1"])), 5),
       "ratio": round(float(np.mean(ms[other]) / np.mean(ms["n1"])), 5)}
try:  # the box's copy rate (bench.py's probe), after the timed rounds
    import bench
    dev = arms["n1"].env.device
    nb = bench.stream_probe_bytes(dev)
    res["copy_gbs"] = bench.stream_probe(torch.cuda.current_stream(dev), nb)["copy_gbs"] if nb else None
except torch.cuda.OutOfMemoryError as e:
    res["copy_gbs"] = None
    res["copy_skipped"] = str(e).splitlines()[0][:120]
line = json.dumps(res)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
