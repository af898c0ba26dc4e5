"""A/B: the learn alone at C3 size (1024 envs x 16 agents = 16,384 agents, rings
full, fp16) with launch-scalar hyperparameters against the same learn with
per-agent arrays that hold the same values (AgentConfig.sweep with one-value
lists: dmdqn_learn_hp, the HP kernel instantiations).  The two agents hold the
same nets and replay; the runs alternate, each timed with device events around
N launches after a warm-up.  Prints one JSON line: per-launch ms of every
round, each arm's mean and the scalar arm's own spread -- a difference within
that spread is no difference.  Two agents differ in their memory as well as
their kernels, and where two working sets of this size land can matter more
than the kernels: --arrays-first swaps the build order as a
control, and --one-agent times both kernels on one agent's memory.
usage: python tools/hparams_ab.py [--launches N] [--rounds R] [--envs E] [--agents A]
       [--precision fp16|bf16|fp32] [--tau T] [--arrays-first] [--one-agent] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dmdqn_amd.agent import AgentConfig, BatchedDQN  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--launches", type=int, default=200)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--envs", type=int, default=1024)
ap.add_argument("--agents", type=int, default=16)
ap.add_argument("--precision", default="fp16")
ap.add_argument("--tau", type=float, default=0.0, help="> 0: soft learns (the tau arrays too)")
ap.add_argument("--arrays-first", action="store_true",
                help="build and time the arrays arm before the scalar one (a control: a "
                     "difference that follows the order belongs to the allocations, not the kernels)")
ap.add_argument("--one-agent", action="store_true",
                help="one agent with uniform arrays serves both arms (the scalar arm launches "
                     "without its arrays, which hold the config's values): the same memory "
                     "under both kernels, so what remains is the kernels' difference")
ap.add_argument("--out", default=None)
args = ap.parse_args()
E, A, CAP = args.envs, args.agents, 1000

base = dict(learning_rate=0.001, gamma=0.99, tau=args.tau)
sweep = {k: [v] for k, v in base.items() if k != "tau" or v > 0}


def build(sw):
    ag = BatchedDQN(E, A, AgentConfig(precision=args.precision, seed=0, replay_buffer_size=CAP,
                                      sweep=sw, **base))
    g = torch.Generator(device="cuda").manual_seed(0)
    for t in range(CAP + 40):  # full rings, wrapped
        s = torch.randint(-1, 24, (E, A, 89), device="cuda", generator=g).float()
        a = torch.randint(0, 4, (E, A), device="cuda", generator=g, dtype=torch.int32)
        r = -torch.rand((E, A), device="cuda", generator=g, dtype=torch.float64) * 100
        ag.remember(s, a, r, s, t % 60 == 59)
    return ag


order = ("arrays", "scalar") if args.arrays_first else ("scalar", "arrays")
HP = ("hp_lr", "hp_gamma", "hp_tau", "hp_omt")
if args.one_agent:
    one = build(sweep)
    arms = {k: one for k in order}
    held = {n: getattr(one, n) for n in HP}
else:
    arms = {k: build(sweep if k == "arrays" else None) for k in order}
    assert arms["arrays"].swept and not arms["scalar"].swept


def select(name):
    """--one-agent: launch with the arrays (arrays arm) or without (scalar arm)."""
    if args.one_agent:
        for n in HP:
            setattr(one, n, held[n] if name == "arrays" else None)
        assert one.swept == (name == "arrays")


for name, ag in arms.items():
    select(name)
    for _ in range(10):
        ag.learn()
torch.cuda.synchronize()
# the same bits so far (the contract the tests pin at small shapes)
same = all(torch.equal(getattr(arms["scalar"], n), getattr(arms["arrays"], n))
           for n in ("params", "adam_m", "adam_v", "target"))
ms = {k: [] for k in arms}
for _ in range(args.rounds):
    for name, ag in arms.items():
        select(name)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.launches):
            ag.learn()
        e1.record()
        torch.cuda.synchronize()
        ms[name].append(e0.elapsed_time(e1) / args.launches)
res = {"agents": E * A, "precision": args.precision, "tau": args.tau, "launches": args.launches,
       "order": list(order), "one_agent": args.one_agent,
       "same_bits_after_warmup": None if args.one_agent else bool(same),  # (one agent: one net)
       "ms_per_learn": {k: [round(x, 5) for x in v] for k, v in ms.items()},
       "mean_ms": {k: round(float(np.mean(v)), 5) for k, v in ms.items()},
       "scalar_spread_ms": round(float(max(ms["scalar"]) - min(ms["scalar"])), 5),
       "arrays_minus_scalar_ms": round(float(np.mean(ms["arrays"]) - np.mean(ms["scalar"])), 5)}
line = json.dumps(res)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
