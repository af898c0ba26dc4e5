"""Measurement: the rule-based controllers (dmdqn_act_rule) at C3 size -- a 4x4
grid x 1024 replicas, NA = 16,384 agents -- in one process, what
AgentConfig.behavior costs a training run end to end, and the per-mode
evaluation table on the shipped grid_3x3 scenario.

Kernel (profiles/rule/rule.json): on the observations of a warmed-up C3
Trainer, `--rounds` rounds of, each between two device events: `--reps`
launches of act_rule for each rule (with and without the score output) and of
the greedy forward q_argmax it stands in for.  Medians over the rounds.

End to end (profiles/rule/e2e.json): two C3 Trainers (overlap "env"), behavior
None and behavior "max_pressure" for the whole run (behavior_steps 0), timed in
alternating windows of `--steps` steps (host clock around a device sync),
`--rounds` rounds.  The run with the policy launches act_rule once per step on
the side stream and its act draws randint for a tenth of the agents only.

Evaluation (profiles/rule/eval.json): evaluate.summarize over `--episodes`
episodes per mode of random, fixed, program, longest_queue and max_pressure on
config/scenarios/grid_3x3_p06.npz.  A recorded result, not a claim: the
simulator has no yellow between agent-chosen greens.

  python tools/rule_bench.py [--rounds 3] [--steps 1000] [--outdir profiles/rule]

Prints one JSON line per part.  Needs a GPU."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from dmdqn_amd import _lib, evaluate as EV, kernels as K  # noqa: E402
from dmdqn_amd.agent import AgentConfig, PRECISIONS  # noqa: E402
from dmdqn_amd.env import EnvConfig  # noqa: E402
from dmdqn_amd.trainer import Trainer  # noqa: E402

SCENARIO = os.path.join(ROOT, "config", "scenarios", "grid_3x3_p06.npz")
EVAL_MODES = ("random", "fixed", "program", "longest_queue", "max_pressure")


def window(fn, reps, stream):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    for _ in range(reps):
        fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b) / reps  # ms per launch


def make_trainer(args, behavior):
    return Trainer(EnvConfig(rows=args.rows, cols=args.cols, num_envs=args.envs, seed=1000),
                   AgentConfig(precision=args.precision, seed=1000, behavior=behavior,
                               behavior_steps=0, behavior_eps=args.eps),
                   overlap="env")


def kernel_part(args, tr, dev):
    ag = tr.agent
    tr.synchronize()
    stream = torch.cuda.current_stream(dev)
    obs = tr.obs.clone()
    out = torch.empty((ag.E, ag.A), dtype=torch.int32, device=dev)
    score = torch.empty((ag.E, ag.A, 4), dtype=torch.int32, device=dev)
    flat = obs.reshape(ag.NA, 89)
    fns = {
        "longest_queue": lambda: K.act_rule(obs, args.rows, args.cols, 0, out=out),
        "max_pressure": lambda: K.act_rule(obs, args.rows, args.cols, 1, out=out),
        "max_pressure_score": lambda: K.act_rule(obs, args.rows, args.cols, 1, out=out,
                                                 score=score),
        "q_argmax": lambda: ag._ops.q_argmax(ag.params, ag.H, PRECISIONS[args.precision], flat,
                                             out, None, False),
    }
    for fn in fns.values():  # warm-up
        window(fn, 3, stream)
    ms = {k: [] for k in fns}
    for _ in range(args.rounds):
        for k, fn in fns.items():
            ms[k].append(window(fn, args.reps, stream))
    med = {k: statistics.median(v) for k, v in ms.items()}
    read = ag.NA * 89 * 4
    return {"what": "dmdqn_act_rule on a warmed-up C3 Trainer's observations beside the greedy "
                    "forward (dmdqn_q_argmax) it stands in for, back-to-back launches on one "
                    "stream, medians over the rounds",
            "device": torch.cuda.get_device_name(dev), "lib_digest": _lib.LIB_DIGEST,
            "NA": ag.NA, "precision": args.precision, "rounds": args.rounds,
            "reps_per_window": args.reps,
            "ms_rounds": {k: [round(x, 5) for x in v] for k, v in ms.items()},
            "ms_median": {k: round(x, 5) for k, x in med.items()},
            "obs_bytes": read,
            "max_pressure_GBps": round(read / (med["max_pressure"] * 1e-3) / 1e9, 1),
            "rule_over_q_argmax": round(med["max_pressure"] / med["q_argmax"], 4)}


def e2e_part(args, trainers, dev):
    rates = {k: [] for k in trainers}
    for _ in range(args.rounds):
        for name, tr in trainers.items():
            tr.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                tr.step()
            tr.synchronize()
            el = time.perf_counter() - t0
            rates[name].append(args.steps * tr.agent.NA / el)
    med = {k: statistics.median(v) for k, v in rates.items()}
    off = rates["off"]
    on = trainers["on"].agent
    torch.cuda.synchronize(dev)
    return {"what": "C3 Trainer (overlap env) with behavior None and behavior max_pressure for "
                    "the whole run, alternating windows in one process, agent-env steps/s",
            "device": torch.cuda.get_device_name(dev), "lib_digest": _lib.LIB_DIGEST,
            "NA": on.NA, "precision": args.precision, "steps_per_window": args.steps,
            "rounds": args.rounds, "behavior_eps": args.eps,
            "learn_steps": {k: int(t.agent.learn_step_counter) for k, t in trainers.items()},
            "pair_launches": {k: int(t.agent.pair_launches) for k, t in trainers.items()},
            "steps_per_s": {k: [round(x, 1) for x in v] for k, v in rates.items()},
            "median": {k: round(v, 1) for k, v in med.items()},
            "on_over_off": round(med["on"] / med["off"], 4),
            "off_spread": round((max(off) - min(off)) / med["off"], 4)}


def eval_part(args, dev):
    rows = EV.evaluate(EnvConfig(scenario=SCENARIO), EVAL_MODES, episodes=args.episodes)
    table = EV.summarize(rows)
    return {"what": f"evaluate.summarize, {args.episodes} episodes per mode (seeds from 10000) on "
                    "config/scenarios/grid_3x3_p06.npz, fixed signal durations; the reward is the "
                    "training path's (sum over steps and agents)",
            "device": torch.cuda.get_device_name(dev), "lib_digest": _lib.LIB_DIGEST,
            "summary": {m: {k: round(float(v), 4) for k, v in table.loc[m].items()}
                        for m in table.index}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--rows", type=int, default=4)
    ap.add_argument("--cols", type=int, default=4)
    ap.add_argument("--precision", default="fp16", choices=["fp16", "bf16"])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=50, help="launches per kernel window")
    ap.add_argument("--steps", type=int, default=1000, help="trainer steps per end-to-end window")
    ap.add_argument("--eps", type=float, default=0.1,
                    help="behavior_eps of the run with the policy")
    ap.add_argument("--warmup", type=int, default=140, help="steps before timing (learns from 128)")
    ap.add_argument("--episodes", type=int, default=10, help="evaluation episodes per mode")
    ap.add_argument("--outdir", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rule_bench needs a GPU: a CPU run measures nothing")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    trainers = {"off": make_trainer(args, None), "on": make_trainer(args, "max_pressure")}
    for tr in trainers.values():
        for _ in range(args.warmup + args.steps):
            tr.step()
        tr.synchronize()
        assert tr.agent.learn_step_counter > 0
    parts = {"rule": kernel_part(args, trainers["on"], dev)}
    parts["e2e"] = e2e_part(args, trainers, dev)
    del trainers
    parts["eval"] = eval_part(args, dev)
    for name, res in parts.items():
        print(json.dumps(res), flush=True)
        if args.outdir:
            os.makedirs(args.outdir, exist_ok=True)
            with open(os.path.join(args.outdir, f"{name}.json"), "w") as f:
                f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
