"""Measurement: the network health probe (dmdqn_net_probe, dmdqn_layer_norms)
at C3 size -- a 4x4 grid x 1024 replicas, NA = 16,384 fp16 agents -- in one
process, and what AgentConfig.health_every costs a training run end to end.

Kernels (profiles/health/probe.json): after a warm-up that fills the rings and
starts the learns, `--rounds` rounds of, each between two device events: the
probe, dmdqn_layer_norms in both modes, the learn alone (bench.py's learn-alone
probe: learn_begin + learn_range bracketed by events) and dmdqn_stream_probe's
float4 copy.  Medians over the rounds.  The probe's algorithmic bytes are
131,088 per agent (28,548 f32 parameters, 128 rows of 128 B and 128 indices of
4 B read; 92 B written), a learn's 891,632 (bench.learn_bytes_per_agent).

End to end (profiles/health/e2e.json): two C3 Trainers in the process, one with
health_every 0 and one with `--every` (100), timed in alternating windows of
`--steps` steps (host clock around a device sync), `--rounds` rounds.

  python tools/health_bench.py [--rounds 3] [--steps 200] [--every 100] [--outdir profiles/health]

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

from bench import learn_bytes_per_agent  # noqa: E402
from dmdqn_amd import _lib, kernels as K  # noqa: E402
from dmdqn_amd.agent import AgentConfig, PRECISIONS  # noqa: E402
from dmdqn_amd.env import EnvConfig  # noqa: E402
from dmdqn_amd.trainer import Trainer  # noqa: E402

PROBE_READ_BYTES_PER_AGENT = 28548 * 4 + 128 * 128 + 128 * 4  # 131,088


def window(fn, reps, stream):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    for _ in range(reps):
        fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b) / reps  # ms per launch


def make_trainer(args, health_every):
    return Trainer(EnvConfig(rows=args.rows, cols=args.cols, num_envs=args.envs, seed=1000),
                   AgentConfig(precision=args.precision, seed=1000, health_every=health_every),
                   overlap="env")


def kernel_part(args, tr, dev):
    ag = tr.agent
    NA, P = ag.NA, ag.P
    stream = torch.cuda.current_stream(dev)
    tr.synchronize()
    tok = ag._last_tok
    counts, stats, mask = K.net_probe(ag.ring.s, tok.idx, ag.params, tok.start, ag.H,
                                      PRECISIONS[args.precision])
    out = torch.empty((NA, K.NORM_VARS), dtype=torch.float64, device=dev)
    eps = tok.adam[3]
    n_copy = min(1 << 30, torch.cuda.mem_get_info(dev)[0] // 4) // 16 * 16
    src = torch.empty(n_copy, dtype=torch.uint8, device=dev).random_(0, 256)
    dst = torch.empty_like(src)

    def probe():
        K.net_probe(ag.ring.s, tok.idx, ag.params, tok.start, ag.H, PRECISIONS[args.precision],
                    counts, stats, mask)

    def norms0():
        K.layer_norms(ag.params, ag.H, out=out)

    def norms1():
        K.layer_norms(ag.adam_m, ag.H, y=ag.adam_v, eps=eps, out=out)

    def copy():
        _lib.call("dmdqn_stream_probe", _lib.ptr(dst), _lib.ptr(src), n_copy, 0, _lib.stream_of(dev))

    def learn_alone():
        # bench.py full_probes: the learn launched alone, bracketed by events
        times = []
        for _ in range(args.learns):
            assert ag.learn_begin()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            ag.learn_range(0, NA)
            e1.record(stream)
            e1.synchronize()
            times.append(e0.elapsed_time(e1))
        return statistics.median(times)

    for fn in (probe, norms0, norms1, copy):  # warm-up: code objects loaded, pages touched
        window(fn, 3, stream)
    ms = {"probe": [], "norms_mode0": [], "norms_mode1": [], "learn_alone": [], "copy": []}
    for _ in range(args.rounds):
        ms["probe"].append(window(probe, args.reps, stream))
        ms["norms_mode0"].append(window(norms0, args.reps, stream))
        ms["norms_mode1"].append(window(norms1, args.reps, stream))
        ms["learn_alone"].append(learn_alone())
        ms["copy"].append(window(copy, args.reps, stream))
    med = {k: statistics.median(v) for k, v in ms.items()}
    copy_gbs = 2 * n_copy / (med["copy"] * 1e-3) / 1e9
    probe_bytes = NA * PROBE_READ_BYTES_PER_AGENT
    learn_bytes = NA * learn_bytes_per_agent(P)
    res = {"what": "dmdqn_net_probe / dmdqn_layer_norms beside the learn alone and the "
                   "dmdqn_stream_probe copy, one process, medians over the rounds",
           "device": torch.cuda.get_device_name(dev), "lib_digest": _lib.LIB_DIGEST,
           "NA": NA, "P": P, "precision": args.precision, "rounds": args.rounds,
           "reps_per_window": args.reps, "ms_rounds": {k: [round(x, 4) for x in v] for k, v in ms.items()},
           "ms_median": {k: round(v, 4) for k, v in med.items()},
           "copy_GBps": round(copy_gbs, 1),
           "probe_bytes_per_agent": PROBE_READ_BYTES_PER_AGENT, "probe_bytes": probe_bytes,
           "probe_GBps": round(probe_bytes / (med["probe"] * 1e-3) / 1e9, 1),
           "probe_frac_of_copy": round(probe_bytes / (med["probe"] * 1e-3) / 1e9 / copy_gbs, 4),
           "norms_mode0_GBps": round(NA * P * 4 / (med["norms_mode0"] * 1e-3) / 1e9, 1),
           "norms_mode1_GBps": round(NA * P * 8 / (med["norms_mode1"] * 1e-3) / 1e9, 1),
           "learn_bytes_per_agent": learn_bytes_per_agent(P),
           "byte_ratio_probe_over_learn": round(probe_bytes / learn_bytes, 4),
           "probe_share_of_learn": round(med["probe"] / med["learn_alone"], 4),
           "probe_and_norms_share_of_learn": round(
               (med["probe"] + med["norms_mode0"] + med["norms_mode1"]) / med["learn_alone"], 4)}
    return res


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
    return {"what": "C3 Trainer (overlap env) with health_every 0 and "
                    f"{args.every}, alternating windows in one process, agent-env steps/s",
            "device": torch.cuda.get_device_name(dev), "lib_digest": _lib.LIB_DIGEST,
            "NA": on.NA, "precision": args.precision, "steps_per_window": args.steps,
            "rounds": args.rounds, "health_every": args.every,
            "probes_run": int(on.health["learn_step"]) // args.every if on.health else 0,
            "steps_per_s": {k: [round(x, 1) for x in v] for k, v in rates.items()},
            "median": {k: round(v, 1) for k, v in med.items()},
            "on_over_off": round(med["on"] / med["off"], 4),
            "off_spread": round((max(off) - min(off)) / med["off"], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--rows", type=int, default=4)
    ap.add_argument("--cols", type=int, default=4)
    ap.add_argument("--precision", default="fp16", choices=["fp16", "bf16"])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10, help="launches per kernel window")
    ap.add_argument("--learns", type=int, default=6, help="learns timed alone per round")
    ap.add_argument("--steps", type=int, default=200, help="trainer steps per end-to-end window")
    ap.add_argument("--every", type=int, default=100, help="health_every of the probed run")
    ap.add_argument("--warmup", type=int, default=140, help="steps before timing (learns from 128)")
    ap.add_argument("--outdir", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("health_bench needs a GPU: a CPU run measures nothing")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    trainers = {"off": make_trainer(args, 0), "on": make_trainer(args, args.every)}
    for tr in trainers.values():
        for _ in range(args.warmup):
            tr.step()
        tr.synchronize()
        assert tr.agent.learn_step_counter > 0
    parts = {"probe": kernel_part(args, trainers["on"], dev)}
    trainers["on"].join_streams()
    parts["e2e"] = e2e_part(args, trainers, dev)
    for name, res in parts.items():
        print(json.dumps(res), flush=True)
        if args.outdir:
            os.makedirs(args.outdir, exist_ok=True)
            with open(os.path.join(args.outdir, f"{name}.json"), "w") as f:
                f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
