"""Measurement: dead-unit recycling (dmdqn_redo) at C3 size -- a 4x4 grid x 1024
replicas, NA = 16,384 fp16 agents -- in one process, and what
AgentConfig.redo_every costs a training run end to end.

Kernel (profiles/redo/redo.json): two C3 Trainers are warmed up (`--warmup`
steps, learns from step 128) and one more window of `--steps` steps each is
run; the dead mask of a probe of the trained nets of the run WITHOUT recycling
is the "realistic share".  Then `--rounds` rounds of, each between two device
events: the recycle launch on a zero mask (nothing fires), the recycle launch
on that mask at patience 1 (every dead unit fires, every launch: the streak
returns to 0 and the same mask fires it again) on copies of params / adam_m /
adam_v, the probe, and the learn alone.  Medians over the rounds.  The launch's
algorithmic bytes come from the mask (redo_bytes below).

End to end (profiles/redo/e2e.json): the two Trainers, redo_every 0 and
`--every` (1000), timed in alternating windows of `--steps` steps (host clock
around a device sync), `--rounds` rounds; then one probe of each run's nets
for the dead fractions with and without recycling (a single run).

  python tools/redo_bench.py [--rounds 3] [--steps 1000] [--every 1000] [--outdir profiles/redo]

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

from dmdqn_amd import _lib, kernels as K  # noqa: E402
from dmdqn_amd.agent import AgentConfig, PRECISIONS  # noqa: E402
from dmdqn_amd.env import EnvConfig  # noqa: E402
from dmdqn_amd.trainer import Trainer  # noqa: E402

NO_FIRE_BYTES = 32 + 256 + 256 + 40  # mask and streak read, streak, fired words and counts written


def window(fn, reps, stream):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    for _ in range(reps):
        fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b) / reps  # ms per launch


def redo_bytes(n1, n2, overlap):
    """Algorithmic bytes of the fired units over params, adam_m and adam_v
    (DESIGN section 5): n1 / n2 fired layer-1 / layer-2 units in all, overlap
    = sum over agents of n1 * n2 (the W2 chunks counted for both, which are
    stored once).  A fired layer-1 unit: its 88 tiled weights as 22 stored
    chunks (48 B each over the three arrays); its column entry, its bias and
    its 128 outgoing weights, one per W2T chunk, as 130 read-modify-written
    chunks (96 B each): 13,536 B.  A fired layer-2 unit: its 128 incoming
    weights as 32 stored chunks, its bias and 4 outgoing weights as 5
    read-modify-written chunks: 2,016 B.  An upper bound where fired units
    share a chunk."""
    store, rmw = 3 * 16, 3 * 32
    b1 = 22 * store + (1 + 1 + 128) * rmw
    b2 = 32 * store + (1 + 4) * rmw
    return n1 * b1 + n2 * b2 - overlap * rmw


def make_trainer(args, redo_every):
    return Trainer(EnvConfig(rows=args.rows, cols=args.cols, num_envs=args.envs, seed=1000),
                   AgentConfig(precision=args.precision, seed=1000, redo_every=redo_every),
                   overlap="env")


def dead_fracs(ag):
    h = ag.probe_health()
    c = h["counts"].double()
    return [float(c[:, 1].mean() / ag.H), float(c[:, 3].mean() / ag.H)], h


def kernel_part(args, tr, dev):
    ag = tr.agent
    NA = ag.NA
    stream = torch.cuda.current_stream(dev)
    tr.synchronize()
    tok = ag._last_tok
    frac, h = dead_fracs(ag)
    mask = h["dead_mask"].clone()
    counts = h["counts"].clone()
    zero = torch.zeros_like(mask)
    params, m, v = ag.params.clone(), ag.adam_m.clone(), ag.adam_v.clone()
    streak = torch.zeros((NA, 2, ag.H), dtype=torch.uint8, device=dev)
    rec = torch.zeros((NA, 2, 4), dtype=torch.int32, device=dev)
    nrec = torch.zeros((NA, 2), dtype=torch.int32, device=dev)
    pc, ps, pm = K.net_probe(ag.ring.s, tok.idx, ag.params, tok.start, ag.H,
                             PRECISIONS[args.precision])

    def redo_with(msk):
        K.redo(msk, streak, params, m, v, ag.H, 0, 1000, 1, 1, rec, nrec)

    def probe():
        K.net_probe(ag.ring.s, tok.idx, ag.params, tok.start, ag.H, PRECISIONS[args.precision],
                    pc, ps, pm)

    def learn_alone():
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

    for fn in (lambda: redo_with(zero), lambda: redo_with(mask), probe):  # warm-up
        window(fn, 3, stream)
    fired = nrec.double().sum(0).tolist()  # what a launch on the mask fires
    assert fired == [float(counts[:, 1].sum()), float(counts[:, 3].sum())]
    overlap = float((nrec[:, 0].double() * nrec[:, 1].double()).sum())
    ms = {"redo_no_fire": [], "redo_fire": [], "probe": [], "learn_alone": []}
    for _ in range(args.rounds):
        ms["redo_no_fire"].append(window(lambda: redo_with(zero), args.reps, stream))
        ms["redo_fire"].append(window(lambda: redo_with(mask), args.reps, stream))
        ms["probe"].append(window(probe, args.reps, stream))
        ms["learn_alone"].append(learn_alone())
    med = {k: statistics.median(x) for k, x in ms.items()}
    fire_bytes = NA * NO_FIRE_BYTES + redo_bytes(fired[0], fired[1], overlap)
    return {"what": "dmdqn_redo on a zero mask and on the dead mask of the trained nets (patience "
                    "1: every dead unit fires), beside the probe and the learn alone, one "
                    "process, medians over the rounds",
            "device": torch.cuda.get_device_name(dev), "lib_digest": _lib.LIB_DIGEST,
            "NA": NA, "precision": args.precision, "rounds": args.rounds,
            "reps_per_window": args.reps, "learn_step": int(ag.learn_step_counter),
            "dead_frac_of_the_mask": [round(x, 5) for x in frac],
            "fired_units": fired, "fired_per_agent": [round(x / NA, 3) for x in fired],
            "agents_touched": int((nrec.sum(1) > 0).sum()),
            "ms_rounds": {k: [round(x, 4) for x in v] for k, v in ms.items()},
            "ms_median": {k: round(x, 4) for k, x in med.items()},
            "no_fire_bytes": NA * NO_FIRE_BYTES,
            "no_fire_GBps": round(NA * NO_FIRE_BYTES / (med["redo_no_fire"] * 1e-3) / 1e9, 1),
            "fire_bytes": fire_bytes,
            "fire_GBps": round(fire_bytes / (med["redo_fire"] * 1e-3) / 1e9, 1),
            "fire_share_of_learn": round(med["redo_fire"] / med["learn_alone"], 4),
            "no_fire_share_of_learn": round(med["redo_no_fire"] / med["learn_alone"], 4)}


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
    dead = {}
    for name, tr in trainers.items():
        tr.quiesce()
        dead[name] = [round(x, 5) for x in dead_fracs(tr.agent)[0]]
        tr.join_streams()
    torch.cuda.synchronize(dev)
    return {"what": "C3 Trainer (overlap env) with redo_every 0 and "
                    f"{args.every}, alternating windows in one process, agent-env steps/s; the "
                    "dead fractions of one probe of each run's nets at the end (a single run)",
            "device": torch.cuda.get_device_name(dev), "lib_digest": _lib.LIB_DIGEST,
            "NA": on.NA, "precision": args.precision, "steps_per_window": args.steps,
            "rounds": args.rounds, "redo_every": args.every, "redo_rounds": int(on.redo_rounds),
            "recycled_total": [int(x) for x in on.redo_total.cpu()],
            "learn_steps": {k: int(t.agent.learn_step_counter) for k, t in trainers.items()},
            "dead_frac_end": dead,
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
    ap.add_argument("--steps", type=int, default=1000, help="trainer steps per end-to-end window")
    ap.add_argument("--every", type=int, default=1000, help="redo_every of the recycling run")
    ap.add_argument("--warmup", type=int, default=140, help="steps before timing (learns from 128)")
    ap.add_argument("--outdir", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("redo_bench needs a GPU: a CPU run measures nothing")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    trainers = {"off": make_trainer(args, 0), "on": make_trainer(args, args.every)}
    for tr in trainers.values():
        for _ in range(args.warmup + args.steps):
            tr.step()
        tr.synchronize()
        assert tr.agent.learn_step_counter > 0
    parts = {"redo": kernel_part(args, trainers["off"], dev)}
    trainers["off"].join_streams()
    parts["e2e"] = e2e_part(args, trainers, dev)
    for name, res in parts.items():
        print(json.dumps(res), flush=True)
        if args.outdir:
            os.makedirs(args.outdir, exist_ok=True)
            with open(os.path.join(args.outdir, f"{name}.json"), "w") as f:
                f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
