"""Measurement: the population-based training row exchange (dmdqn_pbt_exchange)
at C3 size beside the plain 16-B copy of dmdqn_stream_probe, in one process.

C3 is a 4x4 grid x 1024 replicas: NA = 16,384 agents of P = 28,548 parameters
(Ph = 28,552), and truncation 0.25 replaces 256 replicas = 4,096 agents.  The
exchange moves 2 * (16 P + 2 Ph) counted bytes per copied agent (each row read
once and written once: params, target, Adam m and v in f32, the 16-bit target
shadow); the probe copies half as many bytes from one buffer to another, so
both move the same total.  The two alternate, window by window, after a
warm-up; every window is `--reps` launches between two device events.

  python tools/pbt_bench.py [--rounds 10] [--reps 40] [--out FILE.json]

Prints one JSON line: GB/s of each (median, min, max over the windows), the
exchange's ratio to the probe and the probe's own spread.  Needs a GPU."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from dmdqn_amd import _lib  # noqa: E402
from dmdqn_amd.agent import n_params  # noqa: E402
from dmdqn_amd.ops import load as ops  # noqa: E402


def counted_bytes(copied_agents, P, Ph, with_h=True):
    """Bytes the exchange must move: every copied row read once, written once."""
    return 2 * (16 * P + (2 * Ph if with_h else 0)) * copied_agents


def window(fn, reps, stream):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    for _ in range(reps):
        fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b) / reps  # ms per launch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--agents", type=int, default=16, help="junctions per replica (4x4 grid)")
    ap.add_argument("--hidden", type=int, default=128)
    ap.add_argument("--truncation", type=float, default=0.25)
    ap.add_argument("--rounds", type=int, default=10, help="alternating windows of each kind")
    ap.add_argument("--reps", type=int, default=40, help="launches per window")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pbt_bench needs a GPU: a CPU run measures nothing")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    D = ops()
    E, A = args.envs, args.agents
    P = n_params(args.hidden)
    Ph = (P + 7) // 8 * 8
    NA, n = E * A, int(args.truncation * E)
    g = torch.Generator(device=dev).manual_seed(0)
    rows = [torch.randn((NA, P), dtype=torch.float32, device=dev, generator=g) for _ in range(4)]
    target_h = torch.randn((NA, Ph), dtype=torch.float32, device=dev, generator=g).half()
    # the worst n replicas take the best n: here the last n from the first n
    src = torch.arange(E, dtype=torch.int32)
    src[E - n:] = torch.arange(n - 1, -1, -1, dtype=torch.int32)
    src = src.to(dev)
    moved = counted_bytes(n * A, P, Ph)
    half = moved // 2 // 16 * 16
    probe_src = torch.empty(half, dtype=torch.uint8, device=dev).random_(0, 256, generator=g)
    probe_dst = torch.empty_like(probe_src)
    stream = torch.cuda.current_stream(dev)

    def exchange():
        D.pbt_exchange(src, A, *rows, target_h)

    def probe():
        _lib.call("dmdqn_stream_probe", _lib.ptr(probe_dst), _lib.ptr(probe_src), half, 0,
                  _lib.stream_of(dev))

    for fn in (exchange, probe):  # warm-up: code objects loaded, pages touched
        window(fn, 5, stream)
    ms = {"exchange": [], "probe_copy": []}
    for _ in range(args.rounds):
        ms["exchange"].append(window(exchange, args.reps, stream))
        ms["probe_copy"].append(window(probe, args.reps, stream))
    assert torch.equal(rows[0][(E - 1) * A:], rows[0][:A])  # the exchange did copy

    def rates(times, nbytes):
        gbs = sorted(nbytes / (t * 1e-3) / 1e9 for t in times)
        return {"median": round(statistics.median(gbs), 1), "min": round(gbs[0], 1),
                "max": round(gbs[-1], 1), "ms_median": round(statistics.median(times), 4)}
    ex, pr = rates(ms["exchange"], moved), rates(ms["probe_copy"], 2 * half)
    res = {"what": "dmdqn_pbt_exchange vs dmdqn_stream_probe copy, alternating windows, one process",
           "device": torch.cuda.get_device_name(dev), "lib_digest": _lib.LIB_DIGEST,
           "E": E, "A": A, "P": P, "Ph": Ph, "copied_replicas": n, "copied_agents": n * A,
           "counted_bytes": moved, "probe_bytes": 2 * half, "rounds": args.rounds,
           "reps_per_window": args.reps, "exchange_GBps": ex, "probe_copy_GBps": pr,
           "exchange_over_probe": round(ex["median"] / pr["median"], 4),
           "probe_spread": round((pr["max"] - pr["min"]) / pr["median"], 4),
           "exchange_spread": round((ex["max"] - ex["min"]) / ex["median"], 4)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
