"""Gate of the paired learn: dmdqn_learn_pair (one k_learn_*_x2 launch) against
the same two learns as two dmdqn_learn launches, alone on the chip, on the
same box and the same inputs, alternating.  C3-size state by default (1024
envs x 16 agents, fp16, replay 10000 in full, wrapped rings of random rows);
learn stream only, nothing on any other stream.

Timing (default mode): R rounds; in each, N pair launches, then N times the two
single launches, each timed with fence-free events (dmdqn_timing_event_create)
around it.  A third arm (--range-agents K, 0 = off) runs the pair kernel as a
plain loop of launches over ranges of K agents (offset pointers), so that at
most K workgroups -- K x ~400 KB of state -- are in flight: it tells the
cache's capacity from its policy.  Before the rounds each arm runs once from
the same starting state and the sha1 of the weights is compared.
The decision rule (DESIGN §6 "Paired learn"): integrate the pair into the trainer only if it
takes at least 5 % less time than the two singles in EVERY round.

Counters (--counters, for a `rocprofv3 --pmc FETCH_SIZE` or `--pmc WRITE_SIZE`
run of its own, no tracing flags): a few launches of each arm and nothing else
after the setup; --reduce FETCH.csv WRITE.csv then folds the two CSVs into the
JSON (FETCH_SIZE doubled, as tools/pmc_learn.py does).

usage: python tools/ab_learn_pair.py [--rounds 6] [--reps 20] [--envs 1024] [--agents 16]
           [--replay 10000] [--bf16] [--tau-permille 0] [--range-agents 256] [--out FILE.json]
       python tools/ab_learn_pair.py --counters [--replay 1000] ...
       python tools/ab_learn_pair.py --reduce FETCH.csv WRITE.csv --out FILE.json
(--out: the JSON is merged into FILE.json if it exists; always printed)"""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _opt(name, default, kind=int):
    if name in sys.argv:
        i = sys.argv.index(name)
        v = kind(sys.argv[i + 1])
        del sys.argv[i:i + 2]
        return v
    return default


def _flag(name):
    if name in sys.argv:
        sys.argv.remove(name)
        return True
    return False


def _merge(out, d):
    print(json.dumps(d))
    if not out:
        return
    old = {}
    if os.path.exists(out):
        with open(out) as f:
            old = json.load(f)
    old.update(d)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(old, f, indent=1)


def reduce_counters(fetch_csv, write_csv, out):
    """Per-dispatch mean FETCH_SIZE / WRITE_SIZE (KB) of the single and the
    paired kernel; HBM bytes = 2 x fetch + write (MI355X: FETCH_SIZE reports
    half of a wide stream)."""
    from tools.pmc_learn import per_kernel
    d = {}
    for arm, name in (("single", "k_learn_f16<"), ("single", "k_learn_bf16<"),
                      ("pair", "k_learn_f16_x2"), ("pair", "k_learn_bf16_x2")):
        fv = per_kernel(fetch_csv, "FETCH_SIZE", name)
        wv = per_kernel(write_csv, "WRITE_SIZE", name)
        if not fv or not wv:
            continue
        f_kb, w_kb = sum(fv) / len(fv), sum(wv) / len(wv)
        d[arm] = {"kernel": name.rstrip("<"), "dispatches": [len(fv), len(wv)],
                  "FETCH_SIZE_KB_raw": f_kb, "WRITE_SIZE_KB_raw": w_kb,
                  "read_bytes_per_launch": int(round(2.0 * f_kb * 1024)),
                  "write_bytes_per_launch": int(round(w_kb * 1024)),
                  "hbm_bytes_per_launch": int(round((2.0 * f_kb + w_kb) * 1024))}
    if "single" in d and "pair" in d:
        two = 2 * d["single"]["hbm_bytes_per_launch"]
        d["pair_over_two_singles_bytes"] = round(d["pair"]["hbm_bytes_per_launch"] / two, 4)
    _merge(out, {"counters": d})


def main():
    out = _opt("--out", None, str)
    if "--reduce" in sys.argv:
        i = sys.argv.index("--reduce")
        return reduce_counters(sys.argv[i + 1], sys.argv[i + 2], out)
    counters = _flag("--counters")
    R, N = _opt("--rounds", 6), _opt("--reps", 20)
    E, A = _opt("--envs", 1024), _opt("--agents", 16)
    cap = _opt("--replay", 1000 if counters else 10000)
    tau = _opt("--tau-permille", 0) / 1000.0
    K = _opt("--range-agents", 256)
    prec = "bf16" if _flag("--bf16") else "fp16"

    import torch
    from dmdqn_amd import _lib
    from dmdqn_amd.agent import AgentConfig, BatchedDQN, CLearn

    ag = BatchedDQN(E, A, AgentConfig(precision=prec, seed=0, replay_buffer_size=cap, tau=tau,
                                      target_update_frequency=0 if tau else 10 ** 9))
    NA, ring = ag.NA, ag.ring
    g = torch.Generator(device="cuda").manual_seed(0)
    # full rings of random rows, wrapped: the features, then the s' row's tail
    # (action, done flag, f64 reward: include/dmdqn.h DMDQN_ROW_A / _D / _R)
    for rows in (ring.s, ring.n):
        for lo in range(0, NA, 1024):
            rows[lo:lo + 1024, :, :89].random_(-1, 24, generator=g)
    for lo in range(0, NA, 1024):
        n = ring.n[lo:lo + 1024]
        n[:, :, 96].random_(0, 4, generator=g)
        n[:, :, 97] = 0
        n[:, :, 98:].zero_()
        n.view(torch.float64)[:, :, 13] = -100.0 * torch.rand(n.shape[:2], device="cuda",
                                                              dtype=torch.float64, generator=g)
    ring.a.copy_(ring.n[:, :, 96].to(torch.uint8))
    ring.r.copy_(ring.n.view(torch.float64)[:, :, 13])
    ring.total = cap + cap // 3 + 7  # full and wrapped
    for _ in range(3):
        ag.learn()
    torch.cuda.synchronize()

    learns, keep = [], []
    for _ in range(2):  # two consecutive learns: their own draws, loss buffer and Adam constants
        assert ag.learn_begin()
        a = ag.c_learn_args()
        idx = ag.idx.clone()
        a.idx = idx.data_ptr()
        keep.append(idx)
        learns.append(a)
    a0, a1 = learns
    lib = _lib.load()
    stream = torch.cuda.current_stream()
    sp = C.c_void_p(stream.cuda_stream)

    def pair():
        assert lib.dmdqn_learn_pair(C.byref(a0), C.byref(a1), None, None, sp) == 0, \
            lib.dmdqn_last_error()

    def singles():
        assert lib.dmdqn_learn(C.byref(a0), sp) == 0 and lib.dmdqn_learn(C.byref(a1), sp) == 0, \
            lib.dmdqn_last_error()

    # the pair kernel over ranges of K agents: every per-agent pointer offset
    Ph = (ag.P + 7) // 8 * 8
    stride = dict(ring_s=ring.slots * 128, ring_n=ring.slots * 128, ring_a=ring.slots,
                  ring_d=ring.slots, ring_r=ring.slots * 8, idx=128 * 4, params=ag.P * 4,
                  adam_m=ag.P * 4, adam_v=ag.P * 4, target=ag.P * 4, target_h=Ph * 2, loss=4)
    ranges = []
    if K > 0:
        for lo in range(0, NA, K):
            blocks = []
            for a in (a0, a1):
                b = CLearn.from_buffer_copy(bytes(a))
                b.NA = min(K, NA - lo)
                for f, s in stride.items():
                    setattr(b, f, getattr(a, f) + lo * s)
                blocks.append(b)
            ranges.append(blocks)

    def ranged():
        for b0, b1 in ranges:
            assert lib.dmdqn_learn_pair(C.byref(b0), C.byref(b1), None, None, sp) == 0, \
                lib.dmdqn_last_error()

    arms = {"pair": pair, "two_singles": singles}
    if ranges:
        arms[f"pair_ranges_of_{K}"] = ranged

    names = ("params", "target", "adam_m", "adam_v", "target_h")
    state = [getattr(ag, n).clone() for n in names]

    def restore():
        for n, src in zip(names, state):
            getattr(ag, n).copy_(src)

    if counters:  # a counter pass: a few launches of each arm, nothing else
        for fn in (pair, singles):
            restore()
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        return

    res = {"config": {"envs": E, "agents": A, "precision": prec, "replay": cap, "tau": tau,
                      "rounds": R, "reps": N, "device": torch.cuda.get_device_name(0),
                      "lib_digest": _lib.LIB_DIGEST}, "arms": {}}
    for name, fn in arms.items():
        restore()
        fn()
        torch.cuda.synchronize()
        res["arms"][name] = {"params_sha1": hashlib.sha1(
            ag.params.cpu().numpy().tobytes()).hexdigest()[:16], "rounds_median_ms": [],
            "rounds_min_ms": []}
    res["weights_equal"] = len({d["params_sha1"] for d in res["arms"].values()}) == 1
    for _ in range(R):
        for name, fn in arms.items():
            restore()
            ms = []
            for _ in range(N):
                e0, e1 = _lib.TimingEvent(), _lib.TimingEvent()
                e0.record(stream)
                fn()
                e1.record(stream)
                e1.synchronize()
                ms.append(e0.elapsed_time(e1))
            res["arms"][name]["rounds_median_ms"].append(round(float(np.median(ms)), 4))
            res["arms"][name]["rounds_min_ms"].append(round(float(min(ms)), 4))
    for d in res["arms"].values():
        d["median_ms"] = round(float(np.median(d["rounds_median_ms"])), 4)
    p, s = res["arms"]["pair"]["rounds_median_ms"], res["arms"]["two_singles"]["rounds_median_ms"]
    res["pair_over_two_singles"] = [round(x / y, 4) for x, y in zip(p, s)]
    res["gate_5pct_every_round"] = all(x <= 0.95 * y for x, y in zip(p, s))
    _merge(out, {"timing": res})


if __name__ == "__main__":
    main()
