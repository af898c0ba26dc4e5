"""A/B of the soft (Polyak) target update at benchmark size, one process per
configuration, every launch through the C ABI on the same inputs:

  a      the learn with tau = 0 (what every learn ran before soft updates)
  b      the fused soft learn (dmdqn_learn_args.tau > 0, DMDQN_OPT_SOFT_PATH fused)
  c      the tau = 0 learn followed by dmdqn_target_soft_update (two launches)
  hard   the learn that ends with the hard target copy (sync_target)
  parent (--parent-lib) dmdqn_learn of another build of the library, e.g. the
         parent commit's from tools/build_rev.py, with the args of `a` (the
         struct of every revision is a prefix of this one's)

The modes alternate over --rounds rounds; each sample is a window of --reps
launches between two HIP events on one stream, synchronised at its end
(reps x ~2.5 ms at C3: well above the per-launch overheads; the window length
is written with the numbers).  The weights are restored before every window, so
each times the same work.  Rates are algorithmic bytes (bench.py
learn_bytes_per_agent; the soft update adds 10 B per parameter: target f32 read
and write, 16-bit shadow write; the hard copy 6 B) over the median window, as a
fraction of 8 TB/s, beside this process's float4 copy rate.

Without --child this is the driver: it runs C3 (4x4 x 1024) and C2 (2x2 x 256)
in fp16 and bf16, rings full, each child under its own `timeout`, stops at the first
failure and writes profiles/soft_target/<name>.json.
usage: python tools/soft_target_ab.py [--parent-lib lib.so] [--out DIR] [--rounds R] [--reps N]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# reps: launches per window, sized for a window of ~60-100 ms of the plain learn
CONFIGS = {"c3_fp16": dict(envs=1024, agents=16, precision="fp16", reps=40),
           "c2_bf16": dict(envs=256, agents=4, precision="bf16", reps=400),
           "c3_bf16": dict(envs=1024, agents=16, precision="bf16", reps=40),
           "c2_fp16": dict(envs=256, agents=4, precision="fp16", reps=400),
           # between the two, for the launcher's fused / two-launch cut
           "na2048_fp16": dict(envs=512, agents=4, precision="fp16", reps=200),
           "na4096_fp16": dict(envs=256, agents=16, precision="fp16", reps=100),
           "na8192_fp16": dict(envs=512, agents=16, precision="fp16", reps=60)}
TAU = 0.005


def child(a):
    import numpy as np
    import torch

    from bench import HBM_PEAK_GBS, learn_bytes_per_agent, stream_probe, stream_probe_bytes
    from dmdqn_amd import _lib
    from dmdqn_amd.agent import AgentConfig, BatchedDQN, PRECISIONS, soft_update_consts

    E, A = a.envs, a.agents
    ag = BatchedDQN(E, A, AgentConfig(precision=a.precision, seed=0, target_update_frequency=0,
                                      replay_buffer_size=a.replay))
    g = torch.Generator(device="cuda").manual_seed(0)
    pool = []
    for _ in range(4):
        s = torch.randint(-1, 24, (E, A, 89), device="cuda", generator=g).float()
        act = torch.randint(0, 4, (E, A), device="cuda", generator=g, dtype=torch.int32)
        r = -torch.rand((E, A), device="cuda", generator=g, dtype=torch.float64) * 100
        pool.append((s, act, r))
    for t in range(a.replay):  # rings full
        s, act, r = pool[t % 4]
        ag.remember(s, act, r, pool[(t + 1) % 4][0], t % 240 == 239)
    for _ in range(3):
        ag.learn()
    torch.cuda.synchronize()
    lib = _lib.load()
    _lib.set_option("soft_path", "fused")  # b times the fused kernel at every size
    stream = torch.cuda.current_stream()
    sp = C.c_void_p(stream.cuda_stream)
    tau_f, omt_f = soft_update_consts(TAU)

    def args_of(tau=0.0, sync=0):
        x = ag.c_learn_args()
        x.sync_target = sync
        x.tau, x.one_minus_tau = (tau_f, omt_f) if tau else (0.0, 0.0)
        return x

    plain, soft, hard = args_of(), args_of(TAU), args_of(sync=1)
    soft_call = (_lib.ptr(ag.params), _lib.ptr(ag.target), _lib.ptr(ag.target_h), ag.NW, ag.P,
                 ag.Ph, PRECISIONS[a.precision], C.c_float(tau_f), C.c_float(omt_f), sp)

    def learn_with(fn, x):
        def go():
            rc = fn(C.byref(x), sp)
            assert rc == 0, (rc, lib.dmdqn_last_error())
        return go

    def two_launches():
        learn_with(lib.dmdqn_learn, plain)()
        _lib.call("dmdqn_target_soft_update", *soft_call)

    P = ag.P
    base = learn_bytes_per_agent(P)
    modes = {"a": (learn_with(lib.dmdqn_learn, plain), base),
             "b": (learn_with(lib.dmdqn_learn, soft), base + 10 * P),
             "c": (two_launches, base + 14 * P),  # + the online net read again
             "hard": (learn_with(lib.dmdqn_learn, hard), base + 6 * P)}
    for i, path in enumerate(a.soft_lib or []):  # another build's fused soft learn
        fn = C.CDLL(os.path.abspath(path)).dmdqn_learn
        fn.argtypes, fn.restype = [C.c_void_p, C.c_void_p], C.c_int
        modes[f"b_alt{i}"] = (learn_with(fn, soft), base + 10 * P)
    if a.parent_lib:
        fn = C.CDLL(os.path.abspath(a.parent_lib)).dmdqn_learn
        fn.argtypes, fn.restype = [C.c_void_p, C.c_void_p], C.c_int
        modes["parent"] = (learn_with(fn, plain), base)

    keep = ("params", "target", "adam_m", "adam_v", "target_h")
    state = [getattr(ag, n).clone() for n in keep]

    def restore():
        for n, src in zip(keep, state):
            getattr(ag, n).copy_(src)

    # b and c leave the same bits (the contract the tests check at small size)
    finals = {}
    for name in [n for n in modes if n[0] in "bc"]:
        restore()
        modes[name][0]()
        torch.cuda.synchronize()
        finals[name] = [getattr(ag, n).clone() for n in keep]
    same_bits = all(torch.equal(x.view(torch.int16), y.view(torch.int16))
                    for f in finals.values() for x, y in zip(f, finals["c"]))

    ms = {name: [] for name in modes}
    for _ in range(a.rounds):
        for name, (go, _) in modes.items():
            restore()
            go()  # untimed first launch
            e0, e1 = _lib.TimingEvent(), _lib.TimingEvent()
            e0.record(stream)
            for _ in range(a.reps):
                go()
            e1.record(stream)
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1) / a.reps)
    n_probe = stream_probe_bytes(ag.device)
    probe = stream_probe(stream, n_probe) if n_probe else {}
    out = {"config": a.name, "envs": E, "agents_per_env": A, "precision": a.precision,
           "replay": a.replay, "tau": TAU, "rounds": a.rounds, "launches_per_window": a.reps,
           "b_equals_c_bitwise": bool(same_bits), "copy_gbs": probe.get("copy_gbs"),
           "library_digest": _lib.LIB_DIGEST, "parent_lib": a.parent_lib, "modes": {}}
    for name, v in ms.items():
        med = float(np.median(v))
        gbs = ag.NA * modes[name][1] / (med / 1e3) / 1e9
        out["modes"][name] = {
            "median_ms": round(med, 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
            "window_ms": round(med * a.reps, 1), "alg_bytes_per_agent": modes[name][1],
            "alg_gbs": round(gbs, 1), "frac_of_8tbs": round(gbs / HBM_PEAK_GBS, 3),
            "frac_of_copy": round(gbs / probe["copy_gbs"], 3) if probe.get("copy_gbs") else None}
    am = out["modes"]["a"]["median_ms"]
    out["ratios"] = {k: round(out["modes"][k]["median_ms"] / am, 4) for k in out["modes"]}
    out["a_spread"] = round((out["modes"]["a"]["max_ms"] - out["modes"]["a"]["min_ms"]) / am, 4)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--name", default="c3_fp16", choices=list(CONFIGS))
    ap.add_argument("--envs", type=int)
    ap.add_argument("--agents", type=int)
    ap.add_argument("--precision")
    ap.add_argument("--replay", type=int, default=10000)
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--reps", type=int, default=None, help="launches per window (default: CONFIGS)")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--soft-lib", action="append",
                    help="another build of this library (tools/build_exp.py): its fused soft "
                         "learn is timed as b_alt<i>")
    ap.add_argument("--only", default=None, help="run this configuration only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "soft_target"))
    ap.add_argument("--timeout", type=int, default=240, help="seconds per child")
    a = ap.parse_args()
    if a.child:
        for k, v in CONFIGS[a.name].items():
            if getattr(a, k) is None:
                setattr(a, k, v)
        return child(a)
    os.makedirs(a.out, exist_ok=True)
    for name in CONFIGS if a.only is None else [a.only]:
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__),
               "--child", "--name", name, "--replay", str(a.replay), "--rounds", str(a.rounds)]
        if a.reps:
            cmd += ["--reps", str(a.reps)]
        if a.parent_lib:
            cmd += ["--parent-lib", a.parent_lib]
        for p in a.soft_lib or []:
            cmd += ["--soft-lib", p]
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
        if r.returncode != 0:  # a fault, an abort or the time limit: nothing more runs
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            raise SystemExit(f"{name}: exit status {r.returncode}; stopping")
        line = r.stdout.strip().splitlines()[-1]
        with open(os.path.join(a.out, f"{name}.json"), "w") as f:
            f.write(json.dumps(json.loads(line), indent=1) + "\n")
        print(line)


if __name__ == "__main__":
    main()
