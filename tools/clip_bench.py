"""What global-norm gradient clipping costs (DESIGN §6 "Gradient clipping"),
two measurements on one box, arms alternating, at C3 size by default (1024 envs
x 16 agents, fp16):

kernel (default): dmdqn_adam_agents_clip against the flat dmdqn_adam_agents
  (learn_h16.hpp's k_adam_agents_*, the code of the revision before clipping)
  on the same gradient buffer and state, alone on the chip: R rounds; in each,
  N launches of either arm, every launch between two fence-free timing events.
  Per target mode (none, soft).  The byte counts are equal but for 4 B per
  agent, so the expectation is parity; the allowance is the flat kernel's own
  round-to-round spread in this job.

--e2e: Trainer.step throughput (overlap "env") with global_clipnorm set against
  the same config without it (fused learn, paired), two trainers in one
  process, rounds alternating.  Reported, not gated.

usage: python tools/clip_bench.py [--rounds 4] [--reps 30] [--envs 1024] [--agents 16] [--bf16]
           [--out FILE.json]
       python tools/clip_bench.py --e2e [--rounds 3] [--steps 200] [--replay 10000] [--clip 10]
           [--out FILE.json]
(--out: the JSON is merged into FILE.json if it exists; always printed)"""
import ctypes as C
import hashlib
import json
import os
import sys
import time

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


def _digests():
    from dmdqn_amd import _lib, build
    with open(os.path.join(build.CSRC, "adam_clip.hip"), "rb") as f:
        clip = hashlib.sha256(f.read()).hexdigest()[:16]
    return {"lib_digest": _lib.LIB_DIGEST, "learn_sources_digest": build.source_digest("learn"),
            "adam_clip_hip_sha256": clip}


def kernel(out):
    R, N = _opt("--rounds", 4), _opt("--reps", 30)
    E, A = _opt("--envs", 1024), _opt("--agents", 16)
    prec = "bf16" if _flag("--bf16") else "fp16"
    import torch
    from dmdqn_amd import _lib
    from dmdqn_amd.agent import CLearn, H16_DTYPES, PRECISIONS, keras_adam_consts, n_params, \
        soft_update_consts
    lib = _lib.load()
    NA, P = E * A, n_params(128)
    Ph = (P + 7) // 8 * 8
    g = torch.Generator(device="cuda").manual_seed(0)

    def rand(scale):
        t = torch.empty((NA, P), dtype=torch.float32, device="cuda")
        for lo in range(0, NA, 2048):
            t[lo:lo + 2048].normal_(0.0, scale, generator=g)
        return t
    params, m, v, target = rand(0.1), rand(1e-3), rand(1e-2).abs_(), rand(0.1)
    target_h = torch.zeros((NA, Ph), dtype=H16_DTYPES[prec], device="cuda")
    # 16-bit gradient values, the agents' norms spread over two decades around the clip
    grad = rand(0.05)
    grad *= 10.0 ** torch.empty((NA, 1), device="cuda").uniform_(-1.0, 1.0, generator=g)
    grad.copy_(grad.to(H16_DTYPES[prec]).float())
    gnorm = torch.zeros(NA, dtype=torch.float32, device="cuda")
    clip = float(np.float32(0.05 * np.sqrt(P)))
    alpha, c1, c2, eps = keras_adam_consts(100, 1e-3)
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    sp = C.c_void_p(stream.cuda_stream)
    gp = C.c_void_p(grad.data_ptr())

    res = {"config": dict(envs=E, agents=A, precision=prec, rounds=R, reps=N, clip=clip,
                          device=torch.cuda.get_device_name(0), **_digests()), "modes": {}}
    for mode, tau in (("none", 0.0), ("soft", 0.01)):
        a = CLearn()
        a.NA, a.cap, a.batch, a.hidden, a.precision, a.P = NA, 302, 128, 128, PRECISIONS[prec], P
        a.params, a.adam_m, a.adam_v, a.target = (t.data_ptr() for t in (params, m, v, target))
        a.target_h = target_h.data_ptr()
        a.alpha, a.c1, a.c2, a.eps = alpha, c1, c2, eps
        a.tau, a.one_minus_tau = soft_update_consts(tau) if tau else (0.0, 1.0)

        def flat():
            assert lib.dmdqn_adam_agents(C.byref(a), gp, sp) == 0, lib.dmdqn_last_error()

        def clipped():
            assert lib.dmdqn_adam_agents_clip(C.byref(a), None, gp, C.c_float(clip),
                                              C.c_void_p(gnorm.data_ptr()), sp) == 0, \
                lib.dmdqn_last_error()
        arms = {"flat": flat, "clip": clipped}
        for fn in arms.values():  # code loaded, caches in their steady state
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        d = {k: {"rounds_median_ms": [], "rounds_min_ms": []} for k in arms}
        for _ in range(R):
            for name, fn in arms.items():
                ms = []
                for _ in range(N):
                    e0, e1 = _lib.TimingEvent(), _lib.TimingEvent()
                    e0.record(stream)
                    fn()
                    e1.record(stream)
                    e1.synchronize()
                    ms.append(e0.elapsed_time(e1))
                d[name]["rounds_median_ms"].append(round(float(np.median(ms)), 4))
                d[name]["rounds_min_ms"].append(round(float(min(ms)), 4))
        f, c = d["flat"]["rounds_median_ms"], d["clip"]["rounds_median_ms"]
        # algorithmic bytes: 28 B / parameter (g, and w, m, v read and written),
        # + 8 (soft: target read and written) + 2 (its shadow); + 4 B / agent
        bytes_flat = NA * P * (28 + (10 if tau else 0))
        d["clip_over_flat"] = [round(x / y, 4) for x, y in zip(c, f)]
        d["flat_spread_max_over_min"] = round(max(f) / min(f), 4)
        d["clip_within_flat_spread"] = bool(min(f) <= float(np.median(c)) <= max(f))
        d["flat_GBps"] = round(bytes_flat / (float(np.median(f)) * 1e-3) / 1e9, 1)
        d["clip_GBps"] = round((bytes_flat + 4 * NA) / (float(np.median(c)) * 1e-3) / 1e9, 1)
        d["clipped_frac"] = float((gnorm > clip).float().mean())
        res["modes"][mode] = d
    _merge(out, {"kernel": res})


def e2e(out):
    R, steps = _opt("--rounds", 3), _opt("--steps", 200)
    E, rows, cols = _opt("--envs", 1024), _opt("--rows", 4), _opt("--cols", 4)
    cap, clip = _opt("--replay", 10000), _opt("--clip", 10.0, float)
    prec = "bf16" if _flag("--bf16") else "fp16"
    import torch
    from bench import PREFILL_LEARN_TAIL, fill_rings
    from dmdqn_amd.agent import AgentConfig
    from dmdqn_amd.env import EnvConfig
    from dmdqn_amd.trainer import Trainer
    work = torch.cuda.Stream()
    torch.cuda.set_stream(work)
    trs = {}
    for name, c in (("off", 0.0), ("clip", clip)):
        tr = Trainer(EnvConfig(rows=rows, cols=cols, num_envs=E, seed=1000),
                     AgentConfig(precision=prec, seed=1000, replay_buffer_size=cap,
                                 global_clipnorm=c), overlap="env")
        tail = min(cap, PREFILL_LEARN_TAIL)
        fill_rings(tr, cap - tail)
        for _ in range(tail + 10):
            tr.step()
        tr.sync_outputs()
        torch.cuda.synchronize()
        trs[name] = tr
    NA = trs["off"].agent.NA
    res = {"config": dict(envs=E, rows=rows, cols=cols, precision=prec, replay=cap, clip=clip,
                          steps=steps, rounds=R, overlap="env",
                          device=torch.cuda.get_device_name(0), **_digests()),
           "arms": {k: {"rounds_Msteps_per_s": []} for k in trs}}
    for _ in range(R):
        for name, tr in trs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                tr.step()
            tr.sync_outputs()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            res["arms"][name]["rounds_Msteps_per_s"].append(round(steps * NA / dt / 1e6, 4))
    for name, tr in trs.items():
        res["arms"][name]["pair_launches"] = tr.agent.pair_launches
        res["arms"][name]["learn_launches"] = tr.agent.learn_launches
    o, c = (res["arms"][k]["rounds_Msteps_per_s"] for k in ("off", "clip"))
    res["clip_over_off"] = [round(x / y, 4) for x, y in zip(c, o)]
    res["clip_over_off_median"] = round(float(np.median(c) / np.median(o)), 4)
    met = trs["clip"].agent.learn_metrics()
    res["last_learn"] = {k: met[k] for k in ("grad_norm_mean", "grad_norm_max", "clipped_frac")}
    _merge(out, {"e2e": res})


if __name__ == "__main__":
    out_ = _opt("--out", None, str)
    e2e(out_) if _flag("--e2e") else kernel(out_)
