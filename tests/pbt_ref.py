"""Population-based training: a pure-Python restatement of the contract of
AgentConfig.pbt / dmdqn_pbt_score / dmdqn_pbt_select / dmdqn_pbt_exchange
(include/dmdqn.h) and of BatchedDQN.pbt_explore.

Python floats are IEEE doubles and `+` / `*` on them are single rounded
operations, so the sums and products below are the bits the device and the
host code must produce.  Replicas are indexed 0 .. E-1; agent = e * A + j."""
import math

import numpy as np

from dmdqn_amd.agent import SWEEP_KEYS, nstep_gamma, soft_update_consts


def truncated(truncation, E):
    """n = floor(truncation * E)."""
    return int(math.floor(truncation * E))


def score(fitness, reward):
    """fitness[e] + ((r[e][0] + r[e][1]) + ...): a new list."""
    out = []
    for f, row in zip(fitness, reward):
        t = float(row[0])
        for r in row[1:]:
            t = t + float(r)
        out.append(float(f) + t)
    return out


def ranks(fitness):
    """rank[e] = #{x : f'[x] > f'[e]} + #{x < e : f'[x] == f'[e]}, NaN as -inf."""
    f = [-math.inf if x != x else float(x) for x in fitness]
    E = len(f)
    return [sum(1 for x in range(E) if f[x] > f[e]) + sum(1 for x in range(e) if f[x] == f[e])
            for e in range(E)]


def select(fitness, n):
    """(src, rank): src[e] = e for rank[e] < E - n, else the replica of rank
    E - 1 - rank[e]."""
    rank = ranks(fitness)
    E = len(rank)
    by_rank = {r: e for e, r in enumerate(rank)}
    src = [e if rank[e] < E - n else by_rank[E - 1 - rank[e]] for e in range(E)]
    return src, rank


def pairs(src):
    """[[dst, src], ...] of the copied replicas, dst ascending."""
    return [[e, s] for e, s in enumerate(src) if s != e]


def explore(values, src, perturb, bounds, seed, k, env_offset=0):
    """The values after round k: {key: [E floats]} -> a new dict.  One
    randint(0, len(factors), size=E) per perturbed key in SWEEP_KEYS order,
    drawn for every replica; a copied replica takes its source's value, times
    its factor and clipped on a perturbed key."""
    E = len(src)
    rs = np.random.RandomState(np.array([seed, k, env_offset], dtype=np.uint32))
    out = {key: [float(x) for x in v] for key, v in values.items()}
    for key in SWEEP_KEYS:
        c = None
        if key in perturb:
            c = rs.randint(0, len(perturb[key]), size=E)
        if key not in values:
            continue
        for e, s in enumerate(src):
            if s == e:
                continue
            v = float(values[key][s])
            if c is not None:
                lo, hi = bounds[key]
                v = min(max(v * float(perturb[key][c[e]]), lo), hi)
            out[key][e] = v
    return out


def fitness_vectors(E):
    """The selection tests' inputs for E replicas, {name: f64 [E]}: distinct
    values, ties, all equal, negatives only, +0.0 / -0.0 among small values,
    a NaN (alone, and beside a real -inf and ties)."""
    rng = np.random.RandomState(1000 + E)
    out = {"distinct": rng.permutation(E).astype(np.float64) * 1.5 - 3.0,
           "ties": rng.randint(0, 3, size=E).astype(np.float64),
           "equal": np.full(E, -7.25),
           "negative": -np.abs(rng.normal(scale=1e3, size=E)) - 1.0}
    z = rng.randint(-1, 2, size=E).astype(np.float64) * 1e-300
    z[::2] = 0.0
    z[1::4] = -0.0
    out["zeros"] = z
    nan = rng.normal(size=E)
    nan[E // 2] = np.nan
    out["nan"] = nan
    mixed = rng.randint(-2, 2, size=E).astype(np.float64)
    mixed[0] = -np.inf
    mixed[E - 1] = np.nan
    out["nan_inf_ties"] = mixed
    return out


def device_arrays(values, n_step, A):
    """The per-agent device arrays the values stand for, by the host formulas
    of dmdqn_amd.agent: {name: np array [E * A]}."""
    out = {}
    if "learning_rate" in values:
        out["hp_lr"] = np.repeat(np.asarray(values["learning_rate"], np.float64).astype(np.float32), A)
    if "gamma" in values:
        g = [nstep_gamma(v, n_step) for v in values["gamma"]]
        out["hp_gamma"] = np.repeat(np.asarray(g, np.float64).astype(np.float32), A)
        out["nstep_gamma_a"] = np.repeat(np.asarray(values["gamma"], np.float64), A)
    if "tau" in values:
        consts = [soft_update_consts(v) for v in values["tau"]]
        out["hp_tau"] = np.repeat(np.asarray([c[0] for c in consts], np.float32), A)
        out["hp_omt"] = np.repeat(np.asarray([c[1] for c in consts], np.float32), A)
    return out
