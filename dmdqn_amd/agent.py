"""Batched Double-DQN agents on the GPU (replaces src/agents/dqn_agent.py).

`BatchedDQN` holds NA = E*A independent agents (one per junction per env
replica): online / target Q-networks, Keras-3 Adam slots, replay rings and the
per-env random streams, all resident in HBM.  One call of each method acts,
stores or learns for every agent:

  act(obs)                         DQNAgent.select_action  (dqn_agent.py:246-274)
  remember(s, a, r, s', done)      DQNAgent.remember       (:312-326)
  replay()                         DQNAgent.replay / learn (:328-380, :428-434)
  update_target_network()          (:382-387)
  update_target_network_soft()     (:389-399; cfg.tau > 0: fused into replay())

Draw-order contract (bit-exact with the reference when E = 1 and the global
streams are seeded with random.seed(s) / np.random.seed(s)): per env, agents
in junction order draw from that env's numpy stream for act and from its
CPython `random` stream for replay sampling.

Hyperparameter sweeps: AgentConfig.sweep gives every env replica its own
learning_rate / gamma / tau (a grid of variants, replica g runs variant g % G),
carried to the kernels as per-agent device arrays (include/dmdqn.h
dmdqn_agent_hparams).  A replica computes, bit for bit, what it computes in a
run whose scalar config holds its variant's values.

n-step returns: with AgentConfig.n_step > 1, remember() (or a fused env step)
writes the raw transition into a staging ring of n_step slots and one more
launch (dmdqn_replay_nstep_commit) stores the n-step transition of the oldest
staged one into the replay ring; the learn is unchanged and bootstraps with
gamma^n_step, and its batch z-score runs over the stored returns.

Population-based training: with AgentConfig.pbt the replicas are a population.
pbt_score() adds a step's reward to each replica's fitness; at a round
pbt_select() ranks them, pbt_exchange() copies the best replicas' nets and Adam
slots over the worst ones' in place and pbt_explore() perturbs the copied
per-agent hyperparameters (the Trainer calls all four).

Gradient clipping: with AgentConfig.global_clipnorm > 0 every learn runs as the
split learn whose Adam launch first clips each agent's gradient by its global
norm (Keras's Adam(global_clipnorm=...); include/dmdqn.h dmdqn_adam_agents_clip);
grad_norm holds the norms before clipping and learn_metrics() reports them.

Network health probe: probe_health() runs every agent's online forward on its
last batch and reduces it to dead / active ReLU units, non-finite
pre-activations and per-variable weight norms and update-to-weight ratios
(include/dmdqn.h dmdqn_net_probe, dmdqn_layer_norms); it only reads.  With
AgentConfig.health_every = N a Trainer calls it after every N-th learn and
learn_metrics() reports the last probe under "health".

Dead-unit recycling: redo() runs that probe and gives every hidden unit that
was dead on redo_patience probes in a row fresh incoming weights, zero outgoing
weights and zero Adam moments (ReDo; include/dmdqn.h dmdqn_redo).  With
AgentConfig.redo_every = N a Trainer calls it after every N-th learn and
learn_metrics() reports the rounds under "redo".
"""
import itertools
import math
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np
import torch

from . import _lib
from . import kernels as K
from .ops import load as _ops

D_IN = 89
N_ACTIONS = 4


CLearn = _lib.CLearn  # include/dmdqn.h dmdqn_learn_args
CHParams = _lib.CHParams  # include/dmdqn.h dmdqn_agent_hparams

PRECISIONS = {"fp32": 0, "fp16": 1, "bf16": 2}
# include/dmdqn.h DMDQN_LOSS_*: the reference's MSE (dqn_agent.py:352) and the
# Huber loss of src/experimental/agent.py:99 (delta 1)
LOSSES = {"mse": 0, "huber": 1}
# dtype of the 16-bit operand copies (target shadow, shared online copy)
H16_DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16}


D_PAD = 96  # feature stride of an observation row in the replay ring (qnet_layout.hpp)
D_TILED = 88  # layer-1 features held in 16x16 tiles; feature 88 is a separate column


def n_params_keras(hidden, n_actions=N_ACTIONS):
    """Parameters of the reference Keras model (dqn_agent.py:153-184)."""
    H = hidden
    return D_IN * H + H + H * H + H + H * n_actions + n_actions


def n_params(hidden, n_actions=N_ACTIONS):
    """Floats per agent in the device layout (qnet_layout.hpp):
    W1T[H][0..87] | W1T[H][88] | W2T[H][H] | W3T[4][H] | b1[H] | b2[H] | b3[4]
    -- the Keras parameter count, no padding."""
    H = hidden
    return H * D_IN + H * H + n_actions * H + 2 * H + n_actions


def tile_wt(WT):
    """[..., N, K] row-major W^T -> [..., N*K] tiled device order (qnet_layout.hpp
    qn_wt): 16 x 16 tiles in row-major tile order, each [K%16 / 8][N%16][K%8]."""
    lead, (N, K) = WT.shape[:-2], WT.shape[-2:]
    t = WT.reshape(lead + (N // 16, 16, K // 16, 2, 8))
    n = len(lead)
    t = np.moveaxis(t, [n + 0, n + 2, n + 3, n + 1, n + 4], list(range(n, n + 5)))
    return t.reshape(lead + (N * K,))


def untile_wt(flat, N, K):
    """Inverse of tile_wt: [..., N*K] tiled -> [..., N, K] row-major."""
    lead = flat.shape[:-1]
    n = len(lead)
    t = flat.reshape(lead + (N // 16, K // 16, 2, 16, 8))
    t = np.moveaxis(t, list(range(n, n + 5)), [n + 0, n + 2, n + 3, n + 1, n + 4])
    return t.reshape(lead + (N, K))


def tile_w1(W1T):
    """[..., H, 89] row-major W1^T -> [..., 89*H] device order (qnet_layout.hpp
    qn_w1): per 16 neurons the tiles of features 0..79 and the first half
    (80..87) of the next, then the column of feature 88."""
    lead, H = W1T.shape[:-2], W1T.shape[-2]
    pad = np.zeros(lead + (H, D_PAD), np.float32)
    pad[..., :D_IN] = W1T
    t = tile_wt(pad).reshape(lead + (H // 16, 6, 2, 16, 8))
    blk = np.concatenate([t[..., :5, :, :, :].reshape(lead + (H // 16, 1280)),
                          t[..., 5, 0, :, :].reshape(lead + (H // 16, 128))], axis=-1)
    return np.concatenate([blk.reshape(lead + (H * D_TILED,)), W1T[..., D_TILED]], axis=-1)


def untile_w1(flat, H):
    """Inverse of tile_w1: [..., 89*H] -> [..., H, 89]."""
    lead = flat.shape[:-1]
    blk = flat[..., :H * D_TILED].reshape(lead + (H // 16, D_TILED * 16))
    t = np.zeros(lead + (H // 16, 6, 2, 16, 8), np.float32)
    t[..., :5, :, :, :] = blk[..., :1280].reshape(lead + (H // 16, 5, 2, 16, 8))
    t[..., 5, 0, :, :] = blk[..., 1280:].reshape(lead + (H // 16, 16, 8))
    W1T = untile_wt(t.reshape(lead + (H * D_PAD,)), H, D_PAD)[..., :D_IN].copy()
    W1T[..., D_TILED] = flat[..., H * D_TILED:H * D_IN]
    return W1T


def keras_to_kernel(flat, hidden):
    """[..., P_keras] Keras get_weights order -> [..., P_kernel] device layout."""
    H = hidden
    flat = np.asarray(flat, dtype=np.float32)
    lead = flat.shape[:-1]
    o = 0
    W1 = flat[..., o:o + D_IN * H].reshape(lead + (D_IN, H)); o += D_IN * H
    b1 = flat[..., o:o + H]; o += H
    W2 = flat[..., o:o + H * H].reshape(lead + (H, H)); o += H * H
    b2 = flat[..., o:o + H]; o += H
    W3 = flat[..., o:o + H * N_ACTIONS].reshape(lead + (H, N_ACTIONS)); o += H * N_ACTIONS
    b3 = flat[..., o:o + N_ACTIONS]
    parts = [tile_w1(np.swapaxes(W1, -1, -2)), tile_wt(np.swapaxes(W2, -1, -2)),
             np.swapaxes(W3, -1, -2).reshape(lead + (-1,)), b1, b2, b3]
    return np.concatenate(parts, axis=-1)


def kernel_to_keras(flat, hidden):
    """Inverse of keras_to_kernel."""
    H = hidden
    flat = np.asarray(flat, dtype=np.float32)
    lead = flat.shape[:-1]
    o = 0
    W1T = untile_w1(flat[..., o:o + H * D_IN], H); o += H * D_IN
    W2T = untile_wt(flat[..., o:o + H * H], H, H); o += H * H
    W3T = flat[..., o:o + N_ACTIONS * H].reshape(lead + (N_ACTIONS, H)); o += N_ACTIONS * H
    b1 = flat[..., o:o + H]; o += H
    b2 = flat[..., o:o + H]; o += H
    b3 = flat[..., o:o + N_ACTIONS]
    parts = [np.swapaxes(W1T, -1, -2).reshape(lead + (-1,)), b1,
             np.swapaxes(W2T, -1, -2).reshape(lead + (-1,)), b2,
             np.swapaxes(W3T, -1, -2).reshape(lead + (-1,)), b3]
    return np.concatenate(parts, axis=-1)


def keras_adam_factors(t, b1=0.9, b2=0.999):
    """(s, d) = (sqrt(1 - b2^t), 1 - b1^t) as float32: the two factors of
    keras/src/optimizers/adam.py update_step's step size that do not depend on
    the learning rate, alpha = fl32(fl32(lr * s) / d).  The kernels form alpha
    from them and a per-agent lr (dmdqn_agent_hparams.adam_s / .adam_d)."""
    f = np.float32
    b1p = np.power(f(b1), f(t), dtype=np.float32)
    b2p = np.power(f(b2), f(t), dtype=np.float32)
    return np.sqrt(f(1) - b2p, dtype=np.float32), f(f(1) - b1p)


def keras_adam_consts(t, lr, b1=0.9, b2=0.999, eps=1e-7):
    """keras/src/optimizers/adam.py update_step constants for local step t (f32 ops)."""
    f = np.float32
    s, d = keras_adam_factors(t, b1, b2)
    alpha = f(f(lr) * s) / d
    return float(alpha), float(f(1 - b1)), float(f(1 - b2)), float(f(eps))


def soft_update_consts(tau):
    """(tau_f, omt_f) of the soft target update (update_target_network_soft,
    dqn_agent.py:389-399) as the kernels receive them: float32(tau) and
    float32(1.0 - tau), the subtraction in double as Python evaluates
    `1.0 - self.tau`, rounded once."""
    tau = float(tau)
    return np.float32(tau), np.float32(1.0 - tau)


def check_tau(tau, allow_zero=True):
    """tau as a float, or ValueError: finite, in [0, 1] (0 = hard updates only)
    or, for an explicit soft update, in (0, 1]."""
    try:
        t = float(tau)
    except (TypeError, ValueError):
        raise ValueError(f"tau must be a number, got {tau!r}") from None
    if not (0.0 <= t <= 1.0) or (t == 0.0 and not allow_zero):
        raise ValueError(f"tau must be in {'[' if allow_zero else '('}0, 1], got {tau!r}")
    return t


def check_clipnorm(clip):
    """global_clipnorm as a float, or ValueError: finite and >= 0 (0 = no
    clipping), and, when on, finite and > 0 as the float32 the kernel takes."""
    try:
        c = float(clip)
    except (TypeError, ValueError):
        raise ValueError(f"global_clipnorm must be a number, got {clip!r}") from None
    if not (math.isfinite(c) and c >= 0.0):
        raise ValueError(f"global_clipnorm must be finite and >= 0, got {clip!r}")
    with np.errstate(over="ignore"):
        c32 = np.float32(c)
    if c > 0.0 and not (np.isfinite(c32) and c32 > 0.0):
        raise ValueError(f"global_clipnorm = {clip!r} is not a positive finite float32")
    return c


def check_health_every(n):
    """health_every as an int, or ValueError: an integer >= 0 (0 = no probe)."""
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or int(n) < 0:
        raise ValueError(f"health_every must be an integer >= 0, got {n!r}")
    return int(n)


def check_redo(every, patience):
    """(redo_every, redo_patience) as ints, or ValueError: redo_every an integer
    >= 0 (0 = no recycling), redo_patience an integer in 1..255 (the streak is
    one byte per unit)."""
    if isinstance(every, bool) or not isinstance(every, (int, np.integer)) or int(every) < 0:
        raise ValueError(f"redo_every must be an integer >= 0, got {every!r}")
    if (isinstance(patience, bool) or not isinstance(patience, (int, np.integer))
            or not 1 <= int(patience) <= 255):
        raise ValueError(f"redo_patience must be an integer in 1..255, got {patience!r}")
    return int(every), int(patience)


# rule-based behaviour policies (kernels.RULES, include/dmdqn.h dmdqn_act_rule)
BEHAVIORS = tuple(K.RULES)


def check_behavior(behavior, steps, eps):
    """(behavior, behavior_steps, behavior_eps) checked, or ValueError:
    behavior None or one of BEHAVIORS, behavior_steps an integer >= 0 (0 = the
    whole run), behavior_eps a number in [0, 1]."""
    if behavior is not None and behavior not in BEHAVIORS:
        raise ValueError(f"behavior must be None or one of {list(BEHAVIORS)}, got {behavior!r}")
    if isinstance(steps, bool) or not isinstance(steps, (int, np.integer)) or int(steps) < 0:
        raise ValueError(f"behavior_steps must be an integer >= 0, got {steps!r}")
    try:
        e = float(eps)
    except (TypeError, ValueError):
        raise ValueError(f"behavior_eps must be a number in [0, 1], got {eps!r}") from None
    if not 0.0 <= e <= 1.0:  # (false for NaN too)
        raise ValueError(f"behavior_eps must be in [0, 1], got {eps!r}")
    return behavior, int(steps), e


# the Keras variables of one net, in get_weights order (dmdqn_layer_norms' columns)
VARIABLES = ("W1", "b1", "W2", "b2", "W3", "b3")

SWEEP_KEYS = ("learning_rate", "gamma", "tau")

CNStep = _lib.CNStep  # include/dmdqn.h dmdqn_nstep_args
NSTEP_MAX = _lib.NSTEP_MAX


def check_n_step(n_step, replay_buffer_size):
    """n_step as an int, or ValueError: an integer in 1..NSTEP_MAX, at most
    replay_buffer_size (a window never outgrows the deque it feeds)."""
    if isinstance(n_step, bool) or not isinstance(n_step, (int, np.integer)):
        raise ValueError(f"n_step must be an integer in 1..{NSTEP_MAX}, got {n_step!r}")
    n = int(n_step)
    if not 1 <= n <= NSTEP_MAX:
        raise ValueError(f"n_step must be in 1..{NSTEP_MAX}, got {n_step!r}")
    if n > int(replay_buffer_size):
        raise ValueError(f"n_step = {n} exceeds replay_buffer_size = {replay_buffer_size}")
    return n


def nstep_gamma(gamma, n_step):
    """The bootstrap discount of an n-step transition, gamma^n as 1.0
    multiplied n times by the Python float (n = 1: gamma exactly).  The learn
    receives float32 of it in place of gamma (dqn_agent.py:347); a window cut
    short by an episode end stores d = 1, which masks the bootstrap."""
    G = 1.0
    for _ in range(int(n_step)):
        G = G * float(gamma)
    return G


def sweep_variants(cfg):
    """The variants of cfg.sweep: a list of {learning_rate, gamma, tau} dicts,
    the grid product of the swept keys' lists in key insertion order (last key
    fastest); a key absent from the sweep keeps cfg's scalar.  No sweep: the
    one variant of the scalar config.  ValueError on an unknown key, an empty
    list, a non-finite value, learning_rate <= 0, gamma outside [0, 1], tau
    outside (0, 1] (hard-only and soft nets cannot share a launch, so a tau
    sweep cannot include 0) or a sweep over shared parameters (one net has one
    set of hyperparameters)."""
    base = {k: float(getattr(cfg, k)) for k in SWEEP_KEYS}
    sweep = cfg.sweep
    if sweep is None:
        return [base]
    if not isinstance(sweep, dict):
        raise ValueError(f"sweep must be a dict of lists, got {type(sweep).__name__}")
    if cfg.shared_params:
        raise ValueError("sweep needs independent networks: shared_params trains one net, "
                         "which has one set of hyperparameters")
    lists = []
    for k, vals in sweep.items():
        if k not in SWEEP_KEYS:
            raise ValueError(f"sweep key {k!r}: only {', '.join(SWEEP_KEYS)} can be swept")
        try:
            vals = [float(v) for v in vals]
        except (TypeError, ValueError):
            raise ValueError(f"sweep[{k!r}] must be a list of numbers, got {vals!r}") from None
        if not vals:
            raise ValueError(f"sweep[{k!r}] is empty")
        for v in vals:
            ok = math.isfinite(v) and (v > 0.0 if k == "learning_rate" else
                                       0.0 <= v <= 1.0 if k == "gamma" else 0.0 < v <= 1.0)
            if not ok:
                rng = {"learning_rate": "> 0", "gamma": "in [0, 1]", "tau": "in (0, 1]"}[k]
                raise ValueError(f"sweep[{k!r}]: {v!r} must be finite and {rng}")
        lists.append(vals)
    return [dict(base, **dict(zip(sweep, combo))) for combo in itertools.product(*lists)]


PBT_KEYS = ("interval", "truncation", "perturb", "bounds", "seed")
PBT_PERTURB = {"learning_rate": [0.8, 1.25]}
PBT_BOUNDS = {"learning_rate": [1e-6, 1e-1], "gamma": [0.5, 0.9999], "tau": [1e-4, 1.0]}


def normalize_pbt(pbt):
    """AgentConfig.pbt with its defaults filled in, or None: {interval,
    truncation, perturb {key: [factors]}, bounds {key: [lo, hi]} for every
    sweep key, seed}, the two inner dicts in SWEEP_KEYS order.  ValueError on
    an unknown key, a missing or non-positive interval, a truncation that is
    not a finite number, a perturb / bounds key that is not a sweep key, an
    empty factor list, a factor that is not finite and > 0, a bound that is not
    a finite [lo, hi] with lo <= hi, or a negative seed."""
    if pbt is None:
        return None
    if not isinstance(pbt, dict):
        raise ValueError(f"pbt must be a dict, got {type(pbt).__name__}")
    for k in pbt:
        if k not in PBT_KEYS:
            raise ValueError(f"pbt key {k!r}: only {', '.join(PBT_KEYS)} are known")

    def integer(name, lo):
        v = pbt.get(name)
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or int(v) < lo:
            raise ValueError(f"pbt[{name!r}] must be an integer >= {lo}, got {v!r}")
        return int(v)
    if "interval" not in pbt:
        raise ValueError("pbt needs 'interval' (trainer steps between rounds)")
    out = {"interval": integer("interval", 1)}
    try:
        out["truncation"] = float(pbt.get("truncation", 0.25))
    except (TypeError, ValueError):
        raise ValueError(f"pbt['truncation'] must be a number, got {pbt['truncation']!r}") from None
    if not math.isfinite(out["truncation"]):
        raise ValueError(f"pbt['truncation'] must be finite, got {pbt['truncation']!r}")
    for name, default in (("perturb", PBT_PERTURB), ("bounds", PBT_BOUNDS)):
        given = pbt.get(name, default)
        if not isinstance(given, dict):
            raise ValueError(f"pbt[{name!r}] must be a dict of lists, got {given!r}")
        for k in given:
            if k not in SWEEP_KEYS:
                raise ValueError(f"pbt[{name!r}] key {k!r}: only {', '.join(SWEEP_KEYS)}")
        lists = {}
        for k in SWEEP_KEYS:
            if k not in given and name == "perturb":
                continue
            try:
                vals = [float(v) for v in given.get(k, PBT_BOUNDS[k])]
            except (TypeError, ValueError):
                raise ValueError(f"pbt[{name!r}][{k!r}] must be a list of numbers, "
                                 f"got {given[k]!r}") from None
            if not all(math.isfinite(v) for v in vals):
                raise ValueError(f"pbt[{name!r}][{k!r}]: {vals!r} must be finite")
            if name == "perturb" and (not vals or min(vals) <= 0.0):
                raise ValueError(f"pbt['perturb'][{k!r}]: {vals!r} must be a non-empty list of "
                                 "factors > 0")
            if name == "bounds" and (len(vals) != 2 or vals[0] > vals[1]):
                raise ValueError(f"pbt['bounds'][{k!r}]: {vals!r} must be [lo, hi] with lo <= hi")
            lists[k] = vals
        out[name] = lists
    out["seed"] = integer("seed", 0) if "seed" in pbt else 0
    return out


def pbt_truncated(truncation, num_envs):
    """n = floor(truncation * E), the replicas replaced per round."""
    return int(math.floor(float(truncation) * int(num_envs)))


def check_pbt(cfg, num_envs):
    """normalize_pbt(cfg.pbt) checked against the run, plus "n" (the replicas
    replaced per round), or None.  ValueError (before any device work) when
    n < 1 or 2 n > E (winners and losers must be disjoint: that is what makes
    the in-place exchange free of races), with shared_params (one net has no
    population), or when tau is perturbed while the run's tau is 0 (hard-only
    and soft nets cannot share a launch)."""
    pbt = normalize_pbt(cfg.pbt)
    if pbt is None:
        return None
    if cfg.shared_params:
        raise ValueError("pbt needs independent networks: shared_params trains one net, "
                         "which has no population")
    n = pbt_truncated(pbt["truncation"], num_envs)
    if n < 1 or 2 * n > int(num_envs):
        raise ValueError(f"pbt: truncation {pbt['truncation']!r} of {num_envs} replicas replaces "
                         f"n = {n}; need 1 <= n and 2 n <= E")
    if "tau" in pbt["perturb"] and float(cfg.tau) == 0.0 and "tau" not in (cfg.sweep or {}):
        raise ValueError("pbt perturbs tau but the run's tau is 0 (hard target updates only)")
    return dict(pbt, n=n)


def pbt_config_list(pbt):
    """normalize_pbt(pbt) as nested lists of plain values, key order fixed: what
    a checkpoint stores and compares (None stays None)."""
    p = normalize_pbt(pbt)
    if p is None:
        return None
    return [["interval", p["interval"]], ["truncation", p["truncation"]],
            ["perturb", [[k, list(v)] for k, v in p["perturb"].items()]],
            ["bounds", [[k, list(v)] for k, v in p["bounds"].items()]], ["seed", p["seed"]]]


def variant_assignment(n_variants, num_envs, env_offset=0):
    """int64 [num_envs]: replica with global index g = env_offset + e runs
    variant g % G, so a rank of a sharded run holds the variants a
    single-process run gives those replicas."""
    return (np.arange(num_envs, dtype=np.int64) + int(env_offset)) % int(n_variants)


def keras_initial_weights(rng, hidden, n_agents):
    """HeNormal (truncated at 2 sigma, stddev sqrt(2/fan_in)/0.8796) for the ReLU
    layers, GlorotUniform for the output layer, zero biases (dqn_agent.py:160-181).
    TF's RNG stream is not reproducible here, so initial weights are an input."""
    H = hidden

    def he(fi, fo):
        std = np.sqrt(2.0 / fi) / 0.87962566103423978
        w = rng.normal(0, std, size=(n_agents, fi, fo))
        bad = np.abs(w) > 2 * std
        while bad.any():
            w[bad] = rng.normal(0, std, size=int(bad.sum()))
            bad = np.abs(w) > 2 * std
        return w.reshape(n_agents, -1)

    lim = np.sqrt(6.0 / (H + N_ACTIONS))
    parts = [he(D_IN, H), np.zeros((n_agents, H)), he(H, H), np.zeros((n_agents, H)),
             rng.uniform(-lim, lim, size=(n_agents, H * N_ACTIONS)), np.zeros((n_agents, N_ACTIONS))]
    return np.concatenate(parts, axis=1).astype(np.float32)


def initial_weights(seed, env_seeds, n_agents, hidden, shared=False):
    """Initial weights [NW, P_keras] for the agents of the replicas whose env
    seeds are `env_seeds` (n_agents per replica).  Each replica's agents draw
    from their own generator, keyed on (seed, env seed), so a rank that owns
    replicas [r*E, (r+1)*E) builds exactly the weights those replicas get in a
    single-process run (shards are independent).  The shared net
    (C5) draws from `seed` alone, identical on every rank."""
    if shared:
        return keras_initial_weights(np.random.RandomState(seed & 0xFFFFFFFF), hidden, 1)
    return np.concatenate([
        keras_initial_weights(np.random.RandomState([seed & 0xFFFFFFFF, int(s) & 0xFFFFFFFF,
                                                     0x5EED]), hidden, n_agents)
        for s in env_seeds])


@dataclass
class AgentConfig:
    """Keys of config/agent_config.yaml; defaults are the values train.py uses
    (train.py:110-121), not the YAML file's (A-17)."""
    learning_rate: float = 0.001
    gamma: float = 0.99
    epsilon_start: float = 1.0
    epsilon_min: float = 0.01
    epsilon_decay_steps: int = 200000
    replay_buffer_size: int = 10000
    batch_size: int = 128
    target_update_frequency: int = 500
    nn_layers: List[int] = field(default_factory=lambda: [128, 128])
    # build-only knobs (additive)
    precision: str = "fp32"          # "fp32" | "fp16" (mixed, the reference's policy) | "bf16"
    loss: str = "mse"                # "mse" (dqn_agent.py:352) | "huber" (experimental/agent.py:99)
    count_env_steps: bool = False    # True fixes A-1 (epsilon decays); False = reference
    seed: int = 0
    # C5 (not in the reference): ONE network shared by every agent,
    # trained on the mean of the per-agent losses; gradients all-reduced over
    # RCCL across ranks.  Requires precision "fp16" and nn_layers [128, 128].
    shared_params: bool = False
    # replay row storage: "int8" (batched path, exact for this env, others
    # raise) | "f32" (any observation value, as dqn_agent.py:39-56 stores it;
    # the per-agent drop-in DQNAgent uses it)
    replay_rows: str = "int8"
    # physical ring slots beyond replay_buffer_size (kernels.ReplayRing): with
    # s spare slots the trainer's "env" schedule lets its side stream run up to
    # s env steps ahead of the learn, which marks every s-th learn for it
    ring_spare: int = 16
    # soft (Polyak) target updates, the reference's update_target_network_soft
    # (dqn_agent.py:372-373, 389-399; docs/improvements.md item 9): after every
    # learn target <- tau * online + (1 - tau) * target, fused into the learn
    # kernels.  0 = off (the reference's training path).  The hard sync of
    # target_update_frequency still runs when due and wins on that learn;
    # target_update_frequency 0 = never hard-sync.
    tau: float = 0.0
    # hyperparameter sweep across env replicas (sweep_variants): e.g.
    # {"learning_rate": [1e-4, 3e-4, 1e-3], "gamma": [0.95, 0.99]} is a grid of
    # G = 6 variants (key order, last key fastest); env replica g trains all its
    # agents with variant g % G.  Keys: learning_rate, gamma, tau; an absent key
    # keeps the scalar above.  None = every replica runs the scalar config.
    sweep: Optional[dict] = None
    # n-step returns (docs/improvements.md item 7): every stored transition is
    # (s_i, a_i, r_i + gamma r_{i+1} + ... , s'_{i+m-1}, d_{i+m-1}) over a window
    # of up to n_step raw transitions, cut at an episode end, and the learn
    # bootstraps with gamma^n_step.  The raw transitions pass through a staging
    # ring of n_step slots (BatchedDQN.stage), so the transition that starts at
    # raw store i is committed at raw store i + n_step - 1 and the last
    # n_step - 1 raw transitions of a run are never committed.  1..32 and at
    # most replay_buffer_size; 1 = the reference's one-step transitions (no
    # staging ring, no extra launch).  Not a sweep key.
    n_step: int = 1
    # population-based training across the env replicas (normalize_pbt): every
    # `interval` trainer steps the n = floor(truncation * E) replicas of lowest
    # fitness (the reward summed over the window) take over the nets, Adam
    # slots and hyperparameters of the n best, and each copied value of a
    # `perturb` key is multiplied by a factor drawn from its list and clipped
    # to `bounds`.  {"interval": 500} alone: truncation 0.25, perturb
    # {"learning_rate": [0.8, 1.25]}, seed 0.  A perturbed key is per agent like
    # a swept one (starting from the scalar when not swept).  None = off:
    # nothing is allocated or launched.
    pbt: Optional[dict] = None
    # gradient clipping by global norm, Keras's Adam(global_clipnorm=...) (one
    # keyword at dqn_agent.py:140, which the reference does not set): before
    # the Adam step every agent's gradient g is scaled by about
    # min(1, global_clipnorm / ||g||) over all of its parameters
    # (include/dmdqn.h dmdqn_adam_agents_clip has the exact rule), and the norm
    # is kept (BatchedDQN.grad_norm, learn_metrics).  0 = off: nothing is
    # allocated or launched.  On, every learn runs as the split learn
    # (set_split_learn) with the clipping Adam launch, alone (never paired):
    # fp16 / bf16 independent networks on int8 replay rows.  Not a sweep key.
    global_clipnorm: float = 0.0
    # network health probe (docs/improvements.md item 2, "Tensorboard
    # activation checks"): a Trainer probes every agent's online net after each
    # health_every-th learn (BatchedDQN.probe_health: dead and active ReLU
    # units, non-finite pre-activations, per-variable weight norms and
    # update-to-weight ratios) and learn_metrics() gains a "health" block.  The
    # probe only reads: training state is the same bits with and without it.
    # 0 = off: nothing is allocated or launched.  fp16 / bf16 independent
    # 128-wide networks on int8 replay rows.  Not a sweep key.
    health_every: int = 0
    # dead-unit recycling, ReDo with tau = 0 (Sokar et al. 2023; also
    # docs/improvements.md item 3, "improve weight inits"): after each
    # redo_every-th learn a Trainer probes every agent's online net
    # (BatchedDQN.redo) and a hidden unit that was dead on redo_patience such
    # probes in a row gets fresh HeUniform incoming weights, zero outgoing
    # weights and zero Adam moments (include/dmdqn.h dmdqn_redo): the network's
    # function on the probed batch is unchanged.  learn_metrics() gains a
    # "redo" block.  0 = off: nothing is allocated or launched.  The probe's
    # limits: fp16 / bf16 independent 128-wide networks on int8 replay rows.
    # Not sweep keys.
    redo_every: int = 0
    redo_patience: int = 1
    # rule-based behaviour policy (include/dmdqn.h dmdqn_act_rule): while it is
    # active -- for the first behavior_steps env steps, or the whole run with
    # behavior_steps 0 -- act_inputs() hands the act the rule's actions
    # ("longest_queue" / "max_pressure", from the current observation) as its
    # greedy actions and behavior_eps as its epsilon: every agent draws rand()
    # as ever and takes a uniform action below behavior_eps, the rule's
    # otherwise.  The replay rings then fill with a controller's transitions
    # instead of uniformly random ones (A-1: epsilon stays 1.0 on the
    # reference training path).  Afterwards everything is as without it.
    # learn_metrics() gains a "behavior" block.  None = off: nothing is
    # allocated or launched.  Runs with every net configuration (the rule needs
    # no net); under a Trainer with overlap "none" or "env".  Not sweep keys.
    behavior: Optional[str] = None
    behavior_steps: int = 0
    behavior_eps: float = 0.1

    @classmethod
    def from_dict(cls, d):
        known = {k: v for k, v in d.items() if k in cls.__dataclass_fields__}
        return cls(**known)


class LearnToken:
    """What learn_begin() fixes of one learn, so that its launch may follow
    later (the trainer's paired learns, learn_pair_range): the index and loss /
    metrics buffers of the agent's rotations, the ring window, the Keras Adam
    constants and factors of this learn's step count, and whether it -- or the
    learn after it -- is a hard target sync."""
    __slots__ = ("idx", "loss", "qstats", "adam", "factors", "sync", "next_sync", "start", "n",
                 "gnorm")

    def __init__(self, **kw):
        for k, v in kw.items():
            setattr(self, k, v)


def _soft_after_shared(agent, sync):
    """The shared net's soft target update: one more launch on the one net
    after its Adam step (every rank holds the same net and takes the same
    step), unless this learn hard-synced (dqn_agent.py:372-377)."""
    if agent.cfg.tau > 0 and not sync:
        agent.update_target_network_soft()


class BatchedDQN:
    """E*A independent DQN agents (agent index = env * A + junction).

    variant_of_env ([E] indices into sweep_variants(cfg)) says which variant of
    cfg.sweep each replica trains with.  Any assignment is allowed; the
    default is e % G, and a Trainer passes (env_offset + e) % G
    (variant_assignment).  A checkpoint stores the assignment beside the
    sweep and a resume under another one is refused."""

    # rotating per-step output buffers (loss, qstats, actions, idx; see
    # __init__): at least 3, and ring_spare + 2 -- under trainer overlap "env"
    # the side stream runs up to ring_spare steps ahead of the learn stream, so
    # it writes the buffers of step t + ring_spare + 1 while the learn of step
    # t and then the caller's reads of step t's outputs may still be queued
    OUT_BUFS = 3

    def __init__(self, num_envs, n_agents, cfg: AgentConfig = None, device="cuda",
                 env_seeds=None, init_weights=None, streams=None, variant_of_env=None,
                 env_offset=0):
        self.cfg = cfg = cfg or AgentConfig()
        # the sweep's variants and each replica's (refusals before any device work)
        self.variants = sweep_variants(cfg)
        # population-based training: the checked config (+ "n"), or None
        self.pbt = check_pbt(cfg, num_envs)
        self.env_offset = int(env_offset)  # global index of replica 0 (the explore draws' key)
        self.n_step = check_n_step(cfg.n_step, cfg.replay_buffer_size)
        # what the learn takes for gamma: gamma^n_step (n_step 1: gamma itself)
        self.gamma_n = nstep_gamma(cfg.gamma, self.n_step)
        if variant_of_env is None:
            variant_of_env = variant_assignment(len(self.variants), num_envs)
        voe = np.asarray(variant_of_env, dtype=np.int64).reshape(-1)
        if voe.shape != (num_envs,) or (voe < 0).any() or (voe >= len(self.variants)).any():
            raise ValueError(f"variant_of_env must hold {num_envs} indices in "
                             f"[0, {len(self.variants)})")
        self._ops = _ops()
        H = cfg.nn_layers[0]
        if len(cfg.nn_layers) != 2 or cfg.nn_layers[1] != H or H not in (64, 128):
            raise ValueError("the fused learn kernel supports nn_layers [64,64] or [128,128]")
        if cfg.batch_size != 128:
            raise ValueError("the fused learn kernel is built for batch_size 128")
        if cfg.precision not in PRECISIONS:
            raise ValueError(f"precision must be one of {list(PRECISIONS)}")
        if cfg.loss not in LOSSES:
            raise ValueError(f"loss must be one of {list(LOSSES)}")
        check_tau(cfg.tau)
        # gradient clipping rides on the split learn: its limits are refused
        # here, before anything is allocated
        self.clipnorm = check_clipnorm(cfg.global_clipnorm)
        if self.clipnorm > 0 and (cfg.precision not in H16_DTYPES or cfg.shared_params
                                  or cfg.replay_rows != "int8"):
            raise ValueError("global_clipnorm does not run with precision 'fp32', shared_params "
                             "or float replay rows (replay_rows 'f32'): fp16 / bf16 independent "
                             "networks on int8 replay rows are supported")
        # the health probe runs the 16-bit learn's forward: the same limits,
        # refused here as well
        self.health_every = check_health_every(cfg.health_every)
        if self.health_every > 0 and not self._probe_supported(cfg):
            raise ValueError("health_every: " + self._PROBE_LIMITS)
        self.health = None      # probe_health()'s outputs (device tensors), None before it ran
        # dead-unit recycling acts on the probe's dead mask: the probe's limits
        self.redo_every, self.redo_patience = check_redo(cfg.redo_every, cfg.redo_patience)
        if self.redo_every > 0 and not self._probe_supported(cfg):
            raise ValueError("redo_every: " + self._PROBE_LIMITS)
        # redo()'s state (device tensors; allocated with redo_every > 0 or by the
        # first call): every unit's streak of dead probes, the last call's fired
        # mask and counts, the running totals; and the number of calls
        self.redo_streak = self.redo_last = self.redo_total = None
        self.redo_rounds = 0
        # rule-based behaviour policy: the checked config and the env steps
        # taken so far (remember() / remembered() count them; checkpointed)
        self.behavior, self.behavior_steps, self.behavior_eps = check_behavior(
            cfg.behavior, cfg.behavior_steps, cfg.behavior_eps)
        self.behavior_step_count = 0
        if int(cfg.target_update_frequency) < 0:
            raise ValueError("target_update_frequency must be >= 0 (0 = never hard-sync)")
        if cfg.shared_params and (cfg.precision != "fp16" or H != 128):
            raise ValueError("shared_params needs precision 'fp16' and nn_layers [128, 128]")
        self.device = dev = torch.device(device)
        self.E, self.A = num_envs, n_agents
        self.NA = NA = num_envs * n_agents
        self.shared = cfg.shared_params
        self.NW = NW = 1 if self.shared else NA   # parameter sets
        self.H, self.P = H, n_params(H)
        seeds = (np.arange(num_envs, dtype=np.int64) + cfg.seed if env_seeds is None
                 else np.asarray(env_seeds))
        if init_weights is None:
            init_weights = initial_weights(cfg.seed, seeds, n_agents, H, self.shared)
        init = np.asarray(init_weights, dtype=np.float32).reshape(NW, -1)
        if init.shape[1] == n_params_keras(H):
            init = keras_to_kernel(init, H)
        w = torch.as_tensor(init.reshape(NW, self.P))
        self.params = w.to(dev).contiguous()
        self.target = self.params.clone()
        # fp16 / bf16 paths: the target forward reads a 16-bit copy (padded row
        # stride Ph) in the MFMA operand type
        self.Ph = (self.P + 7) // 8 * 8
        self.target_h = self.params_h = None
        h16 = H16_DTYPES.get(cfg.precision)
        if h16 is not None:
            # f16 copies the forwards read (Keras casts the f32 variables to f16);
            # the online copy only for the shared net, whose Adam is a separate
            # pass (fused into the per-agent learn, the extra stores cost more
            # than the halved fragment reads save)
            self.target_h = torch.zeros((NW, self.Ph), dtype=h16, device=dev)
            self._refresh_target_h()
            if self.shared:
                self.params_h = torch.zeros((NW, self.Ph), dtype=h16, device=dev)
                self._refresh_params_h()
        if self.shared:
            # one partial gradient per persistent workgroup (one per CU)
            n_cu = torch.cuda.get_device_properties(dev).multi_processor_count
            self.n_slabs = max(1, min(NA, n_cu))
            self.slab = torch.empty((self.n_slabs, self.P), dtype=torch.float32, device=dev)
            self.grad = torch.zeros(self.P, dtype=torch.float32, device=dev)
            # each batch row's TD target + action between the shared learn's two passes
            self.shared_work = torch.empty(NA * cfg.batch_size * 5, dtype=torch.uint8, device=dev)
        self.adam_m = torch.zeros_like(self.params)
        self.adam_v = torch.zeros_like(self.params)
        if cfg.replay_rows not in ("int8", "f32"):
            raise ValueError("replay_rows must be 'int8' or 'f32'")
        if self.shared and cfg.replay_rows != "int8":
            raise ValueError("the shared-network learn reads int8 replay rows only")
        self.ring = K.ReplayRing(NA, cfg.replay_buffer_size, device=dev, row_format=cfg.replay_rows,
                                 spare=cfg.ring_spare)
        # n_step > 1: the last n_step raw transitions of every agent, a replay
        # ring of n_step slots that remember() / a fused env step write instead
        # of self.ring; from the n_step-th raw store on, each raw store is
        # followed by one commit of the window's oldest start into self.ring
        # (commit_nstep).  store_ring is the ring raw stores go to.  The range
        # flag of the staging ring's int8 stores is the main ring's (one pinned
        # word), so ring.poll() / ring.check() cover both.
        self.stage = None
        if self.n_step > 1:
            self.stage = K.ReplayRing(NA, self.n_step - 1, device=dev, spare=1,
                                      row_format=cfg.replay_rows)
            self.stage.err = self.ring.err
        self.store_ring = self.ring if self.stage is None else self.stage
        self.nstep_gamma_a = None  # f64 [NA]: the commit's per-agent gamma (a gamma sweep)
        self.OUT_BUFS = max(BatchedDQN.OUT_BUFS, self.ring.spare + 2)
        self._xs = self._xn = None  # float rows: the learn's pre-gathered batch
        if streams is not None:
            # shared (np_state, py_state) device streams, e.g. the process-global
            # ones behind the per-agent DQNAgent surface
            self.np_state, self.py_state = streams
        else:
            self.np_state = K.seed_streams(seeds, "np", dev)
            self.py_state = K.seed_streams(seeds, "py", dev)
        # rotating index buffers: presample() may draw the next learn's batch
        # (on another stream) while the current learn still reads its own, and
        # a caller's read of step t's indices on its stream (queued behind
        # learn t) must not meet the draws of step t+2 (the side stream of
        # trainer overlap "env" waits only for learn t): OUT_BUFS of them
        self._idx_bufs = [torch.empty((NA, cfg.batch_size), dtype=torch.int32, device=dev)
                          for _ in range(self.OUT_BUFS)]
        self._idx_i = 0
        self.idx = self._idx_bufs[0]
        self._presampled = None  # (n, buffer) drawn ahead by presample()
        # per-learn outputs rotate over OUT_BUFS buffers (learn k writes buffer
        # k % OUT_BUFS): under trainer overlap "env" with side_learn, the side
        # stream's learn of step t+1 may run before the caller's main-stream
        # read of step t's loss / stats, and the side stream is ordered only
        # after learn t-1 -- so learn t+1 and t+2 must write other buffers
        # than the one step t's reader holds
        self._loss_bufs = [torch.zeros(NA, dtype=torch.float32, device=dev)
                           for _ in range(self.OUT_BUFS)]
        self._qstats_bufs = [torch.zeros((NA, 6), dtype=torch.float32, device=dev)
                             for _ in range(self.OUT_BUFS)]
        self.loss, self.qstats = self._loss_bufs[0], self._qstats_bufs[0]
        # global_clipnorm: every agent's gradient norm before clipping, f32 [NA],
        # rotating with the loss; None without clipping
        self._gnorm_bufs = self.grad_norm = None
        if self.clipnorm > 0:
            self._gnorm_bufs = [torch.zeros(NA, dtype=torch.float32, device=dev)
                                for _ in range(self.OUT_BUFS)]
            self.grad_norm = self._gnorm_bufs[0]
        # rotating action buffers: a caller may still read step t's actions on
        # its stream while the trainer's side stream writes steps t+1 and t+2
        # (overlap "env": the side stream waits only for learn t, before which
        # the caller's read of step t is queued) -- OUT_BUFS of them
        self._act_bufs = [torch.empty((num_envs, n_agents), dtype=torch.int32, device=dev)
                          for _ in range(self.OUT_BUFS)]
        self._act_i = 0
        self.actions = self._act_bufs[0]
        self.greedy = torch.empty((num_envs, n_agents), dtype=torch.int32, device=dev)
        self._done_flags = [torch.full((NA,), v, dtype=torch.uint8, device=dev) for v in (0, 1)]
        self.global_step_count = 0
        self.learn_step_counter = 0
        self.epsilon = cfg.epsilon_start
        self.learn_launches = 0
        self.pair_launches = 0  # learn_pair_range launches (two of the learns begun each)
        self._last_tok = None
        self.learn_hook = None  # optional callable(before: bool), e.g. HIP event timing
        self.stamps = None      # optional int64 [NA, 16] device tensor: phase timestamps
        self.rn_out = None      # optional f32 [NA, batch] device tensor: the z-scored rewards
        self._split_grad = None  # [NA, P] f32 scratch of the split learn (set_split_learn)
        # the shared net's learns by launch sequence (tests assert which ran):
        # "adam_slabs" = one rank's fused slab reduction + Adam; "allreduce" =
        # k_reduce_slabs -> all-reduce over ranks -> k_adam(gscale = 1/world)
        self.shared_paths = {"adam_slabs": 0, "allreduce": 0}
        # per-agent hyperparameters of a sweep: f32 [NA] device arrays (agent =
        # env * A + junction; every agent of a replica has its variant), built
        # once; None for a key that is not swept (the launch scalar is used)
        self.variant_of_env = torch.as_tensor(voe)
        self._variant_of_agent = self.variant_of_env.repeat_interleave(n_agents).to(dev)
        self.hp_lr = self.hp_gamma = self.hp_tau = self.hp_omt = None
        # (a key population-based training perturbs is per agent like a swept
        # one; not swept, every variant holds the scalar it starts from)
        swept = set(cfg.sweep or {}) | set(self.pbt["perturb"] if self.pbt else ())
        per_agent = np.repeat(voe, n_agents)

        def column(values):
            return torch.as_tensor(np.asarray(values, dtype=np.float32)[per_agent]).to(dev)
        if "learning_rate" in swept:
            self.hp_lr = column([v["learning_rate"] for v in self.variants])
        if "gamma" in swept:
            # float32(gamma_v^n_step) for the learn; the n-step commit forms its
            # returns with the variants' Python floats, in f64
            self.hp_gamma = column([nstep_gamma(v["gamma"], self.n_step) for v in self.variants])
            if self.stage is not None:
                g64 = np.asarray([v["gamma"] for v in self.variants], dtype=np.float64)
                self.nstep_gamma_a = torch.as_tensor(g64[per_agent]).to(dev)
        if "tau" in swept:
            consts = [soft_update_consts(v["tau"]) for v in self.variants]
            self.hp_tau = column([c[0] for c in consts])
            self.hp_omt = column([c[1] for c in consts])
        self._last_factors = (1.0, 1.0)
        # population-based training: the master values of every per-agent key
        # (host f64 [E], SWEEP_KEYS order), the window's fitness (device f64
        # [E]) and the index of the next round; nothing without cfg.pbt
        self.pbt_values = self.fitness = None
        self.pbt_round = 0
        if self.pbt is not None:
            self.pbt_values = {k: np.asarray([self.variants[i][k] for i in voe], dtype=np.float64)
                               for k in SWEEP_KEYS if k in swept}
            self.fitness = torch.zeros(num_envs, dtype=torch.float64, device=dev)
            self._pbt_rank = torch.empty(num_envs, dtype=torch.int32, device=dev)
            self._pbt_src = torch.empty(num_envs, dtype=torch.int32, device=dev)
        if self.clipnorm > 0:  # the clipping Adam launch is the split learn's second one
            self.set_split_learn(True)
        if self.redo_every > 0:
            self._redo_alloc()

    @property
    def swept(self):
        """Whether any hyperparameter is per agent (the _hp entry points run)."""
        return self.hp_lr is not None or self.hp_gamma is not None or self.hp_tau is not None

    def set_split_learn(self, on=True):
        """Run each independent-agent learn as two launches (dmdqn_learn_grad,
        dmdqn_adam_agents): bit-identical to the fused kernel, 4 more bytes of
        HBM traffic per parameter each way, but its bandwidth-bound Adam half
        can share the chip with the next step's act / sim / observe (trainer
        overlap "full"), which the fused kernel's LDS-heavy workgroups leave no
        room for.  fp16 / bf16, independent networks only."""
        if on:
            if self.shared or self.cfg.precision not in H16_DTYPES or self.ring.row_format != "int8":
                raise ValueError("the split learn is for independent fp16 / bf16 networks "
                                 "on int8 replay rows")
            if self._split_grad is None:
                self._split_grad = torch.empty((self.NA, self.P), dtype=torch.float32,
                                               device=self.device)
        else:
            if self.clipnorm > 0:
                raise ValueError("global_clipnorm runs as the split learn: it cannot be turned off")
            self._split_grad = None

    @property
    def split_learn(self):
        return self._split_grad is not None

    # -------------------------------------------------------------- health probe
    _PROBE_LIMITS = ("the network health probe does not run with precision 'fp32', "
                     "shared_params, nn_layers other than [128, 128] or float replay rows "
                     "(replay_rows 'f32'): fp16 / bf16 independent 128-wide networks on int8 "
                     "replay rows are supported")

    @staticmethod
    def _probe_supported(cfg):
        return (cfg.precision in H16_DTYPES and not cfg.shared_params
                and list(cfg.nn_layers) == [128, 128] and cfg.replay_rows == "int8")

    def probe_health(self, idx=None):
        """Probe every agent's online net on the current stream (dmdqn_net_probe
        and dmdqn_layer_norms; they only read): the forward of the batch at deque
        positions idx [NA, 128] -- default: the last learn's draws, in that
        learn's ring window -- reduced to counts / stats / dead_mask, and the
        per-variable sums of squares of params (w2), of the Adam step m /
        (sqrt(v) + eps) (u2) and, when the split learn's gradient buffer exists,
        of the last gradient (g2, else None).  Fills and returns self.health, a
        dict of device tensors: those, alpha f32 [NA] (the Adam factor of the
        learn just done, per agent under a learning-rate sweep; 0 before the
        first learn) and learn_step (int64 scalar); beside them "idx" and
        "start", the index tensor and ring start the probe read.  The
        update-to-weight ratio of a variable is alpha * sqrt(u2) / sqrt(w2)."""
        if not self._probe_supported(self.cfg):
            raise ValueError("probe_health: " + self._PROBE_LIMITS)
        tok = self._last_tok
        if idx is None:
            if tok is None:
                raise RuntimeError("probe_health: no learn has drawn a batch yet (pass idx)")
            idx, start = tok.idx, tok.start
        else:
            start = self.ring.start
        NA, dev = self.NA, self.device
        h = self.health
        if h is None:
            h = self.health = {
                "counts": torch.zeros((NA, K.PROBE_COUNTS), dtype=torch.int32, device=dev),
                "stats": torch.zeros((NA, K.PROBE_STATS), dtype=torch.float64, device=dev),
                "dead_mask": torch.zeros((NA, 2, 4), dtype=torch.int32, device=dev),
                "w2": torch.zeros((NA, K.NORM_VARS), dtype=torch.float64, device=dev),
                "u2": torch.zeros((NA, K.NORM_VARS), dtype=torch.float64, device=dev),
                "g2": None,
                "alpha": torch.zeros(NA, dtype=torch.float32, device=dev),
                "learn_step": torch.zeros((), dtype=torch.int64, device=dev)}
        K.net_probe(self.ring.s, idx, self.params, start, self.H, PRECISIONS[self.cfg.precision],
                    h["counts"], h["stats"], h["dead_mask"])
        eps = keras_adam_consts(1, self.cfg.learning_rate)[3]
        K.layer_norms(self.params, self.H, out=h["w2"])
        K.layer_norms(self.adam_m, self.H, y=self.adam_v, eps=eps, out=h["u2"])
        if self._split_grad is not None:
            if h["g2"] is None:
                h["g2"] = torch.zeros((NA, K.NORM_VARS), dtype=torch.float64, device=dev)
            K.layer_norms(self._split_grad, self.H, out=h["g2"])
        else:
            h["g2"] = None
        if tok is None:
            h["alpha"].zero_()
        elif self.hp_lr is not None:
            # fl32(fl32(lr * s) / d): the kernels' hp_alpha, two rounded f32 ops
            s, d = tok.factors
            torch.div(self.hp_lr * float(s), float(d), out=h["alpha"])
        else:
            h["alpha"].fill_(tok.adam[0])
        h["learn_step"].fill_(self.learn_step_counter)
        h["idx"], h["start"] = idx, int(start)  # what the probe read (not outputs)
        return h

    def health_metrics(self, sel=slice(None)):
        """The "health" block of learn_metrics() from the last probe_health(),
        reduced over the agents `sel`: per hidden layer dead_frac (mean over
        agents of dead units / 128), dead_frac_max, active_frac, act_mean (the
        mean activation) and preact_absmax; q_absmax; nonfinite_agents (agents
        with a non-finite pre-activation or Q); per variable weight_norm (mean),
        update_ratio (mean and max of alpha * sqrt(u2) / sqrt(w2) over the
        agents whose variable is not all zero; None if there is none) and, with
        the split learn's gradient, grad_layer_norm (mean).  Syncs."""
        h = self.health
        cnt = h["counts"][sel].double().cpu()
        st = h["stats"][sel].cpu()
        n = float(self.cfg.batch_size * self.H)
        rec = {"learn_step": int(h["learn_step"]), "layers": [],
               "q_absmax": float(st[:, 4].max()),
               "nonfinite_agents": int((cnt[:, 4] > 0).sum())}
        for layer in range(2):
            dead = cnt[:, 2 * layer + 1] / self.H
            rec["layers"].append({
                "dead_frac": float(dead.mean()), "dead_frac_max": float(dead.max()),
                "active_frac": float((cnt[:, 2 * layer] / n).mean()),
                "act_mean": float((st[:, layer] / n).mean()),
                "preact_absmax": float(st[:, 2 + layer].max())})
        w = h["w2"][sel].sqrt().cpu()
        step = h["alpha"][sel].double().cpu()[:, None] * h["u2"][sel].sqrt().cpu()
        rec["weight_norm"] = {v: float(w[:, i].mean()) for i, v in enumerate(VARIABLES)}
        ratio = {}
        for i, v in enumerate(VARIABLES):
            ok = w[:, i] > 0
            r = step[ok, i] / w[ok, i]
            ratio[v] = ({"mean": float(r.mean()), "max": float(r.max())} if bool(ok.any())
                        else {"mean": None, "max": None})
        rec["update_ratio"] = ratio
        if h["g2"] is not None:
            g = h["g2"][sel].sqrt().cpu()
            rec["grad_layer_norm"] = {v: float(g[:, i].mean()) for i, v in enumerate(VARIABLES)}
        return rec

    # -------------------------------------------------------------- dead-unit recycling
    def _redo_alloc(self):
        if self.redo_streak is None:
            NA, dev = self.NA, self.device
            self.redo_streak = torch.zeros((NA, 2, self.H), dtype=torch.uint8, device=dev)
            self.redo_last = {
                "recycled": torch.zeros((NA, 2, 4), dtype=torch.int32, device=dev),
                "n_recycled": torch.zeros((NA, 2), dtype=torch.int32, device=dev),
                "learn_step": torch.zeros((), dtype=torch.int64, device=dev)}
            self.redo_total = torch.zeros(2, dtype=torch.int64, device=dev)

    def redo(self, idx=None):
        """Recycle dead units (ReDo, include/dmdqn.h dmdqn_redo) on the current
        stream: probe_health(idx), then every hidden unit whose bit of the
        probe's dead_mask was set on redo_patience calls in a row gets fresh
        incoming weights, zero outgoing weights and zero Adam moments, in place
        in params / adam_m / adam_v; the target net, the rings and the random
        streams are not touched.  The fresh weights are keyed by cfg.seed, the
        learn step counter and the agent's global index (env_offset + e) * A +
        j.  Updates redo_streak uint8 [NA, 2, 128], redo_last (the fired units
        of this call as "recycled" int32 [NA, 2, 4] bits, their counts
        "n_recycled" int32 [NA, 2], "learn_step"), redo_total int64 [2] and
        redo_rounds; no host synchronisation.  The caller orders it against
        other streams' use of the nets (Trainer: quiesce / join_streams).
        Returns redo_last."""
        h = self.probe_health(idx)
        self._redo_alloc()
        last = self.redo_last
        K.redo(h["dead_mask"], self.redo_streak, self.params, self.adam_m, self.adam_v, self.H,
               self.env_offset * self.A, self.cfg.seed, self.learn_step_counter,
               self.redo_patience, last["recycled"], last["n_recycled"])
        self.redo_total += last["n_recycled"].sum(0)
        last["learn_step"].fill_(self.learn_step_counter)
        self.redo_rounds += 1
        return last

    def redo_metrics(self, sel=slice(None)):
        """The "redo" block of learn_metrics(): rounds (calls of redo() so
        far), learn_step of the last one, recycled [n1, n2] (the units it
        rewrote per hidden layer, summed over the agents `sel`),
        agents_touched (how many of them had one) and recycled_total (the
        run's totals over all agents).  Syncs."""
        n = self.redo_last["n_recycled"][sel].cpu()
        return {"rounds": int(self.redo_rounds),
                "learn_step": int(self.redo_last["learn_step"]),
                "recycled": [int(x) for x in n.sum(0)],
                "recycled_total": [int(x) for x in self.redo_total.cpu()],
                "agents_touched": int((n.sum(1) > 0).sum())}

    def behavior_metrics(self):
        """The "behavior" block of learn_metrics(): the configured policy, its
        epsilon and whether the next act still takes it."""
        return {"policy": self.behavior, "eps": float(self.behavior_eps),
                "active": bool(self.behavior_active())}

    # -------------------------------------------------------------- act
    def current_epsilon(self):
        """dqn_agent.py:258-261 (global_step_count never moves on the reference
        training path, so epsilon stays 1.0 -- A-1)."""
        g = self.global_step_count
        if g < 8000:
            self.epsilon = 1.0
        elif self.epsilon > self.cfg.epsilon_min:
            self.epsilon = max(0.01, 1.0 * float(np.exp(-(g - 8000) / 16000)))
        return self.epsilon

    def act(self, obs, eps=None):
        """obs f32 [E, A, 89] -> actions int32 [E, A] (device).  eps overrides the
        schedule (evaluation, test.py:84-87)."""
        eps, greedy, out = self.act_inputs(obs, eps)
        return K.act(self.np_state, self.A, eps=eps, n_actions=N_ACTIONS, greedy=greedy, out=out)

    def behavior_active(self):
        """Whether the next training act takes the behaviour policy's actions
        (AgentConfig.behavior): fewer than behavior_steps env steps stored so
        far, or behavior_steps 0."""
        return self.behavior is not None and (
            self.behavior_steps == 0 or self.behavior_step_count < self.behavior_steps)

    def act_inputs(self, obs, eps=None):
        """What a fused env step (TrafficEnv.step_fused) needs to draw act()'s
        actions itself: (eps, greedy or None, the actions buffer to fill).
        The greedy forward (eps < 1) is launched here, as act() does.  While a
        behaviour policy is active (AgentConfig.behavior; training acts only,
        eps None) the epsilon is behavior_eps and the greedy actions are the
        rule's, from the observation alone (the grid enters only as its A
        junctions): one act_rule launch in place of the forward."""
        rule = eps is None and self.behavior_active()
        eps = self.current_epsilon() if eps is None else float(eps)
        if rule:  # (the nets' schedule above moved as without the policy)
            eps = self.behavior_eps
        greedy = None
        if eps < 1.0:
            if rule:
                K.act_rule(obs.reshape(self.E, self.A, D_IN).contiguous(), 1, self.A,
                           self.behavior, out=self.greedy)
            else:
                self._ops.q_argmax(self.params, self.H, PRECISIONS[self.cfg.precision],
                                   obs.reshape(self.NA, D_IN).contiguous(), self.greedy, None,
                                   self.shared)
            greedy = self.greedy
        self._act_i = (self._act_i + 1) % self.OUT_BUFS
        self.actions = self._act_bufs[self._act_i]
        return eps, greedy, self.actions

    def remembered(self):
        """The bookkeeping of remember() after a fused env step stored the
        transition into slot store_ring.next_slot of store_ring (self.ring, or
        the n-step staging ring)."""
        self.store_ring.advance()
        self.commit_nstep()
        self.ring.poll()
        self.behavior_step_count += 1
        if self.cfg.count_env_steps:
            self.global_step_count += 1

    def commit_nstep(self):
        """n_step > 1, after a raw store into the staging ring: once it holds
        n_step raw transitions, commit the n-step transition of the oldest one
        into self.ring on the current stream (one launch) and advance it.  Raw
        stores 0 .. n_step - 2 commit nothing.  A no-op for n_step = 1."""
        st = self.stage
        if st is not None and st.total >= st.slots:
            # after the store the oldest raw transition sits in the slot the
            # next store overwrites
            self.ring.commit_nstep(st, st.next_slot, self.cfg.gamma, self.nstep_gamma_a)

    # -------------------------------------------------------------- replay
    def remember(self, obs, actions, rewards, next_obs, done):
        """One transition per agent (ReplayBuffer.add).  obs/next_obs [E,A,89] f32,
        actions [E,A] int32, rewards [E,A] f64, done: bool or uint8 [E]."""
        NA = self.NA
        if isinstance(done, (bool, np.bool_, int)):
            d = self._done_flags[int(bool(done))]  # constant [NA] u8 (no per-step fill)
        else:
            d = done.to(torch.uint8).reshape(self.E, 1).expand(self.E, self.A).reshape(NA).contiguous()
        self.store_ring.store(obs.reshape(NA, D_IN), next_obs.reshape(NA, D_IN),
                              actions.reshape(NA), rewards.reshape(NA), d)
        self.commit_nstep()
        self.ring.poll()  # raises (one store late, no stall) on a non-int8 observation
        self.behavior_step_count += 1
        if self.cfg.count_env_steps:
            self.global_step_count += 1

    def replay(self):
        """DQNAgent.replay for every agent: returns the loss tensor [NA] (device),
        or None while the buffers hold fewer than batch_size transitions."""
        return self.learn()

    def learn(self, collect_stats=False):
        """One fused learn for every agent (None while underfilled).  With
        collect_stats, self.qstats [NA, 6] receives the batch metrics of
        dqn_agent.py:361-363 (see learn_metrics)."""
        if not self.learn_begin(collect_stats):
            return None
        return self.learn_range(0, self.NA)

    def learn_begin(self, collect_stats=False):
        """The host half of learn(): the replay draws (or the presampled ones),
        the learn counter and the Keras Adam constants of this learn.  False
        while underfilled, else the learn's LearnToken (true; it also fixes the
        ring window, for a launch that follows later: learn_pair_range, or
        learn_range(lo, hi, tok)).  The launches follow with learn_range(lo, hi) over
        agent ranges that cover [0, NA) -- independent agents, so ranges may
        run on different streams (trainer overlap "env" with side_learn)."""
        n = len(self.ring)
        if n < self.cfg.batch_size:
            return False
        cfg = self.cfg
        if self._presampled is not None:
            pn, buf = self._presampled
            self._presampled = None
            if pn != n:
                raise RuntimeError(f"presample drew for n={pn}, the ring holds {n}")
            self.idx = buf
        else:
            K.replay_sample(self.py_state, self.A, n, cfg.batch_size, out=self.idx)
        self.learn_step_counter += 1
        alpha, c1, c2, eps = keras_adam_consts(self.learn_step_counter, cfg.learning_rate)
        # a swept learning rate: the kernels form each agent's alpha from these
        s, d = keras_adam_factors(self.learn_step_counter)
        self._last_factors = (float(s), float(d))
        # target_update_frequency 0: never hard-sync (soft updates alone)
        sync = (cfg.target_update_frequency > 0
                and self.learn_step_counter % cfg.target_update_frequency == 0)
        k = self.learn_step_counter % self.OUT_BUFS
        self.loss = self._loss_bufs[k]
        if self._gnorm_bufs is not None:
            self.grad_norm = self._gnorm_bufs[k]
        qstats = None
        if collect_stats:
            # zeroed per agent range by learn_range, on the stream that launches
            # the range (the side stream's part must not wait on main)
            self.qstats = qstats = self._qstats_bufs[k]
        self._last_learn = (alpha, c1, c2, eps, sync, qstats)
        self.learn_launches += 1
        nxt = self.learn_step_counter + 1
        self._last_tok = LearnToken(
            idx=self.idx, loss=self.loss, qstats=qstats, adam=(alpha, c1, c2, eps),
            factors=self._last_factors, sync=sync, start=self.ring.start, n=self.learn_step_counter,
            gnorm=self.grad_norm,
            next_sync=cfg.target_update_frequency > 0 and nxt % cfg.target_update_frequency == 0)
        return self._last_tok

    @staticmethod
    def _slice(lo, hi):
        """t -> the rows of agents [lo, hi) of a per-agent tensor (None stays None)."""
        return lambda t: None if t is None else t[lo:hi]

    def _hp_kwargs(self, sl):
        """The per-agent hyperparameter arrays of an agent range (its _slice),
        under the operators' keyword names; None where a key is not swept."""
        return dict(lr=sl(self.hp_lr), gamma_a=sl(self.hp_gamma), tau_a=sl(self.hp_tau),
                    one_minus_tau_a=sl(self.hp_omt))

    def learn_range(self, lo, hi, tok=None):
        """Launch the learn begun by learn_begin() -- the last one, or the one
        whose token is given -- for agents [lo, hi) on the current stream (the
        whole range for the shared net).  The timing hook brackets the range
        that starts at agent 0.  Returns the learn's loss buffer."""
        tok = tok or self._last_tok
        (alpha, c1, c2, eps), sync, qstats = tok.adam, tok.sync, tok.qstats
        cfg, ring = self.cfg, self.ring
        tau_f, omt_f = soft_update_consts(cfg.tau)
        hook = self.learn_hook if lo == 0 else None
        if qstats is not None:
            qstats[lo:hi].zero_()  # the kernels accumulate into it
        if hook:
            hook(True)
        if self.shared:
            if (lo, hi) != (0, self.NA):
                raise ValueError("the shared-net learn runs over every agent at once")
            self._learn_shared(alpha, c1, c2, eps, sync, qstats)
        else:
            xs = xn = None
            if ring.row_format == "f32":  # float rows: the batch gathered in order first
                if (lo, hi) != (0, self.NA):
                    raise ValueError("float-row learns run over every agent at once")
                if self._xs is None:
                    shape = (self.NA, cfg.batch_size, K.ROW_FLOATS)
                    self._xs = torch.empty(shape, dtype=torch.float32, device=self.device)
                    self._xn = torch.empty(shape, dtype=torch.float32, device=self.device)
                ring.gather_f32(tok.idx, self._xs, self._xn)
                xs, xn = self._xs, self._xn
            sl = self._slice(lo, hi)
            args = (sl(ring.s), sl(ring.n), sl(ring.a), sl(ring.d), sl(ring.r),
                    sl(tok.idx), sl(self.params), sl(self.adam_m), sl(self.adam_v),
                    sl(self.target), sl(self.target_h), sl(tok.loss), tok.start,
                    self.H, PRECISIONS[cfg.precision], sync, self.gamma_n, alpha, c1, c2,
                    eps, LOSSES[cfg.loss], sl(qstats), sl(self.rn_out), sl(self.stamps))
            kw = dict(grad=sl(self._split_grad), xs=xs, xn=xn, tau=float(tau_f),
                      one_minus_tau=float(omt_f))
            op = "learn_step"
            if self.clipnorm > 0 or self.swept:  # the per-agent arrays and this learn's factors
                op = "learn_step_hp"
                kw.update(self._hp_kwargs(sl), adam_s=tok.factors[0], adam_d=tok.factors[1])
            if self.clipnorm > 0:  # the split learn with the clipping Adam launch
                op = "learn_step_clip"
                kw.update(clip=self.clipnorm, gnorm=sl(tok.gnorm))
            getattr(self._ops, op)(*args, **kw)
        if hook:
            hook(False)
        return tok.loss

    def learn_pair_range(self, tok0, tok1, lo, hi):
        """Launch two consecutive learns -- tok0's, then tok1's, the tokens of
        two learn_begin() calls in a row -- for agents [lo, hi) as ONE launch on
        the current stream (dmdqn_learn_pair: each agent's second learn reads
        its weights, Adam slots and target while the first one's writes are
        still on the chip).  Bit-identical to learn_range(lo, hi, tok0) followed
        by learn_range(lo, hi, tok1).  16-bit independent nets on int8 rows;
        neither learn a hard target sync, neither with metrics' buffers missing
        on one side.  Returns (tok0.loss, tok1.loss)."""
        cfg, ring = self.cfg, self.ring
        if self.shared or ring.row_format != "int8" or cfg.precision not in H16_DTYPES:
            raise ValueError("learn_pair_range: 16-bit independent nets on int8 rows only")
        if self._split_grad is not None:
            raise ValueError("learn_pair_range: not with the split learn")
        if tok0.sync or tok1.sync:
            raise ValueError("learn_pair_range: a hard target sync runs as a single learn")
        if tok1.n != tok0.n + 1 or tok0.idx is tok1.idx or tok0.loss is tok1.loss:
            raise RuntimeError("learn_pair_range: not two consecutive learns with buffers of "
                               "their own")
        tau_f, omt_f = soft_update_consts(cfg.tau)
        for t in (tok0, tok1):
            if t.qstats is not None:
                t.qstats[lo:hi].zero_()  # the kernels accumulate into it
        sl = self._slice(lo, hi)
        self._ops.learn_pair(
            sl(ring.s), sl(ring.n), sl(ring.a), sl(ring.d), sl(ring.r), sl(self.params),
            sl(self.adam_m), sl(self.adam_v), sl(self.target), sl(self.target_h), sl(tok0.idx),
            sl(tok1.idx), sl(tok0.loss), sl(tok1.loss), tok0.start, tok1.start, self.H,
            PRECISIONS[cfg.precision], self.gamma_n, list(tok0.adam), list(tok1.adam),
            LOSSES[cfg.loss], qstats0=sl(tok0.qstats), qstats1=sl(tok1.qstats),
            tau=float(tau_f), one_minus_tau=float(omt_f), **self._hp_kwargs(sl),
            factors0=list(tok0.factors), factors1=list(tok1.factors))
        if lo == 0:
            self.pair_launches += 1
        return tok0.loss, tok1.loss

    def c_learn_args(self):
        """The dmdqn_learn_args struct of the last learn (ctypes), for tests that
        call the C ABI directly; the tensors it points at belong to self."""
        alpha, c1, c2, eps, sync, qstats = self._last_learn
        cfg = self.cfg
        return CLearn(self.NA, self.ring.slots, self.ring.start, cfg.batch_size, self.H,
                      PRECISIONS[cfg.precision], int(sync), self.P,
                      *[None if t is None else t.data_ptr()
                        for t in [self.ring.s, self.ring.n, self.ring.a, self.ring.d, self.ring.r,
                                  self.idx, self.params, self.adam_m, self.adam_v, self.target,
                                  self.target_h, self.loss]],
                      np.float32(self.gamma_n), alpha, c1, c2, eps,
                      None if self.stamps is None else self.stamps.data_ptr(),
                      None if qstats is None else qstats.data_ptr(),
                      None if self.params_h is None else self.params_h.data_ptr(),
                      LOSSES[cfg.loss], None if self.rn_out is None else self.rn_out.data_ptr(),
                      int(self.ring.row_format == "f32"),
                      None if self._xs is None else self._xs.data_ptr(),
                      None if self._xn is None else self._xn.data_ptr(),
                      *soft_update_consts(cfg.tau))

    def c_learn_hparams(self):
        """The dmdqn_agent_hparams block of the last learn (ctypes), next to
        c_learn_args(): the per-agent arrays of the sweep (NULL where a key is
        not swept) and the Adam factors of that learn."""
        s, d = self._last_factors
        return CHParams(*[None if t is None else t.data_ptr()
                          for t in [self.hp_lr, self.hp_gamma, self.hp_tau, self.hp_omt]], s, d)

    def presample(self, n, lds_budget=0):
        """Draw the next learn's replay indices now (ReplayBuffer.sample,
        dqn_agent.py:59-63) for a ring of n transitions, into the index buffer
        the current learn does not read, on the current stream.  The draws
        depend only on the CPython stream and n, never on the ring contents, so
        they may run before the store that brings the ring to n (trainer
        overlap).  The next learn() must see len(ring) == n.  lds_budget:
        kernels.replay_sample's (the sampler beside the shared learn)."""
        if n < self.cfg.batch_size:
            return False
        if self._presampled is not None:
            raise RuntimeError("presample called twice before a learn")
        self._idx_i = (self._idx_i + 1) % self.OUT_BUFS
        buf = self._idx_bufs[self._idx_i]
        K.replay_sample(self.py_state, self.A, n, self.cfg.batch_size, out=buf,
                        lds_budget=lds_budget)
        self._presampled = (n, buf)
        return True

    def learn_metrics(self, by_variant=False):
        """The scalars dqn_agent.py:361-370 logs, from the last learn(collect_stats=True):
        mean over agents of q_values_mean / q_values_std (population std over
        each batch's 128x4 online Q values), the action histogram summed over
        agents, mean loss and epsilon, plus "n_step" (the config's: what the
        loss and Q values were learned under).  With global_clipnorm also
        "grad_norm_mean" / "grad_norm_max" (the agents' gradient norms before
        clipping) and "clipped_frac" (the share of agents with norm > clip);
        without it the record has no such keys.  With health_every on and after a
        probe (probe_health) also "health", the block of health_metrics().
        With redo_every on also "redo", the block of redo_metrics().
        With a behaviour policy configured also "behavior", the block of
        behavior_metrics().
        by_variant: a list with one such record
        per sweep variant, reduced over the agents of the variant's replicas,
        plus "variant" (its index), its learning_rate / gamma / tau and "envs"
        (how many replicas run it; the scalars are None for a variant without
        replicas).  Under population-based training by_variant raises
        ValueError: the variants dissolve at the first round.  Syncs."""
        if by_variant and self.pbt is not None:
            raise ValueError("learn_metrics(by_variant=True): population-based training moves "
                             "the replicas off the sweep's variants (see pbt_values)")
        qs = self.qstats.double()
        n = float(self.cfg.batch_size * N_ACTIONS)
        mean = qs[:, 0] / n
        std = (qs[:, 1] / n - mean * mean).clamp_min(0).sqrt()
        loss = self.loss.double()

        gn = None if self.grad_norm is None else self.grad_norm.double()

        def record(sel):
            rec = {"loss": float(loss[sel].mean()), "epsilon": float(self.epsilon),
                   "n_step": self.n_step, "q_values_mean": float(mean[sel].mean()),
                   "q_values_std": float(std[sel].mean()),
                   "action_distribution": qs[sel, 2:6].sum(0).round().long().tolist()}
            if gn is not None:  # global_clipnorm: the norms before clipping
                clip = float(np.float32(self.clipnorm))  # what the kernel compares with
                rec.update(grad_norm_mean=float(gn[sel].mean()), grad_norm_max=float(gn[sel].max()),
                           clipped_frac=float((gn[sel] > clip).double().mean()))
            if self.health_every > 0 and self.health is not None:
                rec["health"] = self.health_metrics(sel)
            if self.redo_every > 0:
                rec["redo"] = self.redo_metrics(sel)
            if self.behavior is not None:
                rec["behavior"] = self.behavior_metrics()
            return rec
        if not by_variant:
            return record(slice(None))
        out = []
        for i, v in enumerate(self.variants):
            envs = int((self.variant_of_env == i).sum())
            rec = dict(variant=i, **v, envs=envs)
            if envs:
                rec.update(record(self._variant_of_agent == i))
            else:
                rec.update(loss=None, epsilon=float(self.epsilon), n_step=self.n_step,
                           q_values_mean=None,
                           q_values_std=None, action_distribution=[0] * N_ACTIONS)
                if gn is not None:
                    rec.update(grad_norm_mean=None, grad_norm_max=None, clipped_frac=None)
                if self.health_every > 0 and self.health is not None:
                    rec["health"] = None
                if self.redo_every > 0:
                    rec["redo"] = None
                if self.behavior is not None:
                    rec["behavior"] = self.behavior_metrics()
            out.append(rec)
        return out

    def _learn_shared(self, alpha, c1, c2, eps, sync, qstats):
        """C5: grad = mean over this rank's agents of the per-agent gradients,
        all-reduced (sum, RCCL) across ranks, then one Adam step with 1/world."""
        import torch.distributed as dist
        ring, cfg = self.ring, self.cfg
        world = 1
        if dist.is_available() and dist.is_initialized():
            world = dist.get_world_size()
        # one rank: the slab reduction and the Adam step as one launch
        # (dmdqn_adam_slabs, the same bits); more ranks: reduce, all-reduce, Adam
        self._ops.learn_shared_grad(ring.s, ring.n, ring.a, ring.d, ring.r, self.idx, self.params,
                                    self.target, self.target_h, self.params_h, self.loss,
                                    ring.start, nstep_gamma(cfg.gamma, cfg.n_step),
                                    LOSSES[cfg.loss], qstats, self.rn_out,
                                    self.slab, self.grad if world > 1 else None, 1.0 / self.NA,
                                    work=self.shared_work)
        if world == 1:
            self.shared_paths["adam_slabs"] += 1
            self._ops.adam_slabs(self.params, self.adam_m, self.adam_v, self.target, self.target_h,
                                 self.params_h, self.slab, self.grad, 1.0 / self.NA, 1.0, alpha,
                                 c1, c2, eps, sync)
            _soft_after_shared(self, sync)
            return
        if world > 1:
            # one flat 114 KB buffer per learn, bounded (dist.BoundedAllReduce:
            # the host runs a few learns ahead; a stalled peer raises DistError)
            from . import dist as D
            if getattr(self, "_allreduce", None) is None:
                self._allreduce = D.BoundedAllReduce()
            if dist.get_backend() == "gloo" and self.grad.is_cuda:
                # gloo (several ranks on one device: the multi-process tests) reduces host memory
                g = self.grad.cpu()
                self._allreduce(g)
                self.grad.copy_(g)
            else:
                self._allreduce(self.grad)
            self.shared_paths["allreduce"] += 1
        self._ops.adam(self.params, self.adam_m, self.adam_v, self.target, self.target_h,
                       self.params_h, self.grad, 1.0 / world, alpha, c1, c2, eps, sync)
        _soft_after_shared(self, sync)

    def drain_collectives(self):
        """Wait (bounded, dist.BoundedAllReduce.drain) for the shared net's
        outstanding gradient all-reduces; a no-op without any."""
        ar = getattr(self, "_allreduce", None)
        if ar is not None:
            ar.drain()

    def _refresh_params_h(self):
        if self.params_h is not None:
            self.params_h[:, :self.P].copy_(self.params.to(self.params_h.dtype))

    def _refresh_target_h(self):
        if self.target_h is not None:
            self.target_h[:, :self.P].copy_(self.target.to(self.target_h.dtype))

    def update_target_network(self):
        """dqn_agent.py:382-387: target <- online, and the 16-bit shadow."""
        self._ops.target_sync(self.params, self.target, self.target_h,
                              PRECISIONS[self.cfg.precision])

    def update_target_network_soft(self, tau=None):
        """dqn_agent.py:389-399 outside a learn: target <- tau * online +
        (1 - tau) * target for every net (three rounded f32 ops per parameter),
        and the 16-bit shadow.  tau: cfg.tau by default (each net its own
        under a tau sweep); must be in (0, 1]."""
        if tau is None and self.hp_tau is not None:
            self._ops.target_soft_update_hp(self.params, self.target, self.target_h,
                                            PRECISIONS[self.cfg.precision], self.hp_tau,
                                            self.hp_omt)
            return
        tau_f, omt_f = soft_update_consts(
            check_tau(self.cfg.tau if tau is None else tau, allow_zero=False))
        self._ops.target_soft_update(self.params, self.target, self.target_h,
                                     PRECISIONS[self.cfg.precision], float(tau_f), float(omt_f))

    # -------------------------------------------------------------- population-based training
    def _pbt_on(self):
        if self.pbt is None:
            raise ValueError("population-based training is off (AgentConfig.pbt is None)")

    def pbt_score(self, reward):
        """fitness[e] += the step's reward f64 [E, A] summed over the junctions
        in order (dmdqn_pbt_score), on the current stream."""
        self._pbt_on()
        self._ops.pbt_score(reward, self.fitness)

    def pbt_select(self):
        """Truncation selection on the window's fitness (dmdqn_pbt_select):
        (src, rank) as host int32 [E] arrays -- replica e copies replica
        src[e] (itself for all but the n worst), rank 0 is the best.  One
        device-to-host copy; syncs the current stream."""
        self._pbt_on()
        self._ops.pbt_select(self.fitness, self.pbt["n"], self._pbt_rank, self._pbt_src)
        both = torch.stack([self._pbt_src, self._pbt_rank]).cpu().numpy()
        return both[0].copy(), both[1].copy()

    def _pbt_src_checked(self, src):
        src = np.asarray(src, dtype=np.int64).reshape(-1)
        if src.shape != (self.E,) or (src < 0).any() or (src >= self.E).any():
            raise ValueError(f"src must hold {self.E} replica indices in [0, {self.E})")
        if (src[src] != src).any():
            # a source that is itself overwritten would race its own copy
            raise ValueError("src: every source must be a fixed point (src[src[e]] == src[e])")
        return src

    def pbt_exchange(self, src):
        """Exploit: for every replica e with src[e] != e, the params, target,
        Adam m / v rows (and the 16-bit target shadow's) of its agents are
        overwritten, as bits, with those of replica src[e]'s (dmdqn_pbt_exchange,
        in place, on the current stream).  src: host [E]; every source must be
        a fixed point.  Replay rings, staging rings, RNG streams and the env
        stay each replica's own; the streaks of dead-unit recycling
        (redo_streak), which describe the nets, move with them."""
        self._pbt_on()
        src = self._pbt_src_checked(src)
        self._pbt_src.copy_(torch.as_tensor(src.astype(np.int32)))
        self._ops.pbt_exchange(self._pbt_src, self.A, self.params, self.target, self.adam_m,
                               self.adam_v, self.target_h)
        if self.redo_streak is not None:
            # the streaks of dead probes belong to the nets, not to the replica
            rows = self.redo_streak.view(self.E, -1)
            rows.copy_(rows[self._pbt_src.long()])

    def pbt_explore(self, src):
        """Explore, round self.pbt_round: every copied replica (src[e] != e)
        takes its source's value of each per-agent key, a perturbed key's
        multiplied by a factor drawn from its list and clipped to its bounds;
        the draws come from RandomState([seed, round, env_offset]), one
        randint(0, len(factors), size=E) per perturbed key in SWEEP_KEYS order
        (drawn for every replica, copied or not).  The per-agent device arrays
        are then rebuilt from pbt_values (on the current stream), so a clone
        computes what a scalar run with its new values computes."""
        self._pbt_on()
        src = self._pbt_src_checked(src)
        p = self.pbt
        rs = np.random.RandomState(np.array([p["seed"], self.pbt_round, self.env_offset],
                                            dtype=np.uint32))
        for k in SWEEP_KEYS:
            if k in p["perturb"]:
                factors = p["perturb"][k]
                lo, hi = p["bounds"][k]
                c = rs.randint(0, len(factors), size=self.E)
            v = self.pbt_values.get(k)
            if v is None:
                continue
            for e in np.nonzero(src != np.arange(self.E))[0]:
                x = float(v[src[e]])
                if k in p["perturb"]:
                    x = min(max(x * factors[c[e]], lo), hi)
                v[e] = x
        self._pbt_upload()

    def _pbt_upload(self):
        """The per-agent device arrays from pbt_values, by the formulas that
        built them (in place: the learn kernels re-read them every launch)."""
        def put(dst, values, dtype):
            host = np.repeat(np.asarray(values, dtype=dtype), self.A)
            dst.copy_(torch.as_tensor(host))
        pv = self.pbt_values
        if "learning_rate" in pv:
            put(self.hp_lr, pv["learning_rate"], np.float32)
        if "gamma" in pv:
            put(self.hp_gamma, [nstep_gamma(g, self.n_step) for g in pv["gamma"]], np.float32)
            if self.nstep_gamma_a is not None:
                put(self.nstep_gamma_a, pv["gamma"], np.float64)
        if "tau" in pv:
            consts = [soft_update_consts(t) for t in pv["tau"]]
            put(self.hp_tau, [c[0] for c in consts], np.float32)
            put(self.hp_omt, [c[1] for c in consts], np.float32)

    def pbt_population(self):
        """{key: [min, median, max]} of pbt_values, per per-agent key."""
        return {k: [float(np.min(v)), float(np.median(v)), float(np.max(v))]
                for k, v in self.pbt_values.items()}

    # -------------------------------------------------------------- weights
    def keras_params(self, which="params"):
        """[NA, P_keras] copy of params / target / adam_m / adam_v in Keras order."""
        return kernel_to_keras(getattr(self, which).cpu().numpy(), self.H)

    def get_weights(self, agent):
        """Keras get_weights() order for one agent: [W1, b1, W2, b2, W3, b3]."""
        p = kernel_to_keras(self.params[0 if self.shared else agent].cpu().numpy(), self.H)
        H = self.H
        shapes = [(D_IN, H), (H,), (H, H), (H,), (H, N_ACTIONS), (N_ACTIONS,)]
        out, o = [], 0
        for sh in shapes:
            n = int(np.prod(sh))
            out.append(p[o:o + n].reshape(sh).copy())
            o += n
        return out

    def set_weights(self, agent, weights):
        flat = np.concatenate([np.asarray(w, np.float32).reshape(-1) for w in weights])
        agent = 0 if self.shared else agent
        self.params[agent].copy_(torch.from_numpy(keras_to_kernel(flat, self.H)))
        self.target[agent].copy_(self.params[agent])
        self._refresh_params_h()
        self._refresh_target_h()

    def state_dict(self):
        return {"params": self.params.cpu(), "target": self.target.cpu(),
                "adam_m": self.adam_m.cpu(), "adam_v": self.adam_v.cpu(),
                "learn_step_counter": self.learn_step_counter,
                "global_step_count": self.global_step_count}

    def load_state_dict(self, sd):
        for k in ["params", "target", "adam_m", "adam_v"]:
            getattr(self, k).copy_(sd[k].to(self.device))
        self._refresh_params_h()
        self._refresh_target_h()
        self.learn_step_counter = int(sd["learn_step_counter"])
        self.global_step_count = int(sd["global_step_count"])
