"""src/scripts/train.py -- drop-in training driver on the MI355X kernels.

Same loop as the reference (src/scripts/train.py:182-316): per episode reset,
then while not done: every agent selects an action, the env takes one RL step
(ACTION_MAP phases, STEP_DURATION one-second substeps), rewards are
0.3*local + 0.7*global on the PRE-step state, every agent remembers and
replays (one learn step).  Differences, all outside the hot path:
  * SUMO/TraCI is replaced by the GPU simulator (src/env/traffic_env.py);
  * wandb (network) is replaced by an offline JSONL metrics file;
  * seeds are explicit (--seed), the reference never seeds (A-2).
`--batched` runs the same loop for --envs replicas with one kernel launch per
stage for all agents (dmdqn_amd.trainer.Trainer) -- the throughput path.

  python -m src.scripts.train --episodes 2
  python -m src.scripts.train --batched --envs 1024 --grid 4x4 --episodes 1
  python -m src.scripts.train --batched --envs 64 --grid 2x2 --episodes 1 \
      --sweep learning_rate=1e-4,5e-4,1e-3          # 3 variants in one run, ranked
  python -m src.scripts.train --batched --envs 64 --grid 2x2 --episodes 1 \
      --sweep learning_rate=1e-4,1e-3 --pbt interval=200   # the best replicas replace the worst
  python -m src.scripts.train --batched --envs 64 --grid 2x2 --episodes 1 --n_step 3
  python -m src.scripts.train --batched --envs 64 --grid 2x2 --episodes 1 --global_clipnorm 10
"""
import argparse
import json
import logging
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from src.agents import dqn_agent  # noqa: E402
from src.agents.dqn_agent import DQNAgent  # noqa: E402
from src.env.traffic_env import EnvConfig, TrafficEnv  # noqa: E402

EPISODES = 100
MAX_LANES_PER_DIRECTION = 3
STEP_DURATION = 10.0
ACTION_MAP = {0: 0, 1: 3, 2: 6, 3: 9}
MAX_SIM_TIME = 2400

logger = logging.getLogger("dmdqn_logger")

AGENT_CONFIG = {  # train.py:111-121
    "learning_rate": 0.001,
    "gamma": 0.99,
    "epsilon_start": 1.0,
    "epsilon_min": 0.01,
    "epsilon_decay_steps": 200000,
    "replay_buffer_size": 10000,
    "batch_size": 128,
    "target_update_frequency": 500,
    "nn_layers": [128, 128],
}


class SmoothedValue:  # train.py:144-156
    def __init__(self, alpha=0.5):
        self.alpha = alpha
        self.value = None

    def update(self, new_val):
        if self.value is None:
            self.value = new_val
        else:
            self.value = self.alpha * new_val + (1 - self.alpha) * self.value

    def get_value(self):
        return self.value


# SUMO_CFG_PATH of the reference (train.py:50: grid_3x3.sumocfg), derived into the
# simulator's tables by tests/golden/make_scenario.py
DEFAULT_SCENARIO = os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(
    os.path.abspath(__file__)))), "config", "scenarios", "grid_3x3_p06.npz")


def calculate_local_reward(current_state, next_state):  # train.py:159-160
    return -1.0 * sum(current_state[:12])


def calculate_global_reward(global_state: dict, next_global_state: dict):  # train.py:163-165
    return -1.0 * sum(sum(state[:12]) for state in global_state.values())


def initialize_environment(rows=3, cols=3, seed=0, signal_features="reference", scenario=None):
    env = TrafficEnv(EnvConfig(rows=rows, cols=cols, num_envs=1, seed=seed,
                               step_duration=int(STEP_DURATION), max_sim_time=MAX_SIM_TIME,
                               signal_features=signal_features, scenario=scenario))
    return env, env.get_controlled_intersection_ids()


def create_agents(tl_junctions, config=AGENT_CONFIG):
    return {j: DQNAgent(state_size=89, action_size=4, agent_id=j, config=config) for j in tl_junctions}


def target_config(tau=0.0, target_update_frequency=None, config=AGENT_CONFIG, n_step=1,
                  global_clipnorm=0.0, health_every=0, redo_every=0, redo_patience=1,
                  behavior=None, behavior_steps=0, behavior_eps=0.1):
    """AGENT_CONFIG with the target-network rule of --tau /
    --target_update_frequency: soft updates (dqn_agent.py:372-373, 389-399) of
    rate tau after every learn, hard syncs every target_update_frequency learns
    (0 = never; None = the config's); --n_step: n-step returns built at the
    replay store (AgentConfig.n_step; 1 = the reference's one-step transitions);
    and --global_clipnorm: gradient clipping by global norm
    (AgentConfig.global_clipnorm; 0 = off, the reference's optimizer); and
    --health_every: the network health probe after every N-th learn
    (AgentConfig.health_every; 0 = off); and --redo_every / --redo_patience:
    dead-unit recycling after every N-th learn (AgentConfig.redo_every; 0 =
    off); and --behavior / --behavior_steps / --behavior_eps: a rule-based
    behaviour policy for the first steps or the whole run (AgentConfig.behavior;
    None = off)."""
    config = dict(config)
    if behavior:
        config.update(behavior=behavior, behavior_steps=int(behavior_steps),
                      behavior_eps=float(behavior_eps))
    if redo_every:
        config["redo_every"], config["redo_patience"] = int(redo_every), int(redo_patience)
    if health_every:
        config["health_every"] = int(health_every)
    if n_step != 1:
        config["n_step"] = n_step
    if global_clipnorm:
        config["global_clipnorm"] = float(global_clipnorm)
    if tau:
        config["tau"] = float(tau)
    if target_update_frequency is not None:
        config["target_update_frequency"] = int(target_update_frequency)
    return config


def parse_sweep(items):
    """--sweep KEY=v1,v2,... (repeatable) -> AgentConfig.sweep: {key: [floats]}
    in the order given (the grid's key order), or None for no items.  The keys
    and values are checked where the sweep is used (agent.sweep_variants); here
    only the syntax, and a key given twice."""
    if not items:
        return None
    sweep = {}
    for item in items:
        key, sep, vals = str(item).partition("=")
        key = key.strip()
        if not sep or not key or not vals.strip():
            raise ValueError(f"--sweep {item!r}: expected KEY=v1,v2,...")
        if key in sweep:
            raise ValueError(f"--sweep {key} given twice")
        try:
            sweep[key] = [float(v) for v in vals.split(",")]
        except ValueError:
            raise ValueError(f"--sweep {item!r}: values must be numbers") from None
    return sweep


def parse_pbt(spec, perturb_items=None):
    """--pbt interval=500,truncation=0.25,seed=0 and the repeatable
    --pbt_perturb KEY=f1,f2,... -> AgentConfig.pbt, or None without --pbt.
    Only the syntax is checked here (and a key given twice, --pbt_perturb
    without --pbt); the values where the config is used (agent.check_pbt)."""
    if spec is None:
        if perturb_items:
            raise ValueError("--pbt_perturb needs --pbt")
        return None
    pbt = {}
    for item in str(spec).split(","):
        key, sep, val = item.partition("=")
        key, val = key.strip(), val.strip()
        if not sep or not key or not val:
            raise ValueError(f"--pbt {spec!r}: expected interval=N[,truncation=F][,seed=N]")
        if key not in ("interval", "truncation", "seed"):
            raise ValueError(f"--pbt key {key!r}: interval, truncation or seed")
        if key in pbt:
            raise ValueError(f"--pbt {key} given twice")
        try:
            pbt[key] = float(val) if key == "truncation" else int(val)
        except ValueError:
            raise ValueError(f"--pbt {item!r}: not a number") from None
    if perturb_items:
        try:
            pbt["perturb"] = parse_sweep(perturb_items)
        except ValueError as e:
            raise ValueError(str(e).replace("--sweep", "--pbt_perturb")) from None
    return pbt


def train_agents(episodes=EPISODES, rows=3, cols=3, seed=0, metrics=None, scenario=None,
                 save_dir=None, tau=0.0, target_update_frequency=None, n_step=1):
    dqn_agent.seed(seed)
    env, tl_junctions = initialize_environment(rows, cols, seed, scenario=scenario)
    agents = create_agents(tl_junctions,
                           target_config(tau, target_update_frequency, n_step=n_step))
    assert len(agents) == env.R * env.C
    smooth_total = SmoothedValue(alpha=0.3)
    out = open(metrics, "w") if metrics else None
    for episode in range(episodes):
        state_dict = env.reset_dict()
        done, step_count, total_reward = False, 0, 0.0
        while not done:
            actions = {j: agents[j].select_action(state_dict[j][None]) for j in tl_junctions}
            next_state_dict, rewards, done, info = env.step_dict(actions)
            total_reward = sum(rewards.values())
            smooth_total.update(total_reward)
            total_loss = 0.0
            for j in tl_junctions:
                agents[j].remember(state_dict[j][None], actions[j], rewards[j],
                                   next_state_dict[j][None], done)
                total_loss += agents[j].replay()
            if out:
                out.write(json.dumps({"episode": episode, "step": step_count,
                                      "total_reward": total_reward, "total_loss": total_loss,
                                      "smooth_total_reward": smooth_total.get_value()}) + "\n")
            state_dict = next_state_dict
            step_count += 1
        logger.info(f"Episode {episode + 1} complete. Total Reward: {total_reward}")
    if out:
        out.close()
    if save_dir:  # additive: the reference never saves (test.py:195 expects this naming)
        os.makedirs(save_dir, exist_ok=True)
        for j in tl_junctions:
            agents[j].save_model(os.path.join(save_dir, f"agent_{j}.weights.npz"))
    return agents


def train_batched(episodes, rows, cols, envs, precision, seed, metrics=None, scenario=None,
                  shared=False, save_dir=None, resume=None, log_every=20, loss="mse",
                  actuated=False, tau=0.0, target_update_frequency=None, sweep=None, n_step=1,
                  pbt=None, global_clipnorm=0.0, health_every=0, redo_every=0, redo_patience=1,
                  behavior=None, behavior_steps=0, behavior_eps=0.1):
    """E env replicas of the loop on the GPU.  The optional JSONL carries the
    reference's learn scalars (dqn_agent.py:361-370: loss, epsilon,
    q_values_mean / _std, action_distribution) and its per-step rewards with
    EMA smoothing (train.py:295-307, SmoothedValue alpha 0.3), averaged over
    replicas, every `log_every` steps (each record syncs).  sweep
    (AgentConfig.sweep, parse_sweep): replica g trains with variant g % G; each
    record then carries "variants" (per variant: its hyperparameters, replicas,
    total / smoothed total reward and learn scalars), the final line ranks the
    variants by smoothed total reward, and the exported Keras weights are those
    of the best variant's first replica (the checkpoint holds them all).
    global_clipnorm (AgentConfig.global_clipnorm): each record's learn scalars
    then carry grad_norm_mean / grad_norm_max / clipped_frac too.  health_every
    (AgentConfig.health_every): once a probe has run, each record's learn
    scalars (per variant too) carry the "health" block of the last probe, and
    the final line's variants their dead_frac and update_ratio.  redo_every /
    redo_patience (AgentConfig.redo_every): each record's learn scalars carry
    the "redo" block (rounds, the units recycled last round and in total).
    behavior / behavior_steps / behavior_eps (AgentConfig.behavior): every
    record carries the "behavior" block (policy, eps, active).  pbt
    (AgentConfig.pbt, parse_pbt): population-based training; the variants then
    dissolve, so a record written at a round carries that round's pbt_log
    entry, the final line a "pbt" block (rounds, copies, the best replica of
    the last completed window with its values, the population's [min, median,
    max] per key) instead of "variants", and the exported weights are that
    best replica's."""
    from dmdqn_amd.agent import AgentConfig
    from dmdqn_amd.trainer import Trainer
    cfg = AgentConfig.from_dict(target_config(tau, target_update_frequency, n_step=n_step,
                                              global_clipnorm=global_clipnorm,
                                              health_every=health_every,
                                              redo_every=redo_every,
                                              redo_patience=redo_patience,
                                              behavior=behavior, behavior_steps=behavior_steps,
                                              behavior_eps=behavior_eps))
    cfg.precision, cfg.seed, cfg.shared_params, cfg.loss = precision, seed, shared, loss
    cfg.sweep, cfg.pbt = sweep, pbt
    tr = Trainer(EnvConfig(rows=rows, cols=cols, num_envs=envs, seed=seed, scenario=scenario,
                           actuated=actuated), cfg)
    from dmdqn_amd import checkpoint as CK
    if resume:
        CK.load(resume, tr)
    out = open(metrics, "w") if metrics else None
    smooth_global, smooth_total = SmoothedValue(alpha=0.3), SmoothedValue(alpha=0.3)
    variants = tr.agent.variants if sweep and not pbt else []
    smooth_variant = VariantSmoothedValues(alpha=0.3)
    t0 = time.perf_counter()
    steps = 0
    while tr.episode < episodes:
        log = out is not None and steps % log_every == 0
        if out is not None and pbt and (tr.total_steps + 1) % tr.agent.pbt["interval"] == 0:
            log = True  # the step a round may follow: its record carries the round
        if log:  # global reward of the PRE-step state (train.py:241, A-3)
            glob = -tr.env.local[..., :12].sum(dim=(1, 2), dtype=torch.float64)
        st = tr.step(collect_stats=log)
        steps += 1
        if variants and (steps - 1) % log_every == 0:  # (the ranking needs no metrics file)
            vr = tr.variant_rewards_device()  # stays on the device: no sync without a record
            smooth_variant.update(vr)
        if log:
            total = tr.last_reward.sum(dim=1)                  # train.py:255 per replica
            g, tt = float(glob.mean()), float(total.mean())
            smooth_global.update(g)
            smooth_total.update(tt)
            rec = {"episode": tr.episode, "step": steps, "global_reward": g, "total_reward": tt,
                   "smooth_global_reward": smooth_global.get_value(),
                   "smooth_total_reward": smooth_total.get_value()}
            if st.loss_launched:
                rec.update(tr.agent.learn_metrics())
            if tr.agent.behavior is not None:  # (before the first learn too)
                rec["behavior"] = tr.agent.behavior_metrics()
            if variants:
                if st.loss_launched:
                    vrec = tr.agent.learn_metrics(by_variant=True)
                else:
                    voe = tr.agent.variant_of_env
                    vrec = [dict(variant=i, **v, envs=int((voe == i).sum()))
                            for i, v in enumerate(variants)]
                for r, total_r, sm in zip(vrec, _host_values(vr), smooth_variant.get_values()):
                    r.update(total_reward=total_r, smooth_total_reward=sm)
                rec["variants"] = vrec
            if tr.pbt_log and tr.pbt_log[-1]["step"] == tr.total_steps:
                rec["pbt"] = tr.pbt_log[-1]
            out.write(json.dumps(rec) + "\n")
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    final = {"agent_env_steps": steps * tr.env.E * tr.env.A, "seconds": round(el, 3),
             "agent_env_steps_per_s": round(steps * tr.env.E * tr.env.A / el, 1)}
    best_env = 0
    if variants:
        final["variants"] = rank_variants(variants, tr.agent.variant_of_env.tolist(),
                                          smooth_variant.get_values() or [None] * len(variants))
        if final["variants"]:
            best_env = final["variants"][0]["first_env"]
        if health_every and tr.agent.health is not None:  # the last probe, per variant
            tr.sync_outputs()
            for row in final["variants"]:
                h = tr.agent.health_metrics(tr.agent._variant_of_agent == row["variant"])
                row["dead_frac"] = [layer["dead_frac"] for layer in h["layers"]]
                row["update_ratio"] = {k: v["mean"] for k, v in h["update_ratio"].items()}
    if pbt:
        ag = tr.agent
        if tr.pbt_log:
            best_env = tr.pbt_log[-1]["best_env"]
        final["pbt"] = {"rounds": len(tr.pbt_log),
                        "copies": sum(len(r["copied"]) for r in tr.pbt_log),
                        "best_env": best_env,
                        "best": {k: float(v[best_env]) for k, v in ag.pbt_values.items()},
                        "population": ag.pbt_population()}
    print(json.dumps(final))
    if out:
        out.close()
    if save_dir:
        os.makedirs(save_dir, exist_ok=True)
        CK.save(os.path.join(save_dir, "checkpoint.pt"), tr)
        CK.export_keras_weights(tr.agent, save_dir, tr.env.grid.junction_ids, env_index=best_env)
    return tr


def _host_values(t):
    """A float64 device vector as a list, None for NaN (a variant without
    replicas).  Syncs."""
    return [None if v != v else v for v in t.tolist()]


class VariantSmoothedValues:
    """One SmoothedValue per sweep variant, kept together as a float64 vector
    on the device (SmoothedValue's rule, elementwise, in its order of
    operations): update() queues device work only, get_values() copies to the
    host and syncs -- once per metrics record and once at the end of the run."""

    def __init__(self, alpha=0.5):
        self.alpha = alpha
        self.value = None

    def update(self, new_val):
        if self.value is None:
            self.value = new_val
        else:
            self.value = self.alpha * new_val + (1 - self.alpha) * self.value

    def get_values(self):
        return [] if self.value is None else _host_values(self.value)


def rank_variants(variants, variant_of_env, smoothed):
    """The variants that have replicas, best smoothed total reward first (ties
    and variants without a reward yet keep their grid order, after the others):
    [{rank, variant, learning_rate, gamma, tau, envs, first_env,
    smooth_total_reward}]."""
    rows = []
    for i, v in enumerate(variants):
        envs = [e for e, k in enumerate(variant_of_env) if k == i]
        if envs:
            rows.append(dict(variant=i, **v, envs=len(envs), first_env=envs[0],
                             smooth_total_reward=smoothed[i]))
    rows.sort(key=lambda r: (r["smooth_total_reward"] is None,
                             -(r["smooth_total_reward"] or 0.0), r["variant"]))
    return [dict(rank=k + 1, **r) for k, r in enumerate(rows)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--episodes", type=int, default=EPISODES)
    ap.add_argument("--grid", default="3x3")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--batched", action="store_true")
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--precision", default="fp16", choices=["fp32", "fp16", "bf16"])
    ap.add_argument("--metrics", default=None, help="offline JSONL metrics (replaces wandb)")
    ap.add_argument("--scenario", default=None,
                    help="SUMO scenario: a .sumocfg or a .npz from sumo_scenario (default for the "
                         "single-env path: the reference's grid_3x3 + grid_3x3_p06 routes, as "
                         "train.py's SUMO_CONFIG); 'synthetic' = generated demand for --grid")
    ap.add_argument("--shared", action="store_true",
                    help="batched only: one network shared by all agents (C5)")
    ap.add_argument("--save_dir", default=None,
                    help="write agent_<id>.weights.npz (and, batched, checkpoint.pt) at the end")
    ap.add_argument("--resume", default=None, help="batched only: a checkpoint.pt to resume from")
    ap.add_argument("--log_every", type=int, default=20, help="batched metrics interval (steps)")
    ap.add_argument("--loss", default="mse", choices=["mse", "huber"],
                    help="batched only: mse (dqn_agent.py:352) or huber (experimental/agent.py:99)")
    ap.add_argument("--actuated", action="store_true",
                    help="batched only: SUMO's actuated gap-out on phase 0 (default fixed durations)")
    ap.add_argument("--tau", type=float, default=0.0,
                    help="soft target updates of this rate after every learn "
                         "(dqn_agent.py:389-399); 0 = off (the reference's training path)")
    ap.add_argument("--target_update_frequency", type=int, default=None,
                    help="hard target sync every N learns (default 500, train.py:118); 0 = never")
    ap.add_argument("--sweep", action="append", default=None, metavar="KEY=v1,v2,...",
                    help="batched only, repeatable: a hyperparameter sweep across the env "
                         "replicas (KEY: learning_rate, gamma or tau); the variants are the grid "
                         "of all --sweep lists, replica g runs variant g mod G")
    ap.add_argument("--n_step", type=int, default=1,
                    help="n-step returns: every stored transition carries the discounted sum of "
                         "up to N rewards and the learn bootstraps with gamma^N (1..32; 1 = the "
                         "reference's one-step transitions); the last N-1 raw transitions of a "
                         "run are never stored")
    ap.add_argument("--pbt", default=None, metavar="interval=N[,truncation=F][,seed=N]",
                    help="batched only: population-based training across the env replicas -- "
                         "every N steps the worst share F (default 0.25) of the replicas take "
                         "over the nets and hyperparameters of the best, perturbed")
    ap.add_argument("--pbt_perturb", action="append", default=None, metavar="KEY=f1,f2,...",
                    help="with --pbt, repeatable: the factors a copied value of KEY "
                         "(learning_rate, gamma or tau) is multiplied by, one drawn per copy "
                         "(default learning_rate=0.8,1.25)")
    ap.add_argument("--global_clipnorm", type=float, default=0.0, metavar="F",
                    help="batched only: clip every agent's gradient to global norm F before the "
                         "Adam step (Keras Adam(global_clipnorm=F)); 0 = off.  fp16 / bf16 "
                         "independent nets; the metrics gain grad_norm_mean / _max / clipped_frac")
    ap.add_argument("--health_every", type=int, default=0, metavar="N",
                    help="batched only: probe every agent's network after each N-th learn (dead "
                         "and active ReLU units, non-finite activations, weight norms, "
                         "update-to-weight ratios); the metrics gain a \"health\" block.  0 = "
                         "off.  fp16 / bf16 independent nets")
    ap.add_argument("--redo_every", type=int, default=0, metavar="N",
                    help="batched only: after each N-th learn probe every agent's network and "
                         "recycle its dead ReLU units (ReDo: fresh incoming weights, zero "
                         "outgoing weights, zero Adam moments); the metrics gain a \"redo\" "
                         "block.  0 = off.  fp16 / bf16 independent nets")
    ap.add_argument("--redo_patience", type=int, default=1, metavar="K",
                    help="with --redo_every: a unit is recycled once it was dead on K probes in "
                         "a row (1..255)")
    ap.add_argument("--behavior", default=None, choices=["longest_queue", "max_pressure"],
                    help="batched only: a rule-based behaviour policy -- while it is active the "
                         "agents take the controller's action (a uniform one below "
                         "--behavior_eps) instead of epsilon-greedy on their nets, so the "
                         "replay fills with a controller's transitions; the metrics gain a "
                         "\"behavior\" block.  Default: off")
    ap.add_argument("--behavior_steps", type=int, default=0, metavar="N",
                    help="with --behavior: active for the first N env steps (0 = the whole run)")
    ap.add_argument("--behavior_eps", type=float, default=0.1, metavar="F",
                    help="with --behavior: the share of uniformly random actions, in [0, 1]")
    args = ap.parse_args()
    try:
        sweep = parse_sweep(args.sweep)
        pbt = parse_pbt(args.pbt, args.pbt_perturb)
        from dmdqn_amd.agent import (check_behavior, check_clipnorm, check_health_every,
                                     check_n_step, check_redo)
        check_behavior(args.behavior, args.behavior_steps, args.behavior_eps)
        check_health_every(args.health_every)
        check_redo(args.redo_every, args.redo_patience)
        check_n_step(args.n_step, AGENT_CONFIG["replay_buffer_size"])
        check_clipnorm(args.global_clipnorm)
    except ValueError as e:
        ap.error(str(e))
    if sweep and not args.batched:
        ap.error("--sweep needs --batched")
    if pbt and not args.batched:
        ap.error("--pbt needs --batched")
    if args.global_clipnorm and not args.batched:
        ap.error("--global_clipnorm needs --batched (the drop-in DQNAgent keeps float rows)")
    if args.global_clipnorm and (args.shared or args.precision == "fp32"):
        ap.error("--global_clipnorm runs with --precision fp16 / bf16, not with --shared")
    if args.health_every and not args.batched:
        ap.error("--health_every needs --batched")
    if args.health_every and (args.shared or args.precision == "fp32"):
        ap.error("--health_every runs with --precision fp16 / bf16, not with --shared")
    if args.redo_every and not args.batched:
        ap.error("--redo_every needs --batched")
    if args.redo_every and (args.shared or args.precision == "fp32"):
        ap.error("--redo_every runs with --precision fp16 / bf16, not with --shared")
    if args.behavior and not args.batched:
        ap.error("--behavior needs --batched")
    logging.basicConfig(level=logging.INFO)
    rows, cols = (int(x) for x in args.grid.split("x"))
    scenario = args.scenario
    if scenario is None and not args.batched:
        scenario = DEFAULT_SCENARIO
    if scenario == "synthetic":
        scenario = None
    if args.batched:
        train_batched(args.episodes, rows, cols, args.envs, args.precision, args.seed, args.metrics,
                      scenario, args.shared, args.save_dir, args.resume, args.log_every, args.loss,
                      args.actuated, args.tau, args.target_update_frequency, sweep, args.n_step,
                      pbt, args.global_clipnorm, args.health_every, args.redo_every,
                      args.redo_patience, args.behavior, args.behavior_steps, args.behavior_eps)
    else:
        train_agents(args.episodes, rows, cols, args.seed, args.metrics, scenario, args.save_dir,
                     args.tau, args.target_update_frequency, args.n_step)


if __name__ == "__main__":
    main()
