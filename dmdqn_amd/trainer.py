"""The batched reference training loop (src/scripts/train.py:188-316) on the GPU.

One `step()` is one iteration of the loop body for every agent of every env
replica:  act (select_action) -> env step (setPhase, K substeps) -> observe /
reward -> remember -> replay (learn), in the reference's order.  All of it is
kernel launches; the host keeps only counters.

Schedules (`overlap`).  The reference loop is sequential, but its data flow
is not: the replay draws of a step depend only on the CPython stream and the
ring length (never on the ring contents), and with the reference's epsilon
(1.0 on the training path, A-1) the next act and env step need nothing from
the learn.  Every schedule gives each kernel exactly the inputs of the
sequential order, so results are bit-identical (tests/test_gpu_overlap.py).

  "none"    (default) one stream: act, sim, observe, store, sample, learn.
            With fused=True (default; int8 replay rows) act, sim, observe and
            store are ONE launch per replica (dmdqn_env_step, bit-identical).
  "sample"  the replay draws of step t run on a side stream beside
            act/sim/observe/store of step t (all latency-bound, low occupancy);
            the side stream waits for learn t-1, so nothing shares the GPU
            with a learn.
              side:  [wait learn t-1] sample_t (ev_s)
              main:  act_t sim_t observe_t store_t [wait ev_s] learn_t
            (fused: main runs env_step_t [wait ev_s] learn_t).
  "full"    step t+1's act -> sim -> observe -> sample run on the side stream
            while learn t runs; only remember (which overwrites ring slots
            learn t may read) waits for learn t.  A greedy act (epsilon < 1)
            also waits for the learn, whose weights it reads.  The learn then
            shares the GPU with the sim, so its own duration grows.
              side:  [wait store t-1] act_t sim_t observe_t sample_t (ev_obs)
              main:                  [wait ev_obs] store_t (ev_store) learn_t
            The fused learn's workgroups fill every CU until they end, so the
            side work queued beside it mostly waits; split_learn=True makes the
            learn two launches whose Adam half leaves room beside it.

  "env"     the fused env step of step t+1 (act, sim, observe, remember) and
            the replay draws of learn t+1 run on a side stream beside learn t.
            The ring has s = AgentConfig.ring_spare spare slots (16;
            kernels.ReplayRing: cap + s slots for a deque of maxlen cap), and
            the stores of steps t+1 .. t+s go to slots learn t cannot sample;
            the store of step t+s+1 waits for learn t (its slot is in learn t's
            window) or a later marked learn -- at fixed epsilon 1 the learn
            stream marks every s-th call with an ordering-only event, and the
            side stream runs up to s steps ahead (the agent's per-step output
            buffers rotate over s + 2 copies for it).  A greedy act (epsilon <
            1) waits for learn t's weights.
              side:  [wait the newest marked learn <= t-1] env_step_{t+1} sample_{t+1} (ev_env)
              main:  [wait ev_env of t] learn_t
            16-bit independent nets run their learns in PAIRS (pair_learns,
            default on): learn t is begun and held back, and the next call
            launches learns t and t+1 as one kernel (dmdqn_learn_pair; the second
            learn re-reads the weights and Adam slots while they are on the chip;
            the same bits).  Hard target syncs, collect_stats steps, a learn_hook
            and the agent's diagnostics buffers keep single launches.
            CHANGES WHAT step() LEAVES: after a call that held its learn back,
            agent.params / adam_m / adam_v / target and agent.loss are one learn
            behind until the next call.  Read them through last_loss or after
            sync_outputs() / synchronize() (they launch the held-back learn), or
            pass pair_learns=False; a loop that does so after EVERY step runs
            every learn alone and gains nothing from pairing.
              main:  [wait ev_env of t] -        [wait ev_env of t+1] learn_{t,t+1}
            With a CU-masked side stream (bench --cu-split) the two split the
            chip.  side_learn=m runs the learn of the last m agents on the side
            stream behind its env step and draws (those CUs idle otherwise):
              side:  ... sample_{t+1} (ev_env) learn_{t+1}[NA-m, NA)
              main:  [wait ev_env] learn_{t+1}[0, NA-m)

  "learn"   the replay draws of step t run on a side stream beside learn t-1
            (everything else on one stream).  For the shared net (C5): its S'
            pass leaves room on every CU for a sampler block, so the draws
            (latency-bound, one block per env) hide behind the learn.
              side:  [wait env_step_{t-1}] sample_t (ev_s)
              main:  env_step_t [wait ev_s] learn_t

n-step returns (AgentConfig.n_step > 1): the raw transition of a step goes to
the agent's staging ring (agent.store_ring) and remember() / remembered()
commit the window's oldest start into agent.ring on the same stream, so the
ring a learn samples lags the raw stores by n_step - 1 steps.  "none" (fused
and fused=False) and "env" (with and without side_learn) run it, bit-identical
to each other; "sample", "learn" and "full" raise ValueError for n_step > 1.

A rule-based behaviour policy (AgentConfig.behavior) enters through
agent.act_inputs(): while it is active the act's greedy actions are the
rule's (one small launch on the stream of the act, reading the observation
only) and its epsilon is behavior_eps.  "none" (fused and fused=False) and
"env" run it, bit-identical to each other; the other schedules raise ValueError.

Population-based training (AgentConfig.pbt): after every step the reward joins
each replica's fitness on the caller's stream, and every `interval` steps a
round runs there between quiesce() and join_streams(): select, the in-place
exchange of the nets and Adam slots, explore (Trainer.pbt_log records it).
"none" and "env" (with and without side_learn) run it, bit-identical to each
other; the other schedules raise ValueError.

What a step returns or exposes per step (obs, reward, loss, agent.actions,
agent.idx) is fresh or double-buffered, so the caller may read it on its own
stream between steps (under "env" with side_learn, read the loss through
last_loss, or call sync_outputs() before reading agent tensors: the side
learn's part is waited for lazily, except on collect_stats steps; with paired
learns a held-back learn is launched by the same two, by synchronize(),
quiesce() and join_streams(): agent.loss and the nets read without them may
lag one learn).  Persistent env/agent state (sim arrays, RNG streams) is
advanced by the next step's side stream without waiting for such reads: read
it host-blocking (.cpu()), and call join_streams() after writing it.
"""
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from .agent import (AgentConfig, BatchedDQN, check_behavior, check_n_step, check_pbt,
                    sweep_variants, variant_assignment)
from .env import EnvConfig, TrafficEnv


SCHEDULES = ("none", "sample", "full", "env", "learn")


def pair_action(pending, plain, next_sync):
    """What a call of the paired "env" schedule does with the learn it has begun
    (pending: a held-back learn of the call before exists; plain: this learn may
    share a launch -- no metrics, no timing hook, no hard sync; next_sync: the
    learn after it is a hard sync): "pair" (one launch for both), "both" (the
    held-back one, then this one, a launch each), "hold" (launch nothing: the
    next call pairs it) or "single"."""
    if pending:
        return "pair" if plain else "both"
    return "hold" if plain and not next_sync else "single"


def pair_mark_due(j, last_mark, spare, mark_every=False):
    """Whether the paired "env" schedule marks call j (all learns up to j's are
    launched), the newest mark being of call last_mark (-1: none yet).  A call
    that holds its learn back cannot be marked, but of two calls in a row one
    can: the call after a held-back one launches both learns, or -- the caller
    having had the held-back learn launched in between -- marks for it first.
    So the next chance after j may be j + 2, and marks are at most `spare`
    calls apart when j is marked from j - last_mark >= spare - 1 on."""
    return mark_every or j - last_mark >= spare - 1


@dataclass
class StepStats:
    loss_launched: bool
    done: bool


class Trainer:
    def __init__(self, env_cfg: EnvConfig = None, agent_cfg: AgentConfig = None, device="cuda",
                 overlap="none", side_stream=None, split_learn=False, fused=True,
                 war_events=True, side_learn=0, mark_every_learn=False, pair_learns=True):
        # a sweep (AgentConfig.sweep) is checked before any device work, which
        # starts with the env below; BatchedDQN, usable without a Trainer,
        # expands the grid again for itself (host work on a few list entries)
        agent_cfg = agent_cfg or AgentConfig()
        n_variants = len(sweep_variants(agent_cfg))
        # n-step returns (AgentConfig.n_step > 1) run under "none" (fused or
        # not) and "env" (with or without side_learn), bit-identical to each
        # other.  "sample", "learn" and "full" draw the next learn's indices
        # before the store, for the ring length they predict from the raw store
        # count; with a staging ring in between that prediction does not hold,
        # so they are refused
        if check_n_step(agent_cfg.n_step, agent_cfg.replay_buffer_size) > 1 and overlap in (
                "sample", "learn", "full", True):
            raise ValueError(f'n_step > 1 runs under overlap "none" or "env", not {overlap!r}')
        # population-based training (AgentConfig.pbt), checked like the sweep
        # before any device work; its rounds run under the two schedules they
        # are tested under, as n-step returns
        env_cfg = env_cfg or EnvConfig()
        if check_pbt(agent_cfg, env_cfg.num_envs) is not None and overlap not in (
                "none", "env", False):
            raise ValueError(f'pbt runs under overlap "none" or "env", not {overlap!r}')
        # a rule-based behaviour policy (AgentConfig.behavior), checked like the
        # two above before any device work and run under the same two schedules
        if check_behavior(agent_cfg.behavior, agent_cfg.behavior_steps,
                          agent_cfg.behavior_eps)[0] is not None and overlap not in (
                "none", "env", False):
            raise ValueError(f'behavior runs under overlap "none" or "env", not {overlap!r}')
        self.pbt_log = []  # one dict per round (_pbt_round)
        self.env = TrafficEnv(env_cfg, device=device)
        if overlap is True or overlap is False:
            overlap = "full" if overlap else "none"
        if overlap not in SCHEDULES:
            raise ValueError(f"overlap must be one of {SCHEDULES}")
        self.overlap = overlap
        # side_stream: e.g. a CU-masked stream (_lib.cu_masked_stream), so the
        # side work and the learn split the chip instead of sharing CU slots
        self.side = None
        if overlap != "none":
            self.side = side_stream if side_stream is not None else torch.cuda.Stream(self.env.device)
        self._ev_store = self._ev_learn = None
        self._side_pending = None  # overlap "env": the side learn, waited for lazily
        self._ev_env_prev = None  # overlap "learn": the last env step
        self._join = True  # the side stream's first work waits for everything before it
        # replica g = env_offset + e runs variant g % G of the sweep
        voe = variant_assignment(n_variants, self.env.E, self.env.cfg.env_offset)
        self.agent = BatchedDQN(self.env.E, self.env.A, agent_cfg, device=device,
                                env_seeds=self.env.seeds, variant_of_env=voe,
                                env_offset=self.env.cfg.env_offset)
        # overlap "learn": the sampler's LDS is what the shared learn's S' pass
        # leaves of a CU, so one sampler block runs beside each S' workgroup
        # (with the default four-blocks-per-CU budget the two serialise); the
        # CU's LDS is the device's (160 KB on gfx950), and the launcher clamps
        # the budget to what one workgroup may hold
        self._sampler_lds = 0
        if overlap == "learn" and self.agent.shared:
            self._sampler_lds = max(0, _lib.device_lds_per_cu(self.env.device)
                                    - _lib.learn_shared_lds_bytes())
        # split_learn (agent.set_split_learn): the learn as two launches so its
        # Adam half can share the chip with the next step's side-stream work
        # (overlap "full").  Off by default: measured at C2 (round 3), the
        # overlapped sim / act ran 2x / 6x slower beside the bandwidth-bound
        # Adam and the step lost 3 % (3.01 vs 3.09 M steps/s).
        if split_learn:
            self.agent.set_split_learn(True)
        # fused: act + env step + remember as one launch (TrafficEnv.step_fused)
        # on the one-stream schedules; "full" splits them across its streams
        self.fused = bool(fused) and overlap != "full" and self.agent.ring.row_format == "int8"
        if overlap == "env" and not self.fused:
            raise ValueError('overlap "env" runs the fused env step (int8 replay rows, fused=True)')
        # overlap "env": the learn of the last `side_learn` agents runs on the
        # side stream behind the env step and the draws (its CUs idle
        # otherwise while the learn stream works), the rest on the learn
        # stream; independent agents, so the results are the same
        self.side_learn = int(side_learn)
        if self.side_learn:
            if overlap != "env":
                raise ValueError('side_learn runs with overlap "env"')
            if self.agent.shared or not 0 < self.side_learn < self.agent.NA:
                raise ValueError("side_learn: independent nets, 0 < side_learn < E*A")
        # overlap "env" at a fixed epsilon of 1 (A-1: the side stream never reads
        # a learn's output): the learn -> side-stream wait only orders the store
        # of t+2 after learn t's ring reads, so it uses ordering-only events
        # (_lib.OrderEvent, no cache write-back between the learns) from a ring
        # (more events than marks can be alive: a wait never meets a re-record).
        # "Epsilon fixed at 1" stands for "the act's greedy actions never come
        # from the nets", and a behaviour policy (AgentConfig.behavior) keeps
        # that true: while it is active the greedy actions are the rule's,
        # computed on the side stream from the observation that stream itself
        # produced, and agent.current_epsilon() -- what every condition below
        # asks -- stays the nets' schedule, which the policy does not move.
        self._war_ring = ([_lib.OrderEvent() for _ in range(max(4, self.agent.ring.spare + 2))]
                          if war_events and overlap == "env" else None)
        self._war_i = 0
        # overlap "env": (call index, event) of the learns the side stream may
        # wait for, newest last.  The store of call k overwrites the slot of
        # store k - slots, which the learns of calls up to k - 1 - spare read
        # (kernels.ReplayRing, spare = AgentConfig.ring_spare), so env step k
        # waits for the newest marked learn of a call <= k - 2 -- never learn
        # k - 1, beside which it runs.  Any learn of calls k - 1 - spare ..
        # k - 2 will do, so under ordering-only events the learn stream marks
        # every spare-th learn, and the side stream runs up to `spare` env
        # steps ahead (C3 / C2 measured faster with 2 than with a mark per
        # learn: profiles/r06/c3_marks, c2_marks).
        self._marks = []
        self._calls = 0
        self.n_marks = 0  # marked calls that learned (tests: every spare-th learn)
        self._mark_every = bool(mark_every_learn)  # A/B: a marker behind every learn
        # overlap "env": learns in pairs (pair_learns, default on).  The env
        # step, the store and the draws of a step run ahead of its learn, so a
        # learn's inputs exist one call before the next learn's do: the learn of
        # a call is begun (agent.learn_begin: its draws, buffers, Adam constants
        # and ring window are fixed) and held back, and the next call launches
        # both as one dmdqn_learn_pair -- the same bits, the second learn's
        # weights, Adam slots and target still on the chip.  _pending: the token
        # of the held-back learn; _flush_pending() launches it alone (every
        # method that hands state or outputs to the caller does).
        self.pair_learns = bool(pair_learns)
        self._pending = None
        self._pending_stream = None  # the learn stream of the call that held it back
        self._last_mark = -1  # the call of the newest mark (paired marks: see the step)
        self._held = -2       # the last call that held its learn back
        self._pairs_fixed = None
        self.obs = self.env.reset()
        self.episode = 0
        self.step_count = 0
        self.total_steps = 0
        self.last_loss = None
        self.last_reward = None
        self._debug = bool(_lib.load().dmdqn_debug_build())

    def step(self, collect_stats=False):
        """One loop iteration for every replica; collect_stats makes the learn
        also produce the metrics of dqn_agent.py:361-370 (agent.learn_metrics).
        Under the debug-bounds build (DMDQN_VARIANT=debug) every step ends with
        a device sync and the kernels' range checks."""
        # the stream this step's work (its learn among it) is queued on or
        # behind: sync_outputs() orders a read under another stream after it
        self._step_stream = torch.cuda.current_stream(self.env.device)
        st = self._step(collect_stats)
        n, r = self.agent.health_every, self.agent.redo_every
        if r > 0 and st.loss_launched and self.agent.learn_step_counter % r == 0:
            self._redo()  # (its probe is also health_every's, if that falls on this learn)
        elif n > 0 and st.loss_launched and self.agent.learn_step_counter % n == 0:
            self._probe_health()
        if self.agent.pbt is not None:
            self._pbt_after_step()
        if self._debug:
            _lib.debug_check()
        return st

    def _probe_health(self):
        """The network health probe (AgentConfig.health_every) behind the learn
        this step began, on the step's stream: sync_outputs() first launches a
        held-back paired learn and waits for a side learn, so the probe sees the
        nets and Adam slots that learn left; it reads them, that learn's index
        buffer and its ring window, and writes only agent.health.
        Under the "env" schedule the side stream runs ahead of the learn stream,
        and this is safe: the stores of the next ring_spare calls land outside
        the window the probe reads (kernels.ReplayRing), and the first store
        that lands inside it -- like the first reuse of this call's index
        buffer, ring_spare + 2 calls on -- waits for a mark of this call or a
        later one.  Later marks are recorded on the learn stream behind the
        probe; this call's own mark, if it has one, was recorded behind the
        learn and ahead of the probe, so it is recorded again here (no wait on
        it has been issued yet: the side stream waits for marks of calls two or
        more back)."""
        self.sync_outputs()
        self.agent.probe_health()
        if self.overlap == "env" and self._marks and self._marks[-1][0] == self._calls - 1:
            self._marks[-1][1].record(torch.cuda.current_stream(self.env.device))
        if self.side_learn:
            # the next side learn writes its agents' nets on the side stream,
            # which nothing else orders behind this stream's reads of them
            self.side.wait_stream(torch.cuda.current_stream(self.env.device))

    def _redo(self):
        """Dead-unit recycling (AgentConfig.redo_every) behind the learn this
        step began, on the caller's stream: the probe, then the in-place
        rewrite of the fired units' weights and Adam moments (agent.redo).  It
        writes the nets, so it runs in _pbt_round's bracket: quiesce() (a
        held-back paired learn is launched; the side stream's env step, draws
        and side learn are done with the nets, the rings and the index
        buffers) before it and join_streams() (the side stream's next work
        waits for it) after it."""
        self.quiesce()
        self.agent.redo()
        self.join_streams()

    def _pbt_after_step(self):
        """Population-based training, on the caller's stream: the step's reward
        (already recorded to it under "env") joins the window's fitness; at
        the end of a window (total_steps % interval == 0) a round runs if the
        agents have learned, and the fitness restarts either way."""
        agent = self.agent
        agent.pbt_score(self.last_reward)
        if self.total_steps % agent.pbt["interval"]:
            return
        if agent.learn_step_counter > 0:
            self._pbt_round()
        agent.fitness.zero_()

    def _pbt_round(self):
        """select -> exchange -> explore on the caller's stream, between
        quiesce() (the side stream's env step, draws and side learn are done
        with the nets) and join_streams() (its next work waits for the copy)."""
        agent = self.agent
        self.quiesce()
        fit = agent.fitness.cpu().numpy()
        src, rank = agent.pbt_select()
        agent.pbt_exchange(src)
        agent.pbt_explore(src)
        key = np.where(fit != fit, -np.inf, fit)
        order = np.argsort(rank)  # replicas, best first
        self.pbt_log.append({
            "round": agent.pbt_round, "step": self.total_steps,
            "copied": [[int(e), int(s)] for e, s in enumerate(src) if s != e],
            "best_env": int(order[0]),
            "fitness_best": float(key[order[0]]), "fitness_median": float(np.median(key)),
            "fitness_worst": float(key[order[-1]]),
            "values": agent.pbt_population()})
        agent.pbt_round += 1
        self.join_streams()

    def _step(self, collect_stats):
        if self.overlap == "full":
            return self._step_overlap(collect_stats)
        if self.overlap == "env":
            return self._step_env_beside_learn(collect_stats)
        if self.overlap == "sample":
            return self._step_side_sample(collect_stats)
        if self.overlap == "learn":
            return self._step_sample_beside_learn(collect_stats)
        env, agent = self.env, self.agent
        next_obs, reward, done, info = self._env_side()
        loss = agent.learn(collect_stats=collect_stats)
        self.last_loss, self.last_reward = loss, reward
        self.obs = self._after_step(done, next_obs, info)
        return StepStats(loss is not None, done)

    def _env_side(self):
        """act -> env step -> remember (train.py:211-282), fused or as three calls."""
        env, agent = self.env, self.agent
        if self.fused:
            eps, greedy, out = agent.act_inputs(self.obs)
            # (store_ring: agent.ring, or the staging ring of n-step returns)
            res = env.step_fused(agent.np_state, eps, greedy, out, agent.store_ring, self.obs)
            agent.remembered()
            return res
        actions = agent.act(self.obs)                          # train.py:211-222
        next_obs, reward, done, info = env.step(actions)       # train.py:225-270
        agent.remember(self.obs, actions, reward, next_obs, info["done"])  # train.py:274-282
        return next_obs, reward, done, info

    def _step_side_sample(self, collect_stats):
        env, agent, side = self.env, self.agent, self.side
        main = torch.cuda.current_stream(env.device)
        if self._join:
            side.wait_stream(main)
            self._join = False
        elif self._ev_learn is not None:
            side.wait_event(self._ev_learn)  # learn t-1 done: nothing beside the next learn
        ev_s = None
        with torch.cuda.stream(side):
            if agent.presample(min(agent.ring.total + 1, agent.ring.cap)):
                ev_s = torch.cuda.Event()
                ev_s.record(side)
        next_obs, reward, done, info = self._env_side()
        if ev_s is not None:
            main.wait_event(ev_s)
        loss = agent.learn(collect_stats=collect_stats)
        self._ev_learn = torch.cuda.Event()
        self._ev_learn.record(main)
        self.last_loss, self.last_reward = loss, reward
        self.obs = self._after_step(done, next_obs, info)
        return StepStats(loss is not None, done)

    def _step_sample_beside_learn(self, collect_stats):
        env, agent, side = self.env, self.agent, self.side
        main = torch.cuda.current_stream(env.device)
        if self._join:
            side.wait_stream(main)
            self._join = False
        elif self._ev_env_prev is not None:
            # env step t-1 done: these draws run beside learn t-1.  They read
            # only the CPython stream and the ring length after this step's
            # store; the index buffer they fill was last read three learns
            # back (agent.OUT_BUFS rotation), before env step t-1
            side.wait_event(self._ev_env_prev)
        ev_s = None
        with torch.cuda.stream(side):
            if agent.presample(min(agent.ring.total + 1, agent.ring.cap),
                               lds_budget=self._sampler_lds):
                ev_s = torch.cuda.Event()
                ev_s.record(side)
        next_obs, reward, done, info = self._env_side()
        self._ev_env_prev = torch.cuda.Event()
        self._ev_env_prev.record(main)
        if ev_s is not None:
            main.wait_event(ev_s)
        loss = agent.learn(collect_stats=collect_stats)
        self.last_loss, self.last_reward = loss, reward
        self.obs = self._after_step(done, next_obs, info)
        return StepStats(loss is not None, done)

    def _step_overlap(self, collect_stats):
        env, agent, side = self.env, self.agent, self.side
        main = torch.cuda.current_stream(env.device)
        if self._join:  # first step, or the caller touched state on its stream
            side.wait_stream(main)
            self._join = False
        elif self._ev_store is not None:
            side.wait_event(self._ev_store)  # remember t-1 has read obs/actions/reward
        if agent.current_epsilon() < 1.0 and self._ev_learn is not None:
            side.wait_event(self._ev_learn)  # greedy act reads the updated weights
        with torch.cuda.stream(side):
            actions = agent.act(self.obs)                          # train.py:211-222
            next_obs, reward, done, info = env.step(actions)       # train.py:225-270
            agent.presample(min(agent.ring.total + 1, agent.ring.cap))
            ev_obs = torch.cuda.Event()
            ev_obs.record(side)
        main.wait_event(ev_obs)
        for t in (self.obs, next_obs, reward, env.local):
            t.record_stream(main)  # side-allocated, read on main
        agent.remember(self.obs, actions, reward, next_obs, info["done"])  # train.py:274-282
        self._ev_store = torch.cuda.Event()
        self._ev_store.record(main)
        loss = agent.learn(collect_stats=collect_stats)
        self._ev_learn = torch.cuda.Event()
        self._ev_learn.record(main)
        self.last_loss, self.last_reward = loss, reward
        self.obs = self._after_step(done, next_obs, info, side=side, main=main)
        return StepStats(loss is not None, done)

    def _step_env_beside_learn(self, collect_stats):
        env, agent, side = self.env, self.agent, self.side
        main = torch.cuda.current_stream(env.device)
        if self._join:  # first step, or the caller touched state on its stream
            side.wait_stream(main)
            self._join = False
        k = self._calls
        self._calls += 1
        spare = agent.ring.slots - agent.ring.cap
        if self._held == k - 1 and self._pending is None and pair_mark_due(
                k - 1, self._last_mark, spare, self._mark_every):
            # paired learns: call k - 1 held its learn back (no mark then) and
            # the caller has had it launched since (last_loss, sync_outputs,
            # ...): its mark, due by the rule below, goes behind that launch now
            # (on the stream that launch went to: the learn stream of call k - 1)
            ev = self._war_ring[self._war_i]
            self._war_i = (self._war_i + 1) % len(self._war_ring)
            ev.record(self._pending_stream or main)
            self._ev_learn = ev
            self._marks.append((k - 1, ev))
            self._last_mark = k - 1
            self.n_marks += 1
        marks = [m for m in self._marks if m[0] <= k - 2]
        if k - 1 - spare >= 0 and not (marks and marks[-1][0] >= k - 1 - spare):
            # (every call k' has a mark in [k' - 1 - spare, k' - 2]: see below)
            raise RuntimeError(f"env schedule: no mark covers call {k - 1 - spare}")
        if marks:
            j, ev = marks[-1]
            # call k - 1 - spare must be covered -- its learn's ring reads and
            # the caller's reads of its outputs, queued on main before the mark
            # of any later call (the main stream is in order: the wait covers
            # every earlier call too)
            if isinstance(ev, _lib.OrderEvent):
                ev.wait(side)
            else:
                side.wait_event(ev)
        self._marks = [m for m in self._marks if m[0] >= k - 1 - spare]
        if agent.current_epsilon() < 1.0 and self._ev_learn is not None:
            # greedy act reads the updated weights (recorded as a full event:
            # an ordering-only one is used only while epsilon is fixed at 1)
            side.wait_event(self._ev_learn)
        with torch.cuda.stream(side):
            next_obs, reward, done, info = self._env_side()
            agent.presample(len(agent.ring))
            self.obs = self._after_step(done, next_obs, info)  # (an episode reset: on side)
            ev_env = torch.cuda.Event()
            ev_env.record(side)
        tok = agent.learn_begin(collect_stats)  # the draws above, the Adam constants
        learned = bool(tok)
        ev_side = None
        if learned and self.side_learn:
            with torch.cuda.stream(side):
                agent.learn_range(agent.NA - self.side_learn, agent.NA)
                ev_side = torch.cuda.Event()
                ev_side.record(side)
        main.wait_event(ev_env)  # the store learn t reads; what the caller reads after step()
        # side-allocated outputs the caller reads on main: without
        # this the allocator could hand their blocks to step t+2's side work
        # while a main-stream read of them is still queued
        for t in (next_obs, reward, env.local, self.obs):
            t.record_stream(main)
        war = (self._war_ring is not None and not agent.cfg.count_env_steps
               and agent.current_epsilon() >= 1.0)
        loss = None
        pairing = war and self._pairs()
        if self._pending is not None and self._pending_stream != main:
            # the caller changed streams between two calls: the held-back learn
            # goes to the learn stream it was begun for, and this one follows it
            self._flush_pending()
        if not pairing or not learned:
            self._flush_pending()
            if learned:
                loss = agent.learn_range(0, agent.NA - self.side_learn)
        else:
            # this learn may share a launch: no metrics, no timing hook (it
            # brackets single launches), no hard sync (another compile-time
            # variant of the kernel)
            plain = not (collect_stats or agent.learn_hook or tok.sync)
            pend, self._pending = self._pending, None
            loss = tok.loss
            what = pair_action(pend is not None, plain, tok.next_sync)
            if what == "pair":
                agent.learn_pair_range(pend, tok, 0, agent.NA)
            elif what == "both":
                agent.learn_range(0, agent.NA, pend)
                agent.learn_range(0, agent.NA, tok)
            elif what == "hold":
                # the next call launches it with its own learn (the loss buffer
                # is filled then; last_loss launches it at once)
                self._pending = tok
                self._pending_stream = main
                self._held = k
            else:
                agent.learn_range(0, agent.NA, tok)
        if self._pending is not None:
            # No mark can follow a learn that is not launched: a mark of call j
            # stands behind the launch that holds learn j (the side stream's
            # store of call j + 1 + spare, and its reuse of call j's index
            # buffer, wait for it).  The next call launches and may mark.
            pass
        elif pairing:
            # Marks with held-back learns: a launching call k marks when the
            # newest mark is of call k - (spare - 1) or older.  A held-back
            # call k is followed by a launching call k + 1, or its learn is
            # launched for the caller in between and call k + 1 marks for it
            # first (at the top): of two calls in a row one can be marked, so
            # two marks are at most `spare` calls apart and every window
            # [k' - 1 - spare, k' - 2] holds one (checked at the top of each
            # call): the side stream runs at most spare - 1 steps ahead of a
            # held-back learn.
            if pair_mark_due(k, self._last_mark, spare, self._mark_every):
                ev = self._war_ring[self._war_i]
                self._war_i = (self._war_i + 1) % len(self._war_ring)
                ev.record(main)
                self._ev_learn = ev
                self._marks.append((k, ev))
                self._last_mark = k
                self.n_marks += learned
        elif war and spare >= 2 and not self._mark_every and k % spare:
            # under ordering-only events only every spare-th call is marked
            # (whether or not it learned: the mark also orders the side
            # stream's reuse of the per-step output buffers after the caller's
            # reads of them): any `spare` consecutive calls hold a mark, so
            # the newest mark of a call <= k' - 2 always covers call
            # k' - 1 - spare (checked above)
            pass
        elif war:
            # epsilon cannot fall below 1 later (count_env_steps off): no act
            # will read this learn's weights through the side stream.  What the
            # side stream reads of main's work is then nothing: the side learn
            # (side_learn) reads only its own agents' weights, rings and draws,
            # all written on the side stream -- so an ordering-only event
            # (write after read: the store of t+2 after learn t's ring reads)
            # is enough.  A data hand-over main -> side takes a full event.
            if not self._side_reads_nothing_from_main():  # (not an assert: kept under -O)
                raise RuntimeError("ordering-only learn event with a read-after-write hazard")
            ev = self._war_ring[self._war_i]
            self._war_i = (self._war_i + 1) % len(self._war_ring)
            ev.record(main)
            self._ev_learn = ev
            self._marks.append((k, ev))
            self._last_mark = k
            self.n_marks += learned
        else:
            self._ev_learn = torch.cuda.Event()
            self._ev_learn.record(main)
            self._marks.append((k, self._ev_learn))
            self._last_mark = k
            self.n_marks += learned
        # the side learn's outputs (its agents' loss, stats and weights) for the
        # caller's stream.  The next learn needs no wait for them: the side
        # stream runs the next env step behind the side learn, and the next
        # learn waits for that.  So a step with stats (their readers follow at
        # once) waits here; otherwise the wait is left to the caller's reads
        # (the last_loss property, sync_outputs()) -- a barrier packet less per
        # step on the learn stream (C2 +2.5 %)
        self._side_pending = None
        if ev_side is not None:
            if collect_stats:
                main.wait_event(ev_side)
            else:
                self._side_pending = ev_side
        self.last_loss, self.last_reward = loss, reward
        return StepStats(loss is not None, done)

    def _pairs(self):
        """Whether the "env" schedule runs its learns in pairs: the option, and
        what dmdqn_learn_pair takes -- 16-bit independent nets on int8 rows in
        one fused launch on the learn stream (no side learn, no split learn) --
        with at least two spare ring slots (a held-back learn lags its store by
        one more call) and without the agent's diagnostics buffers (rn_out,
        stamps: one buffer each, read after the step that wrote it)."""
        ag = self.agent
        if self._pairs_fixed is None:  # what cannot change after construction
            self._pairs_fixed = (
                self.pair_learns and self.overlap == "env" and not ag.shared
                and ag.cfg.precision in ("fp16", "bf16") and ag.ring.row_format == "int8"
                and ag.ring.slots - ag.ring.cap >= 2 and not self.side_learn)
        return (self._pairs_fixed and ag.rn_out is None and ag.stamps is None
                and not ag.split_learn)

    def _flush_pending(self):
        """Launch a held-back learn (paired learns) alone, on the learn stream of
        the call that began it -- where its env step and draws were waited for,
        where the next learns follow it and where its mark is recorded -- and
        make the current stream, if it is another one, wait for it."""
        pend, self._pending = self._pending, None
        if pend is None:
            return
        stream = self._pending_stream
        cur = torch.cuda.current_stream(self.env.device)
        with torch.cuda.stream(stream):
            self.agent.learn_range(0, self.agent.NA, pend)
        if cur != stream:
            ev = torch.cuda.Event()
            ev.record(stream)
            cur.wait_event(ev)

    @property
    def last_loss(self):
        """The last learn's per-agent losses (None before the first learn),
        complete on the caller's current stream."""
        self.sync_outputs()
        return self._last_loss

    @last_loss.setter
    def last_loss(self, v):
        self._last_loss = v

    def sync_outputs(self):
        """Make the agent's loss, stats and weights complete for reads on the
        current stream.  Schedule "env" with paired learns: a held-back learn
        is LAUNCHED now (a kernel, on the learn stream of the step that began
        it; the current stream waits for it) -- so a loop that calls this, or
        reads last_loss, after every step never pairs.  With side_learn: the
        current stream waits for the last step's side-stream learn.  Called
        under another stream than the last step's: the current stream waits
        for what that step queued (a learn launched within the step is not
        otherwise ordered before a read there).  A no-op otherwise."""
        if getattr(self, "_pending", None) is not None:
            self._flush_pending()
        last = getattr(self, "_step_stream", None)
        if last is not None:
            cur = torch.cuda.current_stream(self.env.device)
            if cur != last:
                ev = torch.cuda.Event()
                ev.record(last)
                cur.wait_event(ev)
        if getattr(self, "_side_pending", None) is not None:
            torch.cuda.current_stream(self.env.device).wait_event(self._side_pending)

    def _side_reads_nothing_from_main(self):
        """The "env" schedule's invariant for ordering-only learn events: no
        greedy act (its forward reads the learn stream's weights) and the side
        learn's agent range [NA - side_learn, NA) disjoint from the learn
        stream's [0, NA - side_learn) (no side learn for the shared net, whose
        one learn reads every agent)."""
        ag = self.agent
        return (ag.current_epsilon() >= 1.0 and not ag.cfg.count_env_steps
                and 0 <= self.side_learn < ag.NA and not (ag.shared and self.side_learn))

    def _after_step(self, done, next_obs, info, side=None, main=None):
        """Counters and the observation the next act sees (train.py:188-209).
        Replicas that restart on their own `done` (env.drains_early) were reset
        by env.step itself: info["obs_next"] already holds their restart state.
        Otherwise every replica ends together, and the whole batch reloads."""
        env, agent = self.env, self.agent
        self.step_count += 1
        self.total_steps += 1
        if "obs_next" in info:
            if info["restarted"].any():
                agent.ring.check()  # episode boundary: every store so far was exact
                self.episode = int(env.env_episodes.min())
                self.step_count = int(env.env_steps.min())
            return info["obs_next"]
        if not done:
            return next_obs
        agent.ring.check()  # episode boundary: every store so far was exact
        self.episode += 1                                      # train.py:188-190
        self.step_count = 0
        if side is None:
            return env.reset()
        with torch.cuda.stream(side):
            obs = env.reset()
        main.wait_stream(side)
        obs.record_stream(main)
        env.local.record_stream(main)
        return obs

    def join_streams(self):
        """Call after changing trainer state on the caller's stream between
        steps (checkpoint restore, weight loads): the next step's side-stream
        work then waits for it.  Also orders the caller's stream after the
        last side-stream learn (schedule "env" with side_learn), so later
        caller-side writes cannot race it; call quiesce() BEFORE such writes."""
        self.sync_outputs()
        self._side_pending = None
        self._join = True

    def quiesce(self):
        """Order the caller's stream after every piece of trainer work queued
        so far on any stream (the side stream's env step, draws and side
        learn), so the caller may overwrite trainer state on it (checkpoint
        restore).  No host block."""
        self.sync_outputs()
        self._side_pending = None
        if self.side is not None:
            torch.cuda.current_stream(self.env.device).wait_stream(self.side)

    def variant_rewards(self):
        """Per sweep variant, the mean over its replicas of the last step's
        total reward (last_reward.sum(dim=1), train.py:254's sum over
        junctions); None for a variant without replicas, [] before the first
        step.  Syncs."""
        if self.last_reward is None:
            return []
        total = self.last_reward.double().sum(dim=1).cpu()
        voe = self.agent.variant_of_env
        return [float(total[voe == i].mean()) if bool((voe == i).any()) else None
                for i in range(len(self.agent.variants))]

    def variant_rewards_device(self):
        """variant_rewards() as a float64 [G] tensor on the device (NaN for a
        variant without replicas), queued on the current stream: no copy to
        the host and no sync, so a loop can accumulate it every step and read
        it once.  The sums run in another order than variant_rewards()'s, so
        the last bits may differ."""
        if getattr(self, "_variant_weights", None) is None:
            voe, G = self.agent.variant_of_env, len(self.agent.variants)
            w = (voe[None, :] == torch.arange(G)[:, None]).double()  # [G, E] membership
            n = w.sum(dim=1, keepdim=True)
            w = torch.where(n > 0, w / n.clamp(min=1), torch.full_like(w, float("nan")))
            self._variant_weights = w.to(self.env.device)
        total = self.last_reward.double().sum(dim=1)
        return (self._variant_weights * total[None, :]).sum(dim=1)

    def agent_env_steps(self, n_steps):
        return n_steps * self.env.E * self.env.A

    def synchronize(self):
        """Wait for all device work, and (C5 over RCCL) first for every
        outstanding gradient all-reduce, bounded: a peer that stalled on or
        skipped one raises DistError instead of hanging the synchronize."""
        self.sync_outputs()  # (a held-back learn of the paired "env" schedule is launched)
        self.agent.drain_collectives()
        torch.cuda.synchronize(self.env.device)
