"""Rule-based controllers on the GPU: dmdqn_act_rule bit for bit against the
numpy restatement (rule_ref.py) through ctypes and the operator, on random
observations, the shared fixture and a real TrafficEnv; the host refusals; the
evaluation modes; and Trainers whose behaviour policy equals a hand loop and is
bit-identical across schedules and across a checkpoint."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import rule_ref as RR  # noqa: E402
from dmdqn_amd import checkpoint as CK  # noqa: E402
from dmdqn_amd import evaluate as EV  # noqa: E402
from dmdqn_amd import kernels as K  # noqa: E402
from dmdqn_amd._lib import call, stream_of  # noqa: E402
from dmdqn_amd.agent import AgentConfig  # noqa: E402
from dmdqn_amd.env import EnvConfig, TrafficEnv  # noqa: E402
from dmdqn_amd.trainer import Trainer  # noqa: E402

DEV = "cuda"
RULES = (("longest_queue", RR.LONGEST_QUEUE), ("max_pressure", RR.MAX_PRESSURE))
CANARY, PAD = -559038737, 8  # 0xDEADBEEF as int32; guard words on each side


def _ctypes_rule(obs, R, C_, rule, want_score=True):
    """dmdqn_act_rule through ctypes into buffers with PAD canary words before
    and after (the score pointer is then only 4-byte aligned past a 32-B
    offset, the actions pointer too); returns (actions, score or None)."""
    E, A = obs.shape[:2]
    NA = E * A
    act = torch.full((NA + 2 * PAD,), CANARY, dtype=torch.int32, device=DEV)
    sc = torch.full((4 * NA + 2 * PAD + 1,), CANARY, dtype=torch.int32, device=DEV)
    sc_ptr = C.c_void_p(sc.data_ptr() + 4 * (PAD + 1)) if want_score else None
    call("dmdqn_act_rule", R, C_, E, rule, C.c_void_p(obs.data_ptr()),
         C.c_void_p(act.data_ptr() + 4 * PAD), sc_ptr, stream_of())
    torch.cuda.synchronize()
    act, sc = act.cpu().numpy(), sc.cpu().numpy()
    assert (act[:PAD] == CANARY).all() and (act[PAD + NA:] == CANARY).all(), "actions canary"
    if want_score:
        assert (sc[:PAD + 1] == CANARY).all() and (sc[PAD + 1 + 4 * NA:] == CANARY).all(), \
            "score canary"
        return act[PAD:PAD + NA].reshape(E, A), sc[PAD + 1:PAD + 1 + 4 * NA].reshape(E, A, 4)
    assert (sc == CANARY).all()
    return act[PAD:PAD + NA].reshape(E, A), None


def _check_all(obs_host, R, C_):
    obs = torch.from_numpy(obs_host).to(DEV).contiguous()
    for name, rule in RULES:
        want_a, want_s = RR.act_rule(obs_host, rule)
        got_a, got_s = _ctypes_rule(obs, R, C_, rule)
        assert np.array_equal(got_s, want_s), (name, R, C_, obs_host.shape)
        assert np.array_equal(got_a, want_a), (name, R, C_, obs_host.shape)
        # without the score output: the same actions
        none_a, _ = _ctypes_rule(obs, R, C_, rule, want_score=False)
        assert np.array_equal(none_a, want_a)
        # the operator, bit-identical to the ctypes call
        out = torch.full(obs.shape[:2], CANARY, dtype=torch.int32, device=DEV)
        sc = torch.full(obs.shape[:2] + (4,), CANARY, dtype=torch.int32, device=DEV)
        assert K.act_rule(obs, R, C_, name, out=out, score=sc) is out
        assert np.array_equal(out.cpu().numpy(), got_a) and np.array_equal(sc.cpu().numpy(), got_s)
        assert np.array_equal(K.act_rule(obs, R, C_, rule).cpu().numpy(), got_a)


# --------------------------------------------------------------------------- 1. the kernel
@pytest.mark.parametrize("R,C_", [(1, 1), (1, 3), (3, 1), (2, 2), (3, 3)])
def test_kernel_is_the_restatement_bit_for_bit(R, C_):
    """E*A from 1 to 63: fewer agents than the 8 groups of a block, more than
    one block, and mostly no multiple of 8 (tail groups); counts 0..24, -1
    padding."""
    rng = np.random.default_rng(10 * R + C_)
    for E in (1, 3, 7):
        _check_all(RR.random_obs(rng, R, C_, E), R, C_)


def test_kernel_on_the_fixture_and_known_answers():
    for R, C_, obs in RR.check_fixture(RR.fixture_parts()):
        _check_all(obs, R, C_)
    for row, rule, want_sc, want_a in RR.known_rows():
        got_a, got_s = _ctypes_rule(torch.from_numpy(row).to(DEV).view(1, 1, 89), 1, 1, rule)
        assert got_s.reshape(4).tolist() == want_sc and got_a.item() == want_a


def test_kernel_on_arbitrary_rows_and_many_blocks():
    """Every value of the int8 range in every position, flags that are neither
    0 nor 1, and E*A = 1003 agents: 126 blocks, the last with 3 live groups."""
    rng = np.random.default_rng(3)
    obs = rng.integers(-127, 128, size=(59, 17, 89)).astype(np.float32)
    obs[..., 17:21] = rng.integers(-1, 3, size=(59, 17, 4))
    _check_all(obs, 1, 17)


def test_real_environment_observations():
    env = TrafficEnv(EnvConfig(rows=2, cols=2, num_envs=4, seed=11, max_sim_time=600))
    np_state = K.seed_streams(env.seeds, "np", DEV)
    obs = env.reset()
    seen = 0
    for _ in range(20):
        host = obs.cpu().numpy()
        for name, rule in RULES:
            want_a, want_s = RR.act_rule(host, rule)
            sc = torch.empty((4, 4, 4), dtype=torch.int32, device=DEV)
            got = K.act_rule(obs, 2, 2, name, score=sc)
            assert np.array_equal(got.cpu().numpy(), want_a)
            assert np.array_equal(sc.cpu().numpy(), want_s)
        seen += int(host[..., :12].sum())
        obs, _, _, info = env.step(K.act(np_state, 4, uniform=True))
        obs = info.get("obs_next", obs)
    assert seen > 0  # queues formed: the scores were not all zero


def test_refused_arguments_launch_nothing():
    obs = torch.zeros((2, 4, 89), device=DEV)
    out = torch.full((2, 4), CANARY, dtype=torch.int32, device=DEV)
    sc = torch.full((2, 4, 4), CANARY, dtype=torch.int32, device=DEV)
    # refused by the C entry point: its message is raised
    for (R, C_, rule), msg in (((0, 4, 0), "dmdqn_act_rule: grid 0x4"),
                               ((4, -1, 0), "dmdqn_act_rule: grid 4x-1"),
                               ((2, 2, 2), "dmdqn_act_rule: unknown rule 2"),
                               ((2, 2, -1), "dmdqn_act_rule: unknown rule -1")):
        with pytest.raises(RuntimeError, match=msg):
            K.act_rule(obs, R, C_, rule, out=out, score=sc)
    with pytest.raises(RuntimeError, match="must be >= 1"):
        K.act_rule(obs[:0], 2, 2, 0, out=out[:0], score=None)
    # refused by the operator's own checks
    for bad, msg in ((dict(obs=obs[..., :88].contiguous()), "obs must be"),
                     (dict(obs=obs[:, :3].contiguous()), "obs must be"),
                     (dict(obs=obs.double()), "obs must be Float"),
                     (dict(obs=obs.transpose(0, 1)), "obs must be|contiguous"),
                     (dict(out=out.long()), "actions must be Int"),
                     (dict(out=out[:1]), "actions has"),
                     (dict(score=sc[:, :, :3].contiguous()), "score has"),
                     (dict(obs=obs.cpu()), "device|backend")):
        kw = dict(obs=obs, out=out, score=sc)
        kw.update(bad)
        with pytest.raises((RuntimeError, NotImplementedError), match=msg):
            K.act_rule(kw["obs"], 2, 2, 1, out=kw["out"], score=kw["score"])
    with pytest.raises(ValueError, match="unknown rule"):
        K.act_rule(obs, 2, 2, "fifo", out=out)
    torch.cuda.synchronize()
    assert bool((out == CANARY).all()) and bool((sc == CANARY).all())


# --------------------------------------------------------------------------- 2. evaluation
EVAL_CFG = EnvConfig(rows=2, cols=2, max_sim_time=150)


def _host_loop(mode, episodes, seed0, max_steps):
    """run_mode's bookkeeping with the restatement's actions fed to env.step."""
    from dataclasses import replace
    cfg = replace(EVAL_CFG, num_envs=episodes, seed=seed0, env_offset=0)
    env = TrafficEnv(cfg)
    E, A = env.E, env.A
    obs = env.reset()
    total, qsum = np.zeros(E), np.zeros(E)
    steps = np.zeros(E, dtype=np.int64)
    ended = np.zeros(E, dtype=bool)
    for _ in range(max_steps):
        host = obs.cpu().numpy()
        act, _ = RR.act_rule(host, RR.RULE_NAMES[mode])
        live = ~ended
        qsum += live * host[..., :12].astype(np.float64).sum(axis=(1, 2))
        nxt, reward, done, info = env.step(torch.from_numpy(act).to(DEV))
        total += live * reward.sum(dim=1).cpu().numpy()
        steps[live] += 1
        if "obs_next" in info:
            ended |= info["restarted"]
            obs = info["obs_next"]
        else:
            obs = nxt
            if done:
                ended[:] = True
        if ended.all():
            break
    return total, qsum / (steps * A), steps


@pytest.mark.parametrize("mode", ["longest_queue", "max_pressure", "program"])
def test_eval_modes(mode):
    rows = EV.run_mode(EVAL_CFG, mode, episodes=2, eval_seed_start=300, max_steps=12)
    again = EV.run_mode(EVAL_CFG, mode, episodes=2, eval_seed_start=300, max_steps=12)
    assert rows == again and len(rows) == 2
    for r in rows:
        assert r["mode"] == mode and r["steps"] == 12
        assert all(np.isfinite(r[k]) for k in ("total_reward", "avg_reward_per_agent",
                                               "avg_step_queue_sum"))
    assert any(r["avg_step_queue_sum"] > 0 for r in rows)
    if mode != "program":
        total, qavg, steps = _host_loop(mode, 2, 300, 12)
        for e, r in enumerate(rows):
            assert r["total_reward"] == float(total[e]) and r["steps"] == int(steps[e])
            assert r["avg_step_queue_sum"] == float(qavg[e])
    assert not EV.summarize(rows).isna().any().any()


def test_eval_program_mode_sets_no_phase():
    """'program' hands the sim -1 everywhere: the junctions' phases are those of
    an env that only advances (no setPhase), not those of any fixed action."""
    from dataclasses import replace
    cfg = replace(EVAL_CFG, num_envs=2, seed=300)
    a, b = TrafficEnv(cfg), TrafficEnv(cfg)
    a.reset(), b.reset()
    none = torch.full((2, 4), -1, dtype=torch.int32, device=DEV)
    for _ in range(6):
        a.step(none)
        b.advance()
        assert torch.equal(a.phase, b.phase) and torch.equal(a.halt, b.halt)
    assert int(a.phase.max()) > 0  # the program moved on by itself
    with pytest.raises(ValueError, match="unknown mode"):
        EV.run_mode(EVAL_CFG, "fifo", episodes=1)


# --------------------------------------------------------------------------- 3. the Trainer
E_TR, STEPS, SWITCH, CKPT_AT, EPS = 4, 140, 12, 8, 0.25
TR_STATE = ("params", "adam_m", "adam_v", "target", "target_h", "np_state", "py_state")


def _trainer(overlap="none", fused=True, env_kw=None, **kw):
    agent = dict(precision="fp16", replay_buffer_size=200, seed=9, target_update_frequency=5)
    agent.update(kw)
    return Trainer(EnvConfig(rows=2, cols=2, num_envs=E_TR, seed=9, max_sim_time=600,
                             **(env_kw or {})),
                   AgentConfig(**agent), overlap=overlap, fused=fused)


def _run(tr, steps, ckpt=None, at=CKPT_AT, actions=None):
    for t in range(1, steps + 1):
        tr.step()
        if actions is not None:
            tr.sync_outputs()
            actions.append(tr.agent.actions.clone())
        if ckpt is not None and t == at:
            CK.save(ckpt, tr)
    tr.synchronize()


def _same(a, b, what):
    for k in TR_STATE:
        x, y = getattr(a.agent, k), getattr(b.agent, k)
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8)), f"{what}: {k}"
    for k in ("s", "n", "a", "r", "d"):
        x, y = getattr(a.agent.ring, k), getattr(b.agent.ring, k)
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8)), f"{what}: ring.{k}"
    assert torch.equal(a.obs, b.obs), what
    assert a.agent.learn_step_counter == b.agent.learn_step_counter, what
    assert a.agent.behavior_step_count == b.agent.behavior_step_count, what


BEHAVIOR = dict(behavior="max_pressure", behavior_steps=SWITCH, behavior_eps=EPS)


@pytest.fixture(scope="module")
def main_run(tmp_path_factory):
    """"none", fused, the policy for the first SWITCH steps; every step's
    actions beside a hand loop's (act_rule -> act with behavior_eps on a copy
    of the act stream, then the ordinary act at epsilon 1)."""
    path = str(tmp_path_factory.mktemp("rule") / "mid.pt")
    tr = _trainer(**BEHAVIOR)
    ag = tr.agent
    np_state = ag.np_state.clone()
    got, hand, active, rule = [], [], [], []
    for t in range(STEPS):
        obs = tr.obs.clone()
        active.append(ag.behavior_active())
        if t < SWITCH:
            greedy = K.act_rule(obs, 2, 2, "max_pressure")
            rule.append(greedy)
            hand.append(K.act(np_state, ag.A, eps=EPS, greedy=greedy))
        else:
            hand.append(K.act(np_state, ag.A, eps=1.0))
        tr.step()
        got.append(ag.actions.clone())
        if t + 1 == CKPT_AT:
            CK.save(path, tr)
    tr.synchronize()
    return tr, path, got, hand, active, rule


def test_policy_actions_equal_the_hand_loop(main_run):
    tr, _, got, hand, active, rule = main_run
    assert active == [t < SWITCH for t in range(STEPS)]
    for t in range(STEPS):
        assert torch.equal(got[t], hand[t]), t
    # the phase is the rule's play with some uniform actions: of SWITCH * 16
    # agent-steps about 1 - EPS * 3 / 4 = 0.81 take the rule's action
    share = float(torch.stack([got[t] == rule[t] for t in range(SWITCH)]).float().mean())
    print("share of the rule's actions in the phase", share)
    assert 0.6 < share < 1.0
    ag = tr.agent
    assert ag.learn_step_counter == STEPS - 127 and ag.behavior_step_count == STEPS
    rec = ag.learn_metrics()
    assert rec["behavior"] == {"policy": "max_pressure", "eps": EPS, "active": False}
    assert rec["epsilon"] == 1.0  # the nets' schedule is not the policy's


def test_schedules_are_bit_identical(main_run):
    ref = main_run[0]
    for what, kw in (("unfused", dict(fused=False)), ("env", dict(overlap="env"))):
        tr = _trainer(**kw, **BEHAVIOR)
        _run(tr, STEPS)
        _same(ref, tr, what)
    assert tr.side is not None and tr.agent.pair_launches > 2  # "env" still pairs its learns


def test_checkpoint_resume_straddles_the_switch(main_run):
    ref, path = main_run[0], main_run[1]
    st = torch.load(path, map_location="cpu", weights_only=True)
    assert st["behavior"] == {"steps_taken": CKPT_AT} and CKPT_AT < SWITCH
    assert st["agent_cfg"]["behavior"] == "max_pressure"
    tr = _trainer(overlap="env", **BEHAVIOR)
    CK.load(path, tr)
    assert tr.agent.behavior_active() and tr.agent.behavior_step_count == CKPT_AT
    _run(tr, STEPS - CKPT_AT)
    _same(ref, tr, "resumed")
    for other in (dict(behavior=None), dict(BEHAVIOR, behavior="longest_queue"),
                  dict(BEHAVIOR, behavior_steps=SWITCH + 1), dict(BEHAVIOR, behavior_eps=0.5)):
        with pytest.raises(ValueError, match="behavior"):
            CK.load(path, _trainer(**other))


def test_behavior_none_is_the_run_without_the_keys():
    """behavior=None with the other two keys set: the nets, rings, streams and
    every step's actions of a Trainer built without any of the keys -- whose
    actions are the ordinary act's at epsilon 1."""
    plain = Trainer(EnvConfig(rows=2, cols=2, num_envs=E_TR, seed=9, max_sim_time=600),
                    AgentConfig(precision="fp16", replay_buffer_size=200, seed=9,
                                target_update_frequency=5), overlap="env")
    a_plain, a_off = [], []
    np_state = plain.agent.np_state.clone()
    _run(plain, STEPS, actions=a_plain)
    off = _trainer(overlap="env", behavior=None, behavior_steps=7, behavior_eps=0.9)
    _run(off, STEPS, actions=a_off)
    _same(plain, off, "behavior=None")
    for t in range(STEPS):
        assert torch.equal(a_plain[t], a_off[t]), t
        assert torch.equal(a_plain[t], K.act(np_state, plain.agent.A, eps=1.0)), t
    assert not off.agent.behavior_active() and "behavior" not in off.agent.learn_metrics()
    st = CK.trainer_state(off)
    assert "behavior" not in st


def test_eps_zero_stores_the_rule_actions():
    """behavior_eps = 0, the whole run: every stored action is the rule's for
    the observation stored with it."""
    n = 30
    tr = _trainer(behavior="longest_queue", behavior_steps=0, behavior_eps=0.0)
    want = []
    for _ in range(n):
        want.append(RR.act_rule(tr.obs.cpu().numpy(), RR.LONGEST_QUEUE)[0].reshape(-1))
        tr.step()
    tr.synchronize()
    ag = tr.agent
    assert ag.behavior_active() and ag.ring.total == n
    stored = ag.ring.a[:, :n].cpu().numpy()
    assert np.array_equal(stored, np.stack(want, axis=1).astype(stored.dtype))
    assert len({int(x) for x in stored.reshape(-1)}) > 1


@pytest.mark.parametrize("what,kw", [
    ("shared", dict(shared_params=True)),
    ("sweep", dict(sweep={"learning_rate": [1e-4, 1e-3]})),
    ("pbt", dict(sweep={"learning_rate": [1e-4, 1e-3]}, pbt={"interval": 135, "seed": 3})),
    ("nstep", dict(n_step=3)),
])
def test_policy_runs_with_the_other_features(what, kw):
    """The rule needs no net: a short run of each, whole-run policy, learns
    included, "none" against "env"."""
    cfg = dict(behavior="max_pressure", behavior_steps=0, behavior_eps=0.1, **kw)
    a = _trainer(**cfg)
    _run(a, 136)
    b = _trainer(overlap="env", **cfg)
    _run(b, 136)
    _same(a, b, what)
    assert a.agent.learn_step_counter > 0 and a.agent.behavior_active()
    assert bool(torch.isfinite(a.last_loss).all())
