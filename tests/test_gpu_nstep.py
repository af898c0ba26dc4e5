"""GPU: n-step returns (AgentConfig.n_step, dmdqn_replay_nstep_commit) against
the pure-Python restatement of the contract (tests/nstep_ref.py), bit for bit:
the commit kernel on both row formats, the operator against the C ABI, the
learn's gamma^n, the Trainer schedules, the shared net, checkpoint / resume and
the drop-in DQNAgent."""
import ctypes as C
import struct

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import nstep_ref as NR  # noqa: E402
from dmdqn_amd import _lib, checkpoint as CK, kernels as K  # noqa: E402
from dmdqn_amd.agent import AgentConfig, BatchedDQN  # noqa: E402
from dmdqn_amd.env import EnvConfig  # noqa: E402
from dmdqn_amd.ops import load as ops  # noqa: E402
from dmdqn_amd.trainer import Trainer  # noqa: E402

DEV = "cuda"
RING = ["s", "n", "a", "r", "d"]
NA = 5
GAMMAS = [0.99, 0.9, 0.5, 1.0, 0.123456789]  # the per-agent array: five distinct values


def _np(ring, upto=None):
    return {k: getattr(ring, k)[:, :upto].cpu().numpy() for k in RING}


def expected_ring(raw, n, gammas, slots, first_slot=0):
    """The replay ring arrays [NA, slots, ...] (zero where nothing was
    committed) the restatement gives for the raw transitions `raw` (ring
    arrays [NA, T, ...] as the store kernels wrote them, in store order), and
    the window length m of every commit."""
    n_agents, T = raw["a"].shape
    i8 = raw["s"].dtype == np.int8
    out = {k: np.zeros((n_agents, slots) + raw[k].shape[2:], raw[k].dtype) for k in RING}
    ms = []
    for ag in range(n_agents):
        # the observations' stand-in is the raw index: a commit names its rows
        tr = [(k, int(raw["a"][ag, k]), float(raw["r"][ag, k]), k, int(raw["d"][ag, k]))
              for k in range(T)]
        for j, (i, a, R, last, d) in enumerate(NR.nstep_commits(tr, n, gammas[ag])):
            slot = (first_slot + j) % slots
            out["s"][ag, slot] = raw["s"][ag, i]
            row = raw["n"][ag, last].copy()
            if i8:  # a, done, six zero bytes, the f64 return (include/dmdqn.h DMDQN_ROW_*)
                row[96:112] = np.frombuffer(struct.pack("<BB6xd", a, d, R), np.int8)
            out["n"][ag, slot] = row
            out["a"][ag, slot], out["r"][ag, slot], out["d"][ag, slot] = a, R, d
            ms.append(last - i + 1)
    return out, ms


def _same_ring(got, want, what=""):
    for k in RING:
        g, w = got[k], want[k]
        if k == "r":  # bits, not values (-0.0, and no tolerance)
            g, w = g.view(np.int64), w.view(np.int64)
        assert np.array_equal(g, w), f"{what}ring.{k} differs"


def _done_patterns(n, T, rng):
    d = np.zeros((NA, T), np.uint8)                    # agent 0: no done at all
    d[1, [0, 3, 4, 5]] = 1                             # done at step 0, consecutive dones
    d[2, [n + 1, n + 1 + max(1, n // 2)]] = 1          # two dones inside one window
    d[2, T - 1] = 1                                    # ... and one at the last store
    d[3] = rng.random(T) < 0.3
    d[4, n + 2] = 1    # n - 1 clean entries before it: it sits at every window position
    return d


def _inputs(fmt, T, rng):
    if fmt == "int8":  # integer observations, as this env's (-1 padding .. 23 queued)
        obs = rng.integers(-1, 24, size=(T + 1, NA, 89)).astype(np.float32)
    else:
        obs = rng.normal(size=(T + 1, NA, 89)).astype(np.float32)
    act = rng.integers(0, 4, size=(T, NA)).astype(np.int32)
    rew = rng.normal(scale=30.0, size=(T, NA))  # f64, negatives included
    rew[0, 0] = -0.0
    return (torch.from_numpy(obs).to(DEV), torch.from_numpy(act).to(DEV),
            torch.from_numpy(rew).to(DEV))


def _commit(dst, stage, head, gamma=0.0, gamma_a=None):
    ops().replay_nstep_commit(head, dst.next_slot, stage.s, stage.n, stage.a, stage.r, stage.d,
                              dst.s, dst.n, dst.a, dst.r, dst.d, gamma, gamma_a)
    dst.advance()


@pytest.mark.parametrize("per_agent", [False, True], ids=["scalar", "array"])
@pytest.mark.parametrize("fmt", ["int8", "f32"])
@pytest.mark.parametrize("n", [1, 2, 3, 5, 32])
def test_commit_kernel_is_the_restatement(n, fmt, per_agent):
    rng = np.random.default_rng(100 * n + per_agent)
    T = 3 * n + 7
    obs, act, rew = _inputs(fmt, T, rng)
    dones = _done_patterns(n, T, rng)
    done_t = torch.from_numpy(dones).to(DEV)
    rawring = K.ReplayRing(NA, T, device=DEV, row_format=fmt, spare=1)   # the record
    stage = K.ReplayRing(NA, n - 1, device=DEV, row_format=fmt, spare=1)  # n slots
    dst = K.ReplayRing(NA, 10, device=DEV, row_format=fmt, spare=1)       # cap = 11 slots
    assert stage.slots == n and dst.slots == 11
    dst.total = first = 4  # so that slot reaches cap - 1 and wraps for every n
    gammas = GAMMAS if per_agent else [0.97] * NA
    gamma_a = torch.tensor(GAMMAS, dtype=torch.float64, device=DEV) if per_agent else None
    slots_hit = []
    for k in range(T):
        for ring in (rawring, stage):
            ring.store(obs[k], obs[k + 1], act[k], rew[k], done_t[:, k].contiguous())
        if k >= n - 1:
            slots_hit.append(dst.next_slot)
            _commit(dst, stage, stage.next_slot, 0.97, gamma_a)
    rawring.check()
    want, ms = expected_ring(_np(rawring, T), n, gammas, dst.slots, first)
    got = _np(dst)
    _same_ring(got, want)
    # slot reaches cap - 1 and the ring wraps
    assert len(slots_hit) == T - n + 1 and slots_hit[:8] == [4, 5, 6, 7, 8, 9, 10, 0]
    assert set(ms) == set(range(1, n + 1))  # a done at every window position, and none
    if fmt == "int8":  # the s' row byte for byte: what k_replay_store leaves zero stays zero
        rows = got["n"][:, sorted(set(slots_hit))]
        assert not rows[..., 98:104].any() and not rows[..., 112:128].any()
        assert not rows[..., 89:96].any()
        assert np.array_equal(rows[..., 96].view(np.uint8), got["a"][:, sorted(set(slots_hit))])


@pytest.mark.parametrize("fmt", ["int8", "f32"])
def test_one_step_commit_is_replay_store(fmt):
    rng = np.random.default_rng(5)
    T = 13
    obs, act, rew = _inputs(fmt, T, rng)
    done_t = torch.from_numpy((rng.random((NA, T)) < 0.4).astype(np.uint8)).to(DEV)
    direct = K.ReplayRing(NA, 10, device=DEV, row_format=fmt, spare=1)
    dst = K.ReplayRing(NA, 10, device=DEV, row_format=fmt, spare=1)
    stage = K.ReplayRing(NA, 0, device=DEV, row_format=fmt, spare=1)
    for k in range(T):
        d = done_t[:, k].contiguous()
        direct.store(obs[k], obs[k + 1], act[k], rew[k], d)
        stage.store(obs[k], obs[k + 1], act[k], rew[k], d)
        _commit(dst, stage, 0, 0.9)
    _same_ring(_np(dst), _np(direct))


@pytest.mark.parametrize("fmt", ["int8", "f32"])
def test_operator_matches_c_abi(fmt):
    rng = np.random.default_rng(9)
    n, T = 3, 9
    obs, act, rew = _inputs(fmt, T, rng)
    done_t = torch.from_numpy((rng.random((NA, T)) < 0.3).astype(np.uint8)).to(DEV)
    stage = K.ReplayRing(NA, n - 1, device=DEV, row_format=fmt, spare=1)
    by_op = K.ReplayRing(NA, 6, device=DEV, row_format=fmt, spare=1)
    by_c = K.ReplayRing(NA, 6, device=DEV, row_format=fmt, spare=1)
    gamma_a = torch.tensor(GAMMAS, dtype=torch.float64, device=DEV)
    for k in range(T):
        stage.store(obs[k], obs[k + 1], act[k], rew[k], done_t[:, k].contiguous())
        if k < n - 1:
            continue
        ga = gamma_a if k % 2 else None
        args = _lib.CNStep(NA, n, stage.next_slot, by_c.slots, by_c.next_slot, int(fmt == "f32"),
                           stage.s.data_ptr(), stage.n.data_ptr(), stage.a.data_ptr(),
                           stage.r.data_ptr(), stage.d.data_ptr(),
                           by_c.s.data_ptr(), by_c.n.data_ptr(), by_c.a.data_ptr(),
                           by_c.r.data_ptr(), by_c.d.data_ptr(), 0.95,
                           None if ga is None else ga.data_ptr())
        _lib.call("dmdqn_replay_nstep_commit", C.byref(args), _lib.stream_of())
        by_c.advance()
        _commit(by_op, stage, stage.next_slot, 0.95, ga)
    _same_ring(_np(by_op), _np(by_c))
    assert by_op.total == T - n + 1 and np.abs(_np(by_op)["r"]).sum() > 0
    D = ops()
    with pytest.raises(RuntimeError, match="gamma_a"):  # f32 where f64 is expected
        D.replay_nstep_commit(0, 0, stage.s, stage.n, stage.a, stage.r, stage.d, by_op.s, by_op.n,
                              by_op.a, by_op.r, by_op.d, 0.9, gamma_a.float())
    with pytest.raises(RuntimeError, match="head"):     # refused by the C entry point
        D.replay_nstep_commit(n, 0, stage.s, stage.n, stage.a, stage.r, stage.d, by_op.s, by_op.n,
                              by_op.a, by_op.r, by_op.d, 0.9, None)
    with pytest.raises(RuntimeError, match="ring_s"):   # rows of the other format
        other = K.ReplayRing(NA, 6, device=DEV, row_format="f32" if fmt == "int8" else "int8",
                             spare=1)
        D.replay_nstep_commit(0, 0, stage.s, stage.n, stage.a, stage.r, stage.d, other.s, other.n,
                              by_op.a, by_op.r, by_op.d, 0.9, None)


# --------------------------------------------------------------------------- the learn sees gamma^n
def _feed(E, A, T, rng):
    obs = torch.from_numpy(rng.integers(-1, 24, size=(T + 1, E, A, 89)).astype(np.float32)).to(DEV)
    act = torch.from_numpy(rng.integers(0, 4, size=(T, E, A)).astype(np.int32)).to(DEV)
    rew = torch.from_numpy(rng.normal(scale=20.0, size=(T, E, A))).to(DEV)
    return obs, act, rew


@pytest.mark.parametrize("precision,sweep", [("fp32", False), ("fp16", False), ("bf16", False),
                                             ("fp16", True)])
def test_learn_sees_gamma_to_the_n(precision, sweep):
    E, A, T, n = 2, 2, 140, 3
    g3 = [float(np.float32(g * g * g)) for g in (0.9, 0.8)]
    base = dict(replay_buffer_size=300, target_update_frequency=4, seed=3, precision=precision)
    ag = BatchedDQN(E, A, AgentConfig(n_step=n, gamma=0.9, **base,
                                      sweep={"gamma": [0.9, 0.8]} if sweep else None), device=DEV)
    ref = BatchedDQN(E, A, AgentConfig(gamma=g3[0], **base,
                                       sweep={"gamma": g3} if sweep else None), device=DEV)
    assert ag.stage.slots == n and ag.store_ring is ag.stage and ref.stage is None
    assert ref.store_ring is ref.ring
    gam = np.repeat([0.9, 0.8] if sweep else [0.9, 0.9], A)  # per agent, env-major
    if sweep:
        assert ag.nstep_gamma_a.dtype == torch.float64 and ag.nstep_gamma_a.tolist() == list(gam)
        assert ag.hp_gamma.tolist() == ref.hp_gamma.tolist() == list(np.repeat(np.float32(g3), A))
    assert np.float32(ag.gamma_n) == NR.bootstrap_gamma(0.9, n) == np.float32(ref.gamma_n)
    rng = np.random.default_rng(21)
    obs, act, rew = _feed(E, A, T, rng)
    rew_h, learns = rew.cpu().numpy().reshape(T, E * A), 0
    dones = [(k % 37) == 36 for k in range(T)]
    for k in range(T):
        ag.remember(obs[k], act[k], rew[k], obs[k + 1], dones[k])
        la = ag.learn()
        if k < n - 1:
            assert la is None and len(ag.ring) == 0
            continue
        # the comparison agent stores the restatement's transition of start i
        i = k - n + 1
        com = [NR.window_commit([(None, 0, rew_h[j, a], j, dones[j]) for j in range(i, k + 1)],
                                gam[a]) for a in range(E * A)]
        last = com[0][3]
        assert all(c[3] == last for c in com)  # done is per step, the same for every agent
        R = torch.tensor([c[2] for c in com], dtype=torch.float64, device=DEV).reshape(E, A)
        ref.remember(obs[i], act[i], R, obs[last + 1], bool(com[0][4]))
        lr = ref.learn()
        assert (la is None) == (lr is None) == (k < 127 + n - 1), k
        if la is None:
            continue
        learns += 1
        assert torch.equal(la, lr), f"loss differs at raw store {k}"
        for name in ["params", "adam_m", "adam_v", "target", "idx"]:
            assert torch.equal(getattr(ag, name), getattr(ref, name)), (name, k)
        if ag.target_h is not None:
            assert torch.equal(ag.target_h, ref.target_h)
    assert learns == T - (127 + n - 1) == ag.learn_launches and len(ag.ring) == T - n + 1
    _same_ring(_np(ag.ring), _np(ref.ring))
    ag.learn(collect_stats=True)
    assert ag.learn_metrics()["n_step"] == n and ref.learn_metrics()["n_step"] == 1


# --------------------------------------------------------------------------- Trainer
STEPS, CKPT_AT = 142, 133


def _trainer(n_step=3, **kw):
    shared = kw.pop("shared", False)
    return Trainer(EnvConfig(rows=2, cols=2, num_envs=4, seed=11, max_sim_time=500),
                   AgentConfig(replay_buffer_size=300, target_update_frequency=5, seed=4,
                               precision="fp16", n_step=n_step, shared_params=shared), **kw)


def _run(tr, steps, out=None):
    out = [] if out is None else out
    for _ in range(steps):
        tr.step()
        out.append((None if tr.last_loss is None else tr.last_loss.clone(), tr.obs.clone(),
                    tr.last_reward.clone(), tr.agent.actions.clone()))
    torch.cuda.synchronize()
    return out


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """The raw stream (an n_step = 1, fused=False run: epsilon stays 1, A-1, so
    it does not depend on learning) and the n_step = 3 runs of every schedule;
    the fused one-stream run also leaves a checkpoint at step CKPT_AT."""
    one = _trainer(1, fused=False)
    _run(one, STEPS)
    assert one.agent.stage is None and len(one.agent.ring) == STEPS
    raw = _np(one.agent.ring, STEPS)
    path = str(tmp_path_factory.mktemp("nstep") / "mid.pt")
    fused = _trainer()
    log = _run(fused, CKPT_AT)
    CK.save(path, fused)
    out = {"raw": raw, "ckpt": path, "fused": (fused, _run(fused, STEPS - CKPT_AT, log))}
    for name, kw in [("unfused", dict(fused=False)), ("env", dict(overlap="env")),
                     ("env+side", dict(overlap="env", side_learn=6))]:
        tr = _trainer(**kw)
        out[name] = (tr, _run(tr, STEPS))
    return out


def _same_trainers(ta, la, tb, lb, what):
    assert len(la) == len(lb)
    for t, (x, y) in enumerate(zip(la, lb)):
        assert (x[0] is None) == (y[0] is None), (what, t)
        for i, name in enumerate(["loss", "obs", "reward", "actions"]):
            if x[i] is not None:
                assert torch.equal(x[i], y[i]), f"{what}: {name} differs at step {t}"
    tb.sync_outputs()
    a, b = ta.agent, tb.agent
    for name in ["params", "target", "target_h", "adam_m", "adam_v", "np_state", "py_state", "idx"]:
        assert torch.equal(getattr(a, name), getattr(b, name)), (what, name)
    _same_ring(_np(a.ring), _np(b.ring), what + " ")
    _same_ring(_np(a.stage), _np(b.stage), what + " staging ")
    assert (a.ring.total, a.stage.total, a.learn_launches) == (b.ring.total, b.stage.total,
                                                              b.learn_launches)


@pytest.mark.parametrize("other", ["unfused", "env", "env+side"])
def test_trainer_schedules_are_bit_identical(runs, other):
    ref, log = runs["fused"]
    tr, log2 = runs[other]
    assert ref.fused and tr.fused == (other != "unfused") and (tr.side is None) == (other == "unfused")
    _same_trainers(ref, log, tr, log2, other)


def test_trainer_ring_is_the_restatement_of_the_raw_stream(runs):
    tr, log = runs["fused"]
    ag = tr.agent
    assert int(tr.env.env_episodes.min()) >= 2  # every replica restarted at least twice
    assert runs["raw"]["d"].sum(axis=1).min() >= 2
    assert len(ag.ring) == STEPS - 2 == ag.ring.total and ag.stage.total == STEPS
    # the first learn comes at step 130 (raw store 127 + n_step)
    assert [x[0] is not None for x in log].index(True) == 129 and ag.learn_launches == STEPS - 129
    want, ms = expected_ring(runs["raw"], 3, [ag.cfg.gamma] * ag.NA, ag.ring.slots)
    assert set(ms) == {1, 2, 3}
    _same_ring(_np(ag.ring), want)
    # the staging ring holds the last three raw transitions
    for k in range(STEPS - 3, STEPS):
        for f in RING:
            assert np.array_equal(getattr(ag.stage, f)[:, k % 3].cpu().numpy(), runs["raw"][f][:, k])


def test_shared_net_trainer(runs):
    steps = 135
    tr = _trainer(shared=True)
    log = _run(tr, steps)
    ag = tr.agent
    assert ag.shared and len(ag.ring) == steps - 2 and ag.learn_launches == steps - 129
    raw = {k: v[:, :steps] for k, v in runs["raw"].items()}
    want, _ = expected_ring(raw, 3, [ag.cfg.gamma] * ag.NA, ag.ring.slots)
    _same_ring(_np(ag.ring), want)
    assert log[128][0] is None and all(bool(torch.isfinite(x[0]).all()) for x in log[129:])


def test_checkpoint_resumes_mid_window(runs):
    ref, log = runs["fused"]
    st = torch.load(runs["ckpt"], map_location="cpu", weights_only=True)
    assert st["format"] == "dmdqn-ckpt-8" and st["agent_cfg"]["n_step"] == 3
    assert st["nstep"]["total"] == CKPT_AT and CKPT_AT % 3 != 0  # saved mid-window
    assert tuple(st["nstep"]["s"].shape) == (ref.agent.NA, 3, 128)
    tr = _trainer()
    CK.load(runs["ckpt"], tr)
    assert tr.agent.stage.total == CKPT_AT and tr.agent.ring.total == CKPT_AT - 2
    log2 = _run(tr, STEPS - CKPT_AT)
    _same_trainers(ref, log[CKPT_AT:], tr, log2, "resumed")
    with pytest.raises(ValueError, match="n_step"):
        CK.load(runs["ckpt"], _trainer(1))
    # a one-step Trainer's checkpoint has no staging key
    one = _trainer(1)
    assert "nstep" not in CK.trainer_state(one)
    # a staging tensor of another shape is refused before anything is copied
    bad = dict(st, nstep=dict(st["nstep"], r=st["nstep"]["r"][:, :2]))
    path = runs["ckpt"] + ".bad"
    torch.save(bad, path)
    fresh = _trainer()
    before = fresh.agent.params.clone()
    with pytest.raises(ValueError, match="nstep.r"):
        CK.load(path, fresh)
    assert torch.equal(fresh.agent.params, before) and fresh.agent.stage.total == 0


# --------------------------------------------------------------------------- drop-in DQNAgent
def test_dropin_agent_builds_two_step_transitions():
    from src.agents import dqn_agent
    dqn_agent.seed(5)
    agent = dqn_agent.DQNAgent(89, 4, "J_0_0", {"n_step": 2, "gamma": 0.9})
    assert agent.n_step == 2 and agent.replay_buffer.ring.row_format == "f32"
    rng = np.random.default_rng(2)
    obs = rng.normal(size=(6, 89)).astype(np.float32)  # float rows keep any value
    raw = [(k, int(rng.integers(0, 4)), float(rng.normal()), k + 1, int(k == 2)) for k in range(5)]
    for k, a, r, _, d in raw:
        agent.remember(obs[k][None], a, r, obs[k + 1][None], bool(d))
        assert len(agent.replay_buffer) == max(0, k)
    want = NR.nstep_commits(raw, 2, 0.9)
    assert len(want) == 4 and [c[4] for c in want] == [0, 1, 1, 0]
    ring = agent.replay_buffer.ring
    for j, (i, a, R, nxt, d) in enumerate(want):
        assert np.array_equal(ring.s[0, j, :89].cpu().numpy(), obs[i])
        assert np.array_equal(ring.n[0, j, :89].cpu().numpy(), obs[nxt])
        assert not ring.s[0, j, 89:].any() and not ring.n[0, j, 89:].any()
        assert int(ring.a[0, j]) == a and int(ring.d[0, j]) == d
        assert struct.pack("<d", float(ring.r[0, j])) == struct.pack("<d", R)
    with pytest.raises(ValueError, match="n_step"):
        dqn_agent.DQNAgent(89, 4, "J_0_1", {"n_step": 33})
