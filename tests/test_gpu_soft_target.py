"""GPU: soft (Polyak) target updates (the reference's
update_target_network_soft, dqn_agent.py:372-373, 389-399) fused into the learn
kernels, against the existing kernels plus the float32 numpy restatement of
the update -- bit for bit.

The bit contract: a learn with tau > 0 leaves the bits of the same learn with
tau = 0 followed by dmdqn_target_soft_update, and both equal the numpy formula
target = fl32(fl32(tau_f * online) + fl32(omt_f * target)) on the online net
after the learn's Adam step.  The references here are the tau = 0 kernels (the
code as it was) and numpy, never the soft path itself.  Shapes are the smallest
that run every index map: one or two envs of two or three agents, replay 300
filled past a wrap.

The last test replays tests/golden/soft_target.npz, the reference's own
DQNAgent.learn + update_target_network_soft under the TF restatement
(tests/golden/make_soft_golden.py: the reference's Python on a torch-backed
shim, not real TensorFlow), at the fp32 pinned tolerances of
test_gpu_pinned.py: loss rtol 1e-4, final online / target atol 5e-5."""
import ctypes
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from dmdqn_amd import _lib  # noqa: E402
from dmdqn_amd import checkpoint as CK  # noqa: E402
from dmdqn_amd.agent import (AgentConfig, BatchedDQN, PRECISIONS, keras_initial_weights,  # noqa: E402
                             kernel_to_keras, n_params, soft_update_consts)
from dmdqn_amd.env import EnvConfig  # noqa: E402
from dmdqn_amd.trainer import Trainer  # noqa: E402

from test_gpu_learn import _fill  # noqa: E402
from test_soft_target_cpu import soft_update_np  # noqa: E402

DEV = "cuda"
STATE = ("params", "adam_m", "adam_v", "target", "target_h")


def _bits(t):
    return t.view({4: torch.int32, 2: torch.int16}[t.element_size()])


def _assert_same(a, b, names=STATE, what=""):
    for n in names:
        x, y = getattr(a, n), getattr(b, n)
        if x is None and y is None:
            continue
        assert torch.equal(_bits(x), _bits(y)), f"{what}{n}: {int((_bits(x) != _bits(y)).sum())} differ"


def _agent(precision="fp32", hidden=128, rows="int8", tau=0.0, tuf=0, E=1, A=2, shared=False,
           fill=330):
    cfg = AgentConfig(precision=precision, nn_layers=[hidden, hidden], replay_buffer_size=300,
                      target_update_frequency=tuf, seed=3, replay_rows=rows, tau=tau,
                      shared_params=shared)
    ag = BatchedDQN(E, A, cfg)
    _fill(ag, fill, np.random.RandomState(1))  # wraps the ring (start 30)
    assert ag.ring.start == max(0, fill - 300)
    return ag


def _host_soft(ag, tau):
    """The numpy soft update of ag's target from its online net, written back
    (and the 16-bit shadow refreshed by the existing RNE cast)."""
    t = soft_update_np(ag.params.cpu().numpy(), ag.target.cpu().numpy(), tau)
    ag.target.copy_(torch.from_numpy(t))
    ag._refresh_target_h()


# --------------------------------------------------------------------------- 1
@pytest.mark.parametrize("precision,hidden", [("fp32", 128), ("fp16", 128), ("bf16", 128),
                                              ("fp32", 64)])
@pytest.mark.parametrize("tau", [0.005, 0.5])
def test_standalone_kernel_matches_numpy(precision, hidden, tau):
    NW, P = 3, n_params(hidden)
    Ph = (P + 7) // 8 * 8
    g = torch.Generator(device=DEV).manual_seed(7)
    params = torch.randn((NW, P), device=DEV, generator=g)
    target = torch.randn((NW, P), device=DEV, generator=g)
    h16 = {"fp16": torch.float16, "bf16": torch.bfloat16}.get(precision)
    th = None if h16 is None else torch.full((NW, Ph), 7.0, dtype=h16, device=DEV)
    want = soft_update_np(params.cpu().numpy(), target.cpu().numpy(), tau)
    tau_f, omt_f = soft_update_consts(tau)
    _lib.call("dmdqn_target_soft_update", _lib.ptr(params), _lib.ptr(target), _lib.ptr(th), NW, P,
              Ph, PRECISIONS[precision], ctypes.c_float(tau_f), ctypes.c_float(omt_f),
              _lib.stream_of())
    got = target.cpu().numpy()
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    if th is not None:
        assert torch.equal(_bits(th[:, :P]), _bits(torch.from_numpy(want).to(h16).to(DEV)))
        assert (th[:, P:] == 7.0).all()  # the padding is not written


def test_standalone_tau_one_copies_the_online_net():
    ag = _agent("fp16", fill=140)
    ag.learn()
    assert not torch.equal(ag.target, ag.params)
    ag.update_target_network_soft(1.0)
    assert torch.equal(ag.target, ag.params)
    assert torch.equal(ag.target_h[:, :ag.P], ag.params.to(torch.float16))


# --------------------------------------------------------------------------- 2
# path: the 16-bit launchers' DMDQN_OPT_SOFT_PATH -- "fused" (the soft
# instantiation of the learn kernel) or "split" (the plain kernel, then
# k_target_soft); auto picks by agent count, so the small shapes here force each
@pytest.mark.parametrize("stats", [False, True])
@pytest.mark.parametrize("precision,hidden,rows,path", [
    ("fp32", 64, "int8", "auto"), ("fp32", 128, "int8", "auto"), ("fp32", 128, "f32", "auto"),
    ("fp16", 128, "int8", "fused"), ("bf16", 128, "int8", "fused"), ("fp16", 128, "f32", "fused"),
    ("bf16", 128, "f32", "fused"), ("fp16", 128, "int8", "split"), ("bf16", 128, "int8", "split")])
def test_fused_soft_learn_matches_plain_learn_plus_numpy(precision, hidden, rows, path, stats,
                                                         lib_option):
    lib_option("soft_path", path)
    tau = 0.01
    a = _agent(precision, hidden, rows, tau=tau)
    b = _agent(precision, hidden, rows, tau=0.0)
    _assert_same(a, b, what="start ")
    for k in range(1, 5):  # the moved target feeds the next learn's target forward
        la, lb = a.learn(collect_stats=stats), b.learn(collect_stats=stats)
        _host_soft(b, tau)
        assert torch.equal(_bits(la), _bits(lb)), f"loss of learn {k}"
        _assert_same(a, b, what=f"learn {k} ")
        if stats:
            assert torch.equal(a.qstats, b.qstats)
    assert not torch.equal(a.target, a.params)


# --------------------------------------------------------------------------- 3
@pytest.mark.parametrize("precision", ["fp16", "bf16"])
def test_split_soft_learn_bit_identical_to_fused(precision, lib_option):
    lib_option("soft_path", "fused")
    a = _agent(precision, tau=0.01, E=2, A=3)
    b = _agent(precision, tau=0.01, E=2, A=3)
    b.set_split_learn(True)
    for k in range(1, 4):
        la, lb = a.learn(), b.learn()
        assert torch.equal(_bits(la), _bits(lb))
        _assert_same(a, b, what=f"learn {k} ")


# --------------------------------------------------------------------------- 4
def test_soft_learn_without_the_shadow_through_the_c_abi(lib_option):
    """target_h = NULL (no soft instantiation: the plain kernel, then
    k_target_soft, even when the fused path is asked for): params and target
    as the fused soft learn's."""
    lib_option("soft_path", "fused")
    a = _agent("fp16", tau=0.01)
    b = _agent("fp16", tau=0.01)
    for k in range(1, 5):
        la = a.learn()
        assert b.learn_begin()
        args = b.c_learn_args()
        assert args.tau == np.float32(0.01) and args.one_minus_tau == np.float32(0.99)
        args.target_h = None
        _lib.call("dmdqn_learn", ctypes.byref(args), _lib.stream_of())
        assert torch.equal(_bits(la), _bits(b.loss))
        _assert_same(a, b, names=("params", "adam_m", "adam_v", "target"), what=f"learn {k} ")


# --------------------------------------------------------------------------- 5
@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_soft_and_hard_rules_compose(precision, lib_option):
    """tau = 0.01 with a hard sync every 3 learns: the hard copy wins on learn 3
    (dqn_agent.py:372-377), the soft formula holds on learns 1, 2 and 4."""
    lib_option("soft_path", "fused")
    tau = 0.01
    a = _agent(precision, tau=tau, tuf=3)
    b = _agent(precision, tau=0.0, tuf=0)
    for k in range(1, 5):
        a.learn()
        b.learn()
        if k == 3:
            b.target.copy_(b.params)
            b._refresh_target_h()
        else:
            _host_soft(b, tau)
        _assert_same(a, b, what=f"learn {k} ")
        assert torch.equal(a.target, a.params) == (k == 3)


# --------------------------------------------------------------------------- 6
def test_shared_net_soft_update():
    tau = 0.01
    a = _agent("fp16", tau=tau, E=1, A=4, shared=True, fill=200)
    b = _agent("fp16", tau=0.0, E=1, A=4, shared=True, fill=200)
    assert a.params.shape[0] == 1
    for k in range(1, 4):
        la, lb = a.learn(), b.learn()
        _host_soft(b, tau)
        assert torch.equal(_bits(la), _bits(lb))
        _assert_same(a, b, what=f"learn {k} ")
        assert torch.equal(_bits(a.params_h), _bits(b.params_h))  # untouched by the soft step


# --------------------------------------------------------------------------- 7
def _dropin(cfg_extra):
    from src.agents import dqn_agent as DA
    DA.seed(2)
    cfg = {"replay_buffer_size": 300, "nn_layers": [128, 128], "target_update_frequency": 0}
    cfg.update(cfg_extra)
    ag = DA.DQNAgent(89, 4, "J_0_0", cfg)
    rng = np.random.RandomState(6)
    for t in range(130):
        s = rng.randint(-1, 24, size=(1, 89)).astype(np.float32)
        n = rng.randint(-1, 24, size=(1, 89)).astype(np.float32)
        ag.remember(s, int(rng.randint(0, 4)), -float(rng.rand()) * 50, n, t % 60 == 59)
    return ag


def test_dropin_soft_updates():
    ag = _dropin({"tau": 0.01})
    assert ag.tau == 0.01
    core = ag._core
    t0 = core.target.cpu().numpy().copy()
    assert ag.learn() is not None
    want = soft_update_np(core.params.cpu().numpy(), t0, 0.01)
    assert np.array_equal(core.target.cpu().numpy().view(np.int32), want.view(np.int32))
    # by hand, with an assigned tau, as a caller of the reference would
    ag2 = _dropin({})
    assert ag2.tau is None
    with pytest.raises(AttributeError, match="tau"):
        ag2.update_target_network_soft()
    assert ag2.learn() is not None
    c2 = ag2._core
    t0 = c2.target.cpu().numpy().copy()
    ag2.tau = 0.1
    ag2.update_target_network_soft()
    want = soft_update_np(c2.params.cpu().numpy(), t0, 0.1)
    assert np.array_equal(c2.target.cpu().numpy().view(np.int32), want.view(np.int32))
    assert not np.array_equal(want, t0)


# --------------------------------------------------------------------------- 8
def _trainer(overlap, tau=0.01):
    return Trainer(EnvConfig(rows=2, cols=2, num_envs=2, seed=11),
                   AgentConfig(replay_buffer_size=300, target_update_frequency=0, seed=4,
                               precision="fp16", tau=tau), overlap=overlap)


def _run(tr, n):
    out = []
    for _ in range(n):
        tr.step()
        out.append((None if tr.last_loss is None else tr.last_loss.clone(), tr.obs.clone()))
    tr.synchronize()
    return out


def _same_runs(a, b):
    for (la, oa), (lb, ob) in zip(a, b):
        assert (la is None) == (lb is None) and torch.equal(oa, ob)
        if la is not None:
            assert torch.equal(_bits(la), _bits(lb))


def test_trainer_overlap_and_resume_with_soft_updates(tmp_path):
    ref, ovl = _trainer("none"), _trainer(True)
    assert ovl.side is not None and ref.side is None
    a, b = _run(ref, 148), _run(ovl, 148)  # 21 learns past the gate
    _same_runs(a, b)
    _assert_same(ref.agent, ovl.agent)
    assert not torch.equal(ref.agent.target, ref.agent.params)
    path = os.path.join(str(tmp_path), "ck.pt")
    CK.save(path, ref)
    cont = _run(ref, 6)
    tr2 = _trainer("none")
    CK.load(path, tr2)
    _same_runs(cont, _run(tr2, 6))
    _assert_same(ref.agent, tr2.agent)
    with pytest.raises(ValueError, match="tau"):
        CK.load(path, _trainer("none", tau=0.02))


# --------------------------------------------------------------------------- 9
def test_dropin_matches_reference_soft_updates():
    """The drop-in DQNAgent with tau = 0.01 over the fixture's loop vs the
    reference's own learn() + update_target_network_soft() (under the TF
    restatement, not real TensorFlow): 73 learns, never re-synced."""
    from src.agents import dqn_agent as DA
    G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                             "soft_target.npz"))
    steps, buf, tuf, seed, init_seed, stride = (int(x) for x in G["cfg"])
    obs = G["obs"].astype(np.float32)
    cfg = {"learning_rate": 0.001, "gamma": 0.99, "epsilon_start": 1.0, "epsilon_min": 0.01,
           "epsilon_decay_steps": 200000, "replay_buffer_size": buf, "batch_size": 128,
           "target_update_frequency": tuf, "nn_layers": [128, 128], "precision": "fp32",
           "tau": float(G["tau"][0])}
    DA.seed(seed)
    ag = DA.DQNAgent(89, 4, "J_0_0", cfg)
    w0 = keras_initial_weights(np.random.RandomState(init_seed), 128, 1)[0]
    shapes = [(89, 128), (128,), (128, 128), (128,), (128, 4), (4,)]
    offs = np.cumsum([0] + [int(np.prod(sh)) for sh in shapes])
    ag._core.set_weights(0, [w0[offs[i]:offs[i + 1]].reshape(sh) for i, sh in enumerate(shapes)])
    losses = np.full(steps, np.nan)
    t1 = None
    for t in range(steps):
        a = ag.select_action(obs[t][None])
        assert a == G["actions"][t], f"step {t}"
        ag.remember(obs[t][None], a, float(G["rew"][t]), obs[t + 1][None], bool(G["done"][t]))
        loss = ag.learn()
        if loss is not None:
            losses[t] = loss
            if ag.learn_step_counter == 1:
                t1 = kernel_to_keras(ag._core.target[0].cpu().numpy(), 128)
    assert ag.learn_step_counter == int(G["learn_steps"][0]) == 73
    ref = G["losses"]
    assert np.array_equal(np.isnan(losses), np.isnan(ref))
    ok = ~np.isnan(ref)
    online = np.concatenate([w.reshape(-1) for w in ag._core.get_weights(0)])
    target = kernel_to_keras(ag._core.target[0].cpu().numpy(), 128)
    rel = np.abs(losses[ok] - ref[ok]) / np.abs(ref[ok])
    print(f"soft fp32: loss rel err max {rel.max():.3g}; |d online| max "
          f"{np.abs(online - G['final_online']).max():.3g}; |d target| max "
          f"{np.abs(target - G['final_target']).max():.3g}; |d t1| max "
          f"{np.abs(t1[::stride] - G['t1']).max():.3g}")
    np.testing.assert_allclose(losses[ok], ref[ok], rtol=1e-4)
    np.testing.assert_allclose(t1[::stride], G["t1"], atol=5e-5)
    np.testing.assert_allclose(online, G["final_online"], atol=5e-5)
    np.testing.assert_allclose(target, G["final_target"], atol=5e-5)
    assert np.abs(target - online).max() > 1e-3  # the target lags: no hard sync ran
