"""GPU: per-agent hyperparameters (AgentConfig.sweep -- learning_rate, gamma and
tau per env replica, include/dmdqn.h dmdqn_agent_hparams) against the scalar
kernels as they stand, bit for bit.

The bit contract: an agent whose values come from the per-agent arrays computes
what it computes in a scalar launch with those values -- the same operations on
the same operands (the kernel forms alpha = fl32(fl32(lr * s) / d) as the host
does, gamma and tau are read instead of passed) -- so every comparison here is
bit equality, and the references are scalar BatchedDQN / Trainer runs (and, for
the standalone soft update, the float32 numpy formula), never the new path.

Shapes are the smallest that run every index map: 2 or 3 envs of 2 agents (the
trainer: 4 envs of a 2x2 grid), replay 300 filled to 330 so the ring has
wrapped, 5 learns with target_update_frequency 3 so a hard sync falls inside."""
import ctypes
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from dmdqn_amd import _lib  # noqa: E402
from dmdqn_amd import checkpoint as CK  # noqa: E402
from dmdqn_amd.agent import (AgentConfig, BatchedDQN, PRECISIONS, n_params,  # noqa: E402
                             soft_update_consts)
from dmdqn_amd.env import EnvConfig  # noqa: E402
from dmdqn_amd.ops import load as load_ops  # noqa: E402
from dmdqn_amd.trainer import Trainer  # noqa: E402

from test_gpu_learn import _fill  # noqa: E402
from test_soft_target_cpu import soft_update_np  # noqa: E402

DEV = "cuda"
STATE = ("params", "adam_m", "adam_v", "target", "target_h")
LEARNS = 5
BASE = dict(learning_rate=7e-4, gamma=0.97, tau=0.01)


def _bits(t):
    return t.view({4: torch.int32, 2: torch.int16}[t.element_size()])


def _same(x, y, what):
    assert torch.equal(_bits(x), _bits(y)), f"{what}: {int((_bits(x) != _bits(y)).sum())} differ"


def _assert_same(a, b, what="", rows=slice(None), names=STATE):
    for n in names:
        x, y = getattr(a, n), getattr(b, n)
        if x is None and y is None:
            continue
        _same(x[rows], y[rows], f"{what}{n}")


def _agent(precision="fp16", hidden=128, rows="int8", E=2, A=2, sweep=None, variant_of_env=None,
           **hp):
    kw = dict(BASE, **hp)
    cfg = AgentConfig(precision=precision, nn_layers=[hidden, hidden], replay_buffer_size=300,
                      target_update_frequency=3, seed=3, replay_rows=rows, sweep=sweep, **kw)
    ag = BatchedDQN(E, A, cfg, variant_of_env=variant_of_env)
    _fill(ag, 330, np.random.RandomState(1))  # wraps the ring (start 30)
    assert ag.ring.start == 30
    return ag


# --------------------------------------------------------------------------- 1
# path: the 16-bit launchers' DMDQN_OPT_SOFT_PATH ("fused": the soft
# instantiation of the learn kernel; "split": the plain kernel, then
# k_target_soft with one tau per net); auto picks by agent count
CASES = [("fp32", 64, "int8", "auto"), ("fp32", 128, "int8", "auto"), ("fp32", 128, "f32", "auto"),
         ("fp16", 128, "int8", "fused"), ("bf16", 128, "int8", "fused"),
         ("fp16", 128, "f32", "fused"), ("bf16", 128, "f32", "fused"),
         ("fp16", 128, "int8", "split"), ("bf16", 128, "int8", "split")]


def _uniform_pair(precision, hidden, rows, keys=("learning_rate", "gamma", "tau")):
    sweep = {k: [BASE[k]] for k in keys}
    a = _agent(precision, hidden, rows, sweep=sweep)
    b = _agent(precision, hidden, rows)
    assert a.swept and not b.swept and len(a.variants) == 1
    for k, t in (("learning_rate", a.hp_lr), ("gamma", a.hp_gamma), ("tau", a.hp_tau),
                 ("tau", a.hp_omt)):
        assert (t is not None) == (k in keys)
        assert t is None or (t.shape == (a.NA,) and t.dtype == torch.float32 and t.is_cuda)
    _assert_same(a, b, what="start ")
    return a, b


def _learn_both(a, b, stats):
    for k in range(1, LEARNS + 1):  # learn 3 hard-syncs; the others move the target softly
        la, lb = a.learn(collect_stats=stats), b.learn(collect_stats=stats)
        _same(la, lb, f"loss of learn {k}")
        _assert_same(a, b, what=f"learn {k} ")
        if stats:
            assert torch.equal(a.qstats, b.qstats), f"qstats of learn {k}"
        assert torch.equal(a.target, a.params) == (k == 3)


@pytest.mark.parametrize("stats", [False, True])
@pytest.mark.parametrize("precision,hidden,rows,path", CASES)
def test_uniform_arrays_equal_the_scalar_path(precision, hidden, rows, path, stats, lib_option):
    lib_option("soft_path", path)
    a, b = _uniform_pair(precision, hidden, rows)
    _learn_both(a, b, stats)


@pytest.mark.parametrize("stats", [False, True])
@pytest.mark.parametrize("precision", ["fp16", "bf16"])
def test_uniform_arrays_equal_the_scalar_path_split_learn(precision, stats, lib_option):
    """dmdqn_learn_grad_hp + dmdqn_adam_agents_hp against dmdqn_learn_grad +
    dmdqn_adam_agents."""
    lib_option("soft_path", "fused")
    a, b = _uniform_pair(precision, 128, "int8")
    a.set_split_learn(True)
    b.set_split_learn(True)
    _learn_both(a, b, stats)


@pytest.mark.parametrize("key", ["learning_rate", "gamma", "tau"])
@pytest.mark.parametrize("precision,path", [("fp32", "auto"), ("fp16", "fused"), ("fp16", "split")])
def test_one_array_alone_equals_the_scalar_path(precision, path, key, lib_option):
    """A block with one array (the others NULL: their launch scalars hold)."""
    lib_option("soft_path", path)
    a, b = _uniform_pair(precision, 128, "int8", keys=(key,))
    _learn_both(a, b, False)
    if precision == "fp16" and path == "fused":
        a.set_split_learn(True)
        b.set_split_learn(True)
        la, lb = a.learn(), b.learn()
        _same(la, lb, "split loss")
        _assert_same(a, b, what="split learn ")


# --------------------------------------------------------------------------- 2
# E = 3, A = 2, two variants in use, variant 0 on envs 0 and 2.  lr x gamma: a
# 2 x 2 grid of which the replicas run variants 0 and 3 (both values differ);
# tau alone: G = 2 with the default assignment g % G.
DISTINCT = {
    "lr_gamma": (dict(learning_rate=[1e-3, 2e-4], gamma=[0.99, 0.9]), [0, 3, 0]),
    "tau": (dict(tau=[0.005, 0.5]), None),
}


@pytest.mark.parametrize("which", list(DISTINCT))
@pytest.mark.parametrize("precision,path,split", [
    ("fp32", "auto", False), ("fp16", "fused", False), ("fp16", "split", False),
    ("bf16", "fused", False), ("fp16", "fused", True)])
def test_distinct_variants_equal_their_own_scalar_runs(precision, path, split, which, lib_option):
    lib_option("soft_path", path)
    sweep, voe = DISTINCT[which]
    E, A = 3, 2
    sw = _agent(precision, E=E, A=A, sweep=sweep, variant_of_env=voe)
    voe = sw.variant_of_env.tolist()
    assert voe == [0, 3, 0] if which == "lr_gamma" else voe == [0, 1, 0]
    used = sorted(set(voe))
    assert len(used) == 2
    scalar = {v: _agent(precision, E=E, A=A, **sw.variants[v]) for v in used}
    agents = [sw] + list(scalar.values())
    for ag in agents:
        ag.set_split_learn(split)
    for k in range(1, LEARNS + 1):
        losses = [ag.learn(collect_stats=True) for ag in agents]
        for e in range(E):
            rows, ref = slice(e * A, (e + 1) * A), scalar[voe[e]]
            i = agents.index(ref)
            _same(losses[0][rows], losses[i][rows], f"learn {k} env {e} loss")
            _assert_same(sw, ref, what=f"learn {k} env {e} ", rows=rows)
            assert torch.equal(sw.qstats[rows], ref.qstats[rows])
        # not vacuous: on the same env the two scalar runs differ
        s0, s1 = scalar[used[0]], scalar[used[1]]
        assert not torch.equal(s0.target[:A], s1.target[:A])
        if which == "lr_gamma":
            assert not torch.equal(s0.params[:A], s1.params[:A])


# --------------------------------------------------------------------------- 3
@pytest.mark.parametrize("precision,split", [("fp32", False), ("fp16", False), ("fp16", True)])
def test_ranges_leave_the_bits_of_one_learn(precision, split, lib_option):
    """learn_begin + learn_range(0, 2) + learn_range(2, NA) with distinct
    variants: a range must read its own slice of the per-agent arrays."""
    lib_option("soft_path", "fused")
    sweep = dict(learning_rate=[1e-3, 2e-4], gamma=[0.99, 0.9], tau=[0.005, 0.5])
    voe = [0, 7, 2]
    a = _agent(precision, E=3, A=2, sweep=sweep, variant_of_env=voe)
    b = _agent(precision, E=3, A=2, sweep=sweep, variant_of_env=voe)
    a.set_split_learn(split)
    b.set_split_learn(split)
    for k in range(1, LEARNS + 1):
        la = a.learn(collect_stats=True)
        assert b.learn_begin(True)
        b.learn_range(0, 2)
        lb = b.learn_range(2, b.NA)
        _same(la, lb, f"learn {k} loss")
        _assert_same(a, b, what=f"learn {k} ")
        assert torch.equal(a.qstats, b.qstats)


# --------------------------------------------------------------------------- 4
@pytest.mark.parametrize("precision,hidden", [("fp32", 128), ("fp16", 128), ("bf16", 128),
                                              ("fp32", 64)])
def test_standalone_soft_update_with_one_tau_per_net(precision, hidden):
    NW, P = 3, n_params(hidden)
    Ph = (P + 7) // 8 * 8
    taus = [0.005, 0.5, 1.0]
    g = torch.Generator(device=DEV).manual_seed(7)
    params = torch.randn((NW, P), device=DEV, generator=g)
    target = torch.randn((NW, P), device=DEV, generator=g)
    h16 = {"fp16": torch.float16, "bf16": torch.bfloat16}.get(precision)
    th = None if h16 is None else torch.full((NW, Ph), 7.0, dtype=h16, device=DEV)
    want = np.stack([soft_update_np(params[w].cpu().numpy(), target[w].cpu().numpy(), taus[w])
                     for w in range(NW)])
    consts = [soft_update_consts(t) for t in taus]
    tau_a = torch.tensor([float(c[0]) for c in consts], dtype=torch.float32, device=DEV)
    omt_a = torch.tensor([float(c[1]) for c in consts], dtype=torch.float32, device=DEV)
    load_ops().target_soft_update_hp(params, target, th, PRECISIONS[precision], tau_a, omt_a)
    got = target.cpu().numpy()
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    assert np.array_equal(got[2], params[2].cpu().numpy())  # tau = 1 copies the online net
    if th is not None:
        assert torch.equal(_bits(th[:, :P]), _bits(torch.from_numpy(want).to(h16).to(DEV)))
        assert (th[:, P:] == 7.0).all()  # the padding is not written
    with pytest.raises(RuntimeError, match="tau"):
        load_ops().target_soft_update_hp(params, target, th, PRECISIONS[precision], tau_a[:2],
                                         omt_a)


def test_agent_soft_update_uses_the_swept_tau():
    ag = _agent("fp16", E=3, A=2, sweep=dict(tau=[0.005, 0.5]))
    ag.learn()
    t0 = ag.target.cpu().numpy()
    ag.update_target_network_soft()
    taus = [ag.variants[v]["tau"] for v in ag.variant_of_env.tolist() for _ in range(ag.A)]
    want = np.stack([soft_update_np(ag.params[i].cpu().numpy(), t0[i], taus[i])
                     for i in range(ag.NA)])
    assert np.array_equal(ag.target.cpu().numpy().view(np.int32), want.view(np.int32))
    _same(ag.target_h[:, :ag.P], torch.from_numpy(want).to(torch.float16).to(DEV), "shadow")


# --------------------------------------------------------------------------- 5
@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_c_abi_null_block_is_the_scalar_entry(precision, lib_option):
    """dmdqn_learn_hp with hp = NULL, and with a block of NULL arrays, leaves
    the bits of dmdqn_learn."""
    from dmdqn_amd.agent import CHParams
    lib_option("soft_path", "fused")
    a, b, c = (_agent(precision) for _ in range(3))
    for k in range(1, LEARNS + 1):
        for ag in (a, b, c):
            assert ag.learn_begin()
        args = [ag.c_learn_args() for ag in (a, b, c)]
        _lib.call("dmdqn_learn", ctypes.byref(args[0]), _lib.stream_of())
        _lib.call("dmdqn_learn_hp", ctypes.byref(args[1]), None, _lib.stream_of())
        null = CHParams(None, None, None, None, 0.0, 0.0)  # (the factors are not read)
        _lib.call("dmdqn_learn_hp", ctypes.byref(args[2]), ctypes.byref(null), _lib.stream_of())
        for other in (b, c):
            _same(a.loss, other.loss, f"learn {k} loss")
            _assert_same(a, other, what=f"learn {k} ")


@pytest.mark.parametrize("precision,split", [("fp32", False), ("fp16", False), ("fp16", True)])
def test_c_abi_equals_the_operator(precision, split, lib_option):
    lib_option("soft_path", "fused")
    sweep = dict(learning_rate=[1e-3, 2e-4], gamma=[0.99, 0.9], tau=[0.005, 0.5])
    voe = [0, 7]
    a = _agent(precision, sweep=sweep, variant_of_env=voe)
    b = _agent(precision, sweep=sweep, variant_of_env=voe)
    a.set_split_learn(split)
    grad = torch.empty((b.NA, b.P), dtype=torch.float32, device=DEV) if split else None
    for k in range(1, LEARNS + 1):
        la = a.learn()
        assert b.learn_begin()
        args, hp = b.c_learn_args(), b.c_learn_hparams()
        assert hp.lr == b.hp_lr.data_ptr() and hp.one_minus_tau == b.hp_omt.data_ptr()
        if split:
            _lib.call("dmdqn_learn_grad_hp", ctypes.byref(args), ctypes.byref(hp), _lib.ptr(grad),
                      _lib.stream_of())
            _lib.call("dmdqn_adam_agents_hp", ctypes.byref(args), ctypes.byref(hp), _lib.ptr(grad),
                      _lib.stream_of())
        else:
            _lib.call("dmdqn_learn_hp", ctypes.byref(args), ctypes.byref(hp), _lib.stream_of())
        _same(la, b.loss, f"learn {k} loss")
        _assert_same(a, b, what=f"learn {k} ")


def test_operator_checks_its_per_agent_tensors():
    a = _agent("fp16", sweep=dict(gamma=[0.9, 0.99]))
    assert a.learn_begin()
    good = a.hp_gamma
    for bad, match in ((good[:3], "elements"), (good.double(), "Float"), (good.cpu(), "device"),
                       (torch.stack([good, good], 1)[:, 0], "contiguous")):
        a.hp_gamma = bad
        with pytest.raises(RuntimeError, match=match):
            a.learn_range(0, a.NA)
    a.hp_gamma = good
    a.learn_range(0, a.NA)


# --------------------------------------------------------------------------- 6
# 2x2 grid (A = 4), E = 4, G = 2: replicas 0, 2 run variant 0 and 1, 3 variant 1.
TR_SWEEP = dict(learning_rate=[1e-3, 2e-4], gamma=[0.9], tau=[0.02])
TR_STEPS = 138  # the learns start at step 128 (batch_size transitions): 11 learns


def _trainer(overlap="none", E=4, sweep=None, side_learn=0, **hp):
    return Trainer(EnvConfig(rows=2, cols=2, num_envs=E, seed=11),
                   AgentConfig(replay_buffer_size=300, target_update_frequency=3, seed=4,
                               precision="fp16", sweep=sweep, **hp),
                   overlap=overlap, side_learn=side_learn)


def _run(tr, n, stats_last=False):
    for i in range(n):
        tr.step(collect_stats=stats_last and i == n - 1)
    tr.sync_outputs()
    tr.synchronize()


@pytest.fixture(scope="module")
def scalar_trainers():
    """One scalar Trainer per variant of TR_SWEEP, same env config, run once."""
    from dmdqn_amd.agent import sweep_variants
    out = []
    for v in sweep_variants(AgentConfig(sweep=TR_SWEEP)):
        tr = _trainer("none", **v)
        _run(tr, TR_STEPS, stats_last=True)
        assert tr.agent.learn_launches == TR_STEPS - 127
        out.append(tr)
    assert not torch.equal(out[0].agent.params, out[1].agent.params)
    return out


@pytest.mark.parametrize("overlap,side_learn", [("env", 6), ("none", 0)])
def test_trainer_sweep_equals_scalar_trainers(overlap, side_learn, scalar_trainers):
    tr = _trainer(overlap, sweep=TR_SWEEP, side_learn=side_learn)
    ag = tr.agent
    assert ag.variant_of_env.tolist() == [0, 1, 0, 1] and ag.A == 4
    _run(tr, TR_STEPS, stats_last=True)
    assert ag.learn_launches == TR_STEPS - 127
    A = ag.A
    for e in range(tr.env.E):
        rows, ref = slice(e * A, (e + 1) * A), scalar_trainers[e % 2].agent
        _assert_same(ag, ref, what=f"env {e} ", rows=rows)
        _same(ag.loss[rows], ref.loss[rows], f"env {e} loss")
        assert torch.equal(ag.qstats[rows], ref.qstats[rows])
    # the per-variant metrics are the unsplit ones, split
    whole, parts = ag.learn_metrics(), ag.learn_metrics(by_variant=True)
    assert [p["variant"] for p in parts] == [0, 1] and [p["envs"] for p in parts] == [2, 2]
    assert [p["learning_rate"] for p in parts] == [1e-3, 2e-4]
    assert all(p["gamma"] == 0.9 and p["tau"] == 0.02 for p in parts)
    assert np.sum([p["action_distribution"] for p in parts], 0).tolist() == \
        whole["action_distribution"]
    assert sum(whole["action_distribution"]) == ag.NA * 128
    # equal-sized variants: the mean of the means, up to float64 summation order
    for key in ("loss", "q_values_mean", "q_values_std"):
        np.testing.assert_allclose(np.mean([p[key] for p in parts]), whole[key], rtol=1e-12)
    vr = tr.variant_rewards()
    total = tr.last_reward.double().sum(dim=1).cpu()
    assert vr == [float(total[[0, 2]].mean()), float(total[[1, 3]].mean())]
    # the device-side form (no sync; float64 sums in another order)
    dev = tr.variant_rewards_device()
    assert dev.is_cuda and dev.dtype == torch.float64
    np.testing.assert_allclose(dev.cpu().numpy(), vr, rtol=1e-12)


def test_trainer_shard_holds_the_global_variants():
    """A rank that owns replicas [1, 3) of the run above gives them the
    variants (and the bits) the single-process run gives them."""
    tr = Trainer(EnvConfig(rows=2, cols=2, num_envs=2, seed=11, env_offset=1),
                 AgentConfig(replay_buffer_size=300, target_update_frequency=3, seed=4,
                             precision="fp16", sweep=TR_SWEEP))
    assert tr.agent.variant_of_env.tolist() == [1, 0]


# --------------------------------------------------------------------------- 7
def test_checkpoint_resume_is_bit_exact_and_refuses_another_sweep(tmp_path):
    K = 6
    ref = _trainer("none", E=2, sweep=TR_SWEEP)
    _run(ref, 132)
    path = os.path.join(str(tmp_path), "ck.pt")
    CK.save(path, ref)
    _run(ref, K)
    tr2 = _trainer("none", E=2, sweep=TR_SWEEP)
    CK.load(path, tr2)
    _run(tr2, K)
    _assert_same(ref.agent, tr2.agent)
    _same(ref.agent.loss, tr2.agent.loss, "loss")
    assert torch.equal(ref.obs, tr2.obs)
    assert ref.agent.learn_step_counter == tr2.agent.learn_step_counter == 132 + K - 127
    other = dict(TR_SWEEP, learning_rate=[1e-3, 3e-4])
    for cfg in (dict(sweep=other), dict(sweep=None)):
        with pytest.raises(ValueError, match="sweep"):
            CK.load(path, _trainer("none", E=2, **cfg))
    # the assignment is stored too: the same sweep with the replicas' variants
    # swapped (a BatchedDQN takes any assignment) is refused
    st = torch.load(path, map_location="cpu", weights_only=True)
    assert st["variant_of_env"] == [0, 1]
    st["variant_of_env"] = [1, 0]
    swapped = os.path.join(str(tmp_path), "swapped.pt")
    torch.save(st, swapped)
    with pytest.raises(ValueError, match="variant_of_env"):
        CK.load(swapped, tr2)
