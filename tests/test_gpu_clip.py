"""Global-norm gradient clipping on the GPU (dmdqn_adam_agents_clip,
AgentConfig.global_clipnorm): the kernel bit for bit against the numpy
restatement (clip_ref.py) on synthetic gradients and through BatchedDQN, with
hard syncs, soft updates and a swept learning rate; clipping off is the code as
it was; a clip far above every norm leaves the fused learn's bits; the trainer's
schedules agree; the split learn's limits are refused at construction.

Bit equality rests on one condition, not a tolerance: the kernel's f64 sum of
squares (any order) is within P * 2^-53 < 2^-38 relative of the exact sum, so
its float32 norm is the reference's whenever sqrt(S) is further than that from
a float32 rounding boundary -- clip_ref.boundary_margin(S) > 2^-36, asserted
for every finite agent of the synthetic fixture (its builder moves to another
seed otherwise).  The gradients the learn itself exports are compared bit for
bit as they come; a mismatch there reports the agent's margin."""
import ctypes
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import clip_ref as CR  # noqa: E402
from dmdqn_amd.agent import (AgentConfig, BatchedDQN, CLearn, PRECISIONS,  # noqa: E402
                             keras_adam_consts, keras_adam_factors, n_params,
                             soft_update_consts)
from dmdqn_amd.env import EnvConfig  # noqa: E402
from dmdqn_amd.trainer import Trainer  # noqa: E402

DEV = "cuda"
P = n_params(128)
MARGIN = 2.0 ** -36
f32 = np.float32
H16 = {"fp16": torch.float16, "bf16": torch.bfloat16}


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.int32)


def _to16(x, precision):
    """float32 values rounded to the 16-bit type (RNE), as float32."""
    return torch.from_numpy(np.asarray(x, np.float32)).to(H16[precision]).float().numpy()


# --------------------------------------------------------------------------- 1. entry point
MAIN_CLIP = f32(40.0)
AGENTS = ("zeros", "big", "tiny", "first", "random_hi", "inf", "random_lo", "last", "edge")


def _build(precision, seed):
    rs = np.random.RandomState(seed)

    def rnd(lo, hi):  # magnitudes 2^lo .. 2^hi, log-uniform, random signs
        x = 2.0 ** rs.uniform(lo, hi, P) * rs.choice([-1.0, 1.0], P)
        return _to16(x.astype(np.float32), precision)
    big = 65504.0 if precision == "fp16" else 2.0 ** 100  # S stays finite in f64
    g = {"zeros": np.zeros(P, np.float32),
         "big": (big * rs.choice([-1.0, 1.0], P)).astype(np.float32),
         "tiny": np.full(P, 2.0 ** -24, np.float32),
         "first": np.zeros(P, np.float32), "last": np.zeros(P, np.float32),
         "random_hi": rnd(-20, 4), "random_lo": rnd(-20, 0), "edge": rnd(-20, 2),
         "inf": rnd(-20, 4)}
    g["first"][0] = 3.0
    g["last"][P - 1] = -0.75  # the last float4 group: the workgroup's partly filled round
    g["inf"][1234] = np.inf
    grad = np.stack([g[k] for k in AGENTS])
    assert np.array_equal(grad, _to16(grad, precision))  # 16-bit values, as the learn exports
    state = {"params": (rs.standard_normal((len(AGENTS), P)) * 0.1).astype(np.float32),
             "adam_m": (rs.standard_normal((len(AGENTS), P)) * 1e-3).astype(np.float32),
             "adam_v": (np.abs(rs.standard_normal((len(AGENTS), P))) * 1e-4).astype(np.float32)}
    S = [CR.sum_squares(row) for row in grad]
    return grad, state, S


@functools.lru_cache(maxsize=None)
def fixture_of(precision):
    """(grad, state, S, clips) -- the first seed at which every finite agent is
    clear of a float32 rounding boundary.  No agent is ever left out."""
    for seed in range(100, 120):
        grad, state, S = _build(precision, seed)
        if all(CR.boundary_margin(s) > MARGIN for s in S):
            break
    else:
        raise AssertionError("no seed clears the float32 rounding boundaries")
    norms = {k: CR.norm_of(s) for k, s in zip(AGENTS, S)}
    assert norms["zeros"] == 0 and np.isinf(norms["inf"])
    assert norms["random_lo"] < MAIN_CLIP < f32(0.25) * norms["random_hi"]
    assert norms["tiny"] < MAIN_CLIP < norms["big"]
    e = norms["edge"]
    up = np.nextafter(np.nextafter(e, f32(np.inf)), f32(np.inf))
    dn = np.nextafter(np.nextafter(e, f32(0)), f32(0))
    clips = {"main": MAIN_CLIP, "edge+2ulp": up, "edge-2ulp": dn, "edge": e}
    return grad, state, S, clips


@pytest.mark.parametrize("which", ["main", "edge+2ulp", "edge-2ulp", "edge"])
@pytest.mark.parametrize("precision", ["fp16", "bf16"])
def test_entry_point_bit_exact_on_synthetic_gradients(precision, which):
    from dmdqn_amd import _lib
    grad, state, S, clips = fixture_of(precision)
    for k, s in zip(AGENTS, S):
        if np.isfinite(s):
            assert CR.boundary_margin(s) > MARGIN, k
    clip = clips[which]
    alpha, c1, c2, eps = keras_adam_consts(7, 1e-3)
    NA = len(AGENTS)
    dev = {k: torch.from_numpy(v).to(DEV) for k, v in state.items()}
    g_dev = torch.from_numpy(grad).to(DEV)
    target = torch.zeros((NA, P), dtype=torch.float32, device=DEV)
    gnorm = torch.full((NA,), -1.0, dtype=torch.float32, device=DEV)
    a = CLearn()
    a.NA, a.cap, a.batch, a.hidden, a.precision, a.P = NA, 302, 128, 128, PRECISIONS[precision], P
    a.params, a.adam_m, a.adam_v = (dev[k].data_ptr() for k in ("params", "adam_m", "adam_v"))
    a.target = target.data_ptr()
    a.alpha, a.c1, a.c2, a.eps = alpha, c1, c2, eps
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.call("dmdqn_adam_agents_clip", ctypes.byref(a), None, ctypes.c_void_p(g_dev.data_ptr()),
              ctypes.c_float(float(clip)), ctypes.c_void_p(gnorm.data_ptr()), stream)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in dev.items()}
    got_norm = gnorm.cpu().numpy()
    assert np.array_equal(_bits(g_dev.cpu().numpy()), _bits(grad))  # grad is read-only
    assert not target.any()  # TGT_NONE
    for i, k in enumerate(AGENTS):
        norm, p1, m1, v1 = CR.clip_adam(state["params"][i], state["adam_m"][i],
                                        state["adam_v"][i], grad[i], clip, alpha, c1, c2, eps)
        if k == "inf":  # NaN everywhere; its neighbours are checked like everyone
            assert np.isinf(got_norm[i]) and got_norm[i] > 0
            for name in ("params", "adam_m", "adam_v"):
                assert np.isnan(got[name][i]).all(), name
            continue
        assert _bits(got_norm[i]) == _bits(norm), (k, got_norm[i], norm)
        for name, want in (("adam_m", m1), ("adam_v", v1), ("params", p1)):
            bad = int((_bits(got[name][i]) != _bits(want)).sum())
            assert bad == 0, (k, name, bad)
    if which != "main":  # the edge agent sits 2 ulps under / over / on the clip
        e = CR.norm_of(S[AGENTS.index("edge")])
        assert abs(int(_bits(clip)[0]) - int(_bits(e)[0])) == (0 if which == "edge" else 2)


# --------------------------------------------------------------------------- 2. through the agent
def _fill(ag, n, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    for t in range(n):
        s = torch.randint(-1, 24, (ag.E, ag.A, 89), device=DEV, generator=g).float()
        a = torch.randint(0, 4, (ag.E, ag.A), device=DEV, generator=g, dtype=torch.int32)
        r = -torch.rand((ag.E, ag.A), device=DEV, generator=g, dtype=torch.float64) * 100
        ag.remember(s, a, r, s.flip(-1), t % 50 == 49)


VARIANTS = {"plain": {}, "hard": dict(target_update_frequency=2),
            "soft": dict(tau=0.01, target_update_frequency=0),
            "swept": dict(sweep={"learning_rate": [1e-4, 1e-3]})}


def _agent(precision, clip, kw):
    ag = BatchedDQN(4, 4, AgentConfig(precision=precision, seed=6, replay_buffer_size=300,
                                      global_clipnorm=clip, **kw))
    _fill(ag, 130, 2)
    return ag


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("precision", ["fp16", "bf16"])
def test_agent_learns_are_the_rule_on_the_exported_gradient(precision, variant):
    kw = VARIANTS[variant]
    probe = _agent(precision, 1.0, kw)
    assert probe.split_learn and probe.grad_norm is not None
    probe.learn()
    first = np.sort(probe.grad_norm.cpu().numpy())
    del probe
    # between the 8th and 9th of the first learn's 16 norms (they do not depend on the clip)
    assert first[7] < first[8]
    clip = float(f32((float(first[7]) + float(first[8])) / 2))
    ag = _agent(precision, clip, kw)
    cfg = ag.cfg
    assert ag.split_learn and ag.clipnorm == clip
    tau_f, omt_f = soft_update_consts(cfg.tau)
    seen = set()
    for k in range(4):
        _fill(ag, 1, 50 + k)
        before = {n: getattr(ag, n).cpu().numpy().copy()
                  for n in ("params", "adam_m", "adam_v", "target")}
        th0 = ag.target_h.clone()
        ag.learn(collect_stats=True)
        t = ag.learn_step_counter
        g = ag._split_grad.cpu().numpy()
        got = {n: getattr(ag, n).cpu().numpy() for n in before}
        got_norm = ag.grad_norm.cpu().numpy()
        alpha, c1, c2, eps = keras_adam_consts(t, cfg.learning_rate)
        alphas = [alpha] * ag.NA
        if variant == "swept":
            s, d = keras_adam_factors(t)
            alphas = [f32(f32(lr) * s) / d for lr in ag.hp_lr.cpu().numpy()]
            assert len({float(x) for x in alphas}) == 2
        want_t = np.empty_like(before["target"])
        n_clipped = 0
        for i in range(ag.NA):
            norm, p1, m1, v1 = CR.clip_adam(before["params"][i], before["adam_m"][i],
                                            before["adam_v"][i], g[i], f32(clip), alphas[i], c1,
                                            c2, eps)
            n_clipped += bool(norm > f32(clip))
            # (the margin in the message: a real gradient may sit closer to a
            # rounding boundary than the synthetic fixture's condition allows)
            assert _bits(got_norm[i]) == _bits(norm), (
                k, i, got_norm[i], norm, CR.boundary_margin(CR.sum_squares(g[i])))
            for name, want in (("adam_m", m1), ("adam_v", v1), ("params", p1)):
                bad = int((_bits(got[name][i]) != _bits(want)).sum())
                assert bad == 0, (k, i, name, bad)
            sync = cfg.target_update_frequency > 0 and t % cfg.target_update_frequency == 0
            want_t[i] = (p1 if sync else CR.soft_target(p1, before["target"][i], tau_f, omt_f)
                         if cfg.tau > 0 else before["target"][i])
        assert np.array_equal(_bits(got["target"]), _bits(want_t)), k
        changed = variant == "soft" or (variant == "hard" and t % 2 == 0)
        want_h = torch.from_numpy(want_t).to(H16[precision]) if changed else th0[:, :P].cpu()
        assert torch.equal(ag.target_h[:, :P].cpu().view(torch.int16), want_h.view(torch.int16)), k
        met = ag.learn_metrics()
        assert met["clipped_frac"] == n_clipped / ag.NA
        assert met["grad_norm_max"] == float(got_norm.max())
        assert met["grad_norm_mean"] == pytest.approx(float(got_norm.astype(np.float64).mean()),
                                                      rel=1e-12)
        seen |= {"clipped"} if n_clipped else set()
        seen |= {"unclipped"} if n_clipped < ag.NA else set()
        if k == 0:
            assert n_clipped == 8
    assert seen == {"clipped", "unclipped"}


# --------------------------------------------------------------------------- 3. off is off
@pytest.mark.parametrize("precision", ["fp16", "bf16"])
def test_off_is_off(precision):
    out = []
    for kw in ({}, {"global_clipnorm": 0.0}):
        ag = BatchedDQN(4, 4, AgentConfig(precision=precision, seed=6, replay_buffer_size=300,
                                          target_update_frequency=2, **kw))
        assert not ag.split_learn and ag.grad_norm is None and ag._split_grad is None
        _fill(ag, 130, 2)
        losses = []
        for k in range(3):
            _fill(ag, 1, 50 + k)
            losses.append(ag.learn(collect_stats=True).clone())
        met = ag.learn_metrics()
        assert not {"grad_norm_mean", "grad_norm_max", "clipped_frac"} & set(met)
        out.append(([torch.stack(losses)] + [getattr(ag, n).clone() for n in
                                             ("params", "adam_m", "adam_v", "target", "target_h")],
                    met))
    for a, b in zip(out[0][0], out[1][0]):
        bits = torch.int32 if a.element_size() == 4 else torch.int16
        assert torch.equal(a.view(bits), b.view(bits))
    assert out[0][1] == out[1][1]


# --------------------------------------------------------------------------- 4. a huge clip
@pytest.mark.parametrize("precision", ["fp16", "bf16"])
def test_huge_clip_leaves_the_fused_learns_bits(precision):
    clip = 2.0 ** 40
    for norm in (0.0, 1e-3, 1.0, 1e6):  # far above any norm: the scale is exactly 1
        assert _bits(CR.clip_scale(f32(norm), f32(clip))) == _bits(f32(1.0))
    state = {}
    for c in (0.0, clip):
        ag = BatchedDQN(4, 4, AgentConfig(precision=precision, seed=3, replay_buffer_size=400,
                                          target_update_frequency=4, global_clipnorm=c))
        assert ag.split_learn == (c > 0)
        _fill(ag, 130, 1)
        losses = []
        for k in range(6):  # one target sync
            _fill(ag, 1, 100 + k)
            losses.append(ag.learn().clone())
            if c > 0:
                assert float(ag.grad_norm.max()) < clip
        torch.cuda.synchronize()
        state[c] = [torch.stack(losses)] + [getattr(ag, n).clone() for n in
                                            ("params", "adam_m", "adam_v", "target", "target_h")]
    for a, b in zip(state[0.0], state[clip]):
        bits = torch.int32 if a.element_size() == 4 else torch.int16
        assert torch.equal(a.view(bits), b.view(bits))


# --------------------------------------------------------------------------- 5. schedules
def test_trainer_schedules_bit_identical_with_clipping():
    """2x2 grid x 8 replicas, 140 steps (13 learns), replay 200: the one-stream
    order, the "env" schedule and the "env" schedule with a side-stream learn
    range.  Clipping runs every learn alone: nothing is paired."""
    res = {}
    for name, kw in (("none", dict(overlap="none")), ("env", dict(overlap="env")),
                     ("env+side", dict(overlap="env", side_learn=12))):
        tr = Trainer(EnvConfig(rows=2, cols=2, num_envs=8, seed=4),
                     AgentConfig(precision="fp16", replay_buffer_size=200, seed=4,
                                 global_clipnorm=1.0), **kw)
        assert tr.agent.split_learn and tr.agent.NA == 32
        losses, norms = [], []
        for _ in range(140):
            tr.step()
            if tr.last_loss is not None:
                losses.append(tr.last_loss.clone())
                norms.append(tr.agent.grad_norm.clone())
        torch.cuda.synchronize()
        assert tr.agent.pair_launches == 0 and len(losses) == 13
        res[name] = (torch.stack(losses).cpu(), torch.stack(norms).cpu(), tr.agent.params.cpu(),
                     tr.agent.adam_v.cpu(), tr.obs.cpu())
        del tr
        torch.cuda.empty_cache()
    assert bool((res["none"][1] > 0).all())
    for name in ("env", "env+side"):
        for a, b in zip(res["none"], res[name]):
            np.testing.assert_array_equal(a.numpy(), b.numpy())


# --------------------------------------------------------------------------- 6. refusals
@pytest.mark.parametrize("kw", [dict(precision="fp32"), dict(precision="fp16", shared_params=True),
                                dict(precision="fp16", replay_rows="f32")])
def test_refusals_at_construction(kw):
    with pytest.raises(ValueError, match="global_clipnorm"):
        BatchedDQN(2, 2, AgentConfig(global_clipnorm=1.0, **kw))
    ag = BatchedDQN(2, 2, AgentConfig(precision="fp16", global_clipnorm=1.0))
    with pytest.raises(ValueError, match="global_clipnorm"):
        ag.set_split_learn(False)
