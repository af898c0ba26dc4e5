"""Dead-unit recycling on the GPU: dmdqn_redo bit for bit against the Keras-order
restatement (redo_ref.py) on the exact-forward fixtures, through ctypes, the
operator and BatchedDQN.redo(); the patience and clean-net cases; the host
refusals; and Trainers whose runs are bit-identical across schedules, across a
checkpoint, and -- while no unit fires -- with and without the feature."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import exact_fixture as XF  # noqa: E402
import health_ref as HR  # noqa: E402
import redo_ref as RR  # noqa: E402
from dmdqn_amd import checkpoint as CK  # noqa: E402
from dmdqn_amd import kernels as K  # noqa: E402
from dmdqn_amd._lib import CRedo, call, stream_of  # noqa: E402
from dmdqn_amd.agent import (AgentConfig, BatchedDQN, keras_to_kernel,  # noqa: E402
                             kernel_to_keras)
from dmdqn_amd.env import EnvConfig  # noqa: E402
from dmdqn_amd.trainer import Trainer  # noqa: E402

DEV = "cuda"
L1_DEAD, L2_DEAD = (0, 5, 17, 64, 127), (3, 31, 96)  # agent 0
OTHER, OTHER_L1, OTHER_L2 = 3, 40, 41                 # one more agent: the overlap entry


def _var(nets, j, name, H=128):
    o, sh = XF.block_slices(H)[name]
    return nets[j, o:o + int(np.prod(sh))].reshape(sh)


def _dead_nets(fx):
    """The fixture's online nets (Keras order): agent 0 with layer-1 units
    {0, 5, 17, 64, 127} and layer-2 units {3, 31, 96} dead (a first, middle and
    last unit, two units of one 16-tile, both halves of an 8-group), agent 3
    with one dead unit per layer, the others clean."""
    nets = fx.online.astype(np.float32).copy()
    for j, l1, l2 in ((0, L1_DEAD, L2_DEAD), (OTHER, (OTHER_L1,), (OTHER_L2,))):
        for u in l1:
            _var(nets, j, "W1")[:, u] = 0.0
            _var(nets, j, "b1")[u] = -1.0 if u in (5, 64) else 0.0
        for u in l2:
            _var(nets, j, "W2")[:, u] = 0.0
            _var(nets, j, "b2")[u] = 0.0
    return nets


def _agent(fx, nets, **kw):
    """test_gpu_health._agent's ring load: cap 160, fill 200, start 40."""
    cfg = AgentConfig(replay_buffer_size=fx.cap, nn_layers=[fx.H, fx.H], seed=fx.seed,
                      target_update_frequency=500, precision=fx.precision, **kw)
    ag = BatchedDQN(fx.E, fx.A, cfg, init_weights=nets)
    shape = (fx.fill, fx.E, fx.A)
    s = torch.from_numpy(fx.obs_s.astype(np.float32).reshape(shape + (89,))).to(DEV)
    n = torch.from_numpy(fx.obs_n.astype(np.float32).reshape(shape + (89,))).to(DEV)
    a = torch.from_numpy(fx.act.reshape(shape)).to(DEV)
    r = torch.from_numpy(fx.rew.reshape(shape)).to(DEV)
    d = torch.from_numpy(fx.done).to(DEV)
    for t in range(fx.fill):
        ag.remember(s[t], a[t], r[t], n[t], d[t])
    ag.ring.check()
    assert ag.ring.start == 40 and len(ag.ring) == fx.cap
    # Adam moments: non-zero, position-coded (exact f32 values)
    n_all = ag.NA * ag.P
    code = torch.arange(1, n_all + 1, dtype=torch.float32, device=DEV).view(ag.NA, ag.P)
    ag.adam_m.copy_(code * 2.0 ** -20)
    ag.adam_v.copy_(code * 2.0 ** -20 + 0.5)
    return ag


def _i32(t):
    return t.contiguous().view(torch.int32).cpu().numpy()


def _want(params, m, v, streak, mask, patience, seed, rnd, agent0):
    """The restatement on device-layout host arrays, back in the device layout."""
    got = RR.redo_ref(kernel_to_keras(params, 128), kernel_to_keras(m, 128),
                      kernel_to_keras(v, 128), streak, mask, patience, seed, rnd, agent0)
    return tuple(keras_to_kernel(x, 128) for x in got[:3]) + got[3:]


def _check(got, want, what):
    """got: device (params, m, v, streak, recycled, n_recycled)."""
    for name, g, w in zip(("params", "adam_m", "adam_v"), got[:3], want[:3]):
        np.testing.assert_array_equal(_i32(g), w.view(np.int32), err_msg=f"{what}: {name}")
    np.testing.assert_array_equal(got[3].cpu().numpy(), want[3], err_msg=f"{what}: streak")
    np.testing.assert_array_equal(got[4].cpu().numpy().view(np.uint32), want[4],
                                  err_msg=f"{what}: recycled")
    np.testing.assert_array_equal(got[5].cpu().numpy(), want[5], err_msg=f"{what}: n_recycled")


def _state(ag):
    """Clones of (params, m, v, streak = 0, recycled = -1, n_recycled = -1)."""
    return (ag.params.clone(), ag.adam_m.clone(), ag.adam_v.clone(),
            torch.zeros((ag.NA, 2, 128), dtype=torch.uint8, device=DEV),
            torch.full((ag.NA, 2, 4), -1, dtype=torch.int32, device=DEV),
            torch.full((ag.NA, 2), -1, dtype=torch.int32, device=DEV))


def _ctypes_redo(mask, st, patience, seed, rnd, agent0):
    a = CRedo()
    a.NA, a.P, a.hidden, a.agent0, a.patience = st[0].shape[0], st[0].shape[1], 128, agent0, patience
    a.round, a.seed, a.lim1, a.lim2 = rnd, seed, K.REDO_LIM1, K.REDO_LIM2
    a.dead_mask = mask.data_ptr()
    for f, t in zip(("params", "adam_m", "adam_v", "streak", "recycled", "n_recycled"), st):
        setattr(a, f, t.data_ptr())
    call("dmdqn_redo", C.byref(a), stream_of())


# --------------------------------------------------------------------------- 1. the kernel
@pytest.mark.parametrize("name", ["f16", "bf16"])
def test_kernel_is_the_restatement_bit_for_bit(name):
    fx = XF.fixture(name)
    assert fx.NA == 6 and fx.cap == 160 and fx.fill == 200
    nets = _dead_nets(fx)
    ag = _agent(fx, nets)
    idx = torch.from_numpy(fx.idx).to(DEV)
    untouched = {k: getattr(ag, k).clone() for k in ("target", "target_h", "np_state", "py_state")}
    untouched.update({"ring_" + k: getattr(ag.ring, k).clone() for k in ("s", "n", "a", "r", "d")})
    mask = ag.probe_health(idx)["dead_mask"].clone()
    # the probe's mask is the restatement's: the dead units above, nothing else
    want_mask = np.zeros((fx.NA, 2, 4), np.uint32)
    for j in (0, OTHER):
        want_mask[j] = HR.probe_ref(XF.split(nets[j].astype(np.float64), fx.H), fx.batch(j)[0],
                                    fx.precision)[2]
    bits = RR.mask_bits(want_mask)
    assert np.flatnonzero(bits[0, 0]).tolist() == list(L1_DEAD)
    assert np.flatnonzero(bits[0, 1]).tolist() == list(L2_DEAD)
    assert np.flatnonzero(bits[OTHER, 0]).tolist() == [OTHER_L1]
    assert np.flatnonzero(bits[OTHER, 1]).tolist() == [OTHER_L2]
    np.testing.assert_array_equal(mask.cpu().numpy().view(np.uint32), want_mask)

    host = [t.cpu().numpy() for t in (ag.params, ag.adam_m, ag.adam_v)]
    streak0 = np.zeros((fx.NA, 2, 128), np.uint8)
    seed = 0x9ABCDEF012345678  # the seed is a u64
    runs = {}
    # (the last: round + 1 is formed in u64)
    for agent0, rnd in ((0, 0), (4099, 0), (7, 0xFFFFFFFF)):
        want = _want(*host, streak0, want_mask, 1, seed, rnd, agent0)
        assert want[5].tolist() == [[5, 3], [0, 0], [0, 0], [1, 1], [0, 0], [0, 0]]
        st = _state(ag)
        _ctypes_redo(mask, st, 1, seed, rnd, agent0)
        torch.cuda.synchronize()
        _check(st, want, f"ctypes agent0={agent0}")
        st2 = _state(ag)
        K.redo(mask, st2[3], st2[0], st2[1], st2[2], 128, agent0, seed, rnd, 1, st2[4], st2[5])
        torch.cuda.synchronize()
        _check(st2, want, f"op agent0={agent0}")
        runs[agent0] = want
    # another global index draws other weights (and only the weights differ)
    assert not np.array_equal(runs[0][0], runs[4099][0])
    np.testing.assert_array_equal(runs[0][1], runs[4099][1])
    # the overlap entry exists and is zero; fresh beside it
    W2 = XF.split(kernel_to_keras(runs[0][0], 128)[OTHER], 128)[2]
    assert W2[OTHER_L1, OTHER_L2] == 0.0 and W2[OTHER_L1 + 1, OTHER_L2] != 0.0

    # BatchedDQN.redo(): probe + recycle on the agent's own tensors, keyed by
    # cfg.seed, the learn step counter (0) and env_offset * A (0)
    want = _want(*host, streak0, want_mask, 1, fx.seed, 0, 0)
    last = ag.redo(idx)
    torch.cuda.synchronize()
    _check((ag.params, ag.adam_m, ag.adam_v, ag.redo_streak, last["recycled"],
            last["n_recycled"]), want, "BatchedDQN.redo")
    assert ag.redo_total.tolist() == [6, 4] and ag.redo_rounds == 1
    assert int(last["learn_step"]) == 0
    for k, t in untouched.items():
        now = getattr(ag.ring, k[5:]) if k.startswith("ring_") else getattr(ag, k)
        assert torch.equal(now.view(torch.uint8), t.view(torch.uint8)), k
    # the function on the probed batch is unchanged: a second probe sees the
    # same Q (its largest |q|) and the recycled layer-1 units alive or dead by
    # their fresh weights, no longer by zeros
    h = ag.probe_health(idx)
    torch.cuda.synchronize()
    q_before = [HR.probe_ref(XF.split(nets[j].astype(np.float64), fx.H), fx.batch(j)[0],
                             fx.precision)[1][4] for j in range(fx.NA)]
    assert h["stats"][:, 4].cpu().tolist() == q_before


# --------------------------------------------------------------------------- 2. patience
def test_patience_two_fires_on_the_second_dead_probe():
    fx = XF.fixture("bf16")
    ag = _agent(fx, _dead_nets(fx))
    idx = torch.from_numpy(fx.idx).to(DEV)
    mask = ag.probe_health(idx)["dead_mask"].clone()
    live = torch.zeros_like(mask)
    mask_h = mask.cpu().numpy().view(np.uint32)
    host = [t.cpu().numpy() for t in (ag.params, ag.adam_m, ag.adam_v)]
    st = _state(ag)

    def launch(m, rnd):
        K.redo(m, st[3], st[0], st[1], st[2], 128, 0, 7, rnd, 2, st[4], st[5])
        torch.cuda.synchronize()

    # first dead probe: nothing but the streak (and the zero outputs) changes
    launch(mask, 1)
    w1 = _want(*host, np.zeros((fx.NA, 2, 128), np.uint8), mask_h, 2, 7, 1, 0)
    assert not w1[5].any() and w1[3].sum() == 10 and w1[3].max() == 1
    _check(st, w1, "first call")
    for g, h in zip(st[:3], host):
        np.testing.assert_array_equal(_i32(g), h.view(np.int32))
    # a live probe in between resets the streak
    launch(live, 2)
    assert not st[3].any() and not st[5].any()
    # two dead probes in a row: the second fires
    launch(mask, 3)
    _check(st, w1, "dead again")
    launch(mask, 4)
    w2 = _want(*w1[:3], w1[3], mask_h, 2, 7, 4, 0)
    assert w2[5].tolist() == [[5, 3], [0, 0], [0, 0], [1, 1], [0, 0], [0, 0]] and not w2[3].any()
    _check(st, w2, "second call")
    assert not np.array_equal(w2[0], host[0])


# --------------------------------------------------------------------------- 3. clean nets
def test_clean_nets_write_nothing_but_the_streak_and_zero_counts():
    fx = XF.fixture("f16")
    ag = _agent(fx, fx.online.astype(np.float32).copy())
    idx = torch.from_numpy(fx.idx).to(DEV)
    mask = ag.probe_health(idx)["dead_mask"].clone()
    assert not mask.any()
    st = _state(ag)
    st[3].fill_(9)  # streaks of earlier dead probes: a live probe resets them
    K.redo(mask, st[3], st[0], st[1], st[2], 128, 0, 1, 1, 1, st[4], st[5])
    torch.cuda.synchronize()
    assert not st[3].any() and not st[4].any() and not st[5].any()
    for g, t in zip(st[:3], (ag.params, ag.adam_m, ag.adam_v)):
        assert torch.equal(g.view(torch.int32), t.view(torch.int32))


# --------------------------------------------------------------------------- 4. refusals
def test_host_refusals_launch_nothing():
    from dmdqn_amd import _lib
    from test_redo_cpu import check_host_refusals
    check_host_refusals(_lib.load())
    # through the operator, on real tensors: refused, nothing written
    NA, P = 2, XF.n_params(128)
    p = torch.ones((NA, P), device=DEV)
    m, v = p.clone(), p.clone()
    mask = torch.full((NA, 2, 4), -1, dtype=torch.int32, device=DEV)  # every unit dead
    streak = torch.zeros((NA, 2, 128), dtype=torch.uint8, device=DEV)
    for kw, word in ((dict(patience=0), "patience"), (dict(patience=256), "patience"),
                     (dict(agent0=-1), "agent0"), (dict(hidden=64), "hidden|streak")):
        args = dict(hidden=128, agent0=0, patience=1)
        args.update(kw)
        with pytest.raises(RuntimeError, match=word):
            K.redo(mask, streak, p, m, v, args["hidden"], args["agent0"], 1, 1, args["patience"])
    with pytest.raises(RuntimeError, match="P="):
        K.redo(mask, streak, p[:, :P - 4].contiguous(), m[:, :P - 4].contiguous(),
               v[:, :P - 4].contiguous(), 128, 0, 1, 1, 1)
    torch.cuda.synchronize()
    assert bool((p == 1).all()) and bool((m == 1).all()) and not streak.any()


# --------------------------------------------------------------------------- 5. the Trainer
E_TR, STEPS, CKPT_AT, EVERY = 6, 172, 150, 4
TR_STATE = ("params", "adam_m", "adam_v", "target", "target_h", "np_state", "py_state")


def _seed_dead_units(tr):
    """A few units that are dead whatever the input (zero incoming weights, bias
    -1: no gradient ever reaches them), in other agents and at other units per
    replica."""
    ag = tr.agent
    nets = ag.keras_params()
    for e in range(ag.E):
        j = e * ag.A + e % ag.A
        for u in (e, 64 + 3 * e, 127 - e):
            _var(nets, j, "W1")[:, u] = 0.0
            _var(nets, j, "b1")[u] = -1.0
        for o in (2 * e + 1, 100 + e):
            _var(nets, j, "W2")[:, o] = 0.0
            _var(nets, j, "b2")[o] = -1.0
    tr.quiesce()
    ag.params.copy_(torch.from_numpy(keras_to_kernel(nets, 128)))
    ag.target.copy_(ag.params)
    ag._refresh_target_h()
    tr.join_streams()


def _trainer(redo_every=EVERY, patience=1, overlap="none", pbt=None, **kw):
    extra = {}
    if pbt is not None:
        extra = dict(sweep={"learning_rate": [1e-4, 1e-3]}, pbt=pbt)
    tr = Trainer(EnvConfig(rows=2, cols=2, num_envs=E_TR, seed=5, max_sim_time=500),
                 AgentConfig(precision="bf16", replay_buffer_size=300, seed=5,
                             target_update_frequency=7, redo_every=redo_every,
                             redo_patience=patience, **extra, **kw), overlap=overlap)
    _seed_dead_units(tr)
    return tr


def _run(tr, steps, ckpt=None):
    for t in range(1, steps + 1):
        tr.step()
        if ckpt is not None and t == CKPT_AT:
            CK.save(ckpt, tr)
    tr.synchronize()


def _same(a, b, what, names=TR_STATE):
    for k in names:
        x, y = getattr(a.agent, k), getattr(b.agent, k)
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8)), f"{what}: {k}"
    for k in ("s", "n", "a", "r", "d"):
        x, y = getattr(a.agent.ring, k), getattr(b.agent.ring, k)
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8)), f"{what}: ring.{k}"
    assert torch.equal(a.obs, b.obs), what
    assert a.agent.learn_step_counter == b.agent.learn_step_counter


def _same_redo(a, b, what):
    assert torch.equal(a.agent.redo_streak, b.agent.redo_streak), what
    assert torch.equal(a.agent.redo_total, b.agent.redo_total), what
    assert a.agent.redo_rounds == b.agent.redo_rounds, what
    for k in ("recycled", "n_recycled", "learn_step"):
        assert torch.equal(a.agent.redo_last[k], b.agent.redo_last[k]), (what, k)


@pytest.fixture(scope="module")
def main_run(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("redo") / "mid.pt")
    tr = _trainer()
    _run(tr, STEPS, ckpt=path)
    return tr, path


def test_trainer_recycles_the_seeded_units(main_run):
    tr = main_run[0]
    ag = tr.agent
    learns = ag.learn_step_counter
    assert learns == STEPS - 127 and ag.redo_rounds == learns // EVERY
    # the first round fired every seeded unit (patience 1): 3 + 2 per replica
    total = ag.redo_total.tolist()
    print("recycled in total", total, "rounds", ag.redo_rounds)
    assert total[0] >= 3 * E_TR and total[1] >= 2 * E_TR
    nets = ag.keras_params()
    for e in range(E_TR):
        j = e * ag.A + e % ag.A
        for u in (e, 64 + 3 * e, 127 - e):
            assert _var(nets, j, "W1")[:, u].all()  # fresh, never 0
    rec = ag.learn_metrics()
    assert set(rec["redo"]) == {"rounds", "learn_step", "recycled", "recycled_total",
                                "agents_touched"}
    assert rec["redo"]["rounds"] == ag.redo_rounds and rec["redo"]["recycled_total"] == total
    assert rec["redo"]["learn_step"] == learns - learns % EVERY
    assert "health" not in rec  # health_every is off: the redo probe is not reported as one


def test_trainer_schedules_are_bit_identical(main_run):
    ref = main_run[0]
    tr = _trainer(overlap="env")
    _run(tr, STEPS)
    assert tr.side is not None and ref.side is None and tr.agent.pair_launches > 5
    _same(ref, tr, "env")
    _same_redo(ref, tr, "env")


def test_checkpoint_resumes_bit_identical(main_run):
    ref, path = main_run
    st = torch.load(path, map_location="cpu", weights_only=True)
    assert set(st["redo"]) == {"streak", "total", "rounds"}
    assert st["redo"]["rounds"] == (CKPT_AT - 127) // EVERY and st["redo"]["total"].sum() > 0
    tr = _trainer()
    CK.load(path, tr)
    _run(tr, STEPS - CKPT_AT)
    _same(ref, tr, "resumed")
    _same_redo(ref, tr, "resumed")
    # another schedule or patience, or none, is another run
    for other in (dict(redo_every=EVERY + 1), dict(patience=2), dict(redo_every=0)):
        with pytest.raises(ValueError, match="redo"):
            CK.load(path, _trainer(**other))


def test_no_fire_run_equals_the_run_without_the_feature():
    """redo_patience above the number of probes: the probe only reads and a
    no-fire launch only touches its own buffers, under the paired schedule."""
    off = _trainer(redo_every=0, overlap="env")
    _run(off, STEPS)
    on = _trainer(redo_every=EVERY, patience=255, overlap="env")
    _run(on, STEPS)
    assert off.agent.pair_launches > 5 and on.agent.pair_launches > 5
    _same(off, on, "patience 255")
    ag = on.agent
    assert ag.redo_total.tolist() == [0, 0] and ag.redo_rounds == (STEPS - 127) // EVERY
    # every seeded unit has been dead on every probe
    assert int(ag.redo_streak.max()) == ag.redo_rounds
    assert int((ag.redo_streak == ag.redo_rounds).sum()) >= 5 * E_TR
    assert off.agent.redo_streak is None and "redo" not in off.agent.learn_metrics()
    assert on.agent.learn_metrics()["redo"]["recycled"] == [0, 0]


def test_pbt_round_copies_the_streaks_with_the_nets():
    pbt = {"interval": 40, "truncation": 0.34, "seed": 3}
    tr = _trainer(redo_every=EVERY, patience=255, pbt=pbt)
    ag = tr.agent
    for _ in range(159):
        tr.step()
    before = ag.redo_streak.clone().view(E_TR, -1)
    assert not tr.pbt_log and before.any()
    tr.step()  # step 160: the first round after learning started
    torch.cuda.synchronize()
    assert len(tr.pbt_log) == 1 and tr.pbt_log[0]["copied"]
    after = ag.redo_streak.view(E_TR, -1)
    copied = dict(tr.pbt_log[0]["copied"])
    for e in range(E_TR):
        s = copied.get(e, e)
        if s != e:
            assert not torch.equal(before[e], before[s])  # the replicas' dead units differ
        assert torch.equal(after[e], before[s]), (e, s)
