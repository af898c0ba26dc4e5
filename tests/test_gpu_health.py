"""The network health probe on the GPU: dmdqn_net_probe bit for bit on the
exact-forward fixtures (dead units, an overflowing and a NaN output column,
a wrapped ring), dmdqn_layer_norms against numpy's f64 sums, consistency with
gradient clipping's norm and with the Adam step actually taken, and a Trainer
whose state does not change by a bit under health_every."""
import ctypes as C
import json

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import exact_fixture as XF  # noqa: E402
import health_ref as HR  # noqa: E402
from dmdqn_amd import kernels as K  # noqa: E402
from dmdqn_amd._lib import CProbe, call, ptr, stream_of  # noqa: E402
from dmdqn_amd.agent import (AgentConfig, BatchedDQN, PRECISIONS, keras_to_kernel,  # noqa: E402
                             n_params)
from dmdqn_amd.env import EnvConfig  # noqa: E402
from dmdqn_amd.ops import load as ops_load  # noqa: E402
from dmdqn_amd.trainer import Trainer  # noqa: E402

DEV = "cuda"


# --------------------------------------------------------------------------- 1. the probe
def _mutated_nets(fx):
    """The fixture's online nets (Keras order) with three agents mutated."""
    sl = XF.block_slices(fx.H)
    nets = fx.online.astype(np.float32).copy()

    def var(j, name):
        o, sh = sl[name]
        return nets[j, o:o + int(np.prod(sh))].reshape(sh)
    # agent 0: layer-1 units dead under `>` only (z == 0) and dead either way
    # (z == -1); layer-2 units with z == 0
    for u in (0, 17, 127):
        var(0, "W1")[:, u] = 0.0
        var(0, "b1")[u] = 0.0
    for u in (5, 64):
        var(0, "W1")[:, u] = 0.0
        var(0, "b1")[u] = -1.0
    for u in (3, 31, 96):
        var(0, "W2")[:, u] = 0.0
        var(0, "b2")[u] = 0.0
    if fx.precision == "fp16":
        var(1, "W3")[:, 0] = 65504.0     # agent 1: Q[:, 0] overflows f16 on every row
    var(2, "b3")[2] = np.nan             # agent 2: Q[:, 2] is NaN on every row
    return nets


def _agent(fx, nets):
    """test_gpu_learn_exact._agent's ring load: cap 160, fill 200, start 40."""
    cfg = AgentConfig(replay_buffer_size=fx.cap, nn_layers=[fx.H, fx.H], seed=fx.seed,
                      target_update_frequency=500, precision=fx.precision)
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
    return ag


@pytest.mark.parametrize("name", ["f16", "bf16"])
def test_probe_bit_for_bit_on_exact_fixtures(name):
    fx = XF.fixture(name)
    assert fx.NA == 6 and fx.cap == 160 and fx.fill == 200
    nets = _mutated_nets(fx)
    ag = _agent(fx, nets)
    idx = torch.from_numpy(fx.idx).to(DEV)
    # the restatement, on the rows a probe that honours `start` reads
    want_c, want_s, want_m = [], [], []
    for j in range(fx.NA):
        S = fx.batch(j)[0]
        # a probe that ignores start reads other rows
        assert not np.array_equal(S, fx.batch(j, use_start=False)[0])
        c, s, m = HR.probe_ref(XF.split(nets[j].astype(np.float64), fx.H), S, fx.precision)
        want_c.append(c)
        want_s.append(s)
        want_m.append(m)
    want_c, want_s, want_m = np.stack(want_c), np.stack(want_s), np.stack(want_m)
    # what the mutations were built to give
    assert want_c[0, 1] == 5 and want_c[0, 3] == 3
    assert want_m[0, 0].tolist() == [(1 << 0) | (1 << 5) | (1 << 17), 0, 1 << 0, 1 << 31]
    assert want_m[0, 1].tolist() == [(1 << 3) | (1 << 31), 0, 0, 1 << 0]
    clean = [3, 4, 5] + ([1] if fx.precision != "fp16" else [])
    assert (want_c[clean, 4] == 0).all() and want_c[0, 4] == 0
    assert (want_c[1:, 1] == 0).all() and (want_c[1:, 3] == 0).all() and not want_m[1:].any()
    assert want_c[2, 4] == 128
    if fx.precision == "fp16":
        # every row's exact sum is far above the f16 overflow threshold 65,520,
        # all terms >= 0: no summation order can bring a partial sum back under it
        W3 = XF.split(nets[1].astype(np.float64), fx.H)[4]
        z2 = HR.forward(XF.split(nets[1].astype(np.float64), fx.H), fx.batch(1)[0], "fp16")[1]
        acc = np.maximum(z2, 0) @ W3[:, 0]
        print(f"agent 1: smallest exact sum of the overflowing column {acc.min():.0f}")
        assert acc.min() >= 872405 > 10 * 65520
        assert want_c[1, 4] == 128

    # the ctypes call
    c1 = torch.full((fx.NA, 5), -1, dtype=torch.int32, device=DEV)
    s1 = torch.full((fx.NA, 5), -1.0, dtype=torch.float64, device=DEV)
    m1 = torch.full((fx.NA, 2, 4), -1, dtype=torch.int32, device=DEV)
    args = CProbe(fx.NA, ag.ring.slots, ag.ring.start, 128, fx.H, PRECISIONS[fx.precision], ag.P,
                  *[t.data_ptr() for t in (ag.ring.s, idx, ag.params, c1, s1, m1)])
    call("dmdqn_net_probe", C.byref(args), stream_of())
    # the torch op (through BatchedDQN.probe_health, before any learn)
    h = ag.probe_health(idx)
    torch.cuda.synchronize()
    got_c, got_s = c1.cpu().numpy(), s1.cpu().numpy()
    got_m = m1.cpu().numpy().view(np.uint32)
    print(name, "counts", got_c.tolist())
    np.testing.assert_array_equal(got_c, want_c)
    np.testing.assert_array_equal(got_s.view(np.int64), want_s.view(np.int64))
    np.testing.assert_array_equal(got_m, want_m)
    assert torch.equal(h["counts"], c1) and torch.equal(h["dead_mask"], m1)
    assert torch.equal(h["stats"].view(torch.int64), s1.view(torch.int64))
    assert int(h["learn_step"]) == 0 and not h["alpha"].any() and h["g2"] is None
    # dead_mask = NULL is allowed
    c2 = torch.zeros_like(c1)
    s2 = torch.zeros_like(s1)
    ops_load().net_probe(ag.ring.s, idx, ag.params, ag.ring.start, fx.H, PRECISIONS[fx.precision],
                         c2, s2, None)
    assert torch.equal(c2, c1) and torch.equal(s2.view(torch.int64), s1.view(torch.int64))


# --------------------------------------------------------------------------- 2. layer_norms
def _loguniform(rs, shape):
    return np.exp2(rs.uniform(-20.0, 4.0, size=shape)).astype(np.float32)


def _synthetic_nets(rs, Hd, n):
    """n nets in Keras order: zeros; a lone 3.0 at the first and a lone -0.75 at
    the last element of every variable; log-uniform 2^-20 .. 2^4 with signs; all
    +-2^60; one inf."""
    Pk = XF.n_params(Hd)
    sl = XF.block_slices(Hd)
    nets = np.zeros((5, Pk), np.float32)
    for name in HR.VARIABLES:
        o, sh = sl[name]
        nets[1, o] = 3.0
        nets[1, o + int(np.prod(sh)) - 1] = -0.75
    nets[2] = _loguniform(rs, Pk) * rs.choice([-1.0, 1.0], size=Pk)
    nets[3] = np.float32(2.0 ** 60) * rs.choice([-1.0, 1.0], size=Pk)
    nets[4] = nets[2]
    nets[4, sl["W2"][0] + 777] = np.inf
    return nets[:n]


def _check_sums(got, want):
    """Each sum within relative 2^-38 of numpy's f64 sum (P * 2^-53 rounded up:
    at most P - 1 f64 additions of non-negative exact squares, each within
    2^-53 relative of its exact value); zero and infinite sums exact."""
    assert got.shape == want.shape
    special = (want == 0) | ~np.isfinite(want)
    np.testing.assert_array_equal(got[special], want[special])
    rel = np.abs(got[~special] - want[~special]) / want[~special]
    print(f"layer_norms: worst relative error {rel.max():.3e} (bound {2.0 ** -38:.3e})")
    assert rel.max() <= 2.0 ** -38


@pytest.mark.parametrize("Hd,n", [(128, 5), (64, 3)])
def test_layer_norms_against_f64_numpy(Hd, n):
    rs = np.random.RandomState(5 + Hd)
    x = keras_to_kernel(_synthetic_nets(rs, Hd, n), Hd)
    assert x.shape == (n, n_params(Hd))
    xd = torch.from_numpy(x).to(DEV)
    got = K.layer_norms(xd, Hd).cpu().numpy()
    want = HR.layer_sums_ref(x, Hd)
    assert (want[0] == 0).all()
    np.testing.assert_array_equal(want[1], np.full(6, 9.5625))
    if n == 5:
        # squares that overflow f32 but not f64, and the one infinite sum
        assert np.isfinite(want[3]).all() and (want[3] > 3.5e38).any()
        assert np.isinf(want[4]).tolist() == [False, False, True, False, False, False]
    _check_sums(got, want)
    # mode 1: m log-uniform with signs and zeros, v log-uniform, zero where m is
    P = n_params(Hd)
    m = _loguniform(rs, (n, P)) * rs.choice([-1.0, 0.0, 1.0], size=(n, P)).astype(np.float32)
    v = np.where(m == 0, np.float32(0), _loguniform(rs, (n, P))).astype(np.float32)
    m[0], v[0] = 0.0, 0.0
    eps = np.float32(1e-7)
    got = K.layer_norms(torch.from_numpy(m).to(DEV), Hd, y=torch.from_numpy(v).to(DEV),
                        eps=float(eps)).cpu().numpy()
    want = HR.layer_sums_ref(m, Hd, y=v, eps=eps)
    assert (want[0] == 0).all() and (want[1:] > 0).all()
    _check_sums(got, want)
    if Hd == 128:  # NW = 1: the shared net's shape; the ctypes entry gives the op's bits
        one = K.layer_norms(xd[2:3].contiguous(), Hd)
        out = torch.zeros((1, 6), dtype=torch.float64, device=DEV)
        row = xd[2:3].contiguous()
        call("dmdqn_layer_norms", ptr(row), None, C.c_float(0.0), 0, 1, P, Hd, ptr(out), stream_of())
        torch.cuda.synchronize()
        assert torch.equal(one, out)
        np.testing.assert_array_equal(one.cpu().numpy()[0], K.layer_norms(xd, Hd).cpu().numpy()[2])


# --------------------------------------------------------------------------- 3. clipping
def test_probe_is_consistent_with_clipping_and_the_adam_step():
    """One learn under global_clipnorm, then probe_health(): the six g2 sum to
    the clipping kernel's norm, and alpha * sqrt(u2) is the norm of the step
    the parameters took, per variable."""
    E, A, Hd = 2, 2, 128
    cfg = AgentConfig(precision="fp16", replay_buffer_size=200, seed=3, global_clipnorm=10.0)
    ag = BatchedDQN(E, A, cfg)
    rs = np.random.RandomState(3)
    for _ in range(130):
        s = torch.from_numpy(rs.randint(-1, 7, size=(E, A, 89)).astype(np.float32)).to(DEV)
        n = torch.from_numpy(rs.randint(-1, 7, size=(E, A, 89)).astype(np.float32)).to(DEV)
        a = torch.from_numpy(rs.randint(0, 4, size=(E, A)).astype(np.int32)).to(DEV)
        r = torch.from_numpy(-rs.randint(0, 40, size=(E, A)).astype(np.float64)).to(DEV)
        ag.remember(s, a, r, n, bool(rs.rand() < 0.2))
    before = ag.params.double().cpu().numpy()
    assert ag.learn() is not None
    h = ag.probe_health()
    torch.cuda.synchronize()
    assert int(h["learn_step"]) == 1 and h["g2"] is not None
    g2 = h["g2"].cpu().numpy()
    norm = np.sqrt(g2.sum(axis=1)).astype(np.float32)
    gn = ag.grad_norm.cpu().numpy()
    assert (gn > 0).all()
    # the order of summation differs (per variable, then six): one f32 ulp
    assert (np.abs(norm.astype(np.float64) - gn) <= np.spacing(gn)).all(), (norm, gn)
    _check_sums(g2, HR.layer_sums_ref(ag._split_grad.cpu().numpy(), Hd))
    after = ag.params.double().cpu().numpy()
    # per variable, the sum of squares of the f64 difference before - after
    # (kernel_to_keras works on f32: the index map of the layout instead)
    from dmdqn_amd.agent import kernel_to_keras
    perm = kernel_to_keras(np.arange(ag.P, dtype=np.float32)[None], Hd)[0].astype(np.int64)
    sl = XF.block_slices(Hd)
    exact2 = np.zeros((E * A, 6))
    for j in range(E * A):
        dk = (before[j] - after[j])[perm]
        for i, name in enumerate(HR.VARIABLES):
            o, sh = sl[name]
            exact2[j, i] = (dk[o:o + int(np.prod(sh))] ** 2).sum()
    alpha = h["alpha"].double().cpu().numpy()[:, None]
    assert (alpha > 0).all() and (alpha == np.float32(ag._last_tok.adam[0])).all()
    pred = alpha * np.sqrt(h["u2"].cpu().numpy())
    took = np.sqrt(exact2)
    assert (took > 0).all()
    rel = np.abs(pred - took) / took
    print("update norm: worst relative error per variable", rel.max(axis=0))
    # 1e-5: the f32 rounding of each parameter's subtraction w - step
    assert rel.max() <= 1e-5
    # w2: the weights the learn left
    _check_sums(h["w2"].cpu().numpy(), HR.layer_sums_ref(ag.params.cpu().numpy(), Hd))


# --------------------------------------------------------------------------- 4. the Trainer
def _run_trainer(spare, health_every, steps=420):
    tr = Trainer(EnvConfig(rows=2, cols=2, num_envs=8, seed=6),
                 AgentConfig(precision="bf16", replay_buffer_size=300, seed=6, ring_spare=spare,
                             health_every=health_every), overlap="env")
    ag = tr.agent
    losses, checked, held = [], 0, []
    for _ in range(steps):
        st = tr.step()
        if st.loss_launched:
            held.append(tr._last_loss)
        if tr._pending is None and held:  # every learn begun so far is launched
            losses.extend(t.clone() for t in held)
            held = []
        n = ag.learn_step_counter
        if health_every and st.loss_launched and n % health_every == 0 and n in (7, 140, 287):
            # the probe against a direct call on the same tensors, bit for bit
            tr.synchronize()
            h = ag.health
            assert int(h["learn_step"]) == n and h["idx"] is ag._last_tok.idx
            assert h["start"] == ag._last_tok.start
            c, s, m = K.net_probe(ag.ring.s, h["idx"], ag.params, h["start"], ag.H,
                                  PRECISIONS["bf16"])
            w2 = K.layer_norms(ag.params, ag.H)
            u2 = K.layer_norms(ag.adam_m, ag.H, y=ag.adam_v, eps=ag._last_tok.adam[3])
            torch.cuda.synchronize()
            assert torch.equal(h["counts"], c) and torch.equal(h["dead_mask"], m)
            assert torch.equal(h["stats"].view(torch.int64), s.view(torch.int64))
            assert torch.equal(h["w2"].view(torch.int64), w2.view(torch.int64))
            assert torch.equal(h["u2"].view(torch.int64), u2.view(torch.int64))
            assert h["g2"] is None and bool((h["counts"][:, 0] > 0).all())
            checked += 1
    tr.synchronize()
    losses.extend(t.clone() for t in held)
    if health_every:
        assert checked == 3 and int(ag.health["learn_step"]) == 287
        rec = ag.learn_metrics()["health"]
        assert rec["learn_step"] == 287 and len(rec["layers"]) == 2
        assert set(rec["update_ratio"]) == set(HR.VARIABLES) and "grad_layer_norm" not in rec
    else:
        assert ag.health is None and "health" not in ag.learn_metrics()
    assert ag.ring.total > ag.ring.slots  # the rings wrapped
    out = {"losses": torch.stack(losses).cpu(), "pairs": ag.pair_launches}
    for k in ("params", "adam_m", "adam_v", "target", "np_state", "py_state"):
        out[k] = getattr(ag, k).cpu()
    for k in ("s", "n", "a", "r", "d"):
        out["ring_" + k] = getattr(ag.ring, k).cpu()
    out["obs"] = tr.obs.cpu()
    del tr
    torch.cuda.empty_cache()
    return out


@pytest.mark.parametrize("spare", [2, 16])
def test_trainer_state_is_bit_identical_with_the_probe(spare):
    off, on = _run_trainer(spare, 0), _run_trainer(spare, 7)
    assert off["pairs"] > 100 and on["pairs"] > 80  # paired learns in both runs
    assert off["losses"].shape == on["losses"].shape == (293, 32)
    for k in off:
        if k == "pairs":
            continue
        a, b = off[k], on[k]
        assert a.dtype == b.dtype and a.shape == b.shape
        assert torch.equal(a.view(torch.uint8) if a.dtype != torch.uint8 else a,
                           b.view(torch.uint8) if b.dtype != torch.uint8 else b), k


def _train_cli(monkeypatch, capsys, tmp_path, extra):
    """train.py --batched --grid 2x2 --envs 8 --health_every 5 (one episode of
    240 steps, 113 learns), in this process: (the JSONL records, the last line)."""
    from src.scripts import train
    path = str(tmp_path / "m.jsonl")
    monkeypatch.setattr("sys.argv", ["train.py", "--batched", "--grid", "2x2", "--envs", "8",
                                     "--episodes", "1", "--health_every", "5", "--metrics",
                                     path] + extra)
    train.main()
    final = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    with open(path) as f:
        return [json.loads(line) for line in f], final


def test_train_cli_writes_the_health_block(monkeypatch, capsys, tmp_path):
    recs, _ = _train_cli(monkeypatch, capsys, tmp_path, [])
    with_h = [r for r in recs if "health" in r]
    assert with_h and all("loss" in r for r in with_h)
    assert not any("health" in r for r in recs if "loss" not in r)
    h = with_h[-1]["health"]
    assert h["learn_step"] % 5 == 0 and h["learn_step"] > 0
    for layer in h["layers"]:
        assert 0.0 <= layer["dead_frac"] <= layer["dead_frac_max"] <= 1.0
        assert 0.0 < layer["active_frac"] < 1.0 and layer["act_mean"] > 0
        assert layer["preact_absmax"] > 0
    assert h["q_absmax"] > 0 and h["nonfinite_agents"] == 0
    assert set(h["weight_norm"]) == set(h["update_ratio"]) == set(HR.VARIABLES)
    assert 0 < h["update_ratio"]["W2"]["mean"] <= h["update_ratio"]["W2"]["max"] < 1


def test_train_cli_writes_the_health_block_per_variant(monkeypatch, capsys, tmp_path):
    recs, final = _train_cli(monkeypatch, capsys, tmp_path,
                             ["--sweep", "learning_rate=1e-4,1e-2"])
    with_h = [r for r in recs if "health" in r]
    assert with_h
    vs = with_h[-1]["variants"]
    assert len(vs) == 2 and all("health" in v for v in vs)
    lo, hi = (v["health"]["update_ratio"]["W2"]["mean"] for v in vs)
    assert 0 < lo < hi  # the step grows with the learning rate
    assert len(final["variants"]) == 2
    for row in final["variants"]:
        assert len(row["dead_frac"]) == 2 and set(row["update_ratio"]) == set(HR.VARIABLES)
