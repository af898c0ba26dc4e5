"""The learn kernels on exact-forward fixtures (tests/exact_fixture.py): one
learn per case on a wrapped ring (cap 160, fill 200, start 40), and 100 % of the
gradient entries compared with an f64 reference under a bound derived in
advance -- no share, nothing excluded.

Per case: (1) Q and the argmax on the batch's S and S' rows bit-equal to the
reference (tie agents included: first max); (2) every agent's loss within its
bound; (3) every gradient entry within its bound (exact_fixture.compare; the
shared kernel's gradient is ag.grad, the independent kernels' is adam_m / c1);
(4) Adam consistent with itself bit for bit; (5) target and its 16-bit shadow
bit-unchanged on this non-sync learn, the 16-bit online copy = rnd(params');
(6) shared only: gradient bits equal with collect_stats on and off, and the 1-,
5- and 12-slab gradients within the bound of each other and of the reference.

Worst |delta| / bound per kernel and block kind, measured on the MI355X
(worst over the cases of a kernel):
  kernel             loss   W1 tiles W1[88,:] b1     W2 tiles b2     W3     b3
  k_learn_f32        0.003  0.003    0.002    0.001  0.011    0.005  0.008  0.004
  k_learn_f16        0.001  0.237    0.232    0.195  0.662    0.235  0.237  0.234
  k_learn_bf16       0.003  0.232    0.232    0.232  0.232    0.232  0.232  0.215
  shared, 12 slabs   0.004  0.001    0.001    0.000  0.007    0.004  0.006  0.003
  shared, 5 slabs    0.004  0.001    0.000    0.001  0.005    0.003  0.005  0.003
  shared, 1 slab     0.004  0.002    0.001    0.001  0.017    0.004  0.016  0.002
The independent 16-bit kernels' 0.23: on the entries whose one rounding is
bit-determined the bound is the 2^-22 |g| of recovering g from adam_m / c1
alone, and that recovery's own rounding is up to a quarter of it -- the
kernel's 16-bit gradient is there the reference's, bit for bit.  k_learn_f16's
0.662: one dW2 entry with a rounding boundary inside its interval, rounded to
the neighbouring f16 value.
The fp16 fixtures hold 0.8 - 1.7 % f16-subnormal backward operands; ratios this
small leave no room for an MFMA that flushes them (one flushed dZ2 operand near
2^-14 would alone move a shared dW2 entry by a ratio of order 0.1).
"""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import oracle as O  # noqa: E402
import exact_fixture as X  # noqa: E402
from dmdqn_amd._lib import call, ptr, stream_of  # noqa: E402
from dmdqn_amd.agent import (AgentConfig, BatchedDQN, PRECISIONS, keras_adam_consts,  # noqa: E402
                             keras_to_kernel, kernel_to_keras)

DEV = "cuda"
_REF, _RUN = {}, {}


def _reference(name, loss):
    if (name, loss) not in _REF:
        _REF[name, loss] = X.reference(X.fixture(name), loss)
    return _REF[name, loss]


def _agent(fx, loss):
    cfg = AgentConfig(replay_buffer_size=fx.cap, nn_layers=[fx.H, fx.H], seed=fx.seed,
                      target_update_frequency=500, precision=fx.precision, loss=loss,
                      shared_params=fx.shared)
    ag = BatchedDQN(fx.E, fx.A, cfg, init_weights=fx.online)
    ag.target.copy_(torch.from_numpy(keras_to_kernel(fx.target, fx.H)))
    ag._refresh_target_h()
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
    # every value loaded with no loss
    np.testing.assert_array_equal(ag.keras_params("params"), fx.online)
    np.testing.assert_array_equal(ag.keras_params("target"), fx.target)
    if ag.target_h is not None:
        np.testing.assert_array_equal(ag.target_h[:, :ag.P].float().cpu().numpy(),
                                      ag.target.cpu().numpy())
    return ag


def _run(name, loss, collect_stats=False):
    """One learn of a fresh agent on the fixture; everything the checks read,
    as host arrays (cached: the shared cases compare runs with each other)."""
    key = (name, loss, collect_stats)
    if key in _RUN:
        return _RUN[key]
    fx = X.fixture(name)
    ag = _agent(fx, loss)
    pre = {k: getattr(ag, k).clone() for k in ("params", "target", "adam_m", "adam_v")}
    pre["target_h"] = None if ag.target_h is None else ag.target_h.clone()
    out = {"ag": ag, "pre": pre}
    out["loss"] = ag.learn(collect_stats=collect_stats).cpu().numpy().astype(np.float64)
    out["idx"] = ag.idx.cpu().numpy()
    for k in ("params", "adam_m", "adam_v"):
        out[k] = getattr(ag, k).cpu().numpy()
    if fx.shared:
        out["grad_dev"] = ag.grad.cpu().numpy()
        out["g"] = kernel_to_keras(out["grad_dev"][None], fx.H).astype(np.float64)
    else:
        c1 = np.float64(np.float32(keras_adam_consts(1, X.LR)[1]))
        out["g"] = kernel_to_keras(out["adam_m"], fx.H).astype(np.float64) / c1
    _RUN[key] = out
    return out


def _check_batch(fx, ag, idx, ref):
    """The draws are the predicted ones, the fixture conditions hold on them,
    and the ring rows they select are the fixture's transitions."""
    np.testing.assert_array_equal(idx, fx.idx)
    if not getattr(fx, "_checked_on_gpu_idx", False):
        X.check_conditions(fx, idx)
        fx._checked_on_gpu_idx = True
    for j in range(fx.NA):
        slots = ag.ring.slots_of(idx[j])
        a = ref.agents[j]
        np.testing.assert_array_equal(ag.ring.s[j].cpu().numpy()[slots, :89], a["S"])
        np.testing.assert_array_equal(ag.ring.n[j].cpu().numpy()[slots, :89], a["S2"])
        np.testing.assert_array_equal(ag.ring.a[j].cpu().numpy()[slots], a["A"])
        np.testing.assert_array_equal(ag.ring.d[j].cpu().numpy()[slots], a["D"])
        np.testing.assert_array_equal(O.zscore(ag.ring.r[j].cpu().numpy()[slots]), a["rn"])


def _check_forward(fx, ag, params0, ref):
    """Check 1: Q(S) and Q(S') of the pre-learn online net, and their argmax."""
    NA, prec = fx.NA, PRECISIONS[fx.precision]
    for rows, want in (("S", "q"), ("S2", "q_next_online")):
        x = np.stack([a[rows] for a in ref.agents], axis=1).astype(np.float32)  # [128, NA, 89]
        q_ref = np.stack([a[want] for a in ref.agents], axis=1).astype(np.float32)
        obs = torch.from_numpy(x).to(DEV)
        q = torch.empty((128, NA, 4), dtype=torch.float32, device=DEV)
        am = torch.empty((128, NA), dtype=torch.int32, device=DEV)
        if fx.shared:
            call("dmdqn_q_argmax_shared", ptr(params0), 128 * NA, ag.P, ag.H, prec, ptr(obs),
                 ptr(am), ptr(q), stream_of())
        else:
            for b in range(128):
                call("dmdqn_q_argmax", ptr(params0), NA, ag.P, ag.H, prec, ptr(obs[b]), ptr(am[b]),
                     ptr(q[b]), stream_of())
        q, am = q.cpu().numpy(), am.cpu().numpy()
        bad = np.argwhere(q != q_ref)
        assert bad.size == 0, (rows, bad[:4], q[tuple(bad[0])], q_ref[tuple(bad[0])])
        np.testing.assert_array_equal(am, q_ref.argmax(2), err_msg=rows)  # numpy: first max
    a_star = np.stack([a["a_star"] for a in ref.agents], axis=1)
    np.testing.assert_array_equal(am, a_star)


def _ulps32(x, y):
    return np.abs(x.astype(np.float64) - y) / np.spacing(np.abs(y).astype(np.float32)).astype(
        np.float64)


def _check_adam(out, lr=X.LR):
    """Check 4, in the device layout: w' == w - (m' alpha) / (sqrt(v') + eps) in
    f32 from the GPU's own m', v'; v' within 4 f32 ulps of c2 (m' / c1)^2."""
    f = np.float32
    alpha, c1, c2, eps = (f(x) for x in keras_adam_consts(1, lr))
    w0 = out["pre"]["params"].cpu().numpy()
    m, v, w = out["adam_m"], out["adam_v"], out["params"]
    assert not out["pre"]["adam_m"].any() and not out["pre"]["adam_v"].any()
    np.testing.assert_array_equal(w, w0 - (m * alpha) / (np.sqrt(v) + eps))
    g = m.astype(np.float64) / np.float64(c1)
    v_exp = np.float64(c2) * g * g
    nz = v_exp > 0
    assert (v[~nz] == 0).all()
    assert _ulps32(v[nz], v_exp[nz]).max() <= 4
    assert np.count_nonzero(m) > 0.5 * m.size  # a real step, not zeros against zeros


def _check_unchanged(fx, out):
    """Check 5: a non-sync learn leaves target and its shadow alone; the 16-bit
    online copy (the shared net keeps one) is the rounding of the new weights."""
    ag, pre = out["ag"], out["pre"]
    assert torch.equal(ag.target, pre["target"])
    if ag.target_h is not None:
        assert torch.equal(ag.target_h, pre["target_h"])
    if ag.params_h is not None:
        assert torch.equal(ag.params_h[:, :ag.P], ag.params.to(ag.params_h.dtype))
    assert not torch.equal(ag.params, pre["params"])


def _check_learn(name, loss, collect_stats=False, tag=None):
    fx = X.fixture(name)
    ref = _reference(name, loss)
    out = _run(name, loss, collect_stats)
    ag = out["ag"]
    _check_batch(fx, ag, out["idx"], ref)
    _check_forward(fx, ag, out["pre"]["params"], ref)
    lr = X.ratio(out["loss"] - ref.loss, ref.loss_bound)
    print(f"{tag or name} {loss}: loss worst ratio {lr.max():.3f}")
    assert lr.max() <= 1, (lr, out["loss"], ref.loss)
    total = {}
    for w in range(fx.NW):
        cmp = X.compare(out["g"][w], ref, w)
        for k, v in X.summary(cmp).items():
            total[k] = max(total.get(k, 0.0), v)
        r, block, where = X.worst(cmp)
        assert r <= 1, (w, block, where, r, out["g"][w][where], ref.g[w][where],
                        ref.bound[w][where])
    print(f"{tag or name} {loss}: gradient worst ratio per block",
          {k: round(v, 3) for k, v in total.items()})
    _check_adam(out)
    _check_unchanged(fx, out)
    return out, ref


@pytest.mark.parametrize("loss", ["mse", "huber"])
@pytest.mark.parametrize("name", ["f32_128", "f32_64"])
def test_learn_f32_exact(name, loss):
    """k_learn_f32, H = 128 and 64, E = 2, A = 3."""
    _check_learn(name, loss)


@pytest.mark.parametrize("loss", ["mse", "huber"])
@pytest.mark.parametrize("name", ["f16", "bf16"])
def test_learn_h16_exact(name, loss):
    """k_learn_f16 / k_learn_bf16, E = 2, A = 3."""
    _check_learn(name, loss)


SHARED = {"mse": "shared_a", "huber": "shared_b"}  # tied columns (1, 2) / (0, 3)


@pytest.mark.parametrize("collect_stats", [False, True])
@pytest.mark.parametrize("loss", ["mse", "huber"])
def test_learn_shared_exact(loss, collect_stats):
    """k_shared_next + k_shared_grad4 through BatchedDQN.learn (12 agents, 12
    slabs), E = 3, A = 4; the gradient bits do not depend on collect_stats."""
    out, _ = _check_learn(SHARED[loss], loss, collect_stats, tag="shared")
    other = _run(SHARED[loss], loss, not collect_stats)
    np.testing.assert_array_equal(out["grad_dev"], other["grad_dev"])
    np.testing.assert_array_equal(out["loss"], other["loss"])
    if collect_stats:
        qs = out["ag"].qstats.cpu().numpy()
        np.testing.assert_array_equal(qs[:, 2:6].sum(1), 128)


@pytest.mark.parametrize("loss", ["mse", "huber"])
def test_learn_shared_exact_across_slab_counts(loss):
    """The shared gradient through the C ABI with 1 slab and with 5 (12 agents
    walked 3, 3, 2, 2, 2): each within the bound of the reference, and the 1-,
    5- and 12-slab gradients within the bound of each other."""
    name = SHARED[loss]
    fx, ref = X.fixture(name), _reference(name, loss)
    out = _run(name, loss, False)
    ag = out["ag"]
    ag.params.copy_(out["pre"]["params"])  # the learn stepped Adam: back to the fixture's net
    ag._refresh_params_h()
    gs = {12: out["g"][0]}
    for n in (1, 5):
        slab = torch.empty((n, ag.P), dtype=torch.float32, device=DEV)
        g = torch.empty(ag.P, dtype=torch.float32, device=DEV)
        a = ag.c_learn_args()
        call("dmdqn_learn_shared_grad", C.byref(a), ptr(slab), n, ptr(g), C.c_float(1.0 / ag.NA),
             ptr(ag.shared_work), stream_of())
        gs[n] = kernel_to_keras(g.cpu().numpy()[None], fx.H)[0].astype(np.float64)
        lr = X.ratio(ag.loss.cpu().numpy().astype(np.float64) - ref.loss, ref.loss_bound)
        assert lr.max() <= 1, (n, lr)
        cmp = X.compare(gs[n], ref, 0)
        print(f"shared {loss} {n} slab(s): gradient worst ratio per block",
              {k: round(v, 3) for k, v in X.summary(cmp).items()})
        r, block, where = X.worst(cmp)
        assert r <= 1, (n, block, where, r)
    for a_, b_ in ((1, 5), (1, 12), (5, 12)):
        r = X.ratio(gs[a_] - gs[b_], ref.bound[0])
        assert r.max() <= 1, (a_, b_, r.max(), int(r.argmax()))
    ag.params.copy_(torch.from_numpy(out["params"]))  # as the cached run left it
    ag._refresh_params_h()
