"""The exact-forward fixtures (tests/exact_fixture.py) checked on the CPU: the
builder's conditions, the f64 reference against the pinned checkers
(oracle.learn, oracle.learn_mixed), the tightness of the derived bounds and the
power of the comparator -- it must reject seeded corruptions of a correct
gradient, in the block they hit, and the gradients of mutated (wrong) learns.

Tightness, measured (largest bound / largest |g| over the blocks of a fixture,
MSE / Huber): fp32 H = 128 5.3e-4 / 5.5e-4, H = 64 4.7e-4 / 4.7e-4; fp16 2.0e-3
/ 1.3e-3; shared fp16 6.7e-4 / 4.4e-4; bf16 9.8e-3 / 9.2e-3.  One bf16 ulp is
up to 2^-7 = 7.8e-3 of the value it rounds, so the bf16 margin is thin: of the
22 seeds in 11..59 that meet the fixture conditions, 13 and 32 also keep every
block within 1e-2 (the others reach 1.04e-2 .. 1.36e-2 on a W1 tile), and the
bf16 fixture uses 13.
"""
import numpy as np
import pytest

import oracle as O
import exact_fixture as X

ALL = list(X.FIXTURES)
LOSSES = ("mse", "huber")


@pytest.mark.parametrize("name", ALL)
def test_builder_conditions_hold(name):
    """Every fixture the GPU tests use builds (exactness proven in integer fixed
    point: the worst layer stays below 2^20 quanta) and meets the fixture
    conditions on the predicted replay draws."""
    fx = X.fixture(name)
    st = fx.stats
    assert max(st["quanta"]) < 2 ** 20
    assert min(st["active1"] + st["active2"]) >= 0.3 and max(st["active1"] + st["active2"]) <= 0.7
    assert min(st["both_ways"]) >= 0.9 and min(st["zero_preact"]) >= 1
    assert fx.idx.shape == (fx.NA, 128) and fx.idx.min() >= 0 and fx.idx.max() < fx.cap
    assert not np.array_equal(fx.online, fx.target)
    for w in (fx.online, fx.target):
        assert np.array_equal(O.round_bf16(w), w)
    if fx.precision == "fp16":
        assert st["subnormal"] <= 0.02
        assert abs(st["subnormal"] - X.SUBNORMAL_SHARE[name]) < 5e-4, st["subnormal"]
    print(name, {k: (min(v), max(v)) if isinstance(v, list) and len(v) > 3 else v
                 for k, v in st.items()})


def test_builder_raises_rather_than_weakening():
    with pytest.raises(ValueError):  # sixteenths of thirds are no dyadic rationals
        X._exact_dense(np.ones((2, 3)), np.full((3, 2), 1 / 3.0), np.zeros(2), X._rnd16("fp32"), "x")
    with pytest.raises(ValueError, match="2\\^20"):
        X._exact_dense(np.full((1, 4), 2.0 ** 19), np.ones((4, 1)), np.zeros(1), X._rnd16("fp32"),
                       "x")
    with pytest.raises(ValueError, match="tie decides"):  # a seed that misses a condition
        X.build(**dict(X.FIXTURES["f32_64"], seed=12))


def _oracle_learn(fx, j, kind):
    S, A, r, S2, D = fx.batch(j)
    w = fx.net_of(j)
    p, t = fx.online[w].copy(), fx.target[w].copy()
    m, v = np.zeros_like(p), np.zeros_like(p)
    args = (p, t, m, v, S.astype(np.float32), A.astype(np.int32), O.zscore(r),
            S2.astype(np.float32), D, 1)
    if fx.precision == "fp32":
        return O.learn(*args, H1=fx.H, H2=fx.H, want_grad=True, loss_kind=kind)
    return O.learn_mixed(*args, precision=fx.precision, H=fx.H, loss_kind=kind,
                         round_grad=not fx.shared, want_grad=True)


@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("name", ALL)
def test_reference_agrees_with_pinned_checkers(name, loss):
    """oracle.learn (fp32) / oracle.learn_mixed (fp16, bf16; round_grad=False and
    the mean over agents for the shared net) on the fixture: loss and every
    gradient entry within the derived bound of the f64 reference."""
    fx = X.fixture(name)
    ref = X.reference(fx, loss, from_adam=False)
    out = [_oracle_learn(fx, j, X.LOSS_KINDS[loss]) for j in range(fx.NA)]
    lr = X.ratio(np.array([o[0] for o in out], np.float64) - ref.loss, ref.loss_bound)
    assert lr.max() <= 1, lr
    g = np.stack([o[1] for o in out]).astype(np.float64)
    if fx.shared:
        g = g.mean(0)[None]
    for w in range(fx.NW):
        r, block, where = X.worst(X.compare(g[w], ref, w))
        assert r <= 1, (w, block, where, r)


@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("name", ALL)
def test_bounds_are_tight(name, loss):
    """For every block the largest bound is at most 1e-2 of the block's largest
    |g| (as the GPU tests compare it: from adam_m / c1 for the independent
    kernels)."""
    fx = X.fixture(name)
    ref = X.reference(fx, loss)
    worst = {}
    for w in range(fx.NW):
        for block, ix in X.blocks(fx.H).items():
            t = ref.bound[w][ix].max() / np.abs(ref.g[w][ix]).max()
            kind = block if block in ("W1[88,:]", "b1", "b2", "W3", "b3") else block[:2] + " tiles"
            worst[kind] = max(worst.get(kind, 0.0), float(t))
    print(name, loss, {k: f"{v:.2e}" for k, v in worst.items()})
    assert max(worst.values()) <= 1e-2, worst


# ---------------------------------------------------------------- power: corruptions
def _tile(H, o, kt, nt, rows=16):
    return o + (np.arange(16 * kt, 16 * kt + rows)[:, None] * H
                + np.arange(16 * nt, 16 * nt + 16)[None]).ravel()


def _corruptions(fx, g, rng):
    """name -> (corrupted copy of g, the blocks it must be rejected in)."""
    H = fx.H
    sl = X.block_slices(H)
    o1, o2, o3 = sl["W1"][0], sl["W2"][0], sl["b3"][0]
    NT = H // 16
    out = {}
    kt, nt = rng.randint(NT), rng.randint(NT - 1)
    a, b = _tile(H, o2, kt, nt), _tile(H, o2, kt, nt + 1)
    c = g.copy()
    c[a], c[b] = g[b], g[a]
    out["two neighbouring dW2 tiles swapped"] = (c, [
        f"W2[{16 * kt}:{16 * kt + 16},{16 * n}:{16 * n + 16}]" for n in (nt, nt + 1)])
    kt, nt = rng.randint(5), rng.randint(NT)
    c = g.copy()
    c[_tile(H, o1, kt, nt)] *= 1 + 2.0 ** -7
    out["one dW1 tile scaled by 1 + 2^-7"] = (c, [f"W1[{16 * kt}:{16 * kt + 16},"
                                                   f"{16 * nt}:{16 * nt + 16}]"])
    c = g.copy()
    c[o1 + 88 * H:o1 + 89 * H] = 0
    out["the feature-88 column zeroed"] = (c, ["W1[88,:]"])
    c = g.copy()
    c[o3:o3 + 4] = np.roll(g[o3:o3 + 4], 1)
    out["db3 rotated by one"] = (c, ["b3"])
    kt, n = rng.randint(NT), rng.randint(H)
    rows = np.arange(16 * kt, 16 * kt + 16) * H
    c = g.copy()
    c[o2 + rows + n], c[o2 + rows + (n ^ 16)] = g[o2 + rows + (n ^ 16)], g[o2 + rows + n]
    out["one partner column (n ^ 16) exchanged"] = (c, [
        f"W2[{16 * kt}:{16 * kt + 16},{16 * (m // 16)}:{16 * (m // 16) + 16}]"
        for m in (n, n ^ 16)])
    return out


CORRUPTIONS = ("two neighbouring dW2 tiles swapped", "one dW1 tile scaled by 1 + 2^-7",
               "the feature-88 column zeroed", "db3 rotated by one",
               "one partner column (n ^ 16) exchanged")
CORRUPTION_CASES = [(n, c) for n in ALL for c in CORRUPTIONS]


@pytest.mark.parametrize("name,what", CORRUPTION_CASES)
def test_comparator_rejects_corrupted_gradients(name, what):
    """A seeded corruption of a correct gradient (the reference's own) is
    rejected in exactly the blocks it touches; the uncorrupted gradient passes
    with ratio 0."""
    fx = X.fixture(name)
    ref = X.reference(fx, "mse")
    rng = np.random.RandomState(5)
    for w in range(min(fx.NW, 2)):
        assert X.worst(X.compare(ref.g[w], ref, w))[0] == 0
        c, expect = _corruptions(fx, ref.g[w], rng)[what]
        cmp = X.compare(c, ref, w)
        bad = sorted(k for k, (r, _) in cmp.items() if r > 1)
        assert bad == sorted(expect), (what, bad, expect)


# ---------------------------------------------------------------- power: mutated learns
@pytest.mark.parametrize("mutation", X.MUTATIONS)
@pytest.mark.parametrize("name", ALL)
def test_comparator_rejects_mutated_learns(name, mutation):
    """The gradient of a wrong learn -- online Q for the target's, last max on
    ties, done ignored, ReLU mask >=, backprop through the post-Adam W3, MSE dq
    under Huber, batch rows without the ring's start -- is rejected for every
    net (last max: for the nets with tied columns)."""
    fx = X.fixture(name)
    loss = "huber" if mutation == "mse_dq_under_huber" else "mse"
    ref = X.reference(fx, loss)
    mut = X.reference(fx, loss, mutate=(mutation,))
    nets = range(len(fx.ties)) if mutation == "last_max" else range(fx.NW)
    for w in nets:
        r, block, _ = X.worst(X.compare(mut.g[w], ref, w))
        assert r > 1, (w, block, r)
    if mutation == "last_max" and not fx.shared:  # and nothing else moved
        for w in range(len(fx.ties), fx.NW):
            assert X.worst(X.compare(mut.g[w], ref, w))[0] == 0
