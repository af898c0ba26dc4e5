"""Exact-forward fixtures for the learn kernels: batches and weights on which
the Q-network forward is exact in every summation order, an f64 reference of
one learn under the rounding-point model of oracle.learn_mixed, a derived error
bound beside every gradient entry, and a comparator that covers every entry.

Construction (build): observations are integers in [-1, 7); every weight is 0
(half of them) or +-1, +-2 over a power-of-two denominator (DENOMS), every bias
a small multiple of its layer's grid (1/16 for weights in sixteenths), drawn in
+-8 steps and then shifted so that each hidden unit is centred on the mean of
its inputs (a unit that is on or off for a whole batch tests nothing) -- dyadic
rationals of at most 8 significant bits, which f32, f16 and bf16 all hold
exactly (asserted).  For every ring row (S and S'),
both nets and each layer, the builder scales the layer's inputs and weights to
integers by their quanta and asserts sum|terms| + |bias| < 2^20 quanta: that
leaves 4 bits under f32's 24, so every partial sum of the layer is exact in any
order (given an MFMA that keeps 24 bits below its largest term).  The inputs of
a layer are the activations as the precision rounds them (z = rnd(rnd(x @ W) +
b), oracle._mixed_fwd), so their quantum is recomputed per precision; rounding
an exact sum is deterministic.  No ReLU flip and no argmax flip is then
possible, dQ and dZ2 (one exact product per entry: W3 holds powers of two) are
bit-determined, and what is left of a correct kernel's gradient error is the
f32 accumulation of the backward sums plus the model's 16-bit roundings.

Bounds (derived, not measured).  u = 2^-22 per addition (2^-23 for a GPU
addition that may truncate, 2^-24 for an RNE reference, rounded up); ulp16(v) is
one unit in the last place of v in the kernel's 16-bit type, floored at the f16
subnormal spacing 2^-24:
  dW3, db3, dW2, db2:  128 u sum|terms|
                       + ulp16(g_ref)        independent 16-bit kernels (one
                                             rounding of dW) -- only where a
                                             16-bit rounding boundary lies
                                             within the rest of the bound of
                                             the exact sum; elsewhere the
                                             rounded entry is bit-determined: 0
                       + NA u sum|terms|     shared kernel (sums over agents
                                             and slabs, no rounding of dW)
  dZ1 (active):        ulp16(dH1) + 128 u sum_k |dZ2 W2|   (fp32: no ulp16)
                       16-bit: only where a 16-bit rounding boundary lies within
                       128 u sum_k |dZ2 W2| of the exact dH1; elsewhere every f32
                       sum that close rounds to the reference's value: 0
  dZ1 (inactive):      0
  dW1, db1:            the first rule + sum_r |x_r| bound(dZ1_r)
  loss:                128 u mean|term|
  gradient recovered as adam_m / c1 at t = 1:  + 2^-22 |g|

f16-subnormal backward operands (fp16 fixtures; dq, dZ2, dZ1 of the reference,
share of the non-zero ones below 2^-14, worst agent and loss), measured on the
fixtures the tests use: f16 1.67 %, shared_a 0.79 %, shared_b 1.01 %
(SUBNORMAL_SHARE; build() raises above 2 %).  With every weight in sixteenths
the share is 4 - 5 %; the fp16 fixtures take W1 in 256ths and W2, W3 in halves
(the same Q scale, 64 times the backward gain), after which what is left are
the rows whose TD error is below ~0.02: dq itself is then subnormal.
"""
import numpy as np

import oracle as O

D_IN, NACT, B = 89, 4, 128
SPARE = 16               # kernels.ReplayRing.SPARE: physical slots beyond the deque
U = 2.0 ** -22           # per addition (see the module docstring)
ULP16_FLOOR = 2.0 ** -24
F16_MIN_NORMAL = 2.0 ** -14
F16_MAX = 65504.0
GAMMA, LR = 0.99, 1e-3

# measured share of f16-subnormal non-zero backward operands per fp16 fixture
# (worst agent and loss); build() raises above 2 %
SUBNORMAL_SHARE = {"f16": 0.0167, "shared_a": 0.0079, "shared_b": 0.0101}

# denominators of (W1, W2, W3) per precision: fp16 takes W1 in 256ths and W2, W3
# in halves so that the backward operands stay clear of f16's subnormal range
DENOMS = {"fp32": (16, 16, 16), "bf16": (16, 16, 16), "fp16": (256, 2, 2)}


def _rnd16(precision):
    if precision == "fp32":
        return lambda x: np.asarray(x, np.float64)
    r = O.MIXED_ROUND[precision]

    def rnd(x):
        x = np.asarray(x, np.float64)
        x32 = x.astype(np.float32)
        assert np.array_equal(x32.astype(np.float64), x), "value is not an f32"
        return r(x32).astype(np.float64)
    return rnd


def ulp16(v, precision):
    """One unit in the last place of v in the 16-bit type, floored at 2^-24."""
    v = np.abs(np.asarray(v, np.float64))
    bits = 10 if precision == "fp16" else 7
    e = np.floor(np.log2(np.maximum(v, 2.0 ** -60)))
    return np.maximum(2.0 ** (e - bits), ULP16_FLOOR)


def quantum(x):
    """The largest power of two (at most 1) that divides every value of x."""
    x = np.asarray(x, np.float64)
    for k in range(0, 60):
        y = x * 2.0 ** k
        if np.array_equal(y, np.rint(y)):
            return 2.0 ** -k
    raise ValueError("values are not small dyadic rationals")


def split(flat, H):
    """Keras-order flat [.., P] -> (W1 [89,H], b1, W2 [H,H], b2, W3 [H,4], b3)."""
    sizes = [D_IN * H, H, H * H, H, H * NACT, NACT]
    shapes = [(D_IN, H), (H,), (H, H), (H,), (H, NACT), (NACT,)]
    o, out = 0, []
    for n, sh in zip(sizes, shapes):
        out.append(np.asarray(flat[o:o + n]).reshape(sh))
        o += n
    return out


def n_params(H):
    return D_IN * H + H + H * H + H + H * NACT + NACT


def block_slices(H):
    """{name: (offset, shape)} of the six Keras blocks in the flat vector."""
    sizes = [D_IN * H, H, H * H, H, H * NACT, NACT]
    shapes = [(D_IN, H), (H,), (H, H), (H,), (H, NACT), (NACT,)]
    o, out = 0, {}
    for name, n, sh in zip(("W1", "b1", "W2", "b2", "W3", "b3"), sizes, shapes):
        out[name] = (o, sh)
        o += n
    return out


def blocks(H):
    """The comparator's blocks: {name: flat index array into the Keras-order
    vector}.  Every 16 x 16 tile of W1 (features 0..87: five full tiles and the
    half tile 80..87 per 16 neurons) and of W2, the feature-88 column of W1 (the
    H weights of feature 88), b1, b2, W3, b3.  Together they cover every
    parameter exactly once."""
    sl = block_slices(H)
    out = {}
    o1 = sl["W1"][0]
    i1 = o1 + np.arange(D_IN * H).reshape(D_IN, H)
    for kt in range(6):
        for nt in range(H // 16):
            out[f"W1[{16 * kt}:{min(16 * kt + 16, 88)},{16 * nt}:{16 * nt + 16}]"] = \
                i1[16 * kt:min(16 * kt + 16, 88), 16 * nt:16 * nt + 16].ravel()
    out["W1[88,:]"] = i1[88]
    o2 = sl["W2"][0]
    i2 = o2 + np.arange(H * H).reshape(H, H)
    for kt in range(H // 16):
        for nt in range(H // 16):
            out[f"W2[{16 * kt}:{16 * kt + 16},{16 * nt}:{16 * nt + 16}]"] = \
                i2[16 * kt:16 * kt + 16, 16 * nt:16 * nt + 16].ravel()
    for name in ("b1", "b2", "W3", "b3"):
        o, sh = sl[name]
        out[name] = o + np.arange(int(np.prod(sh)))
    return out


# ---------------------------------------------------------------- exact forward
def _exact_dense(x, W, b, rnd, what):
    """z = rnd(rnd(x @ W) + b) with the proof that x @ W + b is exact in f32 in
    any summation order: everything scaled to integers by the quanta of the
    inputs and of the weights, sum|terms| + |bias| < 2^20 quanta.  Raises
    ValueError when a condition fails.  Returns (z, worst sum|terms| in quanta,
    worst sum|terms| as a value)."""
    qx, qw = quantum(x), quantum(W)
    q = qx * qw
    xi, wi, bi = x / qx, W / qw, b / q
    for name, v in (("inputs", xi), ("weights", wi), ("bias", bi)):
        if not np.array_equal(v, np.rint(v)):
            raise ValueError(f"{what}: {name} are not integers at quantum {q}")
    xi, wi, bi = (np.rint(v).astype(np.int64) for v in (xi, wi, bi))
    tot = np.abs(xi) @ np.abs(wi) + np.abs(bi)
    if not tot.max() < 2 ** 20:
        raise ValueError(f"{what}: sum|terms| + |bias| = {tot.max()} quanta >= 2^20")
    acc = (xi @ wi).astype(np.float64) * q        # exact: an integer below 2^20 times 2^-k
    z = rnd(rnd(acc) + b)                         # rnd(acc) + b: both multiples of q, exact
    if not np.abs(z).max() < F16_MAX:
        raise ValueError(f"{what}: f16 overflow")
    return z, int(tot.max()), float((np.abs(xi) @ np.abs(wi)).max() * q)


def exact_forward(ws, X, rnd, what="forward"):
    """(z1, z2, q, proof) of the Keras Sequential forward on exact inputs; proof
    = [(sum|terms| quanta, sum|terms| value)] per layer."""
    W1, b1, W2, b2, W3, b3 = (np.asarray(w, np.float64) for w in ws)
    X = np.asarray(X, np.float64)
    z1, t1, s1 = _exact_dense(X, W1, b1, rnd, what + " layer 1")
    z2, t2, s2 = _exact_dense(np.maximum(z1, 0), W2, b2, rnd, what + " layer 2")
    q, t3, s3 = _exact_dense(np.maximum(z2, 0), W3, b3, rnd, what + " layer 3")
    return z1, z2, q, [(t1, s1), (t2, s2), (t3, s3)]


# ---------------------------------------------------------------- builder
class Fixture:
    """What build() returns.  online / target: f32 [NW, P] Keras order (NW = 1
    for the shared net); obs_s / obs_n: int8 [fill, NA, 89]; act: int32 [fill,
    NA]; rew: f64 [fill, NA]; done: uint8 [fill, E]; idx: int32 [NA, 128] the
    replay draws of the first learn of an agent seeded with `seed` (per replica,
    agents in junction order on the replica's CPython stream)."""

    def net_of(self, j):
        return 0 if self.shared else j

    def slot_transition(self):
        """[slots] the transition each physical ring slot holds after `fill`
        stores (-1: never written)."""
        slots = self.cap + SPARE
        t = np.full(slots, -1, np.int64)
        for k in range(self.fill):
            t[k % slots] = k
        return t

    def batch(self, j, idx=None, use_start=True):
        """The batch of agent j at deque positions idx: (S, A, r, S2, D).
        use_start=False takes ring slot idx itself (a mutation)."""
        idx = np.asarray(self.idx[j] if idx is None else idx, np.int64)
        slots = self.cap + SPARE
        n = min(self.fill, self.cap)
        start = (self.fill - n) % slots
        t = self.slot_transition()[((start if use_start else 0) + idx) % slots]
        assert (t >= 0).all()
        e = j // self.A
        return (self.obs_s[t, j].astype(np.float64), self.act[t, j].astype(np.int64),
                self.rew[t, j], self.obs_n[t, j].astype(np.float64),
                self.done[t, e].astype(np.float32))


def _bias_quanta(den):
    """The grid of each layer's biases: 1/16 scaled by the layers' cumulative
    gain relative to weights in sixteenths (den = 16, 16, 16: 1/16 throughout),
    so that a bias stays in proportion to its layer's pre-activations."""
    s = [16.0 / d for d in den]
    return [s[0] / 16.0, s[0] * s[1] / 16.0, s[0] * s[1] * s[2] / 16.0]


def _draw_net(rng, H, den):
    bq = _bias_quanta(den)

    def w(shape, d):
        v = rng.choice([-2.0, -1.0, 1.0, 2.0], size=shape)
        return v * (rng.random_sample(shape) < 0.5) / d

    def b(n, q):
        return rng.randint(-8, 9, size=n) * q
    parts = [w((D_IN, H), den[0]), b(H, bq[0]), w((H, H), den[1]), b(H, bq[1]),
             w((H, NACT), den[2]), b(NACT, bq[2])]
    # centre every layer-1 unit on the observations' mean (2.5): without it a
    # unit whose weights sum far from 0 is on (or off) for the whole batch
    parts[1] = parts[1] - np.rint(2.5 * parts[0].sum(0) / bq[0]) * bq[0]
    return parts


def _flat(parts):
    return np.concatenate([np.asarray(p, np.float64).ravel() for p in parts])


def sample_idx(seed, E, A, n):
    """The first learn's replay draws of BatchedDQN(E, A, seed=seed): replica e
    draws on random.seed(seed + e), its agents in junction order."""
    out = np.zeros((E * A, B), np.int32)
    for e in range(E):
        s = O.py_stream(int(seed) + e)
        for a in range(A):
            out[e * A + a] = O.py_sample(s, n, B)
    return out


def build(seed, H, NA, precision, cap=160, fill=200, E=None, shared=False, ties=None,
          losses=("mse", "huber")):
    """The fixture for NA agents (E replicas of NA / E junctions) of width H.
    ties: the tied online W3 column pairs, per net in order -- default: nets 0
    and 1 get (1, 2) and (0, 3); the shared net gets ties[0].  Raises ValueError
    when any exactness or fixture condition fails (never a weaker fixture)."""
    E = E or (3 if shared else 2)
    assert NA % E == 0
    fx = Fixture()
    fx.seed, fx.H, fx.NA, fx.E, fx.A = int(seed), H, NA, E, NA // E
    fx.precision, fx.cap, fx.fill, fx.shared = precision, cap, fill, bool(shared)
    fx.NW = NW = 1 if shared else NA
    fx.ties = list(ties if ties is not None else [(1, 2), (0, 3)])[:NW]
    rng = np.random.RandomState(seed)
    den = DENOMS[precision]
    fx.obs_s = rng.randint(-1, 7, size=(fill, NA, D_IN)).astype(np.int8)
    fx.obs_n = rng.randint(-1, 7, size=(fill, NA, D_IN)).astype(np.int8)
    online, target, bq2 = [], [], _bias_quanta(den)[1]
    for w in range(NW):
        on, tg = _draw_net(rng, H, den), _draw_net(rng, H, den)
        if w < len(fx.ties):
            a, b = fx.ties[w]
            on[4][:, b] = on[4][:, a]
            on[5][b] = on[5][a]
        # centre every layer-2 unit on the mean of its inputs over the ring rows
        mine = slice(None) if shared else w
        rows = np.concatenate([fx.obs_s[:, mine], fx.obs_n[:, mine]]).reshape(-1, D_IN)
        for net in (on, tg):
            h1 = np.maximum(rows.astype(np.float64) @ net[0] + net[1], 0).mean(0)
            net[3] = net[3] - np.rint(h1 @ net[2] / bq2) * bq2
        online.append(_flat(on))
        target.append(_flat(tg))
    fx.online = np.stack(online).astype(np.float32)
    fx.target = np.stack(target).astype(np.float32)
    # at most 8 significant bits: bf16 (and so f16 and f32) holds every value exactly
    for w64, w32 in ((np.stack(online), fx.online), (np.stack(target), fx.target)):
        if not (np.array_equal(w32.astype(np.float64), w64)
                and np.array_equal(O.round_bf16(w32), w32)):
            raise ValueError(f"fixture seed {seed}: a weight needs more than 8 significant bits")
    fx.act = rng.randint(0, NACT, size=(fill, NA)).astype(np.int32)
    loc = rng.randint(0, 40, size=(fill, NA))
    glob = np.repeat(rng.randint(0, 400, size=(fill, E)), fx.A, axis=1)
    fx.rew = 0.3 * (-1.0 * loc) + 0.7 * (-1.0 * glob)
    fx.done = (rng.random_sample((fill, E)) < 0.25).astype(np.uint8)
    fx.idx = sample_idx(seed, E, fx.A, min(fill, cap))
    # exactness, proven in integer fixed point on every ring row, S and S', both nets
    rnd = _rnd16(precision)
    fx.proof = []
    for j in range(NA):
        w = fx.net_of(j)
        rows = np.concatenate([fx.obs_s[:, j], fx.obs_n[:, j]]).astype(np.float64)
        for name, net in (("online", fx.online[w]), ("target", fx.target[w])):
            fx.proof.append(exact_forward(split(net, H), rows, rnd, f"agent {j} {name}")[3])
    fx.stats = check_conditions(fx, losses=losses)
    return fx


def check_conditions(fx, idx=None, losses=("mse", "huber")):
    """Assert the fixture conditions on the batches at deque positions idx
    (default: the predicted draws); ValueError names the first that fails.
    Returns the measured figures."""
    idx = fx.idx if idx is None else np.asarray(idx)
    st = {"active1": [], "active2": [], "zero_preact": [], "both_ways": [], "subnormal": 0.0,
          "sum_terms": np.max([[s for _, s in p] for p in fx.proof], axis=0).tolist(),
          "quanta": np.max([[t for t, _ in p] for p in fx.proof], axis=0).tolist()}

    def need(ok, what):
        if not ok:
            raise ValueError(f"fixture seed {fx.seed} ({fx.precision}): {what}")
    for j in range(fx.NA):
        S, A, r, S2, D = fx.batch(j, idx[j])
        need(8 <= D.sum() <= B - 8, f"agent {j}: done rows {int(D.sum())}")
        need(np.bincount(A, minlength=NACT).min() >= 8, f"agent {j}: rows per action")
        for kind in losses:
            ref = learn_ref(fx, j, LOSS_KINDS[kind], idx=idx[j])
            big = int((np.abs(ref["e"]) > 1).sum())
            need(big >= 16 and B - big >= 16, f"agent {j} {kind}: {big} rows with |e| > 1")
            if fx.precision == "fp16":
                ops = np.concatenate([np.abs(ref[k]).ravel() for k in ("dq", "dz2", "dz1")])
                ops = ops[ops > 0]
                st["subnormal"] = max(st["subnormal"], float(np.mean(ops < F16_MIN_NORMAL)))
            back = max(np.abs(ref[k]).max() for k in ("dq", "dh2", "dh1", "g"))
            need(back < F16_MAX, f"agent {j} {kind}: f16 overflow in the backward ({back})")
            for z, key in ((ref["z1"], "1"), (ref["z2"], "2")):
                act = z > 0
                st["active" + key].append(float(act.mean()))
                need(0.3 <= act.mean() <= 0.7, f"agent {j}: layer {key} {act.mean():.2f} active")
                on = act.sum(0)
                both = float(np.mean((on >= 8) & (B - on >= 8)))
                st["both_ways"].append(both)
                need(both >= 0.9, f"agent {j}: layer {key} only {both:.2f} of the units go both ways")
            nz = int(((ref["z1"] == 0) & (ref["dh1"] != 0)).sum()
                     + ((ref["z2"] == 0) & (ref["dh2"] != 0)).sum())
            st["zero_preact"].append(nz)
            need(nz >= 1, f"agent {j}: no zero pre-activation under a non-zero gradient")
        w = fx.net_of(j)
        if (not fx.shared and j < len(fx.ties)) or (fx.shared and fx.ties):
            a, b = fx.ties[w]
            qo, qt = ref["q_next_online"], ref["q_next_target"]
            need(np.array_equal(qo[:, a], qo[:, b]), f"agent {j}: columns {a}, {b} not tied")
            others = [c for c in range(NACT) if c not in (a, b)]
            top = (qo[:, a][:, None] > qo[:, others]).all(1)
            far = np.abs(qt[:, a] - qt[:, b]) > 0.1
            need(int((top & far).sum()) >= 16,
                 f"agent {j}: tie decides only {int((top & far).sum())} rows")
            tg = split(fx.target[w], fx.H)
            need(not np.array_equal(tg[4][:, a], tg[4][:, b]), "target columns tied")
    need(st["subnormal"] <= 0.02, f"f16-subnormal backward operands {st['subnormal']:.4f}")
    return st


# ---------------------------------------------------------------- reference
LOSS_KINDS = {"mse": 0, "huber": 1}
MUTATIONS = ("online_target", "last_max", "ignore_done", "relu_ge", "post_adam_w3",
             "mse_dq_under_huber", "no_start")


def _adam_step1(w, g):
    """Keras-3 Adam at t = 1 from m = v = 0 (f32 ops)."""
    f = np.float32
    alpha, c1, c2, eps = O.keras_adam_consts(1, LR)
    g = np.asarray(g, f)
    m, v = g * c1, (g * g) * c2
    return (np.asarray(w, f) - (m * alpha) / (np.sqrt(v) + eps)).astype(f)


def learn_ref(fx, j, loss_kind, idx=None, mutate=()):
    """One learn of agent j in f64 under the rounding-point model of
    oracle.learn_mixed (16-bit rounding at the same points; none for fp32;
    dW / db never rounded here -- bounds() adds the independent 16-bit kernels'
    one rounding).  mutate: names from MUTATIONS, each a wrong kernel.  Returns
    a dict: loss, q, q_next_online, q_next_target, a_star, y, e, dq, dz2, dz1,
    z1, z2, dh1, dh2, g (Keras order), sabs (sum|terms| beside g), bz1 parts."""
    for m in mutate:
        assert m in MUTATIONS, m
    f32, H, prec = np.float32, fx.H, fx.precision
    rnd = _rnd16(prec)
    w = fx.net_of(j)
    S, A, r, S2, D = fx.batch(j, idx, use_start="no_start" not in mutate)
    rows = np.arange(B)
    wo, wt = split(fx.online[w].astype(np.float64), H), split(fx.target[w].astype(np.float64), H)
    qo = exact_forward(wo, S2, rnd)[2]
    qt = exact_forward(wo if "online_target" in mutate else wt, S2, rnd)[2]
    a_star = qo.argmax(1)
    if "last_max" in mutate:
        a_star = NACT - 1 - qo[:, ::-1].argmax(1)
    rn = O.zscore(r)
    dn = np.zeros(B, f32) if "ignore_done" in mutate else D.astype(f32)
    # f32 ops, each rounded once (learn_rules.hpp td_discount / td_target)
    y = rn + (f32(GAMMA) * (f32(1.0) - dn)) * qt[rows, a_star].astype(f32)
    z1, z2, q, _ = exact_forward(wo, S, rnd)
    h1, h2 = np.maximum(z1, 0), np.maximum(z2, 0)
    e = q[rows, A].astype(f32) - y
    e64 = e.astype(np.float64)
    if loss_kind == 1:
        terms = np.where(np.abs(e64) <= 1, 0.5 * e64 * e64, np.abs(e64) - 0.5)
        dq = np.where(np.abs(e64) <= 1, e64, np.sign(e64)) / B
    else:
        terms = e64 * e64
    if loss_kind == 0 or "mse_dq_under_huber" in mutate:
        dq = 2.0 * e64 / B
    dq = rnd(dq)
    DQ = np.zeros((B, NACT))
    DQ[rows, A] = dq
    W1, b1, W2, b2, W3, b3 = wo
    gW3, sW3 = h2.T @ DQ, h2.T @ np.abs(DQ)
    gb3, sb3 = DQ.sum(0), np.abs(DQ).sum(0)
    if "post_adam_w3" in mutate:
        W3 = rnd(_adam_step1(W3, gW3).astype(np.float64))
    ge = "relu_ge" in mutate
    dh2 = rnd(DQ @ W3.T)                      # one product per entry, W3 a power of two: exact
    dz2 = np.where(z2 >= 0 if ge else z2 > 0, dh2, 0.0)
    gW2, sW2 = h1.T @ dz2, h1.T @ np.abs(dz2)
    gb2, sb2 = dz2.sum(0), np.abs(dz2).sum(0)
    dh1_exact, s1 = dz2 @ W2.T, np.abs(dz2) @ np.abs(W2.T)
    dh1 = rnd(dh1_exact.astype(f32).astype(np.float64)) if prec != "fp32" else dh1_exact
    act1 = z1 >= 0 if ge else z1 > 0
    dz1 = np.where(act1, dh1, 0.0)
    d1 = 128 * U * s1                         # the f32 sum's distance from the exact one
    if prec == "fp32":
        bz1 = np.where(act1, d1, 0.0)
    else:
        # the kernel rounds an f32 sum within d1 of the exact one: where both
        # ends of that interval round to one 16-bit value (rounding is
        # monotone), so does the kernel's sum and dH1 is bit-determined; only an
        # entry with a rounding boundary inside the interval can move, by an ulp
        lo = rnd((dh1_exact - d1).astype(f32).astype(np.float64))
        hi = rnd((dh1_exact + d1).astype(f32).astype(np.float64))
        bz1 = np.where(act1 & (lo != hi), ulp16(dh1, prec) + d1, 0.0)
    gW1, sW1 = S.T @ dz1, np.abs(S).T @ np.abs(dz1)
    gb1, sb1 = dz1.sum(0), np.abs(dz1).sum(0)
    xW1, xb1 = np.abs(S).T @ bz1, bz1.sum(0)  # the dZ1 error carried into dW1 / db1
    zW = [np.zeros_like(x) for x in (gb2, gW2, gb3, gW3)]
    return dict(loss=float(terms.mean()), loss_abs=float(np.abs(terms).mean()), q=q,
                q_next_online=qo, q_next_target=qt, a_star=a_star, y=y, e=e, dq=dq, dz2=dz2,
                dz1=dz1, z1=z1, z2=z2, dh1=dh1, dh2=dh2, rn=rn, A=A, S=S, S2=S2, D=D,
                g=_flat([gW1, gb1, gW2, gb2, gW3, gb3]),
                sabs=_flat([sW1, sb1, sW2, sb2, sW3, sb3]),
                carried=_flat([xW1, xb1, zW[1], zW[0], zW[3], zW[2]]))


class Reference:
    """reference() of a fixture and loss: per-agent records `agents`, and the
    gradient the kernel must produce with its bound beside every entry: g /
    bound [NW, P] (the shared net: the mean over agents), loss / loss_bound
    [NA]."""


def reference(fx, loss="mse", idx=None, from_adam=None, mutate=()):
    """The f64 reference of one learn of every agent and the derived bounds.
    from_adam: the gradient is compared as adam_m / c1 (default: the
    independent kernels)."""
    kind = LOSS_KINDS[loss]
    idx = fx.idx if idx is None else np.asarray(idx)
    ref = Reference()
    ref.fx, ref.loss_name = fx, loss
    ref.agents = [learn_ref(fx, j, kind, idx[j], mutate) for j in range(fx.NA)]
    ref.loss = np.array([a["loss"] for a in ref.agents])
    ref.loss_bound = np.array([128 * U * a["loss_abs"] for a in ref.agents])
    g = np.stack([a["g"] for a in ref.agents])
    sabs = np.stack([a["sabs"] for a in ref.agents])
    carried = np.stack([a["carried"] for a in ref.agents])
    if fx.shared:
        # the mean over agents of unrounded gradients (round_grad=False)
        g, sabs, carried = g.mean(0)[None], sabs.mean(0)[None], carried.mean(0)[None]
        bound = (128 + fx.NA) * U * sabs + carried
    else:
        bound = 128 * U * sabs + carried
        if fx.precision != "fp32":
            # the kernel rounds, once, an f32 sum within `bound` of the exact
            # one: an entry moves (by an ulp) only where a 16-bit rounding
            # boundary lies inside that interval, and is bit-determined elsewhere
            rnd = _rnd16(fx.precision)
            lo = rnd((g - bound).astype(np.float32).astype(np.float64))
            hi = rnd((g + bound).astype(np.float32).astype(np.float64))
            g = rnd(g.astype(np.float32).astype(np.float64))
            bound = np.where(lo != hi, bound + ulp16(g, fx.precision), 0.0)
        if from_adam is None or from_adam:
            bound = bound + 2.0 ** -22 * np.abs(g)
    ref.g, ref.bound, ref.sabs = g, bound, sabs
    return ref


# ---------------------------------------------------------------- comparator
def ratio(delta, bound):
    """|delta| / bound entry by entry; 0 where both are 0, inf where only the
    bound is."""
    d = np.abs(np.asarray(delta, np.float64))
    b = np.asarray(bound, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(b > 0, d / b, np.where(d > 0, np.inf, 0.0))


def compare(g_gpu, ref, net=0):
    """{block: (worst |delta| / bound, flat Keras index where)} of one net's
    gradient (Keras order) against ref.g[net] / ref.bound[net], over every
    block of blocks(H): every entry is in exactly one block."""
    g_gpu = np.asarray(g_gpu, np.float64)
    assert g_gpu.shape == ref.g[net].shape
    rt = ratio(g_gpu - ref.g[net], ref.bound[net])
    rt = np.where(np.isfinite(g_gpu), rt, np.inf)
    out, seen = {}, 0
    for name, ix in blocks(ref.fx.H).items():
        k = int(np.argmax(rt[ix]))
        out[name] = (float(rt[ix][k]), int(ix[k]))
        seen += ix.size
    assert seen == g_gpu.size
    return out


def worst(cmp):
    """(ratio, block, index) of the worst block of a compare() result."""
    name = max(cmp, key=lambda k: cmp[k][0])
    return cmp[name][0], name, cmp[name][1]


def summary(cmp):
    """Worst ratio per block kind (W1 tiles, W1[88,:], b1, W2 tiles, b2, W3, b3)."""
    out = {}
    for name, (r, _) in cmp.items():
        kind = name if name in ("W1[88,:]", "b1", "b2", "W3", "b3") else name[:2] + " tiles"
        out[kind] = max(out.get(kind, 0.0), r)
    return out


# the fixtures the GPU tests use: name -> build() arguments
FIXTURES = {
    "f32_128": dict(seed=11, H=128, NA=6, precision="fp32"),
    "f32_64": dict(seed=20, H=64, NA=6, precision="fp32"),
    "f16": dict(seed=11, H=128, NA=6, precision="fp16"),
    "bf16": dict(seed=13, H=128, NA=6, precision="bf16"),
    "shared_a": dict(seed=24, H=128, NA=12, precision="fp16", shared=True, ties=[(1, 2)]),
    "shared_b": dict(seed=25, H=128, NA=12, precision="fp16", shared=True, ties=[(0, 3)]),
}
_CACHE = {}


def fixture(name):
    """build(**FIXTURES[name]), built once per process."""
    if name not in _CACHE:
        _CACHE[name] = build(**FIXTURES[name])
    return _CACHE[name]
