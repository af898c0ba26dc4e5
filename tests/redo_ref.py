"""Numpy restatement of dead-unit recycling (include/dmdqn.h dmdqn_redo) for the
tests, written from the rule in Keras order: plain W1 [89, 128], W2 [128, 128],
W3 [128, 4] and the biases.  The device layout enters only through the
callers' keras_to_kernel / kernel_to_keras, so this is an independent check of
the kernel's index arithmetic.
"""
import numpy as np

import exact_fixture as XF

H, D_IN, NACT = 128, 89, 4
M64 = (1 << 64) - 1
G = 0x9E3779B97F4A7C15
LIM1 = np.float32(np.sqrt(6.0 / 89.0))
LIM2 = np.float32(np.sqrt(6.0 / 128.0))


def mix64(x):
    """The u64 mixer of the rule, on a Python int."""
    x &= M64
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & M64
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & M64
    x ^= x >> 31
    return x


def fresh(seed, rnd, agent, layer, unit, ins, lim):
    """f32 [len(ins)]: the fresh weights `ins` of unit `unit` of `layer` (0:
    a W1 column, 1: a W2 column) of global agent `agent`."""
    seed, rnd, agent, layer, unit = (int(x) for x in (seed, rnd, agent, layer, unit))
    k = mix64(seed + G * (rnd + 1))
    out = np.zeros(len(ins), np.float32)
    for n, i in enumerate(ins):
        c = ((agent * 2 + layer) * 128 + unit) * 128 + int(i)
        u24 = mix64(k + G * (c + 1)) >> 40
        t = np.float32(2 * u24 + 1 - (1 << 24)) * np.float32(2.0 ** -24)  # both exact
        out[n] = np.float32(lim) * t                                       # one f32 multiply
    return out


def mask_bits(mask):
    """uint32 [..., 4] words -> bool [..., 128]."""
    mask = np.asarray(mask, np.uint32)
    u = np.arange(128)
    return ((mask[..., u // 32] >> (u % 32).astype(np.uint32)) & np.uint32(1)).astype(bool)


def bits_mask(bits):
    """bool [..., 128] -> uint32 [..., 4] words."""
    bits = np.asarray(bits, bool)
    out = np.zeros(bits.shape[:-1] + (4,), np.uint32)
    for u in range(128):
        out[..., u // 32] |= bits[..., u].astype(np.uint32) << np.uint32(u % 32)
    return out


def streak_step(streak, dead, patience):
    """(new streak uint8, fired bool) of one probe: dead bool, same shape."""
    s = np.asarray(streak, np.int64)
    s = np.where(dead, np.minimum(s + 1, 255), 0)
    fire = s >= int(patience)
    return np.where(fire, 0, s).astype(np.uint8), fire


def recycle_net(ws, ms, vs, R1, R2, seed, rnd, agent):
    """One agent: ws / ms / vs = [W1, b1, W2, b2, W3, b3] (f32, written in
    place); R1 / R2 bool [128], the fired units of layer 1 / 2."""
    W1, b1, W2, b2, W3, b3 = ws
    written = [np.zeros(w.shape, bool) for w in ws]
    for u in np.flatnonzero(R1):
        W1[:, u] = fresh(seed, rnd, agent, 0, u, range(D_IN), LIM1)
        b1[u] = 0.0
        written[0][:, u] = True
        written[1][u] = True
    for o in np.flatnonzero(R2):
        W2[:, o] = fresh(seed, rnd, agent, 1, o, range(H), LIM2)
        b2[o] = 0.0
        W3[o, :] = 0.0
        written[2][:, o] = True
        written[3][o] = True
        written[4][o, :] = True
    for u in np.flatnonzero(R1):  # zero wins on the overlap
        W2[u, :] = 0.0
        written[2][u, :] = True
    for m, v, wr in zip(ms, vs, written):
        m[wr] = 0.0
        v[wr] = 0.0


def redo_ref(params, adam_m, adam_v, streak, dead_mask, patience, seed, rnd, agent0=0):
    """The whole launch in Keras order.  params / adam_m / adam_v f32 [NA, P]
    (Keras order), streak uint8 [NA, 2, 128], dead_mask uint32 [NA, 2, 4].
    Returns new (params, adam_m, adam_v, streak, recycled uint32 [NA, 2, 4],
    n_recycled int32 [NA, 2]); the inputs are not changed."""
    out = [np.array(x, np.float32, copy=True) for x in (params, adam_m, adam_v)]
    new_streak, fire = streak_step(streak, mask_bits(dead_mask), patience)
    for j in range(out[0].shape[0]):
        if not fire[j].any():
            continue
        parts = [[a.copy() for a in XF.split(x[j], H)] for x in out]
        recycle_net(parts[0], parts[1], parts[2], fire[j, 0], fire[j, 1], seed, rnd, agent0 + j)
        for x, p in zip(out, parts):
            x[j] = np.concatenate([a.ravel() for a in p])
    return (out[0], out[1], out[2], new_streak, bits_mask(fire),
            fire.sum(axis=2).astype(np.int32))
