"""Numpy restatement of the network health probe (include/dmdqn.h
dmdqn_net_probe, dmdqn_layer_norms) for the tests.

The forward figures come from exact_fixture's exact dense layers: on those
fixtures every pre-activation is determined whatever the summation order, so
every count is an integer with one right answer and the f64 sums of the 16-bit
activations are exact (probe_ref asserts it by summing in two orders).  An
output layer that overflows or holds a NaN (the tests mutate W3 / b3 for it)
falls back to oracle._mixed_fwd's dense: f32 products and sums rounded once,
then the 16-bit bias add.  The layer sums come from kernel_to_keras plus f64
numpy.
"""
import numpy as np

import exact_fixture as XF
import oracle as O

B, H, NACT = 128, 128, 4
VARIABLES = ("W1", "b1", "W2", "b2", "W3", "b3")


def forward(ws, X, precision):
    """(z1, z2, q) of the Keras forward under the mixed policy on exact inputs,
    as f64 arrays of 16-bit values (q may hold inf / NaN)."""
    rnd = XF._rnd16(precision)
    W1, b1, W2, b2, W3, b3 = (np.asarray(w, np.float64) for w in ws)
    X = np.asarray(X, np.float64)
    z1 = XF._exact_dense(X, W1, b1, rnd, "layer 1")[0]
    z2 = XF._exact_dense(np.maximum(z1, 0), W2, b2, rnd, "layer 2")[0]
    h2 = np.maximum(z2, 0)
    try:
        q = XF._exact_dense(h2, W3, b3, rnd, "layer 3")[0]
    except ValueError:
        r = O.MIXED_ROUND[precision]
        with np.errstate(over="ignore", invalid="ignore"):
            acc = np.matmul(h2.astype(np.float32), W3.astype(np.float32), dtype=np.float32)
            q = r(r(acc) + r(b3.astype(np.float32))).astype(np.float64)
    return z1, z2, q


def _sum_two_orders(h):
    """The f64 sum of h, asserted exact: the same bits forwards, backwards and
    pairwise (numpy's own order)."""
    flat = np.asarray(h, np.float64).ravel()
    a = float(np.add.reduce(flat))
    b, c = 0.0, 0.0
    for v in flat:
        b += float(v)
    for v in flat[::-1]:
        c += float(v)
    assert a == b == c, (a, b, c)
    return a


def probe_ref(ws, X, precision, relu_ge=False):
    """(counts int64 [5], stats f64 [5], dead_mask uint32 [2, 4]) of one agent.
    relu_ge: a wrong ReLU that takes z >= 0 as active (the tests show that the
    fixtures tell the two apart)."""
    z1, z2, q = forward(ws, X, precision)
    counts, stats = np.zeros(5, np.int64), np.zeros(5, np.float64)
    mask = np.zeros((2, 4), np.uint32)
    for layer, z in enumerate((z1, z2)):
        with np.errstate(invalid="ignore"):
            on = (z >= 0) if relu_ge else (z > 0)   # False for a NaN
        h = np.where(on, z, 0.0)
        counts[2 * layer] = int(on.sum())
        dead = ~on.any(axis=0)
        counts[2 * layer + 1] = int(dead.sum())
        for u in np.flatnonzero(dead):
            mask[layer, u // 32] |= np.uint32(1) << np.uint32(u % 32)
        stats[layer] = _sum_two_orders(h)
    for j, z in enumerate((z1, z2, q)):
        fin = np.isfinite(z)
        counts[4] += int((~fin).sum())
        stats[2 + j] = float(np.abs(z[fin]).max()) if fin.any() else 0.0
    return counts, stats, mask


def layer_sums_ref(x, hidden, y=None, eps=None):
    """f64 [NW, 6]: per Keras variable the sum of squares of x [NW, P] (device
    layout), or with y of u = fl32(x / fl32(fl32(sqrt(y)) + eps)) -- numpy's
    float32 ops round each step as the kernel does."""
    from dmdqn_amd.agent import kernel_to_keras
    x = np.asarray(x, np.float32)
    if y is not None:
        with np.errstate(all="ignore"):
            x = (x / (np.sqrt(np.asarray(y, np.float32)) + np.float32(eps))).astype(np.float32)
    k = kernel_to_keras(x, hidden).astype(np.float64)
    out = np.zeros((x.shape[0], 6), np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        for i, name in enumerate(VARIABLES):
            o, sh = XF.block_slices(hidden)[name]
            seg = k[:, o:o + int(np.prod(sh))]
            out[:, i] = (seg * seg).sum(axis=1)
    return out
