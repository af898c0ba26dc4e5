"""Global-norm gradient clipping (include/dmdqn.h dmdqn_adam_agents_clip; Keras
3 clip_by_global_norm / global_norm) restated in numpy and plain Python, for
tests/test_clip_cpu.py and tests/test_gpu_clip.py:

    S      = sum_i g_i^2                    exact (math.fsum over exact squares)
    norm   = fl32(sqrt(S))                  f64 sqrt, one rounding to f32
    s_fin  = fl32(clip * min(fl32(1 / norm), fl32(1 / clip)))
    scale  = fl32(s_fin + fl32(norm - norm))
    g'_i   = fl32(g_i * scale)

then the f32 Keras-3 Adam step of tests/test_gpu_split.py on g'.  Every f32
operation is a numpy float32 operation, rounded on its own."""
import math

import numpy as np

f32 = np.float32


def sum_squares(g):
    """The exact sum of squares of a float32 vector, rounded once to f64.  A
    float32 square is exact in f64 (48 significant bits at most)."""
    g64 = np.asarray(g, dtype=np.float32).astype(np.float64)
    with np.errstate(over="ignore"):
        sq = g64 * g64
    if not np.isfinite(sq).all():
        return float("nan") if np.isnan(sq).any() else float("inf")
    return math.fsum(sq.tolist())


def norm_of(S):
    with np.errstate(invalid="ignore"):
        return f32(np.sqrt(np.float64(S)))


def global_norm(g):
    return norm_of(sum_squares(g))


def clip_scale(norm, clip):
    norm, clip = f32(norm), f32(clip)
    with np.errstate(all="ignore"):
        s_fin = clip * np.minimum(f32(1) / norm, f32(1) / clip)
        scale = s_fin + (norm - norm)
    assert scale.dtype == np.float32
    return scale


def clip_gradient(g, clip):
    """(norm, g') of one agent's gradient."""
    g = np.asarray(g, dtype=np.float32)
    norm = global_norm(g)
    with np.errstate(all="ignore"):
        gc = g * clip_scale(norm, clip)
    assert gc.dtype == np.float32
    return norm, gc


def keras_adam(p, m, v, g, alpha, c1, c2, eps):
    """keras/src/optimizers/adam.py update_step in f32, every op rounded on its
    own: (p, m, v) after the step."""
    alpha, c1, c2, eps = f32(alpha), f32(c1), f32(c2), f32(eps)
    with np.errstate(all="ignore"):
        m1 = m + (g - m) * c1
        v1 = v + (g * g - v) * c2
        p1 = p - (m1 * alpha) / (np.sqrt(v1) + eps)
    assert p1.dtype == m1.dtype == v1.dtype == np.float32
    return p1, m1, v1


def clip_adam(p, m, v, g, clip, alpha, c1, c2, eps):
    """(norm, p, m, v) after one clipped Adam step of one agent."""
    norm, gc = clip_gradient(g, clip)
    return (norm,) + keras_adam(p, m, v, gc, alpha, c1, c2, eps)


def boundary_margin(S):
    """The relative distance of sqrt(S) from the nearest midpoint between two
    adjacent float32 values: a sum S~ within relative e of S gives the same
    float32 norm when e / 2 (and the f64 sqrt's own 2^-53) stay below it.  inf
    for S == 0 (the norm is exactly 0) and for a non-finite S."""
    if not math.isfinite(S) or S == 0.0:
        return float("inf")
    r = math.sqrt(S)
    with np.errstate(over="ignore"):
        n = f32(r)
        up, dn = np.nextafter(n, f32(np.inf)), np.nextafter(n, f32(-np.inf))
    mids = [(float(n) + float(x)) / 2.0 for x in (up, dn) if np.isfinite(x)]
    return min(abs(r - mid) for mid in mids) / r


def soft_target(w, t, tau_f, omt_f):
    """fl32(fl32(tau * w) + fl32(one_minus_tau * t))."""
    with np.errstate(all="ignore"):
        out = f32(tau_f) * w + f32(omt_f) * t
    assert out.dtype == np.float32
    return out
