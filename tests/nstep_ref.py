"""n-step returns: a pure-Python restatement of the contract of
AgentConfig.n_step / dmdqn_replay_nstep_commit (include/dmdqn.h), for one agent.

A raw transition is a tuple (s, a, r, s2, d) in store order.  Python floats
are IEEE doubles and `*` / `+` on them are single rounded operations, so the
returns below are the bits the kernel must produce."""
from collections import deque

import numpy as np


def nstep_return(rewards, gamma):
    """R = r_0 + g r_1 + g^2 r_2 + ...: w = w * g; R = R + w * r_j, in order."""
    g = float(gamma)
    R, w = float(rewards[0]), 1.0
    for r in rewards[1:]:
        w = w * g
        R = R + w * float(r)
    return R


def window_commit(window, gamma):
    """The transition committed for the start window[0] (len(window) = n)."""
    m = len(window)
    for j, t in enumerate(window, 1):
        if t[4]:
            m = j
            break
    first, last = window[0], window[m - 1]
    return (first[0], first[1], nstep_return([t[2] for t in window[:m]], gamma), last[3],
            1 if last[4] else 0)


def nstep_commits(raw, n, gamma):
    """The committed transitions after the raw stores `raw`, in commit order:
    raw store k >= n - 1 commits the start k - n + 1, from raw[k-n+1 .. k]
    alone; stores 0 .. n-2 commit nothing, and the last n - 1 raw transitions
    are never committed."""
    raw = list(raw)
    return [window_commit(raw[k - n + 1:k + 1], gamma) for k in range(n - 1, len(raw))]


def textbook_commits(raw, n, gamma):
    """The textbook n-step buffer: append; when the deque holds n emit its
    oldest start; on a done flush the deque (every remaining start, each cut at
    the done)."""
    dq, out = deque(), []

    def emit():
        w = list(dq)
        out.append((w[0][0], w[0][1], nstep_return([t[2] for t in w], gamma), w[-1][3],
                    1 if w[-1][4] else 0))
        dq.popleft()

    for t in raw:
        dq.append(t)
        if t[4]:
            while dq:
                emit()
        elif len(dq) == n:
            emit()
    return out


def bootstrap_gamma(gamma, n):
    """What the learn receives for gamma: float32 of 1.0 multiplied n times by
    the Python float."""
    G = 1.0
    for _ in range(n):
        G = G * float(gamma)
    return np.float32(G)
