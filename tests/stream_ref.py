"""The reference of the device MT19937 streams: the real generators.

`np.random.RandomState` is the numpy stream behind select_action
(dqn_agent.py:263-265) and `random.Random` the CPython stream behind
ReplayBuffer.sample (dqn_agent.py:63).  The functions below are thin wrappers
that also record the stream position before every draw, so that the case
tables at the end can be checked (tests/test_stream_ref_cpu.py, and again by
tests/test_gpu_stream_edges.py) for the edges they are meant to reach: a twist
between the two words of one rand(), between rand() and its randint, inside a
rejection redraw, a sample that ends exactly at the end of a 624-word block.

Host only: nothing here touches a GPU.
"""
import math
import random

import numpy as np
import pytest

MT_N = 624

# Random.sample's body changed across CPython versions (3.9 and before convert
# the population another way, 3.12 draws differently for small k): the device
# sampler restates the 3.10 / 3.11 body, so the interpreter must run that one.
_SAMPLE_PIN = [130, 183, 271, 14]  # random.Random(5).sample(range(300), 4) on CPython 3.10.12
if random.Random(5).sample(range(300), 4) != _SAMPLE_PIN:
    pytest.skip("this interpreter's random.Random.sample is not the CPython 3.10/3.11 body "
                "the device sampler restates", allow_module_level=True)


# ---------------------------------------------------------------- numpy stream
def np_pos(rs):
    """The stream position of a RandomState: 0..624 (624 = a twist is due)."""
    return int(rs.get_state()[2])


def np_act(rs, A, eps, n_actions, greedy):
    """select_action for A agents in order on rs: rand(), then randint(0,
    n_actions) if it is below eps, else greedy[j].  Returns (actions int32 [A],
    trace): trace holds one (kind, before, after) per draw, kind "rand" or
    "randint", with the stream position before and after it."""
    out = np.zeros(A, np.int32)
    trace = []
    for j in range(A):
        p0 = np_pos(rs)
        r = rs.rand()
        p1 = np_pos(rs)
        trace.append(("rand", p0, p1))
        if r < eps:
            out[j] = rs.randint(0, n_actions)
            trace.append(("randint", p1, np_pos(rs)))
        else:
            out[j] = greedy[j]
    return out, trace


def np_uniform(rs, A, n_actions):
    """randint(0, n_actions) alone per agent (test.py:92-93)."""
    out = np.zeros(A, np.int32)
    trace = []
    for j in range(A):
        p0 = np_pos(rs)
        out[j] = rs.randint(0, n_actions)
        trace.append(("randint", p0, np_pos(rs)))
    return out, trace


def np_u32(rs, n):
    """n raw tempered words of the stream."""
    return np.frombuffer(rs.bytes(4 * n), dtype="<u4").astype(np.uint64)


def np_state_words(rs):
    """[625] uint32: the 624 key words and the position (the device layout)."""
    st = rs.get_state()
    return np.concatenate([np.asarray(st[1], np.uint32), np.array([st[2]], np.uint32)])


# ---------------------------------------------------------------- CPython stream
def py_sample(r, n, k):
    return np.array(r.sample(range(n), k), np.int32)


def py_u32(r, n):
    return np.array([r.getrandbits(32) for _ in range(n)], np.uint64)


def py_state_words(r):
    """[625] uint32: the 624 key words and the position (the device layout)."""
    return np.array(r.getstate()[1], dtype=np.uint64).astype(np.uint32)


def py_pos(r):
    return int(r.getstate()[1][MT_N])


# ---------------------------------------------------------------- coverage of a trace
def words(before, after):
    """Words a draw consumed (fewer than 624): the position runs 0..624 and a
    draw at 624 twists first and leaves it at 1."""
    return (after - before) % MT_N


def act_coverage(traces):
    """What the draws of a case reached, over all its streams.  traces: one
    list of (kind, before, after) per stream (every call appended)."""
    cov = {"rand_at_623": 0, "randint_at_624": 0, "redraws": 0, "twist_in_redraw": 0,
           "min_words": None}
    for tr in traces:
        total = 0
        for kind, b, a in tr:
            w = words(b, a)
            total += w
            if kind == "rand":
                cov["rand_at_623"] += b == MT_N - 1
            else:
                cov["randint_at_624"] += b == MT_N
                cov["redraws"] += max(w - 1, 0)
                # more than one word, and the position wrapped after the first
                cov["twist_in_redraw"] += w > 1 and b < MT_N and a < b
        cov["min_words"] = total if cov["min_words"] is None else min(cov["min_words"], total)
    return cov


def is_pow2(n):
    return n & (n - 1) == 0


def check_act_coverage(cov, n_actions):
    """The conditions every fixed act case meets (asserted on the CPU and
    again by the GPU test that runs the case)."""
    assert cov["rand_at_623"] >= 1, cov      # a twist between the two words of a rand()
    assert cov["randint_at_624"] >= 1, cov   # a twist between rand() and its randint
    if not is_pow2(n_actions):
        assert cov["redraws"] >= 1, cov
        assert cov["twist_in_redraw"] >= 1, cov
    assert cov["min_words"] >= 3 * MT_N, cov


# ---------------------------------------------------------------- case tables
def act_calls(A):
    return math.ceil(3 * MT_N / (2 * A)) + 1


def fused_steps(A):
    return min(math.ceil(3 * MT_N / (2.5 * A)), 800)


def greedy_table(seed, E, A, n_actions):
    """The fixed `greedy` array of a case, int32 [E, A]."""
    return np.random.RandomState(seed).randint(0, n_actions, size=(E, A)).astype(np.int32)


ACT_E = 8

# dmdqn_act: (A, eps, n_actions, first seed); the streams are seeded first seed
# .. first seed + 7.  Every A at eps 0.5 / n 4, every eps at A 16, every n at
# A 7 and A 64.  A = 209: 3 A > 624, the fixed-count path is never eligible.
# The first seeds come from a CPU search (the smallest multiple of 8 whose
# eight streams meet check_act_coverage); test_stream_ref_cpu.py asserts the
# conditions for exactly these.
ACT_CASES = [
    (1, 0.5, 4, 0), (7, 0.5, 4, 0), (16, 0.5, 4, 0), (64, 0.5, 4, 0), (100, 0.5, 4, 0),
    (209, 0.5, 4, 0),
    (16, 0.05, 4, 8), (16, 0.999, 4, 0),
    (7, 0.5, 2, 0), (7, 0.5, 3, 0), (7, 0.5, 5, 0), (7, 0.5, 12, 0),
    (64, 0.5, 2, 0), (64, 0.5, 3, 0), (64, 0.5, 5, 0), (64, 0.5, 12, 0),
]

# the fused env step: (rows, cols, n_actions, first seed), E = 3 streams,
# eps = 0.5, fused_steps(A) steps: the extra-LDS branch (1x1), the LDS image
# (2x2, 4x4), the 512- and the 1024-thread register kernels (5x5, 8x8).  First
# seeds by the same search (multiples of 3)
FUSED_E = 3
FUSED_EPS = 0.5
FUSED_CASES = [
    (1, 1, 4, 12), (2, 2, 4, 9), (4, 4, 4, 9), (5, 5, 4, 12), (8, 8, 4, 0), (2, 2, 3, 6),
]

# the eps hand-over: A 16, n 4, 60 calls on the same eight streams
HANDOVER_A = 16
HANDOVER_CALLS = 60
HANDOVER_SEED = 0
_HANDOVER_HEAD = [1.0, 1.0, 0.5, 1.0, 0.05, 1.0, 1.0, 0.999, 1.0]


def handover_eps():
    """[1, 1, 0.5, 1, 0.05, 1, 1, 0.999, 1, ...]: the head repeated over 60 calls."""
    return [_HANDOVER_HEAD[i % len(_HANDOVER_HEAD)] for i in range(HANDOVER_CALLS)]


# the sampler's block-end cases: (seed, A, n, k, repetitions, final position).
# After the last sample the CPython stream stands exactly at 624 (the stored
# state must stay the current block with position 624) or at 1.
# Seeds by CPU search (the first that end there).
SAMPLE_END_SET = [(5, 3, 10000, 128, 2, 624), (14, 3, 10000, 128, 2, 1)]
SAMPLE_END_POOL = [(350, 4, 500, 128, 2, 624), (1587, 4, 500, 128, 2, 1)]

# the set branch a third full, (A, n, k): n is the first length past the pool
# threshold of its k, so already-selected and in-chunk repeats are common
SAMPLE_DENSE = [(5, 1046, 341), (2, 4118, 1365)]

# the small shapes of test_gpu_rng_observe.py::test_replay_sample_shapes, here
# with the stored state compared after the second repetition
SAMPLE_SHAPES = [(64, 200, 128), (70, 300, 32), (3, 21, 5), (3, 22, 5), (5, 7, 7),
                 (2, 3000, 1000), (1, 128, 128), (3, 16385, 128)]


def setsize(k):
    """Random.sample's threshold (CPython 3.10 / 3.11): a population of at
    most setsize entries takes the pool branch, a longer one the set branch."""
    s = 21
    if k > 5:
        s += 4 ** math.ceil(math.log(k * 3, 4))
    return s


def run_act_case(A, eps, n_actions, seed0, E=ACT_E, calls=None, starts=None, greedy_n=None):
    """The reference of one act case: (actions [calls, E, A], traces, final
    state words [E, 625], greedy [E, A]).  eps: one value, or one per call.
    starts: a list that receives, per stream, the position before every call.
    greedy_n: the range of the greedy table when it is not n_actions."""
    calls = act_calls(A) if calls is None else calls
    eps_of = eps if isinstance(eps, (list, tuple)) else [eps] * calls  # per call
    greedy = greedy_table(seed0 + 1000003, E, A, greedy_n or n_actions)
    acts = np.zeros((calls, E, A), np.int32)
    traces, states = [], []
    for e in range(E):
        rs = np.random.RandomState(seed0 + e)
        tr, st = [], []
        for c in range(calls):
            st.append(np_pos(rs))
            acts[c, e], t = np_act(rs, A, eps_of[c], n_actions, greedy[e])
            tr += t
        traces.append(tr)
        if starts is not None:
            starts.append(st)
        states.append(np_state_words(rs))
    return acts, traces, np.stack(states), greedy


def run_sample_case(seed, A, n, k, reps):
    """(indices [reps, A, k], final state words, final position)."""
    r = random.Random(seed)
    idx = np.stack([np.stack([py_sample(r, n, k) for _ in range(A)]) for _ in range(reps)])
    return idx, py_state_words(r), py_pos(r)
