"""GPU: the two device MT19937 streams against the real generators
(np.random.RandomState, random.Random; tests/stream_ref.py) where a stream
kernel goes wrong: eps < 1 with twists between the words of one draw, action
counts that redraw, one action, eps = 1 and eps < 1 calls alternating on one
stream, the fused env step's copy of the act, seeds at and past 2**32, samples
that end exactly at a block end, the set branch a third full -- and after every
case all 625 stored words of the stream, not only the draws.  The fixed cases
and the conditions they meet are those of tests/test_stream_ref_cpu.py."""
import functools
import random

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import stream_ref as SR  # noqa: E402
from dmdqn_amd import kernels as K  # noqa: E402
from dmdqn_amd.env import EnvConfig, TrafficEnv  # noqa: E402

DEV = "cuda"


def _words(state):
    """A device stream tensor as uint32 [E, 625]."""
    return state.cpu().numpy().view(np.uint32)


@functools.lru_cache(maxsize=None)
def _act_ref(*args, **kw):
    return SR.run_act_case(*args, **kw)


def _run_act(seed0, E, A, eps_of, n, greedy):
    st = K.seed_streams(list(range(seed0, seed0 + E)), "np")
    g = torch.from_numpy(greedy).to(DEV)
    out = torch.full((len(eps_of), E, A), -1, dtype=torch.int32, device=DEV)
    for c, eps in enumerate(eps_of):
        K.act(st, A, eps=eps, n_actions=n, greedy=g, out=out[c])
    return out.cpu().numpy(), _words(st)  # the actions stay on the device until here


# ---------------------------------------------------------------- dmdqn_act
@pytest.mark.parametrize("case", SR.ACT_CASES, ids=str)
def test_act_matches_numpy_across_twists(case):
    A, eps, n, seed0 = case
    acts, traces, states, greedy = _act_ref(A, eps, n, seed0)
    SR.check_act_coverage(SR.act_coverage(traces), n)
    got, words = _run_act(seed0, SR.ACT_E, A, [eps] * SR.act_calls(A), n, greedy)
    np.testing.assert_array_equal(got, acts)
    np.testing.assert_array_equal(words, states)


def test_act_eps_handover_on_one_stream():
    """A decaying schedule in small: eps = 1 calls (the fixed-count path moves
    only the position word) between eps < 1 calls (the general path stages and
    stores the whole state) on the same streams."""
    eps, A = SR.handover_eps(), SR.HANDOVER_A
    acts, _, states, greedy = SR.run_act_case(A, eps, 4, SR.HANDOVER_SEED, calls=len(eps))
    got, words = _run_act(SR.HANDOVER_SEED, SR.ACT_E, A, eps, 4, greedy)
    np.testing.assert_array_equal(got, acts)
    np.testing.assert_array_equal(words, states)


# ---------------------------------------------------------------- one action
@pytest.mark.parametrize("eps", [1.0, 0.5])
def test_act_one_action_draws_rand_only(eps):
    """randint(0, 1) is 0 and draws no word: two words per agent.  The greedy
    table holds 0..3, so the actions show which agents explored."""
    A, calls = 16, 25  # 800 words: past the seed's twist and the next
    acts, _, states, greedy = SR.run_act_case(A, eps, 1, 40, calls=calls, greedy_n=4)
    got, words = _run_act(40, SR.ACT_E, A, [eps] * calls, 1, greedy)
    np.testing.assert_array_equal(got, acts)
    np.testing.assert_array_equal(words, states)
    assert int(words[0, SR.MT_N]) == (2 * A * calls) % SR.MT_N


def test_uniform_one_action_leaves_the_stream():
    """dmdqn_act_uniform with one action between two four-action calls: zeros,
    and the stream exactly where numpy's is -- also when it stands at 624."""
    seeds, A = [5, 6, 7], 9
    st = K.seed_streams(seeds, "np")
    refs = [np.random.RandomState(s) for s in seeds]
    fresh = np.stack([SR.np_state_words(r) for r in refs])
    a0 = K.act(st, A, n_actions=1, uniform=True).cpu().numpy()  # position 624: no twist
    np.testing.assert_array_equal(a0, 0)
    np.testing.assert_array_equal(_words(st), fresh)
    got = [K.act(st, A, n_actions=n, uniform=True).cpu().numpy() for n in (4, 1, 4, 3, 1)]
    for e, rs in enumerate(refs):
        for i, n in enumerate((4, 1, 4, 3, 1)):
            np.testing.assert_array_equal(got[i][e], SR.np_uniform(rs, A, n)[0])
        np.testing.assert_array_equal(_words(st)[e], SR.np_state_words(rs))


def _fused_setup(rows, cols, seed0):
    A = rows * cols
    env = TrafficEnv(EnvConfig(rows=rows, cols=cols, num_envs=SR.FUSED_E, seed=21))
    obs = env.reset()
    ring = K.ReplayRing(SR.FUSED_E * A, 4)
    st = K.seed_streams(list(range(seed0, seed0 + SR.FUSED_E)), "np")
    return env, obs, ring, st


def test_env_step_refuses_one_action():
    """dmdqn_env_step does not take n_actions == 1 (include/dmdqn.h): EINVAL
    before any launch, the stream and the actions untouched."""
    env, obs, ring, st = _fused_setup(2, 2, 3)
    before = _words(st).copy()
    out = torch.full((SR.FUSED_E, 4), -1, dtype=torch.int32, device=DEV)
    g = torch.zeros((SR.FUSED_E, 4), dtype=torch.int32, device=DEV)
    for eps, greedy in ((1.0, None), (0.5, g)):
        with pytest.raises(RuntimeError, match=r"rc=-1\).*n_actions"):
            env.step_fused(st, eps, greedy, out, ring, obs, n_actions=1)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(_words(st), before)
    assert bool((out == -1).all()) and ring.total == 0
    # and the same call with two actions goes through
    env.step_fused(st, 0.5, g, out, ring, obs, n_actions=2)
    assert int(out.min()) >= 0 and int(out.max()) <= 1


# ---------------------------------------------------------------- the fused env step's act
@pytest.mark.parametrize("case", SR.FUSED_CASES, ids=str)
def test_fused_env_step_act_matches_numpy(case):
    """fused_act (sim.hip) against numpy directly, not against k_act: 1x1 the
    extra-LDS branch, 2x2 / 4x4 the LDS image, 5x5 / 8x8 the 512- and
    1024-thread register kernels."""
    rows, cols, n, seed0 = case
    A, E, steps = rows * cols, SR.FUSED_E, SR.fused_steps(rows * cols)
    acts, traces, states, greedy = _act_ref(A, SR.FUSED_EPS, n, seed0, E=E, calls=steps)
    SR.check_act_coverage(SR.act_coverage(traces), n)
    env, obs, ring, st = _fused_setup(rows, cols, seed0)
    g = torch.from_numpy(greedy).to(DEV)
    out = torch.full((steps, E, A), -1, dtype=torch.int32, device=DEV)
    for t in range(steps):
        nobs, _, done, _ = env.step_fused(st, SR.FUSED_EPS, g, out[t], ring, obs, n_actions=n)
        ring.advance()
        obs = env.reset() if done else nobs
    ring.check()
    np.testing.assert_array_equal(out.cpu().numpy(), acts)
    np.testing.assert_array_equal(_words(st), states)


# ---------------------------------------------------------------- seeding
PY_SEEDS = [2**32 - 1, 2**32, 2**32 + 5, 2**40 + 3, 2**63 - 1]  # one and two key words
NP_SEEDS = [0, 2**32 - 1]


@pytest.mark.parametrize("kind", ["np", "py"])
def test_seed_edges_state_and_draws(kind):
    seeds = NP_SEEDS if kind == "np" else PY_SEEDS
    st = K.seed_streams(seeds, kind)
    refs = [np.random.RandomState(s) if kind == "np" else random.Random(s) for s in seeds]
    words_of, u32 = ((SR.np_state_words, SR.np_u32) if kind == "np"
                     else (SR.py_state_words, SR.py_u32))
    np.testing.assert_array_equal(_words(st), np.stack([words_of(r) for r in refs]))
    for count in (1500, 700):  # continues the stream across twists
        got = K.draw_u32(st, count).cpu().numpy().view(np.uint32)
        for e, r in enumerate(refs):
            np.testing.assert_array_equal(got[e], u32(r, count))
        np.testing.assert_array_equal(_words(st), np.stack([words_of(r) for r in refs]))


@pytest.mark.parametrize("kind,bad", [("np", -1), ("py", -1), ("py", -2**40), ("np", 2**32),
                                      ("np", 2**32 + 5)])
def test_seed_streams_refuses_what_the_generators_refuse(kind, bad):
    with pytest.raises(ValueError):
        K.seed_streams([1, 2, bad], kind)
    with pytest.raises(ValueError):
        K.seed_streams(torch.tensor([bad, 1], dtype=torch.int64, device=DEV), kind)
    if kind == "np":
        with pytest.raises(ValueError):
            np.random.RandomState(bad)


# ---------------------------------------------------------------- ReplayBuffer.sample
def _sample_case(seeds, A, n, k, reps=2):
    st = K.seed_streams(seeds, "py")
    got = [K.replay_sample(st, A, n, k).cpu().numpy().reshape(len(seeds), A, k)
           for _ in range(reps)]
    words = _words(st)
    for e, s in enumerate(seeds):
        idx, state, _ = SR.run_sample_case(s, A, n, k, reps)
        for rep in range(reps):
            np.testing.assert_array_equal(got[rep][e], idx[rep])
        np.testing.assert_array_equal(words[e], state)


@pytest.mark.parametrize("A,n,k", SR.SAMPLE_SHAPES)
def test_replay_sample_leaves_cpythons_state(A, n, k):
    _sample_case([5, 6, 7], A, n, k)


@pytest.mark.parametrize("case", SR.SAMPLE_END_SET + SR.SAMPLE_END_POOL, ids=str)
def test_replay_sample_ending_at_a_block_end(case):
    """The last pick is word 623 of its block (the stored state stays that
    block with position 624, as CPython's) or word 0 of the next (position 1)."""
    seed, A, n, k, reps, pos = case
    idx, state, end = SR.run_sample_case(seed, A, n, k, reps)
    assert end == pos == int(state[SR.MT_N])
    _sample_case([seed], A, n, k, reps)


@pytest.mark.parametrize("tlog", [None, 3])
@pytest.mark.parametrize("A,n,k", SR.SAMPLE_DENSE)
def test_replay_sample_set_branch_a_third_full(A, n, k, tlog, lib_option):
    """Already-selected and in-chunk repeats in every chunk; with the
    first-lane table capped at 8 entries they also share slots."""
    assert n > SR.setsize(k)
    if tlog is not None:
        lib_option("sample_tlog", tlog)
    _sample_case([5, 6, 7], A, n, k)
