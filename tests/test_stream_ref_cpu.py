"""CPU: tests/stream_ref.py (the real numpy / CPython generators) agrees with
the C oracle wherever their domains overlap, and the fixed cases of
tests/test_gpu_stream_edges.py reach the edges they are there for -- on the
reference alone, before any kernel runs."""
import random

import numpy as np
import pytest

import oracle as O
import stream_ref as SR


# ---------------------------------------------------------------- helper == oracle
@pytest.mark.parametrize("eps", [1.0, 0.9, 0.5, 0.05, 0.0])
def test_np_act_equals_oracle_at_four_actions(eps):
    for seed in (3, 100, 2**31 - 1, 4000000000):
        rs, orc = np.random.RandomState(seed), O.np_stream(seed)
        greedy = SR.greedy_table(seed % 1000, 1, 16, 4)[0]
        for _ in range(30):  # 30 x 16 agents x 2-3 words: past two twists
            got, trace = SR.np_act(rs, 16, eps, 4, greedy)
            np.testing.assert_array_equal(got, O.act(orc, 16, eps, greedy))
            assert all(SR.words(b, a) == 2 for kind, b, a in trace if kind == "rand")
        np.testing.assert_array_equal(SR.np_state_words(rs), orc.state_array())


def test_np_uniform_equals_oracle_randint():
    for n in (4, 3, 2, 12):
        rs, orc = np.random.RandomState(9), O.np_stream(9)
        got, _ = SR.np_uniform(rs, 700, n)
        np.testing.assert_array_equal(got, [O.np_randint(orc, n) for _ in range(700)])
        np.testing.assert_array_equal(SR.np_state_words(rs), orc.state_array())


@pytest.mark.parametrize("n,k", [(128, 128), (129, 128), (500, 128), (1045, 128), (1046, 128),
                                 (3000, 128), (4200, 128), (21, 5), (22, 5), (7, 7),
                                 (3000, 1000), (4200, 1365)])
def test_py_sample_equals_oracle_in_both_branches(n, k):
    """n <= 4200 is the oracle's pool limit; 1045 / 1046 and 21 / 22 are the
    two sides of Random.sample's pool / set threshold for k = 128 and k = 5."""
    for seed in (0, 1, 12345):
        r, orc = random.Random(seed), O.py_stream(seed)
        for _ in range(5):
            np.testing.assert_array_equal(SR.py_sample(r, n, k), O.py_sample(orc, n, k))
        np.testing.assert_array_equal(SR.py_state_words(r), orc.state_array())


@pytest.mark.parametrize("seed", [0, 1, 42, 12345, 2**31 - 1, 4000000000, 2**32 - 1])
def test_raw_words_and_state_words_equal_oracle(seed):
    r, rs = random.Random(seed), np.random.RandomState(seed)
    op, on = O.py_stream(seed), O.np_stream(seed)
    # freshly seeded: the key and position 624
    np.testing.assert_array_equal(SR.py_state_words(r), op.state_array())
    np.testing.assert_array_equal(SR.np_state_words(rs), on.state_array())
    assert SR.py_pos(r) == SR.np_pos(rs) == SR.MT_N
    for count in (1500, 700):
        np.testing.assert_array_equal(SR.py_u32(r, count), O.u32(op, count))
        np.testing.assert_array_equal(SR.np_u32(rs, count), O.u32(on, count))
        np.testing.assert_array_equal(SR.py_state_words(r), op.state_array())
        np.testing.assert_array_equal(SR.np_state_words(rs), on.state_array())


# ---------------------------------------------------------------- what the generators do at the edges
def test_randint_of_one_action_draws_nothing():
    """np.random.randint(0, 1) is 0 and leaves the stream where it is: with one
    action select_action consumes rand()'s two words per agent, the uniform
    draw none."""
    rs = np.random.RandomState(11)
    rs.rand()
    before = SR.np_state_words(rs)
    assert rs.randint(0, 1) == 0
    np.testing.assert_array_equal(SR.np_state_words(rs), before)
    acts, trace = SR.np_act(rs, 5, 0.5, 1, np.zeros(5, np.int32))
    assert sum(SR.words(b, a) for _, b, a in trace) == 10 and not acts.any()
    acts, trace = SR.np_uniform(rs, 5, 1)
    assert sum(SR.words(b, a) for _, b, a in trace) == 0 and not acts.any()
    orc = O.np_stream(11)
    assert O.np_randint(orc, 1) == 0 and orc.mti == SR.MT_N


def test_generators_refuse_or_reinterpret_out_of_range_seeds():
    for bad in (-1, 2**32):
        with pytest.raises(ValueError):
            np.random.RandomState(bad)
    assert random.Random(-7).getstate() == random.Random(7).getstate()  # abs(seed)
    # two key words from 2**32 on: another stream than the low word alone
    assert random.Random(2**32 + 5).getstate() != random.Random(5).getstate()


@pytest.mark.parametrize("kind,bad", [("np", -1), ("py", -1), ("np", 2**32), ("np", 2**40 + 3),
                                      ("py", 2**63), ("py", -2**63)])
def test_seed_streams_refuses_before_any_launch(kind, bad):
    """kernels.seed_streams checks the host values first: no device is needed
    to be refused (the GPU test repeats it beside good seeds)."""
    from dmdqn_amd import kernels as K
    for seeds in ([bad], [3, bad, 4], np.array([3, bad], dtype=object)):
        with pytest.raises(ValueError):
            K.seed_streams(seeds, kind)
    with pytest.raises(ValueError):
        K.seed_streams([1], "numpy")


# ---------------------------------------------------------------- the case tables
def test_act_case_table_is_the_sweep_it_claims():
    by = lambda f: {c[:3] for c in SR.ACT_CASES if f(c)}  # noqa: E731
    assert {c[0] for c in by(lambda c: c[1] == 0.5 and c[2] == 4)} == {1, 7, 16, 64, 100, 209}
    assert {c[1] for c in by(lambda c: c[0] == 16 and c[2] == 4)} == {0.05, 0.5, 0.999}
    for A in (7, 64):
        assert {c[2] for c in by(lambda c: c[0] == A and c[1] == 0.5)} == {4, 2, 3, 5, 12}
    assert 3 * 209 > SR.MT_N  # never the fixed-count path
    assert {(r, c) for r, c, n, _ in SR.FUSED_CASES if n == 4} == {(1, 1), (2, 2), (4, 4), (5, 5),
                                                                   (8, 8)}
    assert [(r, c) for r, c, n, _ in SR.FUSED_CASES if n != 4] == [(2, 2)]


@pytest.mark.parametrize("case", SR.ACT_CASES, ids=str)
def test_act_cases_reach_their_edges(case):
    A, eps, n, seed0 = case
    acts, traces, states, greedy = SR.run_act_case(A, eps, n, seed0)
    assert acts.shape == (SR.act_calls(A), SR.ACT_E, A)
    assert acts.min() >= 0 and acts.max() < n and greedy.max() < n
    SR.check_act_coverage(SR.act_coverage(traces), n)


@pytest.mark.parametrize("case", SR.FUSED_CASES, ids=str)
def test_fused_cases_reach_their_edges(case):
    rows, cols, n, seed0 = case
    A = rows * cols
    assert n <= 4  # ACTION_MAP {a: 3a}: the signal program has phases 0, 3, 6, 9
    _, traces, _, _ = SR.run_act_case(A, SR.FUSED_EPS, n, seed0, E=SR.FUSED_E,
                                      calls=SR.fused_steps(A))
    SR.check_act_coverage(SR.act_coverage(traces), n)


def test_handover_case_alternates_both_paths():
    """eps = 1 calls whose 3 A words lie inside the block (the device's
    fixed-count path: only the position moves) before and after eps < 1 calls,
    and eps = 1 calls that cross a block end."""
    eps = SR.handover_eps()
    assert eps[:9] == [1, 1, 0.5, 1, 0.05, 1, 1, 0.999, 1] and len(eps) == 60
    A = SR.HANDOVER_A
    starts = []
    SR.run_act_case(A, eps, 4, SR.HANDOVER_SEED, calls=len(eps), starts=starts)
    inside = crossing = after_general = 0
    for start in starts:
        for c, e in enumerate(eps):
            if e == 1:
                fits = start[c] + 3 * A <= SR.MT_N
                inside += fits
                crossing += not fits
                after_general += fits and c > 0 and eps[c - 1] < 1
    assert inside >= 8 and crossing >= 8 and after_general >= 8


def test_sampler_block_end_cases_end_where_they_say():
    ends = {"set": set(), "pool": set()}
    for name, table in (("set", SR.SAMPLE_END_SET), ("pool", SR.SAMPLE_END_POOL)):
        for seed, A, n, k, reps, pos in table:
            assert k == 128 and SR.setsize(k) == 1045 and (n > 1045) == (name == "set")
            assert SR.run_sample_case(seed, A, n, k, reps)[2] == pos
            ends[name].add(pos)
    assert ends["set"] == {SR.MT_N, 1} and SR.MT_N in ends["pool"]
    assert all(n == 10000 for _, _, n, _, _, _ in SR.SAMPLE_END_SET)


def test_dense_sampler_cases_are_set_branch_and_a_third_full():
    assert SR.SAMPLE_DENSE == [(5, 1046, 341), (2, 4118, 1365)]
    for A, n, k in SR.SAMPLE_DENSE:
        assert n == SR.setsize(k) + 1 and 0.32 < k / n < 0.34
        got = SR.py_sample(random.Random(1), n, k)
        assert len(set(got.tolist())) == k and 0 <= got.min() and got.max() < n
