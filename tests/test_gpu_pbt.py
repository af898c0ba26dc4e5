"""GPU: population-based training (AgentConfig.pbt; dmdqn_pbt_score / _select /
_exchange) against the pure-Python restatement of the contract
(tests/pbt_ref.py) and code that existed before it, bit for bit: the three
kernels through the operators and the C ABI, a Trainer whose rounds are redone
on a Trainer without pbt by torch indexing and the restated formulas, the
schedules, and checkpoint / resume.

The trainer runs take STEPS = 210 steps at interval 40: the learn kernels are
built for batches of 128, so the first learn comes at step 128 (130 with
n_step 3) and the windows that end at steps 40, 80 and 120 must NOT run a
round (learn_step_counter is still 0; their fitness is dropped); the rounds at
steps 160 and 200 are the two that fall after learning starts.  The checkpoint
is saved at step 175: after the first round, in the middle of a window."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import pbt_ref as PR  # noqa: E402
from dmdqn_amd import _lib, checkpoint as CK  # noqa: E402
from dmdqn_amd.agent import AgentConfig  # noqa: E402
from dmdqn_amd.env import EnvConfig  # noqa: E402
from dmdqn_amd.ops import load as ops  # noqa: E402
from dmdqn_amd.trainer import Trainer  # noqa: E402

DEV = "cuda"


def _bits(t):
    """A device f64 / f32 / 16-bit tensor as a host integer array (bits, not
    values: -0.0 and NaN payloads count)."""
    view = {8: torch.int64, 4: torch.int32, 2: torch.int16}[t.element_size()]
    return t.contiguous().view(view).cpu().numpy()


def _f64_bits(values):
    return np.asarray(values, dtype=np.float64).view(np.int64)


# --------------------------------------------------------------------------- score
def _score_both(reward, fitness):
    """One dmdqn_pbt_score through the operator and one through ctypes, each on
    its own copy of fitness; the two must agree.  Returns the new fitness."""
    f_op, f_c = fitness.clone(), fitness.clone()
    ops().pbt_score(reward, f_op)
    E, A = reward.shape
    _lib.call("dmdqn_pbt_score", _lib.ptr(reward), E, A, _lib.ptr(f_c), _lib.stream_of())
    torch.cuda.synchronize()
    assert np.array_equal(_bits(f_op), _bits(f_c))
    return f_op


def test_score_adds_in_junction_order_and_accumulates():
    rng = np.random.default_rng(3)
    r1 = np.array([[1e16, 1.0, -1e16], [1.0, 1e16, -1e16], [-1e16, 1e16, 1.0],
                   [0.1, 0.2, 0.3], [-0.0, -0.0, -0.0]])
    r2 = rng.normal(scale=50.0, size=(5, 3))
    r2[0] = [1.0, -1e16, 1e16]
    # (the order matters: a sum in another order gives other bits)
    assert PR.score([0.0] * 3, r1[:3].tolist()) == [0.0, 0.0, 1.0]
    assert (0.1 + 0.2) + 0.3 != 0.1 + (0.2 + 0.3)
    fit = torch.zeros(5, dtype=torch.float64, device=DEV)
    want = [0.0] * 5
    for r in (r1, r2, r1):
        fit = _score_both(torch.from_numpy(r).to(DEV), fit)
        want = PR.score(want, r.tolist())
        assert np.array_equal(_bits(fit), _f64_bits(want))
    # one junction: the reward itself
    r = rng.normal(size=(5, 1))
    fit = _score_both(torch.from_numpy(r).to(DEV), fit)
    assert np.array_equal(_bits(fit), _f64_bits(PR.score(want, r.tolist())))


# --------------------------------------------------------------------------- select
@pytest.mark.parametrize("E", [2, 5, 8, 67, 130])
def test_select_is_the_restatement(E):
    for name, f in PR.fitness_vectors(E).items():
        fit = torch.from_numpy(f).to(DEV)
        for n in sorted({1, E // 2}):
            out = []
            for how in ("op", "ctypes"):
                rank = torch.full((E,), -1, dtype=torch.int32, device=DEV)
                src = torch.full((E,), -1, dtype=torch.int32, device=DEV)
                if how == "op":
                    ops().pbt_select(fit, n, rank, src)
                else:
                    _lib.call("dmdqn_pbt_select", _lib.ptr(fit), E, n, _lib.ptr(rank),
                              _lib.ptr(src), _lib.stream_of())
                out.append((src.cpu().tolist(), rank.cpu().tolist()))
            assert out[0] == out[1], (name, n)
            src, rank = out[0]
            want_src, want_rank = PR.select(f.tolist(), n)
            assert sorted(rank) == list(range(E)), (name, n, "rank is a permutation")
            assert rank == want_rank, (name, n)
            assert src == want_src, (name, n)


# --------------------------------------------------------------------------- exchange
EX_E, EX_A = 5, 3
EX_SRC = [0, 1, 0, 3, 1]


def _guarded(rng, rows, width, dtype):
    """[rows + 2, width] random bit patterns (NaN payloads included): row 0 and
    the last row are the guards around the rows a kernel may write."""
    info = np.iinfo(dtype)
    a = rng.integers(info.min, int(info.max) + 1, size=(rows + 2, width), dtype=np.int64)
    return torch.from_numpy(a.astype(dtype)).to(DEV)


def _exchange(how, src, f32, h16):
    """dmdqn_pbt_exchange on the inner rows of the guarded tensors."""
    inner = [t[1:-1].view(torch.float32) for t in f32]
    th = None if h16 is None else h16[1:-1].view(torch.float16)
    for t in inner + ([] if th is None else [th]):
        assert t.is_contiguous() and t.data_ptr() % 16 == 0
    s = torch.tensor(src, dtype=torch.int32, device=DEV)
    if how == "op":
        ops().pbt_exchange(s, EX_A, *inner, th)
    else:
        Ph = 0 if th is None else th.shape[1]
        _lib.call("dmdqn_pbt_exchange", _lib.ptr(s), EX_E, EX_A, inner[0].shape[1], Ph,
                  *[_lib.ptr(t) for t in inner], _lib.ptr(th), _lib.stream_of())
    torch.cuda.synchronize()


@pytest.mark.parametrize("with_h", [True, False], ids=["target_h", "no_target_h"])
@pytest.mark.parametrize("P,Ph", [(28548, 28552), (10180, 10184)])
def test_exchange_copies_rows_as_bits_and_nothing_else(P, Ph, with_h):
    rng = np.random.default_rng(P + with_h)
    NA = EX_E * EX_A
    before_f = [_guarded(rng, NA, P, np.int32) for _ in range(4)]
    before_h = _guarded(rng, NA, Ph, np.int16)
    assert bool(torch.isnan(before_f[0].view(torch.float32)).any())  # NaN payloads are in there
    want_f = [t.clone() for t in before_f]
    want_h = before_h.clone()
    for e, s in enumerate(EX_SRC):
        if s != e:
            dst, frm = slice(1 + e * EX_A, 1 + (e + 1) * EX_A), slice(1 + s * EX_A, 1 + (s + 1) * EX_A)
            for w, b in zip(want_f, before_f):
                w[dst] = b[frm]
            if with_h:
                want_h[dst] = before_h[frm]
    results = []
    for how in ("op", "ctypes"):
        f32 = [t.clone() for t in before_f]
        h16 = before_h.clone()
        _exchange(how, EX_SRC, f32, h16 if with_h else None)
        for name, got, want in zip(["params", "target", "adam_m", "adam_v"], f32, want_f):
            assert torch.equal(got[0], want[0]) and torch.equal(got[-1], want[-1]), (how, name, "guard")
            assert torch.equal(got, want), (how, name)
        assert torch.equal(h16, want_h), (how, "target_h")  # (not passed: untouched)
        results.append(f32 + [h16])
    # an identity src writes nothing
    f32 = [t.clone() for t in before_f]
    h16 = before_h.clone()
    _exchange("op", list(range(EX_E)), f32, h16 if with_h else None)
    assert all(torch.equal(g, b) for g, b in zip(f32 + [h16], before_f + [before_h]))


# --------------------------------------------------------------------------- trainer
STEPS, CKPT_AT, INTERVAL, E, N = 210, 175, 40, 8, 2
PERTURB = {"learning_rate": [0.8, 1.25], "gamma": [0.99, 1.005]}
BOUNDS = {"learning_rate": [1e-6, 1e-1], "gamma": [0.5, 0.9999], "tau": [1e-4, 1.0]}  # the defaults
SEED = 5
PBT = {"interval": INTERVAL, "truncation": 0.25, "perturb": PERTURB, "seed": SEED}
LRS = [3e-4, 1e-3]
ROUND_STEPS = [160, 200]
NETS = ["params", "target", "adam_m", "adam_v", "target_h"]
HPS = ["hp_lr", "hp_gamma", "nstep_gamma_a", "hp_tau", "hp_omt"]


def _trainer(precision="fp16", n_step=3, pbt=PBT, **kw):
    sweep = {"learning_rate": LRS}
    if pbt is None:
        sweep["gamma"] = [0.99]  # the reference: a one-value sweep, so the array exists
    return Trainer(EnvConfig(rows=2, cols=2, num_envs=E, seed=11, max_sim_time=500),
                   AgentConfig(replay_buffer_size=300, target_update_frequency=5, seed=4,
                               precision=precision, n_step=n_step, sweep=sweep, pbt=pbt), **kw)


def _step(tr, log):
    tr.step()
    log.append((None if tr.last_loss is None else tr.last_loss.clone(), tr.obs.clone(),
                tr.last_reward.clone()))


def _run(tr, steps, log=None):
    log = [] if log is None else log
    for _ in range(steps):
        _step(tr, log)
    torch.cuda.synchronize()
    return log


def _run_redone_by_hand(precision, n_step):
    """The Trainer WITHOUT pbt; at the end of every window the round is redone
    here: fitness from the recorded rewards and the selection by the
    restatement, the rows copied with torch indexing, the per-agent arrays
    assigned from the restated formulas."""
    tr = _trainer(precision, n_step, pbt=None)
    ag = tr.agent
    A = ag.A
    values = {"learning_rate": [LRS[e % 2] for e in range(E)], "gamma": [0.99] * E}
    fitness, rounds, log = [0.0] * E, [], []
    for t in range(1, STEPS + 1):
        _step(tr, log)
        fitness = PR.score(fitness, tr.last_reward.cpu().tolist())
        if t % INTERVAL:
            continue
        if ag.learn_step_counter > 0:
            src, _ = PR.select(fitness, N)
            dst_rows = [e * A + j for e, s in enumerate(src) if s != e for j in range(A)]
            src_rows = [s * A + j for e, s in enumerate(src) if s != e for j in range(A)]
            for name in NETS:
                rows = getattr(ag, name)
                if rows is not None:
                    rows[dst_rows] = rows[src_rows]
            values = PR.explore(values, src, PERTURB, BOUNDS, SEED, len(rounds), 0)
            for name, arr in PR.device_arrays(values, n_step, A).items():
                if getattr(ag, name) is not None:
                    getattr(ag, name).copy_(torch.from_numpy(arr))
            rounds.append({"round": len(rounds), "step": t, "copied": PR.pairs(src)})
        fitness = [0.0] * E
    torch.cuda.synchronize()
    return tr, log, rounds, values


_PBT_RUNS = {}


def _pbt_run(precision, n_step, tmp=None):
    """The Trainer with pbt under the one-stream schedule (cached per config;
    with tmp it also leaves a checkpoint at step CKPT_AT)."""
    key = (precision, n_step)
    if key not in _PBT_RUNS:
        tr = _trainer(precision, n_step)
        log, probes = [], {}
        for t in range(1, STEPS + 1):
            _step(tr, log)
            if t in (INTERVAL, INTERVAL + 1):
                probes[t] = tr.agent.fitness.clone()
            if t == CKPT_AT and tmp is not None:
                CK.save(str(tmp / "mid.pt"), tr)
        torch.cuda.synchronize()
        _PBT_RUNS[key] = (tr, log, probes)
    return _PBT_RUNS[key]


@pytest.fixture(scope="module")
def main_run(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("pbt")
    return _pbt_run("fp16", 3, tmp) + (str(tmp / "mid.pt"),)


def _same_nets(a, b, what, names=NETS + HPS):
    for name in names:
        x, y = getattr(a, name), getattr(b, name)
        assert (x is None) == (y is None), (what, name)
        if x is not None:
            assert np.array_equal(_bits(x), _bits(y)), f"{what}: {name} differs"


def _same_logs(la, lb, what):
    assert len(la) == len(lb)
    for t, (x, y) in enumerate(zip(la, lb)):
        assert (x[0] is None) == (y[0] is None), (what, t)
        for i, name in enumerate(["loss", "obs", "reward"]):
            if x[i] is not None:
                assert np.array_equal(_bits(x[i]), _bits(y[i])), f"{what}: {name} differs at step {t + 1}"


@pytest.mark.parametrize("precision,n_step", [("fp16", 3), ("fp16", 1), ("fp32", 1)])
def test_trainer_rounds_are_the_restatement(main_run, precision, n_step):
    tr, log, probes = _pbt_run(precision, n_step)
    ref, ref_log, rounds, values = _run_redone_by_hand(precision, n_step)
    ag = tr.agent
    assert (ag.target_h is None) == (precision == "fp32")
    assert (ag.nstep_gamma_a is None) == (n_step == 1) and ag.hp_tau is None
    # the windows that ended before the first learn ran no round, and their
    # fitness was dropped: after step 41 it holds that step's reward alone
    first_learn = [x[0] is not None for x in log].index(True) + 1
    assert first_learn == 127 + n_step > 3 * INTERVAL
    assert not probes[INTERVAL].any()
    assert np.array_equal(_bits(probes[INTERVAL + 1]),
                          _f64_bits(PR.score([0.0] * E, log[INTERVAL][2].cpu().tolist())))
    # two rounds, the restatement's pairs, two clones each
    assert [r["step"] for r in rounds] == ROUND_STEPS and ag.pbt_round == 2
    assert [{k: r[k] for k in ("round", "step", "copied")} for r in tr.pbt_log] == rounds
    assert all(len(r["copied"]) == N for r in rounds)
    for r in tr.pbt_log:
        assert r["fitness_best"] >= r["fitness_median"] >= r["fitness_worst"]
        assert r["best_env"] not in [d for d, _ in r["copied"]]
    assert {k: v.tolist() for k, v in ag.pbt_values.items()} == values
    assert tr.pbt_log[-1]["values"] == {k: [float(np.min(v)), float(np.median(v)), float(np.max(v))]
                                        for k, v in values.items()}
    # the clones' values moved off the sweep's two
    assert len(set(values["learning_rate"])) > 2 and len(set(values["gamma"])) > 1
    _same_logs(log, ref_log, "pbt vs redone by hand")
    _same_nets(ag, ref.agent, "pbt vs redone by hand")
    with pytest.raises(ValueError, match="by_variant"):
        ag.learn_metrics(by_variant=True)


def test_agent_refuses_a_source_that_is_overwritten(main_run):
    ag = main_run[0].agent
    before = ag.params.clone()
    for bad in ([1, 2, 2, 3, 4, 5, 6, 7], [0, 1, 2, 3, 4, 5, 6, 8], [0, 1, 2]):
        with pytest.raises(ValueError, match="src"):
            ag.pbt_exchange(bad)
    assert torch.equal(ag.params, before)


@pytest.mark.parametrize("other", ["env", "env+side"])
def test_trainer_schedules_are_bit_identical(main_run, other):
    ref, log = main_run[0], main_run[1]
    tr = _trainer(overlap="env", side_learn=6 if other == "env+side" else 0)
    log2 = _run(tr, STEPS)
    assert tr.side is not None and ref.side is None
    _same_logs(log, log2, other)
    tr.sync_outputs()
    _same_nets(ref.agent, tr.agent, other, NETS + HPS + ["fitness", "np_state", "py_state"])
    assert tr.pbt_log == ref.pbt_log and len(tr.pbt_log) == 2


def test_trainer_refuses_the_other_schedules():
    for overlap in ("sample", "learn", "full"):
        with pytest.raises(ValueError, match="pbt"):
            _trainer(n_step=1, overlap=overlap)


def test_checkpoint_resumes_mid_window(main_run):
    ref, log, _, path = main_run
    st = torch.load(path, map_location="cpu", weights_only=True)
    assert st["format"] == "dmdqn-ckpt-8" and st["pbt"]["round"] == 1
    assert [r["step"] for r in st["pbt"]["log"]] == ROUND_STEPS[:1] and CKPT_AT % INTERVAL
    assert sorted(st["pbt"]["values"]) == ["gamma", "learning_rate"]
    tr = _trainer()
    CK.load(path, tr)
    assert tr.agent.pbt_round == 1 and tr.pbt_log == ref.pbt_log[:1]
    assert np.array_equal(_bits(tr.agent.fitness), _bits(st["pbt"]["fitness"].to(DEV)))
    log2 = _run(tr, STEPS - CKPT_AT)
    _same_logs(log[CKPT_AT:], log2, "resumed")
    _same_nets(ref.agent, tr.agent, "resumed", NETS + HPS + ["fitness"])
    assert tr.pbt_log == ref.pbt_log
    assert {k: v.tolist() for k, v in tr.agent.pbt_values.items()} == {
        k: v.tolist() for k, v in ref.agent.pbt_values.items()}
    # a resume under another pbt dict, or without one, is refused
    for other in (dict(PBT, seed=SEED + 1), dict(PBT, interval=INTERVAL + 1)):
        with pytest.raises(ValueError, match="pbt"):
            CK.load(path, _trainer(pbt=other))
    with pytest.raises(ValueError, match="pbt|sweep"):
        CK.load(path, _trainer(pbt=None))
