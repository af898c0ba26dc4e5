"""GPU: dmdqn_learn_pair (two consecutive learns of every agent in one launch,
k_learn_f16_x2 / k_learn_bf16_x2) against the same two learns as two
dmdqn_learn_hp launches, bit for bit.

The bit contract (include/dmdqn.h): per agent the pair runs the arithmetic of
the two launches in their order, the second learn reading what the first wrote
-- so every comparison is bit equality, and the reference is the existing
single-learn entry point, never the new one.  Both arms start from one snapshot
of the same agent and take the same two argument blocks.

Shapes: batch 128 and hidden 128 are fixed by the kernels; 1 env of 3 agents
(2 envs of 2 agents where the learning rate differs per replica), replay 160
filled past its wrap.  The two cases: both learns draw the same indices; the
ring window wraps between them (start = cap - 1, then 0)."""
import ctypes
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from dmdqn_amd import _lib  # noqa: E402
from dmdqn_amd.agent import AgentConfig, BatchedDQN, CHParams, CLearn  # noqa: E402

from test_gpu_learn import _fill  # noqa: E402

DEV = "cuda"
STATE = ("params", "adam_m", "adam_v", "target", "target_h")


def _bits(t):
    return t.view({4: torch.int32, 2: torch.int16}[t.element_size()])


@functools.lru_cache(maxsize=None)
def _agent(precision, tau, per_agent, loss):
    """A filled agent and the snapshot of its learnable state (shared by the
    tests of one configuration; every arm restores the snapshot first)."""
    sweep = dict(learning_rate=[1e-3, 2e-4]) if per_agent else None
    cfg = AgentConfig(precision=precision, nn_layers=[128, 128], replay_buffer_size=160,
                      target_update_frequency=1000, seed=5, learning_rate=7e-4, gamma=0.97,
                      tau=tau, loss=loss, sweep=sweep)
    E, A = (2, 2) if per_agent else (1, 3)
    ag = BatchedDQN(E, A, cfg)
    _fill(ag, 175, np.random.RandomState(2))  # past the wrap
    assert len(ag.ring) == 160 and ag.ring.start != 0
    assert ag.swept == per_agent
    ag.learn()  # Adam slots and target no longer at their initial values
    return ag, {n: getattr(ag, n).clone() for n in STATE}


def _restore(ag, snap):
    for n in STATE:
        getattr(ag, n).copy_(snap[n])


def _copy(args):
    return CLearn.from_buffer_copy(bytes(args))


def _two_learns(ag, case):
    """The argument blocks of two consecutive learns of `ag` (learn_begin
    twice: the Adam constants of steps t and t + 1, two loss / qstats buffers),
    each with its own index and z-score buffer; the tensors are returned with
    them (they own the memory the blocks point at)."""
    out = []
    for k in range(2):
        assert ag.learn_begin(collect_stats=True)
        a, hp = ag.c_learn_args(), ag.c_learn_hparams()
        idx = ag.idx.clone()
        rn = torch.zeros((ag.NA, 128), dtype=torch.float32, device=DEV)
        a.idx, a.rn_out = idx.data_ptr(), rn.data_ptr()
        assert not a.sync_target
        out.append(dict(args=a, hp=hp, idx=idx, rn=rn, loss=ag.loss, qstats=ag.qstats))
    l0, l1 = out
    assert l0["loss"].data_ptr() != l1["loss"].data_ptr()
    assert l0["qstats"].data_ptr() != l1["qstats"].data_ptr()
    assert l0["args"].alpha != l1["args"].alpha
    if case == "same_idx":
        l1["idx"].copy_(l0["idx"])
    else:  # the window wraps between the two learns
        l0["args"].start, l1["args"].start = l0["args"].cap - 1, 0
    return l0, l1


def _run(ag, snap, l0, l1, pair):
    _restore(ag, snap)
    for l in (l0, l1):
        l["loss"].fill_(-1.0)
        l["qstats"].zero_()
        l["rn"].zero_()
    hp = [ctypes.byref(l["hp"]) if ag.swept else None for l in (l0, l1)]
    s = _lib.stream_of()
    if pair:
        _lib.call("dmdqn_learn_pair", ctypes.byref(l0["args"]), ctypes.byref(l1["args"]), hp[0],
                  hp[1], s)
    else:
        _lib.call("dmdqn_learn_hp", ctypes.byref(l0["args"]), hp[0], s)
        _lib.call("dmdqn_learn_hp", ctypes.byref(l1["args"]), hp[1], s)
    torch.cuda.synchronize()
    got = {n: getattr(ag, n).clone() for n in STATE}
    for k, l in enumerate((l0, l1)):
        for n in ("loss", "qstats", "rn"):
            got[f"{n}{k}"] = l[n].clone()
    return got


@pytest.mark.parametrize("case", ["same_idx", "wrap"])
@pytest.mark.parametrize("loss", ["mse", "huber"])
@pytest.mark.parametrize("per_agent", [False, True], ids=["scalar", "per_agent_lr"])
@pytest.mark.parametrize("tau", [0.0, 0.01])
@pytest.mark.parametrize("precision", ["fp16", "bf16"])
def test_pair_equals_two_single_learns(precision, tau, per_agent, loss, case, lib_option):
    lib_option("soft_path", "fused")
    ag, snap = _agent(precision, tau, per_agent, loss)
    _restore(ag, snap)
    l0, l1 = _two_learns(ag, case)
    want = _run(ag, snap, l0, l1, pair=False)
    got = _run(ag, snap, l0, l1, pair=True)
    for n in want:
        x, y = _bits(got[n]), _bits(want[n])
        assert torch.equal(x, y), f"{n}: {int((x != y).sum())} of {x.numel()} differ"
    # not vacuous: both learns ran, the second one on the first one's result
    assert not torch.equal(want["params"], snap["params"])
    assert (want["loss0"] >= 0).all() and (want["loss1"] >= 0).all()
    assert not torch.equal(want["loss0"], want["loss1"])
    assert (want["qstats0"][:, 2:].sum(1) == 128).all() and (want["qstats1"][:, 2:].sum(1) == 128).all()
    assert torch.equal(want["target"], snap["target"]) == (tau == 0.0)
    if case == "same_idx":
        assert torch.equal(want["rn0"], want["rn1"]) and want["rn0"].abs().sum() > 0
    else:
        assert not torch.equal(want["rn0"], want["rn1"])


def _refused(ag, snap, a0, a1, match):
    lib = _lib.load()
    _restore(ag, snap)
    rc = lib.dmdqn_learn_pair(ctypes.byref(a0), ctypes.byref(a1), None, None, _lib.stream_of())
    assert rc == -1, rc
    assert match in lib.dmdqn_last_error().decode(), lib.dmdqn_last_error()
    torch.cuda.synchronize()
    for n in STATE:  # nothing was launched
        assert torch.equal(_bits(getattr(ag, n)), _bits(snap[n])), n


def test_pair_argument_checks_return_the_error_code_and_launch_nothing():
    ag, snap = _agent("fp16", 0.0, False, "mse")
    _restore(ag, snap)
    l0, l1 = _two_learns(ag, "same_idx")
    a0, a1 = l0["args"], l1["args"]
    bad = _copy(a1)
    bad.sync_target = 1
    _refused(ag, snap, a0, bad, "sync_target")
    _refused(ag, snap, bad, a1, "sync_target")
    rows = torch.zeros((ag.NA, 128, 96), dtype=torch.float32, device=DEV)
    bad = _copy(a0)
    bad.row_format, bad.xs, bad.xn = 1, rows.data_ptr(), rows.data_ptr()
    _refused(ag, snap, bad, a1, "int8 replay rows")
    other = ag.params.clone()
    bad = _copy(a1)
    bad.params = other.data_ptr()
    _refused(ag, snap, a0, bad, "share")
    bad = _copy(a1)
    bad.target_h = None
    _refused(ag, snap, a0, bad, "share")
    a0n, a1n = _copy(a0), _copy(a1)
    a0n.target_h = a1n.target_h = None
    _refused(ag, snap, a0n, a1n, "target_h")
    bad = _copy(a1)
    bad.tau, bad.one_minus_tau = 0.5, 0.5
    _refused(ag, snap, a0, bad, "soft target update")
    # and the blocks themselves are good
    _restore(ag, snap)
    _lib.call("dmdqn_learn_pair", ctypes.byref(a0), ctypes.byref(a1), None, None, _lib.stream_of())
    torch.cuda.synchronize()
    assert not torch.equal(ag.params, snap["params"])


def test_pair_operator_equals_the_c_abi(lib_option):
    """torch.ops.dmdqn.learn_pair passes what the C entry point takes."""
    from dmdqn_amd.agent import LOSSES, PRECISIONS, soft_update_consts
    from dmdqn_amd.ops import load as load_ops
    lib_option("soft_path", "fused")
    ag, snap = _agent("fp16", 0.01, True, "mse")
    _restore(ag, snap)
    l0, l1 = _two_learns(ag, "wrap")
    want = _run(ag, snap, l0, l1, pair=True)
    _restore(ag, snap)
    for l in (l0, l1):
        l["loss"].fill_(-1.0)
        l["qstats"].zero_()
        l["rn"].zero_()
    a0, a1, ring, cfg = l0["args"], l1["args"], ag.ring, ag.cfg
    tau_f, omt_f = soft_update_consts(cfg.tau)
    load_ops().learn_pair(
        ring.s, ring.n, ring.a, ring.d, ring.r, ag.params, ag.adam_m, ag.adam_v, ag.target,
        ag.target_h, l0["idx"], l1["idx"], l0["loss"], l1["loss"], a0.start, a1.start, ag.H,
        PRECISIONS[cfg.precision], ag.gamma_n, [a0.alpha, a0.c1, a0.c2, a0.eps],
        [a1.alpha, a1.c1, a1.c2, a1.eps], LOSSES[cfg.loss], qstats0=l0["qstats"],
        qstats1=l1["qstats"], rn_out0=l0["rn"], rn_out1=l1["rn"], tau=float(tau_f),
        one_minus_tau=float(omt_f), lr=ag.hp_lr, gamma_a=ag.hp_gamma, tau_a=ag.hp_tau,
        one_minus_tau_a=ag.hp_omt, factors0=[l0["hp"].adam_s, l0["hp"].adam_d],
        factors1=[l1["hp"].adam_s, l1["hp"].adam_d])
    torch.cuda.synchronize()
    for n in STATE:
        assert torch.equal(_bits(getattr(ag, n)), _bits(want[n])), n
    for k, l in enumerate((l0, l1)):
        for n in ("loss", "qstats", "rn"):
            assert torch.equal(_bits(l[n]), _bits(want[f"{n}{k}"])), f"{n}{k}"


# ------------------------------------------------------------------ the trainer
# Schedule "env" with its learns in pairs against the one-stream order, bit for
# bit: 2 x 2 grid x 2 envs, replay 160 (wrapped: learns start at step 128, the
# deque is full from step 160), target_update_frequency 7 so that hard syncs --
# single launches, like the learn before each -- fall on both positions of a
# pair.  The paired run's losses are read one step late, from the learn's own
# buffer (Trainer.last_loss would have a held-back learn launched at once, and
# nothing would ever pair).
from dmdqn_amd import checkpoint as CK  # noqa: E402
from dmdqn_amd.env import EnvConfig  # noqa: E402
from dmdqn_amd.trainer import Trainer  # noqa: E402

FILL = 127  # steps before the first learn (batch 128)
END_STATE = ("params", "adam_m", "adam_v", "target", "target_h", "np_state", "py_state")


def _trainer(overlap, spare=16, precision="fp16", **kw):
    return Trainer(EnvConfig(rows=2, cols=2, num_envs=2, seed=6, max_sim_time=500),
                   AgentConfig(replay_buffer_size=160, target_update_frequency=7, seed=4,
                               precision=precision, ring_spare=spare), overlap=overlap, **kw)


def _steps(tr, n, stats_every=0, lazy=False, out=None):
    """n steps; per step (loss, obs, actions, qstats or None).  lazy: the loss
    and metrics of step t are cloned after step t + 1 from the buffers of that
    learn (complete then: its launch is queued on this stream by then)."""
    out = [] if out is None else out
    held = None
    for t in range(n):
        stats = bool(stats_every) and t % stats_every == 0
        learned = tr.step(collect_stats=stats).loss_launched
        if held is not None:
            i, loss, q = held
            out[i][0] = loss.clone()
            out[i][3] = None if q is None else q.clone()
            held = None
        rec = [None, tr.obs.clone(), tr.agent.actions.clone(), None]
        out.append(rec)
        if learned and lazy:
            held = (len(out) - 1, tr.agent.loss, tr.agent.qstats if stats else None)
        elif learned:
            rec[0] = tr.last_loss.clone()
            rec[3] = tr.agent.qstats.clone() if stats else None
    if held is not None:
        tr.sync_outputs()
        i, loss, q = held
        out[i][0] = loss.clone()
        out[i][3] = None if q is None else q.clone()
    return out


def _same_run(a, b):
    assert len(a) == len(b)
    for t, (x, y) in enumerate(zip(a, b)):
        for k, name in enumerate(("loss", "obs", "actions", "qstats")):
            assert (x[k] is None) == (y[k] is None), (t, name)
            if x[k] is not None:
                assert torch.equal(_bits(x[k]) if x[k].is_floating_point() else x[k],
                                   _bits(y[k]) if y[k].is_floating_point() else y[k]), (t, name)


def _same_end(ref, tr):
    tr.synchronize()
    ref.synchronize()
    for n in END_STATE:
        x, y = getattr(ref.agent, n), getattr(tr.agent, n)
        assert torch.equal(_bits(x) if x.is_floating_point() else x,
                           _bits(y) if y.is_floating_point() else y), n
    for n in ("s", "n", "a", "r", "d"):
        assert torch.equal(getattr(ref.agent.ring, n), getattr(tr.agent.ring, n)), f"ring.{n}"
    assert ref.agent.ring.total == tr.agent.ring.total
    assert ref.agent.learn_step_counter == tr.agent.learn_step_counter


@pytest.mark.parametrize("precision", ["fp16", "bf16"])
@pytest.mark.parametrize("spare", [2, 3, 16])
def test_paired_env_schedule_matches_sequential(spare, precision):
    steps = 360  # 200 past the wrap
    ref, tr = _trainer("none", spare, precision), _trainer("env", spare, precision)
    a, b = _steps(ref, steps), _steps(tr, steps, lazy=True)
    _same_run(a, b)
    _same_end(ref, tr)
    learns = steps - FILL
    assert tr.agent.learn_launches == ref.agent.learn_launches == learns
    # learn n is a hard sync when n % 7 == 0 and runs single: of every seven
    # learns 7m + 1 .. 7m + 6 make three pairs (learn 7m + 6 is a pair's second;
    # as a first it would run single), and so do the learns after the last sync
    assert tr.agent.pair_launches == learns // 7 * 3 + learns % 7 // 2
    assert ref.agent.pair_launches == 0
    assert tr.n_marks > 0 and tr._pending is None


def test_pairing_can_be_switched_off():
    ref, tr = _trainer("none"), _trainer("env", pair_learns=False)
    _same_run(_steps(ref, 200), _steps(tr, 200, lazy=True))
    _same_end(ref, tr)
    assert tr.agent.pair_launches == 0 and tr.agent.learn_launches == 200 - FILL


def test_synchronize_launches_a_held_back_learn():
    """An odd number of learns: the last one was begun and held back; whatever
    hands state to the caller launches it (synchronize here; last_loss,
    sync_outputs, quiesce, join_streams and a checkpoint go through the same)."""
    ref, tr = _trainer("none"), _trainer("env")
    for _ in range(FILL + 1):
        ref.step()
        tr.step()
    while tr._pending is None:  # stop on a call that held its learn back
        ref.step()
        tr.step()
    assert tr.agent.learn_launches == ref.agent.learn_launches
    tr.synchronize()
    assert tr._pending is None
    _same_end(ref, tr)
    # and the loss of that learn is in its buffer
    assert torch.equal(_bits(tr.last_loss), _bits(ref.last_loss))


def test_last_loss_read_under_another_stream(monkeypatch):
    """last_loss (and sync_outputs, quiesce, ...) under a stream that is not the
    step's: the held-back learn is launched on the learn stream -- behind the
    wait for its env step, before the next pair, in front of its mark -- and
    the reading stream waits for it.  Every third step is read that way, so
    pairs and lone launches mix; bit-identical to the one-stream order."""
    ref, tr = _trainer("none", spare=2), _trainer("env", spare=2)
    main, other = torch.cuda.current_stream(), torch.cuda.Stream()
    streams = []
    real = tr.agent.learn_range

    def spy(lo, hi, tok=None):
        streams.append(torch.cuda.current_stream())
        return real(lo, hi, tok)
    monkeypatch.setattr(tr.agent, "learn_range", spy)
    got, want, flushed = [], [], 0
    for t in range(330):
        ref.step()
        tr.step()
        if t >= FILL and t % 3 == 0:
            flushed += tr._pending is not None
            with torch.cuda.stream(other):
                loss = tr.last_loss
                got.append(loss.clone())
                loss.record_stream(other)
            assert tr._pending is None
            want.append(ref.last_loss.clone())
    assert flushed > 10 and tr.agent.pair_launches > 10
    assert streams and all(s == main for s in streams)
    other.synchronize()
    for t, (x, y) in enumerate(zip(got, want)):
        assert torch.equal(_bits(x), _bits(y)), t
    _same_end(ref, tr)


def test_paired_env_schedule_with_metrics_every_fifth_step():
    ref, tr = _trainer("none"), _trainer("env")
    a, b = _steps(ref, 260, stats_every=5), _steps(tr, 260, stats_every=5, lazy=True)
    assert sum(r[3] is not None for r in a) >= 20
    _same_run(a, b)
    _same_end(ref, tr)
    assert 0 < tr.agent.pair_launches < (260 - FILL) // 2  # metrics steps run single


def test_save_and_resume_across_a_held_back_learn(tmp_path):
    ref, tr = _trainer("none"), _trainer("env")
    a = _steps(ref, 230)
    b = _steps(tr, 170, lazy=False)  # (last_loss: every learn launched)
    while tr._pending is None:  # run on to a call that holds its learn back
        tr.step()
        b.append([None, tr.obs.clone(), tr.agent.actions.clone(), None])
    n = len(b)
    path = str(tmp_path / "ck.pt")
    CK.save(path, tr)  # launches the held-back learn first
    assert tr._pending is None
    tr2 = _trainer("env")
    CK.load(path, tr2)
    c = _steps(tr2, 230 - n, lazy=True)
    for t in range(n, 230):
        for k in (0, 1, 2):
            assert torch.equal(a[t][k], c[t - n][k]), (t, k)
    _same_end(ref, tr2)
    assert tr2.agent.pair_launches > 0
