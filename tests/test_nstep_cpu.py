"""n-step returns, the parts that need no GPU: the restatement of the contract
(tests/nstep_ref.py) against the textbook n-step buffer, the config and CLI
refusals, the bootstrap discount, the host-side refusals of
dmdqn_replay_nstep_commit and the checkpoint's configuration keys."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import nstep_ref as NR

NS = (1, 2, 3, 5, 8)
CORNERS = {
    "no done": [0] * 40,
    "done at step 0": [1] + [0] * 30,
    "consecutive dones": [0, 0, 1, 1, 1, 0, 0, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0],
    "two dones inside one window": [0, 0, 0, 1, 0, 1, 0, 0, 0, 0, 0, 0, 1, 0, 0, 1, 0, 0, 0, 0],
    "done at the last store": [0] * 19 + [1],
    "every step done": [1] * 12,
}


def _raw(dones, rng):
    """Raw transitions with scalar stand-ins for the observations: s = k,
    s2 = k + 0.5, so a commit names the entries it was built from."""
    return [(float(k), int(rng.integers(0, 4)), float(rng.normal()), k + 0.5, int(d))
            for k, d in enumerate(dones)]


def _patterns():
    rng = np.random.default_rng(7)
    pats = list(CORNERS.values())
    while len(pats) < 200:
        L = int(rng.integers(1, 50))
        p = float(rng.choice([0.0, 0.05, 0.2, 0.6]))
        pats.append((rng.random(L) < p).astype(int).tolist())
    return pats


def test_restatement_is_the_textbook_buffer_with_a_fixed_delay():
    rng = np.random.default_rng(11)
    pats = _patterns()
    assert len(pats) == 200 and any(not any(p) for p in pats)
    emitted = 0
    for dones in pats:
        raw = _raw(dones, rng)
        for n in NS:
            got = NR.nstep_commits(raw, n, 0.97)
            want = NR.textbook_commits(raw, n, 0.97)
            # one commit per raw store from the n-th on, nothing before
            assert len(got) == max(0, len(raw) - n + 1)
            assert got == want[:len(got)], (dones, n)
            # what the fixed delay has not emitted yet is the textbook's flush
            # of a trailing done, never a full window
            assert len(want) - len(got) <= n - 1
            for i, c in enumerate(got):  # start i; cut at the first done, at most n long
                m = round(c[3] - 0.5) - i + 1
                assert c[0] == float(i) and 1 <= m <= n
                assert c[4] == raw[i + m - 1][4] and not any(t[4] for t in raw[i:i + m - 1])
                assert m == n or c[4] == 1
            emitted += len(got)
    assert emitted > 5000


def test_one_step_is_the_raw_stream():
    rng = np.random.default_rng(3)
    raw = _raw(CORNERS["consecutive dones"], rng)
    assert NR.nstep_commits(raw, 1, 0.5) == raw


def test_return_is_rounded_in_the_contract_order():
    r, g = [0.1, -0.7, 0.3, 1e-9], 0.99
    w1 = 1.0 * g
    w2 = w1 * g
    w3 = w2 * g
    assert NR.nstep_return(r, g) == ((r[0] + w1 * r[1]) + w2 * r[2]) + w3 * r[3]


@pytest.mark.parametrize("bad", [0, 33, 2.5, -1, True, "3", None])
def test_bad_n_step_is_refused(bad):
    from dmdqn_amd.agent import AgentConfig, BatchedDQN, check_n_step
    with pytest.raises(ValueError, match="n_step"):
        check_n_step(bad, 10000)
    with pytest.raises(ValueError, match="n_step"):  # before any device work
        BatchedDQN(1, 1, AgentConfig(n_step=bad), device="cpu")


def test_n_step_bounds_and_buffer_size():
    from dmdqn_amd.agent import AgentConfig, BatchedDQN, NSTEP_MAX, check_n_step, sweep_variants
    assert NSTEP_MAX == 32 and AgentConfig().n_step == 1
    assert [check_n_step(n, 10000) for n in (1, 2, 32, np.int64(5))] == [1, 2, 32, 5]
    assert check_n_step(8, 8) == 8
    with pytest.raises(ValueError, match="n_step"):
        check_n_step(9, 8)
    with pytest.raises(ValueError, match="n_step"):
        BatchedDQN(1, 1, AgentConfig(n_step=9, replay_buffer_size=8), device="cpu")
    # not a sweep key
    with pytest.raises(ValueError, match="n_step"):
        sweep_variants(AgentConfig(sweep={"n_step": [1, 3]}))
    assert AgentConfig.from_dict({"n_step": 4, "gamma": 0.9}).n_step == 4


def test_trainer_refuses_the_presampling_schedules():
    """ "sample", "learn" and "full" predict the ring length from the raw store
    count: refused for n_step > 1, before any device work."""
    from dmdqn_amd.agent import AgentConfig
    from dmdqn_amd.trainer import Trainer
    for overlap in ("sample", "learn", "full", True):
        with pytest.raises(ValueError, match="n_step"):
            Trainer(agent_cfg=AgentConfig(n_step=2), device="cpu", overlap=overlap)
    with pytest.raises(ValueError, match="n_step"):
        Trainer(agent_cfg=AgentConfig(n_step=0), device="cpu")


def test_bootstrap_gamma():
    from dmdqn_amd.agent import nstep_gamma
    for g in (0.99, 0.9, 0.123456789, 1.0, 0.0):
        assert nstep_gamma(g, 1) == g
        assert np.float32(nstep_gamma(g, 1)) == np.float32(g) == NR.bootstrap_gamma(g, 1)
        assert nstep_gamma(g, 3) == (1.0 * g) * g * g
        for n in (2, 3, 32):
            assert np.float32(nstep_gamma(g, n)) == NR.bootstrap_gamma(g, n)
    assert NR.bootstrap_gamma(0.9, 3) == np.float32(0.9 * 0.9 * 0.9)


# --------------------------------------------------------------------------- C ABI
@pytest.fixture(scope="module")
def lib():
    from dmdqn_amd import build
    build.build(verbose=False)
    from dmdqn_amd import _lib
    return _lib.load()


def _args(**kw):
    """A dmdqn_nstep_args whose pointers are never dereferenced: every call
    below is refused on the host."""
    from dmdqn_amd._lib import CNStep
    a = CNStep(NA=5, n=3, head=1, cap=11, slot=4, row_format=0, gamma=0.9, gamma_a=None)
    for f in ("st_s", "st_n", "st_a", "st_r", "st_d", "ring_s", "ring_n", "ring_a", "ring_r",
              "ring_d"):
        setattr(a, f, 16)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


REFUSALS = [
    (dict(n=0), b"n=0"), (dict(n=33), b"n=33"), (dict(n=-1), b"n=-1"),
    (dict(head=3), b"head=3"), (dict(head=-1), b"head=-1"),
    (dict(slot=11), b"slot=11"), (dict(slot=-1), b"slot=-1"),
    (dict(NA=0), b"NA=0"), (dict(NA=-3), b"NA=-3"),
    (dict(row_format=2), b"row_format"), (dict(row_format=-1), b"row_format"),
    (dict(gamma=float("nan")), b"gamma"), (dict(gamma=float("inf")), b"gamma"),
    (dict(gamma=1.5), b"gamma"), (dict(gamma=-0.1), b"gamma"),
] + [({f: None}, b"null pointer") for f in ("st_s", "st_n", "st_a", "st_r", "st_d", "ring_s",
                                            "ring_n", "ring_a", "ring_r", "ring_d")]


@pytest.mark.parametrize("kw,msg", REFUSALS, ids=[str(sorted(k.items())) for k, _ in REFUSALS])
def test_commit_refusals_on_the_host(lib, kw, msg):
    rc = lib.dmdqn_replay_nstep_commit(ctypes.byref(_args(**kw)), None)
    assert rc == -1  # DMDQN_EINVAL
    err = lib.dmdqn_last_error()
    assert b"dmdqn_replay_nstep_commit" in err and msg in err, err


def test_commit_refuses_null_args(lib):
    assert lib.dmdqn_replay_nstep_commit(None, None) == -1
    assert b"dmdqn_replay_nstep_commit" in lib.dmdqn_last_error()


def test_abi_is_additive(lib):
    from dmdqn_amd import _lib, ops
    assert lib.dmdqn_version() == 4
    assert ops.ENTRY_POINTS["dmdqn_replay_nstep_commit"] == "replay_nstep_commit"
    assert "dmdqn_replay_nstep_commit" in _lib.SIGNATURES
    D = ops.load()
    assert D.replay_nstep_commit.default._schema.name == "dmdqn::replay_nstep_commit"


def test_nstep_args_layout_matches_header(tmp_path):
    from dmdqn_amd._lib import CNStep, NSTEP_MAX
    fields = [f for f, _ in CNStep._fields_]
    src = tmp_path / "lay.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dmdqn.h"\nint main(void){'
                   'printf("%d %zu", DMDQN_NSTEP_MAX, sizeof(dmdqn_nstep_args));' +
                   "".join(f'printf(" %zu", offsetof(dmdqn_nstep_args, {f}));' for f in fields) +
                   "return 0;}\n")
    exe = tmp_path / "lay"
    subprocess.run(["gcc", f"-I{os.path.join(ROOT, 'include')}", str(src), "-o", str(exe)],
                   check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True,
                                          check=True).stdout.split()]
    assert got[0] == NSTEP_MAX == 32
    assert got[1] == ctypes.sizeof(CNStep)
    assert got[2:] == [getattr(CNStep, f).offset for f in fields]


# --------------------------------------------------------------------------- checkpoint, CLI
def test_checkpoint_fixes_n_step():
    from dmdqn_amd import checkpoint as CK
    assert "n_step" in CK._AGENT_FIXED and CK._DEFAULTS["n_step"] == 1
    assert CK.FORMAT == "dmdqn-ckpt-8"
    old = {}  # saved before n_step existed: one-step transitions
    CK._check_cfg(old, {"n_step": 1}, ["n_step"], "agent_cfg")
    with pytest.raises(ValueError, match="n_step"):
        CK._check_cfg(old, {"n_step": 3}, ["n_step"], "agent_cfg")
    with pytest.raises(ValueError, match="n_step"):
        CK._check_cfg({"n_step": 3}, {"n_step": 1}, ["n_step"], "agent_cfg")


@pytest.mark.parametrize("value", ["0", "33", "2.5"])
def test_cli_refuses_bad_n_step(monkeypatch, capsys, value):
    from src.scripts import train
    monkeypatch.setattr("sys.argv", ["train.py", "--n_step", value])
    with pytest.raises(SystemExit) as e:
        train.main()
    assert e.value.code == 2 and "n_step" in capsys.readouterr().err


def test_cli_passes_n_step_to_the_config():
    from src.scripts.train import AGENT_CONFIG, target_config
    assert "n_step" not in target_config() and "n_step" not in AGENT_CONFIG
    assert target_config(n_step=3)["n_step"] == 3
