"""Population-based training without a GPU: the restatement (tests/pbt_ref.py)
against the textbook selection, every refusal of the config, the CLI syntax,
the explore draws, the C ABI's host-side refusals and the checkpoint's config
comparison."""
import ctypes
import math

import numpy as np
import pytest

import pbt_ref as PR

E_SIZES = [2, 5, 8, 67]


# --------------------------------------------------------------------------- selection
def textbook_src(f, n):
    """Sort by fitness, best first (stable: ties keep index order); the bottom
    n take the top n, worst <- best."""
    f = np.asarray(f, dtype=np.float64)
    f = np.where(np.isnan(f), -np.inf, f)
    order = np.argsort(-f, kind="stable")
    E = len(f)
    src = np.arange(E)
    for i in range(n):
        src[order[E - 1 - i]] = order[i]
    return order, src.tolist()


@pytest.mark.parametrize("E", E_SIZES)
def test_restated_selection_is_the_textbook_truncation(E):
    vectors = PR.fitness_vectors(E)
    assert set(vectors) >= {"ties", "equal", "negative", "zeros", "nan"}
    for name, f in vectors.items():
        for n in sorted({1, E // 2}):
            src, rank = PR.select(f.tolist(), n)
            order, want = textbook_src(f, n)
            assert sorted(rank) == list(range(E)), (name, "rank is a permutation")
            assert [rank[e] for e in order] == list(range(E)), (name, n)
            assert src == want, (name, n)
            # winners and losers are disjoint, every winner has exactly one clone
            copied = PR.pairs(src)
            assert len(copied) == n and len({s for _, s in copied}) == n
            assert all(src[s] == s for _, s in copied)
    assert PR.select([1.0, 1.0, 1.0, 1.0], 2)[0] == [0, 1, 1, 0]  # ties: the lower index wins
    assert PR.select([0.0, -0.0], 1)[0] == [0, 0]
    assert PR.select([math.nan, -5.0], 1)[0] == [1, 1]


def test_restated_score_adds_in_junction_order():
    big = [[1e16, 1.0, -1e16], [1.0, 1e16, -1e16], [-1e16, 1e16, 1.0]]
    assert PR.score([0.0, 0.0, 0.0], big) == [0.0, 0.0, 1.0]
    assert PR.score([2.0, 0.5], [[3.0], [-0.5]]) == [5.0, 0.0]
    assert PR.truncated(0.25, 8) == 2 and PR.truncated(0.25, 7) == 1 and PR.truncated(0.5, 5) == 2


# --------------------------------------------------------------------------- config
def _cfg(pbt, **kw):
    from dmdqn_amd.agent import AgentConfig
    return AgentConfig(pbt=pbt, **kw)


def test_defaults_and_from_dict():
    from dmdqn_amd.agent import AgentConfig, check_pbt, normalize_pbt
    assert AgentConfig().pbt is None and check_pbt(AgentConfig(), 8) is None
    assert AgentConfig.from_dict({"pbt": {"interval": 5}}).pbt == {"interval": 5}
    p = normalize_pbt({"interval": 500})
    assert p == {"interval": 500, "truncation": 0.25, "perturb": {"learning_rate": [0.8, 1.25]},
                 "bounds": {"learning_rate": [1e-6, 1e-1], "gamma": [0.5, 0.9999],
                            "tau": [1e-4, 1.0]}, "seed": 0}
    full = check_pbt(_cfg({"interval": 40, "perturb": {"gamma": [0.9], "learning_rate": [2.0]},
                           "bounds": {"gamma": [0.1, 0.2]}, "seed": 3}), 8)
    assert full["n"] == 2 and list(full["perturb"]) == ["learning_rate", "gamma"]
    assert full["bounds"]["gamma"] == [0.1, 0.2] and full["bounds"]["tau"] == [1e-4, 1.0]


BAD = [
    ({"interval": 10, "period": 3}, {}, 8, "period"),                 # an unknown key
    ({"truncation": 0.25}, {}, 8, "interval"),                        # interval is required
    ({"interval": 0}, {}, 8, "interval"), ({"interval": 2.5}, {}, 8, "interval"),
    ({"interval": True}, {}, 8, "interval"),
    ({"interval": 10, "truncation": 0.1}, {}, 8, "n = 0"),             # n < 1
    ({"interval": 10, "truncation": 0.75}, {}, 8, "n = 6"),            # 2 n > E
    ({"interval": 10, "truncation": 0.5}, {}, 5, None),                # (2 n = 4 <= 5: accepted)
    ({"interval": 10, "truncation": 0.6}, {}, 5, "n = 3"),
    ({"interval": 10, "truncation": float("nan")}, {}, 8, "truncation"),
    ({"interval": 10}, {"shared_params": True, "precision": "fp16"}, 8, "shared_params"),
    ({"interval": 10, "perturb": {"tau": [0.5, 2.0]}}, {}, 8, "tau"),  # the run's tau is 0
    ({"interval": 10, "perturb": {"tau": [0.5, 2.0]}}, {"tau": 0.01}, 8, None),
    ({"interval": 10, "perturb": {"tau": [0.5]}}, {"sweep": {"tau": [0.1, 0.2]}}, 8, None),
    ({"interval": 10, "perturb": {"n_step": [2.0]}}, {}, 8, "n_step"),
    ({"interval": 10, "perturb": {"gamma": []}}, {}, 8, "gamma"),
    ({"interval": 10, "perturb": {"gamma": [0.0]}}, {}, 8, "gamma"),
    ({"interval": 10, "perturb": {"gamma": [-1.0]}}, {}, 8, "gamma"),
    ({"interval": 10, "perturb": {"gamma": [float("inf")]}}, {}, 8, "gamma"),
    ({"interval": 10, "bounds": {"gamma": [0.9, 0.5]}}, {}, 8, "lo <= hi"),
    ({"interval": 10, "bounds": {"gamma": [0.9]}}, {}, 8, "gamma"),
    ({"interval": 10, "bounds": {"epsilon": [0.0, 1.0]}}, {}, 8, "epsilon"),
    ({"interval": 10, "seed": -1}, {}, 8, "seed"),
    ([("interval", 10)], {}, 8, "dict"),
]


@pytest.mark.parametrize("pbt,kw,E,msg", BAD, ids=[f"{i}-{b[3]}" for i, b in enumerate(BAD)])
def test_config_refusals_come_before_any_device_work(pbt, kw, E, msg):
    from dmdqn_amd.agent import BatchedDQN, check_pbt
    cfg = _cfg(pbt, **kw)
    if msg is None:
        assert check_pbt(cfg, E)["n"] >= 1
        return
    with pytest.raises(ValueError, match=msg):
        check_pbt(cfg, E)
    # the agent refuses it itself, before it touches a device (none exists here)
    with pytest.raises(ValueError, match=msg):
        BatchedDQN(E, 4, cfg, device="cuda")


def test_trainer_refuses_other_schedules_and_bad_configs():
    from dmdqn_amd.env import EnvConfig
    from dmdqn_amd.trainer import Trainer
    env = EnvConfig(rows=2, cols=2, num_envs=8)
    for overlap in ("sample", "learn", "full", True):
        with pytest.raises(ValueError, match="pbt"):
            Trainer(env, _cfg({"interval": 40}), device="cpu", overlap=overlap)
    with pytest.raises(ValueError, match="n = 0"):
        Trainer(EnvConfig(rows=2, cols=2, num_envs=3), _cfg({"interval": 40}), device="cpu")
    with pytest.raises(ValueError, match="period"):
        Trainer(env, _cfg({"interval": 40, "period": 1}), device="cpu", overlap="env")


def test_dropin_agent_refuses_pbt():
    from src.agents import dqn_agent
    with pytest.raises(ValueError, match="pbt"):
        dqn_agent.DQNAgent(89, 4, "J_0_0", {"pbt": {"interval": 10}})


# --------------------------------------------------------------------------- explore
def test_explore_is_deterministic_clipped_and_leaves_the_rest():
    E = 8
    values = {"learning_rate": [1e-3 * (e + 1) for e in range(E)], "gamma": [0.99] * E,
              "tau": [0.01 * (e + 1) for e in range(E)]}
    src = [0, 1, 2, 3, 4, 5, 1, 0]
    perturb = {"learning_rate": [0.5, 2.0], "gamma": [1.5]}
    bounds = {"learning_rate": [1e-6, 1.5e-3], "gamma": [0.5, 0.9999], "tau": [1e-4, 1.0]}
    a = PR.explore(values, src, perturb, bounds, seed=7, k=2, env_offset=16)
    assert a == PR.explore(values, src, perturb, bounds, seed=7, k=2, env_offset=16)
    rs = np.random.RandomState(np.array([7, 2, 16], dtype=np.uint32))
    c_lr, c_g = rs.randint(0, 2, size=E), rs.randint(0, 1, size=E)
    assert not c_g.any()
    for key in values:  # a replica that was not copied keeps every value
        assert a[key][:6] == values[key][:6]
    for e, s in ((6, 1), (7, 0)):
        want = min(max(values["learning_rate"][s] * perturb["learning_rate"][c_lr[e]], 1e-6), 1.5e-3)
        assert a["learning_rate"][e] == want
        assert a["gamma"][e] == 0.9999          # 0.99 * 1.5 clipped to hi
        assert a["tau"][e] == values["tau"][s]   # per agent but not perturbed: the source's
    # another round, seed or rank offset draws other factors (over enough replicas)
    big = {"learning_rate": [1e-3] * 64}
    src64 = [e % 32 for e in range(64)]
    b = {"learning_rate": [1e-9, 1.0]}
    base = PR.explore(big, src64, {"learning_rate": [0.5, 2.0]}, b, 0, 0)["learning_rate"]
    assert set(base[32:]) == {5e-4, 2e-3} and base[:32] == big["learning_rate"][:32]
    for other in ((1, 0, 0), (0, 1, 0), (0, 0, 64)):
        assert PR.explore(big, src64, {"learning_rate": [0.5, 2.0]}, b, *other)[
            "learning_rate"] != base
    # clipping from below
    assert PR.explore({"learning_rate": [1e-6, 1.0]}, [0, 0], {"learning_rate": [0.5]},
                      {"learning_rate": [1e-6, 1e-1]}, 0, 0)["learning_rate"] == [1e-6, 1e-6]


def test_device_array_formulas_are_the_agents():
    from dmdqn_amd.agent import nstep_gamma, soft_update_consts
    vals = {"learning_rate": [1e-3, 3e-4], "gamma": [0.99, 0.9], "tau": [0.01, 0.5]}
    d = PR.device_arrays(vals, 3, 2)
    assert d["hp_lr"].dtype == np.float32 and d["hp_lr"].tolist() == [
        float(np.float32(1e-3))] * 2 + [float(np.float32(3e-4))] * 2
    assert d["hp_gamma"][2] == np.float32(nstep_gamma(0.9, 3)) == np.float32(0.9 * 0.9 * 0.9)
    assert d["nstep_gamma_a"].dtype == np.float64 and d["nstep_gamma_a"].tolist() == [
        0.99, 0.99, 0.9, 0.9]
    assert (d["hp_tau"][0], d["hp_omt"][0]) == soft_update_consts(0.01)
    assert set(PR.device_arrays({"gamma": [0.9]}, 1, 1)) == {"hp_gamma", "nstep_gamma_a"}


# --------------------------------------------------------------------------- CLI
def test_cli_parsing():
    from src.scripts.train import parse_pbt
    assert parse_pbt(None) is None
    assert parse_pbt("interval=500,truncation=0.25,seed=0") == {
        "interval": 500, "truncation": 0.25, "seed": 0}
    assert parse_pbt("interval=200") == {"interval": 200}
    got = parse_pbt("interval=40", ["learning_rate=0.8,1.25", "gamma=0.99,1.01"])
    assert got == {"interval": 40, "perturb": {"learning_rate": [0.8, 1.25], "gamma": [0.99, 1.01]}}
    assert list(got["perturb"]) == ["learning_rate", "gamma"]
    for bad in ("interval", "interval=", "interval=x", "interval=2.5", "every=3",
                "interval=3,interval=4", "interval=3,,seed=1"):
        with pytest.raises(ValueError, match="--pbt"):
            parse_pbt(bad)
    with pytest.raises(ValueError, match="--pbt_perturb"):
        parse_pbt(None, ["gamma=0.9"])
    for bad in (["gamma"], ["gamma=a,b"], ["gamma=0.9", "gamma=0.8"]):
        with pytest.raises(ValueError, match="--pbt_perturb"):
            parse_pbt("interval=5", bad)


@pytest.mark.parametrize("argv", [["--pbt", "interval=200"],
                                  ["--batched", "--pbt", "interval=x"],
                                  ["--batched", "--pbt_perturb", "gamma=0.9,1.1"]])
def test_cli_refuses(monkeypatch, capsys, argv):
    from src.scripts import train
    monkeypatch.setattr("sys.argv", ["train.py"] + argv)
    with pytest.raises(SystemExit) as e:
        train.main()
    assert e.value.code == 2 and "--pbt" in capsys.readouterr().err


# --------------------------------------------------------------------------- C ABI
@pytest.fixture(scope="module")
def lib():
    from dmdqn_amd import build
    build.build(verbose=False)
    from dmdqn_amd import _lib
    return _lib.load()


P, PH = 28548, 28552
X = 4096  # a 16-B aligned address that is never dereferenced: every call is refused first


def _refused(lib, rc, name, msg):
    assert rc == -1  # DMDQN_EINVAL
    err = lib.dmdqn_last_error()
    assert name in err and msg in err, err


def test_score_refusals_on_the_host(lib):
    for args, msg in [((None, 5, 3, X), b"null"), ((X, 5, 3, None), b"null"),
                      ((X, 0, 3, X), b"E = 0"), ((X, 5, 0, X), b"A = 0"),
                      ((X, -1, 3, X), b"E = -1"), ((X, 1 << 20, 1 << 12, X), b"2^31")]:
        _refused(lib, lib.dmdqn_pbt_score(*args, None), b"dmdqn_pbt_score", msg)


def test_select_refusals_on_the_host(lib):
    for args, msg in [((None, 8, 2, X, X), b"null"), ((X, 8, 2, None, X), b"null"),
                      ((X, 8, 2, X, None), b"null"), ((X, 1, 1, X, X), b"E = 1"),
                      ((X, 0, 1, X, X), b"E = 0"), ((X, 65537, 1, X, X), b"E = 65537"),
                      ((X, 8, 0, X, X), b"n = 0"), ((X, 8, 5, X, X), b"n = 5"),
                      ((X, 5, 3, X, X), b"n = 3"), ((X, 8, -1, X, X), b"n = -1")]:
        _refused(lib, lib.dmdqn_pbt_select(*args, None), b"dmdqn_pbt_select", msg)


def test_exchange_refusals_on_the_host(lib):
    ok = dict(src=X, E=5, A=3, P=P, Ph=PH, params=X, target=X, adam_m=X, adam_v=X, target_h=X)
    cases = [(dict(src=None), b"null"), (dict(params=None), b"null"), (dict(target=None), b"null"),
             (dict(adam_m=None), b"null"), (dict(adam_v=None), b"null"),
             (dict(E=0), b"E = 0"), (dict(A=0), b"A = 0"), (dict(E=1 << 20, A=1 << 10), b"2^31"),
             (dict(P=0), b"P = 0"), (dict(P=28550), b"P = 28550"), (dict(P=-4), b"P = -4"),
             (dict(Ph=28548), b"Ph = 28548"), (dict(Ph=28556 + 2), b"Ph = 28558"),
             (dict(Ph=8), b"Ph = 8"),
             (dict(params=X + 4), b"alignment"), (dict(target_h=X + 8), b"alignment")]
    for kw, msg in cases:
        a = dict(ok, **kw)
        rc = lib.dmdqn_pbt_exchange(a["src"], a["E"], a["A"], a["P"], a["Ph"], a["params"],
                                    a["target"], a["adam_m"], a["adam_v"], a["target_h"], None)
        _refused(lib, rc, b"dmdqn_pbt_exchange", msg)


def test_abi_is_additive(lib):
    from dmdqn_amd import _lib, build, ops
    assert lib.dmdqn_version() == 4
    D = ops.load()
    for name in ("pbt_score", "pbt_select", "pbt_exchange"):
        assert ops.ENTRY_POINTS["dmdqn_" + name] == name and "dmdqn_" + name in _lib.SIGNATURES
        assert getattr(D, name).default._schema.name == "dmdqn::" + name
    assert str(D.pbt_exchange.default._schema).count("!") == 5  # every row array is mutated
    assert "pbt.hip" in build.KERNEL_SOURCES["pbt"] and len(build.source_digest("pbt")) == 16
    assert any(p.endswith("pbt.hip") for p in build.tree_files())


# --------------------------------------------------------------------------- checkpoint
def test_checkpoint_fixes_the_pbt_config(tmp_path):
    import torch
    from dmdqn_amd import checkpoint as CK
    assert "pbt" in CK._AGENT_FIXED and CK._DEFAULTS["pbt"] is None
    assert CK.FORMAT == "dmdqn-ckpt-8"  # the format string did not change
    cfg = _cfg({"interval": 40, "perturb": {"gamma": [0.99, 1.01], "learning_rate": [0.8, 1.25]}},
               sweep={"learning_rate": [3e-4, 1e-3]})
    d = CK._cfg_dict(cfg)
    assert d["pbt"][0] == ["interval", 40] and d["pbt"][1] == ["truncation", 0.25]
    assert d["pbt"][2] == ["perturb", [["learning_rate", [0.8, 1.25]], ["gamma", [0.99, 1.01]]]]
    path = str(tmp_path / "cfg.pt")
    torch.save({"agent_cfg": d}, path)
    back = torch.load(path, map_location="cpu", weights_only=True)["agent_cfg"]
    assert back == d
    CK._check_cfg(back, d, CK._AGENT_FIXED, "agent_cfg")
    # the same config with its defaults spelled out is the same config
    same = _cfg({"interval": 40, "truncation": 0.25, "seed": 0,
                 "perturb": {"learning_rate": [0.8, 1.25], "gamma": [0.99, 1.01]}},
                sweep={"learning_rate": [3e-4, 1e-3]})
    CK._check_cfg(back, CK._cfg_dict(same), CK._AGENT_FIXED, "agent_cfg")
    for other in ({"interval": 41}, {"interval": 40, "seed": 1}, {"interval": 40, "truncation": 0.5},
                  {"interval": 40, "perturb": {"gamma": [0.99, 1.01]}}, None):
        cur = CK._cfg_dict(_cfg(other, sweep={"learning_rate": [3e-4, 1e-3]}))
        with pytest.raises(ValueError, match="pbt"):
            CK._check_cfg(back, cur, CK._AGENT_FIXED, "agent_cfg")
    # a checkpoint saved before pbt existed loads into a Trainer without it only
    old = {k: v for k, v in CK._cfg_dict(_cfg(None)).items() if k != "pbt"}
    CK._check_cfg(old, CK._cfg_dict(_cfg(None)), CK._AGENT_FIXED, "agent_cfg")
    with pytest.raises(ValueError, match="pbt"):
        CK._check_cfg(old, CK._cfg_dict(_cfg({"interval": 40})), CK._AGENT_FIXED, "agent_cfg")
