"""Per-agent hyperparameters (AgentConfig.sweep: learning_rate / gamma / tau per
env replica) -- everything that needs no GPU: the additive C ABI
(dmdqn_agent_hparams and the four _hp entry points, version still 4), the
ctypes mirror's layout, the host-side refusals, the bit contract of the
per-agent Adam step size, the variant grid and its assignment to replicas, the
config refusals, --sweep parsing and the checkpoint's config rule."""
import ctypes
import dataclasses
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

HP_ENTRIES = ("dmdqn_learn_hp", "dmdqn_learn_grad_hp", "dmdqn_adam_agents_hp",
              "dmdqn_target_soft_update_hp")


@pytest.fixture(scope="module")
def lib():
    from dmdqn_amd import build
    build.build(verbose=False)
    from dmdqn_amd import _lib, agent  # noqa: F401  (agent registers the signatures)
    return _lib.load()


# --------------------------------------------------------------------------- ABI
def test_abi_is_additive(lib):
    import torch  # noqa: F401
    from dmdqn_amd import _lib, ops
    assert lib.dmdqn_version() == 4
    for name in HP_ENTRIES:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
        assert name in ops.ENTRY_POINTS, name
    assert {ops.ENTRY_POINTS[n] for n in HP_ENTRIES} == {"learn_step_hp", "target_soft_update_hp"}
    D = ops.load()
    sch = D.learn_step_hp.default._schema
    assert sch.name == "dmdqn::learn_step_hp"
    names = [a.name for a in sch.arguments]
    base = [a.name for a in D.learn_step.default._schema.arguments]
    # learn_step's arguments, then the per-agent tensors and the two Adam factors
    assert names == base + ["lr", "gamma_a", "tau_a", "one_minus_tau_a", "adam_s", "adam_d"]
    assert base[-2:] == ["tau", "one_minus_tau"]
    sch = D.target_soft_update_hp.default._schema
    assert sch.name == "dmdqn::target_soft_update_hp"
    assert [a.name for a in sch.arguments] == ["params", "target", "target_h", "precision", "tau",
                                               "one_minus_tau"]


def test_hparams_layout_matches_header(tmp_path):
    """agent.CHParams has the size and field offsets gcc gives include/dmdqn.h's
    dmdqn_agent_hparams (the method of test_learn_args_layout_matches_header)."""
    from dmdqn_amd.agent import CHParams
    fields = [f for f, _ in CHParams._fields_]
    assert fields == ["lr", "gamma", "tau", "one_minus_tau", "adam_s", "adam_d"]
    src = tmp_path / "lay.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dmdqn.h"\nint main(void){'
                   'printf("%zu", sizeof(dmdqn_agent_hparams));' +
                   "".join(f'printf(" %zu", offsetof(dmdqn_agent_hparams, {f}));' for f in fields) +
                   "return 0;}\n")
    exe = tmp_path / "lay"
    subprocess.run(["gcc", f"-I{os.path.join(ROOT, 'include')}", str(src), "-o", str(exe)],
                   check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True,
                                          check=True).stdout.split()]
    assert got[0] == ctypes.sizeof(CHParams)
    assert got[1:] == [getattr(CHParams, f).offset for f in fields]


def _learn_args():
    """A dmdqn_learn_args that passes every host check (dummy pointers: a
    refusal returns before any of them is dereferenced)."""
    from dmdqn_amd.agent import CLearn, n_params
    a = CLearn()
    a.NA, a.cap, a.start, a.batch, a.hidden, a.precision, a.P = 2, 302, 0, 128, 128, 1, n_params(128)
    for f in ["ring_s", "ring_n", "ring_a", "ring_d", "ring_r", "idx", "params", "adam_m",
              "adam_v", "target"]:
        setattr(a, f, 4096)
    return a


@pytest.mark.parametrize("entry", HP_ENTRIES[:3])
def test_host_refusals_of_the_learn_entries(lib, entry):
    """Each refusal returns DMDQN_EINVAL (-1) before any launch, and
    dmdqn_last_error() names the entry point."""
    from dmdqn_amd.agent import CHParams
    a = _learn_args()
    dummy = 4096
    extra = () if entry == "dmdqn_learn_hp" else (ctypes.c_void_p(dummy),)

    def call(hp):
        return getattr(lib, entry)(ctypes.byref(a), ctypes.byref(hp), *extra, None)

    for hp in (CHParams(None, None, dummy, None, 1.0, 1.0),      # tau without one_minus_tau
               CHParams(None, None, None, dummy, 1.0, 1.0)):     # ... and the reverse
        assert call(hp) == -1
        msg = lib.dmdqn_last_error()
        assert entry.encode() in msg and b"go together" in msg, msg
    for s, d in ((0.0, 0.5), (0.5, 0.0), (1.5, 0.5), (0.5, 1.5), (-0.1, 0.5),
                 (float("nan"), 0.5), (0.5, float("nan")), (float("inf"), 0.5)):
        assert call(CHParams(dummy, None, None, None, s, d)) == -1, (s, d)
        msg = lib.dmdqn_last_error()
        assert entry.encode() in msg and b"adam_s" in msg, msg
    # without lr the two factors are not read
    a.NA = 0  # (a later check then refuses the call: nothing is launched)
    assert call(CHParams(None, dummy, None, None, 0.0, float("nan"))) == -1
    assert b"adam_s" not in lib.dmdqn_last_error()


def test_host_refusals_of_the_soft_update_entry(lib):
    from dmdqn_amd.agent import n_params
    P = n_params(128)
    d = ctypes.c_void_p(4096)
    for tau, omt in ((None, d), (d, None), (None, None)):
        rc = lib.dmdqn_target_soft_update_hp(d, d, None, 3, P, P, 0, tau, omt, None)
        assert rc == -1
        msg = lib.dmdqn_last_error()
        assert b"dmdqn_target_soft_update_hp" in msg and b"required" in msg, msg
    # the checks it shares with dmdqn_target_soft_update name this entry too
    assert lib.dmdqn_target_soft_update_hp(d, d, None, 0, P, P, 0, d, d, None) == -1
    assert b"dmdqn_target_soft_update_hp" in lib.dmdqn_last_error()


# --------------------------------------------------------------------------- alpha
@pytest.mark.parametrize("t", [1, 2, 3, 10, 500, 5000, 100000])
@pytest.mark.parametrize("lr", [1e-5, 5e-4, 1e-3, 0.3])
def test_alpha_from_factors_is_the_host_alpha(t, lr):
    """What the kernels compute per agent -- fl32(fl32(lr * s) / d) -- is
    keras_adam_consts' alpha, bit for bit."""
    from dmdqn_amd.agent import keras_adam_consts, keras_adam_factors
    s, d = keras_adam_factors(t)
    assert s.dtype == np.float32 and d.dtype == np.float32
    assert 0.0 < s <= 1.0 and 0.0 < d <= 1.0
    alpha = np.float32(np.float32(lr) * s) / d
    assert alpha.dtype == np.float32
    want = np.float32(keras_adam_consts(t, lr)[0])
    assert alpha.view(np.int32) == want.view(np.int32)


# --------------------------------------------------------------------------- variants
def test_grid_order_and_scalar_fallback():
    from dmdqn_amd.agent import AgentConfig, sweep_variants
    cfg = AgentConfig(tau=0.25, sweep={"learning_rate": [1e-4, 3e-4, 1e-3], "gamma": [0.95, 0.99]})
    v = sweep_variants(cfg)
    assert len(v) == 6
    # key insertion order, last key fastest; tau keeps the scalar
    assert [(x["learning_rate"], x["gamma"]) for x in v] == [
        (1e-4, 0.95), (1e-4, 0.99), (3e-4, 0.95), (3e-4, 0.99), (1e-3, 0.95), (1e-3, 0.99)]
    assert all(x["tau"] == 0.25 for x in v)
    w = sweep_variants(AgentConfig(sweep={"gamma": [0.95, 0.99], "learning_rate": [1e-4, 3e-4]}))
    assert [(x["gamma"], x["learning_rate"]) for x in w] == [
        (0.95, 1e-4), (0.95, 3e-4), (0.99, 1e-4), (0.99, 3e-4)]
    assert sweep_variants(AgentConfig(learning_rate=0.002)) == [
        {"learning_rate": 0.002, "gamma": 0.99, "tau": 0.0}]


def test_variant_assignment():
    from dmdqn_amd.agent import variant_assignment
    assert variant_assignment(6, 6).tolist() == [0, 1, 2, 3, 4, 5]
    # E not a multiple of G
    assert variant_assignment(3, 7).tolist() == [0, 1, 2, 0, 1, 2, 0]
    assert variant_assignment(4, 3).tolist() == [0, 1, 2]
    # a rank's shard holds the variants of a single-process run's replicas
    whole = variant_assignment(3, 8)
    assert variant_assignment(3, 4, env_offset=4).tolist() == whole[4:].tolist() == [1, 2, 0, 1]
    assert variant_assignment(3, 8).dtype == np.int64


@pytest.mark.parametrize("sweep,match", [
    ({"epsilon_start": [1.0]}, "epsilon_start"),
    ({"learning_rate": []}, "empty"),
    ({"gamma": [0.9, float("nan")]}, "finite"),
    ({"learning_rate": [float("inf")]}, "finite"),
    ({"learning_rate": [0.0]}, "learning_rate"),
    ({"learning_rate": [1e-3, -1e-3]}, "learning_rate"),
    ({"gamma": [-0.1]}, "gamma"),
    ({"gamma": [1.01]}, "gamma"),
    ({"tau": [0.0, 0.01]}, "tau"),
    ({"tau": [1.5]}, "tau"),
    ({"tau": [float("nan")]}, "tau"),
])
def test_sweep_refusals(sweep, match):
    from dmdqn_amd.agent import AgentConfig, BatchedDQN, sweep_variants
    with pytest.raises(ValueError, match=match):
        sweep_variants(AgentConfig(sweep=sweep))
    # BatchedDQN refuses before any device work (this runs without a GPU)
    with pytest.raises(ValueError, match=match):
        BatchedDQN(2, 2, AgentConfig(sweep=sweep))


def test_sweep_needs_independent_nets():
    from dmdqn_amd.agent import AgentConfig, BatchedDQN
    cfg = AgentConfig(precision="fp16", shared_params=True, sweep={"gamma": [0.9, 0.99]})
    with pytest.raises(ValueError, match="shared_params"):
        BatchedDQN(2, 2, cfg)


def test_trainer_refuses_before_building_the_env():
    """(No GPU here: reaching the env's device work would raise something else.)"""
    from dmdqn_amd.agent import AgentConfig
    from dmdqn_amd.trainer import Trainer
    with pytest.raises(ValueError, match="tau"):
        Trainer(None, AgentConfig(sweep={"tau": [0.0]}))


def test_accepted_edges():
    from dmdqn_amd.agent import AgentConfig, sweep_variants
    v = sweep_variants(AgentConfig(sweep={"gamma": [0, 1], "tau": [1.0, 1e-3]}))
    assert [(x["gamma"], x["tau"]) for x in v] == [(0.0, 1.0), (0.0, 1e-3), (1.0, 1.0), (1.0, 1e-3)]


def test_config_round_trip():
    from dmdqn_amd.agent import AgentConfig
    cfg = AgentConfig(sweep={"learning_rate": [1e-4, 1e-3], "tau": [0.01]})
    d = dataclasses.asdict(cfg)
    assert d["sweep"] == {"learning_rate": [1e-4, 1e-3], "tau": [0.01]}
    assert AgentConfig.from_dict(d) == cfg
    assert list(AgentConfig.from_dict(d).sweep) == ["learning_rate", "tau"]
    assert AgentConfig().sweep is None and AgentConfig.from_dict({}).sweep is None


# --------------------------------------------------------------------------- train.py
def test_parse_sweep():
    from src.scripts.train import parse_sweep
    assert parse_sweep(None) is None and parse_sweep([]) is None
    got = parse_sweep(["learning_rate=1e-4,5e-4,1e-3", "gamma=0.95"])
    assert got == {"learning_rate": [1e-4, 5e-4, 1e-3], "gamma": [0.95]}
    assert list(got) == ["learning_rate", "gamma"]  # the grid's key order
    assert list(parse_sweep(["gamma=0.9", "learning_rate=1e-3"])) == ["gamma", "learning_rate"]
    for bad in (["gamma"], ["gamma="], ["=0.9"], ["gamma=0.9,x"], ["gamma=0.9", "gamma=0.99"],
                ["gamma=0.9,,0.99"]):
        with pytest.raises(ValueError, match="--sweep"):
            parse_sweep(bad)


def test_rank_variants():
    from src.scripts.train import rank_variants
    v = [{"learning_rate": a, "gamma": 0.99, "tau": 0.0} for a in (1e-4, 5e-4, 1e-3, 2e-3)]
    got = rank_variants(v, [0, 1, 2, 0, 1, 2], [-30.0, -10.0, -20.0, None])
    assert [r["variant"] for r in got] == [1, 2, 0]  # variant 3 has no replica
    assert [r["rank"] for r in got] == [1, 2, 3]
    assert got[0]["first_env"] == 1 and got[0]["envs"] == 2 and got[0]["learning_rate"] == 5e-4
    assert got[0]["smooth_total_reward"] == -10.0


def test_variant_smoothed_values_follow_smoothed_value():
    """The vector form train.py keeps on the device: SmoothedValue's rule per
    element, bit for bit (the same float64 operations in the same order), NaN
    (a variant without replicas) read back as None."""
    import torch
    from src.scripts.train import SmoothedValue, VariantSmoothedValues
    seq = [[-30.5, -10.25, float("nan")], [-28.1, -12.7, float("nan")], [-3.3, -40.9, float("nan")]]
    vs, ref = VariantSmoothedValues(alpha=0.3), [SmoothedValue(alpha=0.3) for _ in range(2)]
    assert vs.get_values() == []
    for row in seq:
        vs.update(torch.tensor(row, dtype=torch.float64))
        for sm, x in zip(ref, row):
            sm.update(x)
        assert vs.get_values() == [ref[0].get_value(), ref[1].get_value(), None]


# --------------------------------------------------------------------------- checkpoint
def test_checkpoint_config_rule():
    from dmdqn_amd import checkpoint as CK
    from dmdqn_amd.agent import AgentConfig
    assert "sweep" in CK._AGENT_FIXED and CK._DEFAULTS["sweep"] is None
    a = CK._cfg_dict(AgentConfig(sweep={"learning_rate": [1e-4, 1e-3], "gamma": [0.9]}))
    same = CK._cfg_dict(AgentConfig(sweep={"learning_rate": [1e-4, 1e-3], "gamma": [0.9]}))
    CK._check_cfg(a, same, CK._AGENT_FIXED, "agent_cfg")
    none = CK._cfg_dict(AgentConfig())
    for other in (none,
                  CK._cfg_dict(AgentConfig(sweep={"learning_rate": [1e-4, 2e-3], "gamma": [0.9]})),
                  # the key order decides which variant a replica runs
                  CK._cfg_dict(AgentConfig(sweep={"gamma": [0.9], "learning_rate": [1e-4, 1e-3]}))):
        with pytest.raises(ValueError, match="sweep"):
            CK._check_cfg(a, other, CK._AGENT_FIXED, "agent_cfg")
        with pytest.raises(ValueError, match="sweep"):
            CK._check_cfg(other, a, CK._AGENT_FIXED, "agent_cfg")
    # a checkpoint saved before the field existed ran no sweep
    old = {k: v for k, v in none.items() if k != "sweep"}
    CK._check_cfg(old, none, CK._AGENT_FIXED, "agent_cfg")
    with pytest.raises(ValueError, match="sweep"):
        CK._check_cfg(old, a, CK._AGENT_FIXED, "agent_cfg")
    # what is saved loads with torch.load(weights_only=True): plain lists
    assert a["sweep"] == [["learning_rate", [1e-4, 1e-3]], ["gamma", [0.9]]]
