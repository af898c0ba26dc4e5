"""Soft (Polyak) target updates, the parts that need no GPU: the additive C ABI
(dmdqn_learn_args.tau / .one_minus_tau, dmdqn_target_soft_update), its host-side
argument checks, the Python configuration surface, the checkpoint rule and the
numpy restatement of the update against the reference's own
update_target_network_soft (tests/golden/soft_target.npz, made by
tests/golden/make_soft_golden.py)."""
import ctypes
import os

import numpy as np
import pytest

from conftest import GOLDEN


def soft_update_np(online, target, tau):
    """dqn_agent.py:389-399 in float32 numpy, as TF's three elementwise kernels
    round it: fl32(fl32(tau_f * online) + fl32(omt_f * target)), tau_f =
    float32(tau), omt_f = float32(1.0 - tau) (the subtraction in double)."""
    tau_f, omt_f = np.float32(tau), np.float32(1.0 - float(tau))
    online, target = np.asarray(online, np.float32), np.asarray(target, np.float32)
    return (tau_f * online).astype(np.float32) + (omt_f * target).astype(np.float32)


@pytest.fixture(scope="module")
def lib():
    from dmdqn_amd import build
    build.build(verbose=False)
    from dmdqn_amd import _lib, agent  # noqa: F401  (agent registers the learn signatures)
    return _lib.load()


def test_abi_is_additive(lib):
    """No version bump; the new entry point is exported, has a ctypes signature
    and is wrapped by a registered operator; learn_step takes tau (default 0)."""
    from dmdqn_amd import _lib, ops
    assert lib.dmdqn_version() == 4
    assert hasattr(lib, "dmdqn_target_soft_update")
    assert len(_lib.SIGNATURES["dmdqn_target_soft_update"]) == 10
    assert ops.ENTRY_POINTS["dmdqn_target_soft_update"] == "target_soft_update"
    D = ops.load()
    assert D.target_soft_update.default._schema.name == "dmdqn::target_soft_update"
    args = {a.name: a for a in D.learn_step.default._schema.arguments}
    assert args["tau"].default_value == 0.0 and args["one_minus_tau"].default_value == 1.0
    assert [a.name for a in D.learn_step.default._schema.arguments][-2:] == ["tau", "one_minus_tau"]


def test_clearn_ends_with_tau():
    from dmdqn_amd.agent import CLearn
    assert [f for f, _ in CLearn._fields_][-2:] == ["tau", "one_minus_tau"]
    assert CLearn().tau == 0.0 and CLearn().one_minus_tau == 0.0  # zero-initialised = off


def _soft(lib, params, target, target_h, NW, P, Ph, precision, tau, omt):
    return lib.dmdqn_target_soft_update(params, target, target_h, NW, P, Ph, precision,
                                        ctypes.c_float(tau), ctypes.c_float(omt), None)


def test_soft_update_argument_checks_on_host(lib):
    """Every refusal happens before a launch: -1 and a message (the pointers
    are never dereferenced)."""
    p = ctypes.c_void_p(4096)
    P = 28548
    assert _soft(lib, None, p, None, 1, P, P, 0, 0.5, 0.5) == -1
    assert b"dmdqn_target_soft_update" in lib.dmdqn_last_error()
    assert _soft(lib, p, None, None, 1, P, P, 0, 0.5, 0.5) == -1
    for tau in (-0.1, 1.5, float("nan"), 0.0):
        assert _soft(lib, p, p, None, 1, P, P, 0, tau, 0.5) == -1, tau
        assert b"tau" in lib.dmdqn_last_error()
    assert _soft(lib, p, p, None, 1, P, P, 0, 0.5, 1.5) == -1
    assert b"one_minus_tau" in lib.dmdqn_last_error()
    assert _soft(lib, p, p, p, 1, P, P - 4, 1, 0.5, 0.5) == -1  # Ph < P
    assert b"Ph=" in lib.dmdqn_last_error()
    assert _soft(lib, p, p, p, 1, P, P, 0, 0.5, 0.5) == -1  # fp32 with a shadow
    assert b"no 16-bit shadow" in lib.dmdqn_last_error()
    assert _soft(lib, p, p, None, 1, P, P, 3, 0.5, 0.5) == -1
    assert b"precision" in lib.dmdqn_last_error()


def test_learn_tau_checked_on_host(lib):
    from dmdqn_amd.agent import CLearn
    for tau in (-0.1, 1.5, float("nan")):
        a = CLearn()
        a.tau, a.one_minus_tau = tau, 0.5
        assert lib.dmdqn_learn(ctypes.byref(a), None) == -1
        assert b"tau" in lib.dmdqn_last_error(), lib.dmdqn_last_error()
    a = CLearn()
    a.tau, a.one_minus_tau = 0.5, -0.5
    assert lib.dmdqn_learn(ctypes.byref(a), None) == -1
    assert b"one_minus_tau" in lib.dmdqn_last_error()
    a = CLearn()  # tau = 0: the other checks answer, as before
    assert lib.dmdqn_learn(ctypes.byref(a), None) == -1
    assert b"tau" not in lib.dmdqn_last_error()


def test_config_validation_before_any_device(lib):
    from dmdqn_amd.agent import AgentConfig, BatchedDQN
    for tau in (1.5, -1, float("nan")):
        with pytest.raises(ValueError, match="tau"):
            BatchedDQN(1, 1, AgentConfig(tau=tau), device="cuda")
    with pytest.raises(ValueError, match="target_update_frequency"):
        BatchedDQN(1, 1, AgentConfig(target_update_frequency=-1), device="cuda")
    assert AgentConfig().tau == 0.0
    assert AgentConfig.from_dict({"tau": 0.01}).tau == 0.01


def test_soft_path_option(lib):
    """DMDQN_OPT_SOFT_PATH (2): auto | fused | split, set through
    dmdqn_set_option like the other launcher hooks."""
    from dmdqn_amd import _lib
    assert lib.dmdqn_get_option(2) == 0
    with _lib.option("soft_path", "fused"):
        assert lib.dmdqn_get_option(2) == 1
        with _lib.option("soft_path", "split"):
            assert lib.dmdqn_get_option(2) == 2
    assert lib.dmdqn_get_option(2) == 0
    assert lib.dmdqn_set_option(2, 3) == -1 and lib.dmdqn_get_option(2) == 0


def test_constants_helper():
    from dmdqn_amd.agent import soft_update_consts
    tau_f, omt_f = soft_update_consts(0.005)
    assert type(tau_f) is np.float32 and type(omt_f) is np.float32
    assert (tau_f, omt_f) == (np.float32(0.005), np.float32(0.995))
    # the subtraction is in double: not float32(1) - float32(tau)
    t = 0.3
    assert soft_update_consts(t)[1] == np.float32(1.0 - t)
    assert soft_update_consts(1.0) == (np.float32(1.0), np.float32(0.0))


def test_checkpoint_cfg_rule():
    from dmdqn_amd import checkpoint as CK
    assert "tau" in CK._AGENT_FIXED and CK._DEFAULTS["tau"] == 0.0
    with pytest.raises(ValueError, match="tau"):
        CK._check_cfg({"tau": 0.01}, {"tau": 0.02}, ["tau"], "agent_cfg")
    with pytest.raises(ValueError, match="tau"):
        CK._check_cfg({}, {"tau": 0.01}, ["tau"], "agent_cfg")  # saved before tau existed
    CK._check_cfg({}, {"tau": 0.0}, ["tau"], "agent_cfg")
    CK._check_cfg({"tau": 0.01}, {"tau": 0.01}, ["tau"], "agent_cfg")


def test_train_script_flags():
    from src.scripts import train as T
    assert T.target_config() == T.AGENT_CONFIG
    c = T.target_config(0.01, 0)
    assert c["tau"] == 0.01 and c["target_update_frequency"] == 0
    assert "tau" not in T.AGENT_CONFIG


def test_numpy_restatement_matches_reference_first_soft_update():
    """The reference's own update_target_network_soft (under the TF
    restatement, see make_soft_golden.py): its target after learn 1 equals the
    numpy formula on its online net after learn 1 and the initial target, bit
    for bit (every 8th parameter is stored)."""
    from dmdqn_amd.agent import keras_initial_weights
    G = np.load(os.path.join(GOLDEN, "soft_target.npz"))
    init_seed, stride = int(G["cfg"][4]), int(G["cfg"][5])
    w0 = keras_initial_weights(np.random.RandomState(init_seed), 128, 1)[0]
    t1 = soft_update_np(G["w1"], w0[::stride], float(G["tau"][0]))
    assert t1.dtype == np.float32
    assert np.array_equal(t1.view(np.int32), G["t1"].view(np.int32))
    assert not np.array_equal(G["t1"], w0[::stride])  # the update moved the target
