"""Network health probe (AgentConfig.health_every; dmdqn_net_probe,
dmdqn_layer_norms) -- everything that needs no GPU: the numpy restatement
(health_ref.py) on the exact-forward fixtures, the additive C ABI and its host
refusals, the operator schemas, the config key and its refusals, the
checkpoint's default and --health_every."""
import ctypes

import numpy as np
import pytest

import exact_fixture as XF
import health_ref as HR


@pytest.fixture(scope="module")
def lib():
    from dmdqn_amd import build
    build.build(verbose=False)
    from dmdqn_amd import _lib, agent  # noqa: F401  (agent registers the signatures)
    return _lib.load()


# --------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("name", ["f16", "bf16"])
def test_restatement_on_the_exact_fixtures(name):
    """probe_ref against the fixture's own exact forward (exact_fixture.learn_ref
    goes through exact_forward, which proves exactness): the counts are those
    of its z1 / z2, no unit is dead as drawn, nothing is non-finite, and the
    batches hold zero pre-activations, so a `>=` ReLU counts otherwise."""
    fx = XF.fixture(name)
    zeros1, zeros2, active = [], [], []
    for j in range(fx.NA):
        S = fx.batch(j)[0]
        ws = XF.split(fx.online[j].astype(np.float64), fx.H)
        counts, stats, mask = HR.probe_ref(ws, S, fx.precision)
        ref = XF.learn_ref(fx, j, 0)
        z1, z2, q = ref["z1"], ref["z2"], ref["q"]
        assert counts[0] == (z1 > 0).sum() and counts[2] == (z2 > 0).sum()
        assert counts[1] == 0 and counts[3] == 0 and counts[4] == 0 and not mask.any()
        assert stats[0] == np.maximum(z1, 0).sum() and stats[1] == np.maximum(z2, 0).sum()
        assert stats[2] == np.abs(z1).max() and stats[3] == np.abs(z2).max()
        assert stats[4] == np.abs(q).max()
        ge = HR.probe_ref(ws, S, fx.precision, relu_ge=True)[0]
        n1, n2 = int((z1 == 0).sum()), int((z2 == 0).sum())
        assert n1 > 0 and n2 > 0
        assert ge[0] == counts[0] + n1 and ge[2] == counts[2] + n2  # the >= variant differs
        zeros1.append(n1)
        zeros2.append(n2)
        active.append(int(counts[0]))
    print(f"{name}: z1 == 0 {min(zeros1)}..{max(zeros1)}, z2 == 0 {min(zeros2)}..{max(zeros2)}, "
          f"active {min(active)}..{max(active)} of {128 * 128}")


def test_restatement_dead_units_and_non_finite():
    """Dead under `>` only (z == 0 on every row), dead either way (z < 0), the
    mask bits, an overflowing and a NaN output column."""
    fx = XF.fixture("f16")
    S = fx.batch(0)[0]
    W1, b1, W2, b2, W3, b3 = (w.copy() for w in XF.split(fx.online[0].astype(np.float64), fx.H))
    for u in (0, 17, 127):
        W1[:, u], b1[u] = 0.0, 0.0
    for u in (5, 64):
        W1[:, u], b1[u] = 0.0, -1.0
    counts, stats, mask = HR.probe_ref((W1, b1, W2, b2, W3, b3), S, "fp16")
    assert counts[1] == 5 and counts[3] == 0 and counts[4] == 0
    assert mask[0].tolist() == [(1 << 0) | (1 << 5) | (1 << 17), 0, 1 << 0, 1 << 31]
    ge = HR.probe_ref((W1, b1, W2, b2, W3, b3), S, "fp16", relu_ge=True)[0]
    assert ge[1] == 2  # z == 0 counts as alive under >=
    W3[:, 0] = 65504.0
    b3[2] = np.nan
    counts, stats, _ = HR.probe_ref((W1, b1, W2, b2, W3, b3), S, "fp16")
    assert counts[4] == 256  # column 0 inf, column 2 NaN, on all 128 rows
    z1, z2, q = HR.forward((W1, b1, W2, b2, W3, b3), S, "fp16")
    assert np.isposinf(q[:, 0]).all() and np.isnan(q[:, 2]).all()
    assert stats[4] == np.abs(q[:, [1, 3]]).max() > 0


def test_layer_sums_ref_segments():
    """A lone value per variable lands in that variable's sum alone, for both
    widths, through keras_to_kernel."""
    from dmdqn_amd.agent import keras_to_kernel
    for Hd in (64, 128):
        sl = XF.block_slices(Hd)
        k = np.zeros((1, XF.n_params(Hd)), np.float32)
        for i, name in enumerate(HR.VARIABLES):
            o, sh = sl[name]
            k[0, o] = 3.0
            k[0, o + int(np.prod(sh)) - 1] = -0.75 if int(np.prod(sh)) > 1 else 3.0
        out = HR.layer_sums_ref(keras_to_kernel(k, Hd), Hd)
        np.testing.assert_array_equal(out, np.full((1, 6), 9.0 + 0.5625))


# --------------------------------------------------------------------------- ABI
def test_abi_is_additive(lib):
    import torch  # noqa: F401
    from dmdqn_amd import _lib, ops
    assert lib.dmdqn_version() == 4
    for name, op in (("dmdqn_net_probe", "net_probe"), ("dmdqn_layer_norms", "layer_norms")):
        assert hasattr(lib, name)
        assert name in _lib.SIGNATURES
        assert ops.ENTRY_POINTS[name] == op
    D = ops.load()
    sch = D.net_probe.default._schema
    assert sch.name == "dmdqn::net_probe"
    assert [a.name for a in sch.arguments] == ["ring_s", "idx", "params", "start", "hidden",
                                               "precision", "counts", "stats", "dead_mask"]
    by_name = {a.name: a for a in sch.arguments}
    for out in ("counts", "stats", "dead_mask"):
        assert by_name[out].alias_info is not None and by_name[out].alias_info.is_write
    for inp in ("ring_s", "idx", "params"):
        assert by_name[inp].alias_info is None  # the probe only reads
    assert by_name["dead_mask"].has_default_value() and by_name["dead_mask"].default_value is None
    sch = D.layer_norms.default._schema
    assert sch.name == "dmdqn::layer_norms"
    assert [a.name for a in sch.arguments] == ["x", "y", "eps", "mode", "hidden", "out"]
    by_name = {a.name: a for a in sch.arguments}
    assert by_name["out"].alias_info.is_write and by_name["x"].alias_info is None


def _probe_args():
    """A dmdqn_probe_args that passes every host check (dummy pointers: a
    refusal returns before any of them is dereferenced)."""
    from dmdqn_amd._lib import CProbe
    from dmdqn_amd.agent import n_params
    a = CProbe()
    a.NA, a.cap, a.start, a.batch, a.hidden, a.precision, a.P = 2, 302, 7, 128, 128, 1, n_params(128)
    for f in ["ring_s", "idx", "params", "counts", "stats", "dead_mask"]:
        setattr(a, f, 4096)
    return a


def test_host_refusals_of_the_probe_entry(lib):
    """Each refusal returns DMDQN_EINVAL (-1) before any launch, and
    dmdqn_last_error() names the entry point."""
    from dmdqn_amd.agent import n_params
    entry = b"dmdqn_net_probe"

    def refused(a, word):
        assert lib.dmdqn_net_probe(ctypes.byref(a), None) == -1
        msg = lib.dmdqn_last_error()
        assert entry in msg and word in msg, msg

    for f in ["ring_s", "idx", "params", "counts", "stats"]:
        a = _probe_args()
        setattr(a, f, None)
        refused(a, b"null")
    assert lib.dmdqn_net_probe(None, None) == -1
    assert entry in lib.dmdqn_last_error()
    for field, values, word in (("NA", (0, -3), b"NA="), ("batch", (64, 256), b"batch="),
                                ("hidden", (64, 256), b"hidden="),
                                ("P", (n_params(64), n_params(128) - 4), b"P="),
                                ("precision", (0, 3), b"precision"),
                                ("start", (-1, 302, 303), b"start=")):
        for v in values:
            a = _probe_args()
            setattr(a, field, v)
            refused(a, word)


def test_host_refusals_of_the_layer_norms_entry(lib):
    from dmdqn_amd.agent import n_params
    entry = b"dmdqn_layer_norms"
    d = ctypes.c_void_p(4096)
    P = n_params(128)

    def refused(word, x=d, y=d, mode=0, NW=2, P=P, hidden=128, out=d):
        assert lib.dmdqn_layer_norms(x, y, ctypes.c_float(1e-7), mode, NW, P, hidden, out, None) == -1
        msg = lib.dmdqn_last_error()
        assert entry in msg and word in msg, msg

    refused(b"null", x=None)
    refused(b"null", out=None)
    refused(b"null", y=None, mode=1)
    refused(b"mode", mode=2)
    refused(b"mode", mode=-1)
    refused(b"NW=", NW=0)
    refused(b"hidden=", hidden=256)
    refused(b"P=", P=n_params(64))
    refused(b"P=", P=n_params(128), hidden=64)
    refused(b"P=", P=P + 4)


# --------------------------------------------------------------------------- config
def test_config_key_and_validation():
    from dmdqn_amd.agent import AgentConfig, check_health_every
    assert AgentConfig().health_every == 0
    assert AgentConfig.from_dict({"health_every": 25, "unknown": 1}).health_every == 25
    assert check_health_every(0) == 0 and check_health_every(100) == 100
    for bad in (-1, 1.5, "3", None, True, float("nan")):
        with pytest.raises(ValueError, match="health_every"):
            check_health_every(bad)


@pytest.mark.parametrize("kw,word", [
    (dict(precision="fp32"), "fp32"),
    (dict(precision="fp16", shared_params=True), "shared_params"),
    (dict(precision="fp16", nn_layers=[64, 64]), "nn_layers"),
    (dict(precision="fp16", replay_rows="f32"), "float replay rows"),
    (dict(precision="bf16", replay_rows="f32"), "float replay rows")])
def test_agent_refuses_the_probes_limits_before_any_allocation(lib, kw, word):
    """Raised at construction before any device tensor exists (so also on a
    host without a GPU); the message names the limits and what is supported."""
    from dmdqn_amd.agent import AgentConfig, BatchedDQN
    with pytest.raises(ValueError) as e:
        BatchedDQN(2, 2, AgentConfig(health_every=10, **kw), device="cuda")
    msg = str(e.value)
    for w in ("health_every", word, "fp16", "bf16", "int8", "[128, 128]"):
        assert w in msg, (w, msg)
    with pytest.raises(ValueError, match="health_every"):
        BatchedDQN(2, 2, AgentConfig(precision="fp16", health_every=-1), device="cuda")


def test_checkpoint_default():
    """health_every is stored with the config and defaults to 0 for a
    checkpoint saved before it existed; the probe's outputs are not state, so
    a resume may set another value (no format bump)."""
    import dataclasses

    from dmdqn_amd import checkpoint as CK
    from dmdqn_amd.agent import AgentConfig
    assert CK._DEFAULTS["health_every"] == 0 and "health_every" not in CK._AGENT_FIXED
    assert "health" not in CK._AGENT_TENSORS
    assert CK.FORMAT == "dmdqn-ckpt-8"
    d = CK._cfg_dict(AgentConfig(precision="bf16", health_every=50))
    assert d["health_every"] == 50
    assert dataclasses.asdict(AgentConfig.from_dict(d))["health_every"] == 50
    old = {k: v for k, v in d.items() if k != "health_every"}  # saved before the key existed
    assert AgentConfig.from_dict(old).health_every == 0
    CK._check_cfg(old, d, CK._AGENT_FIXED, "agent_cfg")  # loads under any health_every


# --------------------------------------------------------------------------- CLI
@pytest.mark.parametrize("argv,word", [(["--batched", "--health_every", "-1"], "health_every"),
                                       (["--health_every", "5"], "--batched"),
                                       (["--batched", "--precision", "fp32", "--health_every", "5"],
                                        "fp16"),
                                       (["--batched", "--shared", "--health_every", "5"],
                                        "--shared")])
def test_cli_refuses_bad_health_every(monkeypatch, capsys, argv, word):
    from src.scripts import train
    monkeypatch.setattr("sys.argv", ["train.py"] + argv)
    with pytest.raises(SystemExit) as e:
        train.main()
    assert e.value.code == 2 and word in capsys.readouterr().err


def test_cli_passes_health_every_to_the_config():
    from dmdqn_amd.agent import AgentConfig
    from src.scripts.train import AGENT_CONFIG, target_config
    assert "health_every" not in target_config() and "health_every" not in AGENT_CONFIG
    assert AgentConfig.from_dict(target_config(health_every=100)).health_every == 100
    assert AgentConfig.from_dict(target_config()).health_every == 0
