"""Global-norm gradient clipping (AgentConfig.global_clipnorm, Keras's
Adam(global_clipnorm=...)) -- everything that needs no GPU: the numpy
restatement of the rule (clip_ref.py) against clip-by-global-norm written with
torch ops, its corner cases (NaN / inf, norm == 0, a clip whose
fl32(clip * fl32(1 / clip)) is not 1), the additive C ABI and its host
refusals, the operator's schema, the config key, the checkpoint's config rule
and --global_clipnorm."""
import ctypes
import math

import numpy as np
import pytest

import clip_ref as CR

f32 = np.float32


@pytest.fixture(scope="module")
def lib():
    from dmdqn_amd import build
    build.build(verbose=False)
    from dmdqn_amd import _lib, agent  # noqa: F401  (agent registers the signatures)
    return _lib.load()


def _bits(x):
    return np.asarray(x, dtype=np.float32).view(np.int32)


# --------------------------------------------------------------------------- the rule
@pytest.mark.parametrize("seed", range(6))
def test_restatement_is_textbook_clip_by_global_norm(seed):
    """clip_ref against g * clip / max(norm, clip) with torch ops in f64: the
    norm to f32 rounding (it is the f32 rounding of the exact f64 norm), g' to
    a few f32 roundings (1 / norm, the min, clip * ., g * scale: 4 ops of 2^-24
    each)."""
    torch = pytest.importorskip("torch")
    rs = np.random.RandomState(seed)
    n = int(rs.randint(1, 5000))
    g = (rs.standard_normal(n) * 10.0 ** rs.uniform(-3, 2)).astype(np.float32)
    tg = torch.from_numpy(g).double()
    tnorm = torch.linalg.vector_norm(tg)
    for clip in (f32(0.5) * f32(tnorm), f32(2.0) * f32(tnorm), f32(1.0)):
        norm, gc = CR.clip_gradient(g, clip)
        assert norm.dtype == np.float32 and gc.dtype == np.float32
        assert _bits(norm) == _bits(tnorm.float().numpy())
        want = (tg * (float(clip) / torch.clamp(tnorm, min=float(clip)))).numpy()
        assert np.all(np.abs(gc.astype(np.float64) - want) <= 4 * 2.0 ** -24 * np.abs(want))
        if float(tnorm) > float(clip):  # clipped: the new norm is the clip
            assert abs(float(CR.global_norm(gc)) / float(clip) - 1.0) < 1e-6


def test_non_finite_gradients_give_a_nan_scale():
    g = np.ones(16, np.float32)
    for bad in (np.inf, -np.inf, np.nan):
        h = g.copy()
        h[5] = bad
        norm, gc = CR.clip_gradient(h, f32(1.0))
        assert not np.isfinite(norm)
        assert np.isnan(gc).all()  # every entry, the finite ones too
        p, m, v = CR.keras_adam(g, g, g, gc, 1e-3, 0.1, 0.001, 1e-7)
        assert np.isnan(p).all() and np.isnan(m).all() and np.isnan(v).all()
    # (inf - inf, not the min, makes the NaN: the min alone would give 0)
    assert np.isnan(CR.clip_scale(f32(np.inf), f32(1.0)))


def test_zero_norm_takes_one_over_clip():
    for clip in (f32(0.1), f32(1.0), f32(40.0)):
        norm, gc = CR.clip_gradient(np.zeros(8, np.float32), clip)
        assert norm == 0.0 and _bits(norm) == 0
        assert _bits(CR.clip_scale(norm, clip)) == _bits(clip * (f32(1) / clip))
        assert not gc.any()


def test_a_clip_whose_unclipped_scale_is_not_one_exists():
    """fl32(clip * fl32(1 / clip)) is 1 for most clip values and 1 - 2^-24 for
    some: an unclipped gradient is still multiplied by it, as in Keras."""
    ones, others = [], []
    for k in range(1, 400):
        clip = f32(k) / f32(8)
        s = CR.clip_scale(f32(0.0), clip)
        (ones if s == f32(1) else others).append((float(clip), s))
    assert ones and others
    assert len(ones) > len(others)
    for clip, s in others:
        assert _bits(s) == _bits(f32(1) - f32(2.0 ** -24)), (clip, s)
    clip = f32(others[0][0])
    g = np.asarray([0.5, -0.25, 3.0], np.float32) * f32(1e-3)
    norm, gc = CR.clip_gradient(g, clip)
    assert norm < clip and not np.array_equal(_bits(gc), _bits(g))


def test_boundary_margin():
    assert CR.boundary_margin(0.0) == math.inf and CR.boundary_margin(math.inf) == math.inf
    assert 0.2 * 2.0 ** -24 < CR.boundary_margin(4.0) <= 0.5 * 2.0 ** -23  # sqrt exact: half an ulp
    n = f32(3.0)
    mid = (float(n) + float(np.nextafter(n, f32(4)))) / 2.0
    assert CR.boundary_margin(mid * mid) < 2.0 ** -50
    assert CR.boundary_margin(mid * mid * (1 + 2.0 ** -30)) > 2.0 ** -33


# --------------------------------------------------------------------------- ABI
def test_abi_is_additive(lib):
    import torch  # noqa: F401
    from dmdqn_amd import _lib, ops
    assert lib.dmdqn_version() == 4
    assert hasattr(lib, "dmdqn_adam_agents_clip")
    assert "dmdqn_adam_agents_clip" in _lib.SIGNATURES
    assert ops.ENTRY_POINTS["dmdqn_adam_agents_clip"] == "learn_step_clip"
    D = ops.load()
    sch = D.learn_step_clip.default._schema
    assert sch.name == "dmdqn::learn_step_clip"
    names = [a.name for a in sch.arguments]
    base = [a.name for a in D.learn_step_hp.default._schema.arguments]
    assert names == base + ["clip", "gnorm"]
    by_name = {a.name: a for a in sch.arguments}
    assert not by_name["grad"].has_default_value()  # required here, optional in learn_step_hp
    assert not by_name["clip"].has_default_value()
    assert by_name["gnorm"].has_default_value() and by_name["gnorm"].default_value is None


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


def test_host_refusals_of_the_clip_entry(lib):
    """Each refusal returns DMDQN_EINVAL (-1) before any launch, and
    dmdqn_last_error() names the entry point."""
    from dmdqn_amd.agent import CHParams
    entry = b"dmdqn_adam_agents_clip"
    dummy = ctypes.c_void_p(4096)

    def call(a, clip=1.0, grad=dummy, hp=None):
        return lib.dmdqn_adam_agents_clip(ctypes.byref(a), None if hp is None else ctypes.byref(hp),
                                          grad, ctypes.c_float(clip), None, None)

    for clip in (0.0, -1.0, float("inf"), float("-inf"), float("nan")):
        assert call(_learn_args(), clip) == -1, clip
        msg = lib.dmdqn_last_error()
        assert entry in msg and b"clip" in msg, msg
    for precision in (0, 3):
        a = _learn_args()
        a.precision = precision
        assert call(a) == -1
        msg = lib.dmdqn_last_error()
        assert entry in msg and b"precision" in msg, msg
    from dmdqn_amd.agent import n_params
    for P in (n_params(64), n_params(128) - 4, n_params(128) + 4):
        a = _learn_args()
        a.P = P
        assert call(a) == -1
        msg = lib.dmdqn_last_error()
        assert entry in msg and b"P=" in msg, msg
    assert call(_learn_args(), grad=None) == -1
    msg = lib.dmdqn_last_error()
    assert entry in msg and b"null" in msg, msg
    # what dmdqn_adam_agents_hp refuses
    assert call(_learn_args(), hp=CHParams(None, None, 4096, None, 1.0, 1.0)) == -1
    assert entry in lib.dmdqn_last_error() and b"go together" in lib.dmdqn_last_error()
    assert call(_learn_args(), hp=CHParams(4096, None, None, None, 0.0, 0.5)) == -1
    assert entry in lib.dmdqn_last_error() and b"adam_s" in lib.dmdqn_last_error()
    a = _learn_args()
    a.tau = 1.5
    assert call(a) == -1
    assert entry in lib.dmdqn_last_error() and b"tau" in lib.dmdqn_last_error()
    assert lib.dmdqn_adam_agents_clip(None, None, dummy, ctypes.c_float(1.0), None, None) == -1


# --------------------------------------------------------------------------- config
def test_config_key_and_validation():
    from dmdqn_amd.agent import AgentConfig, check_clipnorm
    assert AgentConfig().global_clipnorm == 0.0
    cfg = AgentConfig.from_dict({"global_clipnorm": 2.5, "unknown": 1})
    assert cfg.global_clipnorm == 2.5
    assert check_clipnorm(0) == 0.0 and check_clipnorm(0.0) == 0.0 and check_clipnorm("3") == 3.0
    for bad in (-1.0, float("nan"), float("inf"), -0.5, "x", None, 1e-60, 1e60):
        with pytest.raises(ValueError, match="global_clipnorm"):
            check_clipnorm(bad)


@pytest.mark.parametrize("kw", [dict(precision="fp32"), dict(precision="fp16", shared_params=True),
                                dict(precision="fp16", replay_rows="f32"),
                                dict(precision="bf16", replay_rows="f32")])
def test_agent_refuses_the_split_learns_limits_before_any_allocation(lib, kw):
    """Raised at construction before any device tensor exists (so also on a
    host without a GPU); the message names the limits and what is supported."""
    from dmdqn_amd.agent import AgentConfig, BatchedDQN
    with pytest.raises(ValueError) as e:
        BatchedDQN(2, 2, AgentConfig(global_clipnorm=1.0, **kw), device="cuda")
    msg = str(e.value)
    for word in ("global_clipnorm", "fp32", "shared_params", "float replay rows", "fp16", "bf16",
                 "int8"):
        assert word in msg, (word, msg)
    with pytest.raises(ValueError, match="global_clipnorm"):
        BatchedDQN(2, 2, AgentConfig(precision="fp16", global_clipnorm=-1.0), device="cuda")


def test_checkpoint_fixes_global_clipnorm():
    import dataclasses

    from dmdqn_amd import checkpoint as CK
    from dmdqn_amd.agent import AgentConfig
    assert "global_clipnorm" in CK._AGENT_FIXED and CK._DEFAULTS["global_clipnorm"] == 0.0
    assert CK.FORMAT == "dmdqn-ckpt-8"  # no format bump
    key = ["global_clipnorm"]
    old = {}  # saved before clipping existed: it ran without
    CK._check_cfg(old, {"global_clipnorm": 0.0}, key, "agent_cfg")
    with pytest.raises(ValueError, match="global_clipnorm"):
        CK._check_cfg(old, {"global_clipnorm": 5.0}, key, "agent_cfg")
    with pytest.raises(ValueError, match="global_clipnorm"):
        CK._check_cfg({"global_clipnorm": 5.0}, {"global_clipnorm": 1.0}, key, "agent_cfg")
    CK._check_cfg({"global_clipnorm": 5.0}, {"global_clipnorm": 5.0}, key, "agent_cfg")
    # the value round-trips through what a checkpoint stores
    d = CK._cfg_dict(AgentConfig(global_clipnorm=5.0))
    assert d["global_clipnorm"] == 5.0
    assert dataclasses.asdict(AgentConfig.from_dict(d))["global_clipnorm"] == 5.0


# --------------------------------------------------------------------------- CLI
@pytest.mark.parametrize("argv,word", [(["--batched", "--global_clipnorm", "-1"], "global_clipnorm"),
                                       (["--batched", "--global_clipnorm", "nan"], "global_clipnorm"),
                                       (["--batched", "--global_clipnorm", "x"], "global_clipnorm"),
                                       (["--global_clipnorm", "1"], "--batched"),
                                       (["--batched", "--precision", "fp32", "--global_clipnorm",
                                         "1"], "fp16"),
                                       (["--batched", "--shared", "--global_clipnorm", "1"],
                                        "--shared")])
def test_cli_refuses_bad_global_clipnorm(monkeypatch, capsys, argv, word):
    from src.scripts import train
    monkeypatch.setattr("sys.argv", ["train.py"] + argv)
    with pytest.raises(SystemExit) as e:
        train.main()
    assert e.value.code == 2 and word in capsys.readouterr().err


def test_cli_passes_global_clipnorm_to_the_config():
    from dmdqn_amd.agent import AgentConfig
    from src.scripts.train import AGENT_CONFIG, target_config
    assert "global_clipnorm" not in target_config() and "global_clipnorm" not in AGENT_CONFIG
    cfg = target_config(global_clipnorm=10.0)
    assert cfg["global_clipnorm"] == 10.0
    assert AgentConfig.from_dict(cfg).global_clipnorm == 10.0
    assert AgentConfig.from_dict(target_config()).global_clipnorm == 0.0
