"""Dead-unit recycling (AgentConfig.redo_every; dmdqn_redo) -- everything that
needs no GPU: the draws' known answer, the numpy restatement (redo_ref.py)
against a textbook ReDo on dense matrices, the overlap and streak rules,
function preservation on the exact-forward fixtures, the additive C ABI and its
host refusals, the config keys, the checkpoint's defaults and the CLI flags."""
import ctypes

import numpy as np
import pytest

import exact_fixture as XF
import health_ref as HR
import redo_ref as RR


@pytest.fixture(scope="module")
def lib():
    from dmdqn_amd import build
    build.build(verbose=False)
    from dmdqn_amd import _lib, agent  # noqa: F401  (agent registers the signatures)
    return _lib.load()


# --------------------------------------------------------------------------- the draws
def test_known_answer_and_limits():
    w = RR.fresh(0, 0, 0, 0, 0, range(4), RR.LIM1)
    assert w.dtype == np.float32
    assert w.view(np.uint32).tolist() == [1034035537, 1037434266, 3178239665, 1034311903]
    assert RR.LIM1.view(np.uint32) == 1048899646 and RR.LIM2.view(np.uint32) == 1046328279
    from dmdqn_amd import kernels as K
    assert np.float32(K.REDO_LIM1).view(np.uint32) == 1048899646
    assert np.float32(K.REDO_LIM2).view(np.uint32) == 1046328279
    # every argument of the counter moves the draw
    base = RR.fresh(3, 7, 5, 1, 9, [11], RR.LIM2)[0]
    others = [RR.fresh(4, 7, 5, 1, 9, [11], RR.LIM2)[0], RR.fresh(3, 8, 5, 1, 9, [11], RR.LIM2)[0],
              RR.fresh(3, 7, 6, 1, 9, [11], RR.LIM2)[0], RR.fresh(3, 7, 5, 0, 9, [11], RR.LIM2)[0],
              RR.fresh(3, 7, 5, 1, 10, [11], RR.LIM2)[0], RR.fresh(3, 7, 5, 1, 9, [12], RR.LIM2)[0]]
    assert all(o != base for o in others)


def test_draws_are_never_zero_and_inside_the_limit():
    """t is an odd integer below 2^24 in magnitude times 2^-24: never 0, inside
    (-1, 1), so w = fl32(lim * t) is never 0 and |w| < lim (|t| <= 1 - 2^-24
    and the product rounds to at most lim's predecessor).  The extreme values
    of u24 are checked directly, then a sample of real draws; its mean and
    variance are HeUniform's (0 and lim^2 / 3 = 2 / fan_in)."""
    for lim in (RR.LIM1, RR.LIM2):
        for u24 in (0, 1, (1 << 23) - 1, 1 << 23, (1 << 24) - 1):
            t = np.float32(2 * u24 + 1 - (1 << 24)) * np.float32(2.0 ** -24)
            assert float(t) == (2 * u24 + 1 - (1 << 24)) / 2.0 ** 24  # exact
            w = lim * t
            assert w.dtype == np.float32 and w != 0 and -lim < w < lim
    w = np.concatenate([RR.fresh(0, 3, 2, 1, u, range(128), RR.LIM2) for u in range(128)])
    assert (w != 0).all() and (np.abs(w) < RR.LIM2).all()
    assert (w > 0).any() and (w < 0).any()
    x = w.astype(np.float64) / float(RR.LIM2)
    # 16,384 draws of U(-1, 1): the mean's sd is 0.0045, the variance's 0.0023;
    # six sd each
    assert abs(x.mean()) < 0.027 and abs(x.var() - 1.0 / 3.0) < 0.014
    # lim is sqrt(6 / fan_in) rounded to f32 (relative 2^-24), so lim^2 / 3 is
    # within relative 2^-23 of 2 / fan_in
    for lim, fan_in in ((RR.LIM1, 89.0), (RR.LIM2, 128.0)):
        assert abs(float(lim) ** 2 / 3.0 - 2.0 / fan_in) <= 2.0 ** -23 * 2.0 / fan_in


# --------------------------------------------------------------------------- the restatement
def _random_state(rs, NA=3):
    Pk = XF.n_params(128)
    params = rs.standard_normal((NA, Pk)).astype(np.float32)
    m = (rs.standard_normal((NA, Pk)) * 1e-3).astype(np.float32)
    v = (rs.random_sample((NA, Pk)) * 1e-5 + 1e-9).astype(np.float32)
    return params, m, v


def _textbook_redo(ws, ms, vs, R1, R2, new_w1, new_w2):
    """ReDo as the paper states it, on dense matrices: reinitialise the
    incoming weights and bias of a dormant unit, zero its outgoing weights,
    reset the moments of what was written.  (Incoming first for both layers,
    then outgoing: the rule's "zero wins" on W2[R1, R2].)"""
    W1, b1, W2, b2, W3, b3 = ws
    new = [W1.copy(), b1.copy(), W2.copy(), b2.copy(), W3.copy(), b3.copy()]
    new[0][:, R1], new[1][R1] = new_w1[:, R1], 0.0
    new[2][:, R2], new[3][R2] = new_w2[:, R2], 0.0
    new[2][R1, :] = 0.0
    new[4][R2, :] = 0.0
    wrote = [np.zeros(w.shape, bool) for w in ws]
    wrote[0][:, R1] = wrote[1][R1] = wrote[2][:, R2] = wrote[3][R2] = True
    wrote[2][R1, :] = wrote[4][R2, :] = True
    return new, [np.where(wr, 0.0, m) for m, wr in zip(ms, wrote)], \
        [np.where(wr, 0.0, v) for v, wr in zip(vs, wrote)]


def test_restatement_against_textbook_redo():
    rs = np.random.RandomState(11)
    params, m, v = _random_state(rs)
    R = np.zeros((3, 2, 128), bool)
    R[0, 0, [0, 5, 17, 64, 127]] = True
    R[0, 1, [3, 31, 96]] = True
    R[2, 0, 40] = True
    R[2, 1, 41] = True
    streak = np.zeros((3, 2, 128), np.uint8)
    got = RR.redo_ref(params, m, v, streak, RR.bits_mask(R), 1, seed=9, rnd=77, agent0=12)
    np.testing.assert_array_equal(got[4], RR.bits_mask(R))
    assert got[5].tolist() == [[5, 3], [0, 0], [1, 1]] and not got[3].any()
    for j in range(3):
        new_w1 = np.stack([RR.fresh(9, 77, 12 + j, 0, u, range(89), RR.LIM1)
                           for u in range(128)], axis=1)
        new_w2 = np.stack([RR.fresh(9, 77, 12 + j, 1, u, range(128), RR.LIM2)
                           for u in range(128)], axis=1)
        want = _textbook_redo(XF.split(params[j], 128), XF.split(m[j], 128), XF.split(v[j], 128),
                              R[j, 0], R[j, 1], new_w1, new_w2)
        for k in range(3):
            flat = np.concatenate([a.ravel() for a in want[k]]).astype(np.float32)
            np.testing.assert_array_equal(got[k][j].view(np.int32), flat.view(np.int32))
    # the clean agent keeps every bit; the inputs are not written
    for k, x in enumerate((params, m, v)):
        np.testing.assert_array_equal(got[k][1].view(np.int32), x[1].view(np.int32))
    # b3 is never touched; +0.0 (not -0.0) where written
    sl = XF.block_slices(128)
    o3 = sl["b3"][0]
    np.testing.assert_array_equal(got[0][:, o3:], params[:, o3:])
    changed = got[1].view(np.int32) != m.view(np.int32)
    assert changed.any() and not got[1].view(np.int32)[changed].any()


def test_overlap_rule_zero_wins():
    rs = np.random.RandomState(12)
    params, m, v = _random_state(rs, NA=1)
    R = np.zeros((1, 2, 128), bool)
    R[0, 0, [7, 100]] = True
    R[0, 1, [7, 50]] = True
    got = RR.redo_ref(params, m, v, np.zeros((1, 2, 128), np.uint8), RR.bits_mask(R), 1, 0, 0)
    W1, b1, W2, b2, W3, b3 = XF.split(got[0][0], 128)
    for i in (7, 100):
        assert not W2[i, :].any() and not b1[i]
        for o in (7, 50):
            assert W2[i, o] == 0.0
    keep = np.ones(128, bool)
    keep[[7, 100]] = False
    for o in (7, 50):
        assert (W2[keep, o] != 0).all() and not W3[o, :].any() and not b2[o]
        np.testing.assert_array_equal(W2[keep, o],
                                      RR.fresh(0, 0, 0, 1, o, np.flatnonzero(keep), RR.LIM2))
    M2, V2 = XF.split(got[1][0], 128)[2], XF.split(got[2][0], 128)[2]
    assert not M2[[7, 100], :].any() and not V2[:, [7, 50]].any()


# --------------------------------------------------------------------------- the streak
def test_streak_rule():
    dead = np.array([True, True, False, True])
    s = np.zeros(4, np.uint8)
    # patience 1: a dead unit fires at once and its streak returns to 0
    s1, f1 = RR.streak_step(s, dead, 1)
    assert f1.tolist() == dead.tolist() and not s1.any()
    # patience 3: fires on the third dead probe in a row; a live probe resets
    s, fired = np.zeros(4, np.uint8), []
    for d in ([1, 1, 1, 1], [1, 1, 0, 1], [1, 0, 1, 1], [1, 1, 1, 1], [1, 1, 1, 0]):
        s, f = RR.streak_step(s, np.array(d, bool), 3)
        fired.append(f.tolist())
    assert fired == [[False] * 4, [False] * 4, [True, False, False, True],
                     [False] * 4, [False, False, True, False]]
    assert s.tolist() == [2, 2, 0, 0]  # reset after firing, then counting again
    # patience 255: 254 dead probes do not fire, the 255th does; saturation at
    # 255 never wraps (a streak of 255 under a dead probe stays 255 before the
    # compare)
    s = np.zeros(1, np.uint8)
    for k in range(254):
        s, f = RR.streak_step(s, np.array([True]), 255)
        assert not f[0] and s[0] == k + 1
    s, f = RR.streak_step(s, np.array([True]), 255)
    assert f[0] and s[0] == 0
    s, f = RR.streak_step(np.array([255], np.uint8), np.array([True]), 255)
    assert f[0] and s[0] == 0
    s, f = RR.streak_step(np.array([255], np.uint8), np.array([False]), 255)
    assert not f[0] and s[0] == 0
    # mask words <-> bits
    bits = np.zeros((2, 128), bool)
    bits[0, [0, 31, 32, 127]] = True
    words = RR.bits_mask(bits)
    assert words[0].tolist() == [(1 << 0) | (1 << 31), 1, 0, 1 << 31] and not words[1].any()
    np.testing.assert_array_equal(RR.mask_bits(words), bits)


# --------------------------------------------------------------------------- function preservation
def _dead_nets(fx):
    """test_gpu_health._mutated_nets' dead units, agent 0's only (no NaN agent)."""
    sl = XF.block_slices(fx.H)
    nets = fx.online.astype(np.float32).copy()

    def var(j, name):
        o, sh = sl[name]
        return nets[j, o:o + int(np.prod(sh))].reshape(sh)
    for u in (0, 17, 127):
        var(0, "W1")[:, u] = 0.0
        var(0, "b1")[u] = 0.0
    for u in (5, 64):
        var(0, "W1")[:, u] = 0.0
        var(0, "b1")[u] = -1.0
    for u in (3, 31, 96):
        var(0, "W2")[:, u] = 0.0
        var(0, "b2")[u] = 0.0
    return nets


def _forward_after(ws, X, precision, R1, R2):
    """(z2 of the units outside R2, q) of a recycled net on exact inputs.  The
    fresh weights are not dyadic, so the exact dense layer is taken over what
    is left once the rows that the rule zeroed are dropped -- asserted zero
    here, on finite inputs, so dropping them changes no sum: a term x * 0 is
    +-0 in any order."""
    rnd = XF._rnd16(precision)
    W1, b1, W2, b2, W3, b3 = (np.asarray(w, np.float64) for w in ws)
    k1, k2 = ~R1, ~R2
    assert not W2[R1, :].any() and not W3[R2, :].any()
    z1_fresh = X @ W1[:, R1] + b1[R1]          # whatever the fresh units give,
    assert np.isfinite(z1_fresh).all()         # it is finite
    z1 = XF._exact_dense(X, W1[:, k1], b1[k1], rnd, "layer 1")[0]
    h1 = np.maximum(z1, 0)
    z2_fresh = h1 @ W2[np.ix_(k1, R2)] + b2[R2]
    assert np.isfinite(z2_fresh).all()
    z2 = XF._exact_dense(h1, W2[np.ix_(k1, k2)], b2[k2], rnd, "layer 2")[0]
    q = XF._exact_dense(np.maximum(z2, 0), W3[k2, :], b3, rnd, "layer 3")[0]
    return z2, q


@pytest.mark.parametrize("name", ["f16", "bf16"])
def test_function_is_preserved_on_the_probed_batch(name):
    fx = XF.fixture(name)
    nets = _dead_nets(fx)
    S = fx.batch(0)[0]
    before = XF.split(nets[0].astype(np.float64), fx.H)
    z1, z2, q = HR.forward(before, S, fx.precision)
    mask = HR.probe_ref(before, S, fx.precision)[2]
    R = RR.mask_bits(mask)
    assert np.flatnonzero(R[0]).tolist() == [0, 5, 17, 64, 127]
    assert np.flatnonzero(R[1]).tolist() == [3, 31, 96]
    masks = np.zeros((fx.NA, 2, 4), np.uint32)
    masks[0] = mask
    zeros = np.zeros_like(nets)
    got = RR.redo_ref(nets, zeros, zeros, np.zeros((fx.NA, 2, 128), np.uint8), masks, 1,
                      seed=fx.seed, rnd=1)
    assert got[5].tolist() == [[5, 3]] + [[0, 0]] * (fx.NA - 1)
    np.testing.assert_array_equal(got[0][1:], nets[1:])
    after = XF.split(got[0][0].astype(np.float64), fx.H)
    assert (after[0][:, R[0]] != 0).all() and (after[2][np.ix_(~R[0], R[1])] != 0).all()
    z2_after, q_after = _forward_after(after, S, fx.precision, R[0], R[1])
    assert (q_after == q).all()
    assert (z2_after == z2[:, ~R[1]]).all()


# --------------------------------------------------------------------------- ABI
def test_abi_is_additive(lib):
    import torch  # noqa: F401
    from dmdqn_amd import _lib, build, ops
    assert lib.dmdqn_version() == 4
    assert hasattr(lib, "dmdqn_redo") and "dmdqn_redo" in _lib.SIGNATURES
    assert ops.ENTRY_POINTS["dmdqn_redo"] == "redo"
    assert build.KERNEL_SOURCES["redo"][0] == "redo.hip" and len(build.source_digest("redo")) == 16
    sch = ops.load().redo.default._schema
    assert sch.name == "dmdqn::redo"
    assert [a.name for a in sch.arguments] == [
        "dead_mask", "streak", "params", "adam_m", "adam_v", "hidden", "agent0", "seed", "round",
        "patience", "lim1", "lim2", "recycled", "n_recycled"]
    by_name = {a.name: a for a in sch.arguments}
    for out in ("streak", "params", "adam_m", "adam_v", "recycled", "n_recycled"):
        assert by_name[out].alias_info is not None and by_name[out].alias_info.is_write
    assert by_name["dead_mask"].alias_info is None
    # the ctypes struct is the header's: 5 int32, a uint32, a uint64 on an 8-B
    # boundary, two floats, seven pointers
    assert _lib.CRedo.seed.offset == 24 and _lib.CRedo.lim1.offset == 32
    assert _lib.CRedo.dead_mask.offset == 40 and ctypes.sizeof(_lib.CRedo) == 96


def redo_args():
    """A dmdqn_redo_args that passes every host check (dummy pointers: a
    refusal returns before any of them is dereferenced)."""
    from dmdqn_amd import kernels as K
    from dmdqn_amd._lib import CRedo
    from dmdqn_amd.agent import n_params
    a = CRedo()
    a.NA, a.P, a.hidden, a.agent0, a.patience, a.round, a.seed = 2, n_params(128), 128, 0, 1, 5, 3
    a.lim1, a.lim2 = K.REDO_LIM1, K.REDO_LIM2
    for f in REDO_POINTERS:
        setattr(a, f, 4096)
    return a


REDO_POINTERS = ["dead_mask", "streak", "params", "adam_m", "adam_v", "recycled", "n_recycled"]


def check_host_refusals(lib):
    """Each refusal returns DMDQN_EINVAL (-1) before any launch, and
    dmdqn_last_error() names the entry point and the argument."""
    from dmdqn_amd.agent import n_params
    entry = b"dmdqn_redo"

    def refused(a, word):
        assert lib.dmdqn_redo(ctypes.byref(a), None) == -1
        msg = lib.dmdqn_last_error()
        assert entry in msg and word in msg, msg

    for f in REDO_POINTERS:
        a = redo_args()
        setattr(a, f, None)
        refused(a, b"null")
    assert lib.dmdqn_redo(None, None) == -1
    assert entry in lib.dmdqn_last_error()
    for field, values, word in (("NA", (0, -3), b"NA="), ("hidden", (64, 256), b"hidden="),
                                ("P", (n_params(64), n_params(128) - 4), b"P="),
                                ("patience", (0, -1, 256), b"patience="),
                                ("agent0", (-1, -(1 << 31)), b"agent0=")):
        for v in values:
            a = redo_args()
            setattr(a, field, v)
            refused(a, word)
    a = redo_args()
    a.params = 4096 + 4
    refused(a, b"alignment")


def test_host_refusals(lib):
    check_host_refusals(lib)


# --------------------------------------------------------------------------- config
def test_config_keys_and_validation():
    from dmdqn_amd.agent import AgentConfig, check_redo
    assert AgentConfig().redo_every == 0 and AgentConfig().redo_patience == 1
    cfg = AgentConfig.from_dict({"redo_every": 25, "redo_patience": 3, "unknown": 1})
    assert cfg.redo_every == 25 and cfg.redo_patience == 3
    assert check_redo(0, 1) == (0, 1) and check_redo(1000, 255) == (1000, 255)
    for bad in (-1, 1.5, "3", None, True, float("nan")):
        with pytest.raises(ValueError, match="redo_every"):
            check_redo(bad, 1)
    for bad in (0, 256, -1, 1.5, "3", None, True):
        with pytest.raises(ValueError, match="redo_patience"):
            check_redo(10, bad)


@pytest.mark.parametrize("kw,word", [
    (dict(precision="fp32"), "fp32"),
    (dict(precision="fp16", shared_params=True), "shared_params"),
    (dict(precision="fp16", nn_layers=[64, 64]), "nn_layers"),
    (dict(precision="bf16", replay_rows="f32"), "float replay rows")])
def test_agent_refuses_the_probes_limits_before_any_allocation(lib, kw, word):
    from dmdqn_amd.agent import AgentConfig, BatchedDQN
    with pytest.raises(ValueError) as e:
        BatchedDQN(2, 2, AgentConfig(redo_every=10, **kw), device="cuda")
    msg = str(e.value)
    for w in ("redo_every", word, "fp16", "bf16", "int8", "[128, 128]"):
        assert w in msg, (w, msg)
    with pytest.raises(ValueError, match="redo_patience"):
        BatchedDQN(2, 2, AgentConfig(precision="fp16", redo_every=5, redo_patience=0),
                   device="cuda")


def test_checkpoint_defaults():
    """Both keys are fixed (the schedule and the patience decide which units
    are rewritten) and default to off for a checkpoint saved before them."""
    from dmdqn_amd import checkpoint as CK
    from dmdqn_amd.agent import AgentConfig
    assert CK._DEFAULTS["redo_every"] == 0 and CK._DEFAULTS["redo_patience"] == 1
    assert "redo_every" in CK._AGENT_FIXED and "redo_patience" in CK._AGENT_FIXED
    assert CK.FORMAT == "dmdqn-ckpt-8"
    d = CK._cfg_dict(AgentConfig(precision="bf16", redo_every=50, redo_patience=2))
    assert d["redo_every"] == 50 and d["redo_patience"] == 2
    off = CK._cfg_dict(AgentConfig(precision="bf16"))
    old = {k: v for k, v in off.items() if not k.startswith("redo_")}  # saved before the keys
    assert AgentConfig.from_dict(old).redo_every == 0
    CK._check_cfg(old, off, CK._AGENT_FIXED, "agent_cfg")  # loads as before
    with pytest.raises(ValueError, match="redo_every"):
        CK._check_cfg(old, d, CK._AGENT_FIXED, "agent_cfg")
    with pytest.raises(ValueError, match="redo_patience"):
        CK._check_cfg(CK._cfg_dict(AgentConfig(precision="bf16", redo_every=50)), d,
                      CK._AGENT_FIXED, "agent_cfg")


# --------------------------------------------------------------------------- CLI
@pytest.mark.parametrize("argv,word", [
    (["--batched", "--redo_every", "-1"], "redo_every"),
    (["--batched", "--redo_every", "5", "--redo_patience", "0"], "redo_patience"),
    (["--redo_every", "5"], "--batched"),
    (["--batched", "--precision", "fp32", "--redo_every", "5"], "fp16"),
    (["--batched", "--shared", "--redo_every", "5"], "--shared")])
def test_cli_refuses_bad_redo_flags(monkeypatch, capsys, argv, word):
    from src.scripts import train
    monkeypatch.setattr("sys.argv", ["train.py"] + argv)
    with pytest.raises(SystemExit) as e:
        train.main()
    assert e.value.code == 2 and word in capsys.readouterr().err


def test_cli_passes_the_keys_to_the_config():
    from dmdqn_amd.agent import AgentConfig
    from src.scripts.train import AGENT_CONFIG, target_config
    assert "redo_every" not in target_config() and "redo_every" not in AGENT_CONFIG
    cfg = AgentConfig.from_dict(target_config(redo_every=100, redo_patience=4))
    assert cfg.redo_every == 100 and cfg.redo_patience == 4
    assert AgentConfig.from_dict(target_config()).redo_every == 0
