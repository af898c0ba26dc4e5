"""Rule-based controllers without a GPU: the numpy restatement (rule_ref.py)
against a movement-level brute force, the shared fixture's coverage, the known
answers of include/dmdqn.h, the host-side refusals of dmdqn_act_rule and the
behaviour policy's configuration checks."""
import ctypes
import os
import re

import numpy as np
import pytest

import rule_ref as RR
from conftest import ROOT

GRIDS = [(1, 1), (1, 3), (3, 1), (2, 2), (3, 3)]


# ---------------------------------------------------------------- the restatement
@pytest.mark.parametrize("R,C", GRIDS)
def test_ref_equals_brute_force(R, C):
    """Literal lane groups and out-directions against the phase masks and
    movement(), row by row, on k_observe-shaped random observations."""
    rng = np.random.default_rng(100 * R + C)
    obs = RR.random_obs(rng, R, C, 6).reshape(-1, RR.OBS_DIM)
    for rule in (RR.LONGEST_QUEUE, RR.MAX_PRESSURE):
        act, sc = RR.act_rule(obs, rule)
        for i, row in enumerate(obs):
            want = RR.brute_scores(row, rule)
            assert sc[i].tolist() == want, (rule, i)
            assert act[i] == want.index(max(want))


def test_ref_brute_force_on_arbitrary_rows():
    """Rows that are no observation of any grid (every flag pattern, negative
    values, flags that are neither 0 nor 1): the two still agree."""
    rng = np.random.default_rng(7)
    obs = rng.integers(-127, 128, size=(400, RR.OBS_DIM)).astype(np.float32)
    obs[:, 17:21] = rng.integers(-1, 3, size=(400, 4))
    for rule in (RR.LONGEST_QUEUE, RR.MAX_PRESSURE):
        sc = RR.scores(obs, rule)
        for i, row in enumerate(obs):
            assert sc[i].tolist() == RR.brute_scores(row, rule)


def test_groups_partition_and_out_directions():
    lanes = [lane for g in RR.GROUPS for lane in g]
    assert sorted(lanes) == [(d, k) for d in range(4) for k in range(3)]
    for d in range(4):
        h = d ^ 1
        assert RR.lane_out(d, 0) == RR.lane_out(d, 1) == h
        assert RR.lane_out(d, 2) == RR.right_of(h) ^ 1


def test_scores_stay_inside_int32():
    """|v| <= 127: the largest |score| is 12 * 127 own + 4 * 3 * 127 downstream."""
    obs = np.full((1, RR.OBS_DIM), 127, dtype=np.float32)
    obs[:, 17:21] = 1
    assert np.abs(RR.scores(obs, RR.MAX_PRESSURE)).max() <= 24 * 127 < 2 ** 31


def test_fixture_meets_its_coverage():
    parts = RR.check_fixture(RR.fixture_parts())
    assert [(r, c) for r, c, _ in parts] == [(r, c) for r, c, _ in RR.FIXTURE_GRIDS]
    # a fixture that lacks a condition is refused (here: no 3x3 grid, so no
    # agent with 3 or 4 neighbours)
    with pytest.raises(ValueError, match="neighbours"):
        RR.check_fixture(parts[:3])


def test_known_answers():
    for row, rule, want_sc, want_a in RR.known_rows():
        act, sc = RR.act_rule(row[None], rule)
        assert sc[0].tolist() == want_sc and int(act[0]) == want_a
        assert RR.brute_scores(row, rule) == want_sc


def test_header_states_the_rule_and_its_known_answers():
    txt = open(os.path.join(ROOT, "include", "dmdqn.h")).read()
    sec = txt[txt.index("rule-based controllers"):]
    assert "#define DMDQN_RULE_LONGEST_QUEUE 0" in sec
    assert "#define DMDQN_RULE_MAX_PRESSURE 1" in sec
    for literal in ("0x11BB, 0x11DD, 0xBB11, 0xDD11", "G0 = {n0, n1, s0, s1}", "G1 = {n2, s2}",
                    "G2 = {e0, e1, w0, w1}", "G3 = {e2, w2}", "0 15 0 0", "4 0 3 0", "-18 0 9 -15",
                    "Not in this version", "minimum green"):
        assert literal in sec, literal
    assert re.search(r"int dmdqn_act_rule\(int R, int C, int E, int rule, const float \*obs", sec)


def test_kernel_derives_its_groups_at_compile_time():
    """rule.hip takes the lane groups from sim.hpp's green_mask in constant
    expressions and asserts the partition; it is one of build.py's sources."""
    from dmdqn_amd import build
    src = open(os.path.join(ROOT, "dmdqn_amd", "csrc", "rule.hip")).read()
    assert '#include "sim.hpp"' in src and "green_mask(3 * a)" in src
    assert re.search(r"static_assert\(groups_partition\(\)", src)
    assert "__shared__" not in src and "atomic" not in src.replace("no atomics", "")
    assert build.KERNEL_SOURCES["rule"][0] == "rule.hip" and len(build.source_digest("rule")) == 16
    assert any(p.endswith("rule.hip") for p in build._sources())


# ---------------------------------------------------------------- the C entry point
@pytest.fixture(scope="module")
def lib():
    from dmdqn_amd import build
    build.build(verbose=False)
    from dmdqn_amd import _lib
    return _lib.load()


def test_host_refusals_without_gpu(lib):
    """Every refused argument returns DMDQN_EINVAL with its message, before
    anything is launched (no device here at all)."""
    from dmdqn_amd import _lib
    assert "dmdqn_act_rule" in _lib.SIGNATURES
    p = ctypes.c_void_p(64)  # never dereferenced: the checks fail first
    f = lib.dmdqn_act_rule
    cases = [((0, 2, 1, 0, p, p, None, None), b"must be >= 1"),
             ((2, 0, 1, 0, p, p, None, None), b"must be >= 1"),
             ((2, 2, 0, 1, p, p, None, None), b"must be >= 1"),
             ((2, 2, -3, 1, p, p, None, None), b"must be >= 1"),
             ((2 ** 15, 2 ** 15, 4, 1, p, p, None, None), b"beyond int32"),
             ((2, 2, 1, 2, p, p, None, None), b"unknown rule 2"),
             ((2, 2, 1, -1, p, p, None, None), b"unknown rule -1"),
             ((2, 2, 1, 0, None, p, None, None), b"null obs or actions"),
             ((2, 2, 1, 1, p, None, p, None), b"null obs or actions")]
    for args, msg in cases:
        assert f(*args) == -1, args
        err = lib.dmdqn_last_error()
        assert b"dmdqn_act_rule" in err and msg in err, (args, err)
    assert lib.dmdqn_version() == 4  # additive


def test_operator_registered_and_rule_names(lib):
    import torch
    from dmdqn_amd import kernels as K, ops
    D = ops.load()
    assert ops.ENTRY_POINTS["dmdqn_act_rule"] == "act_rule"
    assert D.act_rule.default._schema.name == "dmdqn::act_rule"
    assert K.rule_id("longest_queue") == 0 and K.rule_id("max_pressure") == 1 and K.rule_id(1) == 1
    with pytest.raises(ValueError, match="unknown rule"):
        K.rule_id("fifo")
    with pytest.raises(NotImplementedError):  # no CPU kernel, no fallback
        D.act_rule(torch.zeros((1, 1, 89)), 1, 1, 0, torch.zeros((1, 1), dtype=torch.int32), None)
    # the Meta kernel: shapes only, no launch
    obs = torch.zeros((2, 4, 89), device="meta")
    D.act_rule(obs, 2, 2, 1, torch.zeros((2, 4), dtype=torch.int32, device="meta"),
               torch.zeros((2, 4, 4), dtype=torch.int32, device="meta"))


# ---------------------------------------------------------------- configuration
def test_check_behavior():
    from dmdqn_amd.agent import BEHAVIORS, AgentConfig, check_behavior
    assert BEHAVIORS == ("longest_queue", "max_pressure")
    assert check_behavior(None, 0, 0.1) == (None, 0, 0.1)
    assert check_behavior("max_pressure", 12, 0) == ("max_pressure", 12, 0.0)
    assert check_behavior("longest_queue", np.int64(3), 1) == ("longest_queue", 3, 1.0)
    for bad in (("fifo", 0, 0.1), ("", 0, 0.1), (1, 0, 0.1), ("max_pressure", -1, 0.1),
                ("max_pressure", 1.5, 0.1), ("max_pressure", True, 0.1),
                ("max_pressure", 0, -0.01), ("max_pressure", 0, 1.01),
                ("max_pressure", 0, float("nan")), ("max_pressure", 0, "x"),
                ("max_pressure", 0, None)):
        with pytest.raises(ValueError, match="behavior"):
            check_behavior(*bad)
    cfg = AgentConfig()
    assert (cfg.behavior, cfg.behavior_steps, cfg.behavior_eps) == (None, 0, 0.1)
    cfg = AgentConfig.from_dict({"behavior": "max_pressure", "behavior_steps": 2000,
                                 "behavior_eps": 0.2})
    assert (cfg.behavior, cfg.behavior_steps, cfg.behavior_eps) == ("max_pressure", 2000, 0.2)


def test_trainer_and_agent_refuse_before_device_work():
    """A bad behaviour config and a schedule that does not run it raise
    ValueError where nothing has touched a device yet (there is none here)."""
    from dmdqn_amd.agent import AgentConfig, BatchedDQN
    from dmdqn_amd.env import EnvConfig
    from dmdqn_amd.trainer import Trainer
    env = EnvConfig(rows=2, cols=2, num_envs=2)
    for kw in ({"behavior": "fifo"}, {"behavior": "max_pressure", "behavior_eps": 2.0},
               {"behavior": "max_pressure", "behavior_steps": -5},
               {"behavior_steps": -1}, {"behavior_eps": -0.5}):
        with pytest.raises(ValueError, match="behavior"):
            Trainer(env, AgentConfig(precision="fp16", **kw), device="cuda")
        with pytest.raises(ValueError, match="behavior"):
            BatchedDQN(2, 4, AgentConfig(precision="fp16", **kw), device="cuda")
    for overlap in ("sample", "learn", "full", True):
        with pytest.raises(ValueError, match='behavior runs under overlap "none" or "env"'):
            Trainer(env, AgentConfig(precision="fp16", behavior="max_pressure"), device="cuda",
                    overlap=overlap)


def test_checkpoint_fixes_the_behavior_keys():
    from dmdqn_amd import checkpoint as CK
    for k in ("behavior", "behavior_steps", "behavior_eps"):
        assert k in CK._AGENT_FIXED and k in CK._DEFAULTS
    old = {"precision": "fp16"}  # a checkpoint from before the keys existed
    CK._check_cfg(old, {"behavior": None, "behavior_steps": 0, "behavior_eps": 0.1},
                  ["behavior", "behavior_steps", "behavior_eps"], "agent_cfg")
    with pytest.raises(ValueError, match="agent_cfg.behavior"):
        CK._check_cfg(old, {"behavior": "max_pressure"}, ["behavior"], "agent_cfg")


def test_eval_modes_and_cli():
    import sys
    from dmdqn_amd import evaluate as EV
    assert set(EV.MODES) == {"dqn", "random", "fixed", "program", "longest_queue", "max_pressure"}
    sys.path.insert(0, os.path.join(ROOT, "src"))
    from scripts.test import parse_eval_args
    a = parse_eval_args(["--modes", "random", "fixed", "program", "longest_queue", "max_pressure"])
    assert a.modes == ["random", "fixed", "program", "longest_queue", "max_pressure"]
    with pytest.raises(SystemExit):
        parse_eval_args(["--modes", "fifo"])
