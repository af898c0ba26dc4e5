"""No GPU: the paired learn's entry point (dmdqn_learn_pair) as far as the host
goes -- it is exported, bound and refuses bad pairs before any launch -- and
the library digest, which now covers every compile flag: a build with
DMDQN_EXTRA_FLAGS switches (an A/B library) is not accepted as the product
library."""
import ctypes

import pytest

from dmdqn_amd import build


@pytest.fixture(scope="module")
def lib():
    build.build(verbose=False)
    from dmdqn_amd import _lib, agent  # noqa: F401  (agent registers the learn signatures)
    return _lib.load()


def _block(**kw):
    """A dmdqn_learn_args that passes dmdqn_learn's own checks: the pointers are
    dummies, never dereferenced (every case below is refused on the host)."""
    from dmdqn_amd.agent import CLearn, n_params
    a = CLearn()
    a.NA, a.cap, a.start, a.batch, a.hidden, a.precision, a.P = 3, 162, 5, 128, 128, 1, n_params(128)
    for k, f in enumerate(("ring_s", "ring_n", "ring_a", "ring_d", "ring_r", "idx", "params",
                           "adam_m", "adam_v", "target", "target_h", "loss")):
        setattr(a, f, 4096 * (k + 1))
    a.alpha, a.c1, a.c2, a.eps, a.gamma = 1e-3, 0.1, 0.001, 1e-7, 0.99
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _rc(lib, a0, a1, hp0=None, hp1=None):
    rc = lib.dmdqn_learn_pair(ctypes.byref(a0), ctypes.byref(a1), hp0, hp1, None)
    return rc, lib.dmdqn_last_error().decode()


def test_entry_point_is_exported_and_bound(lib):
    from dmdqn_amd import _lib, ops
    assert hasattr(lib, "dmdqn_learn_pair")
    assert "dmdqn_learn_pair" in _lib.SIGNATURES
    assert ops.ENTRY_POINTS["dmdqn_learn_pair"] == "learn_pair"
    sch = ops.load().learn_pair.default._schema
    names = [a.name for a in sch.arguments]
    for n in ("idx0", "idx1", "loss0", "loss1", "start0", "start1", "adam0", "adam1", "factors0",
              "factors1", "qstats0", "qstats1", "rn_out0", "rn_out1"):
        assert n in names, n


@pytest.mark.parametrize("change,match", [
    (dict(sync_target=1), "sync_target"),
    (dict(row_format=1, xs=64, xn=128), "int8 replay rows"),
    (dict(params=12345 * 16), "share"),
    (dict(adam_v=12345 * 16), "share"),
    (dict(ring_n=12345 * 16), "share"),
    (dict(cap=163), "share"),
    (dict(NA=4), "share"),
    (dict(tau=0.5, one_minus_tau=0.5), "soft target update"),
    (dict(qstats=64), "qstats"),
    (dict(stamps=64), "stamps"),
    (dict(precision=2), "precision"),
    (dict(batch=64), "batch"),
    (dict(tau=2.0), "tau"),
])
def test_bad_pairs_are_refused_on_the_host(lib, change, match):
    """Each way round: the fault may sit in either learn."""
    for first in (False, True):
        a0, a1 = _block(), _block(loss=4096 * 40)
        for k, v in change.items():
            setattr(a0 if first else a1, k, v)
        rc, msg = _rc(lib, a0, a1)
        assert rc == -1 and "dmdqn_learn" in msg and match in msg, (first, rc, msg)


def test_pair_needs_16_bit_nets_with_a_shadow(lib):
    from dmdqn_amd.agent import n_params
    rc, msg = _rc(lib, _block(precision=0), _block(precision=0))
    assert rc == -1 and "16-bit" in msg, msg
    rc, msg = _rc(lib, _block(hidden=64, P=n_params(64)), _block(hidden=64, P=n_params(64)))
    assert rc == -1 and "hidden" in msg, msg
    rc, msg = _rc(lib, _block(target_h=None), _block(target_h=None))
    assert rc == -1 and "target_h" in msg, msg
    rc = lib.dmdqn_learn_pair(ctypes.byref(_block()), None, None, None, None)
    assert rc == -1 and "null args" in lib.dmdqn_last_error().decode()


def test_pair_outputs_must_be_each_learns_own(lib):
    for kw in (dict(), dict(qstats=64), dict(rn_out=64), dict(qstats=64, rn_out=128)):
        # _block() gives both learns the same loss pointer; qstats / rn_out as given
        rc, msg = _rc(lib, _block(**kw), _block(**kw))
        assert rc == -1 and "each learn's own" in msg, (kw, msg)
    rc, msg = _rc(lib, _block(rn_out=64), _block(rn_out=64, loss=4096 * 40))
    assert rc == -1 and "each learn's own" in msg, msg


def test_pair_checks_its_hyperparameter_blocks(lib):
    from dmdqn_amd.agent import CHParams
    bad = CHParams(None, None, 64, None, 1.0, 1.0)  # tau without one_minus_tau
    for hp0, hp1 in ((ctypes.byref(bad), None), (None, ctypes.byref(bad))):
        rc, msg = _rc(lib, _block(), _block(), hp0, hp1)
        assert rc == -1 and "go together" in msg, msg
    soft = CHParams(None, None, 64, 128, 1.0, 1.0)  # per-agent tau: a soft learn
    rc, msg = _rc(lib, _block(), _block(), ctypes.byref(soft), None)
    assert rc == -1 and "soft target update" in msg, msg


# --------------------------------------------------------------- the digest
def test_digest_changes_with_extra_flags(monkeypatch):
    plain = build.tree_digest()
    monkeypatch.setattr(build, "EXTRA", ["-DDMDQN_EXPERIMENT=1"])
    exp = build.tree_digest()
    assert exp != plain
    monkeypatch.setattr(build, "EXTRA", ["-DDMDQN_EXPERIMENT=0"])
    assert build.tree_digest() not in (plain, exp)
    monkeypatch.setattr(build, "EXTRA", [])
    assert build.tree_digest() == plain


def test_digest_changes_with_per_file_and_variant_flags(monkeypatch):
    plain = build.tree_digest()
    assert build.tree_digest(variant="debug") != plain
    assert build.tree_digest(variant="exp") == plain  # no flags of its own
    monkeypatch.setitem(build.PER_FILE, "learn_f16.hip", ["-ffp-contract=off"])
    assert build.tree_digest() != plain
    monkeypatch.undo()
    monkeypatch.setattr(build, "DEFAULT_FP", ["-ffp-contract=fast"])
    assert build.tree_digest() != plain


def test_product_library_refused_under_other_flags(lib, monkeypatch):
    """The library built without switches does not load as the library of a
    process whose build flags carry one (and the reverse: an A/B build made
    with DMDQN_EXTRA_FLAGS embeds another digest than the plain tree's)."""
    from dmdqn_amd import _lib
    plain = ctypes.CDLL(_lib.LIB_PATH)
    assert _lib.verify_digest(plain, "libdmdqn_hip.so") == build.tree_digest()
    monkeypatch.delenv("DMDQN_ALLOW_FOREIGN_LIB", raising=False)
    monkeypatch.setattr(build, "EXTRA", ["-DDMDQN_EXPERIMENT=1"])
    with pytest.raises(_lib.DmdqnError, match="stale"):
        _lib.verify_digest(plain, "libdmdqn_hip.so")


def test_paired_learn_sources_are_built_and_digested():
    import os
    names = {os.path.basename(p) for p in build.tree_files()}
    for f in ("learn_h16_body.hpp", "learn_f16_x2.hip", "learn_bf16_x2.hip"):
        assert f in names and f in build.KERNEL_SOURCES["learn"], f
    for f in ("learn_f16_x2.hip", "learn_bf16_x2.hip"):
        # the arithmetic flags of the single learn's files
        assert [x for x in build.PER_FILE[f] if x.startswith("-ffp")] == build.PER_FILE[
            f.replace("_x2", "")]


# ------------------------------------------------ marks and buffer rotation
def _model(spare, calls, rng, p_flush, p_stats, sync_every, mark_every=False):
    """The paired "env" schedule's calls as the trainer issues them
    (trainer._step_env_beside_learn), with its own decision functions
    (trainer.pair_action, trainer.pair_mark_due) and a clock of main-stream
    events in place of the GPU: learns launch, marks are recorded, and the side
    stream's work of call k (the store into the slot the learns of calls up to
    k - 1 - spare read; the draws into the index buffer of call k - OUT_BUFS)
    starts behind the mark it waits for.  Returns (marks, pairs, singles)."""
    from dmdqn_amd.trainer import pair_action, pair_mark_due
    OUT = spare + 2                      # BatchedDQN.OUT_BUFS
    clock = [0]
    launched = {}                        # call -> clock of the launch that holds its learn
    marks = []                           # (call, clock)
    last_mark, held, pending = -1, -2, None
    pairs = singles = 0

    def tick():
        clock[0] += 1
        return clock[0]

    def mark(j):
        # a mark of call j stands behind the launch that holds learn j
        assert all(c in launched for c in range(j + 1)), (j, sorted(launched)[-3:])
        marks.append((j, tick()))

    for k in range(calls):
        if held == k - 1 and pending is None and pair_mark_due(k - 1, last_mark, spare, mark_every):
            mark(k - 1)
            last_mark = k - 1
        usable = [m for m in marks if m[0] <= k - 2]
        if k - 1 - spare >= 0:
            assert usable and usable[-1][0] >= k - 1 - spare, f"no mark covers call {k - 1 - spare}"
        if usable:
            j, t = usable[-1]
            # the store of call k: every learn whose window holds its slot is done
            assert all(launched[c] < t for c in range(0, k - spare)), (k, j)
            # the draws of call k reuse the index buffer of call k - OUT: the
            # launch that read it (alone or as a pair) is behind the mark
            if k - OUT >= 0:
                assert launched[k - OUT] < t, (k, j)
        else:
            assert k - OUT < 0 and k - 1 - spare < 0
        n = k + 1                        # every call learns: learn n of this call
        sync, next_sync = n % sync_every == 0, (n + 1) % sync_every == 0
        plain = not (rng.random() < p_stats or sync)
        had, pending = pending, None
        what = pair_action(had is not None, plain, next_sync)
        if what == "pair":
            launched[had] = launched[k] = tick()
            pairs += 1
        elif what == "both":
            launched[had] = tick()
            launched[k] = tick()
            singles += 2
        elif what == "hold":
            pending, held = k, k
        else:
            launched[k] = tick()
            singles += 1
        if pending is None and pair_mark_due(k, last_mark, spare, mark_every):
            mark(k)
            last_mark = k
        if pending is not None and rng.random() < p_flush:  # last_loss, synchronize, ...
            launched[pending] = tick()
            singles += 1
            pending = None
    return marks, pairs, singles


@pytest.mark.parametrize("spare", list(range(2, 33)))
def test_marks_and_buffers_with_held_back_learns(spare):
    import random
    for seed, (p_flush, p_stats, sync_every) in enumerate([
            (0.0, 0.0, 10 ** 9), (0.0, 0.0, 7), (1.0, 0.0, 7), (0.3, 0.2, 7), (0.5, 0.0, 2),
            (0.1, 0.5, 3), (0.0, 1.0, 500), (0.9, 0.1, 500)]):
        calls = 40 * spare + 50
        marks, pairs, singles = _model(spare, calls, random.Random(seed), p_flush, p_stats,
                                       sync_every)
        assert 2 * pairs + singles in (calls, calls - 1)  # (the last learn may be held back)
        gaps = [b[0] - a[0] for a, b in zip(marks, marks[1:])]
        assert marks[0][0] <= spare - 1 and max(gaps) <= spare, (spare, max(gaps))
        if p_flush == p_stats == 0.0 and sync_every > calls:
            assert pairs == calls // 2 and singles == 0
            # no more marks than the unpaired schedule's one per `spare` calls needs
            assert len(marks) <= calls // (spare - 1) + 1
    marks, _, _ = _model(spare, 100, random.Random(9), 0.2, 0.1, 7, mark_every=True)
    assert len(marks) >= 50


def test_pair_action_table():
    from dmdqn_amd.trainer import pair_action
    assert pair_action(True, True, False) == pair_action(True, True, True) == "pair"
    assert pair_action(True, False, False) == pair_action(True, False, True) == "both"
    assert pair_action(False, True, False) == "hold"
    assert pair_action(False, True, True) == pair_action(False, False, False) == "single"


# ------------------------------------------------ the paired kernels' resources
def test_paired_kernels_keep_two_workgroups_per_cu(lib, tmp_path):
    """The paired learn's register, LDS and scratch figures depend on how the
    compiler treats its two rounds (learn_h16.hpp, at the kernel: the second
    entry, -disable-machine-licm).  From the built library's kernel metadata
    (what tools/kernel_resources.py prints; no code is read): every
    k_learn_*_x2 stays within two workgroups of 512 per CU -- <= 128 VGPRs, no
    AGPRs, <= 80 KB LDS -- and within the single kernel's scratch plus the one
    measured exception (soft update with per-agent hyperparameters, f16: 64 B
    against 44).  The lane-address spills this guards against were
    120-600 B."""
    import re
    import subprocess
    from dmdqn_amd import _lib
    from test_isa_cpu import LLVM, _code_objects
    keys = {".vgpr_count": "vgpr", ".agpr_count": "agpr", ".group_segment_fixed_size": "lds",
            ".private_segment_fixed_size": "scratch", ".max_flat_workgroup_size": "wg"}
    found = {}
    for co in _code_objects(_lib.LIB_PATH, tmp_path):
        notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", str(co)], check=True,
                               capture_output=True, text=True).stdout
        for block in notes.split("  - .agpr_count")[1:]:
            block = "  - .agpr_count" + block
            name = re.search(r"\.name:\s+(\S+)", block).group(1)
            if "_x2" in name and "k_learn_" in name:
                found[name] = {v: int(re.search(re.escape(k) + r":\s+(\d+)", block).group(1))
                               for k, v in keys.items()}
    # QSTATS x {TGT_NONE, TGT_SOFT} x HP, f16 and bf16
    assert len(found) == 16, sorted(found)
    for name, v in found.items():
        assert v["wg"] == 512 and v["vgpr"] <= 128 and v["agpr"] == 0, (name, v)
        assert v["lds"] <= 80 * 1024, (name, v)
        assert v["scratch"] <= 64, (name, v)
        if "Li0E" in name:  # TGT_NONE (the flagship's): the single kernel has 0
            assert v["scratch"] <= 8, (name, v)
