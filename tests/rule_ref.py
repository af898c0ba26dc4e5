"""numpy restatement of the rule-based controllers (include/dmdqn.h,
dmdqn_act_rule), with the lane groups and out-directions written out as
literal tables -- independent of the kernel's compile-time derivation from
green_mask -- plus a movement-level brute force from the phase masks, the
fixture the GPU tests share and the known answers of the header."""
import numpy as np

OBS_DIM = 89
LONGEST_QUEUE, MAX_PRESSURE = 0, 1
RULE_NAMES = {"longest_queue": LONGEST_QUEUE, "max_pressure": MAX_PRESSURE}

# approaches d = 0 n, 1 s, 2 e, 3 w; lane (d, k) is obs[3 d + k]
N, S, E_, W = 0, 1, 2, 3
GROUPS = (
    ((N, 0), (N, 1), (S, 0), (S, 1)),   # action 0
    ((N, 2), (S, 2)),                   # action 1
    ((E_, 0), (E_, 1), (W, 0), (W, 1)),  # action 2
    ((E_, 2), (W, 2)),                  # action 3
)
# out-direction of a lane's primary movement: straight (lanes 0, 1), left (lane 2)
OUT_STRAIGHT = {N: 1, S: 0, E_: 3, W: 2}
OUT_LEFT = {N: 2, S: 3, E_: 1, W: 0}


def lane_out(d, k):
    return OUT_STRAIGHT[d] if k < 2 else OUT_LEFT[d]


def as_int(obs):
    """obs [..., 89] float -> int64 (the kernel converts once, to int32; the
    sums below stay far inside both)."""
    o = np.asarray(obs)
    assert o.shape[-1] == OBS_DIM
    return o.astype(np.int64)


def downstream(v):
    """D(o) [..., 4]: the 3 lanes of neighbour o's approach o ^ 1, 0 without it."""
    D = np.zeros(v.shape[:-1] + (4,), dtype=np.int64)
    for o in range(4):
        base = 21 + 17 * o + 3 * (o ^ 1)
        D[..., o] = np.where(v[..., 17 + o] == 1, v[..., base:base + 3].sum(-1), 0)
    return D


def scores(obs, rule):
    """int64 [..., 4]."""
    rule = RULE_NAMES.get(rule, rule)
    v = as_int(obs)
    D = downstream(v)
    out = np.zeros(v.shape[:-1] + (4,), dtype=np.int64)
    for a, lanes in enumerate(GROUPS):
        for d, k in lanes:
            q = v[..., 3 * d + k]
            out[..., a] += q if rule == LONGEST_QUEUE else 3 * q - D[..., lane_out(d, k)]
    return out


def first_max(sc):
    """The first maximum along the last axis (np.argmax's tie rule)."""
    return np.argmax(sc, axis=-1).astype(np.int32)


def act_rule(obs, rule):
    """(actions int32 [...], scores int32 [..., 4])."""
    sc = scores(obs, rule)
    return first_max(sc), sc.astype(np.int32)


# ---------------------------------------------------------------- brute force
# the phase masks of actions 0..3 (phases 0, 3, 6, 9): bit 4 d + m, m = 0 right,
# 1 straight, 2 left, 3 U-turn (include/dmdqn.h; csrc/sim.hpp green_mask)
PHASE_MASKS = (0x11BB, 0x11DD, 0xBB11, 0xDD11)
MV_R, MV_S, MV_L, MV_U = 0, 1, 2, 3


def right_of(h):  # n->e, s->w, e->s, w->n
    return {N: E_, S: W, E_: S, W: N}[h]


def movement(h, o):
    """csrc/sim.hpp movement(): heading h leaves through out-direction o."""
    if o == h:
        return MV_S
    if o == (h ^ 1):
        return MV_U
    if o == right_of(h):
        return MV_R
    return MV_L


def brute_scores(row, rule):
    """One observation row, movement by movement: every (approach, lane) with
    its primary movement (lanes 0, 1 straight; lane 2 left) is looked up in
    each action's phase mask, and its out-direction is searched with
    movement()."""
    v = [int(x) for x in np.asarray(row)]
    out = [0, 0, 0, 0]
    for a, mask in enumerate(PHASE_MASKS):
        for d in range(4):
            for k in range(3):
                m = MV_S if k < 2 else MV_L
                if not (mask >> (4 * d + m)) & 1:
                    continue
                q = v[3 * d + k]
                if rule == LONGEST_QUEUE:
                    out[a] += q
                    continue
                (o,) = [o for o in range(4) if movement(d ^ 1, o) == m]
                D = 0
                if v[17 + o] == 1:
                    D = sum(v[21 + 17 * o + 3 * (o ^ 1) + kk] for kk in range(3))
                out[a] += 3 * q - D
    return out


# ---------------------------------------------------------------- observations
def neighbor(R, C, a, d):
    r, c = divmod(a, C)
    if d == N:
        return a - C if r > 0 else -1
    if d == S:
        return a + C if r < R - 1 else -1
    if d == E_:
        return a + 1 if c < C - 1 else -1
    return a - 1 if c > 0 else -1


def random_obs(rng, R, C, E, hi=24):
    """Observations as k_observe builds them from random halting counts in
    0..hi: own 12 counts, a zero phase block with time -1, the neighbour flags
    and the neighbours' 17-blocks, -1 padding for an absent neighbour."""
    A = R * C
    local = np.zeros((E, A, 17), dtype=np.float32)
    local[..., :12] = rng.integers(0, hi + 1, size=(E, A, 12))
    local[..., 16] = -1.0
    return obs_from_local(local, R, C)


def obs_from_local(local, R, C):
    E, A = local.shape[:2]
    obs = np.full((E, A, OBS_DIM), -1.0, dtype=np.float32)
    obs[..., :17] = local
    for a in range(A):
        for d in range(4):
            b = neighbor(R, C, a, d)
            obs[:, a, 17 + d] = 1.0 if b >= 0 else 0.0
            if b >= 0:
                obs[:, a, 21 + 17 * d:38 + 17 * d] = local[:, b]
    return obs


# ---------------------------------------------------------------- the shared fixture
FIXTURE_SEED = 4
FIXTURE_GRIDS = ((1, 1, 12), (1, 2, 12), (1, 3, 8), (3, 3, 8))  # (R, C, E)


def fixture_parts(seed=FIXTURE_SEED):
    """[(R, C, obs [E, A, 89])]: sparse random counts (many zeros, so exact
    ties happen) on grids whose agents have 0, 1, 2, 3 and 4 neighbours."""
    rng = np.random.default_rng(seed)
    parts = []
    for R, C, E in FIXTURE_GRIDS:
        A = R * C
        local = np.zeros((E, A, 17), dtype=np.float32)
        cnt = rng.integers(0, 7, size=(E, A, 12)) * (rng.random((E, A, 12)) < 0.45)
        local[..., :12] = cnt
        local[..., 16] = -1.0
        parts.append((R, C, obs_from_local(local, R, C)))
    return parts


def check_fixture(parts):
    """Raise unless the reference alone meets the coverage the GPU test relies
    on, for both rules."""
    rows = np.concatenate([o.reshape(-1, OBS_DIM) for _, _, o in parts])
    nn = (rows[:, 17:21] == 1).sum(1)
    for n in (0, 2, 3, 4):
        if (nn == n).sum() < 8:
            raise ValueError(f"fixture: fewer than 8 agents with {n} neighbours")
    acts = {}
    for rule in (LONGEST_QUEUE, MAX_PRESSURE):
        a, sc = act_rule(rows, rule)
        acts[rule] = a
        for k in range(4):
            if (a == k).sum() < 8:
                raise ValueError(f"fixture: rule {rule}: action {k} wins on fewer than 8 agents")
        top = sc.max(1, keepdims=True)
        tie = (sc == top).sum(1) >= 2
        if tie.sum() < 8:
            raise ValueError(f"fixture: rule {rule}: fewer than 8 exact ties")
        if not (a[tie] == np.argmax(sc[tie] == top[tie], axis=1)).all():
            raise ValueError("fixture: a tie not resolved to the lower index")
    if (acts[LONGEST_QUEUE] != acts[MAX_PRESSURE]).sum() < 8:
        raise ValueError("fixture: the rules disagree on fewer than 8 agents")
    D = downstream(as_int(rows))
    # an approach whose straight lanes and whose left lane both drain into a loaded edge
    straight_and_left = np.zeros(len(rows), dtype=bool)
    for d in range(4):
        straight_and_left |= (D[:, lane_out(d, 0)] > 0) & (D[:, lane_out(d, 2)] > 0)
    if not straight_and_left.any():
        raise ValueError("fixture: no agent with both a straight and a left downstream block")
    return parts


# ---------------------------------------------------------------- known answers
def known_rows():
    """[(row [89], rule, scores, action)] -- the literals of include/dmdqn.h."""
    zero = np.zeros(OBS_DIM, dtype=np.float32)
    n2 = zero.copy()
    n2[2] = 5
    full = zero.copy()
    full[0], full[6], full[18] = 4, 3, 1
    full[38:41] = 5
    return [
        (zero, LONGEST_QUEUE, [0, 0, 0, 0], 0), (zero, MAX_PRESSURE, [0, 0, 0, 0], 0),
        (n2, LONGEST_QUEUE, [0, 5, 0, 0], 1), (n2, MAX_PRESSURE, [0, 15, 0, 0], 1),
        (full, LONGEST_QUEUE, [4, 0, 3, 0], 0), (full, MAX_PRESSURE, [-18, 0, 9, -15], 2),
    ]
