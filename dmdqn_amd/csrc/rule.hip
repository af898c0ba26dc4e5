// rule.hip -- rule-based controllers, longest-queue-first and max-pressure, as
// one action per agent from its observation (dmdqn_act_rule; include/dmdqn.h
// has the rule).  The output has dmdqn_act's `greedy` format, so a controller
// stands in for dmdqn_q_argmax without touching the act or env-step kernels.
//
// One 32-lane group (half a wave) per agent, 8 agents per 256-thread block.
// Lane j of a group loads features j, j + 32 and j + 64 of the agent's 89: three
// dword loads on consecutive addresses across the group (rows are 356 B, so only
// 4-byte aligned; one thread per strided row would touch a cache line per
// load).  Every score is sum_i coef[i][a] * int(obs[i]) * present(i): the
// coefficients are compile-time bit planes over the lanes (a shift and a mask
// of an immediate per lane, no table in memory), derived from sim.hpp's
// green_mask and movement.  The four sums cross the group by xor shuffles, so
// every lane ends with all four; lane 0 stores the action, lanes 0..3 a score
// each.  No LDS, no atomics; a tail group past E*A reads agent E*A - 1 again,
// stays in the shuffles and stores nothing.
// Built with the default -ffp-contract=off (no float arithmetic beyond the
// conversions to int32).
#include "sim.hpp"

namespace dmdqn {
namespace {

constexpr int RULE_NT = 256, RULE_G = 32, RULE_PER_BLOCK = RULE_NT / RULE_G;
constexpr int RULE_LOADS = 3;  // features j, j + 32, j + 64
static_assert(RULE_LOADS * RULE_G >= DMDQN_OBS_DIM, "the group covers the row");

// ---------------------------------------------------------------- the rule's geometry
// The primary movement of observed lane k: lanes 0 and 1 straight, lane 2 left.
constexpr int lane_move(int k) { return k < 2 ? MV_S : MV_L; }
// Whether lane k of approach d belongs to action a: its primary movement is
// green in phase 3a of the program.
constexpr bool in_group(int a, int d, int k) {
    return (green_mask(3 * a) >> (4 * d + lane_move(k))) & 1u;
}
// The groups partition the 12 lanes: every lane is in exactly one.
constexpr bool groups_partition() {
    for (int d = 0; d < 4; d++)
        for (int k = 0; k < 3; k++) {
            int n = 0;
            for (int a = 0; a < 4; a++) n += in_group(a, d, k) ? 1 : 0;
            if (n != 1) return false;
        }
    return true;
}
static_assert(groups_partition(), "the actions' lane groups partition the 12 observed lanes");
static_assert(in_group(0, DIR_N, 0) && in_group(0, DIR_S, 1) && in_group(1, DIR_N, 2) &&
                  in_group(2, DIR_E, 0) && in_group(2, DIR_W, 1) && in_group(3, DIR_W, 2),
              "G0 = {n0,n1,s0,s1}, G1 = {n2,s2}, G2 = {e0,e1,w0,w1}, G3 = {e2,w2}");
// The out-direction of lane k of approach d: the o its primary movement takes
// from the heading opp(d).
constexpr int lane_out(int d, int k) {
    for (int o = 0; o < 4; o++)
        if (movement(opp(d), o) == lane_move(k)) return o;
    return -1;
}
static_assert(lane_out(DIR_N, 0) == DIR_S && lane_out(DIR_S, 1) == DIR_N &&
                  lane_out(DIR_E, 0) == DIR_W && lane_out(DIR_W, 0) == DIR_E,
              "straight: n -> s, s -> n, e -> w, w -> e");
static_assert(lane_out(DIR_N, 2) == DIR_E && lane_out(DIR_S, 2) == DIR_W &&
                  lane_out(DIR_E, 2) == DIR_S && lane_out(DIR_W, 2) == DIR_N,
              "left: n -> e, s -> w, e -> s, w -> n");

// Observation index i as (neighbour o, its approach d', lane k'), o = -1 for
// the agent's own 21 features.
constexpr int feat_nbr(int i) { return i < 21 ? -1 : (i - 21) / 17; }
constexpr int feat_local(int i) { return i < 21 ? i : (i - 21) % 17; }
// How many lanes of action a drain into neighbour o: D(o)'s weight in score[a].
constexpr int drains(int a, int o) {
    int n = 0;
    for (int d = 0; d < 4; d++)
        for (int k = 0; k < 3; k++) n += (in_group(a, d, k) && lane_out(d, k) == o) ? 1 : 0;
    return n;
}
// coef[i][a] of the max-pressure score without the own queues' factor 3:
// +1 for an own lane of Ga (the longest-queue coefficient), -drains(a, o) for a
// lane of neighbour o's approach opp(o), 0 elsewhere.
constexpr int own_coef(int i, int a) {
    return i < 12 && in_group(a, i / 3, i % 3) ? 1 : 0;
}
constexpr int down_coef(int i, int a) {
    const int o = feat_nbr(i), f = feat_local(i);
    return o >= 0 && f < 12 && f / 3 == opp(o) ? drains(a, o) : 0;
}
static_assert(down_coef(38, 0) == 2 && down_coef(38, 3) == 1 && down_coef(38, 1) == 0,
              "the south neighbour's approach from the north takes n0, n1 (action 0) and e2 (3)");

// Bit j: whether `pred` holds for feature j + 32 c -- one immediate per use.
template <typename F>
constexpr uint32_t lane_bits(int c, F pred) {
    uint32_t m = 0;
    for (int j = 0; j < RULE_G; j++) {
        const int i = j + RULE_G * c;
        if (i < DMDQN_OBS_DIM && pred(i)) m |= 1u << j;
    }
    return m;
}
template <int C, int A>
struct Planes {
    static constexpr uint32_t own = lane_bits(C, [](int i) { return own_coef(i, A) != 0; });
    static constexpr uint32_t d1 = lane_bits(C, [](int i) { return (down_coef(i, A) & 1) != 0; });
    static constexpr uint32_t d2 = lane_bits(C, [](int i) { return (down_coef(i, A) & 2) != 0; });
    static_assert(lane_bits(C, [](int i) { return down_coef(i, A) > 3; }) == 0, "two bit planes");
};
// The lanes whose feature j + 32 c lies in neighbour o's block (o = -1: the
// agent's own features).
template <int C, int O>
struct Block {
    static constexpr uint32_t in = lane_bits(C, [](int i) { return feat_nbr(i) == O; });
};

// feature c of lane j as the int32 the scores take: 0 when its neighbour is absent
template <int C>
__device__ __forceinline__ int masked(float v, int j, const bool (&pres)[4]) {
    const uint32_t keep = Block<C, -1>::in |
                          (pres[0] ? Block<C, 0>::in : 0u) | (pres[1] ? Block<C, 1>::in : 0u) |
                          (pres[2] ? Block<C, 2>::in : 0u) | (pres[3] ? Block<C, 3>::in : 0u);
    return ((keep >> j) & 1u) ? (int)v : 0;
}

// this lane's part of score[A] from feature c (value x)
template <int RULE, int C, int A>
__device__ __forceinline__ int part(int x, int j) {
    const int own = (int)((Planes<C, A>::own >> j) & 1u);
    if (RULE == DMDQN_RULE_LONGEST_QUEUE) return own * x;
    const int down = (int)((Planes<C, A>::d1 >> j) & 1u) + 2 * (int)((Planes<C, A>::d2 >> j) & 1u);
    return (3 * own - down) * x;
}

template <int RULE, int A>
__device__ __forceinline__ int group_sum(const int (&x)[RULE_LOADS], int j) {
    int s = part<RULE, 0, A>(x[0], j) + part<RULE, 1, A>(x[1], j) + part<RULE, 2, A>(x[2], j);
#pragma unroll
    for (int m = RULE_G / 2; m >= 1; m >>= 1) s += __shfl_xor(s, m, RULE_G);
    return s;
}

template <int RULE>
__global__ void __launch_bounds__(RULE_NT) k_act_rule(int NA, const float *__restrict__ obs,
                                                      int32_t *__restrict__ actions,
                                                      int32_t *__restrict__ score) {
    const int tid = threadIdx.x, j = tid & (RULE_G - 1);
    const int g = blockIdx.x * RULE_PER_BLOCK + (tid >> 5);
    const bool live = g < NA;  // uniform over the group
    const float *row = obs + (size_t)(live ? g : NA - 1) * DMDQN_OBS_DIM;
    float v[RULE_LOADS];
#pragma unroll
    for (int c = 0; c < RULE_LOADS; c++) {
        const int i = j + RULE_G * c;
        v[c] = i < DMDQN_OBS_DIM ? row[i] : 0.0f;
    }
    // the four neighbour flags sit in lanes 17..20 of the first load
    bool pres[4];
#pragma unroll
    for (int o = 0; o < 4; o++) pres[o] = __shfl(v[0], 17 + o, RULE_G) == 1.0f;
    const int x[RULE_LOADS] = {masked<0>(v[0], j, pres), masked<1>(v[1], j, pres),
                               masked<2>(v[2], j, pres)};
    const int s0 = group_sum<RULE, 0>(x, j), s1 = group_sum<RULE, 1>(x, j),
              s2 = group_sum<RULE, 2>(x, j), s3 = group_sum<RULE, 3>(x, j);
    if (!live) return;
    // the first maximum, the lowest index on ties (learn_rules.hpp first_max4)
    int best = 0, bs = s0;
    if (s1 > bs) { best = 1; bs = s1; }
    if (s2 > bs) { best = 2; bs = s2; }
    if (s3 > bs) { best = 3; }
    if (j == 0) actions[g] = best;
    if (score && j < 4) score[(size_t)g * 4 + j] = j == 0 ? s0 : j == 1 ? s1 : j == 2 ? s2 : s3;
}

}  // namespace
}  // namespace dmdqn

using namespace dmdqn;

extern "C" int dmdqn_act_rule(int R, int C, int E, int rule, const float *obs, int32_t *actions,
                              int32_t *score, void *stream) {
    const char *who = "dmdqn_act_rule";
    DMDQN_REQUIRE(R >= 1 && C >= 1 && E >= 1, "%s: grid %dx%d / E=%d must be >= 1", who, R, C, E);
    DMDQN_REQUIRE((long long)R * C * E <= INT32_MAX, "%s: E*R*C = %lld beyond int32", who,
                  (long long)R * C * E);
    DMDQN_REQUIRE(rule == DMDQN_RULE_LONGEST_QUEUE || rule == DMDQN_RULE_MAX_PRESSURE,
                  "%s: unknown rule %d (0 longest queue, 1 max pressure)", who, rule);
    DMDQN_REQUIRE(obs && actions, "%s: null obs or actions", who);
    const int NA = R * C * E;
    const dim3 grid((NA + RULE_PER_BLOCK - 1) / RULE_PER_BLOCK), block(RULE_NT);
    if (rule == DMDQN_RULE_LONGEST_QUEUE)
        hipLaunchKernelGGL(k_act_rule<DMDQN_RULE_LONGEST_QUEUE>, grid, block, 0, as_stream(stream),
                           NA, obs, actions, score);
    else
        hipLaunchKernelGGL(k_act_rule<DMDQN_RULE_MAX_PRESSURE>, grid, block, 0, as_stream(stream),
                           NA, obs, actions, score);
    DMDQN_LAUNCH_CHECK("k_act_rule");
    return DMDQN_OK;
}
