// pbt.hip -- population-based training across the env replicas
// (dmdqn_pbt_score / dmdqn_pbt_select / dmdqn_pbt_exchange, include/dmdqn.h).
//
// Not in the reference (one config per run, train.py:110-121): the E replicas
// of a run are a population.  Every step adds each replica's reward to its
// fitness; every `interval` steps the worst n replicas take over the nets and
// Adam slots of the best n (exploit) and the host perturbs their per-agent
// hyperparameters (explore).  None of it is on the step's hot path:
//   score     one thread per replica, A f64 adds in junction order;
//   select    ranks by counting (E^2 compares over an L2-resident vector, E <=
//             65,536), then each loser looks its winner up -- two launches, so
//             the ranks are complete before they are read;
//   exchange  an in-place row copy: PBT_SPLIT workgroups per destination agent,
//             16-B loads and stores only, eight loads issued before the first
//             store, no LDS and no staging buffer.  The caller guarantees that
//             every source is a fixed point of src, so a source row is never a
//             destination and the copy is free of races.
#include <math.h>

#include "common.hpp"

namespace {

typedef float f4 __attribute__((ext_vector_type(4)));
constexpr int PBT_THREADS = 256;
constexpr int PBT_SPLIT = 4;  // workgroups per destination agent
constexpr int PBT_E_MAX = 65536;

__global__ __launch_bounds__(PBT_THREADS) void k_pbt_score(const double *__restrict__ reward,
                                                           int E, int A,
                                                           double *__restrict__ fitness) {
    const int e = blockIdx.x * PBT_THREADS + threadIdx.x;
    if (e >= E) return;
    const double *r = reward + (size_t)e * A;
    double t = r[0];
    for (int j = 1; j < A; j++) t = t + r[j];
    fitness[e] = fitness[e] + t;
}

__device__ __forceinline__ double pbt_key(double f) {
    return f != f ? -INFINITY : f;  // NaN ranks with -inf
}

// rank[e] = #{x : f'[x] > f'[e]} + #{x < e : f'[x] == f'[e]}
__global__ __launch_bounds__(PBT_THREADS) void k_pbt_rank(const double *__restrict__ fitness,
                                                          int E, int32_t *__restrict__ rank) {
    const int e = blockIdx.x * PBT_THREADS + threadIdx.x;
    if (e >= E) return;
    const double fe = pbt_key(fitness[e]);
    int r = 0;
    for (int x = 0; x < E; x++) {
        const double fx = pbt_key(fitness[x]);
        r += (fx > fe) || (fx == fe && x < e);
    }
    rank[e] = r;
}

// src[e] = e for the E - n best; a loser of rank r copies the replica of rank
// E - 1 - r (the ranks are a permutation: exactly one x matches)
__global__ __launch_bounds__(PBT_THREADS) void k_pbt_src(const int32_t *__restrict__ rank, int E,
                                                         int n, int32_t *__restrict__ src) {
    const int e = blockIdx.x * PBT_THREADS + threadIdx.x;
    if (e >= E) return;
    const int r = rank[e];
    int s = e;
    if (r >= E - n) {
        const int want = E - 1 - r;
        for (int x = 0; x < E; x++)
            if (rank[x] == want) s = x;
    }
    src[e] = s;
}

// One slice of one destination agent's rows.  blockIdx.x = agent * PBT_SPLIT +
// part; the PBT_SPLIT workgroups of an agent stride over its vectors together.
// (No __restrict__: source and destination rows live in the same arrays.)
__global__ __launch_bounds__(PBT_THREADS) void k_pbt_exchange(const int32_t *src, int E, int A,
                                                              int nv, int nvh, f4 *params,
                                                              f4 *target, f4 *adam_m, f4 *adam_v,
                                                              f4 *target_h) {
    const int agent = blockIdx.x / PBT_SPLIT, part = blockIdx.x % PBT_SPLIT;
    const int e = agent / A, j = agent - e * A;
    const int s = src[e];
    // uniform over the workgroup: a replica that keeps its nets (and an index
    // outside the population, which the host refuses where it can see it)
    if (s == e || s < 0 || s >= E) return;
    constexpr int NT = PBT_SPLIT * PBT_THREADS;
    const int t = part * PBT_THREADS + threadIdx.x;
    const size_t from = ((size_t)s * A + j) * nv, to = (size_t)agent * nv;
    f4 *const rows[4] = {params, target, adam_m, adam_v};
    int i = t;
    for (; i + NT < nv; i += 2 * NT) {
        f4 x[4][2];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            x[k][0] = rows[k][from + i];
            x[k][1] = rows[k][from + i + NT];
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
            rows[k][to + i] = x[k][0];
            rows[k][to + i + NT] = x[k][1];
        }
    }
    if (i < nv) {
        f4 x[4];
#pragma unroll
        for (int k = 0; k < 4; k++) x[k] = rows[k][from + i];
#pragma unroll
        for (int k = 0; k < 4; k++) rows[k][to + i] = x[k];
    }
    if (target_h == nullptr) return;
    const size_t fromh = ((size_t)s * A + j) * nvh, toh = (size_t)agent * nvh;
    for (i = t; i < nvh; i += 4 * NT) {
        f4 x[4];
#pragma unroll
        for (int u = 0; u < 4; u++)
            if (i + u * NT < nvh) x[u] = target_h[fromh + i + u * NT];
#pragma unroll
        for (int u = 0; u < 4; u++)
            if (i + u * NT < nvh) target_h[toh + i + u * NT] = x[u];
    }
}

}  // namespace

extern "C" int dmdqn_pbt_score(const double *reward, int E, int A, double *fitness, void *stream) {
    DMDQN_REQUIRE(reward && fitness, "dmdqn_pbt_score: null reward or fitness");
    DMDQN_REQUIRE(E >= 1 && A >= 1 && (long long)E * A <= INT32_MAX,
                  "dmdqn_pbt_score: E = %d, A = %d (both >= 1, E * A < 2^31)", E, A);
    hipLaunchKernelGGL(k_pbt_score, dim3((E + PBT_THREADS - 1) / PBT_THREADS), dim3(PBT_THREADS),
                       0, dmdqn::as_stream(stream), reward, E, A, fitness);
    DMDQN_LAUNCH_CHECK("k_pbt_score");
    return DMDQN_OK;
}

extern "C" int dmdqn_pbt_select(const double *fitness, int E, int n, int32_t *rank, int32_t *src,
                                void *stream) {
    DMDQN_REQUIRE(fitness && rank && src, "dmdqn_pbt_select: null fitness, rank or src");
    DMDQN_REQUIRE(E >= 2 && E <= PBT_E_MAX, "dmdqn_pbt_select: E = %d (2 .. %d)", E, PBT_E_MAX);
    DMDQN_REQUIRE(n >= 1 && n <= E / 2,
                  "dmdqn_pbt_select: n = %d (1 .. E / 2 = %d: winners and losers are disjoint)", n,
                  E / 2);
    const dim3 grid((E + PBT_THREADS - 1) / PBT_THREADS), block(PBT_THREADS);
    hipStream_t s = dmdqn::as_stream(stream);
    hipLaunchKernelGGL(k_pbt_rank, grid, block, 0, s, fitness, E, rank);
    DMDQN_LAUNCH_CHECK("k_pbt_rank");
    hipLaunchKernelGGL(k_pbt_src, grid, block, 0, s, (const int32_t *)rank, E, n, src);
    DMDQN_LAUNCH_CHECK("k_pbt_src");
    return DMDQN_OK;
}

extern "C" int dmdqn_pbt_exchange(const int32_t *src, int E, int A, int P, int Ph, float *params,
                                  float *target, float *adam_m, float *adam_v, uint16_t *target_h,
                                  void *stream) {
    DMDQN_REQUIRE(src && params && target && adam_m && adam_v,
                  "dmdqn_pbt_exchange: null src, params, target, adam_m or adam_v");
    DMDQN_REQUIRE(E >= 1 && A >= 1 && (long long)E * A * PBT_SPLIT <= INT32_MAX,
                  "dmdqn_pbt_exchange: E = %d, A = %d (both >= 1, E * A * %d < 2^31)", E, A,
                  PBT_SPLIT);
    DMDQN_REQUIRE(P >= 4 && P % 4 == 0, "dmdqn_pbt_exchange: P = %d (a positive multiple of 4)", P);
    DMDQN_REQUIRE(!target_h || (Ph >= P && Ph % 8 == 0),
                  "dmdqn_pbt_exchange: Ph = %d (a multiple of 8, >= P = %d)", Ph, P);
    DMDQN_REQUIRE((((uintptr_t)params | (uintptr_t)target | (uintptr_t)adam_m | (uintptr_t)adam_v |
                    (uintptr_t)target_h) % 16) == 0,
                  "dmdqn_pbt_exchange: 16-B alignment of the row arrays");
    hipLaunchKernelGGL(k_pbt_exchange, dim3((unsigned)E * A * PBT_SPLIT), dim3(PBT_THREADS), 0,
                       dmdqn::as_stream(stream), src, E, A, P / 4, target_h ? Ph / 8 : 0,
                       reinterpret_cast<f4 *>(params), reinterpret_cast<f4 *>(target),
                       reinterpret_cast<f4 *>(adam_m), reinterpret_cast<f4 *>(adam_v),
                       reinterpret_cast<f4 *>(target_h));
    DMDQN_LAUNCH_CHECK("k_pbt_exchange");
    return DMDQN_OK;
}
