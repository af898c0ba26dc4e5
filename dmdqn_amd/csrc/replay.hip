// replay.hip -- replay ring store (ReplayBuffer.add, src/agents/dqn_agent.py:31-57).
//
// Layout (per agent slot, capacity cap, ring position = total_adds % cap):
//   ring_s, ring_n : int8  [NA][cap][128]  s and s' rows: features 0..88, zero
//                                          to byte 95; the s' row also holds a
//                                          (byte 96), done (97) and r (f64,
//                                          104..111) -- the learn kernels' copy
//   ring_a         : uint8 [NA][cap]
//   ring_r         : f64   [NA][cap]       Python-float reward, kept in f64 so
//                                          the batch z-score is numpy-exact
//   ring_d         : uint8 [NA][cap]
// Observations of this env are small integers (queue counts <= 23, one-hot,
// time spent, -1 padding), so int8 storage is exact; any value that is not an
// integer in [-128,127] sets *err = DMDQN_ERANGE instead of being rounded.
#include "common.hpp"

namespace dmdqn {

// One thread per (agent, 4-byte group): 32 groups of 4 bytes per row.
__global__ void k_replay_store(int NA, int cap, int slot, const float *obs_s, const float *obs_n,
                               const int32_t *act, const double *rew, const uint8_t *done,
                               int8_t *ring_s, int8_t *ring_n, uint8_t *ring_a, double *ring_r,
                               uint8_t *ring_d, int32_t *err) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    constexpr int G = DMDQN_ROW_BYTES / 4;
    const int agent = t / G, grp = t - agent * G;
    if (agent >= NA) return;
    const size_t row = ((size_t)agent * cap + slot);
    uint32_t ws = 0, wn = 0;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const int i = grp * 4 + q;
        if (i < DMDQN_OBS_DIM) {
            ws |= (uint32_t)(uint8_t)to_i8(obs_s[(size_t)agent * DMDQN_OBS_DIM + i], err) << (8 * q);
            wn |= (uint32_t)(uint8_t)to_i8(obs_n[(size_t)agent * DMDQN_OBS_DIM + i], err) << (8 * q);
        }
    }
    if (4 * grp == DMDQN_ROW_A) {
        static_assert(DMDQN_ROW_D == DMDQN_ROW_A + 1, "a and done share a word");
        wn = (uint32_t)(uint8_t)act[agent] | (done[agent] ? 1u : 0u) << 8;
    } else if (4 * grp == DMDQN_ROW_R || 4 * grp == DMDQN_ROW_R + 4) {
        const unsigned long long rb = __double_as_longlong(rew[agent]);
        wn = (uint32_t)(4 * grp == DMDQN_ROW_R ? rb : rb >> 32);
    }
    reinterpret_cast<uint32_t *>(ring_s + row * DMDQN_ROW_BYTES)[grp] = ws;
    reinterpret_cast<uint32_t *>(ring_n + row * DMDQN_ROW_BYTES)[grp] = wn;
    if (grp == 0) {
        ring_a[row] = (uint8_t)act[agent];
        ring_r[row] = rew[agent];
        ring_d[row] = done[agent] ? 1 : 0;
    }
}

// Float rows (DMDQN_ROWS_F32): one thread per (agent, feature group of 4).
__global__ void k_replay_store_f32(int NA, int cap, int slot, const float *obs_s, const float *obs_n,
                                   const int32_t *act, const double *rew, const uint8_t *done,
                                   float *rows_s, float *rows_n, uint8_t *ring_a, double *ring_r,
                                   uint8_t *ring_d) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    constexpr int G = DMDQN_ROW_FLOATS / 4;
    const int agent = t / G, grp = t - agent * G;
    if (agent >= NA) return;
    const size_t row = (size_t)agent * cap + slot;
    float4 vs = make_float4(0.f, 0.f, 0.f, 0.f), vn = vs;
    float *ps = &vs.x, *pn = &vn.x;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const int i = grp * 4 + q;
        if (i < DMDQN_OBS_DIM) {
            ps[q] = obs_s[(size_t)agent * DMDQN_OBS_DIM + i];
            pn[q] = obs_n[(size_t)agent * DMDQN_OBS_DIM + i];
        }
    }
    reinterpret_cast<float4 *>(rows_s + row * DMDQN_ROW_FLOATS)[grp] = vs;
    reinterpret_cast<float4 *>(rows_n + row * DMDQN_ROW_FLOATS)[grp] = vn;
    if (grp == 0) {
        ring_a[row] = (uint8_t)act[agent];
        ring_r[row] = rew[agent];
        ring_d[row] = done[agent] ? 1 : 0;
    }
}

// xs / xn [NA][batch][96] <- the sampled rows, in batch order.
__global__ void k_replay_gather_f32(const float *rows_s, const float *rows_n, const int32_t *idx,
                                    int NA, int cap, int start, int batch, float *xs, float *xn) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    constexpr int G = DMDQN_ROW_FLOATS / 4;
    const size_t rowi = t / G;
    const int grp = (int)(t - rowi * G);
    if (rowi >= (size_t)NA * batch) return;
    const int agent = (int)(rowi / batch);
    int pos = idx[rowi];
    DMDQN_DBG(pos >= 0 && pos < cap, DBG_LEARN_IDX);  // as the int8 learn's gather
#ifdef DMDQN_DEBUG_BOUNDS
    if (pos < 0 || pos >= cap) pos = 0;
#endif
    int s = start + pos;
    if (s >= cap) s -= cap;
    const size_t src = ((size_t)agent * cap + s) * DMDQN_ROW_FLOATS;
    reinterpret_cast<float4 *>(xs + rowi * DMDQN_ROW_FLOATS)[grp] =
        reinterpret_cast<const float4 *>(rows_s + src)[grp];
    reinterpret_cast<float4 *>(xn + rowi * DMDQN_ROW_FLOATS)[grp] =
        reinterpret_cast<const float4 *>(rows_n + src)[grp];
}

// n-step returns (docs/improvements.md item 7): the transition of the window's
// oldest raw transition, aggregated over up to n staged ones, written into the
// replay ring in the row layout of k_replay_store / k_replay_store_f32.
//
// The staging arrays are a replay ring of n slots per agent (the same layout,
// cap = n); the window is slots head, head+1, ... mod n, oldest first.  With
//   m = the first j in 1..n whose done flag is set, or n
//   R = r_0 + g r_1 + g^2 r_2 + ... + g^(m-1) r_(m-1)
// (w = w * g, R = R + w * r_j: every product and sum one rounded f64 operation,
// in that order) the committed transition is (s_0, a_0, R, s'_(m-1), d_(m-1)).
//
// One thread per (agent, 16-byte chunk of a row): CH chunks cover a row (8 for
// int8 rows, 24 for float rows), each moved with one 16-byte load and store.
// Every lane scans the n done bytes of its agent for m; the lane of chunk MC
// forms R and writes the per-slot arrays -- for int8 rows MC is the chunk that
// holds a, done and r (bytes 96..111 of the s' row), rewritten there.
template <int ROW16, bool I8>
__global__ void k_replay_nstep_commit(dmdqn_nstep_args a) {
    constexpr int CH = ROW16;
    constexpr int MC = I8 ? DMDQN_ROW_A / 16 : 0;
    static_assert(!I8 || (DMDQN_ROW_A % 16 == 0 && DMDQN_ROW_R == DMDQN_ROW_A + 8),
                  "a, done and r share one 16-byte chunk of the s' row");
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int agent = t / CH, ch = t - agent * CH;
    if (agent >= a.NA) return;
    const int n = a.n;
    const size_t st0 = (size_t)agent * n;
    // m - 1 = offset of the window's last entry; pos = its staging slot
    int pos = a.head, last = n - 1;
    for (int j = 0; j < n; j++) {
        if (a.st_d[st0 + pos] != 0) {
            last = j;
            break;
        }
        if (j + 1 < n) pos = pos + 1 == n ? 0 : pos + 1;
    }
    const size_t src_s = (st0 + a.head) * CH + ch, src_n = (st0 + pos) * CH + ch;
    const size_t row = (size_t)agent * a.cap + a.slot;
    const uint4 vs = reinterpret_cast<const uint4 *>(a.st_s)[src_s];
    uint4 vn = reinterpret_cast<const uint4 *>(a.st_n)[src_n];
    if (ch == MC) {
        const double g = a.gamma_a ? a.gamma_a[agent] : a.gamma;
        double R = a.st_r[st0 + a.head], w = 1.0;
        int p = a.head;
        for (int j = 1; j <= last; j++) {
            p = p + 1 == n ? 0 : p + 1;
            w = __dmul_rn(w, g);
            R = __dadd_rn(R, __dmul_rn(w, a.st_r[st0 + p]));
        }
        const uint8_t act = a.st_a[st0 + a.head];
        const uint8_t done = a.st_d[st0 + pos] ? 1 : 0;
        if (I8) {
            const unsigned long long rb = __double_as_longlong(R);
            vn = make_uint4((uint32_t)act | (uint32_t)done << 8, 0u, (uint32_t)rb,
                            (uint32_t)(rb >> 32));
        }
        a.ring_a[row] = act;
        a.ring_r[row] = R;
        a.ring_d[row] = done;
    }
    reinterpret_cast<uint4 *>(a.ring_s)[row * CH + ch] = vs;
    reinterpret_cast<uint4 *>(a.ring_n)[row * CH + ch] = vn;
}

DMDQN_DBG_READER(dbg_flags_replay)

}  // namespace dmdqn

using namespace dmdqn;

extern "C" int dmdqn_replay_nstep_commit(const dmdqn_nstep_args *args, void *stream) {
    DMDQN_REQUIRE(args, "dmdqn_replay_nstep_commit: null args");
    const dmdqn_nstep_args &a = *args;
    DMDQN_REQUIRE(a.n >= 1 && a.n <= DMDQN_NSTEP_MAX,
                  "dmdqn_replay_nstep_commit: n=%d outside 1..%d", a.n, DMDQN_NSTEP_MAX);
    DMDQN_REQUIRE(a.head >= 0 && a.head < a.n, "dmdqn_replay_nstep_commit: head=%d not in [0, %d)",
                  a.head, a.n);
    DMDQN_REQUIRE(a.NA > 0 && a.cap > 0 && a.slot >= 0 && a.slot < a.cap,
                  "dmdqn_replay_nstep_commit: NA=%d cap=%d slot=%d", a.NA, a.cap, a.slot);
    DMDQN_REQUIRE(a.row_format == DMDQN_ROWS_I8 || a.row_format == DMDQN_ROWS_F32,
                  "dmdqn_replay_nstep_commit: unknown row_format %d", a.row_format);
    DMDQN_REQUIRE(a.st_s && a.st_n && a.st_a && a.st_r && a.st_d && a.ring_s && a.ring_n &&
                      a.ring_a && a.ring_r && a.ring_d,
                  "dmdqn_replay_nstep_commit: null pointer");
    DMDQN_REQUIRE(a.gamma_a || (a.gamma >= 0.0 && a.gamma <= 1.0),
                  "dmdqn_replay_nstep_commit: gamma=%g must be finite in [0, 1]", a.gamma);
    constexpr int CH8 = DMDQN_ROW_BYTES / 16, CH32 = DMDQN_ROW_FLOATS * 4 / 16;
    static_assert(DMDQN_ROW_BYTES % 16 == 0 && (DMDQN_ROW_FLOATS * 4) % 16 == 0, "16-byte chunks");
    const bool i8 = a.row_format == DMDQN_ROWS_I8;
    const long long threads = (long long)a.NA * (i8 ? CH8 : CH32);
    DMDQN_REQUIRE(threads <= 0x7fffffffLL, "dmdqn_replay_nstep_commit: NA=%d too large", a.NA);
    const dim3 grid((unsigned)((threads + 255) / 256)), block(256);
    if (i8)
        hipLaunchKernelGGL((k_replay_nstep_commit<CH8, true>), grid, block, 0, as_stream(stream), a);
    else
        hipLaunchKernelGGL((k_replay_nstep_commit<CH32, false>), grid, block, 0, as_stream(stream),
                           a);
    DMDQN_LAUNCH_CHECK("k_replay_nstep_commit");
    return DMDQN_OK;
}

extern "C" int dmdqn_replay_store_f32(int NA, int cap, int slot, const float *obs_s,
                                      const float *obs_n, const int32_t *act, const double *rew,
                                      const uint8_t *done, float *rows_s, float *rows_n,
                                      uint8_t *ring_a, double *ring_r, uint8_t *ring_d,
                                      void *stream) {
    DMDQN_REQUIRE(NA > 0 && cap > 0 && slot >= 0 && slot < cap,
                  "dmdqn_replay_store_f32: NA=%d cap=%d slot=%d", NA, cap, slot);
    DMDQN_REQUIRE(obs_s && obs_n && act && rew && done && rows_s && rows_n && ring_a && ring_r &&
                      ring_d,
                  "dmdqn_replay_store_f32: null pointer");
    const int threads = NA * (DMDQN_ROW_FLOATS / 4);
    hipLaunchKernelGGL(k_replay_store_f32, dim3((threads + 255) / 256), dim3(256), 0,
                       as_stream(stream), NA, cap, slot, obs_s, obs_n, act, rew, done, rows_s,
                       rows_n, ring_a, ring_r, ring_d);
    DMDQN_LAUNCH_CHECK("k_replay_store_f32");
    return DMDQN_OK;
}

extern "C" int dmdqn_replay_gather_f32(const float *rows_s, const float *rows_n,
                                       const int32_t *idx, int NA, int cap, int start, int batch,
                                       float *xs, float *xn, void *stream) {
    DMDQN_REQUIRE(rows_s && rows_n && idx && xs && xn, "dmdqn_replay_gather_f32: null pointer");
    DMDQN_REQUIRE(NA > 0 && cap > 0 && batch > 0 && start >= 0 && start < cap,
                  "dmdqn_replay_gather_f32: NA=%d cap=%d start=%d batch=%d", NA, cap, start, batch);
    const size_t threads = (size_t)NA * batch * (DMDQN_ROW_FLOATS / 4);
    hipLaunchKernelGGL(k_replay_gather_f32, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0,
                       as_stream(stream), rows_s, rows_n, idx, NA, cap, start, batch, xs, xn);
    DMDQN_LAUNCH_CHECK("k_replay_gather_f32");
    return DMDQN_OK;
}

extern "C" int dmdqn_replay_store(int NA, int cap, int slot, const float *obs_s,
                                  const float *obs_n, const int32_t *act, const double *rew,
                                  const uint8_t *done, int8_t *ring_s, int8_t *ring_n,
                                  uint8_t *ring_a, double *ring_r, uint8_t *ring_d,
                                  int32_t *err, void *stream) {
    DMDQN_REQUIRE(NA > 0 && cap > 0 && slot >= 0 && slot < cap,
                  "dmdqn_replay_store: NA=%d cap=%d slot=%d", NA, cap, slot);
    DMDQN_REQUIRE(obs_s && obs_n && act && rew && done && ring_s && ring_n && ring_a && ring_r &&
                      ring_d && err,
                  "dmdqn_replay_store: null pointer");
    const int threads = NA * (DMDQN_ROW_BYTES / 4);
    hipLaunchKernelGGL(k_replay_store, dim3((threads + 255) / 256), dim3(256), 0,
                       as_stream(stream), NA, cap, slot, obs_s, obs_n, act, rew, done, ring_s,
                       ring_n, ring_a, ring_r, ring_d, err);
    DMDQN_LAUNCH_CHECK("k_replay_store");
    return DMDQN_OK;
}
