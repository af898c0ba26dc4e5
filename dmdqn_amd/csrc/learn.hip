// learn.hip -- fused Double-DQN learn step, one workgroup (8 waves) per agent.
//
// Replaces src/agents/dqn_agent.py:328-380 (+ ReplayBuffer.sample's gather and
// reward z-score, :64-84, and the hard target sync :376-377):
//   gather S, S' rows (int8 replay rows -> LDS), z-score the f64 rewards with
//   numpy's pairwise order, a* = argmax online(S'), q_t = target(S')[a*],
//   y = r + gamma (1-d) q_t, q = online(S)[a], L = mean((y-q)^2), backward
//   through the 3 Dense layers, Keras-3 Adam, optional target <- online, or
//   the soft update target <- tau * online + (1 - tau) * target (:389-399).
// All three GEMM chains run on MFMA (v_mfma_f32_16x16x4_f32: exact f32
// products, the strict-parity path).  Work split per layer: 8 waves x one
// 16-wide output-column tile each; the batch (128 rows) is the M dimension.
//
// LDS (H = 128): X f16 [128][96] (replay features are small integers, exact in
// f16) | H1 f32 [128][128] | H2 f32 [128][128] | per-row scratch.
#include <math.h>

#include <type_traits>

#include "common.hpp"
#include "learn_rules.hpp"
#include "qnet_layout.hpp"

namespace dmdqn {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int B_ = LEARN_B; // batch (dqn_agent.py: batch_size 128)
constexpr int D_ = 89;      // observation dim
constexpr int DP = 96;      // padded feature stride of the X image in LDS
constexpr int NACT = 4;

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

template <int H>
struct Lay : QL<H> {
    using QL<H>::P;
    // LDS byte offsets
    static constexpr int X_OFF = 0;
    static constexpr int H1_OFF = B_ * DP * 2;
    static constexpr int H2_OFF = H1_OFF + B_ * H * 4;
    static constexpr int SC_OFF = H2_OFF + B_ * H * 4;
    static constexpr int LDS = SC_OFF + 6400;
    static_assert(SCRATCH_BYTES <= 6400, "per-row scratch");
};

// Y[b][n] = act(X[b][:] . W[:][n] + bias[n]) for the wave's 16-column tile.
// X rows come from LDS (f16 or f32), W^T [N][KS] (tiled, qn_wt; KS = 0: the
// layer-1 block, qn_w1) from global memory.
template <int H, int K, typename TX, bool RELU, int KS>
__device__ __forceinline__ void dense_tile(const TX *X, int ldx, const float *WT, const float *bias,
                                           float *Y, int ldy, int n0, int nvalid) {
    const int l = threadIdx.x & 63, lr = l & 15, lk = l >> 4;
    f32x4 acc[8];
#pragma unroll
    for (int t = 0; t < 8; t++) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int n = n0 + lr;
    for (int k0 = 0; k0 < K; k0 += 4) {
        const int kk = k0 + lk;
        const float bv =
            (kk < K && lr < nvalid) ? WT[KS == 0 ? qn_w1<H>(n, kk) : qn_wt(n, kk, KS)] : 0.0f;
#pragma unroll
        for (int t = 0; t < 8; t++) {
            const float av = (float)X[(16 * t + lr) * ldx + kk];
            acc[t] = mfma4(av, bv, acc[t]);
        }
    }
    if (lr < nvalid) {
        const float bb = bias[n];
#pragma unroll
        for (int t = 0; t < 8; t++)
#pragma unroll
            for (int j = 0; j < 4; j++) {
                float z = acc[t][j] + bb;
                if (RELU) z = z > 0.0f ? z : 0.0f;
                Y[(16 * t + 4 * lk + j) * ldy + n] = z;
            }
    }
}

// Full forward of one 128-row batch: H1, H2 (post-ReLU) in LDS, Q -> z3[128][4].
// X: the f16 LDS image (int8 rows) or the f32 pre-gathered rows (float rows).
// HP (unused here): the per-agent-hyperparameter kernels call their own copy, so
// the inliner sees the scalar kernels' copy with the callers it always had.
template <int H, typename TX, bool HP = false>
__device__ void forward(const float *P, const TX *X, float *H1, float *H2, float *z3) {
    using L = Lay<H>;
    const int w = threadIdx.x >> 6;
    constexpr int NT = H / 16;  // column tiles per layer
    for (int nt = w; nt < NT; nt += 8)
        dense_tile<H, D_, TX, true, 0>(X, DP, P + L::oW1T, P + L::ob1, H1, H, 16 * nt, 16);
    __syncthreads();
    for (int nt = w; nt < NT; nt += 8)
        dense_tile<H, H, float, true, H>(H1, H, P + L::oW2T, P + L::ob2, H2, H, 16 * nt, 16);
    __syncthreads();
    // output layer: 4 columns; wave w computes batch tile w (K = H)
    {
        const int l = threadIdx.x & 63, lr = l & 15, lk = l >> 4;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        const float *W3T = P + L::oW3T;
        for (int k0 = 0; k0 < H; k0 += 4) {
            const int kk = k0 + lk;
            const float bv = lr < NACT ? W3T[lr * H + kk] : 0.0f;
            const float av = H2[(16 * w + lr) * H + kk];
            acc = mfma4(av, bv, acc);
        }
        if (lr < NACT) {
            const float bb = P[L::ob3 + lr];
#pragma unroll
            for (int j = 0; j < 4; j++) z3[(16 * w + 4 * lk + j) * NACT + lr] = acc[j] + bb;
        }
    }
    __syncthreads();
}

struct AdamK {
    float alpha, c1, c2, eps;
    float tau, omt;  // soft target update (dqn_agent.py:389-399) when soft
    bool soft;
};

// Keras-3 Adam (keras_adam_el) on element i, then the target write-out.
__device__ __forceinline__ void adam_el(float *w, float *m, float *v, float *tgt, size_t i,
                                        float g, const AdamK &K, bool sync) {
    float mi = m[i], vi = v[i], wi = w[i];
    keras_adam_el(wi, mi, vi, g, K.alpha, K.c1, K.c2, K.eps);
    m[i] = mi;
    v[i] = vi;
    w[i] = wi;
    if (sync) tgt[i] = wi;  // the hard copy wins over the soft rule (:372-377)
    else if (K.soft) tgt[i] = soft_el(wi, tgt[i], K.tau, K.omt);
}

// XF: float replay rows (DMDQN_ROWS_F32): X(S') / X(S) are read as f32 from the
// pre-gathered a.xn / a.xs (global, batch order) instead of the f16 LDS image.
// HP: per-agent hyperparameters (dmdqn_agent_hparams) replace the launch
// scalars of this workgroup's agent at entry (hp_apply); the scalar
// instantiations take an empty block in its place (no kernel argument: their
// signature, and so their code, is that of a kernel without the feature).
struct NoHp {};
template <bool HP>
using HpArg = typename std::conditional<HP, dmdqn_agent_hparams, NoHp>::type;

template <int H, bool XF, bool HP = false>
__global__ void __launch_bounds__(512) k_learn_f32(dmdqn_learn_args a, HpArg<HP> hp) {
    using L = Lay<H>;
    __shared__ __attribute__((aligned(16))) char smem[L::LDS];
    _Float16 *XL = (_Float16 *)(smem + L::X_OFF);
    using TX = typename std::conditional<XF, float, _Float16>::type;
    float *H1 = (float *)(smem + L::H1_OFF);
    float *H2 = (float *)(smem + L::H2_OFF);
    const Scratch S = scratch_at(smem + L::SC_OFF);
    const int agent = blockIdx.x;
    if constexpr (HP) hp_apply(a, hp, agent);
    const int tid = threadIdx.x, w = tid >> 6, l = tid & 63;
    const size_t P = (size_t)a.P;
    float *Wp = a.params + agent * P, *Mp = a.adam_m + agent * P, *Vp = a.adam_v + agent * P;
    float *Tp = a.target + agent * P;
    const bool sync = a.sync_target != 0;
    const AdamK AK{a.alpha, a.c1, a.c2, a.eps, a.tau, a.one_minus_tau, a.tau > 0.0f};

    // ---- P0: batch metadata (ReplayBuffer.sample :63-64 via deque positions)
    if (tid < B_) {
        int pos = a.idx[(size_t)agent * B_ + tid];
        DMDQN_DBG(pos >= 0 && pos < a.cap, DBG_LEARN_IDX);
#ifdef DMDQN_DEBUG_BOUNDS
        if (pos < 0 || pos >= a.cap) pos = 0;
#endif
        int s = a.start + pos;
        if (s >= a.cap) s -= a.cap;
        size_t r = (size_t)agent * a.cap + s;
        S.slot[tid] = s;
        S.act[tid] = a.ring_a[r];
        DMDQN_DBG(S.act[tid] < NACT, DBG_LEARN_ACT);
#ifdef DMDQN_DEBUG_BOUNDS
        if (S.act[tid] >= NACT) S.act[tid] = 0;
#endif
        S.r64[tid] = a.ring_r[r];
        S.dn[tid] = a.ring_d[r] ? 1.0f : 0.0f;
    }
    // ---- reward z-score (its first barrier completes the metadata)
    zscore(S);
    if (a.rn_out && tid < B_) a.rn_out[(size_t)agent * B_ + tid] = S.rn[tid];

    // ---- P1: gather S' rows
    auto gather = [&](const int8_t *ring) {
        for (int t = tid; t < B_ * (DP / 4); t += 512) {
            int b = t / (DP / 4), q = t - b * (DP / 4);
            const char4 c = reinterpret_cast<const char4 *>(
                ring + ((size_t)agent * a.cap + S.slot[b]) * DMDQN_ROW_BYTES)[q];
            _Float16 *dst = XL + b * DP + 4 * q;
            dst[0] = (_Float16)(float)c.x;
            dst[1] = (_Float16)(float)c.y;
            dst[2] = (_Float16)(float)c.z;
            dst[3] = (_Float16)(float)c.w;
        }
        __syncthreads();
    };
    const TX *X;
    if constexpr (XF) {
        X = a.xn + (size_t)agent * B_ * DP;
    } else {
        gather(a.ring_n);
        X = XL;
    }
    // ---- P2: target forward on S' -> z3 ; P3: online forward on S' -> a*, y
    forward<H, TX, HP>(a.target + agent * P, X, H1, H2, S.z3);
    // online forward on S': layer 3 reads H2 only, so its Q goes to the H1 region
    forward<H, TX, HP>(Wp, X, H1, H2, H1);
    ddqn_target(a, H1, S);
    // ---- P4/P5: gather S, online forward keeping H1, H2; q, loss, dq
    if constexpr (XF) {
        X = a.xs + (size_t)agent * B_ * DP;
    } else {
        gather(a.ring_s);
        X = XL;
    }
    forward<H, TX, HP>(Wp, X, H1, H2, S.z3);
    if (a.qstats) learn_qstats(a.qstats, agent, S.z3, S.act);
    loss_rows(a, agent, S, [&](int row, float dq) { S.dq[row] = dq; });

    // ---- backward
    // dW3[k][a] = sum_b H2[b][k] dq3[b][a] ; db3[a]  (VALU, one thread per element)
    float g3 = 0.0f, gb3 = 0.0f;
    for (int e = tid; e < H * NACT; e += 512) {
        int k = e >> 2, ac = e & 3;
        float s = 0.0f;
        for (int b = 0; b < B_; b++)
            if (S.act[b] == ac) s += H2[b * H + k] * S.dq[b];
        g3 = s;
    }
    if (tid < NACT) {
        float s = 0.0f;
        for (int b = 0; b < B_; b++)
            if (S.act[b] == tid) s += S.dq[b];
        gb3 = s;
    }
    __syncthreads();
    // dZ2 = dq * W3[:, a] masked by ReLU; overwrite H2 in place
    {
        const float *W3T = Wp + L::oW3T;
        for (int e = tid; e < B_ * H; e += 512) {
            int b = e / H, k = e - b * H;
            float h = H2[e];
            H2[e] = h > 0.0f ? S.dq[b] * W3T[S.act[b] * H + k] : 0.0f;
        }
    }
    __syncthreads();
    float gb2 = 0.0f;
    if (tid < H) {
        float s = 0.0f;
        for (int b = 0; b < B_; b++) s += H2[b * H + tid];
        gb2 = s;
    }
    // dW2[j][k] = sum_b H1[b][j] dZ2[b][k]: wave w owns j-tile(s), 8 k-tiles each
    constexpr int NT = H / 16;
    constexpr int QT = (NT + 7) / 8;  // j-tiles per wave
    f32x4 g2[QT][NT];
    {
        const int lr = l & 15, lk = l >> 4;
#pragma unroll
        for (int q = 0; q < QT; q++)
#pragma unroll
            for (int t = 0; t < NT; t++) g2[q][t] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int jt = w, q = 0; jt < NT; jt += 8, q++) {
            for (int b0 = 0; b0 < B_; b0 += 4) {
                const int b = b0 + lk;
                const float av = H1[b * H + 16 * jt + lr];
#pragma unroll
                for (int t = 0; t < NT; t++) g2[q][t] = mfma4(av, H2[b * H + 16 * t + lr], g2[q][t]);
            }
        }
    }
    // dH1[b][j] = sum_k dZ2[b][k] W2[j][k]: wave w owns batch tile w, all j tiles
    f32x4 d1[NT];
    {
        const int lr = l & 15, lk = l >> 4;
        const float *W2T = Wp + L::oW2T;
#pragma unroll
        for (int t = 0; t < NT; t++) d1[t] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int k0 = 0; k0 < H; k0 += 4) {
            const int k = k0 + lk;
            const float av = H2[(16 * w + lr) * H + k];
#pragma unroll
            for (int t = 0; t < NT; t++) d1[t] = mfma4(av, W2T[qn_wt(k, 16 * t + lr, H)], d1[t]);
        }
    }
    __syncthreads();  // everyone done reading H1 (dW2) and old W2 (dH1)
    // dZ1 = dH1 masked by ReLU(H1) -> H1 in place
    {
        const int lr = l & 15, lk = l >> 4;
#pragma unroll
        for (int t = 0; t < NT; t++)
#pragma unroll
            for (int j = 0; j < 4; j++) {
                int idx = (16 * w + 4 * lk + j) * H + 16 * t + lr;
                H1[idx] = H1[idx] > 0.0f ? d1[t][j] : 0.0f;
            }
    }
    // Adam on W2 from the dW2 accumulators (old W2 no longer read)
    {
        const int lr = l & 15, lk = l >> 4;
        for (int jt = w, q = 0; jt < NT; jt += 8, q++)
#pragma unroll
            for (int t = 0; t < NT; t++)
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    size_t i = L::oW2T + qn_wt(16 * t + lr, 16 * jt + 4 * lk + j, H);
                    adam_el(Wp, Mp, Vp, Tp, i, g2[q][t][j], AK, sync);
                }
    }
    __syncthreads();
    // db1 and dW1[i][j] = sum_b X[b][i] dZ1[b][j]; wave owns j-tile, 6 i-tiles
    float gb1 = 0.0f;
    if (tid < H) {
        float s = 0.0f;
        for (int b = 0; b < B_; b++) s += H1[b * H + tid];
        gb1 = s;
    }
    {
        const int lr = l & 15, lk = l >> 4;
        constexpr int IT = DP / 16;  // 6 tiles cover i < 96
        for (int jt = w; jt < NT; jt += 8) {
            f32x4 g1[IT];
#pragma unroll
            for (int t = 0; t < IT; t++) g1[t] = f32x4{0.f, 0.f, 0.f, 0.f};
            for (int b0 = 0; b0 < B_; b0 += 4) {
                const int b = b0 + lk;
                const float bv = H1[b * H + 16 * jt + lr];
#pragma unroll
                for (int t = 0; t < IT; t++)
                    g1[t] = mfma4((float)X[b * DP + 16 * t + lr], bv, g1[t]);
            }
#pragma unroll
            for (int t = 0; t < IT; t++)
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    int i = 16 * t + 4 * lk + j;
                    if (i < D_) adam_el(Wp, Mp, Vp, Tp, L::oW1T + qn_w1<H>(16 * jt + lr, i),
                                        g1[t][j], AK, sync);
                }
        }
    }
    // biases and W3
    if (tid < H) {
        adam_el(Wp, Mp, Vp, Tp, L::ob1 + tid, gb1, AK, sync);
        adam_el(Wp, Mp, Vp, Tp, L::ob2 + tid, gb2, AK, sync);
    }
    for (int e = tid; e < H * NACT; e += 512)
        adam_el(Wp, Mp, Vp, Tp, L::oW3T + (size_t)(e & 3) * H + (e >> 2), g3, AK, sync);
    if (tid < NACT) adam_el(Wp, Mp, Vp, Tp, L::ob3 + tid, gb3, AK, sync);
}

// ------------------------------------------------------------------ greedy act
// The online forward of select_action's greedy branch (dqn_agent.py:268-273)
// under the learn's precision policy: PREC 0 f32; 1 / 2 Keras mixed_float16 /
// mixed_bfloat16 (learn_h16.hpp): weights, biases and inputs cast to 16 bits,
// f32 sums, each matmul result rounded, the bias add rounded again, 16-bit
// Q values -- so the argmax (first max) sees the values Keras' would.
template <int PREC>
__device__ __forceinline__ float rq(float x) {
    if constexpr (PREC == 1) return (float)(_Float16)x;
    else if constexpr (PREC == 2) return (float)(__bf16)x;
    else return x;
}

template <int H, int PREC>
__global__ void __launch_bounds__(256) k_q_argmax(const float *params, size_t pstride,
                                                  const float *obs, int32_t *out, float *q_out) {
    using L = Lay<H>;
    __shared__ float x[D_], h1[H], h2[H], q[NACT];
    const int agent = blockIdx.x, tid = threadIdx.x;
    const float *Wp = params + (size_t)agent * pstride;  // pstride 0: one shared net
    for (int i = tid; i < D_; i += blockDim.x) x[i] = rq<PREC>(obs[(size_t)agent * D_ + i]);
    __syncthreads();
    for (int j = tid; j < H; j += blockDim.x) {
        float s = 0.0f;
        for (int i = 0; i < D_; i++) s += x[i] * rq<PREC>(Wp[L::oW1T + qn_w1<H>(j, i)]);
        s = rq<PREC>(rq<PREC>(s) + rq<PREC>(Wp[L::ob1 + j]));
        h1[j] = s > 0.0f ? s : 0.0f;
    }
    __syncthreads();
    for (int k = tid; k < H; k += blockDim.x) {
        float s = 0.0f;
        for (int j = 0; j < H; j++) s += h1[j] * rq<PREC>(Wp[L::oW2T + qn_wt(k, j, H)]);
        s = rq<PREC>(rq<PREC>(s) + rq<PREC>(Wp[L::ob2 + k]));
        h2[k] = s > 0.0f ? s : 0.0f;
    }
    __syncthreads();
    if (tid < NACT) {
        float s = 0.0f;
        for (int k = 0; k < H; k++) s += h2[k] * rq<PREC>(Wp[L::oW3T + tid * H + k]);
        q[tid] = rq<PREC>(rq<PREC>(s) + rq<PREC>(Wp[L::ob3 + tid]));
    }
    __syncthreads();
    if (tid == 0) {
        int best = 0;
        for (int k = 1; k < NACT; k++)
            if (q[k] > q[best]) best = k;
        out[agent] = best;
        if (q_out)
            for (int k = 0; k < NACT; k++) q_out[(size_t)agent * NACT + k] = q[k];
    }
}

// learn_f16.hip / learn_bf16.hip; hp: never null (a block of null arrays = none)
int launch_learn_f16(const dmdqn_learn_args *a, const dmdqn_agent_hparams *hp, hipStream_t s);
int launch_learn_bf16(const dmdqn_learn_args *a, const dmdqn_agent_hparams *hp, hipStream_t s);
int launch_learn_pair_f16(const dmdqn_learn_args *a0, const dmdqn_learn_args *a1,
                          const dmdqn_agent_hparams *hp0, const dmdqn_agent_hparams *hp1, bool soft,
                          hipStream_t s);
int launch_learn_pair_bf16(const dmdqn_learn_args *a0, const dmdqn_learn_args *a1,
                           const dmdqn_agent_hparams *hp0, const dmdqn_agent_hparams *hp1,
                           bool soft, hipStream_t s);
int launch_learn_grad_f16(const dmdqn_learn_args *a, const dmdqn_agent_hparams *hp, float *grad,
                          hipStream_t s);
int launch_learn_grad_bf16(const dmdqn_learn_args *a, const dmdqn_agent_hparams *hp, float *grad,
                           hipStream_t s);
int launch_adam_agents_f16(const dmdqn_learn_args *a, const dmdqn_agent_hparams *hp,
                           const float *grad, hipStream_t s);
int launch_adam_agents_bf16(const dmdqn_learn_args *a, const dmdqn_agent_hparams *hp,
                            const float *grad, hipStream_t s);
int check_tau(const char *who, float tau, float omt, bool zero_ok);

// Soft target update outside a learn (dqn_agent.py:389-399,
// update_target_network_soft): target <- soft_el(params, target) for NW nets of
// P parameters, and the 16-bit shadow (RNE cast of the new f32 target) when
// target_h is given.  One lane per 4 consecutive parameters (16-byte f32
// accesses, one 8-byte shadow store); P4 = P / 4 lanes per net, n4 = NW * P4.
// PN: one tau per net (dmdqn_target_soft_update_hp), tau_a / omt_a [NW] read by
// the lane's net; otherwise the launch scalars.
template <typename T16, bool PN = false>
__global__ void __launch_bounds__(256) k_target_soft(const float *params, float *target,
                                                     T16 *target_h, int P4, int Ph, long n4,
                                                     float tau, float omt, const float *tau_a,
                                                     const float *omt_a) {
    const long q = (long)blockIdx.x * 256 + threadIdx.x;
    if (q >= n4) return;
    if constexpr (PN) {
        tau = tau_a[q / P4];
        omt = omt_a[q / P4];
    }
    const float4 w = reinterpret_cast<const float4 *>(params)[q];
    const float4 t = soft_el4(w, reinterpret_cast<const float4 *>(target)[q], tau, omt);
    reinterpret_cast<float4 *>(target)[q] = t;
    if (target_h) {
        // (shadow4's store, learn_rules.hpp, with this kernel's own index order)
        const long net = q / P4, k = q - net * P4;
        typedef T16 t16x4 __attribute__((ext_vector_type(4)));
        t16x4 hv;
        hv[0] = (T16)t.x; hv[1] = (T16)t.y; hv[2] = (T16)t.z; hv[3] = (T16)t.w;
        *reinterpret_cast<t16x4 *>(target_h + net * Ph + 4 * k) = hv;
    }
}

// The launch behind dmdqn_target_soft_update; also the second launch of a
// 16-bit soft learn that does not run fused (learn_h16.hpp: target_h == NULL,
// or fewer agents than SOFT_FUSED_MIN_NA).
// tau_a / omt_a: one tau per net ([NW], both or neither) in place of tau / omt.
int launch_target_soft(const float *params, float *target, uint16_t *target_h, int NW, int P,
                       int Ph, int precision, float tau, float omt, const float *tau_a,
                       const float *omt_a, hipStream_t s) {
    const long n4 = (long)NW * (P / 4);
    const dim3 grid((unsigned)((n4 + 255) / 256));
    if (precision == 2) {
        auto k = tau_a ? k_target_soft<__bf16, true> : k_target_soft<__bf16, false>;
        hipLaunchKernelGGL(k, grid, dim3(256), 0, s, params, target,
                           reinterpret_cast<__bf16 *>(target_h), P / 4, Ph, n4, tau, omt, tau_a,
                           omt_a);
    } else {
        auto k = tau_a ? k_target_soft<_Float16, true> : k_target_soft<_Float16, false>;
        hipLaunchKernelGGL(k, grid, dim3(256), 0, s, params, target,
                           reinterpret_cast<_Float16 *>(target_h), P / 4, Ph, n4, tau, omt, tau_a,
                           omt_a);
    }
    DMDQN_LAUNCH_CHECK("k_target_soft");
    return DMDQN_OK;
}

DMDQN_DBG_READER(dbg_flags_learn)

}  // namespace dmdqn

using namespace dmdqn;

static int check_learn_args(const dmdqn_learn_args *a) {
    DMDQN_REQUIRE(a, "dmdqn_learn: null args");
    DMDQN_REQUIRE(a->NA > 0 && a->cap >= a->batch && a->start >= 0 && a->start < a->cap,
                  "dmdqn_learn: NA=%d cap=%d start=%d", a->NA, a->cap, a->start);
    DMDQN_REQUIRE(a->batch == B_, "dmdqn_learn: batch must be %d (got %d)", B_, a->batch);
    DMDQN_REQUIRE(a->row_format == DMDQN_ROWS_I8 || a->row_format == DMDQN_ROWS_F32,
                  "dmdqn_learn: row_format %d", a->row_format);
    DMDQN_REQUIRE((a->row_format == DMDQN_ROWS_F32 ? (a->xs && a->xn) : (a->ring_s && a->ring_n)) &&
                      a->ring_a && a->ring_d && a->ring_r && a->idx && a->params && a->adam_m &&
                      a->adam_v && a->target,
                  "dmdqn_learn: null pointer");
    DMDQN_REQUIRE(a->precision >= 0 && a->precision <= 2, "dmdqn_learn: precision %d",
                  a->precision);
    DMDQN_REQUIRE(a->loss_kind == DMDQN_LOSS_MSE || a->loss_kind == DMDQN_LOSS_HUBER,
                  "dmdqn_learn: loss_kind %d", a->loss_kind);
    return DMDQN_OK;
}

// The soft target update's constants (dmdqn_learn_args.tau / .one_minus_tau):
// tau finite in [0, 1] (zero_ok: 0 = off) or (0, 1], and one_minus_tau in
// [0, 1] when the update is on.  The negated comparisons refuse a NaN.
int dmdqn::check_tau(const char *who, float tau, float omt, bool zero_ok) {
    DMDQN_REQUIRE(tau >= 0.0f && tau <= 1.0f && (zero_ok || tau > 0.0f),
                  "%s: tau=%g must be in %s0, 1]", who, (double)tau, zero_ok ? "[" : "(");
    DMDQN_REQUIRE(!(tau > 0.0f) || (omt >= 0.0f && omt <= 1.0f),
                  "%s: one_minus_tau=%g must be in [0, 1]", who, (double)omt);
    return DMDQN_OK;
}

// The host checks of a dmdqn_agent_hparams block (include/dmdqn.h); *out: the
// block the launchers receive, all-null for hp == NULL.  The negated
// comparisons refuse a NaN.
static int check_hparams(const char *who, const dmdqn_agent_hparams *hp, dmdqn_agent_hparams *out) {
    *out = dmdqn_agent_hparams{};
    if (!hp) return DMDQN_OK;
    DMDQN_REQUIRE((hp->tau != nullptr) == (hp->one_minus_tau != nullptr),
                  "%s: tau and one_minus_tau go together (tau=%p one_minus_tau=%p)", who,
                  (const void *)hp->tau, (const void *)hp->one_minus_tau);
    DMDQN_REQUIRE(!hp->lr || (hp->adam_s > 0.0f && hp->adam_s <= 1.0f && hp->adam_d > 0.0f &&
                              hp->adam_d <= 1.0f),
                  "%s: with lr, adam_s=%g and adam_d=%g must be in (0, 1]", who,
                  (double)hp->adam_s, (double)hp->adam_d);
    *out = *hp;
    return DMDQN_OK;
}

template <int H>
static void launch_learn_f32(const dmdqn_learn_args *a, const dmdqn_agent_hparams &hp,
                             hipStream_t s) {
    const bool xf = a->row_format == DMDQN_ROWS_F32;
    if (hp_any(hp)) {
        auto k = xf ? k_learn_f32<H, true, true> : k_learn_f32<H, false, true>;
        hipLaunchKernelGGL(k, dim3(a->NA), dim3(512), 0, s, *a, hp);
    } else {
        auto k = xf ? k_learn_f32<H, true> : k_learn_f32<H, false>;
        hipLaunchKernelGGL(k, dim3(a->NA), dim3(512), 0, s, *a, NoHp{});
    }
}

// dmdqn_learn / dmdqn_learn_hp (`who` names the entry point in messages)
static int learn_entry(const char *who, const dmdqn_learn_args *a, const dmdqn_agent_hparams *hpp,
                       void *stream) {
    DMDQN_REQUIRE(a, "%s: null args", who);
    dmdqn_agent_hparams hp;
    if (int rc = check_hparams(who, hpp, &hp)) return rc;
    if (int rc = check_tau(who, a->tau, a->one_minus_tau, true)) return rc;
    if (int rc = check_learn_args(a)) return rc;
    if (a->precision == 1) return launch_learn_f16(a, &hp, as_stream(stream));
    if (a->precision == 2) return launch_learn_bf16(a, &hp, as_stream(stream));
    if (a->hidden == 128) {
        DMDQN_REQUIRE(a->P == Lay<128>::P, "dmdqn_learn: P=%d != %d", a->P, Lay<128>::P);
        launch_learn_f32<128>(a, hp, as_stream(stream));
    } else if (a->hidden == 64) {
        DMDQN_REQUIRE(a->P == Lay<64>::P, "dmdqn_learn: P=%d != %d", a->P, Lay<64>::P);
        launch_learn_f32<64>(a, hp, as_stream(stream));
    } else {
        DMDQN_REQUIRE(false, "dmdqn_learn: hidden must be 64 or 128 (got %d)", a->hidden);
    }
    DMDQN_LAUNCH_CHECK("k_learn");
    return DMDQN_OK;
}

extern "C" int dmdqn_learn(const dmdqn_learn_args *a, void *stream) {
    return learn_entry("dmdqn_learn", a, nullptr, stream);
}

extern "C" int dmdqn_learn_hp(const dmdqn_learn_args *a, const dmdqn_agent_hparams *hp,
                              void *stream) {
    return learn_entry("dmdqn_learn_hp", a, hp, stream);
}

// Two consecutive learns of every agent in one launch (include/dmdqn.h).
extern "C" int dmdqn_learn_pair(const dmdqn_learn_args *a0, const dmdqn_learn_args *a1,
                                const dmdqn_agent_hparams *hpp0, const dmdqn_agent_hparams *hpp1,
                                void *stream) {
    const char *who = "dmdqn_learn_pair";
    DMDQN_REQUIRE(a0 && a1, "%s: null args", who);
    dmdqn_agent_hparams hp0, hp1;
    if (int rc = check_hparams(who, hpp0, &hp0)) return rc;
    if (int rc = check_hparams(who, hpp1, &hp1)) return rc;
    if (int rc = check_tau(who, a0->tau, a0->one_minus_tau, true)) return rc;
    if (int rc = check_tau(who, a1->tau, a1->one_minus_tau, true)) return rc;
    if (int rc = check_learn_args(a0)) return rc;
    if (int rc = check_learn_args(a1)) return rc;
    DMDQN_REQUIRE(a0->params == a1->params && a0->adam_m == a1->adam_m &&
                      a0->adam_v == a1->adam_v && a0->target == a1->target &&
                      a0->target_h == a1->target_h && a0->ring_s == a1->ring_s &&
                      a0->ring_n == a1->ring_n && a0->ring_a == a1->ring_a &&
                      a0->ring_d == a1->ring_d && a0->ring_r == a1->ring_r && a0->NA == a1->NA &&
                      a0->cap == a1->cap,
                  "%s: the two learns must share params, adam_m, adam_v, target, target_h, the "
                  "rings, NA and cap", who);
    DMDQN_REQUIRE((a0->precision == 1 || a0->precision == 2) && a1->precision == a0->precision &&
                      a0->hidden == 128 && a1->hidden == 128 && a0->P == a1->P,
                  "%s: precision %d / %d, hidden %d / %d (16-bit learns of hidden 128 only)", who,
                  a0->precision, a1->precision, a0->hidden, a1->hidden);
    DMDQN_REQUIRE(a0->row_format == DMDQN_ROWS_I8 && a1->row_format == DMDQN_ROWS_I8,
                  "%s: int8 replay rows only", who);
    DMDQN_REQUIRE(a0->target_h, "%s: needs the 16-bit target shadow (target_h)", who);
    DMDQN_REQUIRE(!a0->sync_target && !a1->sync_target,
                  "%s: a learn with sync_target runs as a single launch (dmdqn_learn)", who);
    const bool soft0 = a0->tau > 0.0f || hp0.tau, soft1 = a1->tau > 0.0f || hp1.tau;
    DMDQN_REQUIRE(soft0 == soft1, "%s: one learn has a soft target update, the other has not",
                  who);
    DMDQN_REQUIRE((a0->qstats != nullptr) == (a1->qstats != nullptr),
                  "%s: qstats for both learns or for neither", who);
    // outputs of one learn each: the second learn must not write over the first's
    DMDQN_REQUIRE((!a0->loss || a0->loss != a1->loss) && (!a0->qstats || a0->qstats != a1->qstats) &&
                      (!a0->rn_out || a0->rn_out != a1->rn_out),
                  "%s: loss, qstats and rn_out must be buffers of each learn's own", who);
    DMDQN_REQUIRE(!a0->stamps && !a1->stamps,
                  "%s: stamps (one phase record per workgroup) take a single launch", who);
    return a0->precision == 1
               ? launch_learn_pair_f16(a0, a1, &hp0, &hp1, soft0, as_stream(stream))
               : launch_learn_pair_bf16(a0, a1, &hp0, &hp1, soft0, as_stream(stream));
}

static int learn_grad_entry(const char *who, const dmdqn_learn_args *a,
                            const dmdqn_agent_hparams *hpp, float *grad, void *stream) {
    dmdqn_agent_hparams hp;
    if (int rc = check_hparams(who, hpp, &hp)) return rc;
    if (int rc = check_learn_args(a)) return rc;
    DMDQN_REQUIRE(grad, "%s: null grad", who);
    DMDQN_REQUIRE(a->precision == 1 || a->precision == 2,
                  "%s: precision %d (the split learn is fp16 / bf16 only)", who, a->precision);
    return a->precision == 1 ? launch_learn_grad_f16(a, &hp, grad, as_stream(stream))
                             : launch_learn_grad_bf16(a, &hp, grad, as_stream(stream));
}

extern "C" int dmdqn_learn_grad(const dmdqn_learn_args *a, float *grad, void *stream) {
    return learn_grad_entry("dmdqn_learn_grad", a, nullptr, grad, stream);
}

extern "C" int dmdqn_learn_grad_hp(const dmdqn_learn_args *a, const dmdqn_agent_hparams *hp,
                                   float *grad, void *stream) {
    return learn_grad_entry("dmdqn_learn_grad_hp", a, hp, grad, stream);
}

static int adam_agents_entry(const char *who, const dmdqn_learn_args *a,
                             const dmdqn_agent_hparams *hpp, const float *grad, void *stream) {
    dmdqn_agent_hparams hp;
    if (int rc = check_hparams(who, hpp, &hp)) return rc;
    DMDQN_REQUIRE(a && grad && a->NA > 0 && a->params && a->adam_m && a->adam_v && a->target,
                  "%s: null argument", who);
    DMDQN_REQUIRE(a->precision == 1 || a->precision == 2, "%s: precision %d (fp16 / bf16 only)",
                  who, a->precision);
    if (int rc = check_tau(who, a->tau, a->one_minus_tau, true)) return rc;
    return a->precision == 1 ? launch_adam_agents_f16(a, &hp, grad, as_stream(stream))
                             : launch_adam_agents_bf16(a, &hp, grad, as_stream(stream));
}

extern "C" int dmdqn_adam_agents(const dmdqn_learn_args *a, const float *grad, void *stream) {
    return adam_agents_entry("dmdqn_adam_agents", a, nullptr, grad, stream);
}

extern "C" int dmdqn_adam_agents_hp(const dmdqn_learn_args *a, const dmdqn_agent_hparams *hp,
                                    const float *grad, void *stream) {
    return adam_agents_entry("dmdqn_adam_agents_hp", a, hp, grad, stream);
}

template <int H>
static void launch_q_argmax(int precision, int NA, const float *params, size_t pstride,
                            const float *obs, int32_t *out, float *q_out, void *stream) {
    auto k = precision == 1 ? k_q_argmax<H, 1> : precision == 2 ? k_q_argmax<H, 2> : k_q_argmax<H, 0>;
    hipLaunchKernelGGL(k, dim3(NA), dim3(H), 0, as_stream(stream), params, pstride, obs, out, q_out);
}

static int q_argmax(const float *params, size_t pstride, int NA, int P, int hidden, int precision,
                    const float *obs, int32_t *out, float *q_out, void *stream) {
    DMDQN_REQUIRE(params && obs && out && NA > 0, "dmdqn_q_argmax: bad args");
    DMDQN_REQUIRE(precision >= 0 && precision <= 2, "dmdqn_q_argmax: precision %d", precision);
    if (hidden == 128) {
        DMDQN_REQUIRE(P == Lay<128>::P, "dmdqn_q_argmax: P");
        launch_q_argmax<128>(precision, NA, params, pstride, obs, out, q_out, stream);
    } else if (hidden == 64) {
        DMDQN_REQUIRE(P == Lay<64>::P, "dmdqn_q_argmax: P");
        launch_q_argmax<64>(precision, NA, params, pstride, obs, out, q_out, stream);
    } else {
        DMDQN_REQUIRE(false, "dmdqn_q_argmax: hidden must be 64 or 128");
    }
    DMDQN_LAUNCH_CHECK("k_q_argmax");
    return DMDQN_OK;
}

extern "C" int dmdqn_q_argmax(const float *params, int NA, int P, int hidden, int precision,
                              const float *obs, int32_t *out, float *q_out, void *stream) {
    return q_argmax(params, (size_t)P, NA, P, hidden, precision, obs, out, q_out, stream);
}

extern "C" int dmdqn_q_argmax_shared(const float *params, int NA, int P, int hidden, int precision,
                                     const float *obs, int32_t *out, float *q_out, void *stream) {
    return q_argmax(params, 0, NA, P, hidden, precision, obs, out, q_out, stream);
}

// Hard target sync outside a learn (dqn_agent.py:382-387, update_target_network):
// target <- params for NW nets, and the 16-bit shadow the target forward reads
// (RNE; f16 or bf16) when target_h is given.
template <typename T16>
__global__ void __launch_bounds__(256) k_target_sync(const float *params, float *target,
                                                     T16 *target_h, int P, int Ph, long n) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const long w = i / P, k = i - w * P;
    const float x = params[i];
    target[i] = x;
    if (target_h) target_h[w * Ph + k] = (T16)x;
}

extern "C" int dmdqn_target_sync(const float *params, float *target, uint16_t *target_h, int NW,
                                 int P, int Ph, int precision, void *stream) {
    DMDQN_REQUIRE(params && target && NW > 0 && P > 0 && Ph >= P,
                  "dmdqn_target_sync: NW=%d P=%d Ph=%d", NW, P, Ph);
    DMDQN_REQUIRE(precision >= 0 && precision <= 2, "dmdqn_target_sync: precision %d", precision);
    DMDQN_REQUIRE(!target_h || precision != 0, "dmdqn_target_sync: fp32 has no 16-bit shadow");
    const long n = (long)NW * P;
    const dim3 grid((unsigned)((n + 255) / 256));
    if (precision == 2)
        hipLaunchKernelGGL(k_target_sync<__bf16>, grid, dim3(256), 0, as_stream(stream), params,
                           target, reinterpret_cast<__bf16 *>(target_h), P, Ph, n);
    else
        hipLaunchKernelGGL(k_target_sync<_Float16>, grid, dim3(256), 0, as_stream(stream), params,
                           target, reinterpret_cast<_Float16 *>(target_h), P, Ph, n);
    DMDQN_LAUNCH_CHECK("k_target_sync");
    return DMDQN_OK;
}

static int check_soft_update(const char *who, const float *params, const float *target,
                             const uint16_t *target_h, int NW, int P, int Ph, int precision) {
    DMDQN_REQUIRE(params && target && NW > 0 && P > 0 && Ph >= P, "%s: NW=%d P=%d Ph=%d", who, NW,
                  P, Ph);
    DMDQN_REQUIRE(precision >= 0 && precision <= 2, "%s: precision %d", who, precision);
    DMDQN_REQUIRE(!target_h || precision != 0, "%s: fp32 has no 16-bit shadow", who);
    DMDQN_REQUIRE(P % 4 == 0 && (!target_h || Ph % 4 == 0),
                  "%s: P=%d and Ph=%d must be multiples of 4", who, P, Ph);
    DMDQN_REQUIRE(((uintptr_t)params | (uintptr_t)target) % 16 == 0 && (uintptr_t)target_h % 8 == 0,
                  "%s: params / target must be 16-byte aligned, target_h 8", who);
    return DMDQN_OK;
}

extern "C" int dmdqn_target_soft_update(const float *params, float *target, uint16_t *target_h,
                                        int NW, int P, int Ph, int precision, float tau,
                                        float one_minus_tau, void *stream) {
    if (int rc = check_soft_update("dmdqn_target_soft_update", params, target, target_h, NW, P, Ph,
                                   precision))
        return rc;
    if (int rc = check_tau("dmdqn_target_soft_update", tau, one_minus_tau, false)) return rc;
    return launch_target_soft(params, target, target_h, NW, P, Ph, precision, tau, one_minus_tau,
                              nullptr, nullptr, as_stream(stream));
}

extern "C" int dmdqn_target_soft_update_hp(const float *params, float *target, uint16_t *target_h,
                                           int NW, int P, int Ph, int precision, const float *tau,
                                           const float *one_minus_tau, void *stream) {
    if (int rc = check_soft_update("dmdqn_target_soft_update_hp", params, target, target_h, NW, P,
                                   Ph, precision))
        return rc;
    DMDQN_REQUIRE(tau && one_minus_tau,
                  "dmdqn_target_soft_update_hp: tau and one_minus_tau arrays required");
    return launch_target_soft(params, target, target_h, NW, P, Ph, precision, 0.0f, 0.0f, tau,
                              one_minus_tau, as_stream(stream));
}
