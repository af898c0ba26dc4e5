// learn_rules.hpp -- the arithmetic rules that make every learn kernel
// bit-exact against the reference, each defined once: Keras-3 Adam, the target
// write-out with its 16-bit shadow, the numpy-pairwise reward z-score, the
// first-max Double-DQN target, the per-row loss and its reduction, and the
// per-row LDS scratch they work in.  Included by learn.hip (f32), learn_h16.hpp
// (f16 / bf16) and learn_shared.hip (C5); a kernel that keeps a local form of a
// rule for its generated code says so beside it and names the rule here.
// Statement and declaration order in these functions is deliberate: the hot
// kernels' generated code is compared with the previous revision's when they
// change, and the compiler breaks scheduling and register ties by it.
#pragma once
#include "common.hpp"
#include "qnet_layout.hpp"

namespace dmdqn {

constexpr int LEARN_B = 128;  // batch rows (dqn_agent.py: batch_size 128)

// ---------------------------------------------------------------- Keras-3 Adam
// Keras-3 Adam (keras/src/optimizers/adam.py update_step) on one parameter,
// every op rounded on its own as TF's separate elementwise kernels do: no fma
// contraction (mul_rn: the learn files are built with -ffp-contract=fast for
// the MFMA epilogues, which ignores the contract pragma), correctly rounded
// sqrt and divide (HIP's default).
__device__ __forceinline__ void keras_adam_el(float &w, float &m, float &v, float g, float alpha,
                                              float c1, float c2, float eps) {
    m = m + mul_rn(g - m, c1);
    v = v + mul_rn(mul_rn(g, g) - v, c2);
    w = w - (m * alpha) / (sqrtf(v) + eps);
}

// ---------------------------------------------------------------- target write-out
// What follows Adam on a lane's 4 consecutive parameters when the learn also
// updates the target network.  T points at the 4 f32 values; their 16-bit
// shadow (the RNE cast of the new f32 target, type T16) is TH[th..th+3], or
// absent when TH is null.
template <typename T16>
__device__ __forceinline__ void shadow4(T16 *TH, size_t th, const float4 &x) {
    typedef T16 t16x4 __attribute__((ext_vector_type(4)));
    t16x4 hv;
    hv[0] = (T16)x.x; hv[1] = (T16)x.y;
    hv[2] = (T16)x.z; hv[3] = (T16)x.w;
    *reinterpret_cast<t16x4 *>(TH + th) = hv;
}

// The hard copy target <- online (dqn_agent.py:376-387).
template <typename T16>
__device__ __forceinline__ void target_hard4(float *T, T16 *TH, size_t th, const float4 &w) {
    *reinterpret_cast<float4 *>(T) = w;
    if (TH) shadow4(TH, th, w);
}

// The soft update target <- soft_el(online, target) (update_target_network_soft,
// dqn_agent.py:389-399); t: the old target.
__device__ __forceinline__ float4 soft_el4(const float4 &w, float4 t, float tau, float omt) {
    t.x = soft_el(w.x, t.x, tau, omt);
    t.y = soft_el(w.y, t.y, tau, omt);
    t.z = soft_el(w.z, t.z, tau, omt);
    t.w = soft_el(w.w, t.w, tau, omt);
    return t;
}

template <typename T16>
__device__ __forceinline__ void target_soft4(float *T, T16 *TH, size_t th, const float4 &w,
                                             const float4 &t, float tau, float omt) {
    const float4 tn = soft_el4(w, t, tau, omt);
    *reinterpret_cast<float4 *>(T) = tn;
    if (TH) shadow4(TH, th, tn);
}

// ---------------------------------------------------------------- per-row scratch
// The per-row LDS scratch of a one-workgroup-per-agent learn kernel (6240 B).
struct Scratch {
    float *z3;  // [128][4]  target Q(S') then online Q(S)
    float *rn;  // [128] z-scored reward
    float *y;   // [128] TD target
    float *dq;  // [128] dL/dq
    float *dn;  // [128] done
    int *act, *slot;  // [128]
    double *r64;  // [128] rewards
    double *red;  // [12] reduction cells
};
constexpr int SCRATCH_BYTES = 6144 + 12 * 8;

__device__ __forceinline__ Scratch scratch_at(char *sc) {
    return Scratch{(float *)sc,          (float *)(sc + 2048), (float *)(sc + 2560),
                   (float *)(sc + 3072), (float *)(sc + 3584), (int *)(sc + 4096),
                   (int *)(sc + 4608),   (double *)(sc + 5120), (double *)(sc + 6144)};
}

// ---------------------------------------------------------------- reward z-score
// The reward z-score of ReplayBuffer.sample (dqn_agent.py:64-69): f64 mean and
// population std over the 128 rewards in numpy's pairwise order -- 8 partial
// sums of 16 (lane k: rewards k, k + 8, ...), combined by an 8-way tree -- and
// + 1e-8 on the std.
__device__ __forceinline__ double pairwise8(const double *r) {
    return __dadd_rn(__dadd_rn(__dadd_rn(r[0], r[1]), __dadd_rn(r[2], r[3])),
                     __dadd_rn(__dadd_rn(r[4], r[5]), __dadd_rn(r[6], r[7])));
}

// (rk = rewards + k: partial k of the 8)
__device__ __forceinline__ double zs_part_sum(const double *rk) {
    double acc = rk[0];
    for (int i = 1; i < 16; i++) acc = __dadd_rn(acc, rk[8 * i]);
    return acc;
}

__device__ __forceinline__ double zs_part_sqdev(const double *rk, double mean) {
    double acc = 0.0;
    for (int i = 0; i < 16; i++) {
        double d = __dsub_rn(rk[8 * i], mean);
        double sq = __dmul_rn(d, d);
        acc = i == 0 ? sq : __dadd_rn(acc, sq);
    }
    return acc;
}

// mean and std + 1e-8 from the 8 partials; a reward r then scales to
// (float)((r - mean) / std), both ops correctly rounded in f64.
__device__ __forceinline__ double zs_mean(const double *part) {
    return __ddiv_rn(__dadd_rn(0.0, pairwise8(part)), 128.0);
}
__device__ __forceinline__ double zs_std(const double *part) {
    return __dadd_rn(__dsqrt_rn(__ddiv_rn(__dadd_rn(0.0, pairwise8(part)), 128.0)), 1e-8);
}

// Workgroup level, over S.r64 -> S.rn.  Starts with a barrier (S.r64 complete).
__device__ __forceinline__ void zscore(const Scratch &S) {
    const int tid = threadIdx.x;
    __syncthreads();
    if (tid < 8) S.red[tid] = zs_part_sum(S.r64 + tid);
    __syncthreads();
    if (tid == 0) S.red[8] = zs_mean(S.red);
    __syncthreads();
    if (tid < 8) {
        const double mean = S.red[8];
        S.red[tid] = zs_part_sqdev(S.r64 + tid, mean);
    }
    __syncthreads();
    if (tid == 0) S.red[9] = zs_std(S.red);
    __syncthreads();
    if (tid < LEARN_B) S.rn[tid] = (float)__ddiv_rn(__dsub_rn(S.r64[tid], S.red[8]), S.red[9]);
}

// ---------------------------------------------------------------- Double-DQN target
// argmax over the 4 online Q(S') values as tf.argmax: the first max on ties.
__device__ __forceinline__ int first_max4(float q0, float q1, float q2, float q3) {
    float bq = q0;
    int best = 0;
    if (q1 > bq) { best = 1; bq = q1; }
    if (q2 > bq) { best = 2; bq = q2; }
    if (q3 > bq) { best = 3; }
    return best;
}

// y = r^ + (gamma (1 - d)) q_t (dqn_agent.py:342-347), each op rounded as TF's
// (mul_rn: no fma): the discount gd = gamma (1 - d), then the target.
__device__ __forceinline__ float td_discount(float gamma, float dn) { return gamma * (1.0f - dn); }
__device__ __forceinline__ float td_target(float rn, float gd, float tq) {
    return rn + mul_rn(gd, tq);
}

// Workgroup level: qo = online Q(S') [128][4], S.z3 = target Q(S') -> S.y.
// Ends with a barrier.
__device__ __forceinline__ void ddqn_target(const dmdqn_learn_args &a, const float *qo,
                                            const Scratch &S) {
    const int tid = threadIdx.x;
    if (tid < LEARN_B) {
        const float4 q = *reinterpret_cast<const float4 *>(qo + tid * QN_NA);
        const int best = first_max4(q.x, q.y, q.z, q.w);
        const float tq = S.z3[tid * QN_NA + best];
        const float gd = td_discount(a.gamma, S.dn[tid]);
        S.y[tid] = td_target(S.rn[tid], gd, tq);
    }
    __syncthreads();
}

// ---------------------------------------------------------------- loss
// Per-row loss term and dL/dq for a batch of B rows, diff = q - y:
//   DMDQN_LOSS_MSE    (dqn_agent.py:352, MeanSquaredError): diff^2, 2 diff / B
//   DMDQN_LOSS_HUBER  (src/experimental/agent.py:99, keras Huber, delta 1):
//                     |d| <= 1 ? d^2 / 2 : |d| - 1/2,  clip(d, -1, 1) / B
// The loss is the mean of the terms.  kind is uniform over the block, so the
// select costs two VALU ops per row.
__device__ __forceinline__ void loss_term(int kind, float diff, float inv_b, float &term,
                                          float &dq) {
    if (kind == DMDQN_LOSS_HUBER) {
        const float ae = fabsf(diff);
        term = ae <= 1.0f ? mul_rn(0.5f * diff, diff) : ae - 0.5f;
        dq = (ae <= 1.0f ? diff : copysignf(1.0f, diff)) * inv_b;
    } else {
        term = mul_rn(diff, diff);
        dq = 2.0f * diff * inv_b;
    }
}

// Workgroup level: the loss (dqn_agent.py:350-352) of Q_online(S) in S.z3 at
// the taken actions against S.y, its mean written to a.loss[agent]; row_dq(row,
// dq) receives each row's dL/dq (rows 0..127 are waves 0 and 1).  Ends with a
// barrier.
template <typename RowDq>
__device__ __forceinline__ void loss_rows(const dmdqn_learn_args &a, int agent, const Scratch &S,
                                          RowDq row_dq) {
    const int tid = threadIdx.x, w = tid >> 6, l = tid & 63;
    float lsum = 0.0f;
    if (tid < LEARN_B) {
        float q = S.z3[tid * QN_NA + S.act[tid]];
        float dq;
        loss_term(a.loss_kind, q - S.y[tid], 1.0f / (float)LEARN_B, lsum, dq);
        row_dq(tid, dq);
    }
    if (w < 2) {
        for (int off = 32; off > 0; off >>= 1) lsum += __shfl_xor(lsum, off);
        if (l == 0) S.red[10 + w] = (double)lsum;
    }
    __syncthreads();
    if (tid == 0 && a.loss) a.loss[agent] = (float)(S.red[10] + S.red[11]) / (float)LEARN_B;
}

}  // namespace dmdqn
