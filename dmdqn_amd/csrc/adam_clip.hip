// adam_clip.hip -- the split learn's Adam launch with global-norm gradient
// clipping (Keras 3 `global_clipnorm`, keras/src/optimizers/base_optimizer.py
// clip_by_global_norm / global_norm; one keyword of the optimizer at the
// reference's dqn_agent.py:140): dmdqn_adam_agents_clip (include/dmdqn.h has
// the rule).  Clipping needs all of an agent's gradient before its first Adam
// step, so one workgroup serves one agent: it loads the agent's gradient from
// grad[NA][P] into registers once, sums the squares in f64, reduces them in a
// fixed order, forms the scale and runs the Adam step of k_adam_agents_*
// (learn_h16.hpp) on the scaled register values.  The arithmetic rules are
// those of learn_rules.hpp / common.hpp (keras_adam_el, target_hard4,
// target_soft4, hp_alpha); built with the default -ffp-contract=off.
#include <float.h>

#include "common.hpp"
#include "learn_rules.hpp"
#include "qnet_layout.hpp"

namespace dmdqn {

int check_tau(const char *who, float tau, float omt, bool zero_ok);  // learn.hip

namespace {

using L = QL<128>;
// what the launch does to the target (learn_h16.hpp TGT_*, which this file
// does not include: that header instantiates the learn kernels)
constexpr int CT_NONE = 0, CT_HARD = 1, CT_SOFT = 2;

constexpr int CLIP_NT = 1024;                      // threads of the agent's workgroup
constexpr int CLIP_NW = CLIP_NT / 64;              // its waves
constexpr int CLIP_P4 = L::P / 4;                  // float4 groups per agent (7137)
constexpr int CLIP_G = (CLIP_P4 + CLIP_NT - 1) / CLIP_NT;  // groups per thread (7; the last partly)

// scale = fl32(fl32(clip * min(fl32(1 / norm), fl32(1 / clip))) + fl32(norm - norm)):
// Keras's clip_by_global_norm, every op rounded on its own, the divides
// correctly rounded (HIP's default).  norm == 0: 1 / norm = inf, the min picks
// 1 / clip.  norm inf or NaN: norm - norm = NaN, so the scale is NaN whatever
// the min returns.
__device__ __forceinline__ float clip_scale(float norm, float clip) {
    const float s_fin = mul_rn(clip, fminf(1.0f / norm, 1.0f / clip));
    return s_fin + (norm - norm);
}

// One workgroup per agent (blockIdx.x), CLIP_NT threads; thread t holds the
// gradient groups t, t + CLIP_NT, ... in registers (a group past the agent's
// last holds zeros).  TM, HP: as k_adam_agents_* (compile-time, so the streams
// carry no branch).  G is read once and never written.
template <typename T16, int TM, bool HP>
// (<= 64 VGPRs, so two workgroups share a CU; the soft update's extra target
// stream does not fit in 64 without scratch and runs one workgroup per CU)
__global__ void __launch_bounds__(CLIP_NT, TM == CT_SOFT ? 4 : 8)
k_adam_agents_clip(float *__restrict__ W, float *__restrict__ M, float *__restrict__ V,
                   float *__restrict__ T, T16 *__restrict__ TH, const float *__restrict__ G,
                   float *__restrict__ gnorm, float clip, float alpha, float c1, float c2,
                   float eps, float tau, float omt, dmdqn_agent_hparams hp) {
    __shared__ double red[CLIP_NW];
    const int tid = threadIdx.x, agent = blockIdx.x;
    if constexpr (HP) {
        if (hp.lr) alpha = hp_alpha(hp, agent);
        if (TM == CT_SOFT && hp.tau) {
            tau = hp.tau[agent];
            omt = hp.one_minus_tau[agent];
        }
    }
    const size_t base = (size_t)agent * L::P;
    // every load in flight before the first use
    float4 g[CLIP_G];
#pragma unroll
    for (int k = 0; k < CLIP_G; k++) {
        const int q = k * CLIP_NT + tid;
        g[k] = q < CLIP_P4 ? *reinterpret_cast<const float4 *>(G + base + 4 * (size_t)q)
                           : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    // S = sum of squares in f64: the thread's values in index order, then the
    // wave's lanes by a butterfly (every lane ends with the same bits), then
    // the waves' sums in wave order -- no atomics, one order on every run
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < CLIP_G; k++) {
        const float *pg = &g[k].x;
#pragma unroll
        for (int e = 0; e < 4; e++) acc = __dadd_rn(acc, __dmul_rn((double)pg[e], (double)pg[e]));
    }
    for (int off = 32; off > 0; off >>= 1) acc = __dadd_rn(acc, __shfl_xor(acc, off));
    if ((tid & 63) == 0) red[tid >> 6] = acc;
    __syncthreads();
    double S = red[0];
#pragma unroll
    for (int w = 1; w < CLIP_NW; w++) S = __dadd_rn(S, red[w]);
    const float norm = (float)__dsqrt_rn(S);  // f64 sqrt, one rounding to f32
    if (gnorm && tid == 0) gnorm[agent] = norm;
    const float scale = uniform_f32(clip_scale(norm, clip));

    const size_t Ph = ((size_t)L::P + 7) / 8 * 8;  // the shadow's agent stride
#pragma unroll
    for (int k = 0; k < CLIP_G; k++) {
        const int q = k * CLIP_NT + tid;
        if (q >= CLIP_P4) continue;
        const size_t i = base + 4 * (size_t)q;
        float4 w = *reinterpret_cast<const float4 *>(W + i);
        float4 m = *reinterpret_cast<const float4 *>(M + i);
        float4 v = *reinterpret_cast<const float4 *>(V + i);
        float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
        if (TM == CT_SOFT) t = *reinterpret_cast<const float4 *>(T + i);
        float *pw = &w.x, *pm = &m.x, *pv = &v.x;
        const float *pg = &g[k].x;
#pragma unroll
        for (int e = 0; e < 4; e++)
            keras_adam_el(pw[e], pm[e], pv[e], mul_rn(pg[e], scale), alpha, c1, c2, eps);
        *reinterpret_cast<float4 *>(W + i) = w;
        *reinterpret_cast<float4 *>(M + i) = m;
        *reinterpret_cast<float4 *>(V + i) = v;
        const size_t ih = (size_t)agent * Ph + 4 * (size_t)q;
        if (TM == CT_HARD) target_hard4(T + i, TH, ih, w);
        if (TM == CT_SOFT) target_soft4(T + i, TH, ih, w, t, tau, omt);
    }
}

template <typename T16>
int launch_adam_clip(const dmdqn_learn_args *a, const dmdqn_agent_hparams &hp, const float *grad,
                     float clip, float *gnorm, hipStream_t s) {
    const int tm = a->sync_target ? CT_HARD : (a->tau > 0.0f || hp.tau) ? CT_SOFT : CT_NONE;
    auto kern = tm == CT_HARD   ? k_adam_agents_clip<T16, CT_HARD, false>
                : tm == CT_SOFT ? k_adam_agents_clip<T16, CT_SOFT, false>
                                : k_adam_agents_clip<T16, CT_NONE, false>;
    if (hp_adam(hp))  // gamma does not reach the optimizer
        kern = tm == CT_HARD   ? k_adam_agents_clip<T16, CT_HARD, true>
               : tm == CT_SOFT ? k_adam_agents_clip<T16, CT_SOFT, true>
                               : k_adam_agents_clip<T16, CT_NONE, true>;
    hipLaunchKernelGGL(kern, dim3(a->NA), dim3(CLIP_NT), 0, s, a->params, a->adam_m, a->adam_v,
                       a->target, reinterpret_cast<T16 *>(a->target_h), grad, gnorm, clip, a->alpha,
                       a->c1, a->c2, a->eps, a->tau, a->one_minus_tau, hp);
    DMDQN_LAUNCH_CHECK("k_adam_agents_clip");
    return DMDQN_OK;
}

}  // namespace
}  // namespace dmdqn

using namespace dmdqn;

extern "C" int dmdqn_adam_agents_clip(const dmdqn_learn_args *a, const dmdqn_agent_hparams *hpp,
                                      const float *grad, float clip, float *gnorm, void *stream) {
    const char *who = "dmdqn_adam_agents_clip";
    // what dmdqn_adam_agents_hp refuses (learn.hip check_hparams, adam_agents_entry)
    dmdqn_agent_hparams hp{};
    if (hpp) {
        DMDQN_REQUIRE((hpp->tau != nullptr) == (hpp->one_minus_tau != nullptr),
                      "%s: tau and one_minus_tau go together (tau=%p one_minus_tau=%p)", who,
                      (const void *)hpp->tau, (const void *)hpp->one_minus_tau);
        DMDQN_REQUIRE(!hpp->lr || (hpp->adam_s > 0.0f && hpp->adam_s <= 1.0f &&
                                   hpp->adam_d > 0.0f && hpp->adam_d <= 1.0f),
                      "%s: with lr, adam_s=%g and adam_d=%g must be in (0, 1]", who,
                      (double)hpp->adam_s, (double)hpp->adam_d);
        hp = *hpp;
    }
    DMDQN_REQUIRE(a && grad && a->NA > 0 && a->params && a->adam_m && a->adam_v && a->target,
                  "%s: null argument", who);
    DMDQN_REQUIRE(a->precision == 1 || a->precision == 2, "%s: precision %d (fp16 / bf16 only)",
                  who, a->precision);
    if (int rc = check_tau(who, a->tau, a->one_minus_tau, true)) return rc;
    // the negated comparison refuses a NaN
    DMDQN_REQUIRE(clip > 0.0f && clip <= FLT_MAX, "%s: clip=%g must be finite and > 0", who,
                  (double)clip);
    DMDQN_REQUIRE(a->P == L::P, "%s: P=%d != %d (the 128-wide layout)", who, a->P, L::P);
    return a->precision == 1
               ? launch_adam_clip<_Float16>(a, hp, grad, clip, gnorm, as_stream(stream))
               : launch_adam_clip<__bf16>(a, hp, grad, clip, gnorm, as_stream(stream));
}
