// redo.hip -- dead-unit recycling, ReDo with tau = 0 on the health probe's
// dead_mask (dmdqn_redo; include/dmdqn.h has the rule): a hidden unit that was
// dead on `patience` probes in a row gets fresh incoming weights (HeUniform
// from a stateless counter hash), zero outgoing weights and zero Adam moments.
//
// One 256-thread workgroup per agent.
//   phase A  thread t owns (layer t >> 7, unit t & 127): its streak byte and
//            whether the unit fires.  The 256 streak bytes move as 16 uint4 per
//            agent (a 16-lane group shares one load and assembles one store
//            with shuffles); the 2 x 4 fired words come from wave ballots into
//            LDS.  An agent that fired nothing ends here.
//   phase B  the workgroup walks the agent's P / 4 float4 chunks of the device
//            layout (qnet_layout.hpp) and decides each from the fired words
//            alone, before any load: which of its 4 floats change (`cm`) and to
//            what.  cm == 0: neither read nor written.  cm == 15: stored without
//            a load.  Otherwise one 16-B read-modify-write of params, adam_m and
//            adam_v each.  No atomics; LDS holds the 8 fired words only.
// Built with the default -ffp-contract=off.
#include "common.hpp"
#include "qnet_layout.hpp"

namespace dmdqn {
namespace {

constexpr int RH = 128;
using L = QL<RH>;
constexpr int REDO_NT = 256;
static_assert(REDO_NT == 2 * RH, "one thread per (layer, unit)");

__device__ __forceinline__ uint64_t mix64(uint64_t x) {
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x;
}
constexpr uint64_t REDO_G = 0x9E3779B97F4A7C15ull;

// The fresh weight `in` of unit `unit` of `layer` of global agent `agent`.
__device__ __forceinline__ float redo_draw(uint64_t k, uint64_t agent, int layer, int unit, int in,
                                           float lim) {
    const uint64_t c = ((agent * 2 + (uint64_t)layer) * 128 + (uint64_t)unit) * 128 + (uint64_t)in;
    const uint32_t u24 = (uint32_t)(mix64(k + REDO_G * (c + 1)) >> 40);
    const float t = __fmul_rn((float)((int)(2u * u24 + 1u) - (1 << 24)), 0x1p-24f);
    return __fmul_rn(lim, t);
}

// Bits u .. u + 3 (u a multiple of 4) of a layer's 4 fired words.
__device__ __forceinline__ unsigned fired4(const uint32_t *R, int u) {
    return (R[u >> 5] >> (u & 31)) & 0xfu;
}

__global__ void __launch_bounds__(REDO_NT) k_redo(dmdqn_redo_args a) {
    __shared__ __attribute__((aligned(16))) uint32_t R[2][4];
    const int tid = threadIdx.x, agent = blockIdx.x;
    const int l = tid & 63, w = tid >> 6;
    const int layer = tid >> 7, unit = tid & (RH - 1);

    // ---- phase A: streaks and the fired words
    const uint4 dv = reinterpret_cast<const uint4 *>(a.dead_mask)[(size_t)agent * 2 + layer];
    const uint32_t dw = (unit & 64) ? ((unit & 32) ? dv.w : dv.z) : ((unit & 32) ? dv.y : dv.x);
    const bool dead = (dw >> (unit & 31)) & 1u;
    uint4 *sp = reinterpret_cast<uint4 *>(a.streak + (size_t)agent * (2 * RH)) + (tid >> 4);
    const uint4 sv = *sp;  // the 16 streak bytes of this 16-lane group
    const uint32_t sw = (l & 8) ? ((l & 4) ? sv.w : sv.z) : ((l & 4) ? sv.y : sv.x);
    unsigned s = (sw >> (8 * (l & 3))) & 0xffu;
    s = dead ? (s < 255u ? s + 1u : 255u) : 0u;
    const bool fire = s >= (unsigned)a.patience;
    if (fire) s = 0u;
    // the group's 16 new bytes back into one uint4: 4 lanes -> a word, 4 words
    uint32_t nw = s << (8 * (l & 3));
    nw |= __shfl_xor(nw, 1);
    nw |= __shfl_xor(nw, 2);
    const int g0 = l & ~15;
    uint4 ns;
    ns.x = __shfl(nw, g0);
    ns.y = __shfl(nw, g0 + 4);
    ns.z = __shfl(nw, g0 + 8);
    ns.w = __shfl(nw, g0 + 12);
    if ((l & 15) == 0) *sp = ns;
    const unsigned long long fb = __ballot(fire);  // units 64 (w & 1) .. + 63 of layer w >> 1
    if (l == 0) {
        R[w >> 1][2 * (w & 1)] = (uint32_t)fb;
        R[w >> 1][2 * (w & 1) + 1] = (uint32_t)(fb >> 32);
    }
    __syncthreads();
    const uint4 r1 = *reinterpret_cast<const uint4 *>(R[0]);
    const uint4 r2 = *reinterpret_cast<const uint4 *>(R[1]);
    if (tid == 0) {
        uint4 *rec = reinterpret_cast<uint4 *>(a.recycled + (size_t)agent * 8);
        rec[0] = r1;
        rec[1] = r2;
        int2 n;
        n.x = __popc(r1.x) + __popc(r1.y) + __popc(r1.z) + __popc(r1.w);
        n.y = __popc(r2.x) + __popc(r2.y) + __popc(r2.z) + __popc(r2.w);
        *reinterpret_cast<int2 *>(a.n_recycled + (size_t)agent * 2) = n;
    }
    if ((r1.x | r1.y | r1.z | r1.w | r2.x | r2.y | r2.z | r2.w) == 0u) return;  // uniform

    // ---- phase B: the agent's chunks
    const uint64_t k = mix64(a.seed + REDO_G * ((uint64_t)a.round + 1));
    const uint64_t ga = (uint64_t)a.agent0 + (uint64_t)agent;
    const size_t base = (size_t)agent * L::P;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int q = tid; q < L::P / 4; q += REDO_NT) {
        const int o = 4 * q;
        unsigned cm = 0u;  // bit e: float e of the chunk changes
        float nv[4] = {0.f, 0.f, 0.f, 0.f};
        if (o < L::oW1X) {
            // tiled W1: one neuron x 4 consecutive features
            const QnOutIn p = qn_w1_inv<RH>(o);
            if ((R[0][p.out >> 5] >> (p.out & 31)) & 1u) {
                cm = 15u;
#pragma unroll
                for (int e = 0; e < 4; e++) nv[e] = redo_draw(k, ga, 0, p.out, p.in + e, a.lim1);
            }
        } else if (o < L::oW2T) {
            // the feature-88 column: 4 consecutive neurons
            const int u = o - L::oW1X;
            cm = fired4(R[0], u);
#pragma unroll
            for (int e = 0; e < 4; e++)
                if ((cm >> e) & 1u) nv[e] = redo_draw(k, ga, 0, u + e, QN_DT, a.lim1);
        } else if (o < L::oW3T) {
            // tiled W2T: one layer-2 unit x 4 consecutive layer-1 units
            const QnOutIn p = qn_wt_inv(o - L::oW2T, RH);
            const unsigned z = fired4(R[0], p.in);  // outgoing weights of fired layer-1 units
            if ((R[1][p.out >> 5] >> (p.out & 31)) & 1u) {
                cm = 15u;
#pragma unroll
                for (int e = 0; e < 4; e++)
                    if (!((z >> e) & 1u)) nv[e] = redo_draw(k, ga, 1, p.out, p.in + e, a.lim2);
            } else {
                cm = z;
            }
        } else if (o < L::ob1) {
            cm = fired4(R[1], (o - L::oW3T) & (RH - 1));  // W3T[a][k .. k + 3]
        } else if (o < L::ob2) {
            cm = fired4(R[0], o - L::ob1);
        } else if (o < L::ob3) {
            cm = fired4(R[1], o - L::ob2);
        }  // b3: never touched
        if (cm == 0u) continue;
        float4 *pw = reinterpret_cast<float4 *>(a.params + base + o);
        float4 *pm = reinterpret_cast<float4 *>(a.adam_m + base + o);
        float4 *pv = reinterpret_cast<float4 *>(a.adam_v + base + o);
        if (cm == 15u) {
            *pw = make_float4(nv[0], nv[1], nv[2], nv[3]);
            *pm = zero4;
            *pv = zero4;
        } else {
            float4 x = *pw, m = *pm, v = *pv;
            if (cm & 1u) { x.x = nv[0]; m.x = 0.f; v.x = 0.f; }
            if (cm & 2u) { x.y = nv[1]; m.y = 0.f; v.y = 0.f; }
            if (cm & 4u) { x.z = nv[2]; m.z = 0.f; v.z = 0.f; }
            if (cm & 8u) { x.w = nv[3]; m.w = 0.f; v.w = 0.f; }
            *pw = x;
            *pm = m;
            *pv = v;
        }
    }
}

}  // namespace
}  // namespace dmdqn

using namespace dmdqn;

extern "C" int dmdqn_redo(const dmdqn_redo_args *a, void *stream) {
    const char *who = "dmdqn_redo";
    DMDQN_REQUIRE(a && a->dead_mask && a->streak && a->params && a->adam_m && a->adam_v &&
                      a->recycled && a->n_recycled,
                  "%s: null argument", who);
    DMDQN_REQUIRE(a->NA > 0, "%s: NA=%d must be > 0", who, a->NA);
    DMDQN_REQUIRE(a->hidden == RH, "%s: hidden=%d != %d", who, a->hidden, RH);
    DMDQN_REQUIRE(a->P == L::P, "%s: P=%d != %d (the 128-wide layout)", who, a->P, L::P);
    DMDQN_REQUIRE(a->patience >= 1 && a->patience <= 255, "%s: patience=%d outside 1..255", who,
                  a->patience);
    DMDQN_REQUIRE(a->agent0 >= 0, "%s: agent0=%d must be >= 0", who, a->agent0);
    DMDQN_REQUIRE((((uintptr_t)a->dead_mask | (uintptr_t)a->streak | (uintptr_t)a->params |
                    (uintptr_t)a->adam_m | (uintptr_t)a->adam_v | (uintptr_t)a->recycled) % 16) == 0 &&
                      (uintptr_t)a->n_recycled % 8 == 0,
                  "%s: 16-B alignment of the arrays (n_recycled: 8-B)", who);
    hipLaunchKernelGGL(k_redo, dim3(a->NA), dim3(REDO_NT), 0, as_stream(stream), *a);
    DMDQN_LAUNCH_CHECK("k_redo");
    return DMDQN_OK;
}
