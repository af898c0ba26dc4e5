// health.hip -- the network health probe (include/dmdqn.h has the rules):
// dmdqn_net_probe, the online forward of every agent's batch reduced to counts
// of active and dead ReLU units, non-finite pre-activations, activation sums
// and pre-activation maxima; and dmdqn_layer_norms, the per-variable sums of
// squares of a per-net f32 array (weights, gradient, or the Adam step m /
// (sqrt(v) + eps)).  Both only read the training state.
//
// The probe's forward is the 16-bit learn's (learn_h16.hpp forward_x, relu_h4)
// with the learn's ownership: one 512-thread workgroup per agent, wave w owns
// neurons 16w .. 16w + 15 of each layer, weight fragments straight from HBM
// with the cast, the X image [128][96] and one H image [128][128] (H1, then H2
// over it) in LDS in learn_img.hpp's hoff layout -- 56 KB + the reduction
// cells, two workgroups per CU.  (learn_h16.hpp itself instantiates the learn
// kernels, so its small fragment helpers are restated here.)
//   forward  Z^T[n][b] = W^T[n][k] . X[b][k]: lane (lg, lr) of wave w holds
//   neurons 16w + 4lg + e (e = 0..3) of batch row 16t + lr for the 8 row tiles
//   t, so the 128 values of one unit sit in the 16 lanes of one lane group:
//   dead = an in-lane OR over t and a 16-lane butterfly.
// Built with the default -ffp-contract=off.
#include <math.h>

#include "common.hpp"
#include "learn_img.hpp"
#include "qnet_layout.hpp"

namespace dmdqn {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
template <typename T> using vec8 = T __attribute__((ext_vector_type(8)));
template <typename T> using vec4 = T __attribute__((ext_vector_type(4)));

constexpr int PB = 128, PH = 128, PDP = QN_DP, PNACT = QN_NA;
using L = QL<PH>;
constexpr int PROBE_NT = 512, PROBE_NWV = PROBE_NT / 64;

// LDS byte offsets of the probe
constexpr int PX_OFF = 0;                          // X  h16 [128][96]
constexpr int PH_OFF = PX_OFF + PB * PDP * 2;      // H1 / H2 h16 [128][128]
constexpr int PSLOT_OFF = PH_OFF + PB * PH * 2;    // int [128] ring slots
constexpr int PSUM_OFF = PSLOT_OFF + PB * 4;       // double [2][8] sums of h1, h2 per wave
constexpr int PMAX_OFF = PSUM_OFF + 2 * PROBE_NWV * 8;   // float [3][8] maxima per wave
constexpr int PCNT_OFF = PMAX_OFF + 3 * PROBE_NWV * 4;   // int [3][8]: active 1, active 2, non-finite
constexpr int PDEAD_OFF = PCNT_OFF + 3 * PROBE_NWV * 4;  // uint32 [2][8]: the wave's 16 dead bits
constexpr int PROBE_LDS = PDEAD_OFF + 2 * PROBE_NWV * 4;
static_assert(PROBE_LDS <= 81920, "two workgroups per CU");

__device__ __forceinline__ f32x4 mfma16(vec8<_Float16> a, vec8<_Float16> b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ f32x4 mfma16(vec8<__bf16> a, vec8<__bf16> b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

// img[r0 + (l&15)][k0 + 8(l>>4) + e] of a blocked image (hoff): one 16-byte read.
template <typename h16, int LD>
__device__ __forceinline__ vec8<h16> frag_rows(const h16 *img, int r0, int k0) {
    const int l = threadIdx.x & 63;
    return *reinterpret_cast<const vec8<h16> *>(img + hoff<LD>(r0 + (l & 15), k0 + 8 * (l >> 4)));
}

template <typename h16>
__device__ __forceinline__ vec8<h16> cast8(const float4 &x, const float4 &y) {
    vec8<h16> r;
    r[0] = (h16)x.x; r[1] = (h16)x.y; r[2] = (h16)x.z; r[3] = (h16)x.w;
    r[4] = (h16)y.x; r[5] = (h16)y.y; r[6] = (h16)y.z; r[7] = (h16)y.w;
    return r;
}

// A-fragment of the tiled W2T (qn_wt): W2T[n0 + (l&15)][k0 + 8(l>>4) + e] -> h16.
template <typename h16>
__device__ __forceinline__ vec8<h16> w2_frag(const float *W2T, int n0, int k0) {
    const int l = threadIdx.x & 63;
    const float4 *p = reinterpret_cast<const float4 *>(W2T + qn_wt(n0 + (l & 15), k0 + 8 * (l >> 4), PH));
    return cast8<h16>(p[0], p[1]);
}

// Layer-1 A-fragment s (features 32s .. 32s + 31) from the W1 block (qn_w1):
// fragment 2's lane group 3 covers features 88..95, of which only 88 exists
// (the W1T column; 89..95 are zero weights, not stored).  Every lane loads a
// valid tile address; the select follows.
template <typename h16>
__device__ __forceinline__ vec8<h16> w1_frag(const float *W1, int n0, int s) {
    const int l = threadIdx.x & 63, lg = l >> 4, n = n0 + (l & 15);
    const bool tile = s < 2 || lg < 3;
    const float4 *p = reinterpret_cast<const float4 *>(W1 + qn_w1<PH>(n, 32 * s + 8 * (tile ? lg : 2)));
    const float4 x = p[0], y = p[1];
    const float c = s == 2 ? W1[qn_w1<PH>(n, QN_DT)] : 0.0f;
    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
    return tile ? cast8<h16>(x, y) : cast8<h16>(make_float4(c, 0.f, 0.f, 0.f), z);
}

// The output layer's A-fragment: rows 0..3 are W3T[a][k0 + 8(l>>4) + e]
// (row-major), rows 4..15 zero.
template <typename h16>
__device__ __forceinline__ vec8<h16> w3_frag(const float *W3T, int k0) {
    const int l = threadIdx.x & 63, lr = l & 15;
    const float4 *p = reinterpret_cast<const float4 *>(W3T + (lr & (PNACT - 1)) * PH + k0 + 8 * (l >> 4));
    const float4 x = p[0], y = p[1];
    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
    return lr < PNACT ? cast8<h16>(x, y) : cast8<h16>(z, z);
}

// What a lane gathers of one hidden layer over its 8 row tiles x 4 neurons.
struct LaneStats {
    double sum;      // of h, in (tile, neuron) order
    float zmax;      // largest finite |z|
    int active;      // entries with h > 0
    int nonfinite;   // entries of z that are inf or NaN
    unsigned alive;  // bit e: neuron e of the lane had h > 0 on some row
};

__device__ __forceinline__ LaneStats lane_stats_zero() { return LaneStats{0.0, 0.0f, 0, 0, 0u}; }

// One pre-activation into the lane's figures; returns whether the unit is on.
__device__ __forceinline__ bool note_z(float z, LaneStats &s) {
    const bool on = z > 0.0f;                 // false for a NaN, as relu_h4's select
    const bool fin = fabsf(z) < INFINITY;     // false for inf and NaN
    s.active += on ? 1 : 0;
    s.nonfinite += fin ? 0 : 1;
    s.zmax = fin ? fmaxf(s.zmax, fabsf(z)) : s.zmax;
    s.sum = __dadd_rn(s.sum, on ? (double)z : 0.0);
    return on;
}

// Dense + relu under the mixed policy on one MFMA output tile: z = h16(h16(acc)
// + b) (the packed 16-bit add of relu_h4), h = z > 0 ? z : 0, with the lane's
// health figures taken of z and h on the way.
template <typename h16>
__device__ __forceinline__ vec4<h16> dense_relu_stats(f32x4 acc, vec4<h16> b, LaneStats &s) {
    const vec4<h16> z = __builtin_convertvector(acc, vec4<h16>) + b;
    vec4<h16> h;
#pragma unroll
    for (int e = 0; e < 4; e++) {
        const bool on = note_z((float)z[e], s);
        s.alive |= (on ? 1u : 0u) << e;
        h[e] = on ? z[e] : (h16)0.0f;
    }
    return h;
}

// The wave's reduction of a hidden layer's lane figures into its LDS cells.
__device__ __forceinline__ void wave_reduce_layer(LaneStats s, int layer, char *smem) {
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63, lg = l >> 4;
    // a unit's 128 values sit in the 16 lanes of its lane group
    unsigned alive = s.alive;
#pragma unroll
    for (int off = 1; off < 16; off <<= 1) alive |= __shfl_xor(alive, off);
    unsigned dead = (~alive & 0xfu) << (4 * lg);  // neurons 16w + 4lg + e
    dead |= __shfl_xor(dead, 16);
    dead |= __shfl_xor(dead, 32);
    for (int off = 32; off > 0; off >>= 1) {
        s.sum = __dadd_rn(s.sum, __shfl_xor(s.sum, off));
        s.zmax = fmaxf(s.zmax, __shfl_xor(s.zmax, off));
        s.active += __shfl_xor(s.active, off);
    }
    if (l == 0) {
        reinterpret_cast<double *>(smem + PSUM_OFF)[layer * PROBE_NWV + w] = s.sum;
        reinterpret_cast<float *>(smem + PMAX_OFF)[layer * PROBE_NWV + w] = s.zmax;
        reinterpret_cast<int *>(smem + PCNT_OFF)[layer * PROBE_NWV + w] = s.active;
        reinterpret_cast<uint32_t *>(smem + PDEAD_OFF)[layer * PROBE_NWV + w] = dead;
    }
}

template <typename h16>
__global__ void __launch_bounds__(PROBE_NT, 4) k_net_probe(dmdqn_probe_args a) {
    __shared__ __attribute__((aligned(16))) char smem[PROBE_LDS];
    h16 *X = (h16 *)(smem + PX_OFF), *Hb = (h16 *)(smem + PH_OFF);
    int *slot = (int *)(smem + PSLOT_OFF);
    const int tid = threadIdx.x, agent = blockIdx.x;
    const int w = tid >> 6, l = tid & 63, lr = l & 15, lg = l >> 4;
    const int n = 16 * w + 4 * lg;
    const float *Wg = a.params + (size_t)agent * L::P;

    // ring slots of the batch: slot = (start + p) mod cap, whatever p holds
    // (an index outside the deque still reads inside the agent's ring)
    {
        const int pos = a.idx[(size_t)agent * PB + (tid & (PB - 1))];
        int s = (int)(((long long)a.start + (long long)pos) % (long long)a.cap);
        if (s < 0) s += a.cap;
        slot[tid & (PB - 1)] = s;  // the 4 lane groups of 128 store the same values
    }
    // this wave's weight fragments, in flight across the gather
    vec8<h16> w1[3], w2[4];
#pragma unroll
    for (int s = 0; s < 3; s++) w1[s] = w1_frag<h16>(Wg + L::oW1T, 16 * w, s);
#pragma unroll
    for (int s = 0; s < 4; s++) w2[s] = w2_frag<h16>(Wg + L::oW2T, 16 * w, 32 * s);
    const vec4<h16> b1 = __builtin_convertvector(*reinterpret_cast<const f32x4 *>(Wg + L::ob1 + n), vec4<h16>);
    const vec4<h16> b2 = __builtin_convertvector(*reinterpret_cast<const f32x4 *>(Wg + L::ob2 + n), vec4<h16>);
    __syncthreads();
    // the S rows (int8, 96 feature bytes of a 128-B line) -> X h16 [128][96]
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const int t = tid + PROBE_NT * i, b = t / 12, q = t - 12 * (t / 12);
        const uint2 v = reinterpret_cast<const uint2 *>(
            a.ring_s + ((size_t)agent * a.cap + slot[b]) * DMDQN_ROW_BYTES)[q];
        vec8<h16> hv;
#pragma unroll
        for (int e = 0; e < 4; e++) {
            hv[e] = (h16)(float)(int8_t)(v.x >> (8 * e));
            hv[e + 4] = (h16)(float)(int8_t)(v.y >> (8 * e));
        }
        *reinterpret_cast<vec8<h16> *>(X + hoff<PDP>(b, 8 * q)) = hv;
    }
    __syncthreads();

    // layer 1: X -> H1
    LaneStats s1 = lane_stats_zero();
#pragma unroll
    for (int t = 0; t < 8; t++) {
        f32x4 c = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < 3; s++) c = mfma16(w1[s], frag_rows<h16, PDP>(X, 16 * t, 32 * s), c);
        *reinterpret_cast<vec4<h16> *>(Hb + hoff<PH>(16 * t + lr, n)) = dense_relu_stats<h16>(c, b1, s1);
    }
    wave_reduce_layer(s1, 0, smem);
    __syncthreads();

    // layer 2: H1 -> H2 over H1 (the 8 output tiles held across a barrier)
    LaneStats s2 = lane_stats_zero();
    {
        f32x4 acc[8];
#pragma unroll
        for (int t = 0; t < 8; t++) {
            f32x4 c = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < 4; s++) c = mfma16(w2[s], frag_rows<h16, PH>(Hb, 16 * t, 32 * s), c);
            acc[t] = c;
        }
        __syncthreads();  // every wave has read H1
#pragma unroll
        for (int t = 0; t < 8; t++)
            *reinterpret_cast<vec4<h16> *>(Hb + hoff<PH>(16 * t + lr, n)) =
                dense_relu_stats<h16>(acc[t], b2, s2);
    }
    wave_reduce_layer(s2, 1, smem);
    __syncthreads();

    // layer 3: Q^T[a][b] of the wave's 16 rows; lane group 0 holds q[16w + lr][0..3]
    {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < 4; s++)
            acc = mfma16(w3_frag<h16>(Wg + L::oW3T, 32 * s), frag_rows<h16, PH>(Hb, 16 * w, 32 * s), acc);
        const f32x4 b3f = *reinterpret_cast<const f32x4 *>(Wg + L::ob3);
        float qmax = 0.0f;
        int nf = s1.nonfinite + s2.nonfinite;
        if (lg == 0) {
#pragma unroll
            for (int e = 0; e < PNACT; e++) {
                // h16(h16(acc) + h16(b3)): the f32 sum of two 16-bit values
                // rounded once is the correctly rounded 16-bit add
                const float q = (float)(h16)((float)(h16)acc[e] + (float)(h16)b3f[e]);
                const bool fin = fabsf(q) < INFINITY;
                nf += fin ? 0 : 1;
                qmax = fin ? fmaxf(qmax, fabsf(q)) : qmax;
            }
        }
        for (int off = 32; off > 0; off >>= 1) {
            qmax = fmaxf(qmax, __shfl_xor(qmax, off));
            nf += __shfl_xor(nf, off);
        }
        if (l == 0) {
            reinterpret_cast<float *>(smem + PMAX_OFF)[2 * PROBE_NWV + w] = qmax;
            reinterpret_cast<int *>(smem + PCNT_OFF)[2 * PROBE_NWV + w] = nf;
        }
    }
    __syncthreads();

    // the waves' cells in wave order
    if (tid == 0) {
        const double *sum = reinterpret_cast<const double *>(smem + PSUM_OFF);
        const float *mx = reinterpret_cast<const float *>(smem + PMAX_OFF);
        const int *cnt = reinterpret_cast<const int *>(smem + PCNT_OFF);
        const uint32_t *dead = reinterpret_cast<const uint32_t *>(smem + PDEAD_OFF);
        int32_t *oc = a.counts + (size_t)agent * DMDQN_PROBE_COUNTS;
        double *os = a.stats + (size_t)agent * DMDQN_PROBE_STATS;
#pragma unroll
        for (int layer = 0; layer < 2; layer++) {
            double S = sum[layer * PROBE_NWV];
            int act = 0, nd = 0;
#pragma unroll
            for (int k = 1; k < PROBE_NWV; k++) S = __dadd_rn(S, sum[layer * PROBE_NWV + k]);
#pragma unroll
            for (int k = 0; k < PROBE_NWV; k++) {
                act += cnt[layer * PROBE_NWV + k];
                nd += __popc(dead[layer * PROBE_NWV + k]);
            }
            oc[2 * layer] = act;
            oc[2 * layer + 1] = nd;
            os[layer] = S;
            if (a.dead_mask) {
#pragma unroll
                for (int j = 0; j < 4; j++)
                    a.dead_mask[((size_t)agent * 2 + layer) * 4 + j] =
                        dead[layer * PROBE_NWV + 2 * j] | (dead[layer * PROBE_NWV + 2 * j + 1] << 16);
            }
        }
        int nf = 0;
#pragma unroll
        for (int k = 0; k < PROBE_NWV; k++) nf += cnt[2 * PROBE_NWV + k];
        oc[4] = nf;
#pragma unroll
        for (int j = 0; j < 3; j++) {
            float m = mx[j * PROBE_NWV];
#pragma unroll
            for (int k = 1; k < PROBE_NWV; k++) m = fmaxf(m, mx[j * PROBE_NWV + k]);
            os[2 + j] = (double)m;
        }
    }
}

// ---------------------------------------------------------------------------
// dmdqn_layer_norms: one workgroup per net, NORM_NT threads; thread t holds the
// float4 groups t, t + NORM_NT, ... (every segment starts on a multiple of 4
// floats, so a group lies in one segment).
constexpr int NORM_NT = 1024;
constexpr int NORM_NWV = NORM_NT / 64;
constexpr int NORM_G = (QL<128>::P / 4 + NORM_NT - 1) / NORM_NT;  // groups per thread (7)
constexpr int NORM_SEG = 6;

// Segment ends in the device layout, in Keras variable order.
struct NormSegs {
    int w1_end, w2_end, w3_end, b1_end, b2_end;  // W1 | W2 | W3 | b1 | b2 | b3 up to P
};

template <int MODE>
__global__ void __launch_bounds__(NORM_NT) k_layer_norms(const float *__restrict__ x,
                                                        const float *__restrict__ y, float eps,
                                                        int P, NormSegs sg,
                                                        double *__restrict__ out) {
    __shared__ double red[NORM_SEG][NORM_NWV];
    const int tid = threadIdx.x, net = blockIdx.x, P4 = P / 4;
    const size_t base = (size_t)net * P;
    // every load in flight before the first use
    float4 xv[NORM_G], yv[NORM_G];
#pragma unroll
    for (int k = 0; k < NORM_G; k++) {
        const int q = k * NORM_NT + tid;
        xv[k] = q < P4 ? *reinterpret_cast<const float4 *>(x + base + 4 * (size_t)q)
                       : make_float4(0.f, 0.f, 0.f, 0.f);
        if (MODE == 1)
            yv[k] = q < P4 ? *reinterpret_cast<const float4 *>(y + base + 4 * (size_t)q)
                           : make_float4(1.f, 1.f, 1.f, 1.f);
    }
    double acc[NORM_SEG];
#pragma unroll
    for (int s = 0; s < NORM_SEG; s++) acc[s] = 0.0;
#pragma unroll
    for (int k = 0; k < NORM_G; k++) {
        const int i = 4 * (k * NORM_NT + tid);
        // Keras order W1, b1, W2, b2, W3, b3 of the layout's W1 | W2 | W3 | b1 | b2 | b3
        const int seg = i < sg.w1_end ? 0 : i < sg.w2_end ? 2 : i < sg.w3_end ? 4
                        : i < sg.b1_end ? 1 : i < sg.b2_end ? 3 : 5;
        const float *px = &xv[k].x, *py = &yv[k].x;
        double part = 0.0;  // the group's 4 squares in index order
#pragma unroll
        for (int e = 0; e < 4; e++) {
            float u = px[e];
            if (MODE == 1) u = __fdiv_rn(u, __fadd_rn(__fsqrt_rn(py[e]), eps));
            part = __dadd_rn(part, __dmul_rn((double)u, (double)u));
        }
        if (i >= P) part = 0.0;
#pragma unroll
        for (int s = 0; s < NORM_SEG; s++) acc[s] = __dadd_rn(acc[s], seg == s ? part : 0.0);
    }
#pragma unroll
    for (int s = 0; s < NORM_SEG; s++) {
        double v = acc[s];
        for (int off = 32; off > 0; off >>= 1) v = __dadd_rn(v, __shfl_xor(v, off));
        if ((tid & 63) == 0) red[s][tid >> 6] = v;
    }
    __syncthreads();
    if (tid < NORM_SEG) {
        double S = red[tid][0];
#pragma unroll
        for (int k = 1; k < NORM_NWV; k++) S = __dadd_rn(S, red[tid][k]);
        out[(size_t)net * NORM_SEG + tid] = S;
    }
}

}  // namespace
}  // namespace dmdqn

using namespace dmdqn;

extern "C" int dmdqn_net_probe(const dmdqn_probe_args *a, void *stream) {
    const char *who = "dmdqn_net_probe";
    DMDQN_REQUIRE(a && a->ring_s && a->idx && a->params && a->counts && a->stats,
                  "%s: null argument", who);
    DMDQN_REQUIRE(a->NA > 0 && a->cap > 0, "%s: NA=%d cap=%d must be > 0", who, a->NA, a->cap);
    DMDQN_REQUIRE(a->batch == PB, "%s: batch=%d != %d", who, a->batch, PB);
    DMDQN_REQUIRE(a->hidden == PH, "%s: hidden=%d != %d", who, a->hidden, PH);
    DMDQN_REQUIRE(a->P == L::P, "%s: P=%d != %d (the 128-wide layout)", who, a->P, L::P);
    DMDQN_REQUIRE(a->precision == 1 || a->precision == 2, "%s: precision %d (fp16 / bf16 only)",
                  who, a->precision);
    DMDQN_REQUIRE(a->start >= 0 && a->start < a->cap, "%s: start=%d outside [0, cap=%d)", who,
                  a->start, a->cap);
    if (a->precision == 1)
        hipLaunchKernelGGL(k_net_probe<_Float16>, dim3(a->NA), dim3(PROBE_NT), 0, as_stream(stream), *a);
    else
        hipLaunchKernelGGL(k_net_probe<__bf16>, dim3(a->NA), dim3(PROBE_NT), 0, as_stream(stream), *a);
    DMDQN_LAUNCH_CHECK("k_net_probe");
    return DMDQN_OK;
}

extern "C" int dmdqn_layer_norms(const float *x, const float *y, float eps, int mode, int NW, int P,
                                 int hidden, double *out, void *stream) {
    const char *who = "dmdqn_layer_norms";
    DMDQN_REQUIRE(x && out, "%s: null argument", who);
    DMDQN_REQUIRE(mode == 0 || mode == 1, "%s: mode=%d must be 0 or 1", who, mode);
    DMDQN_REQUIRE(mode == 0 || y, "%s: mode 1 needs y (Adam v): null argument", who);
    DMDQN_REQUIRE(NW > 0, "%s: NW=%d must be > 0", who, NW);
    DMDQN_REQUIRE(hidden == 64 || hidden == 128, "%s: hidden=%d must be 64 or 128", who, hidden);
    const int want = hidden == 64 ? QL<64>::P : QL<128>::P;
    DMDQN_REQUIRE(P == want, "%s: P=%d != %d (the %d-wide layout)", who, P, want, hidden);
    NormSegs sg;
    if (hidden == 64)
        sg = NormSegs{QL<64>::oW2T, QL<64>::oW3T, QL<64>::ob1, QL<64>::ob2, QL<64>::ob3};
    else
        sg = NormSegs{QL<128>::oW2T, QL<128>::oW3T, QL<128>::ob1, QL<128>::ob2, QL<128>::ob3};
    if (mode == 0)
        hipLaunchKernelGGL(k_layer_norms<0>, dim3(NW), dim3(NORM_NT), 0, as_stream(stream), x, y, eps,
                           P, sg, out);
    else
        hipLaunchKernelGGL(k_layer_norms<1>, dim3(NW), dim3(NORM_NT), 0, as_stream(stream), x, y, eps,
                           P, sg, out);
    DMDQN_LAUNCH_CHECK("k_layer_norms");
    return DMDQN_OK;
}
