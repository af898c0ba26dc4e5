// sim_rules.hpp -- the rules of the microsimulation, each defined once: the
// signal advance, a front's route decision, move and outcome, the
// rotating grant, the follower update, the entry position, the origin-queue
// insertion, setPhase and `done`.  sim.hip's three storage forms (LDS image
// and global rings in substep, register lanes in k_sim_step_reg) call them with
// plain values; oracle/oracle_sim.c is the independent restatement they are
// held to, bit for bit, so every function keeps its IEEE operation order.
// Arguments stay scalars (five feeder lanes as five ints, not an array): an
// array reference gave every sim kernel scratch memory.
#pragma once
#include "sim.hpp"

namespace dmdqn {

// ---------------------------------------------------------------- small helpers
__device__ __forceinline__ int last_slot(int head, int cnt, int cap) {
    int s = head + cnt - 1;
    return s >= cap ? s - cap : s;
}

// Sum over the wave (integer: exact in any order); the block totals take one
// LDS atomic per wave instead of one per thread at a single address, which
// the LDS serialises lane by lane (up to 1024-way in the 8x8 register path).
__device__ __forceinline__ int wave_sum(int x) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off);
    return x;
}

__device__ __forceinline__ int wave_max_uniform(int x) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x = max(x, __shfl_xor(x, off));
    return __builtin_amdgcn_readfirstlane(x);
}

// ---------------------------------------------------------------- signals
// Natural phase advance of one junction at time t (fixed durations; in
// actuated mode phase 0 gaps out: after minDur, once no vehicle has been over
// a detector of the phase's green lanes for more than max_gap, or at maxDur).
// ldet12: the junction's 12 detector times (read in actuated mode only).
__device__ __forceinline__ void tl_advance(int32_t &phase, int32_t &ts, int t, bool actuated,
                                           const int32_t *ldet12, const IdmK &P) {
    const int p = phase, el = t - ts;
    bool sw;
    if (actuated && p == 0) {
        constexpr uint32_t gl = green_lanes(0x11BB);  // green_mask(0)
        int last = kNoDetection;
#pragma unroll
        for (int k = 0; k < 12; k++)
            if ((gl >> k) & 1u) last = max(last, ldet12[k]);
        sw = el >= kActMax || (el >= kActMin && (float)(t - last) > P.max_gap);
    } else {
        sw = el >= phase_dur(p);
    }
    if (sw) {
        phase = (p + 1) % 12;
        ts = t;
    }
}

// traci.trafficlight.setPhase on an action: phase stride * act, the timer
// restarts at t0.  A negative action is no setPhase: the junction's program
// runs on with its timer (the reference class's skipped actions).
__device__ __forceinline__ void set_phase(int act, int stride, int t0, int32_t &phase,
                                          int32_t &ts) {
    if (act >= 0) {
        phase = stride * act;
        ts = t0;
    }
}

// getMinExpectedNumber() == 0 or t >= MAX_SIM_TIME
__device__ __forceinline__ bool episode_done(int t, int max_time, int running, int pending) {
    return t >= max_time || (running + pending) == 0;
}

// ---------------------------------------------------------------- pass A: fronts
// A vehicle with route word w on an exit edge or on its last edge drives free.
__device__ __forceinline__ bool on_free_road(const Topo &T, int e, int w) {
    return e >= 4 * T.A || on_final_edge(w, e);
}

// The routing decision of the front of a lane of approach edge e is a function
// of e and the front's route word d0 only (static topology): the movement m at
// the junction ahead, the next edge e2 and the movement mv2 there (< 0: the
// connection keeps the lane index, onto exit / final edges).  One word,
// e2 | m << 12 | (mv2 + 1) << 16, which a thread keeps across substeps beside
// d0 (RouteCache) and recomputes only when its front's route word changes -- a
// front waits at the stop line for many substeps.
__device__ __forceinline__ int route_decide(const Topo &T, int e, int d0) {
    const int aj = e >> 2, h = opp(e & 3);
    const int o = out_dir(T, aj, h, d0);
    const int m = movement(h, o);
    DMDQN_DBG(T.nbr(aj, o) >= 0 || T.exit_id[aj * 4 + o] >= 0, DBG_SIM_EDGE);
    const int e2 = next_edge(T, aj, o);
    const int w2 = route_advance(d0);
    int mv2 = -1;
    if (!on_free_road(T, e2, w2)) {
        const int h2 = opp(e2 & 3);
        mv2 = movement(h2, out_dir(T, e2 >> 2, h2, w2));
    }
    return e2 | (m << 12) | ((mv2 + 1) << 16);
}
struct RouteCache {
    int d0 = -1, pk = 0;  // (route words are >= 0)
};
// The lane a front with decision pk on lane index kf heads for (cnt: the
// lanes' vehicle counts).
__device__ __forceinline__ int route_target(int pk, int kf, const int32_t *cnt) {
    const int e2 = pk & 0xfff, mv2 = (pk >> 16) - 1;
    return e2 * 3 + (mv2 < 0 ? kf : lane_for_move(mv2, e2, cnt));
}
// Whether its movement from approach edge e is green in the junction's phase.
__device__ __forceinline__ bool route_green(int pk, int e, int phase) {
    const int m = (pk >> 12) & 0xf;
    return (green_mask(phase) >> ((e & 3) * 4 + m)) & 1;
}

// The front (x0, v0) of a lane of length len moves: one IDM evaluation, its
// inputs chosen by selects -- free road: no interaction term; green with a
// vehicle (xl, vl) on the target lane tl (lead): that vehicle; green without:
// free; red / yellow: the stop line.  It requests tl when it would cross on
// green, kArrive on a free road, and holds at the stop line otherwise.
struct FrontMove {
    float x, v;
    int req;
};
__device__ __forceinline__ FrontMove front_move(float x0, float v0, float len, bool free_road,
                                                bool green, bool lead, float xl, float vl,
                                                int tl, const IdmK &P) {
    const bool nofront = free_road || (green && !lead);
    const float gap = (len - x0) + (green ? (xl - P.length) : P.min_gap);
    const float acc = idm_sel(v0, gap, v0 - (lead ? vl : 0.0f), nofront, P);
    const float vn = clamp_speed(v0 + acc, P);
    const float xn = x0 + vn;
    const bool over = xn > len;
    const bool stop = !free_road && over && !green;
    return FrontMove{stop ? len : xn, stop ? 0.0f : vn,
                     free_road ? kArrive : (over && green ? tl : -1)};
}

// ---------------------------------------------------------------- pass B: grants
// Bit i: feeder lane f_i requests target lane tl.
__device__ __forceinline__ uint32_t request_mask(const int32_t *req, int tl, int f0, int f1,
                                                 int f2, int f3, int f4) {
    return (req[f0] == tl ? 1u : 0u) | (req[f1] == tl ? 2u : 0u) | (req[f2] == tl ? 4u : 0u) |
           (req[f3] == tl ? 8u : 0u) | (req[f4] == tl ? 16u : 0u);
}
// The first requester (mask != 0) in the feeder order rotated by t % 5.
__device__ __forceinline__ int grant_pick(uint32_t mask, int f0, int f1, int f2, int f3, int f4,
                                          int t) {
    const int start = t % 5;
    const uint32_t rot = ((mask >> start) | (mask << (5 - start))) & 31u;
    int k = start + __ffs(rot) - 1;
    if (k >= 5) k -= 5;
    int fsel = f0;
    fsel = k == 1 ? f1 : fsel;
    fsel = k == 2 ? f2 : fsel;
    fsel = k == 3 ? f3 : fsel;
    return k == 4 ? f4 : fsel;
}
// A lane of n vehicles, the last at last_x (read when n > 0), takes one more
// from a junction.
__device__ __forceinline__ bool has_room(int n, int cap, float last_x, const IdmK &P) {
    bool room = n < cap;
    if (room && n > 0) room = (last_x - P.length) >= P.min_gap;
    return room;
}

// ---------------------------------------------------------------- pass C: advance
// What becomes of a front with request rq and tentative move (fx, fv): on a
// free road it leaves once past the lane's end; a granted request leaves; a
// refused one waits at the stop line.  Returns whether it leaves (pop).
__device__ __forceinline__ bool front_outcome(int rq, bool granted, float len, float &fx,
                                              float &fv) {
    if (rq == kArrive) return fx >= len;
    if (rq < 0) return false;
    if (!granted) {
        fx = len;
        fv = 0.0f;
    }
    return granted;
}

// One follower (xi, vi): IDM against the old leader state, no overlap with the
// leader's new position -- it stops at lim, or stands if lim is behind it
// (selects, not branches: the walks run it for every lane of a wave).
__device__ __forceinline__ float2 follow_rule(float xi, float vi, float lead_x_old,
                                              float lead_v_old, float lead_x_new, const IdmK &P) {
    const float gap = (lead_x_old - P.length) - xi;
    const float acc = idm_acc(vi, gap, vi - lead_v_old, P);
    const float vc = clamp_speed(vi + acc, P);
    const float xc = xi + vc;
    const float lim = lead_x_new - P.length, dl = lim - xi;
    const bool over = xc > lim, back = lim < xi;
    return make_float2(over ? (back ? xi : lim) : xc, over ? (back ? 0.0f : dl) : vc);
}

// Actuated mode: a vehicle's body is over the detector point dp of a lane of
// length len during the substep (old front < dp + length, new front >= dp).
struct Detector {
    float dp, dpl;
    __device__ __forceinline__ Detector(float len, const IdmK &P)
        : dp(len - P.det_dist), dpl(dp + P.length) {}
    __device__ __forceinline__ bool crossed(float x_new, float x_old) const {
        return x_new >= dp && x_old < dpl;
    }
};

// ---------------------------------------------------------------- passes D, E: entries
// Where a vehicle that crossed the junction by `over` enters its target lane:
// behind the lane's last vehicle (last_x, read when has_last), not before 0.
__device__ __forceinline__ float entry_x(float over, bool has_last, float last_x, const IdmK &P) {
    float xe = over;
    if (has_last) {
        const float lim = last_x - P.length - P.min_gap;
        if (lim < xe) xe = lim;
    }
    return xe < 0.0f ? 0.0f : xe;
}

// Vehicle `id` of the demand has departed by time t.
__device__ __forceinline__ bool departed(int id, int period_ms, int t) {
    return (long long)id * period_ms <= (long long)t * 1000;
}
// The lane a vehicle with route word d0 departs on from origin edge e (a
// one-edge route departs on the straight lanes: its origin is its end) ...
__device__ __forceinline__ int insert_lane(const Topo &T, int e, int d0, const int32_t *cnt) {
    const int h = opp(e & 3);
    const int m = on_final_edge(d0, e) ? (int)MV_S : movement(h, out_dir(T, e >> 2, h, d0));
    return e * 3 + lane_for_move(m, e, cnt);
}
// ... if that lane of n vehicles, the last at last_x (read when n > 0), has
// room for it at x = length.
__device__ __forceinline__ bool insert_room(int n, int cap, float last_x, const IdmK &P) {
    bool room = n < cap;
    if (room && n > 0) room = last_x >= 2.0f * P.length + P.min_gap;
    return room;
}

}  // namespace dmdqn
