// dmdqn_torch.cpp -- the C ABI (include/dmdqn.h) registered as PyTorch custom
// operators, torch.ops.dmdqn.* ("Native (TORCH_LIBRARY(dmdqn))").
//
// Every op is a thin, allocation-free adapter: it checks device / dtype /
// contiguity / shape with TORCH_CHECK (a Python RuntimeError), takes the
// current HIP stream of the tensors' device and calls the same extern "C"
// entry point as the ctypes binding.  Ops mutate the arguments their schema
// marks (a!), return nothing, and are registered for the CUDA dispatch key
// (HIP tensors on ROCm) plus a Meta kernel (shape-only, no launch), so the
// dispatcher, torch.compile's fake-tensor tracing and HIP-graph capture see
// them like any other op.  There is no CPU kernel: a CPU tensor raises.
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <torch/library.h>

#include "../../include/dmdqn.h"

using at::Tensor;
using OptT = std::optional<Tensor>;

namespace {

void *stream_of(const Tensor &t) {
    return c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(t.device().index()).stream();
}

void check(int rc, const char *what) {
    TORCH_CHECK(rc == DMDQN_OK, what, " failed (rc=", rc, "): ", dmdqn_last_error());
}

template <typename P>
P *dptr(const Tensor &t, at::ScalarType st, const char *name, int64_t numel = -1) {
    TORCH_CHECK(t.is_cuda(), name, " must be a device tensor");
    TORCH_CHECK(t.scalar_type() == st, name, " must be ", st, ", got ", t.scalar_type());
    TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
    TORCH_CHECK(numel < 0 || t.numel() == numel, name, " has ", t.numel(), " elements, expected ",
                numel);
    return reinterpret_cast<P *>(t.data_ptr());
}

template <typename P>
P *optr(const OptT &t, at::ScalarType st, const char *name, int64_t numel = -1) {
    return t.has_value() ? dptr<P>(*t, st, name, numel) : nullptr;
}

// a 16-bit shadow (f16 or bf16) as raw uint16 storage.  precision (1 = f16,
// 2 = bf16; -1 = either) must match the dtype, so bf16 bits never land in an
// f16 tensor; min_numel > 0 checks the size (NW * Ph, Ph >= P).
uint16_t *h16ptr(const OptT &t, const char *name, int64_t precision = -1, int64_t min_numel = 0) {
    if (!t.has_value()) return nullptr;
    TORCH_CHECK(t->scalar_type() == at::kHalf || t->scalar_type() == at::kBFloat16, name,
                " must be float16 or bfloat16");
    TORCH_CHECK(precision < 0 || (precision == 1 && t->scalar_type() == at::kHalf) ||
                    (precision == 2 && t->scalar_type() == at::kBFloat16),
                name, " dtype ", t->scalar_type(), " does not match precision ", precision,
                " (1 = float16, 2 = bfloat16)");
    TORCH_CHECK(t->numel() >= min_numel, name, " holds ", t->numel(), " elements, needs ",
                min_numel);
    TORCH_CHECK(t->is_cuda() && t->is_contiguous(), name, " must be a contiguous device tensor");
    return reinterpret_cast<uint16_t *>(t->data_ptr());
}

int int32_of(int64_t v, const char *name) {
    TORCH_CHECK(v >= INT32_MIN && v <= INT32_MAX, name, " out of int32 range");
    return static_cast<int>(v);
}

constexpr int64_t MT = DMDQN_MT_WORDS;

// ---------------------------------------------------------------- shared checks
// every tensor of ts (nullptr: an absent optional, see opt()) on the device of ref
void same_device(const Tensor &ref, std::initializer_list<const Tensor *> ts, const char *msg) {
    for (const Tensor *t : ts) TORCH_CHECK(t == nullptr || t->device() == ref.device(), msg);
}

const Tensor *opt(const OptT &t) { return t.has_value() ? &*t : nullptr; }

// the two sizes of a [rows, cols] tensor
std::pair<int64_t, int64_t> dims2(const Tensor &t, const char *msg) {
    TORCH_CHECK(t.dim() == 2, msg);
    return {t.size(0), t.size(1)};
}

// err: one int32 in a device tensor, or in pinned host memory the kernel writes directly
int32_t *err_ptr(Tensor &err) {
    TORCH_CHECK(err.is_cuda() || err.is_pinned(), "err must be a device tensor or pinned host memory");
    TORCH_CHECK(err.scalar_type() == at::kInt && err.numel() == 1, "err must be one int32");
    return reinterpret_cast<int32_t *>(err.data_ptr());
}

dmdqn_idm make_idm(at::ArrayRef<double> idm) {
    TORCH_CHECK(idm.size() == 12, "idm: 12 constants (include/dmdqn.h dmdqn_idm order)");
    return dmdqn_idm{(float)idm[0], (float)idm[1], (float)idm[2], (float)idm[3],
                     (float)idm[4], (float)idm[5], (float)idm[6], (float)idm[7],
                     (float)idm[8], (float)idm[9], (float)idm[10], (float)idm[11]};
}

// The five arrays of a replay ring of NA agents x cap slots.  rows: at::kChar
// (DMDQN_ROW_BYTES per row) or at::kFloat (DMDQN_ROW_FLOATS); Undefined: the
// caller does not read the rows (s, n stay null and unchecked).
struct Rings {
    void *s, *n;
    uint8_t *a, *d;
    double *r;
};

int64_t ring_cap(const Tensor &ring_a, int64_t NA) {
    TORCH_CHECK(NA > 0 && ring_a.numel() % NA == 0, "ring_a must be [NA, cap]");
    return ring_a.numel() / NA;
}

Rings ring_ptrs(const Tensor &ring_s, const Tensor &ring_n, const Tensor &ring_a,
                const Tensor &ring_r, const Tensor &ring_d, int64_t NA, int64_t cap,
                at::ScalarType rows, const char *s_name = "ring_s",
                const char *n_name = "ring_n") {
    Rings g{};
    if (rows != at::ScalarType::Undefined) {
        const int64_t row = rows == at::kFloat ? DMDQN_ROW_FLOATS : DMDQN_ROW_BYTES;
        g.s = dptr<void>(ring_s, rows, s_name, NA * cap * row);
        g.n = dptr<void>(ring_n, rows, n_name, NA * cap * row);
    }
    g.a = dptr<uint8_t>(ring_a, at::kByte, "ring_a", NA * cap);
    g.r = dptr<double>(ring_r, at::kDouble, "ring_r", NA * cap);
    g.d = dptr<uint8_t>(ring_d, at::kByte, "ring_d", NA * cap);
    return g;
}

// One transition per agent as the env hands it over (the input of both stores).
struct Stored {
    const float *s, *n;
    const int32_t *a;
    const double *r;
    const uint8_t *d;
};

Stored stored_ptrs(const Tensor &obs_s, const Tensor &obs_n, const Tensor &act_, const Tensor &rew,
                   const Tensor &done, int64_t NA) {
    Stored t{};
    t.s = dptr<float>(obs_s, at::kFloat, "obs_s", NA * DMDQN_OBS_DIM);
    t.n = dptr<float>(obs_n, at::kFloat, "obs_n", NA * DMDQN_OBS_DIM);
    t.a = dptr<int32_t>(act_, at::kInt, "act", NA);
    t.r = dptr<double>(rew, at::kDouble, "rew", NA);
    t.d = dptr<uint8_t>(done, at::kByte, "done", NA);
    return t;
}

// ---------------------------------------------------------------- streams / act
void mt_seed(Tensor &state, const Tensor &seeds, const std::string &kind) {
    const int64_t E = seeds.numel();
    auto s = dptr<uint32_t>(state, at::kInt, "state", E * MT);
    auto sd = dptr<uint64_t>(seeds, at::kLong, "seeds");
    c10::hip::HIPGuardMasqueradingAsCUDA g(state.device());
    TORCH_CHECK(kind == "np" || kind == "py", "kind must be 'np' or 'py'");
    check(kind == "np" ? dmdqn_mt_seed_np(s, sd, (int)E, stream_of(state))
                       : dmdqn_mt_seed_py(s, sd, (int)E, stream_of(state)),
          "dmdqn_mt_seed");
}

void mt_draw_u32(Tensor &state, int64_t count, Tensor &out) {
    const int64_t E = state.numel() / MT;
    auto s = dptr<uint32_t>(state, at::kInt, "state", E * MT);
    auto o = dptr<uint32_t>(out, at::kInt, "out", E * count);
    c10::hip::HIPGuardMasqueradingAsCUDA g(state.device());
    check(dmdqn_mt_draw_u32(s, (int)E, int32_of(count, "count"), o, stream_of(state)),
          "dmdqn_mt_draw_u32");
}

void act(Tensor &np_state, int64_t A, double eps, int64_t n_actions, const OptT &greedy,
         Tensor &actions, bool uniform) {
    const int64_t E = np_state.numel() / MT;
    auto s = dptr<uint32_t>(np_state, at::kInt, "np_state", E * MT);
    auto gr = optr<int32_t>(greedy, at::kInt, "greedy", E * A);
    auto out = dptr<int32_t>(actions, at::kInt, "actions", E * A);
    c10::hip::HIPGuardMasqueradingAsCUDA g(np_state.device());
    if (uniform)
        check(dmdqn_act_uniform(s, (int)E, int32_of(A, "A"), int32_of(n_actions, "n_actions"), out,
                                stream_of(np_state)),
              "dmdqn_act_uniform");
    else
        check(dmdqn_act(s, (int)E, int32_of(A, "A"), eps, int32_of(n_actions, "n_actions"), gr, out,
                        stream_of(np_state)),
              "dmdqn_act");
}

// ---------------------------------------------------------------- observe
void observe(int64_t R, int64_t C, const Tensor &halt, const Tensor &phase, const Tensor &tspent,
             int64_t mode, const OptT &local, const OptT &obs, const OptT &prev_local,
             const OptT &reward) {
    const int64_t A = R * C;
    TORCH_CHECK(A > 0 && halt.numel() % (A * 12) == 0, "halt must be [E, R*C, 12]");
    const int64_t E = halt.numel() / (A * 12);
    auto h = dptr<int32_t>(halt, at::kInt, "halt");
    auto p = dptr<int32_t>(phase, at::kInt, "phase", E * A);
    auto ts = dptr<int32_t>(tspent, at::kInt, "tspent", E * A);
    auto lo = optr<float>(local, at::kFloat, "local", E * A * DMDQN_LOCAL_DIM);
    auto ob = optr<float>(obs, at::kFloat, "obs", E * A * DMDQN_OBS_DIM);
    auto pl = optr<float>(prev_local, at::kFloat, "prev_local", E * A * DMDQN_LOCAL_DIM);
    auto rw = optr<double>(reward, at::kDouble, "reward", E * A);
    TORCH_CHECK((pl == nullptr) == (rw == nullptr), "prev_local and reward go together");
    c10::hip::HIPGuardMasqueradingAsCUDA g(halt.device());
    check(dmdqn_observe((int)R, (int)C, (int)E, h, p, ts, (int)mode, lo, ob, pl, rw,
                        stream_of(halt)),
          "dmdqn_observe");
}

// ---------------------------------------------------------------- replay
void replay_store(int64_t slot, const Tensor &obs_s, const Tensor &obs_n, const Tensor &act_,
                  const Tensor &rew, const Tensor &done, Tensor &ring_s, Tensor &ring_n,
                  Tensor &ring_a, Tensor &ring_r, Tensor &ring_d, Tensor &err) {
    const int64_t NA = act_.numel(), cap = ring_cap(ring_a, NA);
    const Stored t = stored_ptrs(obs_s, obs_n, act_, rew, done, NA);
    const Rings rg = ring_ptrs(ring_s, ring_n, ring_a, ring_r, ring_d, NA, cap, at::kChar);
    auto e = err_ptr(err);
    c10::hip::HIPGuardMasqueradingAsCUDA g(obs_s.device());
    check(dmdqn_replay_store((int)NA, int32_of(cap, "cap"), int32_of(slot, "slot"), t.s, t.n, t.a,
                             t.r, t.d, (int8_t *)rg.s, (int8_t *)rg.n, rg.a, rg.r, rg.d, e,
                             stream_of(obs_s)),
          "dmdqn_replay_store");
}

void replay_store_f32(int64_t slot, const Tensor &obs_s, const Tensor &obs_n, const Tensor &act_,
                      const Tensor &rew, const Tensor &done, Tensor &rows_s, Tensor &rows_n,
                      Tensor &ring_a, Tensor &ring_r, Tensor &ring_d) {
    const int64_t NA = act_.numel(), cap = ring_cap(ring_a, NA);
    const Stored t = stored_ptrs(obs_s, obs_n, act_, rew, done, NA);
    const Rings rg = ring_ptrs(rows_s, rows_n, ring_a, ring_r, ring_d, NA, cap, at::kFloat,
                               "rows_s", "rows_n");
    c10::hip::HIPGuardMasqueradingAsCUDA g(obs_s.device());
    check(dmdqn_replay_store_f32((int)NA, int32_of(cap, "cap"), int32_of(slot, "slot"), t.s, t.n,
                                 t.a, t.r, t.d, (float *)rg.s, (float *)rg.n, rg.a, rg.r, rg.d,
                                 stream_of(obs_s)),
          "dmdqn_replay_store_f32");
}

void replay_gather_f32(const Tensor &rows_s, const Tensor &rows_n, const Tensor &idx,
                       int64_t start, Tensor &xs, Tensor &xn) {
    TORCH_CHECK(idx.dim() == 2, "idx must be [NA, batch]");
    const int64_t NA = idx.size(0), B = idx.size(1);
    TORCH_CHECK(rows_s.dim() == 3 && rows_s.size(0) == NA && rows_s.size(2) == DMDQN_ROW_FLOATS,
                "rows_s must be [NA, cap, ", DMDQN_ROW_FLOATS, "]");
    const int64_t cap = rows_s.size(1);
    auto rs = dptr<float>(rows_s, at::kFloat, "rows_s", NA * cap * DMDQN_ROW_FLOATS);
    auto rn = dptr<float>(rows_n, at::kFloat, "rows_n", NA * cap * DMDQN_ROW_FLOATS);
    auto ix = dptr<int32_t>(idx, at::kInt, "idx", NA * B);
    auto ps = dptr<float>(xs, at::kFloat, "xs", NA * B * DMDQN_ROW_FLOATS);
    auto pn = dptr<float>(xn, at::kFloat, "xn", NA * B * DMDQN_ROW_FLOATS);
    c10::hip::HIPGuardMasqueradingAsCUDA g(rows_s.device());
    check(dmdqn_replay_gather_f32(rs, rn, ix, (int)NA, int32_of(cap, "cap"), int32_of(start, "start"),
                                  (int)B, ps, pn, stream_of(rows_s)),
          "dmdqn_replay_gather_f32");
}

// The n-step transition of the staging window (include/dmdqn.h
// dmdqn_replay_nstep_commit): st_* the staging ring [NA, n, ...], ring_* the
// replay ring; int8 or float rows by the dtype of st_s; gamma_a f64 [NA] or None.
void replay_nstep_commit(int64_t head, int64_t slot, const Tensor &st_s, const Tensor &st_n,
                         const Tensor &st_a, const Tensor &st_r, const Tensor &st_d,
                         Tensor &ring_s, Tensor &ring_n, Tensor &ring_a, Tensor &ring_r,
                         Tensor &ring_d, double gamma, const OptT &gamma_a) {
    TORCH_CHECK(st_a.dim() == 2 && ring_a.dim() == 2 && st_a.size(0) == ring_a.size(0),
                "st_a must be [NA, n] and ring_a [NA, cap]");
    const int64_t NA = st_a.size(0), n = st_a.size(1), cap = ring_a.size(1);
    TORCH_CHECK(NA > 0 && n > 0 && cap > 0, "NA, n and cap must be positive");
    TORCH_CHECK(st_s.scalar_type() == at::kChar || st_s.scalar_type() == at::kFloat,
                "st_s must be int8 (128-byte rows) or float32 rows, got ", st_s.scalar_type());
    const bool f32 = st_s.scalar_type() == at::kFloat;
    const at::ScalarType rt = f32 ? at::kFloat : at::kChar;
    const int64_t rw = f32 ? DMDQN_ROW_FLOATS : DMDQN_ROW_BYTES;
    dmdqn_nstep_args a{};
    a.NA = int32_of(NA, "NA"); a.n = int32_of(n, "n"); a.head = int32_of(head, "head");
    a.cap = int32_of(cap, "cap"); a.slot = int32_of(slot, "slot");
    a.row_format = f32 ? DMDQN_ROWS_F32 : DMDQN_ROWS_I8;
    a.st_s = dptr<void>(st_s, rt, "st_s", NA * n * rw);
    a.st_n = dptr<void>(st_n, rt, "st_n", NA * n * rw);
    a.st_a = dptr<uint8_t>(st_a, at::kByte, "st_a", NA * n);
    a.st_r = dptr<double>(st_r, at::kDouble, "st_r", NA * n);
    a.st_d = dptr<uint8_t>(st_d, at::kByte, "st_d", NA * n);
    const Rings rg = ring_ptrs(ring_s, ring_n, ring_a, ring_r, ring_d, NA, cap, rt);
    a.ring_s = rg.s; a.ring_n = rg.n; a.ring_a = rg.a; a.ring_r = rg.r; a.ring_d = rg.d;
    a.gamma = gamma;
    a.gamma_a = optr<const double>(gamma_a, at::kDouble, "gamma_a", NA);
    same_device(st_s, {&st_n, &st_a, &st_r, &st_d, &ring_s, &ring_n, &ring_a, &ring_r, &ring_d},
                "staging and replay rings must share a device");
    same_device(st_s, {opt(gamma_a)}, "gamma_a must be on the device of the rings");
    c10::hip::HIPGuardMasqueradingAsCUDA g(st_s.device());
    check(dmdqn_replay_nstep_commit(&a, stream_of(st_s)), "dmdqn_replay_nstep_commit");
}

void replay_sample(Tensor &py_state, int64_t A, int64_t n, int64_t k, Tensor &idx,
                   int64_t lds_budget) {
    const int64_t E = py_state.numel() / MT;
    auto s = dptr<uint32_t>(py_state, at::kInt, "py_state", E * MT);
    auto o = dptr<int32_t>(idx, at::kInt, "idx", E * A * k);
    TORCH_CHECK(lds_budget >= 0, "lds_budget must be >= 0");
    c10::hip::HIPGuardMasqueradingAsCUDA g(py_state.device());
    check(dmdqn_replay_sample_budget(s, (int)E, int32_of(A, "A"), int32_of(n, "n"),
                                     int32_of(k, "k"), (size_t)lds_budget, o, stream_of(py_state)),
          "dmdqn_replay_sample");
}

// ---------------------------------------------------------------- simulator
// state (mutable, in order): x, v, dst, head, cnt, req, gfrom, fx, fv, tl_phase,
// tl_ts, qptr, stats, last_det[, t_env]; tables: q_off, q_ids, vdst, exit_id,
// exit_ao, q_dst; dims: R, C, E, cap_lane, period_ms, nveh, actuated.
dmdqn_sim make_sim(at::TensorList state, at::TensorList tables, at::IntArrayRef dims) {
    TORCH_CHECK((state.size() == 14 || state.size() == 15) && tables.size() == 6 && dims.size() == 7,
                "sim: 14 state tensors (+ t_env), 6 tables, 7 dims");
    dmdqn_sim s{};
    s.R = (int)dims[0]; s.C = (int)dims[1]; s.E = (int)dims[2]; s.cap_lane = (int)dims[3];
    s.period_ms = (int)dims[4]; s.nveh = (int)dims[5]; s.actuated = (int)dims[6];
    const int64_t A = (int64_t)s.R * s.C, X = 2 * (int64_t)s.R + 2 * s.C, E = s.E;
    const int64_t NL = 3 * (4 * A + X), ns = E * NL * s.cap_lane;
    s.x = dptr<float>(state[0], at::kFloat, "x", ns);
    s.v = dptr<float>(state[1], at::kFloat, "v", ns);
    s.dst = dptr<int32_t>(state[2], at::kInt, "dst", ns);
    s.head = dptr<int32_t>(state[3], at::kInt, "head", E * NL);
    s.cnt = dptr<int32_t>(state[4], at::kInt, "cnt", E * NL);
    s.req = dptr<int32_t>(state[5], at::kInt, "req", E * NL);
    s.gfrom = dptr<int32_t>(state[6], at::kInt, "gfrom", E * NL);
    s.fx = dptr<float>(state[7], at::kFloat, "fx", E * NL);
    s.fv = dptr<float>(state[8], at::kFloat, "fv", E * NL);
    s.tl_phase = dptr<int32_t>(state[9], at::kInt, "tl_phase", E * A);
    s.tl_ts = dptr<int32_t>(state[10], at::kInt, "tl_ts", E * A);
    s.qptr = dptr<int32_t>(state[11], at::kInt, "qptr", E * 4 * A);
    s.stats = dptr<int32_t>(state[12], at::kInt, "stats", E * 4);
    s.last_det = dptr<int32_t>(state[13], at::kInt, "last_det", E * 12 * A);
    s.t_env = state.size() == 15 ? dptr<int32_t>(state[14], at::kInt, "t_env", E) : nullptr;
    s.q_off = dptr<int32_t>(tables[0], at::kInt, "q_off", E * (4 * A + 1));
    s.q_ids = dptr<uint16_t>(tables[1], at::kShort, "q_ids", E * s.nveh);
    s.vdst = dptr<uint16_t>(tables[2], at::kShort, "vdst", E * s.nveh);
    s.exit_id = dptr<int32_t>(tables[3], at::kInt, "exit_id", A * 4);
    s.exit_ao = dptr<int32_t>(tables[4], at::kInt, "exit_ao", X * 2);
    s.q_dst = dptr<uint16_t>(tables[5], at::kShort, "q_dst", E * s.nveh);
    return s;
}

void sim_reset(at::TensorList state, at::TensorList tables, at::IntArrayRef dims,
               const OptT &mask) {
    dmdqn_sim s = make_sim(state, tables, dims);
    auto m = optr<uint8_t>(mask, at::kByte, "mask", s.E);
    c10::hip::HIPGuardMasqueradingAsCUDA g(state[0].device());
    check(dmdqn_sim_reset_envs(&s, m, stream_of(state[0])), "dmdqn_sim_reset_envs");
}

// what a step of E envs x A junctions writes for the observation that follows
struct StepOut {
    int32_t *halt, *phase, *tspent;
    uint8_t *done;
};

StepOut step_out(Tensor &halt, Tensor &phase, Tensor &tspent, Tensor &done, int64_t E, int64_t A) {
    StepOut o{};
    o.halt = dptr<int32_t>(halt, at::kInt, "halt", E * A * 12);
    o.phase = dptr<int32_t>(phase, at::kInt, "phase", E * A);
    o.tspent = dptr<int32_t>(tspent, at::kInt, "tspent", E * A);
    o.done = dptr<uint8_t>(done, at::kByte, "done", E);
    return o;
}

void sim_step(at::TensorList state, at::TensorList tables, at::IntArrayRef dims,
              at::ArrayRef<double> idm, const OptT &actions, int64_t stride, int64_t t0, int64_t K,
              int64_t max_time, Tensor &halt, Tensor &phase, Tensor &tspent, Tensor &done) {
    dmdqn_sim s = make_sim(state, tables, dims);
    dmdqn_idm p = make_idm(idm);
    const int64_t A = (int64_t)s.R * s.C, E = s.E;
    auto a = optr<int32_t>(actions, at::kInt, "actions", E * A);
    const StepOut o = step_out(halt, phase, tspent, done, E, A);
    c10::hip::HIPGuardMasqueradingAsCUDA g(halt.device());
    check(dmdqn_sim_step(&s, &p, a, (int)stride, int32_of(t0, "t0"), (int)K,
                         int32_of(max_time, "max_time"), o.halt, o.phase, o.tspent, o.done,
                         stream_of(halt)),
          "dmdqn_sim_step");
}

// act + sim_step + observe + replay_store (int8 rows) in one launch per env.
void env_step(at::TensorList state, at::TensorList tables, at::IntArrayRef dims,
              at::ArrayRef<double> idm, int64_t stride, int64_t t0, int64_t K, int64_t max_time,
              Tensor &halt, Tensor &phase, Tensor &tspent, Tensor &done, Tensor &np_state,
              const OptT &greedy, Tensor &actions, double eps, int64_t n_actions, int64_t mode,
              Tensor &local, Tensor &obs, const Tensor &prev_local, Tensor &reward,
              const Tensor &obs_s, int64_t slot, Tensor &ring_s, Tensor &ring_n, Tensor &ring_a,
              Tensor &ring_r, Tensor &ring_d, Tensor &err) {
    dmdqn_sim s = make_sim(state, tables, dims);
    dmdqn_idm p = make_idm(idm);
    const int64_t A = (int64_t)s.R * s.C, E = s.E, NA = E * A;
    const StepOut o = step_out(halt, phase, tspent, done, E, A);
    TORCH_CHECK(ring_a.numel() % NA == 0 && ring_a.numel() > 0, "ring_a must be [E*A, cap]");
    const int64_t cap = ring_a.numel() / NA;
    dmdqn_env_fuse f{};
    f.np_state = dptr<uint32_t>(np_state, at::kInt, "np_state", E * MT);
    f.greedy = optr<int32_t>(greedy, at::kInt, "greedy", NA);
    f.actions = dptr<int32_t>(actions, at::kInt, "actions", NA);
    f.eps = eps;
    f.n_actions = int32_of(n_actions, "n_actions");
    f.mode = (int)mode;
    f.local = dptr<float>(local, at::kFloat, "local", NA * DMDQN_LOCAL_DIM);
    f.obs = dptr<float>(obs, at::kFloat, "obs", NA * DMDQN_OBS_DIM);
    f.prev_local = dptr<float>(prev_local, at::kFloat, "prev_local", NA * DMDQN_LOCAL_DIM);
    f.reward = dptr<double>(reward, at::kDouble, "reward", NA);
    f.obs_s = dptr<float>(obs_s, at::kFloat, "obs_s", NA * DMDQN_OBS_DIM);
    f.cap = int32_of(cap, "cap");
    f.slot = int32_of(slot, "slot");
    const Rings rg = ring_ptrs(ring_s, ring_n, ring_a, ring_r, ring_d, NA, cap, at::kChar);
    f.ring_s = (int8_t *)rg.s; f.ring_n = (int8_t *)rg.n;
    f.ring_a = rg.a; f.ring_r = rg.r; f.ring_d = rg.d;
    f.err = err_ptr(err);
    c10::hip::HIPGuardMasqueradingAsCUDA g(halt.device());
    check(dmdqn_env_step(&s, &p, &f, (int)stride, int32_of(t0, "t0"), (int)K,
                         int32_of(max_time, "max_time"), o.halt, o.phase, o.tspent, o.done,
                         stream_of(halt)),
          "dmdqn_env_step");
}

// ---------------------------------------------------------------- learn
dmdqn_learn_args make_learn(const Tensor &ring_s, const Tensor &ring_n, const Tensor &ring_a,
                            const Tensor &ring_d, const Tensor &ring_r, const Tensor &idx,
                            Tensor &params, const OptT &adam_m, const OptT &adam_v,
                            Tensor &target, const OptT &target_h, const OptT &loss, int64_t start,
                            int64_t hidden, int64_t precision, bool sync, double gamma,
                            double alpha, double c1, double c2, double eps, int64_t loss_kind,
                            const OptT &qstats, const OptT &rn_out, const OptT &params_h,
                            const OptT &stamps, int64_t NA, int64_t NW,
                            const OptT &xs = std::nullopt, const OptT &xn = std::nullopt) {
    dmdqn_learn_args a{};
    const int64_t cap = ring_cap(ring_a, NA), B = idx.numel() / NA;
    TORCH_CHECK(NW > 0 && params.numel() % NW == 0, "params must be [NW, P]");
    const int64_t P = params.numel() / NW;
    a.NA = (int)NA; a.cap = int32_of(cap, "cap"); a.start = int32_of(start, "start");
    a.batch = (int)B; a.hidden = (int)hidden; a.precision = (int)precision;
    a.sync_target = sync ? 1 : 0; a.P = (int)P;
    TORCH_CHECK(xs.has_value() == xn.has_value(), "xs and xn go together");
    if (xs.has_value()) {  // float rows: the batch pre-gathered (replay_gather_f32)
        a.row_format = DMDQN_ROWS_F32;
        a.xs = dptr<float>(*xs, at::kFloat, "xs", NA * B * DMDQN_ROW_FLOATS);
        a.xn = dptr<float>(*xn, at::kFloat, "xn", NA * B * DMDQN_ROW_FLOATS);
    }
    const Rings rg = ring_ptrs(ring_s, ring_n, ring_a, ring_r, ring_d, NA, cap,
                               xs.has_value() ? at::ScalarType::Undefined : at::kChar);
    a.ring_s = (const int8_t *)rg.s; a.ring_n = (const int8_t *)rg.n;
    a.ring_a = rg.a; a.ring_d = rg.d; a.ring_r = rg.r;
    a.idx = dptr<int32_t>(idx, at::kInt, "idx", NA * B);
    a.params = dptr<float>(params, at::kFloat, "params");
    a.adam_m = optr<float>(adam_m, at::kFloat, "adam_m", NW * P);
    a.adam_v = optr<float>(adam_v, at::kFloat, "adam_v", NW * P);
    a.target = dptr<float>(target, at::kFloat, "target", NW * P);
    // the kernels read NW rows of Ph = P rounded up to 8 halves
    const int64_t Ph = (P + 7) / 8 * 8;
    if (precision == 0) TORCH_CHECK(!target_h.has_value(), "target_h is for precision 1 / 2");
    a.target_h = h16ptr(target_h, "target_h", precision == 0 ? -1 : precision, NW * Ph);
    a.loss = optr<float>(loss, at::kFloat, "loss", NA);
    a.gamma = (float)gamma; a.alpha = (float)alpha; a.c1 = (float)c1; a.c2 = (float)c2;
    a.eps = (float)eps;
    a.stamps = optr<uint64_t>(stamps, at::kLong, "stamps", NA * 16);
    a.qstats = optr<float>(qstats, at::kFloat, "qstats", NA * 6);
    a.params_h = h16ptr(params_h, "params_h", precision == 0 ? -1 : precision, NW * Ph);
    a.loss_kind = (int)loss_kind;
    a.rn_out = optr<float>(rn_out, at::kFloat, "rn_out", NA * B);
    return a;
}

// Per-agent hyperparameters (include/dmdqn.h dmdqn_agent_hparams): lr / gamma_a /
// tau_a / one_minus_tau_a f32 [NA] tensors on the device of params, or None (the
// scalar of the same launch); adam_s / adam_d the two Adam factors of the learn
// as float32.
dmdqn_agent_hparams make_hparams(const OptT &lr, const OptT &gamma_a, const OptT &tau_a,
                                 const OptT &one_minus_tau_a, double adam_s, double adam_d,
                                 int64_t NA, const Tensor &params) {
    dmdqn_agent_hparams hp{};
    hp.lr = optr<const float>(lr, at::kFloat, "lr", NA);
    hp.gamma = optr<const float>(gamma_a, at::kFloat, "gamma_a", NA);
    hp.tau = optr<const float>(tau_a, at::kFloat, "tau_a", NA);
    hp.one_minus_tau = optr<const float>(one_minus_tau_a, at::kFloat, "one_minus_tau_a", NA);
    TORCH_CHECK((hp.tau == nullptr) == (hp.one_minus_tau == nullptr),
                "tau_a and one_minus_tau_a go together");
    same_device(params, {opt(lr), opt(gamma_a), opt(tau_a), opt(one_minus_tau_a)},
                "per-agent hyperparameters must be on the device of params");
    hp.adam_s = (float)adam_s;
    hp.adam_d = (float)adam_d;
    return hp;
}

// The one learn behind learn_step / learn_step_hp / learn_step_clip.  The kind
// fixes the C entry points: scalar the plain ones, hp the _hp trio, clip the
// gradient launch of hp and the clipping Adam launch.  grad: the split learn
// (gradient launch, then the Adam launch); null: the fused one.  An optional
// block of a new learn variant belongs here, not in a fourth copy.
enum class Learn { scalar, hp, clip };

void learn_any(Learn kind, const Tensor &ring_s, const Tensor &ring_n, const Tensor &ring_a,
               const Tensor &ring_d, const Tensor &ring_r, const Tensor &idx, Tensor &params,
               Tensor &adam_m, Tensor &adam_v, Tensor &target, const OptT &target_h, Tensor &loss,
               int64_t start, int64_t hidden, int64_t precision, bool sync, double gamma,
               double alpha, double c1, double c2, double eps, int64_t loss_kind,
               const OptT &qstats, const OptT &rn_out, const OptT &stamps, const Tensor *grad,
               const OptT &xs, const OptT &xn, double tau, double one_minus_tau, const OptT &lr,
               const OptT &gamma_a, const OptT &tau_a, const OptT &one_minus_tau_a, double adam_s,
               double adam_d, double clip, const OptT &gnorm) {
    const int64_t NA = loss.numel();
    dmdqn_learn_args a = make_learn(ring_s, ring_n, ring_a, ring_d, ring_r, idx, params, adam_m,
                                    adam_v, target, target_h, loss, start, hidden, precision, sync,
                                    gamma, alpha, c1, c2, eps, loss_kind, qstats, rn_out,
                                    std::nullopt, stamps, NA, NA, xs, xn);
    // the soft target update of this learn (update_target_network_soft,
    // dqn_agent.py:389-399): float32(tau), float32(1 - tau) from the host; 0 = off
    a.tau = (float)tau;
    a.one_minus_tau = (float)one_minus_tau;
    dmdqn_agent_hparams hp{};
    if (kind != Learn::scalar)
        hp = make_hparams(lr, gamma_a, tau_a, one_minus_tau_a, adam_s, adam_d, NA, params);
    float *gr = grad ? dptr<float>(*grad, at::kFloat, "grad", NA * (int64_t)a.P) : nullptr;
    float *gn = nullptr;
    if (kind == Learn::clip) {
        same_device(params, {opt(gnorm)}, "gnorm must be on the device of params");
        gn = optr<float>(gnorm, at::kFloat, "gnorm", NA);
        // (before the gradient launch: the Adam entry point would refuse it after)
        TORCH_CHECK((float)clip > 0.0f && (float)clip <= std::numeric_limits<float>::max(),
                    "clip must be finite and > 0 as float32, got ", clip);
    }
    c10::hip::HIPGuardMasqueradingAsCUDA g(params.device());
    void *st = stream_of(params);
    if (kind == Learn::scalar && gr == nullptr) {
        check(dmdqn_learn(&a, st), "dmdqn_learn");
    } else if (kind == Learn::scalar) {
        check(dmdqn_learn_grad(&a, gr, st), "dmdqn_learn_grad");
        check(dmdqn_adam_agents(&a, gr, st), "dmdqn_adam_agents");
    } else if (gr == nullptr) {
        check(dmdqn_learn_hp(&a, &hp, st), "dmdqn_learn_hp");
    } else {
        check(dmdqn_learn_grad_hp(&a, &hp, gr, st), "dmdqn_learn_grad_hp");
        if (kind == Learn::clip)
            check(dmdqn_adam_agents_clip(&a, &hp, gr, (float)clip, gn, st),
                  "dmdqn_adam_agents_clip");
        else
            check(dmdqn_adam_agents_hp(&a, &hp, gr, st), "dmdqn_adam_agents_hp");
    }
}

void learn_step(const Tensor &ring_s, const Tensor &ring_n, const Tensor &ring_a,
                const Tensor &ring_d, const Tensor &ring_r, const Tensor &idx, Tensor &params,
                Tensor &adam_m, Tensor &adam_v, Tensor &target, const OptT &target_h, Tensor &loss,
                int64_t start, int64_t hidden, int64_t precision, bool sync, double gamma,
                double alpha, double c1, double c2, double eps, int64_t loss_kind,
                const OptT &qstats, const OptT &rn_out, const OptT &stamps, const OptT &grad,
                const OptT &xs, const OptT &xn, double tau, double one_minus_tau) {
    learn_any(Learn::scalar, ring_s, ring_n, ring_a, ring_d, ring_r, idx, params, adam_m, adam_v,
              target, target_h, loss, start, hidden, precision, sync, gamma, alpha, c1, c2, eps,
              loss_kind, qstats, rn_out, stamps, opt(grad), xs, xn, tau, one_minus_tau,
              std::nullopt, std::nullopt, std::nullopt, std::nullopt, 1.0, 1.0, 0.0, std::nullopt);
}

// learn_step with per-agent hyperparameters (make_hparams).  All None: exactly
// learn_step.
void learn_step_hp(const Tensor &ring_s, const Tensor &ring_n, const Tensor &ring_a,
                   const Tensor &ring_d, const Tensor &ring_r, const Tensor &idx, Tensor &params,
                   Tensor &adam_m, Tensor &adam_v, Tensor &target, const OptT &target_h,
                   Tensor &loss, int64_t start, int64_t hidden, int64_t precision, bool sync,
                   double gamma, double alpha, double c1, double c2, double eps, int64_t loss_kind,
                   const OptT &qstats, const OptT &rn_out, const OptT &stamps, const OptT &grad,
                   const OptT &xs, const OptT &xn, double tau, double one_minus_tau,
                   const OptT &lr, const OptT &gamma_a, const OptT &tau_a,
                   const OptT &one_minus_tau_a, double adam_s, double adam_d) {
    learn_any(Learn::hp, ring_s, ring_n, ring_a, ring_d, ring_r, idx, params, adam_m, adam_v,
              target, target_h, loss, start, hidden, precision, sync, gamma, alpha, c1, c2, eps,
              loss_kind, qstats, rn_out, stamps, opt(grad), xs, xn, tau, one_minus_tau, lr,
              gamma_a, tau_a, one_minus_tau_a, adam_s, adam_d, 0.0, std::nullopt);
}

// learn_step_hp as the split learn (grad required) with the gradient of every
// agent clipped by its global norm before the Adam step (include/dmdqn.h
// dmdqn_adam_agents_clip): clip > 0; gnorm f32 [NA] receives the norms before
// clipping, or None.
void learn_step_clip(const Tensor &ring_s, const Tensor &ring_n, const Tensor &ring_a,
                     const Tensor &ring_d, const Tensor &ring_r, const Tensor &idx, Tensor &params,
                     Tensor &adam_m, Tensor &adam_v, Tensor &target, const OptT &target_h,
                     Tensor &loss, int64_t start, int64_t hidden, int64_t precision, bool sync,
                     double gamma, double alpha, double c1, double c2, double eps,
                     int64_t loss_kind, const OptT &qstats, const OptT &rn_out, const OptT &stamps,
                     Tensor &grad, const OptT &xs, const OptT &xn, double tau,
                     double one_minus_tau, const OptT &lr, const OptT &gamma_a, const OptT &tau_a,
                     const OptT &one_minus_tau_a, double adam_s, double adam_d, double clip,
                     const OptT &gnorm) {
    learn_any(Learn::clip, ring_s, ring_n, ring_a, ring_d, ring_r, idx, params, adam_m, adam_v,
              target, target_h, loss, start, hidden, precision, sync, gamma, alpha, c1, c2, eps,
              loss_kind, qstats, rn_out, stamps, &grad, xs, xn, tau, one_minus_tau, lr, gamma_a,
              tau_a, one_minus_tau_a, adam_s, adam_d, clip, gnorm);
}

// Two consecutive learns of every agent in one launch (dmdqn_learn_pair): the
// shared tensors once, then what a step fixes for each learn -- idx, loss,
// start, adam = [alpha, c1, c2, eps], qstats, rn_out and, with per-agent
// hyperparameters, factors = [adam_s, adam_d].
void learn_pair(const Tensor &ring_s, const Tensor &ring_n, const Tensor &ring_a,
                const Tensor &ring_d, const Tensor &ring_r, Tensor &params, Tensor &adam_m,
                Tensor &adam_v, Tensor &target, Tensor &target_h, const Tensor &idx0,
                const Tensor &idx1, Tensor &loss0, Tensor &loss1, int64_t start0, int64_t start1,
                int64_t hidden, int64_t precision, double gamma, at::ArrayRef<double> adam0,
                at::ArrayRef<double> adam1, int64_t loss_kind, const OptT &qstats0,
                const OptT &qstats1, const OptT &rn_out0, const OptT &rn_out1, double tau,
                double one_minus_tau, const OptT &lr, const OptT &gamma_a, const OptT &tau_a,
                const OptT &one_minus_tau_a, at::ArrayRef<double> factors0,
                at::ArrayRef<double> factors1) {
    const int64_t NA = loss0.numel();
    TORCH_CHECK(adam0.size() == 4 && adam1.size() == 4, "adam0 / adam1: [alpha, c1, c2, eps]");
    TORCH_CHECK(factors0.size() == 2 && factors1.size() == 2, "factors0 / factors1: [s, d]");
    TORCH_CHECK(loss1.numel() == NA, "loss0 and loss1 must both be [NA]");
    const OptT th = target_h;
    dmdqn_learn_args a[2];
    dmdqn_agent_hparams hp[2];
    for (int i = 0; i < 2; i++) {
        const at::ArrayRef<double> &ad = i ? adam1 : adam0, &fa = i ? factors1 : factors0;
        const OptT lo = i ? loss1 : loss0;
        a[i] = make_learn(ring_s, ring_n, ring_a, ring_d, ring_r, i ? idx1 : idx0, params, adam_m,
                          adam_v, target, th, lo, i ? start1 : start0, hidden, precision, false,
                          gamma, ad[0], ad[1], ad[2], ad[3], loss_kind, i ? qstats1 : qstats0,
                          i ? rn_out1 : rn_out0, std::nullopt, std::nullopt, NA, NA);
        a[i].tau = (float)tau;
        a[i].one_minus_tau = (float)one_minus_tau;
        hp[i] = make_hparams(lr, gamma_a, tau_a, one_minus_tau_a, fa[0], fa[1], NA, params);
    }
    c10::hip::HIPGuardMasqueradingAsCUDA g(params.device());
    check(dmdqn_learn_pair(&a[0], &a[1], &hp[0], &hp[1], stream_of(params)), "dmdqn_learn_pair");
}

void learn_shared_grad(const Tensor &ring_s, const Tensor &ring_n, const Tensor &ring_a,
                       const Tensor &ring_d, const Tensor &ring_r, const Tensor &idx,
                       const Tensor &params, const Tensor &target, const Tensor &target_h,
                       const Tensor &params_h, Tensor &loss, int64_t start, double gamma,
                       int64_t loss_kind, const OptT &qstats, const OptT &rn_out, Tensor &slab,
                       const OptT &grad, double scale, const OptT &work) {
    const int64_t NA = loss.numel();
    Tensor p = params, t = target;  // read-only here: the Adam step is a separate op
    dmdqn_learn_args a = make_learn(ring_s, ring_n, ring_a, ring_d, ring_r, idx, p, std::nullopt,
                                    std::nullopt, t, target_h, loss, start, 128, 1, false, gamma,
                                    0.0, 0.0, 0.0, 0.0, loss_kind, qstats, rn_out, params_h,
                                    std::nullopt, NA, 1);
    TORCH_CHECK(slab.numel() % a.P == 0, "slab must be [n_slabs, P]");
    const int n_slabs = (int)(slab.numel() / a.P);
    auto sl = dptr<float>(slab, at::kFloat, "slab");
    auto gr = optr<float>(grad, at::kFloat, "grad", a.P);  // None: dmdqn_adam_slabs reduces
    auto wk = optr<uint8_t>(work, at::kByte, "work",
                            (int64_t)dmdqn_learn_shared_work_bytes((int)NA));
    c10::hip::HIPGuardMasqueradingAsCUDA g(params.device());
    check(dmdqn_learn_shared_grad(&a, sl, n_slabs, gr, (float)scale, wk, stream_of(params)),
          "dmdqn_learn_shared_grad");
}

// The shared net as the flat Adam step sees it: n weights, their Adam slots,
// target and gradient, and the f16 shadows k_adam writes (the shared net is
// fp16-only).
struct FlatNet {
    int64_t n;
    float *w, *m, *v, *t, *g;
    uint16_t *th, *wh;
};

FlatNet flat_net(Tensor &params, Tensor &adam_m, Tensor &adam_v, Tensor &target,
                 const OptT &target_h, const OptT &params_h, const Tensor &grad) {
    FlatNet f{};
    f.n = params.numel();
    f.w = dptr<float>(params, at::kFloat, "params");
    f.m = dptr<float>(adam_m, at::kFloat, "adam_m", f.n);
    f.v = dptr<float>(adam_v, at::kFloat, "adam_v", f.n);
    f.t = dptr<float>(target, at::kFloat, "target", f.n);
    f.g = dptr<float>(grad, at::kFloat, "grad", f.n);
    f.th = h16ptr(target_h, "target_h", 1, f.n);
    f.wh = h16ptr(params_h, "params_h", 1, f.n);
    return f;
}

void adam(Tensor &params, Tensor &adam_m, Tensor &adam_v, Tensor &target, const OptT &target_h,
          const OptT &params_h, const Tensor &grad, double gscale, double alpha, double c1,
          double c2, double eps, bool sync) {
    const FlatNet f = flat_net(params, adam_m, adam_v, target, target_h, params_h, grad);
    c10::hip::HIPGuardMasqueradingAsCUDA g(params.device());
    check(dmdqn_adam(f.w, f.m, f.v, f.t, f.th, f.wh, f.g, int32_of(f.n, "n"), (float)gscale,
                     (float)alpha, (float)c1, (float)c2, (float)eps, sync ? 1 : 0,
                     stream_of(params)),
          "dmdqn_adam");
}

void adam_slabs(Tensor &params, Tensor &adam_m, Tensor &adam_v, Tensor &target,
                const OptT &target_h, const OptT &params_h, const Tensor &slab, Tensor &grad,
                double scale, double gscale, double alpha, double c1, double c2, double eps,
                bool sync) {
    const FlatNet f = flat_net(params, adam_m, adam_v, target, target_h, params_h, grad);
    TORCH_CHECK(slab.numel() % f.n == 0, "slab must be [n_slabs, P]");
    auto sl = dptr<float>(slab, at::kFloat, "slab");
    c10::hip::HIPGuardMasqueradingAsCUDA g(params.device());
    check(dmdqn_adam_slabs(f.w, f.m, f.v, f.t, f.th, f.wh, sl,
                           int32_of(slab.numel() / f.n, "n_slabs"), f.g, (float)scale,
                           int32_of(f.n, "n"), (float)gscale, (float)alpha, (float)c1, (float)c2,
                           (float)eps, sync ? 1 : 0, stream_of(params)),
          "dmdqn_adam_slabs");
}

// Ph, the row stride of an optional 16-bit shadow [rows, Ph] beside f32 rows of
// P values (P without one).
int64_t shadow_stride(const OptT &target_h, int64_t rows, int64_t P, const char *msg) {
    const int64_t Ph = target_h.has_value() ? target_h->numel() / rows : P;
    TORCH_CHECK(!target_h.has_value() || (target_h->numel() % rows == 0 && Ph >= P), msg);
    return Ph;
}

// NW online nets [NW, P], their f32 targets and the targets' optional shadow.
struct Nets {
    int64_t NW, P, Ph;
    float *params, *target;
};

Nets nets_of(const Tensor &params, Tensor &target, const OptT &target_h) {
    Nets n{};
    std::tie(n.NW, n.P) = dims2(params, "params must be [NW, P]");
    n.params = dptr<float>(params, at::kFloat, "params");
    n.target = dptr<float>(target, at::kFloat, "target", n.NW * n.P);
    n.Ph = shadow_stride(target_h, n.NW, n.P, "target_h must be [NW, Ph] with Ph >= P");
    return n;
}

void target_sync(const Tensor &params, Tensor &target, const OptT &target_h, int64_t precision) {
    const Nets n = nets_of(params, target, target_h);
    c10::hip::HIPGuardMasqueradingAsCUDA g(params.device());
    check(dmdqn_target_sync(n.params, n.target, h16ptr(target_h, "target_h", precision), (int)n.NW,
                            (int)n.P, (int)n.Ph, (int)precision, stream_of(params)),
          "dmdqn_target_sync");
}

void target_soft_update(const Tensor &params, Tensor &target, const OptT &target_h,
                        int64_t precision, double tau, double one_minus_tau) {
    const Nets n = nets_of(params, target, target_h);
    c10::hip::HIPGuardMasqueradingAsCUDA g(params.device());
    check(dmdqn_target_soft_update(n.params, n.target, h16ptr(target_h, "target_h", precision),
                                   (int)n.NW, (int)n.P, (int)n.Ph, (int)precision, (float)tau,
                                   (float)one_minus_tau, stream_of(params)),
          "dmdqn_target_soft_update");
}

// target_soft_update with one tau per net: tau / one_minus_tau f32 [NW].
void target_soft_update_hp(const Tensor &params, Tensor &target, const OptT &target_h,
                           int64_t precision, const Tensor &tau, const Tensor &one_minus_tau) {
    const Nets n = nets_of(params, target, target_h);
    auto ta = dptr<const float>(tau, at::kFloat, "tau", n.NW);
    auto oa = dptr<const float>(one_minus_tau, at::kFloat, "one_minus_tau", n.NW);
    same_device(params, {&tau, &one_minus_tau},
                "tau / one_minus_tau must be on the device of params");
    c10::hip::HIPGuardMasqueradingAsCUDA g(params.device());
    check(dmdqn_target_soft_update_hp(n.params, n.target, h16ptr(target_h, "target_h", precision),
                                      (int)n.NW, (int)n.P, (int)n.Ph, (int)precision, ta, oa,
                                      stream_of(params)),
          "dmdqn_target_soft_update_hp");
}

void q_argmax(const Tensor &params, int64_t hidden, int64_t precision, const Tensor &obs,
              Tensor &out, const OptT &q, bool shared) {
    const int64_t NA = out.numel();
    const int64_t P = shared ? params.numel() : params.numel() / NA;
    auto p = dptr<float>(params, at::kFloat, "params");
    auto o = dptr<float>(obs, at::kFloat, "obs", NA * DMDQN_OBS_DIM);
    auto g = dptr<int32_t>(out, at::kInt, "out", NA);
    auto qq = optr<float>(q, at::kFloat, "q", NA * 4);
    c10::hip::HIPGuardMasqueradingAsCUDA gd(params.device());
    check(shared ? dmdqn_q_argmax_shared(p, (int)NA, (int)P, (int)hidden, (int)precision, o, g, qq,
                                         stream_of(params))
                 : dmdqn_q_argmax(p, (int)NA, (int)P, (int)hidden, (int)precision, o, g, qq,
                                  stream_of(params)),
          "dmdqn_q_argmax");
}

// ---------------------------------------------------------------- population-based training
void pbt_score(const Tensor &reward, Tensor &fitness) {
    const auto [E, A] = dims2(reward, "reward must be [E, A]");
    auto r = dptr<const double>(reward, at::kDouble, "reward");
    auto f = dptr<double>(fitness, at::kDouble, "fitness", E);
    same_device(reward, {&fitness}, "fitness must be on the device of reward");
    c10::hip::HIPGuardMasqueradingAsCUDA g(reward.device());
    check(dmdqn_pbt_score(r, int32_of(E, "E"), int32_of(A, "A"), f, stream_of(reward)),
          "dmdqn_pbt_score");
}

void pbt_select(const Tensor &fitness, int64_t n, Tensor &rank, Tensor &src) {
    const int64_t E = fitness.numel();
    auto f = dptr<const double>(fitness, at::kDouble, "fitness");
    auto r = dptr<int32_t>(rank, at::kInt, "rank", E);
    auto s = dptr<int32_t>(src, at::kInt, "src", E);
    same_device(fitness, {&rank, &src}, "rank / src must be on the device of fitness");
    c10::hip::HIPGuardMasqueradingAsCUDA g(fitness.device());
    check(dmdqn_pbt_select(f, int32_of(E, "E"), int32_of(n, "n"), r, s, stream_of(fitness)),
          "dmdqn_pbt_select");
}

void pbt_exchange(const Tensor &src, int64_t A, Tensor &params, Tensor &target, Tensor &adam_m,
                  Tensor &adam_v, const OptT &target_h) {
    const auto [NA, P] = dims2(params, "params must be [E * A, P]");
    const int64_t E = src.numel();
    TORCH_CHECK(A >= 1 && NA == E * A, "params holds ", NA, " rows, src ", E, " replicas of ", A);
    auto sp = dptr<const int32_t>(src, at::kInt, "src");
    auto p = dptr<float>(params, at::kFloat, "params");
    auto t = dptr<float>(target, at::kFloat, "target", NA * P);
    auto m = dptr<float>(adam_m, at::kFloat, "adam_m", NA * P);
    auto v = dptr<float>(adam_v, at::kFloat, "adam_v", NA * P);
    const int64_t Ph = shadow_stride(target_h, NA, P, "target_h must be [E * A, Ph] with Ph >= P");
    same_device(params, {&target, &adam_m, &adam_v, &src},
                "every tensor must be on the device of params");
    same_device(params, {opt(target_h)}, "target_h must be on the device of params");
    c10::hip::HIPGuardMasqueradingAsCUDA g(params.device());
    check(dmdqn_pbt_exchange(sp, int32_of(E, "E"), int32_of(A, "A"), int32_of(P, "P"),
                             int32_of(Ph, "Ph"), p, t, m, v, h16ptr(target_h, "target_h"),
                             stream_of(params)),
          "dmdqn_pbt_exchange");
}

// ---------------------------------------------------------------- network health probe
// The online forward of every agent's batch reduced to health figures
// (include/dmdqn.h dmdqn_net_probe): counts int32 [NA, 5], stats f64 [NA, 5],
// dead_mask int32 [NA, 2, 4] (the uint32 words as bits) or None.  Reads only.
void net_probe(const Tensor &ring_s, const Tensor &idx, const Tensor &params, int64_t start,
               int64_t hidden, int64_t precision, Tensor &counts, Tensor &stats,
               const OptT &dead_mask) {
    const auto [NA, P] = dims2(params, "params must be [NA, P]");
    TORCH_CHECK(NA > 0 && idx.numel() % NA == 0, "idx must be [NA, batch]");
    const int64_t B = idx.numel() / NA;
    TORCH_CHECK(ring_s.numel() % (NA * DMDQN_ROW_BYTES) == 0 && ring_s.numel() > 0,
                "ring_s must be [NA, cap, ", DMDQN_ROW_BYTES, "]");
    const int64_t cap = ring_s.numel() / (NA * DMDQN_ROW_BYTES);
    dmdqn_probe_args a{};
    a.NA = int32_of(NA, "NA"); a.cap = int32_of(cap, "cap"); a.start = int32_of(start, "start");
    a.batch = int32_of(B, "batch"); a.hidden = int32_of(hidden, "hidden");
    a.precision = int32_of(precision, "precision"); a.P = int32_of(P, "P");
    a.ring_s = dptr<const int8_t>(ring_s, at::kChar, "ring_s");
    a.idx = dptr<const int32_t>(idx, at::kInt, "idx", NA * B);
    a.params = dptr<const float>(params, at::kFloat, "params");
    a.counts = dptr<int32_t>(counts, at::kInt, "counts", NA * DMDQN_PROBE_COUNTS);
    a.stats = dptr<double>(stats, at::kDouble, "stats", NA * DMDQN_PROBE_STATS);
    a.dead_mask = optr<uint32_t>(dead_mask, at::kInt, "dead_mask", NA * 2 * 4);
    same_device(params, {&ring_s, &idx, &counts, &stats},
                "every tensor must be on the device of params");
    same_device(params, {opt(dead_mask)}, "dead_mask must be on the device of params");
    c10::hip::HIPGuardMasqueradingAsCUDA g(params.device());
    check(dmdqn_net_probe(&a, stream_of(params)), "dmdqn_net_probe");
}

// Per-variable sums of squares of x [NW, P] (include/dmdqn.h dmdqn_layer_norms):
// mode 0 of x, mode 1 of x / (sqrt(y) + eps); out f64 [NW, 6] in Keras order.
void layer_norms(const Tensor &x, const OptT &y, double eps, int64_t mode, int64_t hidden,
                 Tensor &out) {
    const auto [NW, P] = dims2(x, "x must be [NW, P]");
    auto xp = dptr<const float>(x, at::kFloat, "x");
    auto yp = optr<const float>(y, at::kFloat, "y", NW * P);
    auto o = dptr<double>(out, at::kDouble, "out", NW * 6);
    same_device(x, {&out, opt(y)}, "every tensor must be on the device of x");
    c10::hip::HIPGuardMasqueradingAsCUDA g(x.device());
    check(dmdqn_layer_norms(xp, yp, (float)eps, int32_of(mode, "mode"), int32_of(NW, "NW"),
                            int32_of(P, "P"), int32_of(hidden, "hidden"), o, stream_of(x)),
          "dmdqn_layer_norms");
}

// ---------------------------------------------------------------- dead-unit recycling
// ReDo on the probe's dead mask (include/dmdqn.h dmdqn_redo): streak uint8
// [NA, 2, 128], recycled int32 [NA, 2, 4] (the uint32 words as bits), n_recycled
// int32 [NA, 2].  Writes streak, params, adam_m, adam_v and the two outputs.
void redo(const Tensor &dead_mask, Tensor &streak, Tensor &params, Tensor &adam_m, Tensor &adam_v,
          int64_t hidden, int64_t agent0, int64_t seed, int64_t round, int64_t patience,
          double lim1, double lim2, Tensor &recycled, Tensor &n_recycled) {
    const auto [NA, P] = dims2(params, "params must be [NA, P]");
    TORCH_CHECK(NA > 0, "params must be [NA, P] with NA > 0");
    TORCH_CHECK(round >= 0 && round <= (int64_t)UINT32_MAX, "round out of uint32 range");
    dmdqn_redo_args a{};
    a.NA = int32_of(NA, "NA"); a.P = int32_of(P, "P"); a.hidden = int32_of(hidden, "hidden");
    a.agent0 = int32_of(agent0, "agent0"); a.patience = int32_of(patience, "patience");
    a.round = (uint32_t)round; a.seed = (uint64_t)seed;
    a.lim1 = (float)lim1; a.lim2 = (float)lim2;
    a.dead_mask = dptr<const uint32_t>(dead_mask, at::kInt, "dead_mask", NA * 2 * 4);
    a.streak = dptr<uint8_t>(streak, at::kByte, "streak", NA * 2 * hidden);
    a.params = dptr<float>(params, at::kFloat, "params");
    a.adam_m = dptr<float>(adam_m, at::kFloat, "adam_m", NA * P);
    a.adam_v = dptr<float>(adam_v, at::kFloat, "adam_v", NA * P);
    a.recycled = dptr<uint32_t>(recycled, at::kInt, "recycled", NA * 2 * 4);
    a.n_recycled = dptr<int32_t>(n_recycled, at::kInt, "n_recycled", NA * 2);
    same_device(params, {&dead_mask, &streak, &adam_m, &adam_v, &recycled, &n_recycled},
                "every tensor must be on the device of params");
    c10::hip::HIPGuardMasqueradingAsCUDA g(params.device());
    check(dmdqn_redo(&a, stream_of(params)), "dmdqn_redo");
}

// ---------------------------------------------------------------- rule-based controllers
// Longest-queue / max-pressure actions from the observations (include/dmdqn.h
// dmdqn_act_rule): obs f32 [E, R*C, 89], actions int32 [E*R*C] (any shape),
// score int32 [E*R*C, 4] or None.  The grid, E and the rule are refused by the
// C entry point (its message is raised), before any launch.
void act_rule(const Tensor &obs, int64_t R, int64_t C, int64_t rule, Tensor &actions,
              const OptT &score) {
    TORCH_CHECK(obs.dim() == 3 && obs.size(2) == DMDQN_OBS_DIM, "obs must be [E, R*C, 89]");
    const int64_t E = obs.size(0), A = obs.size(1);
    TORCH_CHECK(R < 1 || C < 1 || A == R * C, "obs must be [E, R*C, 89]: ", A, " agents for a ", R,
                "x", C, " grid");
    auto o = dptr<const float>(obs, at::kFloat, "obs");
    auto a = dptr<int32_t>(actions, at::kInt, "actions", E * A);
    auto sc = optr<int32_t>(score, at::kInt, "score", E * A * 4);
    same_device(obs, {&actions, opt(score)}, "every tensor must be on the device of obs");
    c10::hip::HIPGuardMasqueradingAsCUDA g(obs.device());
    check(dmdqn_act_rule(int32_of(R, "R"), int32_of(C, "C"), int32_of(E, "E"),
                         int32_of(rule, "rule"), o, a, sc, stream_of(obs)),
          "dmdqn_act_rule");
}

}  // namespace

// The tree digest this operator library was built from (build.py passes it as
// a define; ops.load() compares it with the tree, like libdmdqn_hip.so's).
extern "C" const char *dmdqn_torch_source_digest(void) { return DMDQN_SOURCE_DIGEST; }

// Schemas: each op cites the reference call it replaces (include/dmdqn.h has
// the argument meanings).
TORCH_LIBRARY(dmdqn, m) {
    // random.seed / np.random.seed of the per-replica streams (dqn_agent.py:63, :263-265)
    m.def("mt_seed(Tensor(a!) state, Tensor seeds, str kind) -> ()");
    m.def("mt_draw_u32(Tensor(a!) state, int count, Tensor(b!) out) -> ()");
    // DQNAgent.select_action (dqn_agent.py:246-274)
    // (uniform: test.py:92-93's randint-only draw)
    m.def("act(Tensor(a!) np_state, int A, float eps, int n_actions, Tensor? greedy, "
          "Tensor(b!) actions, bool uniform=False) -> ()");
    // get_own_state / build_state_vector / rewards (order_lanes.py:430-555, train.py:159-165,254)
    m.def("observe(int R, int C, Tensor halt, Tensor phase, Tensor tspent, int mode, "
          "Tensor(a!)? local, Tensor(b!)? obs, Tensor? prev_local, Tensor(c!)? reward) -> ()");
    // ReplayBuffer.add (dqn_agent.py:31-57)
    m.def("replay_store(int slot, Tensor obs_s, Tensor obs_n, Tensor act, Tensor rew, Tensor done, "
          "Tensor(a!) ring_s, Tensor(b!) ring_n, Tensor(c!) ring_a, Tensor(d!) ring_r, "
          "Tensor(e!) ring_d, Tensor(f!) err) -> ()");
    // random.sample(self.buffer, k) (dqn_agent.py:63)
    m.def("replay_sample(Tensor(a!) py_state, int A, int n, int k, Tensor(b!) idx, "
          "int lds_budget=0) -> ()");
    // ReplayBuffer.add / .sample on float rows (the per-agent drop-in, dqn_agent.py:39-64)
    m.def("replay_store_f32(int slot, Tensor obs_s, Tensor obs_n, Tensor act, Tensor rew, "
          "Tensor done, Tensor(a!) rows_s, Tensor(b!) rows_n, Tensor(c!) ring_a, Tensor(d!) ring_r, "
          "Tensor(e!) ring_d) -> ()");
    m.def("replay_gather_f32(Tensor rows_s, Tensor rows_n, Tensor idx, int start, Tensor(a!) xs, "
          "Tensor(b!) xn) -> ()");
    // n-step returns built at the replay store (docs/improvements.md item 7; the reference
    // stores one-step transitions, dqn_agent.py:31-57, for the target of :347)
    m.def("replay_nstep_commit(int head, int slot, Tensor st_s, Tensor st_n, Tensor st_a, "
          "Tensor st_r, Tensor st_d, Tensor(a!) ring_s, Tensor(b!) ring_n, Tensor(c!) ring_a, "
          "Tensor(d!) ring_r, Tensor(e!) ring_d, float gamma, Tensor? gamma_a=None) -> ()");
    // traci.load (train.py:190); setPhase x A + simulationStep x K (train.py:225-236)
    m.def("sim_reset(Tensor(a!)[] state, Tensor[] tables, int[] dims, Tensor? mask=None) -> ()");
    m.def("sim_step(Tensor(a!)[] state, Tensor[] tables, int[] dims, float[] idm, Tensor? actions, "
          "int stride, int t0, int K, int max_time, Tensor(b!) halt, Tensor(c!) phase, "
          "Tensor(d!) tspent, Tensor(e!) done) -> ()");
    // the env side of one loop iteration in one launch: select_action, setPhase + K
    // substeps, observation / reward, ReplayBuffer.add (train.py:211-282)
    m.def("env_step(Tensor(a!)[] state, Tensor[] tables, int[] dims, float[] idm, int stride, "
          "int t0, int K, int max_time, Tensor(b!) halt, Tensor(c!) phase, Tensor(d!) tspent, "
          "Tensor(e!) done, Tensor(f!) np_state, Tensor? greedy, Tensor(g!) actions, float eps, "
          "int n_actions, int mode, Tensor(h!) local, Tensor(i!) obs, Tensor prev_local, "
          "Tensor(j!) reward, Tensor obs_s, int slot, Tensor(k!) ring_s, Tensor(l!) ring_n, "
          "Tensor(m!) ring_a, Tensor(n!) ring_r, Tensor(o!) ring_d, Tensor(p!) err) -> ()");
    // DQNAgent.learn + the target sync (dqn_agent.py:328-387)
    m.def("learn_step(Tensor ring_s, Tensor ring_n, Tensor ring_a, Tensor ring_d, Tensor ring_r, "
          "Tensor idx, Tensor(a!) params, Tensor(b!) adam_m, Tensor(c!) adam_v, Tensor(d!) target, "
          "Tensor(e!)? target_h, Tensor(f!) loss, int start, int hidden, int precision, bool sync, "
          "float gamma, float alpha, float c1, float c2, float eps, int loss_kind, "
          "Tensor(g!)? qstats, Tensor(h!)? rn_out, Tensor(i!)? stamps, Tensor(j!)? grad=None, "
          "Tensor? xs=None, Tensor? xn=None, float tau=0.0, float one_minus_tau=1.0) -> ()");
    // DQNAgent.learn with per-agent learning_rate / gamma / tau (dqn_agent.py:112-113, :140,
    // :347, :389-399: one config for every agent there, one value per agent here)
    m.def("learn_step_hp(Tensor ring_s, Tensor ring_n, Tensor ring_a, Tensor ring_d, Tensor ring_r, "
          "Tensor idx, Tensor(a!) params, Tensor(b!) adam_m, Tensor(c!) adam_v, Tensor(d!) target, "
          "Tensor(e!)? target_h, Tensor(f!) loss, int start, int hidden, int precision, bool sync, "
          "float gamma, float alpha, float c1, float c2, float eps, int loss_kind, "
          "Tensor(g!)? qstats, Tensor(h!)? rn_out, Tensor(i!)? stamps, Tensor(j!)? grad=None, "
          "Tensor? xs=None, Tensor? xn=None, float tau=0.0, float one_minus_tau=1.0, "
          "Tensor? lr=None, Tensor? gamma_a=None, Tensor? tau_a=None, "
          "Tensor? one_minus_tau_a=None, float adam_s=1.0, float adam_d=1.0) -> ()");
    // learn_step_hp as the split learn with Keras's global_clipnorm on each agent's gradient
    // (tf.keras.optimizers.Adam(global_clipnorm=...), one keyword at dqn_agent.py:140)
    m.def("learn_step_clip(Tensor ring_s, Tensor ring_n, Tensor ring_a, Tensor ring_d, "
          "Tensor ring_r, Tensor idx, Tensor(a!) params, Tensor(b!) adam_m, Tensor(c!) adam_v, "
          "Tensor(d!) target, Tensor(e!)? target_h, Tensor(f!) loss, int start, int hidden, "
          "int precision, bool sync, float gamma, float alpha, float c1, float c2, float eps, "
          "int loss_kind, Tensor(g!)? qstats, Tensor(h!)? rn_out, Tensor(i!)? stamps, "
          "Tensor(j!) grad, Tensor? xs=None, Tensor? xn=None, float tau=0.0, "
          "float one_minus_tau=1.0, Tensor? lr=None, Tensor? gamma_a=None, Tensor? tau_a=None, "
          "Tensor? one_minus_tau_a=None, float adam_s=1.0, float adam_d=1.0, *, float clip, "
          "Tensor(k!)? gnorm=None) -> ()");
    // two consecutive DQNAgent.learn calls of every agent in one launch (dmdqn_learn_pair)
    m.def("learn_pair(Tensor ring_s, Tensor ring_n, Tensor ring_a, Tensor ring_d, Tensor ring_r, "
          "Tensor(a!) params, Tensor(b!) adam_m, Tensor(c!) adam_v, Tensor(d!) target, "
          "Tensor(e!) target_h, Tensor idx0, Tensor idx1, Tensor(f!) loss0, Tensor(g!) loss1, "
          "int start0, int start1, int hidden, int precision, float gamma, float[] adam0, "
          "float[] adam1, int loss_kind, Tensor(h!)? qstats0=None, Tensor(i!)? qstats1=None, "
          "Tensor(j!)? rn_out0=None, Tensor(k!)? rn_out1=None, float tau=0.0, "
          "float one_minus_tau=1.0, Tensor? lr=None, Tensor? gamma_a=None, Tensor? tau_a=None, "
          "Tensor? one_minus_tau_a=None, float[] factors0=[1.0, 1.0], "
          "float[] factors1=[1.0, 1.0]) -> ()");
    // C5: per-agent gradients of one shared net, summed
    m.def("learn_shared_grad(Tensor ring_s, Tensor ring_n, Tensor ring_a, Tensor ring_d, "
          "Tensor ring_r, Tensor idx, Tensor params, Tensor target, Tensor target_h, "
          "Tensor params_h, Tensor(a!) loss, int start, float gamma, int loss_kind, "
          "Tensor(b!)? qstats, Tensor(c!)? rn_out, Tensor(d!) slab, Tensor(e!)? grad, "
          "float scale, Tensor(f!)? work=None) -> ()");
    // C5, one rank: the slab reduction and the Keras-3 Adam step in one launch
    m.def("adam_slabs(Tensor(a!) params, Tensor(b!) adam_m, Tensor(c!) adam_v, Tensor(d!) target, "
          "Tensor(e!)? target_h, Tensor(f!)? params_h, Tensor slab, Tensor(g!) grad, float scale, "
          "float gscale, float alpha, float c1, float c2, float eps, bool sync) -> ()");
    // Keras-3 Adam (dqn_agent.py:357, A-11) on a flat gradient
    m.def("adam(Tensor(a!) params, Tensor(b!) adam_m, Tensor(c!) adam_v, Tensor(d!) target, "
          "Tensor(e!)? target_h, Tensor(f!)? params_h, Tensor grad, float gscale, float alpha, "
          "float c1, float c2, float eps, bool sync) -> ()");
    // DQNAgent.update_target_network (dqn_agent.py:382-387)
    m.def("target_sync(Tensor params, Tensor(a!) target, Tensor(b!)? target_h, int precision) -> ()");
    // DQNAgent.update_target_network_soft (dqn_agent.py:372-373, 389-399)
    m.def("target_soft_update(Tensor params, Tensor(a!) target, Tensor(b!)? target_h, "
          "int precision, float tau, float one_minus_tau) -> ()");
    // update_target_network_soft with one tau per net
    m.def("target_soft_update_hp(Tensor params, Tensor(a!) target, Tensor(b!)? target_h, "
          "int precision, Tensor tau, Tensor one_minus_tau) -> ()");
    // the greedy branch of select_action (dqn_agent.py:268-273)
    m.def("q_argmax(Tensor params, int hidden, int precision, Tensor obs, Tensor(a!) out, "
          "Tensor(b!)? q, bool shared) -> ()");
    // population-based training across the replicas (nothing in the reference)
    m.def("pbt_score(Tensor reward, Tensor(a!) fitness) -> ()");
    m.def("pbt_select(Tensor fitness, int n, Tensor(a!) rank, Tensor(b!) src) -> ()");
    m.def("pbt_exchange(Tensor src, int A, Tensor(a!) params, Tensor(b!) target, "
          "Tensor(c!) adam_m, Tensor(d!) adam_v, Tensor(e!)? target_h) -> ()");
    // the network health probe (docs/improvements.md item 2, "Tensorboard activation checks";
    // nothing in the reference's code computes it)
    m.def("net_probe(Tensor ring_s, Tensor idx, Tensor params, int start, int hidden, "
          "int precision, Tensor(a!) counts, Tensor(b!) stats, Tensor(c!)? dead_mask=None) -> ()");
    m.def("layer_norms(Tensor x, Tensor? y, float eps, int mode, int hidden, "
          "Tensor(a!) out) -> ()");
    // dead-unit recycling on the probe's dead mask (ReDo; docs/improvements.md item 3,
    // "improve weight inits"; nothing in the reference's code does it)
    m.def("redo(Tensor dead_mask, Tensor(a!) streak, Tensor(b!) params, Tensor(c!) adam_m, "
          "Tensor(d!) adam_v, int hidden, int agent0, int seed, int round, int patience, "
          "float lim1, float lim2, Tensor(e!) recycled, Tensor(f!) n_recycled) -> ()");
    // rule-based controllers in dmdqn_act's greedy format (longest queue, max pressure;
    // nothing in the reference's code has them)
    m.def("act_rule(Tensor obs, int R, int C, int rule, Tensor(a!) actions, "
          "Tensor(b!)? score) -> ()");
}

// Every operator, once: both dispatch keys below are filled from this list, so
// an operator cannot have one kernel and not the other.
#define DMDQN_OPS(X)                                                                              \
    X(mt_seed) X(mt_draw_u32) X(act) X(observe) X(replay_store) X(replay_sample)                  \
    X(replay_store_f32) X(replay_gather_f32) X(replay_nstep_commit) X(sim_reset) X(sim_step)      \
    X(env_step) X(learn_step) X(learn_step_hp) X(learn_step_clip) X(learn_pair)                   \
    X(learn_shared_grad) X(adam) X(adam_slabs) X(target_sync) X(target_soft_update)               \
    X(target_soft_update_hp) X(q_argmax) X(pbt_score) X(pbt_select) X(pbt_exchange) X(net_probe)  \
    X(layer_norms) X(redo) X(act_rule)

TORCH_LIBRARY_IMPL(dmdqn, CUDA, m) {
#define X(op) m.impl(#op, &op);
    DMDQN_OPS(X)
#undef X
}

// Meta kernels: the ops only mutate their (a!) arguments, so tracing needs no
// shape function beyond "nothing is returned" -- the implementation's own
// signature with an empty body.
template <typename F> struct NoLaunch;
template <typename... A> struct NoLaunch<void(A...)> {
    static void run(A...) {}
};

TORCH_LIBRARY_IMPL(dmdqn, Meta, m) {
#define X(op) m.impl(#op, &NoLaunch<decltype(op)>::run);
    DMDQN_OPS(X)
#undef X
}
