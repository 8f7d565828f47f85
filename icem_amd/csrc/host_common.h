// host_common.h -- what the host-side translation units of libicem_hip.so share: the handle, error plumbing,
// per-kernel timing scopes, the launcher interfaces between them, and what the batched steps share (arg_array.h, admit_batch,
// results_row, call_base / shift_rows / elite_parity; their blobs' sections are block_layout.h's, the recorded-launch plan of
// plan.hip, cem_step.hip and random_step.hip is recorded_batch.h's).
//   generic_kernels.hip  the generic (f32 / f64, any shape) kernels + their launchers (gk_*)
//   plan.hip             the fused MPC step: icem_plan_* / icem_get_action and the f32 throughput-path orchestration
//   learned_step.hip     the learned-dynamics MPC step: icem_plan_step_learned*
//   cem_step.hip         the CEM baseline's MPC step: icem_plan_step_cem, icem_plan_step_cem_batch
//   random_step.hip      the random-shooting baseline's MPC step: icem_plan_step_random, icem_plan_step_random_batch
//   exchange.hip        the in-library elite exchange between GPUs (icem_exchange_*)
//   abi.hip              handle life cycle and the stateless operators of include/icem_hip.h
// Internal; not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <atomic>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/icem_hip.h"
#include "arg_array.h"
#include "icem_fused.h"
#include "options.h"

namespace icem {

inline thread_local std::string g_err;

inline int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

#define ICEM_HIP_TRY(expr)                                                                      \
    do {                                                                                        \
        hipError_t e_ = (expr);                                                                 \
        if (e_ != hipSuccess)                                                                   \
            return ::icem::fail(ICEM_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

constexpr int WG = 256;          // 4 wavefronts of 64
constexpr int TOPK_CHUNK = 1024; // costs per workgroup in the block-level top-k

struct Exchange;  // exchange.hip

// icem_plan_step_learned* (learned_step.hip): what the step keeps with its FIRST handle
struct LearnedCtx {
    // argument arrays by the first handle's step parity: the elite halves alternate per iteration.  Each has room for the
    // largest batch: a batch that grows later allocates nothing
    DeviceArgArray<2> args;
    float* pool = nullptr;                   // a batch's [rows, hd] actions | [rows] costs | [n, 230] observations
    size_t pool_rows = 0;
    int pool_n = 0;
    int* idx = nullptr;                      // [ICEM_MAX_BATCH, ICEM_MAX_ELITES]: the updates' index output (not kept)
    long long launches = 0;                  // kernel launches of the last learned step this handle led
    long long mlp_launches = 0;              // ... and of the last icem_plan_step_mlp
    // the pool of a batch of n problems with cap_rows rows in all (icem_plan_step_learned_batch, icem_plan_step_cem_learned_batch:
    // both lay it out as above); it only grows, behind a synchronisation of `st` (an earlier step's launches may still use the old one)
    hipError_t reserve(size_t cap_rows, int n, int hd, hipStream_t st) {
        if (pool_rows >= cap_rows && pool_n >= n) return hipSuccess;
        const size_t rws = std::max(cap_rows, pool_rows);
        const int pn = std::max(n, pool_n);
        if (pool) {
            if (hipError_t e = hipStreamSynchronize(st)) return e;
            (void)hipFree(pool);
            pool = nullptr;
            pool_rows = 0;
        }
        if (hipError_t e = hipMalloc((void**)&pool, (rws * (size_t)(hd + 1) + (size_t)pn * ICEM_RSSM_OBS_DIM) * sizeof(float))) return e;
        pool_rows = rws;
        pool_n = pn;
        return hipSuccess;
    }
    // the pool's parts as reserve() laid them out (nullptr: no pool yet -- one problem alone needs none)
    float* pool_actions() const { return pool; }
    float* pool_costs(int hd) const { return pool ? pool + pool_rows * (size_t)hd : nullptr; }
    float* pool_obs(int hd) const { return pool ? pool + pool_rows * (size_t)(hd + 1) : nullptr; }
    // icem_plan_step_learned_models whose caller brought no member_costs: [members, rows] of one iteration; grows like the pool
    float* member_costs = nullptr;
    size_t member_cap = 0;
    hipError_t reserve_members(size_t floats, hipStream_t st) {
        if (member_cap >= floats) return hipSuccess;
        if (member_costs) {
            if (hipError_t e = hipStreamSynchronize(st)) return e;
            (void)hipFree(member_costs);
            member_costs = nullptr;
            member_cap = 0;
        }
        if (hipError_t e = hipMalloc((void**)&member_costs, floats * sizeof(float))) return e;
        member_cap = floats;
        return hipSuccess;
    }
    ~LearnedCtx() {
        if (pool) (void)hipFree(pool);
        if (idx) (void)hipFree(idx);
        if (member_costs) (void)hipFree(member_costs);
    }
};

// icem_plan_step_random* (random_step.hip): device words of the selection launch, zeroed once (the launch leaves them zero)
struct RandomWs {
    void* dev = nullptr;
    size_t bytes = 0;
    RandomWs() = default;
    RandomWs(const RandomWs&) = delete;
    RandomWs& operator=(const RandomWs&) = delete;
    ~RandomWs() {
        if (dev) (void)hipFree(dev);
    }
};

}  // namespace icem

struct icem_handle {
    icem_config cfg;
    int F = 0, HMAX = 0, hd = 0;
    size_t tsize = 4;
    void* W_dev = nullptr;
    int model_kind = 0, obs_dim = 0, O = 0;
    void* A_dev = nullptr;
    void* B_dev = nullptr;
    bool has_model = false, has_cost = false;
    icem_cost_spec cost;
    icem_cost_terms terms;
    bool has_terms = false;  // any term of icem_cost_terms switched on
    void* host_stage = nullptr;  // pinned, device-mapped block of icem_get_action [obs | action, best cost | flag]
    void* host_stage_dev = nullptr;
    unsigned io_seq = 0;
    std::vector<int> pop;
    int n_reuse = 0;
    int n_local_max = 0;
    int rssm_act = 0;   // icem_set_rssm_act_dim: the action width of the RSSM the learned-dynamics steps roll out through (0: never bound)
    // optional per-kernel timing with HIP events on the caller's stream (bench.py roofline leg)
    bool profiling = false;
    struct Span {
        int kind;
        long long units;
        hipEvent_t a, b;
    };
    bool use_fast = true;
    long long* dbg = nullptr;
    // what the local launch of an iteration tells its merge (icem_plan_iter_local and icem_plan_iter_merge are separate calls)
    struct LocalReport {
        int lists = 0;      // candidate lists written by the last matrix-pipe rollout (0 = generic path ran)
        int tail_rows = 0;  // ... and shifted-elite rows behind them that the merge scores through the cost array
        // generic path, world == 1: the iteration's selection waits for the merge call (gk_select_refit: one launch for top-K +
        // gather + refit); sel_cand > 0 = rows with a cost in b->costs, sel_loc of them sampled rows
        int sel_cand = 0, sel_loc = 0;
        void clear() { *this = LocalReport(); }
    } local;
    // icem_plan_step (world == 1): an iteration's merge can ride in the prologue of the next iteration's launch,
    // which then reads the previous pool / lists / distribution while writing new ones -> ping-pong partners of
    // the caller's actions / workspace buffers and of mean | std, owned by the handle
    void* actions_alt = nullptr;
    void* ws_alt = nullptr;
    float* pp_stats = nullptr;          // [2][2 * hd]
    // what rides into the next launch
    struct Riding {
        bool merge_pending = false;     // a stashed merge waits for the next local launch
        icem::MergeSingleArgs merge;
        // sharded runs with merge deferral: an iteration's record pack + push can ride in the NEXT local launch too
        // (workgroup 0 of sample_rollout_kernel) instead of being a launch of its own
        bool pack_pending = false;
        icem::PackPrev pack;
        void clear() { merge_pending = pack_pending = false; }
    } ride;
    // world > 1 with icem_set_merge_deferral(on): the same folding across the split calls; the distribution of the
    // running MPC step lives at cur_mean / cur_std (the caller's buffers or pp_stats)
    bool deferral = false;
    float* cur_mean = nullptr;
    float* cur_std = nullptr;
    // permuted, padded model of the matrix-pipe rollout: column 0 = obs[lin_idx], column 1 = obs[flip_idx]
    bool wide = false;           // obs_dim > 32: the rollout is k_rollout_wide.hip's GEMM kernel (f32 only)
    int Of = 0;                  // O of the 16-trajectory tile kernels (Tile16 / Tile4), or 0 where they do not serve this handle's
                                 // model + cost (wide observations; icem_cost_terms; a cost without its linear term; a shape
                                 // (h, d, O) that is not compiled): the f32 rollout is then the GEMM kernel at ANY width.
                                 // Kept current by update_paths() (abi.hip) behind every model / cost setter.
    // arithmetic of the tile kernels' model step (icem_set_tile_arith): mode -1 = by configuration, 0 = exact f32, 1 = fp16 planes;
    // tile_arith = what the handle's launches use (update_paths: mode + whether Tile16H serves this model)
    int tile_arith_mode = -1;
    int tile_arith = 0;
    int hn_prog[3] = {0, 0, 0};  // ... its term program (N32, N4, NP) and the device copy of the terms sorted into it
    void* hn_cs_dev = nullptr;
    bool hn_tile = false;        // the f32 rollout is k_rollout_hn.hip's TileHN kernel (Door / Relocate / FetchPickAndPlace shapes; fp16 planes)
    float tile_m_scale = 1.f, tile_b_scale = 1.f;   // FastRolloutArgs::m_scale / b_scale (update_paths)
    float tile_inv_m_scale = 1.f, tile_inv_b_scale = 1.f;   // ... and inv_m_scale / inv_b_scale: their exact reciprocals
    float act_mag = 1.f;         // max(|low|, |high|) of the action bounds last seen (FastRolloutArgs::act_mag), from ...
    const void* am_lo = nullptr; // ... this (low, high) buffer pair (refreshed by icem_reset_distribution and the plan calls)
    const void* am_hi = nullptr;
    // fp16-plane tiles (Tile16H / TileHN): served only where no state can leave fp16's range inside the horizon
    double tile_growth = 1.0;    // worst case of |state entry| / max(|obs0|, action bound) over the horizon (update_paths; 1 for tanh)
    int tile_ratio_log2 = 0;     // log2(largest |B entry| / largest |A entry|) (the action operand's scale relative to the state's)
    // trajectories whose cost left a tile kernel non-finite (FastRolloutArgs::nonfinite): a device word, and the value
    // icem_get_action saw at its last call
    unsigned* nonfinite_dev = nullptr;
    unsigned nonfinite_seen = 0;
    void* Mw_dev = nullptr;      // its packed model
    void* Mws_dev = nullptr;     // ... as three bf16 planes (k_rollout_wide_split.hip) ...
    void* Mwh_dev = nullptr;     // ... and as two fp16 planes of the model x 2^k, Mwh_inv = 2^-k: the default wide rollout
    float Mwh_inv = 1.f;
    void* Mwh_ksc_dev = nullptr; // ... and the contraction entries' and output columns' powers of two (the model equilibrated): [Mwh_nk | columns]
    int Mwh_nk = 0;
    float Mwh_sbound = 0.f;
    int wide_mode = -1;          // icem_set_wide_arith: ICEM_WIDE_AUTO (-1) / F16X2 (0) / F32 (1) / BF16X3 (2) as asked for ...
    int wide_eff = 0;            // ... and the one in effect (update_paths: AUTO = fp16 planes unless the balanced model is not)
    int wide_imbalance = 0;      // wide_model_imbalance_log2 of the current model
    int wide_packed = -2;        // which arithmetic Mw_dev / Mwh_dev / Mws_dev currently hold the model for (-2: none)
                                 // (k_rollout_wide.hip + its row kernel), 2 = bf16 planes (6 products)
    void* wide_cs_dev = nullptr; // CostArgs<float> (cost spec + terms) for k_rollout_wide, refreshed by the cost setters
    // float64 handles (icem_set_f64_arith): ICEM_F64_CHAIN = the generic kernels' fma chain (o <= 32), ICEM_F64_MFMA = the f64
    // matrix-core rollout of k_rollout_f64.hip (o <= 384).  `wide` above stays "the f32 GEMM path": an f64 handle wider than
    // 32 has wide == false, O == 0 and its model only in M64_dev
    int f64_arith = 0;
    void* M64_dev = nullptr;     // [A ; B] as f64, row-major, zero-padded to [ceil4(o + d)][ceil16(o)] (abi.hip: sync_f64_mfma)
    bool f64_model_ready = false;   // M64_dev holds the current model
    void* f64_cs_dev = nullptr;  // CostArgs<double> (cost spec + terms) of k_rollout_f64.hip, refreshed by every setter
    void* Mp_dev = nullptr;
    void* perm_dev = nullptr;
    int flip_col = -1;
    bool fast_model_ready = false;
    std::vector<double> A_host, B_host;
    std::vector<Span> spans;
    std::vector<hipEvent_t> free_events;
    icem::Exchange* xchg = nullptr;  // in-library elite exchange (icem_exchange_*), world > 1
    icem::XchgWait xw_last;          // ... and what the merge of the running iteration waits for (set by the push)
    uint64_t episode = 0;            // folded into the noise stream offset (icem_set_episode)
    float* pub_dev = nullptr;        // published merge (PackPrev::pub): [2 * hd] floats, then the flag word
    unsigned pub_seq = 0;
    // noise-ahead pipeline (plan.hip::plan_step_ahead; world == 1, large populations): every iteration's launch
    // also draws the raw noise of the NEXT sampling call into the next pool.  Non-last iterations rotate through three
    // pools owned by the handle (a pool is rewritten by the noise role two launches after the merge that read it).
    struct Ahead {
        void* pool[3] = {nullptr, nullptr, nullptr};
        unsigned long long ctr = 0;          // non-last iterations so far: pool of (step, it) = pool[(ctr + it) % 3]
        // the noise drawn ahead for iteration 0 of the next MPC step
        bool next_valid = false;
        uint64_t next_episode = 0;
        int next_step = -1;
        void* next_pool = nullptr;
        hipStream_t next_stream = nullptr;   // the stream that noise was enqueued on: consumed only by a step on the SAME stream
        // host copy of the action bounds (the transform takes them as scalars: equal in every dimension or no pipeline)
        const void* lo_ptr = nullptr;
        const void* hi_ptr = nullptr;
        bool uniform = false;
        float lo = 0.f, hi = 0.f;
        // part of that noise rides beside the step's LAST merge (the one launch that leaves the chip idle)
        bool tail_pending = false;
        icem::FastSampleArgs tail_args, tail2_args;   // tail2 (n > 0): the next step's shifted elites' noise as well
        // ... and the head of the next step's iteration-1 noise (rows [0, next1_rows) of next1_pool): iteration 0's launch has
        // no merge prologue for its noise role to hide behind, its noise role outlasts its rollout (EXPERIMENTS R5.2)
        int next1_rows = 0;
        void* next1_pool = nullptr;
        // small populations (single-launch kernel): the whole first noise of the next MPC step is drawn beside the last
        // merge into `pre_raw` [pop[0] + n_reuse, h, d]; iteration 0 of that step only maps it (FastSampleArgs::raw_src)
        void* pre_raw = nullptr;
        bool pre_valid = false;
        uint64_t pre_episode = 0;
        int pre_step = -1;
        hipStream_t pre_stream = nullptr;    // (as next_stream)
        int disabled = -1;                   // ICEM_NOISE_AHEAD (latched at first use)
        int min_rows = 0;                    // ICEM_NOISE_AHEAD_MIN_ROWS
    } ahead;
    // icem_plan_step_batch (plan.hip): the device arrays of the batch's argument blocks live with the batch's FIRST handle.
    // Six, by the MPC step modulo 6: the elite buffers ping-pong per ITERATION (with an odd iteration count every second
    // step's blocks are the same again), the noise-ahead launches rotate three pools per step: 2 x 3 steps close every cycle
    icem::DeviceArgArray<6> batch_args;
    unsigned long long batch_uploads = 0;   // how often a batched step of either kind (re)wrote its array (steady state: never)
    long long batch_f64_launches = 0;       // kernel launches of the last icem_plan_step_batch_f64 this handle led
    icem::LearnedCtx learned;               // icem_plan_step_learned* (learned_step.hip)
    long long cem_launches = 0;             // kernel launches of the last icem_plan_step_cem / _cem_learned of this handle (cem_step.hip)
    // icem_plan_step_cem_batch / _cem_learned_batch (cem_step.hip): the batch's argument blocks live with its FIRST handle, by that handle's step parity
    // (the blocks carry no step-dependent value: either slot of a batch whose buffers stay put is uploaded once)
    icem::DeviceArgArray<2> cem_batch_args;
    long long cem_batch_launches = 0;       // kernel launches of the last icem_plan_step_cem_batch this handle led
    // icem_plan_step_random / _random_batch (random_step.hip): the selection's per-workgroup partials + ticket of THIS handle's
    // problem (pools of more than one slice), the batch's argument blocks with its FIRST handle (no step-dependent value in them)
    icem::RandomWs random_ws;
    icem::DeviceArgArray<1> random_batch_args;
    long long random_launches = 0;          // kernel launches of the last icem_plan_step_random of this handle
    long long random_batch_launches = 0;    // kernel launches of the last icem_plan_step_random_batch this handle led
    void* rccl_comm = nullptr;       // collective.hip: the RCCL communicator of icem_allgather_elites (world > 1)
    bool rccl_owned = false;         // ... created by icem_rccl_connect (destroyed with the handle) or adopted
};

namespace icem {

struct ProfScope {
    icem_handle* h;
    hipStream_t st;
    hipEvent_t a = nullptr, b = nullptr;
    int kind;
    long long units;
    static hipEvent_t get(icem_handle* h) {
        if (!h->free_events.empty()) {
            hipEvent_t e = h->free_events.back();
            h->free_events.pop_back();
            return e;
        }
        hipEvent_t e = nullptr;
        (void)hipEventCreate(&e);
        return e;
    }
    ProfScope(const icem_handle* hc, int kind_, long long units_, hipStream_t st_)
        : h(const_cast<icem_handle*>(hc)), st(st_), kind(kind_), units(units_) {
        if (!h->profiling) return;
        a = get(h);
        b = get(h);
        (void)hipEventRecord(a, st);
    }
    ~ProfScope() {
        if (!a) return;
        (void)hipEventRecord(b, st);
        h->spans.push_back({kind, units, a, b});
    }
};

inline int shard_chunk(int n_global, int world) { return (n_global + world - 1) / world; }

// ---- rules that every path of a step must agree on (a controller may alternate icem_plan_step* and _learned*), each written once ----

// Noise stream offset of an MPC step's sampling calls: episode in the high word (icem_set_episode; the reference's
// np.random stream runs on across episodes, icem.py:73), sampling call number of the episode in the low one --
// iteration `it` draws at call_base + it, the shifted elites at call_base + opt_iters.
inline uint64_t call_base(const icem_handle* h, int mpc_step) {
    return (h->episode << 32) + (uint64_t)mpc_step * (uint64_t)(h->cfg.opt_iters + 1);
}

// shifted elites, simulated at iteration 0 of every MPC step but the first (icem.py:131-137): rows behind the sampled ones.
// (icem_create does not refuse a negative fraction_reused, which makes n_reuse negative: the launches then build no such
// rows, while the lists merge's pool size and the batch's dry run have always taken the count as it is -- at_least_0 = false.)
inline int shift_rows(const icem_handle* h, int mpc_step, int it, bool at_least_0 = true) {
    if (it != 0 || !h->cfg.shift_elites || mpc_step <= 0) return 0;
    return at_least_0 ? std::max(0, h->n_reuse) : h->n_reuse;
}

// which of the two elite buffers iteration `it` of step `mpc_step` reads (it writes the other): the global iteration's parity
inline int elite_parity(const icem_handle* h, int mpc_step, int it) { return (int)(((long long)mpc_step * h->cfg.opt_iters + it) & 1); }

// Do two handles share the configuration a batched step needs?  Every launch shape and template instantiation of a batch is
// shared, so everything that decides one is compared (the populations and n_reuse are functions of these fields); seeds differ.
// exact: the learned step also reads the cost mode, the momentum, the initial deviation and the noise exponent from its FIRST
// handle, so there they must be equal too; the recorded steps of icem_plan_step_batch carry each handle's own.
inline bool same_batch_config(const icem_config& a, const icem_config& r, bool exact) {
    return a.horizon == r.horizon && a.act_dim == r.act_dim && a.num_traj == r.num_traj && a.num_elites == r.num_elites &&
           a.elites_size == r.elites_size && a.opt_iters == r.opt_iters && a.use_mean_actions == r.use_mean_actions &&
           a.keep_previous_elites == r.keep_previous_elites && a.shift_elites == r.shift_elites && a.factor_decrease == r.factor_decrease &&
           a.fraction_reused == r.fraction_reused && a.rng_rounds == r.rng_rounds && a.dtype == r.dtype && a.world == r.world &&
           (a.noise_beta > 0) == (r.noise_beta > 0) &&
           (!exact || (a.cost_mode == r.cost_mode && a.rank == r.rank && a.alpha == r.alpha && a.init_std == r.init_std && a.noise_beta == r.noise_beta));
}

// Admission of a batch, before any handle is touched: n in [1, ICEM_MAX_BATCH], no null handle, no handle twice, one
// configuration.  who: prefix of the first three messages; config_msg: the whole text of the fourth.
inline int admit_batch(icem_handle* const* handles, int n, bool other_args, bool exact, const char* who, const char* config_msg) {
    if (!handles || !other_args || n < 1 || n > ICEM_MAX_BATCH) return fail(ICEM_E_INVALID, std::string(who) + "null argument / n outside [1, 32]");
    for (int i = 0; i < n; ++i)
        if (!handles[i]) return fail(ICEM_E_INVALID, std::string(who) + "null handle");
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < i; ++j)
            if (handles[i] == handles[j]) return fail(ICEM_E_INVALID, std::string(who) + "the same handle twice in one batch");
    for (int i = 1; i < n; ++i)
        if (!same_batch_config(handles[i]->cfg, handles[0]->cfg, exact)) return fail(ICEM_E_INVALID, config_msg);
    return ICEM_OK;
}
// The action width of the RSSM a handle's learned-dynamics steps serve: the bound one (icem_set_rssm_act_dim, which only takes the
// handle's own cfg.act_dim), else the declared 6 -- the library cannot see the width a `params` buffer was packed at, so a handle
// of another act_dim is served only once its caller has said that the model is that wide.
inline int rssm_width(const icem_handle* h) { return h->rssm_act ? h->rssm_act : 6; }
// ... and a batch shares one model, so one binding: differing ones are an unequal configuration (config_msg: admit_batch's)
inline int admit_rssm_binding(icem_handle* const* handles, int n, const char* config_msg) {
    for (int i = 1; i < n; ++i)
        if (rssm_width(handles[i]) != rssm_width(handles[0])) return fail(ICEM_E_INVALID, config_msg);
    return ICEM_OK;
}
// problem i's row of a batch's `results` (rows of row_bytes), or nullptr where the caller asked for none
inline void* results_row(void* results, int i, size_t row_bytes) {
    return results ? (unsigned char*)results + (size_t)i * row_bytes : nullptr;
}
inline int topk_blocks(int n) { return (n + TOPK_CHUNK - 1) / TOPK_CHUNK; }

template <typename T>
void split_partial_ws(void* ws, int nblk, int K, T** pc, int** pi) {
    *pc = (T*)ws;
    *pi = (int*)((unsigned char*)ws + (size_t)nblk * K * sizeof(T));
}

inline int check_handle(const icem_handle* h) {
    if (!h) return fail(ICEM_E_INVALID, "null handle");
    return ICEM_OK;
}

// ---- generic_kernels.hip: launchers of the generic kernels; pointers are of the handle's dtype ------------------
int gk_sample(const icem_handle* h, int n, long long first_index, const void* mean, const void* std, const void* low,
              const void* high, const void* zr, const void* zi, uint64_t offset, int t_begin, int row0_mean, void* out,
              const LaunchCtx& cx);   // (cx: the step's launch context -- under a recorder the launch is recorded, not issued; also gk_rollout,
                                      //  gk_shift_elites, gk_select_refit: the launches of a float64 step, icem_plan_step_batch_f64)
int gk_sample_truncnorm(const icem_handle* h, int n, long long first_index, const void* mean, const void* std,
                        const void* lower, const void* upper, const void* u, uint64_t offset, void* actions, hipStream_t st);
int gk_sample_piecewise(const icem_handle* h, int n, long long call_offset, int change_freq, long long first_block,
                        const void* low, const void* high, const void* u, void* actions, hipStream_t st);
int gk_cem_bounds(const icem_handle* h, int like_levine, const void* mean, void* std, const void* low, const void* high,
                  void* lower, void* upper, hipStream_t st);
int gk_philox_normals(const icem_handle* h, int n, long long first_index, uint64_t offset, void* z_r, void* z_i,
                      hipStream_t st);
int gk_rollout(const icem_handle* h, int n, const void* obs0, const void* actions, void* costs, void* observations,
               const LaunchCtx& cx);
int gk_trajectory_cost(const icem_handle* h, int n, int o, const void* obs, const void* nxt, long long ts, long long ss,
                       const void* actions, void* costs, hipStream_t st);
int gk_cost_reduce(const icem_handle* h, int n, const void* step_costs, void* costs, hipStream_t st);
int gk_topk(const icem_handle* h, int n, int K, const void* costs, void* out_c, int* out_i, void* ws, hipStream_t st);
int gk_topk_partial(const icem_handle* h, int n_cand, int K, const void* costs, void* ws, int nblk, hipStream_t st);
int gk_local_pack(const icem_handle* h, int nblk, int K, int n_loc, int shard_lo, int n_global, const void* ws,
                  const void* actions, void* records, hipStream_t st);
int gk_gather_refit(const icem_handle* h, const void* actions, const int32_t* idx, int k, void* mean, void* std,
                    void* elites_out, hipStream_t st);
int gk_shift(const icem_handle* h, void* mean, void* std, const void* low, const void* high, hipStream_t st);
int gk_reset(const icem_handle* h, void* mean, void* std, const void* low, const void* high, hipStream_t st);
int gk_shift_elites(const icem_handle* h, int n_extra, const void* elites, void* dst, const LaunchCtx& cx);
// icem_plan_step_learned* (learned_step.hip): the shifted elites of n problems in one launch -- the copy of elites[e, 1:, :] and
// icem_sample_clip(t_begin = h - 1)'s draw of the last action (f32, h <= 32, rng_rounds 10).  One argument block per problem
// in a device array (gk_shift_sample_block writes the host form, stream offset relative to the step's base).
size_t gk_shift_sample_block_bytes();
bool gk_shift_sample_quad(const icem_handle* h);
void gk_shift_sample_block(const icem_handle* h, int n_shift, const void* mean, const void* std, const void* low, const void* high,
                           uint64_t offset_rel, const void* elites_src, void* out, void* dst);
int gk_shift_sample_batch(const icem_handle* h, int n_problems, int n_shift_max, const void* args_dev, const BatchBases& bases, hipStream_t st);
// merge of the all-gathered records (+ kept elites): arguments of merge_refit_kernel, dtype-erased
struct MergeArgsV {
    int n_rec, n_keep, K, h, d, n_global, last;
    double alpha, init_std;
    const void* records;
    const void* elites_cur;
    const void* elites_cost_cur;
    void* elites_next;
    void* elites_cost_next;
    const void* mean_in;
    const void* std_in;
    void* mean;
    void* std;
    const void* low;
    const void* high;
    void* executed;
    void* best_cost;
    XchgWait xw;
};
int gk_merge_refit(const icem_handle* h, const MergeArgsV& a, hipStream_t st);
// world == 1: top-K over the pool's costs (+ kept elites) + gather + refit in ONE launch (a.records / a.n_rec unused)
bool gk_select_ok(const icem_handle* h, int n_cand, int n_keep, int K);
int gk_select_refit(const icem_handle* h, int n_cand, int n_loc, const void* costs, const void* actions, const MergeArgsV& a,
                    const LaunchCtx& cx);
// every index a cost term reads lies inside an observation of width o (nullptr = fine)
const char* cost_indices_error(const icem_handle* h, int o);
// ... of a cost spec + term list pair (terms: NULL = no list), the rule the handle's goes by
const char* cost_indices_error(const icem_cost_spec& cost, const icem_cost_terms* terms, int o);

// ---- k_rollout_f64.hip: the float64 rollout on the f64 matrix cores (icem_set_f64_arith(ICEM_F64_MFMA)) ----------------
size_t f64_mfma_lds_bytes(int o, int d);   // dynamic LDS of a launch (two buffers of 16 padded rows)
int launch_rollout_f64_mfma(const icem_handle* h, int n, const void* obs0, const void* actions, void* costs, void* observations,
                            hipStream_t st);

// ---- exchange.hip: the in-library elite exchange --------------------------------------------------------------------
bool xchg_connected(const icem_handle* h);
unsigned xchg_status_peek(const icem_handle* h);  // != 0: a device-side wait for a peer has timed out (not cleared)
// this rank's K records of the running iteration -> every rank's block (one launch); *wait_out: what the merge polls
// every peer runs in a process (stream) of its own: a launch of ours may wait for something a peer launches later
bool xchg_concurrent_peers(const icem_handle* h);
int xchg_push(icem_handle* h, const void* my_records, hipStream_t st, XchgWait* wait_out);
// ... or, where the caller's own kernel does the push (pack_records_kernel): the arguments for it
int xchg_begin(icem_handle* h, XchgPush* push_out, XchgWait* wait_out);
void xchg_destroy(icem_handle* h);

// Observation widths in (32, 384] exist only in k_rollout_wide.hip (f32, built-in HalfCheetah / HumanoidStandup cost form,
// device noise, K <= 32, costs only).  What a wide handle cannot do, spelled out (nullptr = fine) -- asked by
// icem_set_model / icem_set_cost_terms up front and by icem_rollout_cost / check_plan at use.
inline const char* wide_unsupported(const icem_handle* h, int K, bool external_noise, bool want_observations) {
    if (!h->wide) return nullptr;
    if (K > 32) return "obs_dim > 32 needs num_elites <= 32 (candidate lists of k_rollout_wide)";
    if (external_noise) return "obs_dim > 32 has no external-noise (z_r / z_i) path: the wide rollout is f32 with device noise only";
    if (want_observations) return "obs_dim > 32: icem_rollout_cost returns costs only at this width (observations == NULL)";
    return nullptr;
}

// ---- collective.hip: the RCCL form of the elite all-gather ----------------------------------------------------------
bool rccl_connected(const icem_handle* h);
int rccl_allgather_records(icem_handle* h, void* records, hipStream_t st);
void rccl_release(icem_handle* h);

// ---- plan.hip: the f32 throughput path ---------------------------------------------------------------------------
bool fast_rollout_ok(const icem_handle* h, int K);
// the f32 rollout of this handle is k_rollout_wide*.hip's GEMM kernel (obs_dim > 32, or a narrow model the tile kernels do not serve)
inline bool gemm_rollout(const icem_handle* h) { return h->wide || h->Of == 0; }
bool fast_sample_ok(const icem_handle* h);
int launch_fast_rollout(icem_handle* h, int n_rows, int n_cand, int K, const void* obs0, const void* actions,
                        void* costs, float* part_c, int* part_i, const LaunchCtx& cx, int* lists_out,
                        unsigned long long* part_k = nullptr, int n_tail = 0, int* tail_out = nullptr);
int rssm_launch_result(hipError_t e);   // abi.hip: a learned-dynamics launch's HIP result as an ICEM_* code (+ message)
// abi.hip: what every MLP rollout entry (and icem_plan_step_mlp) checks of a launch's own arguments; *on = the term list switched on
int admit_mlp_launch(const char* who, int32_t horizon, int32_t obs_dim, int32_t act_dim, int32_t layers, int32_t activation,
                     int32_t cost_mode, const icem_cost_spec* cost, const icem_cost_terms* terms, const icem_cost_terms** on);
// abi.hip: the launch icem_rollout_cost picks for this handle (the matrix-pipe rollout where it serves the handle and no
// observations are asked for, else the generic one) -- icem_plan_step_cem (cem_step.hip) rolls out through the same dispatch, and
// icem_plan_step_cem_batch records it (cx.rec: nothing is launched)
int rollout_cost_launch(icem_handle* h, int n, const void* obs0, const void* actions, void* costs, void* observations, const LaunchCtx& cx);
int refresh_act_mag(icem_handle* h, const void* low, const void* high, hipStream_t st, bool force);   // abi.hip
void ahead_destroy(icem_handle* h);
void predraw_next_step(icem_handle* h, const icem_plan_buffers* b, int mpc_step, const LaunchCtx& cx);
int launch_fast_sample(const icem_handle* h, int n, long long first_index, const void* mean, const void* std,
                       const void* low, const void* high, uint64_t offset, int row0_mean, void* out, const LaunchCtx& cx,
                       int n_shift = 0, const void* elites_src = nullptr, uint64_t offset2 = 0);

}  // namespace icem

#define ICEM_DISPATCH(h, expr_f32, expr_f64) ((h)->cfg.dtype == ICEM_F64 ? (expr_f64) : (expr_f32))
