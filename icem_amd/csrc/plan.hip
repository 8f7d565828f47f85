// plan.hip -- the fused MPC step behind icem_plan_iter_local / icem_plan_iter_merge / icem_plan_step / icem_get_action
// (the body of MpcICem.get_action, icem/controllers/icem.py:106-189): which kernels an iteration launches (generic
// path, two-kernel f32 path, single-launch f32 paths), where a merge rides (own launch or the next launch's prologue),
// where a sharded rank's record pack rides (own launch or workgroup 0 of the next local launch), which trailing
// shifted-elite rows go around the candidate lists, and which of the ping-pong buffers each launch reads and writes.  No device code here except the result publisher.
#include "host_common.h"
#include "recorded_batch.h"
#include "cost_terms_dev.h"

using namespace icem;

// icem_get_action: executed action + best cost -> the host-mapped block, then the sequence flag (system scope)
__global__ void publish_result_kernel(const float* executed, const float* best_cost, const unsigned* nonfinite, int d, float* host_out,
                                      unsigned* flag, unsigned seq) {
    const int j = threadIdx.x;
    if (j < d) host_out[j] = executed[j];
    if (j == d) host_out[d] = best_cost[0];
    if (j == d + 1) reinterpret_cast<unsigned*>(host_out)[d + 1] = nonfinite[0];   // the handle's status word (icem_nonfinite_costs)
    __threadfence_system();
    __syncthreads();
    if (j == 0) __hip_atomic_store(flag, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

namespace icem {

// An argument block with EVERY byte defined (padding included): icem_plan_step_batch keeps the blocks of the previous
// same-parity step and compares bytes to decide whether the device copy is still good.  (Members with a non-zero default:
// MergeSingleArgs::keep_base, FastRolloutArgs::act_mag / m_scale / b_scale.)
template <class T>
static T zeroed_args() {
    T t;
    std::memset((void*)&t, 0, sizeof(T));
    return t;
}

// Build the permuted, zero-padded [A ; B] operand of the matrix-pipe rollout (lazily: it depends on
// both icem_set_model and icem_set_cost).  Observation entries are reordered so that the linear cost
// term reads column 0 and the flip term column 0 or 1 -- static registers in the kernel.
int ensure_fast_model(icem_handle* h) {
    if (h->fast_model_ready) return ICEM_OK;
    if (gemm_rollout(h)) {  // the GEMM kernels' model, packed in MFMA operand order (k_rollout_wide.hip, k_rollout_wide_split.hip)
        // ONE packing, the one of the arithmetic in effect (icem_handle::wide_eff): exact f32, two fp16 planes with the
        // equilibrated model's scales, or three bf16 planes.  Everything is uploaded into fresh allocations first and the
        // handle's pointers and scales change together, after the last upload succeeded.
        struct Fresh {
            void* p[4] = {nullptr, nullptr, nullptr, nullptr};
            ~Fresh() { for (void* q : p) if (q) (void)hipFree(q); }
        } fr;
        auto up = [](void** dev, const void* src, size_t bytes) -> int {
            ICEM_HIP_TRY(hipMalloc(dev, bytes));
            ICEM_HIP_TRY(hipMemcpy(*dev, src, bytes, hipMemcpyHostToDevice));
            return ICEM_OK;
        };
        const int eff = h->wide_eff;
        float minv = 1.f, sb = 0.f;
        int nk = 0;
        int rc = ICEM_OK;
        if (eff == 1) {
            std::vector<float> Mw;
            pack_wide_model(h->obs_dim, h->cfg.act_dim, h->A_host.data(), h->B_host.data(), Mw);
            rc = up(&fr.p[0], Mw.data(), Mw.size() * sizeof(float));
        } else {
            std::vector<unsigned short> Mb;
            std::vector<float> ksc, csc;
            pack_wide_model_split(h->obs_dim, h->cfg.act_dim, h->A_host.data(), h->B_host.data(), eff == 2 ? 3 : 2, Mb, &minv, &ksc, &csc, &sb);
            rc = up(&fr.p[0], Mb.data(), Mb.size() * sizeof(unsigned short));
            if (!rc && eff == 0) {   // the scales of the equilibrated model: [ksc | csc] in one allocation
                nk = (int)ksc.size();
                ksc.insert(ksc.end(), csc.begin(), csc.end());
                rc = up(&fr.p[1], ksc.data(), ksc.size() * sizeof(float));
            }
        }
        if (rc) return rc;
        if (h->wide) {   // ... and row-major in f32 for the rows rolled out one by one (rollout_rows_wide_kernel) and TileHN
            std::vector<float> tmp(h->A_host.begin(), h->A_host.end());
            rc = up(&fr.p[2], tmp.data(), tmp.size() * sizeof(float));
            if (rc) return rc;
            tmp.assign(h->B_host.begin(), h->B_host.end());
            rc = up(&fr.p[3], tmp.data(), tmp.size() * sizeof(float));
            if (rc) return rc;
        }
        // commit
        void*& slot = eff == 1 ? h->Mw_dev : (eff == 0 ? h->Mwh_dev : h->Mws_dev);
        for (void** old : {&h->Mw_dev, &h->Mwh_dev, &h->Mws_dev, &h->Mwh_ksc_dev}) {
            if (*old) (void)hipFree(*old);
            *old = nullptr;
        }
        slot = fr.p[0];
        h->Mwh_ksc_dev = fr.p[1];
        h->Mwh_inv = minv;
        h->Mwh_sbound = sb;
        h->Mwh_nk = nk;
        fr.p[0] = fr.p[1] = nullptr;
        if (h->wide) {   // (a narrow model on the GEMM kernel: A_dev / B_dev keep the generic kernels' padded layout)
            if (h->A_dev) (void)hipFree(h->A_dev);
            if (h->B_dev) (void)hipFree(h->B_dev);
            h->A_dev = fr.p[2];
            h->B_dev = fr.p[3];
            fr.p[2] = fr.p[3] = nullptr;
        }
        h->wide_packed = eff;
        h->fast_model_ready = true;
        return ICEM_OK;
    }
    const int O = h->O, o = h->obs_dim, d = h->cfg.act_dim;
    // layout of Tile16 (fused_dev.h): O <= 20 -> one 16-column matrix-pipe tile + extra columns, Mp [O + d + 1, ceil4(O)];
    // O > 20 -> two tiles, observation block padded to 32 rows / columns, Mp [32 + d + 1, 32]
    const bool two = O > 20;
    const int OP = two ? 32 : O;
    const int CT4 = two ? 32 : ((O + 3) / 4) * 4;
    std::vector<int> perm;
    perm.push_back(h->cost.lin_idx);
    h->flip_col = -1;
    if (h->cost.flip_idx >= 0) {
        if (h->cost.flip_idx == h->cost.lin_idx) {
            h->flip_col = 0;
        } else {
            perm.push_back(h->cost.flip_idx);
            h->flip_col = 1;
        }
    }
    for (int k = 0; k < O; ++k)
        if (std::find(perm.begin(), perm.end(), k) == perm.end()) perm.push_back(k);
    std::vector<float> Mp((size_t)(OP + d + 1) * CT4, 0.f);  // + one zero row (contraction slots without an entry)
    auto Aat = [&](int r, int c) { return (r < o && c < o) ? h->A_host[(size_t)r * o + c] : 0.0; };
    auto Bat = [&](int j, int c) { return c < o ? h->B_host[(size_t)j * o + c] : 0.0; };
    for (int k = 0; k < O; ++k)
        for (int c = 0; c < O; ++c) Mp[(size_t)k * CT4 + c] = (float)Aat(perm[k], perm[c]);
    for (int j = 0; j < d; ++j)
        for (int c = 0; c < O; ++c) Mp[(size_t)(OP + j) * CT4 + c] = (float)Bat(j, perm[c]);
    for (int k = 0; k < (int)perm.size(); ++k)
        if (k >= o || perm[k] >= o) perm[k] = 31;  // padding columns start from the zero slot of the staged observation
    perm.resize(32, 31);
    if (h->Mp_dev) (void)hipFree(h->Mp_dev);
    if (h->perm_dev) (void)hipFree(h->perm_dev);
    ICEM_HIP_TRY(hipMalloc(&h->Mp_dev, Mp.size() * sizeof(float)));
    ICEM_HIP_TRY(hipMalloc(&h->perm_dev, perm.size() * sizeof(int)));
    ICEM_HIP_TRY(hipMemcpy(h->Mp_dev, Mp.data(), Mp.size() * sizeof(float), hipMemcpyHostToDevice));
    ICEM_HIP_TRY(hipMemcpy(h->perm_dev, perm.data(), perm.size() * sizeof(int), hipMemcpyHostToDevice));
    h->fast_model_ready = true;
    return ICEM_OK;
}

bool fast_rollout_ok(const icem_handle* h, int K) {
    if (h->cfg.dtype != ICEM_F32 || !h->has_model || !h->has_cost) return false;
    if (h->wide)  // (the only rollout there is at this width: ICEM_DISABLE_FAST does not apply)
        return wide_rollout_supported(h->obs_dim, h->cfg.act_dim, K);
    if (!h->use_fast) return false;
    // o <= 32: the tile kernels where they serve the model + cost (no icem_cost_terms, a linear term, a compiled shape);
    // otherwise the exact-f32 GEMM kernel with its smallest column count -- FetchPickAndPlace (settings/fpp: o = 28, d = 4,
    // a norm cost), Hopper, Reacher, FetchReach ... run at matrix-pipe speed instead of one thread per trajectory
    if (h->Of == 0) return gemm_rollout_supported(h->obs_dim, h->cfg.act_dim, K);
    return fast_rollout_supported(h->cfg.horizon, h->cfg.act_dim, h->Of, K);
}

FastRolloutArgs fast_rollout_args(const icem_handle* h, int n_rows, int n_cand, int K, const void* obs0,
                                  const void* actions, void* costs, float* part_c, int* part_i) {
    FastRolloutArgs a = zeroed_args<FastRolloutArgs>();
    a.n_rows = n_rows;
    a.n_cand = n_cand;
    a.K = K;
    a.o = h->obs_dim;
    a.cost_mode = h->cfg.cost_mode;
    a.Mp = (const float*)h->Mp_dev;
    a.perm = (const int*)h->perm_dev;
    a.obs0 = (const float*)obs0;
    a.ctrl_w = (float)h->cost.ctrl_weight;
    a.lin_w = (float)h->cost.lin_weight;
    a.flip_pen = (float)h->cost.flip_penalty;
    a.flip_th = (float)h->cost.flip_thresh;
    a.flip_col = h->flip_col;
    a.actions = (const float*)actions;
    a.costs = (float*)costs;
    a.part_c = part_c;
    a.part_i = part_i;
    a.part_k = nullptr;
    a.dbg = h->dbg;
    a.arith = h->tile_arith;
    a.act_mag = h->act_mag;
    a.m_scale = h->tile_m_scale;
    a.b_scale = h->tile_b_scale;
    a.inv_m_scale = h->tile_inv_m_scale;
    a.inv_b_scale = h->tile_inv_b_scale;
    a.nonfinite = h->nonfinite_dev;
    return a;
}

// workgroups (= candidate lists) of the single-launch kernel for this handle, 0 where it has none.  (Its small slabs roll out on
// Tile4, the VALU twin of the EXACT tile; a handle whose tile arithmetic is the fp16 planes gets the kernel's Tile16H
// instantiation instead -- one arithmetic per handle, whatever a launch's row count.)
static int one_launch_lists(const icem_handle* h, const BatchHint& bh, int n_rows, int n_tail = 0, int* tail_out = nullptr) {
    if (tail_out) *tail_out = 0;
    const icem_config& c = h->cfg;
    return sample_rollout_lists(bh, c.horizon, c.act_dim, h->Of, c.rng_rounds, n_rows, n_tail, tail_out);
}

// a launcher without a batched form, reached while recording (icem_plan_step_batch checks its configurations up front; belt
// and braces): nothing is launched, the batch is refused
static int no_batched_form(const LaunchCtx& cx, const char* what) {
    cx.rec->unsupported = true;
    return fail(ICEM_E_UNSUPPORTED, std::string(cx.rec->who) + what);
}

// rows -> costs (+ one sorted candidate list per workgroup when K > 0); returns the number of candidate lists
int launch_fast_rollout(icem_handle* h, int n_rows, int n_cand, int K, const void* obs0, const void* actions,
                        void* costs, float* part_c, int* part_i, const LaunchCtx& cx, int* lists_out,
                        unsigned long long* part_k, int n_tail, int* tail_out) {
    hipStream_t st = cx.st;
    int rc = ensure_fast_model(h);   // (per handle, also ahead of a batch's recorded launches: uploads only)
    if (rc) return rc;
    if (tail_out) *tail_out = 0;
    if (h->hn_tile) {   // Door / Relocate / FetchPickAndPlace shapes: TileHN (k_rollout_hn.hip)
        // trailing shifted elites that would open a second round of tiles: workgroups of their own, no list (tail_out rows: the
        // caller's merge takes them as extra candidates through the cost array)
        const int tail = (tail_out && n_cand == n_rows && K > 0) ? hn_tail_rows(cx.hint, n_rows, n_tail) : 0;
        FastRolloutArgs a = fast_rollout_args(h, n_rows, tail ? n_rows - tail : n_cand, K, obs0, actions, costs, part_c, part_i);
        a.part_k = part_k;
        a.arith = 1;
        a.list_wgs = tail ? (n_rows - tail) / 16 : 0;
        if (tail) *tail_out = tail;
        const int ld = h->wide ? h->obs_dim : h->O;   // A_dev / B_dev: row-major f32, unpadded at o > 32, padded to O below
        {
            ProfScope prof(h, ICEM_K_ROLLOUT, (long long)n_rows * h->cfg.horizon, st);
            launch_rollout_hn(cx, a, h->cfg.horizon, h->cfg.act_dim, h->obs_dim, h->model_kind, (const float*)h->A_dev, ld, (const float*)h->B_dev, ld,
                              h->cost.lin_idx, h->cost.flip_idx, h->has_terms ? (const CostArgs<float>*)h->hn_cs_dev : nullptr, h->hn_prog);
        }
        ICEM_HIP_TRY(hipGetLastError());
        if (lists_out) *lists_out = tail ? a.list_wgs : hn_rollout_lists(cx.hint, n_rows);
        return ICEM_OK;
    }
    if (gemm_rollout(h)) {
        // narrow observations always take the exact-f32 kernel (two workgroup barriers per step buy nothing at o <= 32)
        const bool exact = h->wide_eff == 1;   // (update_paths: asked for, a narrow model, or a width the split kernel does not hold)
        // trailing shifted elites that would open a tile of their own: rolled out row by row (rollout_rows_wide_kernel),
        // scored by the merge through the cost array (tail_out rows; the caller's merge takes them as extra candidates)
        // (exact-f32 tile kernel only: the bf16-split kernel's workgroups take a fifth tile instead)
        const bool split_tail = h->wide && exact && tail_out && n_tail > 0 && n_tail <= 64 && n_cand == n_rows && (n_rows - n_tail) % 16 == 0 &&
                                n_rows - n_tail > 0 && h->cfg.dtype == ICEM_F32;
        if (split_tail) {
            n_rows -= n_tail;
            n_cand = n_rows;
            *tail_out = n_tail;
        }
        WideRolloutArgs w{};
        w.n_rows = n_rows;
        w.n_cand = n_cand;
        w.K = K;
        w.o = h->obs_dim;
        w.d = h->cfg.act_dim;
        w.h = h->cfg.horizon;
        w.kb = exact ? wide_kb(w.o, w.d) : wide_split_kb(w.o, w.d);
        w.xs = exact ? wide_xs(w.o, w.d) : wide_split_xs(w.o, w.d);
        w.cost_mode = h->cfg.cost_mode;
        w.lin_idx = h->cost.lin_idx;
        w.flip_idx = h->cost.flip_idx;
        w.ctrl_w = (float)h->cost.ctrl_weight;
        w.lin_w = (float)h->cost.lin_weight;
        w.flip_pen = (float)h->cost.flip_penalty;
        w.flip_th = (float)h->cost.flip_thresh;
        w.cs = h->has_terms ? (const CostArgs<float>*)h->wide_cs_dev : nullptr;
        w.planes = h->wide_eff == 2 ? 3 : 2;    // (split kernel) fp16 planes, or the bf16 ones (asked for, or AUTO on an unbalanced model)
        w.minv = w.planes == 2 ? h->Mwh_inv : 1.f;
        w.ksc = (const float*)h->Mwh_ksc_dev;
        w.csc = w.ksc ? w.ksc + h->Mwh_nk : nullptr;
        w.sbound = h->Mwh_sbound;
        w.Mp = exact ? (const float*)h->Mw_dev : (const float*)(w.planes == 2 ? h->Mwh_dev : h->Mws_dev);
        w.dbg = h->dbg;
        w.obs0 = (const float*)obs0;
        w.actions = (const float*)actions;
        w.costs = (float*)costs;
        w.part_c = part_c;
        w.part_i = part_i;
        w.part_k = part_k;
        {
            ProfScope prof(h, ICEM_K_ROLLOUT, (long long)n_rows * h->cfg.horizon, st);
            if (exact) launch_rollout_wide(cx, w, h->model_kind);
            else launch_rollout_wide_split(cx, w, h->model_kind);
            // (the row-wise kernel BESIDE the tile kernel on a second stream instead of behind it was measured: 4.70
            //  instead of 4.15 ms per MPC step -- the three CUs that host a row workgroup finish their tile workgroup
            //  late, and the launch waits for its slowest workgroup; EXPERIMENTS.md R3.7)
            if (split_tail) launch_rollout_rows_wide(cx, w, n_rows, n_tail, (const float*)h->A_dev, (const float*)h->B_dev, h->model_kind);
        }
        ICEM_HIP_TRY(hipGetLastError());
        if (lists_out) *lists_out = exact ? wide_rollout_lists(n_rows) : wide_split_lists(n_rows);
        return ICEM_OK;
    }
    // (rollout16 alone: a tile shape's two-kernel iteration.  Recorded as LAUNCH_ROLLOUT16 -- icem_plan_step_cem_batch; the steps of
    //  icem_plan_step_batch take the single-launch and noise-ahead families at these shapes and do not come here)
    FastRolloutArgs a = fast_rollout_args(h, n_rows, n_cand, K, obs0, actions, costs, part_c, part_i);
    a.part_k = part_k;
    const int grid = rollout_lists(h->cfg.horizon, h->cfg.act_dim, h->Of, n_rows);
    {
        ProfScope prof(h, ICEM_K_ROLLOUT, (long long)n_rows * h->cfg.horizon, st);
        launch_rollout16(cx, a, h->cfg.horizon, h->cfg.act_dim, h->Of, h->model_kind);
    }
    ICEM_HIP_TRY(hipGetLastError());
    if (lists_out) *lists_out = grid;
    return ICEM_OK;
}

bool fast_sample_ok(const icem_handle* h) {
    return h->use_fast && h->cfg.dtype == ICEM_F32 && fast_sample_supported(h->cfg.horizon, h->cfg.act_dim);
}

FastSampleArgs fast_sample_args(const icem_handle* h, int n, long long first_index, const void* mean, const void* std,
                                const void* low, const void* high, uint64_t offset, int row0_mean, void* out,
                                int n_shift, const void* elites_src, uint64_t offset2) {
    FastSampleArgs a = zeroed_args<FastSampleArgs>();
    a.n = n;
    a.h = h->cfg.horizon;
    a.d = h->cfg.act_dim;
    a.first_index = first_index;
    a.W = (const float*)h->W_dev;
    a.mean = (const float*)mean;
    a.std = (const float*)std;
    a.low = (const float*)low;
    a.high = (const float*)high;
    a.seed_lo = (uint32_t)h->cfg.seed;
    a.seed_hi = (uint32_t)(h->cfg.seed >> 32);
    a.off_lo = (uint32_t)offset;
    a.off_hi = (uint32_t)(offset >> 32);
    a.row0_mean = row0_mean;
    a.out = (float*)out;
    a.n_shift = n_shift;
    a.elites_src = (const float*)elites_src;
    a.off2_lo = (uint32_t)offset2;
    a.off2_hi = (uint32_t)(offset2 >> 32);
    a.white = h->cfg.noise_beta <= 0 ? 1 : 0;
    a.raw_src = nullptr;
    return a;
}

int launch_fast_sample(const icem_handle* h, int n, long long first_index, const void* mean, const void* std,
                       const void* low, const void* high, uint64_t offset, int row0_mean, void* out, const LaunchCtx& cx,
                       int n_shift, const void* elites_src, uint64_t offset2) {
    if (n <= 0 && n_shift <= 0) return ICEM_OK;
    hipStream_t st = cx.st;
    const FastSampleArgs a = fast_sample_args(h, n, first_index, mean, std, low, high, offset, row0_mean, out, n_shift,
                                              elites_src, offset2);
    {
        ProfScope prof(h, ICEM_K_SAMPLE, (long long)n * a.h, st);
        launch_sample_folded(cx, a, h->cfg.rng_rounds);
    }
    ICEM_HIP_TRY(hipGetLastError());
    return ICEM_OK;
}

// Can the f32 launch of an iteration with n_rows local rows (no shifted elites) carry a merge in its prologue?
// (single-launch kernel with <= 4 rollout waves, or the sampler of the two-kernel path)
bool prologue_possible(const icem_handle* h, const BatchHint& bh, int n_rows) {
    const icem_config& c = h->cfg;
    const int K = c.num_elites;
    if (c.dtype != ICEM_F32 || !fast_rollout_ok(h, K) || !fast_sample_ok(h) || n_rows <= 0) return false;
    if (one_launch_lists(h, bh, n_rows) > 0)
        return sample_rollout_merge_ok(bh, c.horizon, c.act_dim, h->Of, c.rng_rounds, n_rows, K);
    return sample_folded_merge_ok(c.horizon, c.act_dim, c.rng_rounds, K);
}

// this rank's shard of iteration `it`: rows [lo, lo + n_loc) of the population (world 1: all of it)
struct Shard {
    int lo, n_loc;
};
static Shard shard_of(const icem_handle* h, int it) {
    const int n_global = h->pop[it];
    const int chunk = shard_chunk(n_global, h->cfg.world);
    const int lo = std::min(n_global, h->cfg.rank * chunk);
    return {lo, std::max(0, std::min(n_global - lo, chunk))};
}

// the gathered records fit the prologue's selection, which holds two records per lane (128 records at most)
static bool records_fit_prologue(const icem_handle* h) { return h->cfg.world * h->cfg.num_elites <= 128 && h->cfg.num_elites <= 32; }

// published merge (PackPrev::pub): workgroup 0 merges the records once and publishes mean | std to the rest
static int ensure_pub(icem_handle* h, hipStream_t st) {
    if (h->pub_dev) return ICEM_OK;
    const size_t bytes = ((size_t)2 * h->hd + 16) * sizeof(float);
    ICEM_HIP_TRY(hipMalloc((void**)&h->pub_dev, bytes));
    ICEM_HIP_TRY(hipMemsetAsync(h->pub_dev, 0, bytes, st));
    return ICEM_OK;
}
static void set_pub(icem_handle* h, PackPrev& p) {
    p.pub = h->pub_dev;
    p.pub_flag = reinterpret_cast<unsigned*>(h->pub_dev + 2 * h->hd);
    p.pub_seq = ++h->pub_seq;
}

// Where an iteration's merge goes: launched now or stashed for the next launch's prologue, and where it writes mean / std
// (nullptr: in place).
struct MergeRoute {
    bool defer = false;
    float* mean_out = nullptr;
    float* std_out = nullptr;
};
// the last iteration's distribution goes to the caller's buffers, a folded one to the handle's ping-pong pair, any other in place
static MergeRoute merge_route(const icem_handle* h, const icem_plan_buffers* b, int it, bool fold) {
    if (it == h->cfg.opt_iters - 1) return {false, (float*)b->mean, (float*)b->std};
    if (!fold) return {};
    float* pp = h->pp_stats + (size_t)(it & 1) * 2 * h->hd;
    return {true, pp, pp + h->hd};
}

// ---- argument blocks ----------------------------------------------------------------------------------------------------

// the fields every form of iteration `it`'s merge shares, in the handle's dtype
template <typename T>
static MergeArgsV merge_args(const icem_handle* h, const icem_plan_buffers* b, int mpc_step, int it, MergeRoute route) {
    const icem_config& c = h->cfg;
    const int hd = h->hd, K = c.num_elites;
    const int cur = elite_parity(h, mpc_step, it), nxt = cur ^ 1;
    T* el = (T*)b->elites;
    T* elc = el + (size_t)2 * K * hd;
    MergeArgsV a{};
    a.n_rec = c.world * K;
    a.n_keep = (it > 0 && c.keep_previous_elites) ? h->n_reuse : 0;
    a.K = K;
    a.h = c.horizon;
    a.d = c.act_dim;
    a.n_global = h->pop[it];
    a.last = it == c.opt_iters - 1;
    a.alpha = c.alpha;
    a.init_std = c.init_std;
    a.records = b->records;
    if (c.world > 1 && xchg_connected(h)) {  // the records of this iteration arrive in the exchange block
        a.xw = h->xw_last;
        a.records = h->xw_last.records;
    }
    a.elites_cur = el + (size_t)cur * K * hd;
    a.elites_cost_cur = elc + (size_t)cur * K;
    a.elites_next = el + (size_t)nxt * K * hd;
    a.elites_cost_next = elc + (size_t)nxt * K;
    a.mean_in = b->mean;
    a.std_in = b->std;
    a.mean = route.mean_out ? (void*)route.mean_out : b->mean;
    a.std = route.std_out ? (void*)route.std_out : b->std;
    a.low = b->low;
    a.high = b->high;
    a.executed = b->executed;
    a.best_cost = b->best_cost;
    return a;
}

// ... as the f32 merge kernels take them: sets the shared fields of `m` in place (a zeroed block keeps its defined padding)
static void fill_single(MergeSingleArgs& m, const MergeArgsV& a) {
    m.n_keep = a.n_keep;
    m.n_global = a.n_global;
    m.K = a.K;
    m.h = a.h;
    m.d = a.d;
    m.last = a.last;
    m.alpha = (float)a.alpha;
    m.init_std = (float)a.init_std;
    m.elites_cur = (const float*)a.elites_cur;
    m.elites_cost_cur = (const float*)a.elites_cost_cur;
    m.elites_next = (float*)a.elites_next;
    m.elites_cost_next = (float*)a.elites_cost_next;
    m.mean = (const float*)a.mean_in;
    m.std = (const float*)a.std_in;
    m.mean_out = (float*)a.mean;
    m.std_out = (float*)a.std;
    m.low = (const float*)a.low;
    m.high = (const float*)a.high;
    m.executed = (float*)a.executed;
    m.best_cost = (float*)a.best_cost;
}

// ... and back, for a stashed records merge that runs on the generic kernel after all
static MergeArgsV generic_from(const MergeSingleArgs& m) {
    MergeArgsV a{};
    a.n_rec = m.n_rec;
    a.n_keep = m.n_keep;
    a.K = m.K;
    a.h = m.h;
    a.d = m.d;
    a.n_global = m.n_global;
    a.last = m.last;
    a.alpha = m.alpha;
    a.init_std = m.init_std;
    a.records = m.records;
    a.elites_cur = m.elites_cur;
    a.elites_cost_cur = m.elites_cost_cur;
    a.elites_next = m.elites_next;
    a.elites_cost_next = m.elites_cost_next;
    a.mean_in = m.mean;
    a.std_in = m.std;
    a.mean = m.mean_out;
    a.std = m.std_out;
    a.low = m.low;
    a.high = m.high;
    a.executed = m.executed;
    a.best_cost = m.best_cost;
    a.xw = m.xw;
    return a;
}

// A sharded rank's K best of its candidate lists -> records for the all-gather (same selection code as the merge): the
// pack launched on its own.  tail > 0: rank 0's shifted elites sit behind the list-writing workgroups -- extra candidates
// of the pack, costs from the cost array (from row n_loc on), key index = their local pool row.
static MergeSingleArgs local_pack_args(const icem_handle* h, int it, int lists, int n_pool, const void* part_k, const float* actions,
                                       int n_loc, int tail, const void* costs) {
    MergeSingleArgs pk{};
    pk.n_lists = lists;
    pk.n_pool = n_pool;
    pk.n_global = h->pop[it];
    pk.K = h->cfg.num_elites;
    pk.h = h->cfg.horizon;
    pk.d = h->cfg.act_dim;
    pk.part_k = (const unsigned long long*)part_k;
    pk.actions = actions;
    if (tail > 0) {
        pk.n_keep = tail;
        pk.elites_cost_cur = (const float*)costs + n_loc;
        pk.keep_base = n_loc;
    }
    return pk;
}

// ... the same pack as a rider of a later launch
static PackPrev make_pack(const MergeSingleArgs& pk, Shard sh, float* records, const XchgPush& px) {
    PackPrev pp;
    pp.part_k = pk.part_k;
    pp.actions = pk.actions;
    pp.n_lists = pk.n_lists;
    pp.n_pool = pk.n_pool;
    pp.n_global = pk.n_global;
    pp.K = pk.K;
    pp.n_loc = sh.n_loc;
    pp.shard_lo = sh.lo;
    pp.n_keep = pk.n_keep;
    pp.keep_costs = pk.elites_cost_cur;
    pp.records = records;
    pp.px = px;
    return pp;
}

// ... and a rider that runs as a launch after all (launch_pack_records / launch_pack_merge)
static MergeSingleArgs pack_launch_args(const icem_handle* h, const PackPrev& pp) {
    MergeSingleArgs pk{};
    pk.n_lists = pp.n_lists;
    pk.n_pool = pp.n_pool;
    pk.n_global = pp.n_global;
    pk.K = pp.K;
    pk.h = h->cfg.horizon;
    pk.d = h->cfg.act_dim;
    pk.part_k = pp.part_k;
    pk.actions = pp.actions;
    pk.n_keep = pp.n_keep;
    pk.elites_cost_cur = pp.keep_costs;
    pk.keep_base = pp.n_loc;
    return pk;
}

// a stashed merge that found no launch to ride in
int launch_pending_merge(icem_handle* h, const LaunchCtx& cx) {
    if (cx.rec) return no_batched_form(cx, "a merge found no launch to ride in");
    hipStream_t st = cx.st;
    const MergeSingleArgs& m = h->ride.merge;
    if (m.records != nullptr) return gk_merge_refit(h, generic_from(m), st);
    {
        ProfScope prof(h, ICEM_K_MERGE_REFIT, m.n_lists * m.K + m.n_keep, st);
        launch_merge_single(cx, m);
    }
    ICEM_HIP_TRY(hipGetLastError());
    return ICEM_OK;
}

// will the merge-prologue launch of an iteration with n_rows local rows take the previous iteration's pack along?
static bool next_launch_takes_pack(const icem_handle* h, const BatchHint& bh, int n_rows) {
    const icem_config& c = h->cfg;
    if (one_launch_lists(h, bh, n_rows) > 0)
        return sample_rollout_pack_ok(bh, c.horizon, c.act_dim, h->Of, c.rng_rounds, n_rows, c.num_elites);
    return sample_folded_pack_ok(c.horizon, c.act_dim, c.rng_rounds, c.num_elites);
}

// a stashed pack that found no launch to ride in
int launch_pending_pack(icem_handle* h, const LaunchCtx& cx) {
    hipStream_t st = cx.st;
    const PackPrev& pp = h->ride.pack;
    {
        ProfScope prof(h, ICEM_K_LOCAL_PACK, pp.n_lists * pp.K, st);
        launch_pack_records(pack_launch_args(h, pp), pp.n_loc, pp.shard_lo, pp.records, st, pp.px);
    }
    ICEM_HIP_TRY(hipGetLastError());
    h->ride.pack_pending = false;
    return ICEM_OK;
}

template <typename T>
int plan_iter_local_t(icem_handle* h, const icem_plan_buffers* b, int mpc_step, int it, const LaunchCtx& cx) {
    hipStream_t st = cx.st;
    const icem_config& c = h->cfg;
    const int hd = h->hd, K = c.num_elites;
    const int n_global = h->pop[it];
    const Shard sh = shard_of(h, it);
    const int lo = sh.lo, n_loc = sh.n_loc;
    const uint64_t base = call_base(h, mpc_step);
    const bool last = it == c.opt_iters - 1;
    T* actions = (T*)b->actions;
    const int n_extra = shift_rows(h, mpc_step, it);
    const T* shift_src = nullptr;
    bool shift_in_sampler = false;
    if (n_extra > 0) {
        shift_src = (const T*)b->elites + (size_t)elite_parity(h, mpc_step, 0) * K * hd;  // the elite buffer holding the previous step's set
        // the fast sampler prepares them in an extra workgroup of its own launch
        shift_in_sampler = std::is_same<T, float>::value && b->z_r == nullptr && b->z_r_shift == nullptr &&
                           fast_rollout_ok(h, K) && fast_sample_ok(h) &&
                           n_extra * c.act_dim <= 256;
        if (!shift_in_sampler) {
            T* dst = actions + (size_t)n_loc * hd;
            int rc = gk_shift_elites(h, n_extra, shift_src, dst, cx);
            if (rc) return rc;
            rc = gk_sample(h, n_extra, 0, b->mean, b->std, b->low, b->high, b->z_r_shift, b->z_i_shift,
                           base + (uint64_t)c.opt_iters, c.horizon - 1, 0, dst, cx);
            if (rc) return rc;
        }
    }
    // candidates: the shard, plus the shifted elites on rank 0 only (they are replicated)
    const int n_cand = n_loc + (c.rank == 0 ? n_extra : 0);
    const int row0 = (last && c.use_mean_actions) ? 1 : 0;
    T* rec = (T*)b->records + (size_t)c.rank * K * (hd + 2);
    h->local.lists = 0;
    h->local.sel_cand = 0;
    if constexpr (std::is_same<T, float>::value) {
        if (fast_rollout_ok(h, K)) {
            // f32 throughput path.  External white noise (b->z_r: the reference's own draws, tests/golden) takes it too: the
            // generic sampler turns the caller's z into the pool (it is the only kernel that reads z), and from there on the
            // tile rollout, the lists and the threshold merges are the ones device noise gets -- the reference's draws reach
            // Tile16 / Tile16H and merge_select*, not only the generic kernels.
            const bool ext_z = b->z_r != nullptr;
            const uint64_t off = base + (uint64_t)it;
            int rc = ensure_fast_model(h);
            if (rc) return rc;
            int lists = 0;
            float* pc;
            int* pi;
            const int n_rows = n_loc + n_extra;
            int tail_rows = 0;  // shifted-elite rows scored through the cost array instead of a list (world 1 only)
            const int one = (!ext_z && fast_sample_ok(h) && (n_extra == 0 || shift_in_sampler))
                                ? one_launch_lists(h, cx.hint, n_rows, shift_in_sampler ? n_extra : 0, &tail_rows) : 0;
            h->local.tail_rows = one > 0 ? tail_rows : 0;
            // the merge finds the lists' indices behind `lists * K` costs
            split_partial_ws<float>(b->workspace, one > 0 ? one : rollout_lists(c.horizon, c.act_dim, h->Of, n_rows), K, &pc, &pi);
            bool prologue = false, ride = false;
            if (h->ride.merge_pending) {
                prologue = !ext_z && n_extra == 0 && prologue_possible(h, cx.hint, n_rows);
                // a stashed pack rides with the merge whose records it produces, or runs now -- in front of that merge
                ride = prologue && h->ride.pack_pending && next_launch_takes_pack(h, cx.hint, n_rows);
                if (h->ride.pack_pending && !ride) {
                    rc = launch_pending_pack(h, cx);
                    if (rc) return rc;
                }
                if (!prologue) {  // cannot ride along after all: run it now
                    rc = launch_pending_merge(h, cx);
                    if (rc) return rc;
                }
                h->ride.merge_pending = false;
            } else if (h->ride.pack_pending) {
                rc = launch_pending_pack(h, cx);
                if (rc) return rc;
            }
            h->ride.pack_pending = false;
            if (one > 0) {
                // small populations: sample + rollout + top-K in one launch
                FastIterArgs fa = zeroed_args<FastIterArgs>();
                fa.m.keep_base = -1;
                if (prologue) fa.m = h->ride.merge;
                if (ride) fa.p = h->ride.pack;
                fa.s = fast_sample_args(h, n_loc, lo, b->mean, b->std, b->low, b->high, off, row0, actions,
                                        shift_in_sampler ? n_extra : 0, shift_src, base + (uint64_t)c.opt_iters);
                if (it == 0 && c.world == 1 && h->ahead.pre_valid) {
                    // this step's first noise (and the shifted elites') was drawn beside the previous step's last merge -- on
                    // pre_stream: a step enqueued on another stream is not ordered behind that launch and redraws instead
                    if (h->ahead.pre_episode == h->episode && h->ahead.pre_step == mpc_step && h->ahead.pre_stream == st) fa.s.raw_src = (const float*)h->ahead.pre_raw;
                    h->ahead.pre_valid = false;
                }
                fa.r = fast_rollout_args(h, n_rows, n_cand, K, b->obs0, actions, b->costs, pc, pi);
                fa.r.part_k = (unsigned long long*)b->workspace;  // read by merge_single_kernel / pack_records_kernel
                fa.r.list_wgs = tail_rows > 0 ? one : 0;
                {
                    ProfScope prof(h, ICEM_K_SAMPLE_ROLLOUT, (long long)n_rows * c.horizon, st);
                    launch_sample_rollout(cx, fa, c.horizon, c.act_dim, h->Of, h->model_kind, prologue);
                }
                ICEM_HIP_TRY(hipGetLastError());
                lists = one;
            }
            if (one == 0) {
                if (prologue) {
                    FastSampleMergeArgs sm = zeroed_args<FastSampleMergeArgs>();
                    sm.s = fast_sample_args(h, n_loc, lo, b->mean, b->std, b->low, b->high, off, row0, actions, 0, nullptr, 0);
                    sm.m = h->ride.merge;
                    if (ride) {
                        sm.p = h->ride.pack;
                        // published merge: workgroup 0 merges the records once and publishes mean | std to the rest
                        const int pub_on = opt_i(OPT_PUBLISHED_MERGE);
                        if (pub_on && sm.m.records) {
                            rc = ensure_pub(h, st);
                            if (rc) return rc;
                            set_pub(h, sm.p);
                        }
                    }
                    {
                        ProfScope prof(h, ICEM_K_SAMPLE, (long long)n_loc * c.horizon, st);
                        launch_sample_folded_merge(cx, sm);
                    }
                    ICEM_HIP_TRY(hipGetLastError());
                    rc = ICEM_OK;
                } else if (ext_z) {
                    rc = gk_sample(h, n_loc, lo, b->mean, b->std, b->low, b->high, b->z_r, b->z_i, off, 0, row0, actions, cx);
                } else if (fast_sample_ok(h)) {
                    rc = launch_fast_sample(h, n_loc, lo, b->mean, b->std, b->low, b->high, off, row0, actions, cx,
                                            shift_in_sampler ? n_extra : 0, shift_src, base + (uint64_t)c.opt_iters);
                } else {
                    rc = gk_sample(h, n_loc, lo, b->mean, b->std, b->low, b->high, nullptr, nullptr, off, 0, row0, actions, cx);
                }
                if (rc) return rc;
                int tail2 = 0;
                rc = launch_fast_rollout(h, n_rows, n_cand, K, b->obs0, actions, b->costs, pc, pi, cx, &lists,
                                         (unsigned long long*)b->workspace, (c.world == 1 && it == 0) ? n_extra : 0, &tail2);
                if (rc) return rc;
                h->local.tail_rows = tail2;
            }
            h->local.lists = lists;
            if (c.world > 1) {
                // this rank's K best -> records for the all-gather
                const MergeSingleArgs pk = local_pack_args(h, it, lists, n_rows, b->workspace, (const float*)actions, n_loc,
                                                           (one > 0 && c.rank == 0) ? tail_rows : 0, b->costs);
                XchgPush px;  // in-library exchange: the pack kernel pushes the records itself where they fit its LDS
                const bool fold_push = xchg_connected(h) && pack_can_push(K, c.horizon, c.act_dim);
                if (fold_push) {
                    rc = xchg_begin(h, &px, &h->xw_last);
                    if (rc) return rc;
                }
                // Riding pack: where this iteration's merge will ride in the next local launch (h->deferral, same
                // conditions as icem_plan_iter_merge's fold) and that launch is a single-launch kernel, the pack rides
                // there too, as its workgroup 0.  Stashed; the next icem_plan_iter_local consumes it (or launches it).
                // (the step's LAST pack: stashed for the merge that waits for its records -- pack_merge_kernel, one launch)
                const int fuse_last = opt_i(OPT_PACK_MERGE);
                const bool rides_next = !last && it + 1 < c.opt_iters;
                if (fold_push && xchg_concurrent_peers(h) && h->deferral && (rides_next || (last && fuse_last)) && lists > 0 && records_fit_prologue(h)) {
                    const int n_next = rides_next ? shard_of(h, it + 1).n_loc : 0;
                    if (!rides_next || (prologue_possible(h, cx.hint, n_next) && next_launch_takes_pack(h, cx.hint, n_next))) {
                        h->ride.pack = make_pack(pk, sh, (float*)rec, px);
                        h->ride.pack_pending = true;
                        return ICEM_OK;
                    }
                }
                {
                    ProfScope prof(h, ICEM_K_LOCAL_PACK, lists * K, st);
                    launch_pack_records(pk, n_loc, lo, (float*)rec, st, px);
                }
                ICEM_HIP_TRY(hipGetLastError());
                if (xchg_connected(h) && !fold_push) return xchg_push(h, rec, st, &h->xw_last);
            }
            ICEM_HIP_TRY(hipGetLastError());
            return ICEM_OK;
        }
    }
    // generic path (f64, external noise, shapes outside the fast list): one kernel per stage
    int rc = gk_sample(h, n_loc, lo, b->mean, b->std, b->low, b->high, b->z_r, b->z_i, base + (uint64_t)it, 0, row0,
                       actions, cx);
    if (rc) return rc;
    rc = gk_rollout(h, n_loc + n_extra, b->obs0, actions, b->costs, nullptr, cx);
    if (rc) return rc;
    h->local.sel_cand = 0;
    if (c.world == 1 && gk_select_ok(h, n_cand, h->n_reuse, K)) {
        // one GPU: nothing to exchange -- the merge call selects straight from the cost array (select_refit_kernel)
        h->local.sel_cand = n_cand;
        h->local.sel_loc = n_loc;
        return ICEM_OK;
    }
    if (cx.rec) return no_batched_form(cx, "the three-launch selection has no batched form");
    const int nblk = std::max(1, topk_blocks(n_cand));
    rc = gk_topk_partial(h, n_cand, K, b->costs, b->workspace, nblk, st);
    if (rc) return rc;
    rc = gk_local_pack(h, nblk, K, n_loc, lo, n_global, b->workspace, actions, rec, st);
    if (rc) return rc;
    if (c.world > 1 && xchg_connected(h)) return xchg_push(h, rec, st, &h->xw_last);
    return ICEM_OK;
}

template <typename T>
int plan_iter_merge_t(icem_handle* h, const icem_plan_buffers* b, int mpc_step, int it, const LaunchCtx& cx, MergeRoute route) {
    hipStream_t st = cx.st;
    const icem_config& c = h->cfg;
    const int K = c.num_elites;
    const MergeArgsV a = merge_args<T>(h, b, mpc_step, it, route);
    if constexpr (std::is_same<T, float>::value) {
        if (c.world == 1 && h->local.lists > 0) {  // lists form: the candidate lists of this GPU's own rollout
            MergeSingleArgs m = zeroed_args<MergeSingleArgs>();
            m.keep_base = -1;
            fill_single(m, a);
            m.n_lists = h->local.lists;
            // iteration 0: shifted elites that sit behind the list-writing workgroups (sample_rollout_lists) come in
            // through the kept-elite slot: costs from the cost array, rows from the pool (index n_global + e < n_pool)
            if (it == 0 && h->local.tail_rows > 0) {
                m.n_keep = h->local.tail_rows;
                m.elites_cost_cur = (const float*)b->costs + h->pop[it];
            }
            m.n_pool = h->pop[it] + shift_rows(h, mpc_step, it, false);
            m.part_k = (const unsigned long long*)b->workspace;
            m.actions = (const float*)b->actions;
            m.dbg = h->dbg;
            if (route.defer && !m.last) {  // rides in the next iteration's launch (icem_plan_step)
                h->ride.merge = m;
                h->ride.merge_pending = true;
                return ICEM_OK;
            }
            if (h->ride.pack_pending) {  // (cannot happen at world == 1; kept symmetrical)
                const int rc = launch_pending_pack(h, cx);
                if (rc) return rc;
            }
            ProfScope prof(h, ICEM_K_MERGE_REFIT, h->local.lists * K + m.n_keep, st);
            if (h->ahead.tail_pending && merge_noise_ok(m, c.rng_rounds)) {
                launch_merge_noise(cx, m, h->ahead.tail_args, h->ahead.tail2_args);  // + (the rest of) the next step's first noise
                h->ahead.tail_pending = false;
            } else {
                launch_merge_single(cx, m);
            }
            ICEM_HIP_TRY(hipGetLastError());
            return ICEM_OK;
        }
        if (h->local.lists > 0 && records_fit_prologue(h)) {
            // records form -- f32 throughput path: the selection / refit code of the single-GPU merge on the records
            MergeSingleArgs m{};
            fill_single(m, a);
            m.records = (const float*)a.records;
            m.xw = a.xw;
            m.n_rec = a.n_rec;
            if (route.defer && !a.last) {  // rides in the next iteration's launch
                h->ride.merge = m;
                h->ride.merge_pending = true;
                return ICEM_OK;
            }
            const int fuse_on = opt_i(OPT_PACK_MERGE);
            if (h->ride.pack_pending && fuse_on && m.records != nullptr && xchg_connected(h)) {
                // the merge runs now, and so must the pack whose records it waits for: ONE launch for the two
                const PackPrev& pp = h->ride.pack;
                ProfScope prof(h, ICEM_K_MERGE_REFIT, a.n_rec + a.n_keep, st);
                launch_pack_merge(pack_launch_args(h, pp), pp.n_loc, pp.shard_lo, pp.records, pp.px, m, st);
                ICEM_HIP_TRY(hipGetLastError());
                h->ride.pack_pending = false;
                return ICEM_OK;
            }
            if (h->ride.pack_pending) {  // (records gathered by a collective between the two: separate launches)
                const int rc = launch_pending_pack(h, cx);
                if (rc) return rc;
            }
            ProfScope prof(h, ICEM_K_MERGE_REFIT, a.n_rec + a.n_keep, st);
            launch_merge_single(cx, m);
            ICEM_HIP_TRY(hipGetLastError());
            return ICEM_OK;
        }
    }
    if (h->ride.pack_pending) {
        const int rc = launch_pending_pack(h, cx);
        if (rc) return rc;
    }
    if (c.world == 1 && h->local.sel_cand > 0 && h->local.lists == 0) {
        const int n_cand = h->local.sel_cand;
        h->local.sel_cand = 0;
        return gk_select_refit(h, n_cand, h->local.sel_loc, b->costs, b->actions, a, cx);
    }
    if (cx.rec) return no_batched_form(cx, "the records merge has no batched form");
    return gk_merge_refit(h, a, st);
}


// ---------------------------------------------------------------------------------------------------------------------
// Noise-ahead pipeline (world == 1, f32, device noise, every iteration's rollout launch >= 4 waves per workgroup)
// ---------------------------------------------------------------------------------------------------------------------
// icem.py:73-79 draws the colored noise first and applies `* std + mean` afterwards: only the affine map depends on the
// previous iteration.  So an iteration is ONE launch (iter_ahead_kernel, k_rollout_ahead.hip): its rollout workgroups run
// the previous iteration's merge in their prologue, map the raw noise of the pool to actions as they load it, roll out
// and emit candidate lists; its noise workgroups draw the NEXT sampling call's noise (iteration i + 1, or iteration 0 of
// the next MPC step) into the next pool beside them; at iteration 0 one more workgroup builds and rolls out the shifted
// elites (icem.py:131-137), which reach the merge through the cost array as in the single-launch kernel's tail shape.
// One stream, six launches per MPC step at five iterations (ten on the default path).  Buffers: the last iteration's
// pool is the caller's `actions`; the others rotate through three pools of the handle.
// The first form of this pipeline drew the noise on a second stream: every cross-stream event wait cost 10-15 us on the
// critical path and a low-priority side stream starved the rollouts (profiles/r03_noise_ahead_*; EXPERIMENTS.md).

void ahead_destroy(icem_handle* h) {
    icem_handle::Ahead& A = h->ahead;
    for (void*& p : A.pool) {
        if (p) (void)hipFree(p);
        p = nullptr;
    }
    if (A.pre_raw) (void)hipFree(A.pre_raw);
    A = icem_handle::Ahead();
}

static bool ahead_eligible(icem_handle* h, const icem_plan_buffers* b, const BatchHint& bh, bool sharded = false) {
    icem_handle::Ahead& A = h->ahead;
    const icem_config& c = h->cfg;
    if (A.disabled < 0) {
        // on by default where it applies (measured 1.09-1.21x the sampler + rollout pair from N = 32 768 to 262 144;
        // option noise_ahead = 0 switches it off -- latched per handle at its first step: the equivalence test and
        // tools/ahead_bench.py flip it between planners)
        A.disabled = opt_i(OPT_NOISE_AHEAD) == 0 ? 1 : 0;
        A.min_rows = opt_i(OPT_NOISE_AHEAD_MIN_ROWS);
    }
    if (A.disabled || (c.world != 1) != sharded || c.dtype != ICEM_F32 || b->z_r != nullptr || !h->use_fast || gemm_rollout(h) ||
        c.opt_iters < 2 || c.rng_rounds != 10)
        return false;
    const int stamps_on = opt_i(OPT_AHEAD_STAMPS);
    if (h->dbg != nullptr && !stamps_on) return false;   // (another kernel is under study; option ahead_stamps = 1: this path's phase stamps)
    if (!fast_rollout_ok(h, c.num_elites) || !fast_sample_ok(h)) return false;
    if (sharded) {
        // peers in processes of their own (the pack rides in the next launch), records that fit the pack's LDS stage and
        // the records merge's two-per-lane layout, the published merge switched on
        const int on = opt_i(OPT_NOISE_AHEAD_SHARDED);
        if (!on || !xchg_connected(h) || !xchg_concurrent_peers(h) || !pack_can_push(c.num_elites, c.horizon, c.act_dim) ||
            !records_fit_prologue(h))
            return false;
    }
    for (size_t it = 0; it < h->pop.size(); ++it) {
        const int n = sharded ? shard_of(h, (int)it).n_loc : h->pop[it];
        if (n < A.min_rows || !rollout_ahead_ok(bh, c.horizon, c.act_dim, h->Of, c.num_elites, n)) return false;
    }
    if (c.shift_elites && h->n_reuse > 16) return false;  // (the shift role rolls its rows out as one 16-row tile)
    // the transform takes the bounds as two scalars: fetch them once per (low, high) buffer pair
    if (A.lo_ptr != b->low || A.hi_ptr != b->high) {
        std::vector<float> lo(c.act_dim), hi(c.act_dim);
        if (hipMemcpy(lo.data(), b->low, lo.size() * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(hi.data(), b->high, hi.size() * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) {
            (void)hipGetLastError();
            return false;
        }
        A.lo_ptr = b->low;
        A.hi_ptr = b->high;
        A.uniform = true;
        for (int j = 1; j < c.act_dim; ++j) A.uniform = A.uniform && lo[j] == lo[0] && hi[j] == hi[0];
        A.lo = lo[0];
        A.hi = hi[0];
    }
    return A.uniform;
}

static int ahead_setup(icem_handle* h) {
    icem_handle::Ahead& A = h->ahead;
    if (A.pool[0]) return ICEM_OK;
    for (void*& p : A.pool) ICEM_HIP_TRY(hipMalloc(&p, icem_plan_buffer_bytes(h, ICEM_BUF_ACTIONS)));
    if (!h->ws_alt) ICEM_HIP_TRY(hipMalloc(&h->ws_alt, icem_plan_buffer_bytes(h, ICEM_BUF_WORKSPACE)));
    if (!h->pp_stats) ICEM_HIP_TRY(hipMalloc((void**)&h->pp_stats, (size_t)4 * h->hd * sizeof(float)));
    return ICEM_OK;
}

// What the pipeline's two forms (one GPU: plan_step_ahead; a rank of a sharded run: plan_step_sharded_ahead) share:
// set-up, the pool rotation, the step's first noise and arming the next step's, the arguments of the roles, the merge routing.
struct AheadStep {
    icem_handle* h;
    const icem_plan_buffers* b;
    int mpc_step;
    LaunchCtx cx;
    const char* name;
    uint64_t base = 0;
    float* cur_mean = nullptr;  // where the current distribution lives
    float* cur_std = nullptr;

    int begin() {
        int rc = ahead_setup(h);
        if (rc) return rc;
        rc = ensure_fast_model(h);
        if (rc) return rc;
        base = call_base(h, mpc_step);
        cur_mean = (float*)b->mean;
        cur_std = (float*)b->std;
        return ICEM_OK;
    }
    // the last iteration's pool is the caller's `actions`; the others rotate through the handle's three
    float* pool_of(int it) const {
        return it == h->cfg.opt_iters - 1 ? (float*)b->actions : (float*)h->ahead.pool[(h->ahead.ctr + (unsigned)it) % 3];
    }
    // ... and the pool that iteration 0 of the NEXT MPC step will find at its pool_of(0)
    void* next_step_pool(unsigned it = 0) const { return h->ahead.pool[(h->ahead.ctr + (unsigned)(h->cfg.opt_iters - 1) + it) % 3]; }
    // rows [first_index, first_index + n) of the sampling call `off`, raw, -> out
    FastSampleArgs noise_args(int n, long long first_index, uint64_t off, void* out) const {
        return fast_sample_args(h, n, first_index, nullptr, nullptr, nullptr, nullptr, off, 0, out, 0, nullptr, 0);
    }
    // iteration `it`'s buffers: its pool, and the distribution where the previous merge left it
    icem_plan_buffers buffers(int it) const {
        icem_plan_buffers bb = *b;
        bb.actions = pool_of(it);
        bb.mean = cur_mean;
        bb.std = cur_std;
        return bb;
    }
    // this step's first noise: drawn by the previous step's last launch -- or, for a step nobody predicted, here
    int first_noise(Shard sh, float* pool, bool* hit_out) {
        icem_handle::Ahead& A = h->ahead;
        const bool hit = A.next_valid && A.next_episode == h->episode && A.next_step == mpc_step && A.next_pool == pool &&
                         A.next_stream == cx.st;   // (another stream is not ordered behind the launch that drew it: a miss)
        A.next_valid = false;
        if (!hit) {   // (issued at once also while a batch records: it writes this handle's own pool, in front of the batch's launches)
            const FastSampleArgs za = noise_args(sh.n_loc, sh.lo, base, pool);
            ProfScope prof(h, ICEM_K_SAMPLE, (long long)sh.n_loc * h->cfg.horizon, cx.st);
            launch_noise_rows(za, h->cfg.rng_rounds, cx.st);
        }
        ICEM_HIP_TRY(hipGetLastError());
        *hit_out = hit;
        return ICEM_OK;
    }
    // ... and the next step's, which this step's last launch draws into `np` (same episode, step + 1 -- checked when it comes)
    void arm_next(void* np) {
        icem_handle::Ahead& A = h->ahead;
        A.next_valid = true;
        A.next_episode = h->episode;
        A.next_step = mpc_step + 1;
        A.next_pool = np;
        A.next_stream = cx.st;
    }
    // the rollout role of iteration `it`: map the shard's raw noise of bb.actions with the current distribution, roll out
    void roll_role(IterAheadArgs& ia, int it, Shard sh, const icem_plan_buffers& bb) const {
        const icem_config& c = h->cfg;
        ia.r = fast_rollout_args(h, sh.n_loc, sh.n_loc, c.num_elites, b->obs0, bb.actions, b->costs, nullptr, nullptr);
        ia.r.part_k = (unsigned long long*)bb.workspace;
        ia.n_xf = sh.n_loc;
        ia.row0_mean = (it == c.opt_iters - 1 && c.use_mean_actions && sh.lo == 0) ? 1 : 0;
        ia.pool = (float*)bb.actions;
        ia.mean = cur_mean;
        ia.std = cur_std;
        ia.lo = h->ahead.lo;
        ia.hi = h->ahead.hi;
    }
    // the shift role (icem.py:91-104, 131-137): rows [n, n + rows) of this pool, costs behind costs[n]
    void shift_role(IterAheadArgs& ia, int n, float* pool, int rows) const {
        if (rows <= 0) return;
        const icem_config& c = h->cfg;
        // (the elite buffer holding the previous step's set)
        const float* src = (const float*)b->elites + (size_t)elite_parity(h, mpc_step, 0) * c.num_elites * h->hd;
        ia.s = fast_sample_args(h, n, 0, cur_mean, cur_std, b->low, b->high, base, 0, pool, rows, src, base + (uint64_t)c.opt_iters);
    }
    int launch(const IterAheadArgs& ia, int n) {
        const icem_config& c = h->cfg;
        {
            ProfScope prof(h, ICEM_K_SAMPLE_ROLLOUT, (long long)n * c.horizon, cx.st);
            launch_iter_ahead(cx, ia, c.horizon, c.act_dim, h->Of, h->model_kind);
        }
        ICEM_HIP_TRY(hipGetLastError());
        h->local.lists = ahead_roll_workgroups(cx.hint, n);
        return ICEM_OK;
    }
    // iteration `it`'s merge: stashed for the next launch, its distribution going to the handle's ping-pong pair, or (last) launched
    int merge(const icem_plan_buffers& bb, int it) {
        const MergeRoute route = merge_route(h, b, it, true);
        const int rc = plan_iter_merge_t<float>(h, &bb, mpc_step, it, cx, route);
        if (rc || it == h->cfg.opt_iters - 1) return rc;
        if (!h->ride.merge_pending) return fail(ICEM_E_STATE, std::string(name) + ": the merge did not defer");
        cur_mean = route.mean_out;
        cur_std = route.std_out;
        return ICEM_OK;
    }
    void end() { h->ahead.ctr += (unsigned long long)(h->cfg.opt_iters - 1); }
};

static int plan_step_ahead(icem_handle* h, const icem_plan_buffers* b, int mpc_step, const LaunchCtx& cx) {
    icem_handle::Ahead& A = h->ahead;
    const icem_config& c = h->cfg;
    const int iters = c.opt_iters, hd = h->hd;
    AheadStep s{h, b, mpc_step, cx, "noise-ahead"};
    int rc = s.begin();
    if (rc) return rc;
    const int n_extra = shift_rows(h, mpc_step, 0);
    int n1_done = 0;   // rows of iteration 1's noise that are there already
    for (int it = 0; it < iters; ++it) {
        const bool last = it == iters - 1;
        const int n = h->pop[it];
        icem_plan_buffers bb = s.buffers(it);
        if (it & 1) bb.workspace = h->ws_alt;
        float* pool = (float*)bb.actions;
        if (it == 0) {
            bool hit = false;
            rc = s.first_noise({0, n}, pool, &hit);
            if (rc) return rc;
            // the head of iteration 1's noise may have been drawn beside the previous step's last merge as well
            n1_done = (hit && iters > 1 && A.next1_pool == s.pool_of(1)) ? std::min(A.next1_rows, h->pop[1]) : 0;
            A.next1_rows = 0;
        }
        IterAheadArgs ia = zeroed_args<IterAheadArgs>();
        ia.m.keep_base = -1;
        s.roll_role(ia, it, {0, n}, bb);
        ia.dbg_slot = it;
        ia.has_merge = h->ride.merge_pending ? 1 : 0;
        if (h->ride.merge_pending) ia.m = h->ride.merge;
        h->ride.merge_pending = false;
        ia.store_back = last ? 1 : 0;
        // the noise role: the next sampling call
        if (!last) {
            const int skip = it == 0 ? n1_done : 0;
            ia.z = s.noise_args(h->pop[it + 1] - skip, skip, s.base + (uint64_t)(it + 1), s.pool_of(it + 1) + (size_t)skip * hd);
        } else {
            // iteration 0 of the NEXT MPC step
            // -- split: what fits beside this launch's rollout here, the rest beside the step's last merge, a launch that
            // leaves 255 of the 256 CUs idle (ICEM_AHEAD_TAIL_FRAC: share of the rows that goes there)
            void* np = s.next_step_pool();
            const uint64_t off0 = call_base(h, mpc_step + 1);
            const double tail_frac = opt(OPT_AHEAD_TAIL_FRAC);
            int n_tail = (int)(tail_frac * h->pop[0]);
            n_tail = std::max(0, std::min(h->pop[0], n_tail));
            const int n_here = h->pop[0] - n_tail;
            ia.z = s.noise_args(n_here, 0, off0, np);
            A.tail_pending = n_tail > 0;
            A.tail2_args = zeroed_args<FastSampleArgs>();
            A.tail2_args.n = 0;
            if (n_tail > 0) {
                A.tail_args = s.noise_args(n_tail, n_here, off0, (float*)np + (size_t)n_here * hd);
                // ... and the head of the next step's iteration-1 noise, into the pool that step will find at pool_of(1)
                // (this step's iteration-2 pool: its last reader was iteration 3's prologue) -- ICEM_AHEAD_NEXT1_FRAC of it
                const double frac1 = opt(OPT_AHEAD_NEXT1_FRAC);
                const int n1 = iters > 2 ? std::max(0, std::min(h->pop[1], (int)(frac1 * h->pop[1]))) : 0;
                if (n1 > 0) {
                    void* np1 = s.next_step_pool(1);
                    A.tail2_args = s.noise_args(n1, 0, off0 + 1u, np1);
                    A.next1_rows = n1;
                    A.next1_pool = np1;
                }
            }
            s.arm_next(np);
        }
        if (it == 0) s.shift_role(ia, n, pool, n_extra);
        rc = s.launch(ia, n);
        if (rc) return rc;
        h->local.tail_rows = it == 0 ? n_extra : 0;
        // ---- its merge: stashed for the next launch's prologue, or (last) a launch of its own ----
        rc = s.merge(bb, it);
        if (rc) return rc;
        if (last && A.tail_pending) {  // (the merge could not take it along: launches of their own)
            if (cx.rec) return no_batched_form(cx, "the next step's noise found no merge to ride with");   // (they would run AHEAD of the recorded launches)
            launch_noise_rows(A.tail_args, c.rng_rounds, cx.st);
            if (A.tail2_args.n > 0) launch_noise_rows(A.tail2_args, c.rng_rounds, cx.st);
            ICEM_HIP_TRY(hipGetLastError());
            A.tail_pending = false;
        }
        if (!last) {
            h->ride.merge.n_raw = n;  // this pool keeps its noise: the next prologue maps the elite rows among rows [0, n)
            h->ride.merge.xf_lo = A.lo;
            h->ride.merge.xf_hi = A.hi;
        }
    }
    s.end();
    return ICEM_OK;
}

// The same pipeline for one rank of a sharded run (world > 1, in-library exchange connected, peers in processes of their
// own).  Per iteration ONE local launch: workgroup 0 packs + pushes the PREVIOUS iteration's K records and runs the
// launch's one records merge for everybody (published mean | std), the rollout workgroups wait for that flag, map and
// roll out this rank's shard, the noise workgroups draw the shard's next noise; rank 0 alone builds and rolls out the
// (replicated) shifted elites.  Every pool is written back (the record pack gathers actions).  The last iteration's
// pack and merge share one launch of their own, as on the sampler + rollout path.
static int plan_step_sharded_ahead(icem_handle* h, const icem_plan_buffers* b, int mpc_step, const LaunchCtx& cx) {
    const icem_config& c = h->cfg;
    const int iters = c.opt_iters, K = c.num_elites, hd = h->hd;
    AheadStep s{h, b, mpc_step, cx, "noise-ahead (sharded)"};
    int rc = s.begin();
    if (rc) return rc;
    rc = ensure_pub(h, cx.st);
    if (rc) return rc;
    const int n_extra = shift_rows(h, mpc_step, 0);
    float* rec = (float*)b->records + (size_t)c.rank * K * (hd + 2);
    PackPrev pack{};        // the previous iteration's pack, riding in this iteration's launch
    bool pack_pending = false;
    for (int it = 0; it < iters; ++it) {
        const bool last = it == iters - 1;
        const Shard sh = shard_of(h, it);
        const icem_plan_buffers bb = s.buffers(it);
        float* pool = (float*)bb.actions;
        if (it == 0) {
            bool hit = false;
            rc = s.first_noise(sh, pool, &hit);
            if (rc) return rc;
        }
        const int tail = (it == 0 && c.rank == 0) ? n_extra : 0;  // shifted elites: rank 0 submits them (they are replicated)
        IterAheadArgs ia{};
        s.roll_role(ia, it, sh, bb);
        ia.store_back = 1;
        if (it > 0) {
            if (!h->ride.merge_pending || !pack_pending) return fail(ICEM_E_STATE, "noise-ahead (sharded): merge / pack not stashed");
            ia.has_merge = 2;
            ia.m = h->ride.merge;
            ia.p = pack;
            set_pub(h, ia.p);
            h->ride.merge_pending = false;
            pack_pending = false;
        }
        // the noise role: the shard's rows of the next sampling call, or (last) of iteration 0 of the NEXT MPC step
        const Shard nx = shard_of(h, last ? 0 : it + 1);
        if (!last) {
            ia.z = s.noise_args(nx.n_loc, nx.lo, s.base + (uint64_t)(it + 1), s.pool_of(it + 1));
        } else {
            void* np = s.next_step_pool();
            ia.z = s.noise_args(nx.n_loc, nx.lo, call_base(h, mpc_step + 1), np);
            s.arm_next(np);
        }
        s.shift_role(ia, sh.n_loc, pool, tail);
        rc = s.launch(ia, sh.n_loc);
        if (rc) return rc;
        h->local.tail_rows = 0;
        // ---- this iteration's pack: stashed for the next launch's workgroup 0, or (last) for the merge below, which takes
        // it along in its own launch (pack_merge_kernel) ----
        const MergeSingleArgs pk = local_pack_args(h, it, h->local.lists, sh.n_loc + tail, b->workspace, pool, sh.n_loc, tail, b->costs);
        XchgPush px;
        rc = xchg_begin(h, &px, &h->xw_last);
        if (rc) return rc;
        if (!last) {
            pack = make_pack(pk, sh, rec, px);
            pack_pending = true;
        } else {
            h->ride.pack = make_pack(pk, sh, rec, px);
            h->ride.pack_pending = true;
        }
        // ---- its merge (records form): stashed for the next launch's pack role, or (last) a launch with the pack ----
        rc = s.merge(bb, it);
        if (rc) return rc;
        if (!last && h->ride.merge.records == nullptr) return fail(ICEM_E_STATE, "noise-ahead (sharded): the merge did not defer");
    }
    s.end();
    return ICEM_OK;
}

// Small populations (the single-launch kernel serves iteration 0): the raw colored noise of the NEXT MPC step's first
// sampling call -- and of its shifted elites' call -- needs neither the observation nor the distribution (icem.py:73-79),
// so it is drawn beside THIS step's last merge, the one launch that leaves 255 CUs idle (merge_noise_kernel), into a
// buffer of the handle; iteration 0 of the next step then only maps it (FastSampleArgs::raw_src).  Same sample_row, same
// map: same bits as sampling in place.  Arms h->ahead.tail_args for plan_iter_merge_t's last launch.
void predraw_next_step(icem_handle* h, const icem_plan_buffers* b, int mpc_step, const LaunchCtx& cx) {
    icem_handle::Ahead& A = h->ahead;
    const icem_config& c = h->cfg;
    const int on = opt_i(OPT_PREDRAW);
    A.pre_valid = false;
    if (!on || c.world != 1 || c.dtype != ICEM_F32 || b->z_r != nullptr || !h->use_fast || gemm_rollout(h) || c.rng_rounds != 10 ||
        h->dbg != nullptr || h->local.lists <= 0 || c.num_elites + 1 > 12 || !fast_rollout_ok(h, c.num_elites) || !fast_sample_ok(h))
        return;
    const int n0 = h->pop[0];
    // (measured: N = 1000 66.7 -> 64.9, N = 4096 67.9 -> 65.9 us per MPC step; 8192 unchanged; at 16 384 the noise outlasts
    //  the merge it rides with, 89.4 -> 91.1: up to 8192 rows)
    if (n0 > 8192) return;
    const int n_shift = shift_rows(h, mpc_step + 1, 0);
    if (n_shift * c.act_dim > 256) return;
    int tail_rows = 0;
    if (one_launch_lists(h, cx.hint, n0 + n_shift, n_shift, &tail_rows) <= 0) return;
    if (!A.pre_raw && hipMalloc(&A.pre_raw, (size_t)(n0 + h->n_reuse + 16) * h->hd * sizeof(float)) != hipSuccess) {
        (void)hipGetLastError();
        A.pre_raw = nullptr;
        return;
    }
    const uint64_t base_next = call_base(h, mpc_step + 1);
    A.tail_args = fast_sample_args(h, n0, 0, nullptr, nullptr, nullptr, nullptr, base_next, 0, A.pre_raw, 0, nullptr, 0);
    A.tail2_args = fast_sample_args(h, n_shift, 0, nullptr, nullptr, nullptr, nullptr, base_next + (uint64_t)c.opt_iters, 0,
                                    (float*)A.pre_raw + (size_t)n0 * h->hd, 0, nullptr, 0);
    A.tail_pending = true;
    A.pre_valid = true;
    A.pre_episode = h->episode;
    A.pre_step = mpc_step + 1;
    A.pre_stream = cx.st;
}

}  // namespace icem

extern "C" {

size_t icem_plan_buffer_bytes(const icem_handle* h, int32_t which) {
    if (!h) return 0;
    const size_t ts = h->tsize, hd = (size_t)h->hd, K = (size_t)h->cfg.num_elites;
    const size_t rows = (size_t)h->n_local_max + (size_t)h->n_reuse;
    switch (which) {
        case ICEM_BUF_MEAN:
        case ICEM_BUF_STD:
            return hd * ts;
        case ICEM_BUF_LOW:
        case ICEM_BUF_HIGH:
        case ICEM_BUF_EXECUTED:
            return (size_t)h->cfg.act_dim * ts;
        case ICEM_BUF_OBS0:
            return (size_t)std::max(1, h->obs_dim) * ts;
        case ICEM_BUF_ACTIONS:
            return rows * hd * ts;
        case ICEM_BUF_COSTS:
            return rows * ts;
        case ICEM_BUF_ELITES:
            return 2 * K * hd * ts + 2 * K * ts;
        case ICEM_BUF_RECORDS:
            return (size_t)h->cfg.world * K * (hd + 2) * ts;
        case ICEM_BUF_WORKSPACE:
            return (size_t)std::max(topk_blocks((int)rows), 1024) * K * (ts + sizeof(int));
        case ICEM_BUF_BEST_COST:
            return ts;
        default:
            return 0;
    }
}

static int check_plan(icem_handle* h, const icem_plan_buffers* b, int32_t mpc_step, int32_t it, hipStream_t st = nullptr) {
    if (check_handle(h)) return ICEM_E_INVALID;
    if (!b) return fail(ICEM_E_INVALID, "null buffers");
    if (!h->has_model || !h->has_cost) return fail(ICEM_E_STATE, "icem_set_model / icem_set_cost must be called first");
    if (mpc_step < 0 || it < 0 || it >= h->cfg.opt_iters) return fail(ICEM_E_INVALID, "mpc_step / iteration out of range");
    if (const char* e = cost_indices_error(h, h->obs_dim)) return fail(ICEM_E_INVALID, e);
    if (const char* e = wide_unsupported(h, h->cfg.num_elites, b->z_r != nullptr, false)) return fail(ICEM_E_UNSUPPORTED, e);
    if (!b->mean || !b->std || !b->low || !b->high || !b->obs0 || !b->actions || !b->costs || !b->elites || !b->records ||
        !b->workspace || !b->executed || !b->best_cost)
        return fail(ICEM_E_INVALID, "null plan buffer");
    if (h->cfg.noise_beta > 0 &&
        ((b->z_r == nullptr) != (b->z_i == nullptr) || (b->z_r_shift == nullptr) != (b->z_i_shift == nullptr)))
        return fail(ICEM_E_INVALID, "z_r/z_i must be given in pairs");
    // fp16-plane tile arithmetic: the launch's scale needs the action bounds' magnitude -- fetched once per (low, high) pair
    // (and at every icem_reset_distribution: abi.hip::refresh_act_mag)
    if (h->tile_arith || h->hn_tile) return refresh_act_mag(h, b->low, b->high, st, false);
    return ICEM_OK;
}

static int ensure_pp_stats(icem_handle* h) {
    if (!h->pp_stats) ICEM_HIP_TRY(hipMalloc((void**)&h->pp_stats, (size_t)4 * h->hd * sizeof(float)));
    return ICEM_OK;
}

// world > 1 with merge deferral: the running step's distribution is at cur_mean / cur_std
static bool deferral_active(const icem_handle* h, const icem_plan_buffers* b) {
    return h->deferral && h->cfg.world > 1 && h->cfg.dtype == ICEM_F32 && b->z_r == nullptr && h->use_fast;
}

int icem_set_merge_deferral(icem_handle* h, int32_t on) {
    if (check_handle(h)) return ICEM_E_INVALID;
    if (h->ride.merge_pending) return fail(ICEM_E_STATE, "a deferred merge is pending: finish the MPC step first");
    h->deferral = on != 0;
    return ICEM_OK;
}

int icem_plan_iter_local(icem_handle* h, const icem_plan_buffers* b, int32_t mpc_step, int32_t it, void* stream) {
    int rc = check_plan(h, b, mpc_step, it, (hipStream_t)stream);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    icem_plan_buffers bb = *b;
    if (deferral_active(h, b)) {
        if (it == 0 || !h->cur_mean) {
            h->cur_mean = (float*)b->mean;
            h->cur_std = (float*)b->std;
        }
        bb.mean = h->cur_mean;
        bb.std = h->cur_std;
    }
    const LaunchCtx cx{st};
    return ICEM_DISPATCH(h, plan_iter_local_t<float>(h, &bb, mpc_step, it, cx), plan_iter_local_t<double>(h, &bb, mpc_step, it, cx));
}

// icem_plan_iter_merge with the merge's route given (icem_plan_step folds merges at world == 1 too)
static int plan_iter_merge_routed(icem_handle* h, const icem_plan_buffers* b, int32_t mpc_step, int32_t it, const LaunchCtx& cx, MergeRoute route) {
    const int rc = check_plan(h, b, mpc_step, it, cx.st);
    if (rc) return rc;
    return ICEM_DISPATCH(h, plan_iter_merge_t<float>(h, b, mpc_step, it, cx, route), plan_iter_merge_t<double>(h, b, mpc_step, it, cx, route));
}

int icem_plan_iter_merge(icem_handle* h, const icem_plan_buffers* b, int32_t mpc_step, int32_t it, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    const bool deferred = h && b && deferral_active(h, b) && h->cur_mean;
    const LaunchCtx cx{st};
    if (!deferred) return plan_iter_merge_routed(h, b, mpc_step, it, cx, MergeRoute());  // launched now, in place
    int rc = check_plan(h, b, mpc_step, it, st);
    if (rc) return rc;
    // sharded, deferral on: a non-last merge may ride in the next icem_plan_iter_local launch (mean / std / elites in
    // the caller's buffers are then current again only after that launch; the last merge always runs here)
    rc = ensure_pp_stats(h);
    if (rc) return rc;
    const bool last = it == h->cfg.opt_iters - 1;
    const bool fold = !last && h->local.lists > 0 && records_fit_prologue(h) && prologue_possible(h, cx.hint, shard_of(h, it + 1).n_loc);
    icem_plan_buffers bb = *b;
    bb.mean = h->cur_mean;
    bb.std = h->cur_std;
    const MergeRoute route = merge_route(h, b, it, fold);
    rc = plan_iter_merge_t<float>(h, &bb, mpc_step, it, cx, route);
    if (rc) return rc;
    if (fold && h->ride.merge_pending) {
        h->cur_mean = route.mean_out;
        h->cur_std = route.std_out;
    }
    if (last) h->cur_mean = h->cur_std = nullptr;
    return ICEM_OK;
}

// A step that failed half way must not leave arguments armed for a later step's launches (stale merge / pack / noise
// arguments would reach kernels with buffers of a step that never completed).
static void disarm(icem_handle* h) {
    h->ride.clear();
    h->local.clear();
    h->ahead.tail_pending = h->ahead.next_valid = h->ahead.pre_valid = false;
    h->ahead.next1_rows = 0;
}
static int disarm_on_error(icem_handle* h, int rc) {
    if (rc != ICEM_OK) disarm(h);
    return rc;
}

static int plan_step_sharded_body(icem_handle* h, const icem_plan_buffers* b, int32_t mpc_step, void* stream) {
    if (h->cfg.world < 2) return icem_plan_step(h, b, mpc_step, stream);
    if (!xchg_connected(h) && !rccl_connected(h))
        return fail(ICEM_E_STATE, "neither the in-library exchange (icem_exchange_create / _connect) nor an RCCL communicator "
                                  "(icem_rccl_connect / _adopt) is connected");
    if (b && b->z_r != nullptr) return fail(ICEM_E_INVALID, "external noise goes through icem_plan_iter_local / _merge");
    // A merge of an earlier step gave up waiting for a peer's records (bounded waits): that step's elites, mean and
    // action are garbage and differ between ranks.  The status word is host memory -- this check costs one load.
    if (xchg_status_peek(h) & 1u)
        return fail(ICEM_E_STATE, "in-library exchange: a wait for a peer's elite records timed out in an earlier MPC step "
                                  "(icem_exchange_status reads and clears the word); the plans since then are not valid");
    if (b && check_plan(h, b, mpc_step, 0, (hipStream_t)stream) == ICEM_OK && !h->ride.merge_pending && !h->ride.pack_pending && ahead_eligible(h, b, BatchHint(), true))
        return plan_step_sharded_ahead(h, b, mpc_step, LaunchCtx{(hipStream_t)stream});
    const bool was = h->deferral;
    h->deferral = true;  // non-last merges ride in the next local launch
    int rc = ICEM_OK;
    const bool by_rccl = !xchg_connected(h);  // the pack left this rank's K records in b->records: gather them in place
    for (int it = 0; it < h->cfg.opt_iters && rc == ICEM_OK; ++it) {
        rc = icem_plan_iter_local(h, b, mpc_step, it, stream);
        if (rc == ICEM_OK && by_rccl) rc = rccl_allgather_records(h, b->records, (hipStream_t)stream);
        if (rc == ICEM_OK) rc = icem_plan_iter_merge(h, b, mpc_step, it, stream);
    }
    h->deferral = was;
    return rc;
}

int icem_plan_step_sharded(icem_handle* h, const icem_plan_buffers* b, int32_t mpc_step, void* stream) {
    if (check_handle(h)) return ICEM_E_INVALID;
    return disarm_on_error(h, plan_step_sharded_body(h, b, mpc_step, stream));
}

static int plan_step_body(icem_handle* h, const icem_plan_buffers* b, int32_t mpc_step, const LaunchCtx& cx) {
    if (h->cfg.world != 1) return fail(ICEM_E_INVALID, "icem_plan_step is the world == 1 path; use iter_local/iter_merge");
    int rc = check_plan(h, b, mpc_step, 0, cx.st);
    if (rc) return rc;
    const icem_config& c = h->cfg;
    const int iters = c.opt_iters;
    if (ahead_eligible(h, b, cx.hint)) return plan_step_ahead(h, b, mpc_step, cx);
    // f32, device noise: iteration it's merge may ride in the prologue of iteration it+1's launch.  That launch
    // reads pool / lists / distribution of iteration it while writing its own, so consecutive iterations alternate
    // between the caller's buffers and the handle's partners (the last iteration always uses the caller's).
    const bool pingpong = c.dtype == ICEM_F32 && b->z_r == nullptr && h->use_fast && iters > 1;
    if (pingpong && !h->actions_alt) ICEM_HIP_TRY(hipMalloc(&h->actions_alt, icem_plan_buffer_bytes(h, ICEM_BUF_ACTIONS)));
    if (pingpong && !h->ws_alt) ICEM_HIP_TRY(hipMalloc(&h->ws_alt, icem_plan_buffer_bytes(h, ICEM_BUF_WORKSPACE)));   // (ahead_setup may own one already)
    if (pingpong) {
        rc = ensure_pp_stats(h);
        if (rc) return rc;
    }
    float* cur_mean = (float*)b->mean;  // where the current distribution lives
    float* cur_std = (float*)b->std;
    for (int it = 0; it < iters; ++it) {
        icem_plan_buffers bb = *b;
        if (pingpong) {
            if ((iters - 1 - it) & 1) bb.actions = h->actions_alt;
            if (it & 1) bb.workspace = h->ws_alt;
            bb.mean = cur_mean;
            bb.std = cur_std;
        }
        // (world == 1: no deferral across calls, and check_plan above holds for every iteration of the step)
        rc = ICEM_DISPATCH(h, plan_iter_local_t<float>(h, &bb, mpc_step, it, cx), plan_iter_local_t<double>(h, &bb, mpc_step, it, cx));
        if (rc) return rc;
        const bool last = it == iters - 1;
        if (last) predraw_next_step(h, b, mpc_step, cx);  // small populations: the next step's first noise rides with the last merge
        bool fold = false;
        if (pingpong && !last && h->local.lists > 0) fold = prologue_possible(h, cx.hint, h->pop[it + 1]);
        const MergeRoute route = merge_route(h, b, it, fold);
        rc = ICEM_DISPATCH(h, plan_iter_merge_t<float>(h, &bb, mpc_step, it, cx, route), plan_iter_merge_t<double>(h, &bb, mpc_step, it, cx, route));
        if (rc) return rc;
        if (last && h->ahead.tail_pending) {  // the merge that ran was not one that takes noise along: no noise was drawn
            h->ahead.tail_pending = false;
            h->ahead.pre_valid = false;
        }
        if (fold && h->ride.merge_pending) {
            cur_mean = route.mean_out;
            cur_std = route.std_out;
        }
    }
    return ICEM_OK;
}

int icem_plan_step(icem_handle* h, const icem_plan_buffers* b, int32_t mpc_step, void* stream) {
    if (check_handle(h)) return ICEM_E_INVALID;
    return disarm_on_error(h, plan_step_body(h, b, mpc_step, LaunchCtx{(hipStream_t)stream}));
}


// ---------------------------------------------------------------------------------------------------------------------
// icem_plan_step_batch: B independent planners, one launch per stage for all of them
// ---------------------------------------------------------------------------------------------------------------------
// The reference runs several controllers side by side (parallel episodes: icem/misc/rollout_utils.py:46-58, 129-152), each
// its own get_action (icem.py:106-189).  At the metric's population (N = 4096) one problem leaves the chip mostly empty and a
// step is a chain of six launch latencies; B problems of one configuration share those six launches: the host side of
// every handle runs exactly as for icem_plan_step -- same buffers, same ping-pong, same noise offsets -- under a launch
// context whose recorder takes every launch (key + argument block; a launcher without a batched form launches nothing and
// has the batch refused), then every stage is ONE launch with blockIdx.y = the problem and the
// blocks in a device array (one upload per step, skipped when nothing but the step number changed: the offsets are stored
// relative to the step's base, which travels in the kernel arguments).  Slab sizes are chosen for all rows together.
// does this handle's step consist of single-launch iterations with merge prologues and one last merge? (the path
// decisions of plan_step_body / plan_iter_local_t / plan_iter_merge_t, evaluated without launching anything)
static const char* batch_ineligible(icem_handle* h, const icem_plan_buffers* b, int32_t mpc_step, const BatchHint& bh) {
    const icem_config& c = h->cfg;
    const int K = c.num_elites;
    if (c.world != 1) return "world must be 1";
    if (c.dtype != ICEM_F32 || !h->use_fast) return "dtype f32 on the throughput kernels only";
    if (b->z_r || b->z_i || b->z_r_shift || b->z_i_shift) return "external noise is not batched";
    if (h->profiling || h->dbg) return "per-kernel profiling / debug stamps are per handle: switch them off";
    const bool gemm = gemm_rollout(h) && !h->hn_tile;   // the GEMM-kernel shapes: wide observations, and the narrow ones no tile kernel serves
    if (!fast_rollout_ok(h, K) || !fast_sample_ok(h) || K + 1 > 12 || c.rng_rounds != 10)
        return (h->hn_tile || gemm) ? "the merge cannot ride in the sampler's prologue (num_elites <= 11, the default generator)" : "shape outside the single-launch kernels";
    if (h->ride.merge_pending || h->ride.pack_pending) return "a deferred merge is pending: finish the MPC step first";
    if (c.opt_iters < 1) return "opt_iters";
    // (TileHN shapes are compiled at h = 30; the GEMM kernels take any horizon, the batched merge-prologue sampler does not)
    if (gemm && !sample_batch_compiled(c.horizon)) return "the batched samplers of a GEMM-kernel shape are compiled for horizon 30 only";
    if (h->hn_tile || gemm) {
        // sampler (shifted elites in its extra workgroup; from iteration 1 on the previous merge in its prologue) + TileHN or GEMM
        // rollout (exact f32 tiles with the row-by-row tail behind them, or the 16-bit planes) per iteration, then the last merge:
        // the path decisions of plan_iter_local_t for these handles
        if (h->pop.empty() || h->pop[0] > 8192) return "populations above 8192 rows per iteration are not batched: they fill the chip by themselves";
        if (shift_rows(h, mpc_step, 0, false) * c.act_dim > 256) return "too many shifted elites for the sampling launch";
        if (c.opt_iters > 1 && !sample_folded_merge_ok(c.horizon, c.act_dim, c.rng_rounds, K))
            return "an iteration cannot carry the previous merge in its prologue";
        return nullptr;
    }
    // (bh: the shapes below are the batch's.)  Where every iteration's rows of ALL problems together fill the
    // noise-ahead launch (>= 4 waves per rollout workgroup), the batch takes that path -- rollout, next noise and shifted elites
    // as roles of one launch (k_rollout_ahead.hip), 107 against 130 us per step at eight problems of 4096 rows -- provided a
    // problem ALONE does not take it (a population above 8192 rows fills the chip by itself: not batched)
    if (ahead_eligible(h, b, BatchHint()))
        return "populations that take the noise-ahead launches alone (> 8192 rows per iteration) are not batched: they fill the chip by themselves";
    if (ahead_eligible(h, b, bh)) return nullptr;   // (false without bh.ahead: option batch_ahead = 0)
    for (int it = 0; it < c.opt_iters; ++it) {
        const int n_extra = shift_rows(h, mpc_step, it, false);
        if (n_extra * c.act_dim > 256) return "too many shifted elites for the sampling launch";
        if (one_launch_lists(h, bh, h->pop[it] + n_extra, n_extra) <= 0) return "an iteration's population has no single-launch kernel";
        if (it > 0 && !prologue_possible(h, bh, h->pop[it])) return "an iteration cannot carry the previous merge in its prologue";
    }
    return nullptr;
}

// What the batched entries share behind their admission: the host side of every problem's step under a recorder, then the
// recorded-launch plan (recorded_batch.h: comparison, placement, copy, launch) with the blob in handles[0]'s six-slot array.
// who: the entry's name for messages; spare: room a new array gets beyond the first blob (a later step's blob may be larger:
// shifted elites -- so the room is this rule, not the layout's); *launches_out: the kernel launches issued.
static int run_recorded_batch(icem_handle* const* handles, int n, const icem_plan_buffers* buffers, int32_t mpc_step, hipStream_t st,
                              const BatchHint& hint, const std::string& who, size_t spare, long long* launches_out) {
    // ---- the host side of every problem's step, recorded ----
    // From here on the handles' host state runs ahead of the device: whatever return leaves before the last launch is
    // enqueued takes every handle's armed state with it.
    struct DisarmGuard {
        icem_handle* const* handles;
        int n;
        bool armed = true;
        ~DisarmGuard() {
            for (int i = 0; armed && i < n; ++i) disarm(handles[i]);
        }
    } disarm_all{handles, n};
    BatchBases bases{};   // each problem's noise stream base of this step: the recorded blocks' offsets are relative to it
    RecordedBatch rb(n);
    bool unsupported = false;
    for (int i = 0; i < n; ++i) {
        LaunchRecorder& rec = rb.recs[i];
        rec.base = bases.v[i] = call_base(handles[i], mpc_step);
        rec.who = who.c_str();
        rec.launches.reserve(3 * handles[i]->cfg.opt_iters + 2);   // (the float64 step's count; the f32 plans record 2 * iters + 1)
        if (int rc = plan_step_body(handles[i], &buffers[i], mpc_step, LaunchCtx{st, hint, &rec})) return rc;
        unsupported = unsupported || rec.unsupported;
    }
    if (unsupported) return fail(ICEM_E_UNSUPPORTED, who + "a launch without a batched form was reached");
    if (int rc = rb.check(who)) return rc;   // nothing was launched: the handles' half-armed state goes
    // ---- argument blocks: one array per launch ----
    BlockLayout layout(n, ICEM_MAX_BATCH);
    rb.place(layout);
    const size_t bytes = layout.bytes();
    std::vector<unsigned char> blob(bytes, 0);
    for (int i = 0; i < n; ++i) rb.copy(i, blob.data());
    icem_handle* owner = handles[0];
    const int slot = mpc_step % 6;
    if (opt_i(OPT_AHEAD_STAMPS) && owner->batch_args.holds(slot).size() == bytes) {   // development: which bytes moved
        const std::vector<unsigned char>& held = owner->batch_args.holds(slot);
        int shown = 0;
        for (size_t l = 0; l < rb.launches() && shown < 12; ++l) {
            const size_t one = rb.block_bytes(l);
            for (size_t o = 0; o < one * (size_t)n && shown < 12; ++o)
                if (blob[rb.at[l] + o] != held[rb.at[l] + o]) {
                    std::fprintf(stderr, "batch args changed: step %d launch %zu kind %d problem %zu byte %zu\n", mpc_step, l, rb.key(l).family, o / one, o % one);
                    ++shown;
                    o = (o / 8 + 1) * 8 - 1;
                }
        }
    }
    ICEM_HIP_TRY(owner->batch_args.put(slot, blob, bytes + spare, st, &owner->batch_uploads));
    // ---- the launches ----
    long long launches = 0;
    if (int rc = rb.launch((const unsigned char*)owner->batch_args.dev(slot), bases, st, &launches)) return rc;
    disarm_all.armed = false;
    if (launches_out) *launches_out = launches;
    return ICEM_OK;
}

extern "C" int icem_plan_step_batch(icem_handle* const* handles, int32_t n, const icem_plan_buffers* buffers, int32_t mpc_step, void* stream) {
    if (int rc = admit_batch(handles, n, buffers != nullptr, false, "",
                             "icem_plan_step_batch: the handles must share one configuration (horizon, act_dim, populations, elites, flags)"))
        return rc;
    if (n == 1) return icem_plan_step(handles[0], &buffers[0], mpc_step, stream);
    hipStream_t st = (hipStream_t)stream;
    // (one configuration; models, costs, seeds, bounds, observations differ)
    const icem_handle* h0 = handles[0];
    for (int i = 0; i < n; ++i) {
        icem_handle* h = handles[i];
        int rc = check_plan(h, &buffers[i], mpc_step, 0, st);
        if (rc) return rc;
        if (h->Of != h0->Of || h->model_kind != h0->model_kind || h->tile_arith != h0->tile_arith)
            return fail(ICEM_E_INVALID, "icem_plan_step_batch: the handles must share the model's width and kind and the tile arithmetic");
        // (a handle that is not on the TileHN kernel beside one that is: refused below, as unsupported)
        if (h->hn_tile && h0->hn_tile && (h->obs_dim != h0->obs_dim || std::memcmp(h->hn_prog, h0->hn_prog, sizeof(h->hn_prog)) != 0))
            return fail(ICEM_E_INVALID, "icem_plan_step_batch: TileHN handles must share the observation width and the compiled term program");
        // GEMM-kernel handles: one launch serves all problems, so one instantiation -- width, kind (above), arithmetic in effect, term list or none
        const bool g = gemm_rollout(h) && !h->hn_tile, g0 = gemm_rollout(h0) && !h0->hn_tile;
        if (g && g0 && (h->obs_dim != h0->obs_dim || h->wide_eff != h0->wide_eff || h->has_terms != h0->has_terms))
            return fail(ICEM_E_INVALID, "icem_plan_step_batch: GEMM-kernel handles must share the observation width, the wide arithmetic in effect "
                                        "(icem_wide_arith) and all or none carry icem_cost_terms");
        if ((g && h0->hn_tile) || (h->hn_tile && g0))
            return fail(ICEM_E_UNSUPPORTED, "icem_plan_step_batch: a TileHN handle and a GEMM-kernel handle take different rollout launches and cannot share a batch");
    }
    // the batch's shape hint.  The noise-ahead launches from where they measure faster than the single-launch kernels: 12 problems
    // of 4096 rows (160 against 161 us per step; 16: 194 against 212; 8: 129 against 128; 6: 115 against 100 -- EXPERIMENTS R6.3)
    BatchHint hint;
    hint.mult = n;
    hint.ahead = opt_i(OPT_BATCH_AHEAD) != 0 && (double)n * (double)(h0->pop.empty() ? 0 : h0->pop[0]) >= opt(OPT_BATCH_AHEAD_MIN_ROWS);
    for (int i = 0; i < n; ++i)
        if (const char* why = batch_ineligible(handles[i], &buffers[i], mpc_step, hint))
            return fail(ICEM_E_UNSUPPORTED, std::string("icem_plan_step_batch: ") + why);
    return run_recorded_batch(handles, n, buffers, mpc_step, st, hint, "icem_plan_step_batch: ", 4096, nullptr);
}

extern "C" int64_t icem_batch_uploads(const icem_handle* h) { return h ? (int64_t)h->batch_uploads : 0; }

// ---------------------------------------------------------------------------------------------------------------------
// icem_plan_step_batch_f64: the same for planners in the strict-parity arithmetic (the generic kernels)
// ---------------------------------------------------------------------------------------------------------------------
// A world-1 float64 step is, per iteration, gk_sample + gk_rollout + gk_select_refit, and in a step with shifted elites
// gk_shift_elites + the t_begin = h - 1 sampler in front of iteration 0: seventeen dependent launches at five iterations, two of
// them a single workgroup.  Their launchers record under a LaunchCtx like the f32 ones (families LAUNCH_GK_*), the batched kernels
// (k_generic_batch.hip) run the solo kernels' bodies (generic_dev.h) on the block of problem blockIdx.y.
// The path decisions of plan_iter_local_t / plan_iter_merge_t and of the generic launchers for a float64 handle, evaluated without
// launching anything: does every launch of this handle's step have a batched twin?
static const char* batch_f64_ineligible(const icem_handle* h, const icem_plan_buffers* b, int32_t mpc_step) {
    const icem_config& c = h->cfg;
    if (c.world != 1) return "world must be 1 (sharded handles are not batched)";
    if (b->z_r || b->z_i || b->z_r_shift || b->z_i_shift) return "external noise is not batched";
    if (h->profiling || h->dbg) return "per-kernel profiling / debug stamps are per handle: switch them off";
    if (opt_i(OPT_GK_SAMPLE) == 0 || opt_i(OPT_GK_ROLLOUT_THREAD) != 0 || opt_i(OPT_GK_SELECT) == 0)
        return "the development options gk_sample / gk_rollout_thread / gk_select must be at their defaults: the batch mirrors the default kernels";
    if (c.act_dim > WG / 4 || (long long)c.num_traj * c.act_dim > 262144) return "the sampler's one-thread-per-row form (num_traj * act_dim > 262144) is not batched";
    if (c.opt_iters < 1 || h->pop.empty()) return "opt_iters";
    if (!(h->O == 8 || h->O == 16 || h->O == 17 || h->O == 18 || h->O == 24 || h->O == 32)) return "the generic rollout is compiled for padded observation widths 8, 16, 17, 18, 24, 32 only";
    if (h->has_terms && !gk_rollout_thread_batched(h->O, h->model_kind))
        return "the thread-form rollout at padded width 32 with a tanh model has no batched instantiation (register budget)";
    for (int it = 0; it < c.opt_iters; ++it) {
        if (h->pop[it] > 8192) return "populations above 8192 rows per iteration are not batched";
        if (!gk_select_ok(h, h->pop[it] + shift_rows(h, mpc_step, it), h->n_reuse, c.num_elites))
            return "an iteration's pool takes the three-launch selection, which is not batched";
    }
    return nullptr;
}

extern "C" int icem_plan_step_batch_f64(icem_handle* const* handles, int32_t n, const icem_plan_buffers* buffers, int32_t mpc_step, void* stream) {
    const std::string who = "icem_plan_step_batch_f64: ";
    if (int rc = admit_batch(handles, n, buffers != nullptr, false, "",
                             "icem_plan_step_batch_f64: the handles must share one configuration (horizon, act_dim, populations, elites, flags, dtype)"))
        return rc;
    if (handles[0]->cfg.dtype != ICEM_F64) return fail(ICEM_E_UNSUPPORTED, who + "dtype f64 only (f32 handles: icem_plan_step_batch)");
    if (n == 1) return icem_plan_step(handles[0], &buffers[0], mpc_step, stream);
    hipStream_t st = (hipStream_t)stream;
    const icem_handle* h0 = handles[0];
    for (int i = 0; i < n; ++i) {
        icem_handle* h = handles[i];
        if (h->cfg.world != 1) return fail(ICEM_E_UNSUPPORTED, who + "world must be 1 (sharded handles are not batched)");
        if (h->f64_arith == ICEM_F64_MFMA)
            return fail(ICEM_E_UNSUPPORTED, who + "handles on ICEM_F64_MFMA are not batched (the f64 matrix-core rollout has no batched twin)");
        int rc = check_plan(h, &buffers[i], mpc_step, 0, st);
        if (rc) return rc;
        if (h->O != h0->O || h->model_kind != h0->model_kind || h->has_terms != h0->has_terms)
            return fail(ICEM_E_INVALID, who + "the handles must share the model's padded width and kind, and all or none carry icem_cost_terms "
                                              "(the term list decides the rollout kernel)");
    }
    for (int i = 0; i < n; ++i)
        if (const char* why = batch_f64_ineligible(handles[i], &buffers[i], mpc_step)) return fail(ICEM_E_UNSUPPORTED, who + why);
    BatchHint hint;
    hint.mult = n;
    long long launches = 0;
    const int rc = run_recorded_batch(handles, n, buffers, mpc_step, st, hint, who, 8192, &launches);
    if (rc == ICEM_OK) handles[0]->batch_f64_launches = launches;
    return rc;
}

extern "C" int64_t icem_batch_f64_launches(const icem_handle* h) { return h ? (int64_t)h->batch_f64_launches : 0; }

// MpcICem.get_action as one call for a host caller: observation in, executed action (+ its pool's best cost) out.
// The handle owns a small pinned, device-mapped block [obs | action, best cost | flag].  On the f32 fast path the first
// launch reads the observation straight from it (no H2D copy command in front of the step) and a one-thread kernel
// behind the last merge writes the result and a sequence flag into it, which the host polls (no D2H copy commands,
// no stream synchronisation wake-up).  Other configurations stage through the same block with copy commands.
int icem_get_action(icem_handle* h, const icem_plan_buffers* b, int32_t mpc_step, const double* obs_host,
                    double* action_host, double* best_cost_host, void* stream) {
    if (check_handle(h)) return ICEM_E_INVALID;
    if (!b || !obs_host || !action_host) return fail(ICEM_E_INVALID, "null argument");
    if (!h->has_model) return fail(ICEM_E_STATE, "icem_set_model / icem_set_cost must be called first");
    hipStream_t st = (hipStream_t)stream;
    const int o = h->obs_dim, d = h->cfg.act_dim;
    const size_t ts = h->tsize;
    constexpr size_t OUT_OFF = ICEM_MAX_OBS_DIM * sizeof(double), FLAG_OFF = OUT_OFF + (ICEM_MAX_ACT_DIM + 1) * sizeof(double);
    if (!h->host_stage) {
        ICEM_HIP_TRY(hipHostMalloc(&h->host_stage, FLAG_OFF + 64, hipHostMallocMapped | hipHostMallocCoherent));
        std::memset(h->host_stage, 0, FLAG_OFF + 64);
        ICEM_HIP_TRY(hipHostGetDevicePointer(&h->host_stage_dev, h->host_stage, 0));
    }
    unsigned char* stage = (unsigned char*)h->host_stage;
    for (int k = 0; k < o; ++k) {
        if (h->cfg.dtype == ICEM_F64) ((double*)stage)[k] = obs_host[k];
        else ((float*)stage)[k] = (float)obs_host[k];
    }
    unsigned char* out = stage + OUT_OFF;
    volatile unsigned* flag = (volatile unsigned*)(stage + FLAG_OFF);
    const bool mapped = h->cfg.dtype == ICEM_F32 && h->use_fast && b->z_r == nullptr && fast_rollout_ok(h, h->cfg.num_elites) &&
                        fast_sample_ok(h);
    icem_plan_buffers bb = *b;
    if (mapped) {
        std::atomic_thread_fence(std::memory_order_release);
        bb.obs0 = h->host_stage_dev;
    } else {
        ICEM_HIP_TRY(hipMemcpyAsync(b->obs0, stage, o * ts, hipMemcpyHostToDevice, st));
    }
    const int rc = icem_plan_step(h, &bb, mpc_step, stream);
    if (rc) return rc;
    if (mapped) {
        // (publishing from inside the last merge kernel instead was tried: no faster than this one-wave launch)
        const unsigned seq = ++h->io_seq;
        unsigned char* dev = (unsigned char*)h->host_stage_dev;
        hipLaunchKernelGGL(publish_result_kernel, dim3(1), dim3(128), 0, st, (const float*)b->executed, (const float*)b->best_cost,
                           (const unsigned*)h->nonfinite_dev, d, (float*)(dev + OUT_OFF), (unsigned*)(dev + FLAG_OFF), seq);
        ICEM_HIP_TRY(hipGetLastError());
        long long spins = 0;
        while (*flag != seq) {
            __builtin_ia32_pause();
            if (++spins > (1ll << 26)) {  // ~ a second: something is wrong on the stream -- let the runtime report it
                ICEM_HIP_TRY(hipStreamSynchronize(st));
                if (*flag != seq) return fail(ICEM_E_HIP, "result flag never arrived");
            }
        }
        std::atomic_thread_fence(std::memory_order_acquire);
    } else {
        ICEM_HIP_TRY(hipMemcpyAsync(out, b->executed, d * ts, hipMemcpyDeviceToHost, st));
        ICEM_HIP_TRY(hipMemcpyAsync(out + (size_t)d * ts, b->best_cost, ts, hipMemcpyDeviceToHost, st));
        ICEM_HIP_TRY(hipMemcpyAsync(out + (size_t)(d + 1) * ts, h->nonfinite_dev, sizeof(unsigned), hipMemcpyDeviceToHost, st));
        ICEM_HIP_TRY(hipStreamSynchronize(st));
    }
    unsigned nonfinite_now = 0;
    std::memcpy(&nonfinite_now, out + (size_t)(d + 1) * ts, sizeof(unsigned));
    for (int j = 0; j <= d; ++j) {
        const double v = h->cfg.dtype == ICEM_F64 ? ((const double*)out)[j] : (double)((const float*)out)[j];
        if (j < d) action_host[j] = v;
        else if (best_cost_host) *best_cost_host = v;
    }
    // Trajectories of THIS step whose cost left a tile kernel non-finite although the observation was finite: a state left
    // the arithmetic's range (f32's, or -- actions outside the bounds the scale was taken from -- the fp16 planes'), where
    // the reference's float64 ranks a finite cost (icem.py:147-159, 199).  The action is returned, and so is the fact.
    const unsigned fresh = nonfinite_now - h->nonfinite_seen;
    h->nonfinite_seen = nonfinite_now;
    if (fresh != 0) {
        bool obs_finite = true;
        for (int k = 0; k < o; ++k) obs_finite = obs_finite && std::isfinite(obs_host[k]);
        if (obs_finite)
            return fail(ICEM_E_RANGE, std::to_string(fresh) + " trajectories of this MPC step came back with a non-finite cost from a finite "
                        "observation: a state left the range of the rollout's arithmetic (icem_tile_arith / icem_tile_growth); the "
                        "reference's float64 ranks finite costs there -- use ICEM_TILE_F32 / dtype f64 for this model");
    }
    return ICEM_OK;
}

}  // extern "C"
