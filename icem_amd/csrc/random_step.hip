// random_step.hip -- the MPC step of the random-shooting baseline (MpcRandom.get_action, icem/controllers/mpc.py:114-138) as one
// C call: icem_plan_step_random.  The step is the operator chain of MpcRandomHip.get_action (icem_amd/controllers.py) as three
// stages with nothing between them:
//   sample   random_sample_kernel (k_random.hip): icem_sample_piecewise's pool at the caller's call offset
//   rollout  rollout_cost_launch (abi.hip): the launch icem_rollout_cost picks for the handle
//   select   random_select_kernel (k_random.hip): icem_topk_sorted(costs, 1), the best row's gather, result
// The arguments go by value.  The entry keeps no step state: the call offset (MpcRandom's counter of sample() calls) is the caller's.
//
// icem_plan_step_random_batch is the same step for B planners of one configuration, every stage ONE launch for all of them:
// random_sample_batch_kernel, the batched twin of the handles' rollout launch (the recorded-launch plan, recorded_batch.h),
// random_select_batch_kernel.  The argument blocks live in a DeviceArgArray of the first handle, laid out by block_layout.h, and carry
// no step-dependent value (the call offsets travel by value): a batch whose buffers stay put uploads them once.
//
// icem_plan_step_random_learned / icem_plan_step_random_learned_batch are the same step through the learned dynamics (the declared
// RSSM, BASELINE configs[4]): the sampler and the selection above around launch_rssm_rollout (one problem) / launch_rssm_split_batch
// (several, their rows back to back in the learned step's pool of the first handle, icem_plan_step_cem_learned_batch's arrangement).
// Unlike the CEM step's, a problem's own pool is NOT scratch here -- a controller keeps it (MpcRandomHip._last_actions / _last_costs)
// -- so the batch's sampler and selection (k_random_learned.hip) work on the pool's slices and mirror the rows they store and the
// costs they read into the problem's own buffers: 3 launches whatever B, every buffer of every problem its solo step's.
//
// icem_plan_step_random_learned_models is that batched step for problems that roll out through models of their own (an ensemble's
// members, a trained model per controller): random_learned_step_batch with the rollout ONE launch_rssm_split_models of n * members
// problems in member-major order (step_models.h, shared with learned_step.hip) and the selection
// random_select_members_batch_kernel (k_random_members.hip), which reduces the members' costs on the way to its keys -- still 3 launches.  One problem
// works in its own actions / costs.
#include "random_step.h"
#include "icem_rssm.h"
#include "recorded_batch.h"
#include "step_models.h"

using namespace icem;

namespace {

// "who is served" (nullptr: this handle is)
const char* random_unserved(const icem_handle* h) {
    const icem_config& c = h->cfg;
    if (opt_i(OPT_RANDOM_STEP) == 0) return "option random_step is 0";
    if (c.world != 1) return "world must be 1";
    if (h->profiling) return "per-kernel profiling is per launch of one operator: switch it off";
    if (h->dbg) return "debug stamps are per launch of one operator: switch them off";
    if (c.rng_rounds != 7 && c.rng_rounds != 10) return "rng_rounds must be 7 or 10";
    if (c.dtype == ICEM_F32 && c.num_traj > (1 << 24)) return "f32: result holds the best index as a float, exact up to num_traj = 2^24";
    return nullptr;
}

static_assert(rssm::DET + rssm::STOCH == ICEM_RSSM_OBS_DIM, "the RSSM's observation width");

// "who is served" through the learned dynamics: the step above, f32 at the RSSM's action width, rolled out by the RSSM's split launch
const char* random_learned_unserved(const icem_handle* h) {
    const icem_config& c = h->cfg;
    if (c.dtype != ICEM_F32) return "the learned-dynamics rollout is f32 only";
    // (a handle bound to an RSSM of its own width -- icem_set_rssm_act_dim, which takes no other -- passes; one never bound is served at 6)
    if (c.act_dim != rssm_width(h)) return "the declared RSSM takes 6 action dimensions";
    if (const char* why = random_unserved(h)) return why;
    if (!rssm_split_ok(c.num_traj, c.horizon)) return "the population's tiles exceed the split launch's limit, or the split launch is switched off";
    return nullptr;
}

bool null_buffer(const icem_random_buffers& b) {
    return !b.low || !b.high || !b.obs0 || !b.actions || !b.costs || !b.best_actions || !b.result;
}

// the refusals that read no handle (the entries make them first), then those of one handle's step: all of them before anything
// is launched or the handle touched
int random_arg_refusal(const icem_random_buffers& b, int32_t change_freq, int64_t call_offset, const std::string& who) {
    if (change_freq < 0) return fail(ICEM_E_INVALID, who + "negative change_freq");
    if (call_offset < 0) return fail(ICEM_E_INVALID, who + "negative call_offset");
    if (null_buffer(b)) return fail(ICEM_E_INVALID, who + "null buffer");
    return ICEM_OK;
}
// (learned: through the RSSM -- no built-in model or cost is asked for)
int random_refusal(const icem_handle* h, int32_t change_freq, const std::string& who, bool learned = false) {
    if (change_freq >= h->cfg.horizon) return fail(ICEM_E_INVALID, who + "change_freq must be below the horizon (mpc.py:92)");
    if (const char* why = learned ? random_learned_unserved(h) : random_unserved(h)) return fail(ICEM_E_UNSUPPORTED, who + why);
    if (learned) return ICEM_OK;
    if (!h->has_model || !h->has_cost) return fail(ICEM_E_STATE, who + "icem_set_model / icem_set_cost must be called first");
    if (const char* e = cost_indices_error(h, h->obs_dim)) return fail(ICEM_E_INVALID, e);
    if (const char* e = wide_unsupported(h, 0, false, false)) return fail(ICEM_E_UNSUPPORTED, e);
    return ICEM_OK;
}

// the selection's partials + ticket of a pool of more than one slice: allocated and zeroed once per handle (ordered on `st`
// before the step's launches); every selection launch leaves the ticket at zero
int reserve_ws(icem_handle* h, hipStream_t st) {
    if (random_select_blocks(h->cfg.num_traj) <= 1 || h->random_ws.dev) return ICEM_OK;
    const size_t bytes = random_ws_bytes(h->cfg.num_traj);
    void* p = nullptr;
    ICEM_HIP_TRY(hipMalloc(&p, bytes));
    if (hipError_t e = hipMemsetAsync(p, 0, bytes, st)) {
        (void)hipFree(p);
        ICEM_HIP_TRY(e);
    }
    h->random_ws.dev = p, h->random_ws.bytes = bytes;
    return ICEM_OK;
}

// the argument blocks' room on the host stack (no padding in either; k_random.hip)
struct alignas(8) Block {
    unsigned char bytes[RANDOM_BLOCK_MAX];
};

// one planner's step behind its refusals.  *launches_out: written on success.
// rssm_params: nullptr (the handle's built-in model), or the packed RSSM the rows are rolled out through
int random_step_solo(icem_handle* h, const icem_random_buffers* b, int32_t change_freq, int64_t call_offset, int64_t first_block, const void* u,
                     void* result_row, hipStream_t st, long long* launches_out, const void* rssm_params = nullptr) {
    if (int rc = reserve_ws(h, st)) return rc;
    Block blk;
    std::memset(&blk, 0, sizeof(blk));
    random_sample_block(h, *b, change_freq, call_offset, first_block, u, &blk);
    launch_random_sample(h, &blk, st);
    ICEM_HIP_TRY(hipGetLastError());
    const icem_config& c = h->cfg;
    if (int rc = rssm_params ? rssm_launch_result(launch_rssm_rollout(c.num_traj, c.horizon, c.act_dim, c.cost_mode, (const unsigned short*)rssm_params,
                                                                      (const float*)b->obs0, (const float*)b->actions, (float*)b->costs, st))
                             : rollout_cost_launch(h, c.num_traj, b->obs0, b->actions, b->costs, nullptr, LaunchCtx{st}))
        return rc;
    std::memset(&blk, 0, sizeof(blk));
    random_select_block(h, *b, result_row, &blk);
    launch_random_select(h, &blk, st);
    ICEM_HIP_TRY(hipGetLastError());
    *launches_out = 3;
    return ICEM_OK;
}

// B > 1 planners behind the admission of the batch.  Host state: the first handle's argument array (+ its upload counter) and its
// random_batch_launches, written behind the last launch; each handle's RandomWs (allocated once, whatever happens later).
// Recording a handle's rollout may upload that handle's packed model (idempotent, what its next solo step would do first).
int random_step_batch(icem_handle* const* handles, int n, const icem_random_buffers* buffers, int32_t change_freq, const int64_t* offsets,
                      void* results, hipStream_t st) {
    const std::string who = "icem_plan_step_random_batch: ";
    icem_handle* h0 = handles[0];
    // ---- every problem's rollout launch, recorded and compared (recorded_batch.h) ----
    RecordedBatch rb(n);
    for (int i = 0; i < n; ++i)
        if (int rc = record_rollout(rb, i, handles[i], buffers[i].obs0, buffers[i].actions, buffers[i].costs, st, who)) return rc;
    if (int rc = rb.check(who)) return rc;
    for (int i = 0; i < n; ++i)
        if (int rc = reserve_ws(handles[i], st)) return rc;
    // ---- argument blocks: [sample x n | rollout launch(es) x n | select x n] ----
    const size_t sb = random_sample_block_bytes(h0), ub = random_select_block_bytes(h0);
    BlockLayout layout(n, ICEM_MAX_BATCH);
    layout.add(sb);   // (at 0)
    rb.place(layout);
    const size_t at_select = layout.add(ub);
    std::vector<unsigned char> blob(layout.bytes(), 0);
    BatchBases bases{};
    for (int i = 0; i < n; ++i) {
        const icem_random_buffers& b = buffers[i];
        bases.v[i] = (unsigned long long)offsets[i];
        random_sample_block(handles[i], b, change_freq, 0, 0, nullptr, blob.data() + sb * i);
        rb.copy(i, blob.data());
        random_select_block(handles[i], b, results_row(results, i, (size_t)(h0->cfg.act_dim + 2) * h0->tsize), blob.data() + at_select + ub * i);
    }
    ICEM_HIP_TRY(h0->random_batch_args.put(0, blob, layout.room(), st, &h0->batch_uploads));
    // ---- the launches ----
    const unsigned char* dev = (const unsigned char*)h0->random_batch_args.dev(0);
    long long launches = 0;
    launch_random_sample_batch(h0, dev, bases, n, st);
    ICEM_HIP_TRY(hipGetLastError());
    ++launches;
    if (int rc = rb.launch(dev, BatchBases{}, st, &launches)) return rc;   // (a rollout draws nothing: no bases)
    launch_random_select_batch(h0, dev + at_select, n, st);
    ICEM_HIP_TRY(hipGetLastError());
    ++launches;
    h0->random_batch_launches = launches;
    return ICEM_OK;
}

// B > 1 planners through the RSSM, behind the admission of the batch, the tile check and rssm_split_prepare.  Problem i's rows are
// drawn into the slice [i * N, (i + 1) * N) of the first handle's learned-step pool AND into its own actions, ONE split launch
// scores the pool, the selection reads the slices and leaves every cost in the problem's own costs as well.  Host state: as
// random_step_batch's, and the first handle's pool.
// mo (icem_plan_step_random_learned_models; params == nullptr): every problem rolls out through models of its own -- the rollout is
// ONE launch_rssm_split_models of n * members problems, the selection reduces the members' costs itself; n == 1 then works in the
// problem's own actions / costs (the pool IS those) and its sampler is the built-in step's batched one.
int random_learned_step_batch(icem_handle* const* handles, int n, const icem_random_buffers* buffers, const void* params, int32_t change_freq,
                              const int64_t* offsets, void* results, hipStream_t st, const StepModels* mo = nullptr) {
    icem_handle* h0 = handles[0];
    const icem_config& c = h0->cfg;
    const int N = c.num_traj, hd = h0->hd;
    LearnedCtx& ctx = h0->learned;
    const bool pooled = n > 1;
    if (pooled) ICEM_HIP_TRY(ctx.reserve((size_t)n * N, n, hd, st));
    const RandomPool<float> pool = pooled ? RandomPool<float>{ctx.pool_actions(), ctx.pool_costs(hd)}
                                          : RandomPool<float>{(float*)buffers[0].actions, (float*)buffers[0].costs};
    ObsGather og{};
    og.dst = pooled ? ctx.pool_obs(hd) : (float*)const_cast<void*>(buffers[0].obs0), og.width = ICEM_RSSM_OBS_DIM;
    for (int i = 0; i < n; ++i) og.src[i] = (const float*)buffers[i].obs0;
    float* member_costs = mo ? mo->member_costs : nullptr;
    if (mo && !member_costs) {   // (the members' costs of the rollout: scratch that only grows)
        ICEM_HIP_TRY(ctx.reserve_members((size_t)mo->members * n * N, st));
        member_costs = ctx.member_costs;
    }
    for (int i = 0; i < n; ++i)
        if (int rc = reserve_ws(handles[i], st)) return rc;
    // ---- argument blocks: [sample x n | select x n], those of icem_plan_step_random_batch (the problems' OWN buffers) ----
    const size_t sb = random_sample_block_bytes(h0), ub = random_select_block_bytes(h0);
    BlockLayout layout(n, ICEM_MAX_BATCH);
    layout.add(sb);   // (at 0)
    const size_t at_select = layout.add(ub);
    std::vector<unsigned char> blob(layout.bytes(), 0);
    BatchBases bases{};
    for (int i = 0; i < n; ++i) {
        bases.v[i] = (unsigned long long)offsets[i];
        random_sample_block(handles[i], buffers[i], change_freq, 0, 0, nullptr, blob.data() + sb * i);
        random_select_block(handles[i], buffers[i], results_row(results, i, (size_t)(c.act_dim + 2) * h0->tsize), blob.data() + at_select + ub * i);
    }
    ICEM_HIP_TRY(h0->random_batch_args.put(0, blob, layout.room(), st, &h0->batch_uploads));
    // ---- the launches ----
    const unsigned char* dev = (const unsigned char*)h0->random_batch_args.dev(0);
    if (pooled) launch_random_sample_gather_batch(h0, dev, bases, og, pool, n, st);
    else launch_random_sample_batch(h0, dev, bases, n, st);
    ICEM_HIP_TRY(hipGetLastError());
    const std::vector<int> rows(n, N);
    if (mo) {
        rssm::Problem pr[rssm::BATCH_MAX];
        models_problems(*mo, n, rows.data(), pr);
        if (int rc = rssm_launch_result(launch_rssm_split_models(n * mo->members, pr, c.horizon, c.act_dim, c.cost_mode, og.dst, pool.actions,
                                                                 member_costs, st)))
            return rc;
        launch_random_select_members_batch(h0, dev + at_select, pool, RandomMembers{member_costs, mo->members, mo->reduce, n * N, (float)(1.0 / mo->members)},
                                           n, st);
    } else {
        if (int rc = rssm_launch_result(launch_rssm_split_batch(n, rows.data(), c.horizon, c.act_dim, c.cost_mode, (const unsigned short*)params, og.dst,
                                                                pool.actions, pool.costs, st)))
            return rc;
        launch_random_select_pool_batch(h0, dev + at_select, pool, n, st);
    }
    ICEM_HIP_TRY(hipGetLastError());
    h0->random_batch_launches = 3;
    return ICEM_OK;
}

}  // namespace

extern "C" {

int icem_plan_step_random_ok(const icem_handle* h) { return (h && random_unserved(h) == nullptr) ? 1 : 0; }

int icem_plan_step_random(icem_handle* h, const icem_random_buffers* b, int32_t change_freq, int64_t call_offset, int64_t first_block,
                          const void* u, void* stream) {
    // ---- refusals: all of them before anything is launched or the handle touched ----
    const std::string who = "icem_plan_step_random: ";
    if (!h || !b) return fail(ICEM_E_INVALID, who + "null handle or buffers");
    if (int rc = random_arg_refusal(*b, change_freq, call_offset, who)) return rc;
    if (int rc = random_refusal(h, change_freq, who)) return rc;
    return random_step_solo(h, b, change_freq, call_offset, first_block, u, nullptr, (hipStream_t)stream, &h->random_launches);
}

int icem_plan_step_random_batch(icem_handle* const* handles, int32_t n, const icem_random_buffers* buffers, int32_t change_freq,
                                const int64_t* call_offsets_host, void* results, void* stream) {
    // ---- refusals: all of them before anything is launched or any handle touched ----
    const std::string who = "icem_plan_step_random_batch: ";
    if (int rc = admit_batch(handles, n, buffers && call_offsets_host, true, who.c_str(),
                             "icem_plan_step_random_batch: the handles must share one configuration (everything but the seed)"))
        return rc;
    for (int i = 0; i < n; ++i)
        if (int rc = random_arg_refusal(buffers[i], change_freq, call_offsets_host[i], who)) return rc;
    for (int i = 0; i < n; ++i)
        if (int rc = random_refusal(handles[i], change_freq, who)) return rc;
    if (n == 1)   // one planner: the solo launches (the same bits by construction) + the results row
        return random_step_solo(handles[0], &buffers[0], change_freq, call_offsets_host[0], 0, nullptr, results, (hipStream_t)stream,
                                &handles[0]->random_batch_launches);
    return random_step_batch(handles, n, buffers, change_freq, call_offsets_host, results, (hipStream_t)stream);
}

int icem_plan_step_random_learned_ok(const icem_handle* h) { return (h && random_learned_unserved(h) == nullptr) ? 1 : 0; }

int icem_plan_step_random_learned(icem_handle* h, const icem_random_buffers* b, const void* params, int32_t change_freq, int64_t call_offset,
                                  void* stream) {
    // ---- refusals: all of them before anything is launched or the handle touched ----
    const std::string who = "icem_plan_step_random_learned: ";
    if (!h || !b || !params) return fail(ICEM_E_INVALID, who + "null handle, buffers or params");
    if (int rc = random_arg_refusal(*b, change_freq, call_offset, who)) return rc;
    if (int rc = random_refusal(h, change_freq, who, true)) return rc;
    // the rollout's staging area and its host-visible status word, BEFORE the first launch (as cem_step.hip)
    if (int rc = rssm_launch_result(rssm_split_prepare((h->cfg.num_traj + 15) / 16, h->cfg.horizon, (hipStream_t)stream))) return rc;
    return random_step_solo(h, b, change_freq, call_offset, 0, nullptr, nullptr, (hipStream_t)stream, &h->random_launches, params);
}

int icem_plan_step_random_learned_batch(icem_handle* const* handles, int32_t n, const icem_random_buffers* buffers, const void* params,
                                        int32_t change_freq, const int64_t* call_offsets_host, void* results, void* stream) {
    // ---- refusals: all of them before anything is launched or any handle touched ----
    const std::string who = "icem_plan_step_random_learned_batch: ";
    if (int rc = admit_batch(handles, n, buffers && params && call_offsets_host, true, who.c_str(),
                             "icem_plan_step_random_learned_batch: the handles must share one configuration (everything but the seed)"))
        return rc;
    if (int rc = admit_rssm_binding(handles, n, "icem_plan_step_random_learned_batch: the handles must share one configuration (everything but the seed)"))
        return rc;
    for (int i = 0; i < n; ++i)
        if (int rc = random_arg_refusal(buffers[i], change_freq, call_offsets_host[i], who)) return rc;
    for (int i = 0; i < n; ++i)
        if (int rc = random_refusal(handles[i], change_freq, who, true)) return rc;
    const icem_config& c = handles[0]->cfg;
    const std::vector<int> rows(n, c.num_traj);
    const int tiles = rssm_batch_tiles(n, rows.data());
    if (tiles < 0 || !rssm_split_batch_ok(tiles, c.horizon))
        return fail(ICEM_E_UNSUPPORTED, who + "the batch's tiles (the sum over the problems of ceil(rows / 16)) exceed the split launch's "
                                              "limit; nothing was launched");
    if (int rc = rssm_launch_result(rssm_split_prepare(tiles, c.horizon, (hipStream_t)stream))) return rc;
    if (n == 1)   // one planner: the solo launches (the same bits by construction) + the results row
        return random_step_solo(handles[0], &buffers[0], change_freq, call_offsets_host[0], 0, nullptr, results, (hipStream_t)stream,
                                &handles[0]->random_batch_launches, params);
    return random_learned_step_batch(handles, n, buffers, params, change_freq, call_offsets_host, results, (hipStream_t)stream);
}

// would a batch of n handles like `h` with `members` models per problem be served?
int icem_plan_step_random_learned_models_ok(const icem_handle* h, int32_t n, int32_t members) {
    if (!h || random_learned_unserved(h) || n < 1 || n > ICEM_MAX_BATCH || members < 1 || members > rssm::BATCH_MAX || n * members > rssm::BATCH_MAX)
        return 0;
    const long long tiles = (long long)n * members * ((h->cfg.num_traj + 15) / 16);
    return tiles <= rssm::SPLIT_TILE_LIMIT && rssm_split_batch_ok((int)tiles, h->cfg.horizon) ? 1 : 0;
}

int icem_plan_step_random_learned_models(icem_handle* const* handles, int32_t n, const icem_random_buffers* buffers, int32_t members,
                                         const void* const* params_host, int32_t reduce, int32_t change_freq, const int64_t* call_offsets_host,
                                         void* member_costs, void* results, void* stream) {
    // ---- refusals: all of them before anything is launched or any handle touched ----
    const std::string who = "icem_plan_step_random_learned_models: ";
    const std::string config_msg = who + "the handles must share one configuration (everything but the seed)";
    // (what the counts and the table alone decide comes first: no handle has been looked at when n x members is refused)
    if (int rc = models_args_refusal(who, handles && buffers && call_offsets_host, n, members, params_host, reduce)) return rc;
    if (int rc = admit_batch(handles, n, true, true, who.c_str(), config_msg.c_str())) return rc;
    if (int rc = admit_rssm_binding(handles, n, config_msg.c_str())) return rc;
    for (int i = 0; i < n; ++i)
        if (int rc = random_arg_refusal(buffers[i], change_freq, call_offsets_host[i], who)) return rc;
    for (int i = 0; i < n; ++i)
        if (int rc = random_refusal(handles[i], change_freq, who, true)) return rc;
    const icem_config& c = handles[0]->cfg;
    const StepModels mo{members, reduce, params_host, (float*)member_costs};
    const int tiles = models_tiles_uniform(mo, n, c.num_traj, c.horizon);
    if (tiles < 0)
        return fail(ICEM_E_UNSUPPORTED, who + "the tiles of the rollout (members x the sum over the problems of ceil(num_traj / 16)) exceed the "
                                              "split launch's limit; nothing was launched");
    if (int rc = rssm_launch_result(rssm_split_prepare(tiles, c.horizon, (hipStream_t)stream))) return rc;
    return random_learned_step_batch(handles, n, buffers, nullptr, change_freq, call_offsets_host, results, (hipStream_t)stream, &mo);
}

int64_t icem_random_step_launches(const icem_handle* h) { return h ? (int64_t)h->random_launches : 0; }
int64_t icem_random_batch_launches(const icem_handle* h) { return h ? (int64_t)h->random_batch_launches : 0; }

}  // extern "C"
