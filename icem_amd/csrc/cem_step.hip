// cem_step.hip -- the MPC step of the CEM baseline (MpcCemStd.get_action, icem/controllers/mpc.py:200-262) as one C call:
// icem_plan_step_cem.  The step is the stage-wise loop of MpcCemStdHip.get_action (icem_amd/controllers.py) with every
// iteration three launches and nothing between them:
//   sample   cem_sample_kernel (k_cem.hip): icem_sample_truncnorm's draw at offset (episode << 32) + step * opt_iters + i
//            (sample_truncnorm_kernel itself where a row of the shape does not fit the sampler's LDS)
//   rollout  rollout_cost_launch (abi.hip): the launch icem_rollout_cost picks for the handle
//   update   cem_update_*_kernel (k_cem.hip): icem_update_distribution's body (f32) / the one-launch selection's (f64), then
//            icem_cem_bounds' arithmetic; the last one carries get_action's epilogue
// The arguments go by value: no device-side argument memory, no upload, nothing allocated by the step itself.
//
// icem_plan_step_cem_batch is the same step for B planners of one configuration -- the reference runs its controllers side by side
// (icem/misc/rollout_utils.py:46-58, 129-152) -- with every one of the three launches ONE launch for all of them: cem_sample_batch_kernel,
// the batched twin of the handles' rollout launch (the recorded-launch plan, recorded_batch.h), cem_update_*_batch_kernel.  The argument
// blocks live in a DeviceArgArray of the first handle, laid out by block_layout.h; they carry no step-dependent value (the sampler's
// offset is relative to the step's base, which travels by value), so a batch whose buffers stay put uploads each of its two slots once.
//
// icem_plan_step_cem_learned / icem_plan_step_cem_learned_batch are the same step through the learned dynamics (the declared RSSM,
// BASELINE configs[4]) -- the planner PlaNet uses: the sampler and the update above around launch_rssm_rollout (one problem) /
// launch_rssm_split_batch (several, their rows back to back in the learned step's pool of the first handle, icem_plan_step_learned_batch's
// arrangement).  The refusals, the block filling and the update launch are the ones above.
//
// icem_plan_step_cem_learned_models is that batched step for problems that roll out through models of their own (an ensemble's
// members, a trained model per controller): cem_step_batch with the rollout ONE launch_rssm_split_models of n * members problems in
// member-major order (step_models.h, shared with learned_step.hip) and the update cem_update_members_batch_kernel
// (k_cem_members.hip), which reduces the members' costs while it builds its keys -- still 3 launches per iteration.  One problem
// works in its own actions / costs.
#include "cem_step.h"
#include "icem_rssm.h"
#include "recorded_batch.h"
#include "step_models.h"

using namespace icem;

namespace {

// "who is served" (nullptr: this handle is)
const char* cem_unserved(const icem_handle* h) {
    const icem_config& c = h->cfg;
    const int N = c.num_traj, K = c.num_elites;
    if (opt_i(OPT_CEM_STEP) == 0) return "option cem_step is 0";
    if (c.world != 1) return "world must be 1";
    if (h->profiling) return "per-kernel profiling is per launch of one operator: switch it off";
    if (c.rng_rounds != 7 && c.rng_rounds != 10) return "rng_rounds must be 7 or 10";
    if (c.opt_iters < 1) return "opt_iters";
    // (every iteration draws num_traj rows, mpc.py:207-209: the handle's decaying population sizes play no part)
    if (c.factor_decrease != 1.0) return "MpcCemStd's population does not decay: factor_decrease must be 1";
    if (c.keep_previous_elites || c.shift_elites) return "MpcCemStd neither keeps nor shifts elites: keep_previous_elites and shift_elites must be off";
    if (c.dtype == ICEM_F32) {
        if (!h->use_fast || !topk_small_ok(N, K)) return "f32: the one-launch update does not take this pool / num_elites (icem_update_distribution_ok)";
    } else if (!gk_select_ok(h, N, 0, K)) {
        return "f64: the one-launch selection does not admit this pool / num_elites";
    }
    return nullptr;
}

// The update's blocks, filled member by member into ZEROED memory (the solo launch's locals, a batch's blob): every byte of a
// block is defined, so a batch's blob compares equal as bytes from step to step.  result: the problem's row of a batch's
// `results` (nullptr: the solo entry -- the kernels then write what they always wrote)
template <typename T>
void fill_tail(const icem_handle* h, const icem_cem_buffers& b, const icem_cem_params& p, bool last, void* result, CemTailArgs<T>& t) {
    t.h = h->cfg.horizon, t.d = h->cfg.act_dim;
    t.like_levine = p.like_levine != 0, t.shift_means = p.shift_means != 0, t.execute_best_elite = p.execute_best_elite != 0;
    t.last = last ? 1 : 0;
    t.init_std = (T)h->cfg.init_std;
    t.mean = (T*)b.mean, t.std = (T*)b.std;
    t.low = (const T*)b.low, t.high = (const T*)b.high;
    t.lower = (T*)b.lower, t.upper = (T*)b.upper;
    t.elites = (const T*)b.elites, t.elite_costs = (const T*)b.elite_costs;
    t.executed = (T*)b.executed, t.best_cost = (T*)b.best_cost;
    t.result = (T*)result;
}

// (icem_update_distribution's block, abi.hip: no kept elites)
void fill_update(const icem_handle* h, const icem_cem_buffers& b, const icem_cem_params& p, bool last, void* result, CemUpdateF32Args& g) {
    const icem_config& c = h->cfg;
    UpdateSmallArgs& u = g.u;
    u.costs = (const float*)b.costs, u.pool = (const float*)b.actions, u.keep_costs = nullptr, u.keep_actions = nullptr;
    u.n = c.num_traj, u.n_keep = 0, u.K = c.num_elites, u.hd = h->hd;
    u.alpha = (float)c.alpha;
    u.mean = (float*)b.mean, u.std = (float*)b.std, u.elites_out = (float*)b.elites, u.elite_costs_out = (float*)b.elite_costs;
    u.idx_out = b.elite_idx;
    fill_tail<float>(h, b, p, last, result, g.t);
}

// (gk_select_refit's block, generic_kernels.hip: every row a sampled one, no kept elites, never the step's "last" -- the
//  CEM epilogue is cem_tail's)
void fill_update(const icem_handle* h, const icem_cem_buffers& b, const icem_cem_params& p, bool last, void* result, CemUpdateF64Args& g) {
    const icem_config& c = h->cfg;
    SelectArgs<double>& s = g.s;
    s.n_cand = s.n_loc = c.num_traj;
    s.cap = SELECT_CAP;
    s.costs = (const double*)b.costs;
    s.actions = (const double*)b.actions;
    MergeArgs<double>& a = s.m;
    a.K = c.num_elites, a.h = c.horizon, a.d = c.act_dim, a.n_global = c.num_traj;
    a.alpha = c.alpha, a.init_std = c.init_std;
    a.elites_next = (double*)b.elites, a.elites_cost_next = (double*)b.elite_costs;
    a.mean_in = (const double*)b.mean, a.std_in = (const double*)b.std;
    a.mean = (double*)b.mean, a.std = (double*)b.std;
    a.low = (const double*)b.low, a.high = (const double*)b.high;
    g.idx_out = b.elite_idx;
    fill_tail<double>(h, b, p, last, result, g.t);
}

void launch_update(const icem_handle* h, const icem_cem_buffers& b, const icem_cem_params& p, bool last, void* result, hipStream_t st) {
    if (h->cfg.dtype == ICEM_F32) {
        CemUpdateF32Args g;
        std::memset((void*)&g, 0, sizeof(g));
        fill_update(h, b, p, last, result, g);
        launch_cem_update(g.u, g.t, st);
        return;
    }
    CemUpdateF64Args g;
    std::memset((void*)&g, 0, sizeof(g));
    fill_update(h, b, p, last, result, g);
    launch_cem_update(g.s, g.idx_out, g.t, st);
}

bool null_buffer(const icem_cem_buffers& b) {
    return !b.mean || !b.std || !b.lower || !b.upper || !b.low || !b.high || !b.obs0 || !b.actions || !b.costs || !b.elites ||
           !b.elite_costs || !b.elite_idx || !b.executed || !b.best_cost;
}

static_assert(rssm::DET + rssm::STOCH == ICEM_RSSM_OBS_DIM, "the RSSM's observation width");

// "who is served" through the learned dynamics: the step above, f32 at the RSSM's action width, drawn by the step's own sampler
// (the batch has no other), rolled out by the RSSM's split launch
const char* cem_learned_unserved(const icem_handle* h) {
    const icem_config& c = h->cfg;
    if (c.dtype != ICEM_F32) return "the learned-dynamics rollout is f32 only";
    // (a handle bound to an RSSM of its own width -- icem_set_rssm_act_dim, which takes no other -- passes; one never bound is served at 6)
    if (c.act_dim != rssm_width(h)) return "the declared RSSM takes 6 action dimensions";
    if (const char* why = cem_unserved(h)) return why;
    if (!cem_sample_ok(h)) return "a row of this shape does not fit the step's sampler (its three probability tables and one row in LDS)";
    if (!rssm_split_ok(c.num_traj, c.horizon)) return "the population's tiles exceed the split launch's limit, or the split launch is switched off";
    return nullptr;
}

// the refusals of one handle's step, all of them before anything is launched or the handle touched (who: the entry's name;
// learned: through the RSSM -- no built-in model or cost is asked for)
int cem_refusal(const icem_handle* h, const icem_cem_buffers& b, int32_t mpc_step, const std::string& who, bool learned = false) {
    if (mpc_step < 0) return fail(ICEM_E_INVALID, who + "negative mpc_step");
    if (null_buffer(b)) return fail(ICEM_E_INVALID, who + "null buffer (everything but workspace is needed)");
    if (const char* why = learned ? cem_learned_unserved(h) : cem_unserved(h)) return fail(ICEM_E_UNSUPPORTED, who + why);
    if (learned) return ICEM_OK;
    if (!h->has_model || !h->has_cost) return fail(ICEM_E_STATE, who + "icem_set_model / icem_set_cost must be called first");
    if (const char* e = cost_indices_error(h, h->obs_dim)) return fail(ICEM_E_INVALID, e);
    if (const char* e = wide_unsupported(h, 0, false, false)) return fail(ICEM_E_UNSUPPORTED, e);
    return ICEM_OK;
}

// one planner's step behind its refusals: 3 launches per iteration, the arguments by value.  *launches_out: written on success.
// rssm_params: nullptr (the handle's built-in model), or the packed RSSM the rows are rolled out through
int cem_step_solo(icem_handle* h, const icem_cem_buffers* b, const icem_cem_params* p, int32_t mpc_step, void* result, hipStream_t st,
                  long long* launches_out, const void* rssm_params = nullptr) {
    const icem_config& c = h->cfg;
    const int N = c.num_traj, iters = c.opt_iters;
    const bool own_sampler = cem_sample_ok(h);
    long long launches = 0;
    for (int it = 0; it < iters; ++it) {
        const uint64_t offset = (h->episode << 32) + (uint64_t)mpc_step * (uint64_t)iters + (uint64_t)it;
        int rc = own_sampler ? launch_cem_sample(h, N, b->mean, b->std, b->lower, b->upper, offset, b->actions, st)
                             : gk_sample_truncnorm(h, N, 0, b->mean, b->std, b->lower, b->upper, nullptr, offset, b->actions, st);
        if (rc) return rc;
        ++launches;
        rc = rssm_params ? rssm_launch_result(launch_rssm_rollout(N, c.horizon, c.act_dim, c.cost_mode, (const unsigned short*)rssm_params,
                                                                  (const float*)b->obs0, (const float*)b->actions, (float*)b->costs, st))
                         : rollout_cost_launch(h, N, b->obs0, b->actions, b->costs, nullptr, LaunchCtx{st});
        if (rc) return rc;
        ++launches;
        launch_update(h, *b, *p, it == iters - 1, result, st);
        ICEM_HIP_TRY(hipGetLastError());
        ++launches;
    }
    *launches_out = launches;
    return ICEM_OK;
}

// B > 1 planners behind the admission of the batch (through the RSSM, params != nullptr: and behind the tile check and
// rssm_split_prepare).  Host state: the step keeps none per handle -- no elite double buffer, no pending merge, the noise offsets
// follow from (episode, mpc_step) which the caller owns.  What exists is the first handle's argument array (cem_batch_args + its
// upload counter batch_uploads; a slot that was uploaded holds exactly what its shadow says, whatever happens later), its
// cem_batch_launches, written behind the last launch only, and through the RSSM its learned-step pool.  Recording a handle's rollout
// may upload that handle's packed model (ensure_fast_model: idempotent, what its next solo step would do first).  So a HIP call
// that fails anywhere below leaves every handle as it was.
// mo (icem_plan_step_cem_learned_models; params == nullptr): every problem rolls out through models of its own -- the rollout is
// ONE launch_rssm_split_models of n * members problems, the update reduces the members' costs itself; n == 1 then works in the
// problem's own actions / costs and needs no pool.
int cem_step_batch(icem_handle* const* handles, int n, const icem_cem_buffers* buffers, const icem_cem_params& p, const void* params,
                   const int32_t* steps, void* results, hipStream_t st, const StepModels* mo = nullptr) {
    const std::string who = "icem_plan_step_cem_batch: ";
    icem_handle* h0 = handles[0];
    const icem_config& c = h0->cfg;
    const int N = c.num_traj, iters = c.opt_iters, hd = h0->hd;
    const bool f64 = c.dtype == ICEM_F64;
    // ---- the rollout.  Through the RSSM: problem i's rows are drawn into the slice [i * N, (i + 1) * N) of the first handle's
    // learned-step pool, ONE split launch scores the pool, every update reads its slice; the first sampler launch also gathers the
    // observations into the pool's [n, 230] table.  Else: every problem's rollout launch, recorded and compared (recorded_batch.h) ----
    const bool learned = params || mo, pooled = learned && n > 1;
    RecordedBatch rb(learned ? 0 : n);
    float *pool_a = nullptr, *pool_c = nullptr, *member_costs = mo ? mo->member_costs : nullptr;
    ObsGather og{};
    if (learned) {
        LearnedCtx& ctx = h0->learned;
        if (pooled) {
            ICEM_HIP_TRY(ctx.reserve((size_t)n * N, n, hd, st));
            pool_a = ctx.pool_actions(), pool_c = ctx.pool_costs(hd);
            og.dst = ctx.pool_obs(hd), og.width = ICEM_RSSM_OBS_DIM;
            for (int i = 0; i < n; ++i) og.src[i] = (const float*)buffers[i].obs0;
        } else {   // (one problem: its own rows, its own observation)
            pool_a = (float*)buffers[0].actions, pool_c = (float*)buffers[0].costs;
            og.dst = (float*)const_cast<void*>(buffers[0].obs0);
        }
        if (mo && !member_costs) {   // (the members' costs of one iteration: scratch that only grows)
            ICEM_HIP_TRY(ctx.reserve_members((size_t)mo->members * n * N, st));
            member_costs = ctx.member_costs;
        }
    } else {
        if (!cem_sample_ok(h0))
            return fail(ICEM_E_UNSUPPORTED, who + "a row of this shape does not fit the step's sampler (its three probability tables and one row in LDS): "
                                                  "the operator's sampler has no batched form");
        for (int i = 0; i < n; ++i)
            if (int rc = record_rollout(rb, i, handles[i], buffers[i].obs0, buffers[i].actions, buffers[i].costs, st, who)) return rc;
        if (int rc = rb.check(who)) return rc;
    }
    // ---- argument blocks: per iteration [sample x n | rollout launch(es) x n | update x n]; no step-dependent value in them ----
    const size_t sb = cem_sample_block_bytes(h0), ub = mo ? sizeof(CemUpdateMembersArgs) : f64 ? sizeof(CemUpdateF64Args) : sizeof(CemUpdateF32Args);
    BlockLayout layout(n, ICEM_MAX_BATCH);
    layout.add(sb);   // (at 0)
    rb.place(layout);
    const size_t at_update = layout.add(ub), per_it = layout.bytes();
    std::vector<unsigned char> blob(per_it * iters, 0);
    BatchBases bases{};
    for (int i = 0; i < n; ++i) bases.v[i] = (handles[i]->episode << 32) + (uint64_t)steps[i] * (uint64_t)iters;
    for (int it = 0; it < iters; ++it) {
        unsigned char* part = blob.data() + per_it * it;
        for (int i = 0; i < n; ++i) {
            icem_cem_buffers b = buffers[i];
            if (pooled) b.actions = pool_a + (size_t)i * N * hd, b.costs = pool_c + (size_t)i * N;   // (the problem's own, but its pool: the slice)
            cem_sample_block(handles[i], N, b.mean, b.std, b.lower, b.upper, (uint64_t)it, b.actions, part + sb * i);
            rb.copy(i, part);
            void* row = results_row(results, i, (size_t)(c.act_dim + 1) * h0->tsize);
            if (mo) {   // (CemUpdateMembersArgs begins with a CemUpdateF32Args)
                CemUpdateMembersArgs& m = *(CemUpdateMembersArgs*)(part + at_update + ub * i);
                fill_update(handles[i], b, p, it == iters - 1, row, m.c);
                m.member_costs = member_costs, m.costs = (float*)b.costs;
                m.members = mo->members, m.reduce = mo->reduce;
                m.stride = n * N, m.row0 = i * N;
                m.inv = (float)(1.0 / mo->members);
            } else if (f64) fill_update(handles[i], b, p, it == iters - 1, row, *(CemUpdateF64Args*)(part + at_update + ub * i));
            else fill_update(handles[i], b, p, it == iters - 1, row, *(CemUpdateF32Args*)(part + at_update + ub * i));
        }
    }
    const int slot = steps[0] & 1;
    ICEM_HIP_TRY(h0->cem_batch_args.put(slot, blob, layout.room() * iters, st, &h0->batch_uploads));
    // ---- the launches: 3 per iteration (+ the GEMM path's row tail, which a CEM step never has: no shifted rows) ----
    const unsigned char* dev = (const unsigned char*)h0->cem_batch_args.dev(slot);
    const std::vector<int> rows(learned ? n : 0, N);
    rssm::Problem pr[rssm::BATCH_MAX];
    if (mo) models_problems(*mo, n, rows.data(), pr);
    long long launches = 0;
    for (int it = 0; it < iters; ++it) {
        const unsigned char* part = dev + per_it * it;
        if (pooled && it == 0) launch_cem_sample_gather_batch(h0, N, part, bases, og, n, st);
        else launch_cem_sample_batch(h0, N, part, bases, n, st);
        ICEM_HIP_TRY(hipGetLastError());
        ++launches;
        if (int rc = mo       ? rssm_launch_result(launch_rssm_split_models(n * mo->members, pr, c.horizon, c.act_dim, c.cost_mode, og.dst, pool_a,
                                                                            member_costs, st))
                     : params ? rssm_launch_result(launch_rssm_split_batch(n, rows.data(), c.horizon, c.act_dim, c.cost_mode, (const unsigned short*)params,
                                                                           og.dst, pool_a, pool_c, st))
                              : rb.launch(part, bases, st, &launches))
            return rc;
        if (learned) ++launches;
        if (mo) launch_cem_update_members_batch((const CemUpdateMembersArgs*)(part + at_update), n, hd, st);
        else if (f64) launch_cem_update_batch((const CemUpdateF64Args*)(part + at_update), n, hd, st);
        else launch_cem_update_batch((const CemUpdateF32Args*)(part + at_update), n, hd, st);
        ICEM_HIP_TRY(hipGetLastError());
        ++launches;
    }
    h0->cem_batch_launches = launches;
    return ICEM_OK;
}

}  // namespace

extern "C" {

int icem_plan_step_cem_ok(const icem_handle* h) { return (h && cem_unserved(h) == nullptr) ? 1 : 0; }

int icem_plan_step_cem(icem_handle* h, const icem_cem_buffers* b, const icem_cem_params* p, int32_t mpc_step, void* stream) {
    // ---- refusals: all of them before anything is launched or the handle touched ----
    if (!h || !b || !p) return fail(ICEM_E_INVALID, "icem_plan_step_cem: null handle, buffers or params");
    if (int rc = cem_refusal(h, *b, mpc_step, "icem_plan_step_cem: ")) return rc;
    h->cem_launches = 0;
    return cem_step_solo(h, b, p, mpc_step, nullptr, (hipStream_t)stream, &h->cem_launches);
}

int icem_plan_step_cem_batch(icem_handle* const* handles, int32_t n, const icem_cem_buffers* buffers, const icem_cem_params* p,
                             const int32_t* mpc_steps_host, void* results, void* stream) {
    // ---- refusals: all of them before anything is launched or any handle touched ----
    if (int rc = admit_batch(handles, n, buffers && p && mpc_steps_host, true, "icem_plan_step_cem_batch: ",
                             "icem_plan_step_cem_batch: the handles must share one configuration (everything but the seed)"))
        return rc;
    for (int i = 0; i < n; ++i)
        if (int rc = cem_refusal(handles[i], buffers[i], mpc_steps_host[i], "icem_plan_step_cem_batch: ")) return rc;
    if (n == 1) {   // one planner: the solo launches (the same bits by construction), the results row from the last update
        long long launches = 0;
        const int rc = cem_step_solo(handles[0], &buffers[0], p, mpc_steps_host[0], results, (hipStream_t)stream, &launches);
        if (rc == ICEM_OK) handles[0]->cem_batch_launches = launches;
        return rc;
    }
    return cem_step_batch(handles, n, buffers, *p, nullptr, mpc_steps_host, results, (hipStream_t)stream);
}

int icem_plan_step_cem_learned_ok(const icem_handle* h) { return (h && cem_learned_unserved(h) == nullptr) ? 1 : 0; }

int icem_plan_step_cem_learned(icem_handle* h, const icem_cem_buffers* b, const icem_cem_params* p, const void* params, int32_t mpc_step,
                               void* stream) {
    // ---- refusals: all of them before anything is launched or the handle touched ----
    if (!h || !b || !p || !params) return fail(ICEM_E_INVALID, "icem_plan_step_cem_learned: null handle, buffers, flags or params");
    if (int rc = cem_refusal(h, *b, mpc_step, "icem_plan_step_cem_learned: ", true)) return rc;
    // the rollout's staging area and its host-visible status word, BEFORE the first launch (as learned_step.hip)
    if (int rc = rssm_launch_result(rssm_split_prepare((h->cfg.num_traj + 15) / 16, h->cfg.horizon, (hipStream_t)stream))) return rc;
    h->cem_launches = 0;
    return cem_step_solo(h, b, p, mpc_step, nullptr, (hipStream_t)stream, &h->cem_launches, params);
}

int icem_plan_step_cem_learned_batch(icem_handle* const* handles, int32_t n, const icem_cem_buffers* buffers, const icem_cem_params* p,
                                     const void* params, const int32_t* mpc_steps_host, void* results, void* stream) {
    // ---- refusals: all of them before anything is launched or any handle touched ----
    const std::string who = "icem_plan_step_cem_learned_batch: ";
    if (int rc = admit_batch(handles, n, buffers && p && params && mpc_steps_host, true, who.c_str(),
                             "icem_plan_step_cem_learned_batch: the handles must share one configuration (everything but the seed)"))
        return rc;
    if (int rc = admit_rssm_binding(handles, n, "icem_plan_step_cem_learned_batch: the handles must share one configuration (everything but the seed)"))
        return rc;
    for (int i = 0; i < n; ++i)
        if (int rc = cem_refusal(handles[i], buffers[i], mpc_steps_host[i], who, true)) return rc;
    const icem_config& c = handles[0]->cfg;
    const std::vector<int> rows(n, c.num_traj);
    const int tiles = rssm_batch_tiles(n, rows.data());
    if (tiles < 0 || !rssm_split_batch_ok(tiles, c.horizon))
        return fail(ICEM_E_UNSUPPORTED, who + "the batch's tiles (the sum over the problems of ceil(rows / 16)) exceed the split launch's "
                                              "limit; nothing was launched");
    if (int rc = rssm_launch_result(rssm_split_prepare(tiles, c.horizon, (hipStream_t)stream))) return rc;
    if (n == 1) {   // one planner: the solo launches (the same bits by construction), the results row from the last update
        long long launches = 0;
        const int rc = cem_step_solo(handles[0], &buffers[0], p, mpc_steps_host[0], results, (hipStream_t)stream, &launches, params);
        if (rc == ICEM_OK) handles[0]->cem_batch_launches = launches;
        return rc;
    }
    return cem_step_batch(handles, n, buffers, *p, params, mpc_steps_host, results, (hipStream_t)stream);
}

// would a batch of n handles like `h` with `members` models per problem be served?
int icem_plan_step_cem_learned_models_ok(const icem_handle* h, int32_t n, int32_t members) {
    if (!h || cem_learned_unserved(h) || n < 1 || n > ICEM_MAX_BATCH || members < 1 || members > rssm::BATCH_MAX || n * members > rssm::BATCH_MAX)
        return 0;
    const long long tiles = (long long)n * members * ((h->cfg.num_traj + 15) / 16);
    return tiles <= rssm::SPLIT_TILE_LIMIT && rssm_split_batch_ok((int)tiles, h->cfg.horizon) ? 1 : 0;
}

int icem_plan_step_cem_learned_models(icem_handle* const* handles, int32_t n, const icem_cem_buffers* buffers, const icem_cem_params* p,
                                      int32_t members, const void* const* params_host, int32_t reduce, const int32_t* mpc_steps_host,
                                      void* member_costs, void* results, void* stream) {
    // ---- refusals: all of them before anything is launched or any handle touched ----
    const std::string who = "icem_plan_step_cem_learned_models: ";
    const std::string config_msg = who + "the handles must share one configuration (everything but the seed)";
    // (what the counts and the table alone decide comes first: no handle has been looked at when n x members is refused)
    if (int rc = models_args_refusal(who, handles && buffers && p && mpc_steps_host, n, members, params_host, reduce)) return rc;
    if (int rc = admit_batch(handles, n, true, true, who.c_str(), config_msg.c_str())) return rc;
    if (int rc = admit_rssm_binding(handles, n, config_msg.c_str())) return rc;
    for (int i = 0; i < n; ++i)
        if (int rc = cem_refusal(handles[i], buffers[i], mpc_steps_host[i], who, true)) return rc;
    const icem_config& c = handles[0]->cfg;
    const StepModels mo{members, reduce, params_host, (float*)member_costs};
    const int tiles = models_tiles_uniform(mo, n, c.num_traj, c.horizon);
    if (tiles < 0)
        return fail(ICEM_E_UNSUPPORTED, who + "the tiles of a rollout (members x the sum over the problems of ceil(num_traj / 16)) exceed the "
                                              "split launch's limit; nothing was launched");
    if (int rc = rssm_launch_result(rssm_split_prepare(tiles, c.horizon, (hipStream_t)stream))) return rc;
    return cem_step_batch(handles, n, buffers, *p, nullptr, mpc_steps_host, results, (hipStream_t)stream, &mo);
}

int64_t icem_cem_step_launches(const icem_handle* h) { return h ? (int64_t)h->cem_launches : 0; }
int64_t icem_cem_batch_launches(const icem_handle* h) { return h ? (int64_t)h->cem_batch_launches : 0; }

}  // extern "C"
