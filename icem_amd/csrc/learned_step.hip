// learned_step.hip -- the MPC step of the learned-dynamics configuration (BASELINE configs[4]: the declared RSSM) as one C
// call, for one planner or for B planners at once: icem_plan_step_learned / icem_plan_step_learned_batch.
//
// The step is the stage-wise loop of the controllers (icem_amd/controllers.py::_get_action_stagewise + _stage_finish) with
// every stage ONE launch for all problems:
//   sample   sample_folded_batch_kernel (k_sample.hip), icem_plan_step_batch's batched sampler: icem_sample_clip's folded sampler,
//            blockIdx.y = the problem, ragged row counts (so never with shifted rows: they are the next launch)
//   shift    iteration 0 of a step > 0: shift_sample_batch_kernel (generic_kernels.hip) -- the copy of elites[e, 1:, :] and
//            icem_sample_clip(t_begin = h - 1)'s draw of the last action, the operator's own arithmetic
//   rollout  launch_rssm_rollout (one problem) / launch_rssm_split_batch (several)
//   update   update_small_batch_kernel (k_merge.hip): icem_update_distribution's body, one workgroup per problem; the last
//            one carries the epilogue (icem_shift's arithmetic, executed, best_cost, the results row)
// i.e. 3 launches per iteration, + 1 in the steps that shift elites.  The step shares icem_plan_step_batch's plumbing rather
// than restating it: the argument blocks live in a DeviceArgArray (arg_array.h) with the step's first handle, their sections laid
// out by block_layout.h, stream offsets relative to each problem's base (BatchBases, call_base), uploaded only when a byte
// changed -- the steady state uploads nothing; a batch is admitted by admit_batch; noise offsets, shifted rows and elite halves
// are host_common.h's call_base, shift_rows and elite_parity, so a controller may alternate between the two steps.  A batch's
// rows sit back to back in a pool of the first handle's (LearnedCtx: the batched rollout wants them contiguous); one problem
// alone uses its own actions / costs buffers.
//
// icem_plan_step_learned_models is the same step for problems that roll out through models of their own (an ensemble's members,
// a trained model per episode): the rollout is launch_rssm_split_models over n * members problems in member-major order, and
// the update is update_small_members_batch_kernel, which reduces the members' costs while it builds its keys -- still 3
// launches per iteration, and the same code below (StepModels, step_models.h: shared with the two baselines' steps through such
// models, cem_step.hip and random_step.hip).
//
// icem_plan_step_mlp is that models step with the feed-forward model (icem_mlp.h) in the RSSM's place: the rollout of an
// iteration is ONE launch_mlp_rollout_models of n * members problems in the same member-major order, the observation table is
// [n, obs_dim], and neither the RSSM's staging area nor its status word nor a handle's RSSM binding is involved.  Everything
// else -- the sampler, the shifted rows, the updates with the members' reduction and the epilogue, the argument blocks -- is the
// code below as it stands (StepMlp switches the rollout and what "served" asks), so a controller may alternate between this
// step, the RSSM steps and the stage-wise loop on one handle.
#include "block_layout.h"
#include "cost_terms_dev.h"
#include "host_common.h"
#include "icem_mlp.h"
#include "icem_rssm.h"
#include "step_models.h"

using namespace icem;

namespace {

int max_rows(const icem_handle* h) {
    int m = 0;
    for (size_t it = 0; it < h->pop.size(); ++it) m = std::max(m, h->pop[it] + (it == 0 ? std::max(0, h->n_reuse) : 0));
    return m;
}

// the rollout of icem_plan_step_mlp: the model's shape (act_dim is the handles') and the launch's cost
struct StepMlp {
    int obs_dim, layers, activation;
    CostArgs<float> cs;
};

// the per-handle part of "who is served" (nullptr: this handle is) -- rssm: by the steps through the declared RSSM, which ask
// for its action width and the split launch on top of what every step below needs; else by icem_plan_step_mlp
const char* step_unserved(const icem_handle* h, bool rssm) {
    const icem_config& c = h->cfg;
    if (rssm && opt_i(OPT_LEARNED_STEP) == 0) return "option learned_step is 0";
    if (!rssm && opt_i(OPT_MLP_STEP) == 0) return "option mlp_step is 0";
    if (c.dtype != ICEM_F32) return "dtype f32 only";
    if (c.world != 1) return "world must be 1";
    // (a handle bound to an RSSM of its own width -- icem_set_rssm_act_dim, which takes no other -- passes; one never bound is served at 6)
    if (rssm && c.act_dim != rssm_width(h)) return "the declared RSSM takes 6 action dimensions";
    if (!h->use_fast) return "the handle's fast path is off";
    if (h->profiling) return "per-kernel profiling is per launch of one handle: switch it off";
    if (!fast_sample_supported(c.horizon, c.act_dim) || c.horizon > 32)
        return "the horizon is outside the folded sampler's list (30, 12, 13, 10)";
    if (h->hd > UPDATE_FINISH_MAX_HD) return "horizon * act_dim exceeds what the last update's epilogue holds (512)";
    if (c.rng_rounds != 10) return "the batched sampler is compiled for the default generator (rng_rounds 10)";
    if ((int)h->pop.size() != c.opt_iters || c.opt_iters < 1) return "opt_iters";
    if (!topk_small_ok(max_rows(h) + std::max(0, h->n_reuse), c.num_elites)) return "the one-launch update does not take this pool / num_elites (<= 16384 candidates, <= 32 elites)";
    if (rssm && !rssm_split_ok(max_rows(h), c.horizon)) return "the population's tiles exceed the split launch's limit, or the split launch is switched off";
    return nullptr;
}
const char* learned_unserved(const icem_handle* h) { return step_unserved(h, true); }

// mlp (with mo): the step of icem_plan_step_mlp; who: the entry's name + ": " in front of the refusals
int learned_step(icem_handle* const* handles, int n, const icem_plan_buffers* buffers, const void* params, const int32_t* steps,
                 void* results, hipStream_t st, const StepModels* mo = nullptr, const StepMlp* mlp = nullptr,
                 const std::string& who = "icem_plan_step_learned: ") {
    icem_handle* h0 = handles[0];
    const icem_config& c = h0->cfg;
    const int H = c.horizon, d = c.act_dim, hd = h0->hd, K = c.num_elites, iters = c.opt_iters, n_reuse = std::max(0, h0->n_reuse);
    // ---- refusals: all of them before anything is launched or any handle touched ----
    for (int i = 0; i < n; ++i) {
        if (steps[i] < 0) return fail(ICEM_E_INVALID, who + "negative mpc_step");
        const icem_plan_buffers& b = buffers[i];
        if (!b.mean || !b.std || !b.low || !b.high || !b.obs0 || !b.actions || !b.costs || !b.elites || !b.executed || !b.best_cost)
            return fail(ICEM_E_INVALID, who + "null buffer (mean, std, low, high, obs0, actions, costs, elites, executed, best_cost)");
    }
    for (int i = 0; i < n; ++i) {
        if (const char* why = step_unserved(handles[i], mlp == nullptr)) return fail(ICEM_E_UNSUPPORTED, who + why);
        const icem_plan_buffers& b = buffers[i];
        if (b.z_r || b.z_i || b.z_r_shift || b.z_i_shift) return fail(ICEM_E_UNSUPPORTED, who + "external noise (z_*) is not served");
    }
    // rows of every problem and iteration; the largest launch's tiles
    std::vector<int> rows((size_t)iters * n), all_rows((size_t)iters);
    int tiles_max = 0, shift_max = 0;
    size_t rows_max = 0;
    for (int it = 0; it < iters; ++it) {
        size_t all = 0;
        for (int p = 0; p < n; ++p) {
            rows[(size_t)it * n + p] = h0->pop[it] + shift_rows(handles[p], steps[p], it);
            all += rows[(size_t)it * n + p];
            shift_max = std::max(shift_max, shift_rows(handles[p], steps[p], it));
        }
        int tiles = 0;
        if (mlp) {   // (no staging area to fit: the grid's x extent is the limit)
            long long wgs = 0;
            for (int p = 0; p < n; ++p) wgs += (rows[(size_t)it * n + p] + 15) / 16;
            if (wgs * mo->members > mlp::WORKGROUPS_MAX)
                return fail(ICEM_E_UNSUPPORTED, who + "the tiles of an iteration (members x the sum over the problems of ceil(rows / 16)) exceed "
                                                      "one launch's grid; nothing was launched");
        } else if (mo) {
            rssm::Problem pr[rssm::BATCH_MAX];
            models_problems(*mo, n, &rows[(size_t)it * n], pr);
            tiles = rssm_models_tiles(n * mo->members, pr);
            if (tiles < 0 || !rssm_split_batch_ok(tiles, H))
                return fail(ICEM_E_UNSUPPORTED, "icem_plan_step_learned_models: the tiles of an iteration (members x the sum over the problems of "
                                                "ceil(rows / 16)) exceed the split launch's limit; nothing was launched");
        } else {
            tiles = rssm_batch_tiles(n, &rows[(size_t)it * n]);
            if (tiles < 0 || !rssm_split_batch_ok(tiles, H))
                return fail(ICEM_E_UNSUPPORTED, "icem_plan_step_learned_batch: the batch's tiles (the sum over the problems of ceil(rows / 16)) exceed "
                                                "the split launch's limit; nothing was launched");
        }
        tiles_max = std::max(tiles_max, tiles);
        rows_max = std::max(rows_max, all);
        all_rows[it] = (int)all;
    }
    // the rollout's staging area and its host-visible status word, BEFORE the first launch: a refused step leaves everything as it was
    if (!mlp)
        if (int rc = rssm_launch_result(rssm_split_prepare(tiles_max, H, st))) return rc;
    // ---- the step's own memory (first call, or a larger batch than before) ----
    LearnedCtx* ctx = &h0->learned;
    if (!ctx->idx) ICEM_HIP_TRY(hipMalloc((void**)&ctx->idx, (size_t)ICEM_MAX_BATCH * ICEM_MAX_ELITES * sizeof(int)));
    const size_t cap_rows = (size_t)n * (size_t)max_rows(h0);   // (what any mix of steps of this batch size needs)
    if (n > 1) ICEM_HIP_TRY(ctx->reserve(cap_rows, n, hd, st));
    float* pool_a = ctx->pool_actions();
    float* pool_c = ctx->pool_costs(hd);
    float* pool_o = ctx->pool_obs(hd);
    // (a models step: the members' costs of one iteration, [members, its rows] -- the caller's buffer, or scratch that only grows)
    float* member_costs = mo ? mo->member_costs : nullptr;
    if (mo && !member_costs) {
        ICEM_HIP_TRY(ctx->reserve_members((size_t)mo->members * cap_rows, st));
        member_costs = ctx->member_costs;
    }
    // ---- argument blocks (block_layout.h): per iteration [sample x n | update x n], then [shift x n] ----
    const size_t sb = sizeof(FastSampleArgs), ub = mo ? sizeof(UpdateMembersArgs) : sizeof(UpdateFinishArgs), hb = gk_shift_sample_block_bytes();
    BlockLayout part(n, ICEM_MAX_BATCH), tail(n, ICEM_MAX_BATCH);
    part.add(sb);   // (at 0)
    const size_t at_update = part.add(ub), per_it = part.bytes(), at_shift = per_it * iters;
    tail.add(hb);
    std::vector<unsigned char> blob(at_shift + tail.bytes(), 0);
    BatchBases bases{};
    for (int p = 0; p < n; ++p) bases.v[p] = call_base(handles[p], steps[p]);
    for (int it = 0; it < iters; ++it) {
        size_t row0 = 0;
        for (int p = 0; p < n; ++p) {
            const icem_handle* h = handles[p];
            const icem_plan_buffers& b = buffers[p];
            const int n_it = h0->pop[it], n_shift = shift_rows(h, steps[p], it), n_rows = n_it + n_shift;
            float* acts = n == 1 ? (float*)b.actions : pool_a + row0 * hd;
            float* csts = n == 1 ? (float*)b.costs : pool_c + row0;
            const size_t first_row = row0;
            row0 += n_rows;
            const int r = elite_parity(h, steps[p], it), w = r ^ 1;
            float* el = (float*)b.elites;
            float* el_w = el + (size_t)w * K * hd;
            const float* el_r = el + (size_t)r * K * hd;
            float* ec_w = el + (size_t)2 * K * hd + (size_t)w * K;
            const float* ec_r = el + (size_t)2 * K * hd + (size_t)r * K;
            FastSampleArgs& s = *(FastSampleArgs*)(blob.data() + per_it * it + sb * p);
            s.n = n_it, s.h = H, s.d = d, s.first_index = 0;
            s.W = (const float*)h->W_dev;
            s.mean = (const float*)b.mean, s.std = (const float*)b.std, s.low = (const float*)b.low, s.high = (const float*)b.high;
            s.seed_lo = (uint32_t)h->cfg.seed, s.seed_hi = (uint32_t)(h->cfg.seed >> 32);
            s.off_lo = (uint32_t)it, s.off_hi = 0;   // (relative to bases.v[p])
            s.row0_mean = (c.use_mean_actions && it == iters - 1) ? 1 : 0;
            s.out = acts;
            s.white = c.noise_beta <= 0 ? 1 : 0;
            if (it == 0)
                gk_shift_sample_block(h, n_shift, b.mean, b.std, b.low, b.high, (uint64_t)iters, el_r, acts + (size_t)n_it * hd,
                                      blob.data() + at_shift + hb * p);
            UpdateFinishArgs& u = *(UpdateFinishArgs*)(blob.data() + per_it * it + at_update + ub * p);   // (UpdateMembersArgs begins with one)
            if (mo) {
                UpdateMembersArgs& m = *(UpdateMembersArgs*)(blob.data() + per_it * it + at_update + ub * p);
                m.member_costs = member_costs, m.costs = csts;
                m.members = mo->members, m.reduce = mo->reduce;
                m.stride = all_rows[it], m.row0 = (int)first_row;
                m.inv = (float)(1.0 / mo->members);
            }
            const bool keep = it > 0 && c.keep_previous_elites && n_reuse > 0;
            u.u.costs = csts, u.u.pool = acts;
            u.u.keep_costs = keep ? ec_r : nullptr, u.u.keep_actions = keep ? el_r : nullptr;
            u.u.n = n_rows, u.u.n_keep = keep ? n_reuse : 0, u.u.K = K, u.u.hd = hd;
            u.u.alpha = (float)c.alpha;
            u.u.mean = (float*)b.mean, u.u.std = (float*)b.std;
            u.u.elites_out = el_w, u.u.elite_costs_out = ec_w;
            u.u.idx_out = ctx->idx + (size_t)p * ICEM_MAX_ELITES;
            if (it == iters - 1) {
                u.d = d;
                u.init_std = (float)c.init_std;
                u.low = (const float*)b.low, u.high = (const float*)b.high;
                u.executed = (float*)b.executed, u.best_cost = (float*)b.best_cost;
                u.result = (float*)results_row(results, p, (size_t)(d + 1) * sizeof(float));
            }
        }
    }
    const int slot = steps[0] & 1;
    ICEM_HIP_TRY(ctx->args.put(slot, blob, part.room() * iters + tail.room(), st, &h0->batch_uploads));
    // ---- the launches ----
    const unsigned char* dev = (const unsigned char*)ctx->args.dev(slot);
    long long launches = 0;
    (mlp ? ctx->mlp_launches : ctx->launches) = 0;
    LaunchKey sk;   // the sampler's: the grid's x extent is the largest problem's (all of them draw pop[it] rows)
    sk.family = LAUNCH_SAMPLE, sk.h = H, sk.d = d, sk.form = 10;
    for (int it = 0; it < iters; ++it) {
        ObsGather og{};
        if (n > 1 && it == 0) {
            for (int p = 0; p < n; ++p) og.src[p] = (const float*)buffers[p].obs0;
            og.dst = pool_o;
            og.width = mlp ? mlp->obs_dim : rssm::DET + rssm::STOCH;
        }
        sk.wgs[0] = sample_row_workgroups(h0->pop[it], d);
        launch_sample_batch(sk, (const FastSampleArgs*)(dev + per_it * it), bases, og, n, st);
        ICEM_HIP_TRY(hipGetLastError());
        ++launches;
        if (it == 0 && shift_max > 0) {
            if (int rc = gk_shift_sample_batch(h0, n, shift_max, dev + at_shift, bases, st)) return rc;
            ++launches;
        }
        hipError_t e;
        if (mlp) {
            mlp::Problem pr[mlp::PROBLEMS_MAX];
            models_problems(*mo, n, &rows[(size_t)it * n], pr);
            e = launch_mlp_rollout_models(n * mo->members, pr, H, mlp->obs_dim, d, mlp->layers, mlp->activation, c.cost_mode, mlp->cs,
                                          n == 1 ? (const float*)buffers[0].obs0 : pool_o, n == 1 ? (const float*)buffers[0].actions : pool_a,
                                          member_costs, nullptr, st);
        } else if (mo) {
            rssm::Problem pr[rssm::BATCH_MAX];
            models_problems(*mo, n, &rows[(size_t)it * n], pr);
            e = launch_rssm_split_models(n * mo->members, pr, H, d, c.cost_mode, n == 1 ? (const float*)buffers[0].obs0 : pool_o,
                                         n == 1 ? (const float*)buffers[0].actions : pool_a, member_costs, st);
        } else if (n == 1)
            e = launch_rssm_rollout(rows[it], H, d, c.cost_mode, (const unsigned short*)params, (const float*)buffers[0].obs0,
                                    (const float*)buffers[0].actions, (float*)buffers[0].costs, st);
        else
            e = launch_rssm_split_batch(n, &rows[(size_t)it * n], H, d, c.cost_mode, (const unsigned short*)params, pool_o, pool_a, pool_c, st);
        if (int rc = rssm_launch_result(e)) return rc;
        ++launches;
        if (mo) launch_update_small_members_batch((const UpdateMembersArgs*)(dev + per_it * it + at_update), n, it == iters - 1, st);
        else launch_update_small_batch((const UpdateFinishArgs*)(dev + per_it * it + at_update), n, it == iters - 1, st);
        ICEM_HIP_TRY(hipGetLastError());
        ++launches;
    }
    (mlp ? ctx->mlp_launches : ctx->launches) = launches;
    return ICEM_OK;
}

}  // namespace

extern "C" {

int icem_plan_step_learned_ok(const icem_handle* h) { return (h && learned_unserved(h) == nullptr) ? 1 : 0; }

int icem_plan_step_learned_batch(icem_handle* const* handles, int32_t n, const icem_plan_buffers* buffers, const void* params,
                                 const int32_t* mpc_steps_host, void* results, void* stream) {
    if (int rc = admit_batch(handles, n, buffers && params && mpc_steps_host, true, "icem_plan_step_learned_batch: ",
                             "icem_plan_step_learned_batch: the handles must share one configuration (everything but the seed)"))
        return rc;
    if (int rc = admit_rssm_binding(handles, n, "icem_plan_step_learned_batch: the handles must share one configuration (everything but the seed)"))
        return rc;
    return learned_step(handles, n, buffers, params, mpc_steps_host, results, (hipStream_t)stream);
}

int icem_plan_step_learned(icem_handle* h, const icem_plan_buffers* b, const void* params, int32_t mpc_step, void* stream) {
    if (!h || !b || !params) return fail(ICEM_E_INVALID, "icem_plan_step_learned: null handle, buffers or params");
    return learned_step(&h, 1, b, params, &mpc_step, nullptr, (hipStream_t)stream);
}

int64_t icem_learned_step_launches(const icem_handle* h) { return h ? (int64_t)h->learned.launches : 0; }

// would a batch of n handles like `h` with `members` models per problem be served?  (the tiles: every problem with its shifted elites)
int icem_plan_step_learned_models_ok(const icem_handle* h, int32_t n, int32_t members) {
    if (!h || learned_unserved(h) || n < 1 || n > ICEM_MAX_BATCH || members < 1 || members > rssm::BATCH_MAX || n * members > rssm::BATCH_MAX)
        return 0;
    const long long tiles = (long long)n * members * ((max_rows(h) + 15) / 16);
    return tiles <= rssm::SPLIT_TILE_LIMIT && rssm_split_batch_ok((int)tiles, h->cfg.horizon) ? 1 : 0;
}

int icem_plan_step_learned_models(icem_handle* const* handles, int32_t n, const icem_plan_buffers* buffers, int32_t members,
                                  const void* const* params_host, int32_t reduce, const int32_t* mpc_steps_host, void* member_costs,
                                  void* results, void* stream) {
    const char* config_msg = "icem_plan_step_learned_models: the handles must share one configuration (everything but the seed)";
    // (what the counts and the table alone decide comes first: no handle has been looked at when n x members is refused)
    if (int rc = models_args_refusal("icem_plan_step_learned_models: ", handles && buffers && mpc_steps_host, n, members, params_host, reduce)) return rc;
    if (int rc = admit_batch(handles, n, true, true, "icem_plan_step_learned_models: ", config_msg)) return rc;
    if (int rc = admit_rssm_binding(handles, n, config_msg)) return rc;
    const StepModels mo{members, reduce, params_host, (float*)member_costs};
    return learned_step(handles, n, buffers, nullptr, mpc_steps_host, results, (hipStream_t)stream, &mo);
}

static_assert(mlp::PROBLEMS_MAX == rssm::BATCH_MAX, "models_args_refusal's limit is both launches' problem table");

int icem_plan_step_mlp_ok(const icem_handle* h, int32_t n, int32_t members) {
    if (!h || step_unserved(h, false) || n < 1 || n > ICEM_MAX_BATCH || members < 1 || members > mlp::PROBLEMS_MAX || n * members > mlp::PROBLEMS_MAX)
        return 0;
    if (h->cfg.act_dim > mlp::ACT_MAX) return 0;
    return (long long)n * members * ((max_rows(h) + 15) / 16) <= mlp::WORKGROUPS_MAX ? 1 : 0;
}

int icem_plan_step_mlp(icem_handle* const* handles, int32_t n, const icem_plan_buffers* buffers, const icem_mlp_step_model* model,
                       int32_t members, const void* const* params_host, int32_t reduce, const int32_t* mpc_steps_host, void* member_costs,
                       void* results, void* stream) {
    const std::string who = "icem_plan_step_mlp: ";
    // (what the counts, the table and the model's own fields decide comes first: no handle has been looked at)
    if (int rc = models_args_refusal(who, handles && buffers && model && mpc_steps_host, n, members, params_host, reduce)) return rc;
    if (!model->cost) return fail(ICEM_E_INVALID, who + "null cost");
    if (model->activation != ICEM_MLP_RELU && model->activation != ICEM_MLP_SWISH)
        return fail(ICEM_E_INVALID, who + "activation must be ICEM_MLP_RELU or ICEM_MLP_SWISH");
    if (!mlp::shape_ok(model->obs_dim, 1, model->layers)) return fail(ICEM_E_UNSUPPORTED, who + "obs_dim must be in [1, 64] and layers in [1, 4]");
    if (int rc = admit_batch(handles, n, true, true, who.c_str(), "icem_plan_step_mlp: the handles must share one configuration (everything but the seed)"))
        return rc;
    const icem_config& c = handles[0]->cfg;
    const icem_cost_terms* on = nullptr;
    if (int rc = admit_mlp_launch("icem_plan_step_mlp", c.horizon, model->obs_dim, c.act_dim, model->layers, model->activation, c.cost_mode,
                                  model->cost, model->terms, &on))
        return rc;
    StepMlp ml{model->obs_dim, model->layers, model->activation, {}};
    fill_cost_args_f32(*model->cost, on, ml.cs);
    const StepModels mo{members, reduce, params_host, (float*)member_costs};
    return learned_step(handles, n, buffers, nullptr, mpc_steps_host, results, (hipStream_t)stream, &mo, &ml, who);
}

int64_t icem_mlp_step_launches(const icem_handle* h) { return h ? (int64_t)h->learned.mlp_launches : 0; }

}  // extern "C"
