// cem_step.hip -- the MPC step of the CEM baseline (MpcCemStd.get_action, icem/controllers/mpc.py:200-262) as one C call:
// icem_plan_step_cem.  The step is the stage-wise loop of MpcCemStdHip.get_action (icem_amd/controllers.py) with every
// iteration three launches and nothing between them:
//   sample   cem_sample_kernel (k_cem.hip): icem_sample_truncnorm's draw at offset (episode << 32) + step * opt_iters + i
//            (sample_truncnorm_kernel itself where a row of the shape does not fit the sampler's LDS)
//   rollout  rollout_cost_launch (abi.hip): the launch icem_rollout_cost picks for the handle
//   update   cem_update_*_kernel (k_cem.hip): icem_update_distribution's body (f32) / the one-launch selection's (f64), then
//            icem_cem_bounds' arithmetic; the last one carries get_action's epilogue
// The arguments go by value: no device-side argument memory, no upload, nothing allocated by the step itself.
#include "cem_step.h"

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

template <typename T>
CemTailArgs<T> tail_args(const icem_handle* h, const icem_cem_buffers& b, const icem_cem_params& p, bool last) {
    CemTailArgs<T> t;
    t.h = h->cfg.horizon, t.d = h->cfg.act_dim;
    t.like_levine = p.like_levine != 0, t.shift_means = p.shift_means != 0, t.execute_best_elite = p.execute_best_elite != 0;
    t.last = last ? 1 : 0;
    t.init_std = (T)h->cfg.init_std;
    t.mean = (T*)b.mean, t.std = (T*)b.std;
    t.low = (const T*)b.low, t.high = (const T*)b.high;
    t.lower = (T*)b.lower, t.upper = (T*)b.upper;
    t.elites = (const T*)b.elites, t.elite_costs = (const T*)b.elite_costs;
    t.executed = (T*)b.executed, t.best_cost = (T*)b.best_cost;
    return t;
}

void launch_update(const icem_handle* h, const icem_cem_buffers& b, const icem_cem_params& p, bool last, hipStream_t st) {
    const icem_config& c = h->cfg;
    const int N = c.num_traj, K = c.num_elites;
    if (c.dtype == ICEM_F32) {
        // (icem_update_distribution's block, abi.hip: no kept elites)
        const UpdateSmallArgs u{(const float*)b.costs, (const float*)b.actions, nullptr, nullptr, N, 0, K, h->hd, (float)c.alpha,
                                (float*)b.mean, (float*)b.std, (float*)b.elites, (float*)b.elite_costs, b.elite_idx};
        launch_cem_update(u, tail_args<float>(h, b, p, last), st);
        return;
    }
    // (gk_select_refit's block, generic_kernels.hip: every row a sampled one, no kept elites, never the step's "last" -- the
    //  CEM epilogue is cem_tail's)
    SelectArgs<double> s;
    std::memset((void*)&s, 0, sizeof(s));
    s.n_cand = s.n_loc = N;
    s.cap = SELECT_CAP;
    s.costs = (const double*)b.costs;
    s.actions = (const double*)b.actions;
    MergeArgs<double>& a = s.m;
    a.K = K, a.h = c.horizon, a.d = c.act_dim, a.n_global = N;
    a.alpha = c.alpha, a.init_std = c.init_std;
    a.elites_next = (double*)b.elites, a.elites_cost_next = (double*)b.elite_costs;
    a.mean_in = (const double*)b.mean, a.std_in = (const double*)b.std;
    a.mean = (double*)b.mean, a.std = (double*)b.std;
    a.low = (const double*)b.low, a.high = (const double*)b.high;
    a.xw = XchgWait{};
    launch_cem_update(s, b.elite_idx, tail_args<double>(h, b, p, last), st);
}

}  // namespace

extern "C" {

int icem_plan_step_cem_ok(const icem_handle* h) { return (h && cem_unserved(h) == nullptr) ? 1 : 0; }

int icem_plan_step_cem(icem_handle* h, const icem_cem_buffers* b, const icem_cem_params* p, int32_t mpc_step, void* stream) {
    // ---- refusals: all of them before anything is launched or the handle touched ----
    if (!h || !b || !p) return fail(ICEM_E_INVALID, "icem_plan_step_cem: null handle, buffers or params");
    if (mpc_step < 0) return fail(ICEM_E_INVALID, "icem_plan_step_cem: negative mpc_step");
    if (!b->mean || !b->std || !b->lower || !b->upper || !b->low || !b->high || !b->obs0 || !b->actions || !b->costs || !b->elites ||
        !b->elite_costs || !b->elite_idx || !b->executed || !b->best_cost)
        return fail(ICEM_E_INVALID, "icem_plan_step_cem: null buffer (everything but workspace is needed)");
    if (const char* why = cem_unserved(h)) return fail(ICEM_E_UNSUPPORTED, std::string("icem_plan_step_cem: ") + why);
    if (!h->has_model || !h->has_cost) return fail(ICEM_E_STATE, "icem_plan_step_cem: icem_set_model / icem_set_cost must be called first");
    if (const char* e = cost_indices_error(h, h->obs_dim)) return fail(ICEM_E_INVALID, e);
    if (const char* e = wide_unsupported(h, 0, false, false)) return fail(ICEM_E_UNSUPPORTED, e);
    const icem_config& c = h->cfg;
    const int N = c.num_traj, iters = c.opt_iters;
    hipStream_t st = (hipStream_t)stream;
    const bool own_sampler = cem_sample_ok(h);
    long long launches = 0;
    h->cem_launches = 0;
    for (int it = 0; it < iters; ++it) {
        const uint64_t offset = (h->episode << 32) + (uint64_t)mpc_step * (uint64_t)iters + (uint64_t)it;
        int rc = own_sampler ? launch_cem_sample(h, N, b->mean, b->std, b->lower, b->upper, offset, b->actions, st)
                             : gk_sample_truncnorm(h, N, 0, b->mean, b->std, b->lower, b->upper, nullptr, offset, b->actions, st);
        if (rc) return rc;
        ++launches;
        rc = rollout_cost_launch(h, N, b->obs0, b->actions, b->costs, nullptr, st);
        if (rc) return rc;
        ++launches;
        launch_update(h, *b, *p, it == iters - 1, st);
        ICEM_HIP_TRY(hipGetLastError());
        ++launches;
    }
    h->cem_launches = launches;
    return ICEM_OK;
}

int64_t icem_cem_step_launches(const icem_handle* h) { return h ? (int64_t)h->cem_launches : 0; }

}  // extern "C"
