// step_models.h -- what the MPC steps through models of their own share on the host (icem_plan_step_learned_models, learned_step.hip;
// icem_plan_step_cem_learned_models, cem_step.hip; icem_plan_step_random_learned_models, random_step.hip): the table of an
// ensemble's members or of a trained model per problem, the problems of the ONE rollout launch that scores them, and the
// refusals that the counts and the table alone decide.  Internal; not part of the public ABI.
#pragma once
#include "host_common.h"
#include "icem_rssm.h"

namespace icem {

// every problem rolls out through `members` models of its own instead of the one shared buffer
struct StepModels {
    int members, reduce;
    const void* const* params;   // [n * members], problem-major
    float* member_costs;         // the caller's [members * n * max_rows], or nullptr: the context's scratch
};

// the rollout of such a step's iteration: n * members problems in member-major order -- problem e * n + p reads problem p's
// action rows and observation row p, so that the costs land as [members, the iteration's rows of all problems]
// (Problem: rssm::Problem, or mlp::Problem of icem_plan_step_mlp -- the same four fields)
template <typename Problem>
inline void models_problems(const StepModels& mo, int n, const int* rows, Problem* out) {
    for (int e = 0; e < mo.members; ++e) {
        long long row0 = 0;
        for (int p = 0; p < n; ++p) {
            out[e * n + p] = {(const unsigned short*)mo.params[(size_t)p * mo.members + e], row0, rows[p], p};
            row0 += rows[p];
        }
    }
}

// what the counts and the table alone decide, before any handle is looked at (who: the entry's name + ": ")
inline int models_args_refusal(const std::string& who, bool args, int n, int members, const void* const* params_host, int reduce) {
    if (!args || !params_host || n < 1 || n > ICEM_MAX_BATCH) return fail(ICEM_E_INVALID, who + "null argument / n outside [1, 32]");
    if (members < 1 || members > rssm::BATCH_MAX) return fail(ICEM_E_INVALID, who + "members must be in [1, 32]");
    if (reduce != ICEM_RSSM_REDUCE_MEAN && reduce != ICEM_RSSM_REDUCE_MAX)
        return fail(ICEM_E_INVALID, who + "reduce must be ICEM_RSSM_REDUCE_MEAN or ICEM_RSSM_REDUCE_MAX");
    for (int i = 0; i < n * members; ++i)
        if (!params_host[i]) return fail(ICEM_E_INVALID, who + "null params entry");
    if (n * members > rssm::BATCH_MAX)
        return fail(ICEM_E_UNSUPPORTED, who + "n x members problems, but one learned-dynamics launch holds 32 (its table travels in the kernel "
                                              "arguments); nothing was launched");
    return ICEM_OK;
}

// the tiles of ONE rollout of n problems of `rows` rows each through `members` models each (-1: beyond what a launch serves)
inline int models_tiles_uniform(const StepModels& mo, int n, int rows, int horizon) {
    rssm::Problem pr[rssm::BATCH_MAX];
    int r[ICEM_MAX_BATCH];
    for (int p = 0; p < n; ++p) r[p] = rows;
    models_problems(mo, n, r, pr);
    const int tiles = rssm_models_tiles(n * mo.members, pr);
    return (tiles < 0 || !rssm_split_batch_ok(tiles, horizon)) ? -1 : tiles;
}

}  // namespace icem
