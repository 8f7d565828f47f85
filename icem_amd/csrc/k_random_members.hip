// k_random_members.hip -- the selection kernel of icem_plan_step_random_learned_models (random_step.hip): the random-shooting
// baseline's MPC step through an ensemble's members or a model per problem.  It is random_select_pool_batch_kernel
// (k_random_learned.hip) with the slice's costs coming out of the members' costs [members, stride = n * N] that the ONE rollout launch
// left -- problem p's rows at p * N -- not out of a plain load: random_select_body<float, MIRROR, MemberCosts> (random_dev.h,
// update_small_body.h: rssm_ensemble_reduce_kernel's arithmetic operation for operation, all of a row's member loads requested
// before the first is consumed).  A translation unit of its own, as k_cem_members.hip is: the units of the existing kernels keep
// the kernels they had.
#include "random_dev.h"

namespace icem {

namespace {

// ... for icem_plan_step_random_learned_models: the slice's costs are not in memory yet -- the rollout left the members' costs
// [members, stride = n * N], problem p's rows at p * N -- so every workgroup reduces its rows' member costs on the way to its keys
// (MemberCosts), stores the reduced cost to the pool's slice (the source) and to the problem's own costs (MIRROR), and keys on
// nan_to_inf of it; the ticket, the finish and the gathers are the body's
__global__ __launch_bounds__(RANDOM_SELECT_NT) void random_select_members_batch_kernel(const RandomSelectArgs<float>* __restrict__ args,
                                                                                       RandomPool<float> pool, RandomMembers mb) {
    RandomSelectArgs<float> a = from_device(args[blockIdx.y]);
    float* own_costs = const_cast<float*>(a.costs);
    float* slice = pool.costs + (size_t)blockIdx.y * (size_t)a.n;
    a.costs = slice;
    a.actions = pool.actions + (size_t)blockIdx.y * (size_t)a.n * (size_t)a.hd;
    const MemberCosts src{mb.member_costs + (size_t)blockIdx.y * (size_t)a.n, slice, (unsigned)mb.stride, mb.members, mb.reduce, mb.inv};
    random_select_body<float, true, MemberCosts>(a, own_costs, src);
}

}  // namespace

void launch_random_select_members_batch(const icem_handle* h, const void* args_dev, const RandomPool<float>& pool, const RandomMembers& mb,
                                        int n_problems, hipStream_t st) {
    const dim3 grid(random_select_blocks(h->cfg.num_traj), n_problems);
    hipLaunchKernelGGL(random_select_members_batch_kernel, grid, dim3(RANDOM_SELECT_NT), 0, st, (const RandomSelectArgs<float>*)args_dev, pool, mb);
}

}  // namespace icem
