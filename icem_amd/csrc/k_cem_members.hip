// k_cem_members.hip -- the update kernel of icem_plan_step_cem_learned_models (cem_step.hip): the CEM baseline's MPC step through
// an ensemble's members or a model per problem.  It is cem_update_f32_batch_kernel (k_cem.hip) with the candidate's cost coming out
// of the members' costs [members, stride] that the ONE rollout launch left, not out of a plain load: update_small_body<false,
// MemberCosts> (update_small_body.h: rssm_ensemble_reduce_kernel's arithmetic operation for operation, all of a row's member
// loads requested before the first is consumed, the reduced cost written to the problem's costs as well), then cem_tail.
// A translation unit of its own: in k_cem.hip a third instantiation of the body moved instructions in the other two kernels.
#include "update_small_body.h"
#include "generic_dev.h"
#include "cem_step.h"
#include "cem_update_dev.h"

namespace icem {

namespace {

__global__ __launch_bounds__(1024) void cem_update_members_batch_kernel(const CemUpdateMembersArgs* __restrict__ args) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const CemUpdateMembersArgs& g = args[blockIdx.x];
    const UpdateSmallArgs u = from_device(g.c.u);
    const CemTailArgs<float> t = from_device(g.c.t);
    const MemberCosts src{gptr(g.member_costs) + g.row0, gptr(g.costs), (unsigned)g.stride, g.members, g.reduce, g.inv};
    update_small_body<false>(u, nullptr, src);
    __syncthreads();
    cem_tail<float, 1024>(t, reinterpret_cast<float*>(smem_raw));
}

}  // namespace

void launch_cem_update_members_batch(const CemUpdateMembersArgs* args_dev, int n_problems, int hd, hipStream_t st) {
    hipLaunchKernelGGL(cem_update_members_batch_kernel, dim3(n_problems), dim3(1024), (size_t)hd * sizeof(float), st, args_dev);
}

}  // namespace icem
