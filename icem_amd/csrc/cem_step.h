// cem_step.h -- what the host side of icem_plan_step_cem / icem_plan_step_cem_batch and of icem_plan_step_cem_learned /
// icem_plan_step_cem_learned_batch (cem_step.hip) asks of its kernels (k_cem.hip).
// Internal; not part of the public ABI.
#pragma once
#include "host_common.h"
#include "cem_dev.h"

namespace icem {

// cem_sample_kernel: n rows of [h, d] from (mean, std, lower, upper), device uniforms; tpw rows per workgroup
template <typename T>
struct CemSampleArgs {
    int n, h, d, tpw;
    const T* mean;
    const T* std;
    const T* lower;
    const T* upper;
    uint32_t seed_lo, seed_hi, off_lo, off_hi;
    T* out;
};

// the step's sampler serves this handle's shape (its LDS holds the three probability tables and at least one row); where it does
// not, the step launches the operator's kernel
bool cem_sample_ok(const icem_handle* h);
int launch_cem_sample(const icem_handle* h, int n, const void* mean, const void* std, const void* lower, const void* upper,
                      uint64_t offset, void* out, hipStream_t st);
// selection + gather + refit + bounds (+ epilogue) in one workgroup: f32 on update_small_kernel's body, f64 on select_refit_kernel's
void launch_cem_update(const UpdateSmallArgs& u, const CemTailArgs<float>& t, hipStream_t st);
void launch_cem_update(const SelectArgs<double>& s, int* idx_out, const CemTailArgs<double>& t, hipStream_t st);

// ---- icem_plan_step_cem_batch: the same three kernels' bodies for B problems per launch, argument blocks in a device array ----
// the update kernels' blocks (the solo kernels take the members one by one)
struct CemUpdateF32Args {
    UpdateSmallArgs u;
    CemTailArgs<float> t;
};
struct CemUpdateF64Args {
    SelectArgs<double> s;
    int* idx_out;
    CemTailArgs<double> t;
};
// the sampler's block of the handle's dtype -> dst (zeroed by the caller; every byte defined); offset_rel: relative to the
// problem's entry of BatchBases
size_t cem_sample_block_bytes(const icem_handle* h);
void cem_sample_block(const icem_handle* h, int n, const void* mean, const void* std, const void* lower, const void* upper,
                      uint64_t offset_rel, void* out, void* dst);
// grid (ceil(n_rows / tpw), n_problems): all problems draw n_rows rows
void launch_cem_sample_batch(const icem_handle* h, int n_rows, const void* args_dev, const BatchBases& bases, int n_problems, hipStream_t st);
// the same launch (f32 handles) whose workgroups of blockIdx.x == 0 also copy their problem's observation og.src[p] [og.width]
// to og.dst + p * og.width: the first iteration's launch of icem_plan_step_cem_learned_batch builds the batched RSSM rollout's
// contiguous observation table on the way (ObsGather: icem_fused.h)
void launch_cem_sample_gather_batch(const icem_handle* h, int n_rows, const void* args_dev, const BatchBases& bases, const ObsGather& og,
                                    int n_problems, hipStream_t st);
// one workgroup per problem; hd: the dynamic LDS of cem_tail's stage
void launch_cem_update_batch(const CemUpdateF32Args* args_dev, int n_problems, int hd, hipStream_t st);
void launch_cem_update_batch(const CemUpdateF64Args* args_dev, int n_problems, int hd, hipStream_t st);

// ---- icem_plan_step_cem_learned_models: the f32 update whose pool costs are not in memory yet -- it reduces them itself from the
// members' (UpdateMembersArgs, icem_fused.h: the same fields with the same meaning, the same arithmetic -- MemberCosts,
// update_small_body.h) and leaves the reduced cost in costs[i] as well.  u.u.costs is unused.
struct CemUpdateMembersArgs {
    CemUpdateF32Args c;
    const float* member_costs;   // [members, stride]
    float* costs;                // [c.u.n] out: the reduced costs
    int members, reduce;         // reduce: ICEM_RSSM_REDUCE_MEAN / _MAX
    int stride, row0;            // the member stride (all problems' rows) and this problem's first row
    float inv;                   // (float)(1.0 / members)
};
void launch_cem_update_members_batch(const CemUpdateMembersArgs* args_dev, int n_problems, int hd, hipStream_t st);

}  // namespace icem
