// k_rollout_wide_split_batch.hip -- the 16-bit-plane GEMM rollout with B problems per launch (icem_plan_step_batch, plan.hip):
// blockIdx.y = the problem, its argument block read from an array in device memory instead of the kernel-argument segment (scalar
// loads: the index is uniform).  The kernel runs the body of rollout_wide_split_kernel (wide_split_body.h; its device functions: wide_split_dev.h): the same text, so a
// problem's costs and candidate lists are bit for bit those of its own launch.  Every problem keeps its SOLO launch shape --
// gridDim.x = its own workgroups, the same tiles per workgroup, the same FIVE decision -- so the lists its workgroups emit are
// its solo lists; one problem of 256 rows is 4 workgroups on 256 CUs, B of them 4 B.  A unit of its own: the build stays parallel.
#include "wide_split_dev.h"

namespace icem {

namespace {

template <int NCT, int KIND, bool EXT, bool FIVE, bool F16>
__global__ __launch_bounds__(64 * SPLIT_WAVES) void rollout_wide_split_batch_kernel(const WideRolloutArgs* __restrict__ args) {
    const WideRolloutArgs a = from_device(args[blockIdx.y]);
#include "wide_split_body.h"
}

}  // namespace

// ---- launcher (LAUNCH_FAMILIES, icem_fused.h): the key is the one the solo launcher recorded for every problem ----

void launch_rollout_wide_split_batch(const LaunchKey& k, const WideRolloutArgs* args_dev, const BatchBases&, int n, hipStream_t st) {
    wide_split_dispatch(k, [&](auto nct, auto kd, auto ext, auto fv, auto f16) {
        auto kfn = rollout_wide_split_batch_kernel<decltype(nct)::value, decltype(kd)::value, decltype(ext)::value, decltype(fv)::value, decltype(f16)::value>;
        const size_t lds = wide_split_lds_bytes(k);
        (void)hipFuncSetAttribute((const void*)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL(kfn, dim3(k.wgs[0], n), dim3(64 * SPLIT_WAVES), lds, st, args_dev);
    });
}

}  // namespace icem
