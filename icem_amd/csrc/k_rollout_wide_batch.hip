// k_rollout_wide_batch.hip -- the exact-f32 GEMM rollout and its row-by-row tail with B problems per launch (icem_plan_step_batch,
// plan.hip): blockIdx.y = the problem, its argument block read from an array in device memory instead of the kernel-argument
// segment (scalar loads: the index is uniform).  Each kernel runs the body of its by-value twin in k_rollout_wide.hip
// (wide_rollout_body.h, wide_rows_body.h): the same text, so a problem's costs and candidate lists are bit for bit those of its own launch.  Every
// problem keeps its SOLO launch shape -- gridDim.x = its own workgroups, tile tile0 = wave * gridDim.x + blockIdx.x as alone -- so
// the lists its workgroups emit are its solo lists.  A unit of its own: the build stays parallel.
#include "wide_rollout_dev.h"

namespace icem {

namespace {

template <int NT, int KIND, int WAVES, bool EXT>
__global__ __launch_bounds__(64 * WAVES) void rollout_wide_batch_kernel(const WideRolloutArgs* __restrict__ args) {
    const WideRolloutArgs a = from_device(args[blockIdx.y]);
#include "wide_rollout_body.h"
}

template <int KIND>
__global__ __launch_bounds__(384) void rollout_rows_wide_batch_kernel(const WideRowsArgs* __restrict__ args) {
    const WideRowsArgs a = from_device(args[blockIdx.y]);
#include "wide_rows_body.h"
}

}  // namespace

// ---- launchers (LAUNCH_FAMILIES, icem_fused.h): the key is the one the solo launcher recorded for every problem ----

void launch_rollout_wide_batch(const LaunchKey& k, const WideRolloutArgs* args_dev, const BatchBases&, int n, hipStream_t st) {
    wide_dispatch(k, [&](auto nt, auto kd, auto ext) {
        auto kfn = rollout_wide_batch_kernel<decltype(nt)::value, decltype(kd)::value, WIDE_WAVES, decltype(ext)::value>;
        const size_t lds = wide_lds_bytes(k);
        (void)hipFuncSetAttribute((const void*)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL(kfn, dim3(k.wgs[0], n), dim3(64 * WIDE_WAVES), lds, st, args_dev);
    });
}

void launch_rollout_rows_wide_batch(const LaunchKey& k, const WideRowsArgs* args_dev, const BatchBases&, int n, hipStream_t st) {
    if (k.kind == 1) hipLaunchKernelGGL((rollout_rows_wide_batch_kernel<1>), dim3(k.wgs[0], n), dim3(384), 0, st, args_dev);
    else hipLaunchKernelGGL((rollout_rows_wide_batch_kernel<0>), dim3(k.wgs[0], n), dim3(384), 0, st, args_dev);
}

}  // namespace icem
