// k_generic_batch.hip -- the generic float64 kernels of an MPC step with B problems per launch (icem_plan_step_batch_f64, plan.hip):
// blockIdx.y = the problem, its argument block read from an array in device memory instead of the kernel-argument segment.  Each
// kernel calls the body its solo twin in generic_kernels.hip calls (generic_dev.h): the same text, the same summation order, so a
// problem's outputs are bit for bit those of its own icem_plan_step.  The block is uniform per workgroup: it is read through a
// const __restrict__ pointer at a wave-uniform index (scalar loads), never copied per lane; only the sampler, which adds the
// step's noise base to its block's relative offset, keeps a (uniform) copy.  The problems of a batch share one configuration
// (admit_batch), hence one grid: no surplus workgroups.
#include "generic_dev.h"

namespace icem {

template <int HMAX, int ROUNDS>
__global__ __launch_bounds__(WG) void sample_clip_quad_batch_kernel(const SampleArgs<double>* __restrict__ args, BatchBases bases) {
    SampleArgs<double> a = args[blockIdx.y];
    const unsigned long long off = (((unsigned long long)a.off_hi << 32) | a.off_lo) + bases.v[blockIdx.y];
    a.off_lo = (uint32_t)off;
    a.off_hi = (uint32_t)(off >> 32);
    sample_clip_quad_body<double, HMAX, ROUNDS>(a);
}

__global__ __launch_bounds__(WG) void shift_elites_batch_kernel(const ShiftElitesArgs<double>* __restrict__ args) {
    const ShiftElitesArgs<double>& a = args[blockIdx.y];
    shift_elites_body<double>(a.n_reuse, a.h, a.d, a.elites, a.dst);
}

template <int O, int KIND>
__global__ __launch_bounds__(WG) void rollout_cost_rows_batch_kernel(const RolloutArgs<double>* __restrict__ args) {
    rollout_cost_rows_body<double, O, KIND>(args[blockIdx.y]);
}

template <int O, int KIND>
__global__ __launch_bounds__(WG) void rollout_cost_batch_kernel(const RolloutArgs<double>* __restrict__ args) {
    rollout_cost_body<double, O, KIND>(args[blockIdx.y]);
}

__global__ __launch_bounds__(SELECT_NT) void select_refit_batch_kernel(const SelectArgs<double>* __restrict__ args) {
    select_refit_body<double>(args[blockIdx.y]);
}

// ---- launchers (LAUNCH_FAMILIES, icem_fused.h): the key is the one the solo launcher recorded for every problem ----

void launch_gk_sample_batch(const LaunchKey& k, const SampleArgs<double>* args_dev, const BatchBases& bases, int n, hipStream_t st) {
    const dim3 grid(k.wgs[0], n);
    const size_t lds = gk_sample_quad_lds(k.waves, k.h, k.d, k.O, sizeof(double));
    if (k.O == 32) {
        if (k.form == 7) hipLaunchKernelGGL((sample_clip_quad_batch_kernel<32, 7>), grid, dim3(WG), lds, st, args_dev, bases);
        else hipLaunchKernelGGL((sample_clip_quad_batch_kernel<32, 10>), grid, dim3(WG), lds, st, args_dev, bases);
    } else {
        if (k.form == 7) hipLaunchKernelGGL((sample_clip_quad_batch_kernel<64, 7>), grid, dim3(WG), lds, st, args_dev, bases);
        else hipLaunchKernelGGL((sample_clip_quad_batch_kernel<64, 10>), grid, dim3(WG), lds, st, args_dev, bases);
    }
}

void launch_gk_shift_batch(const LaunchKey& k, const ShiftElitesArgs<double>* args_dev, const BatchBases&, int n, hipStream_t st) {
    hipLaunchKernelGGL(shift_elites_batch_kernel, dim3(k.wgs[0], n), dim3(WG), 0, st, args_dev);
}

#define ICEM_GK_WIDTHS(X) X(8) X(16) X(17) X(18) X(24) X(32)

void launch_gk_rollout_rows_batch(const LaunchKey& k, const RolloutArgs<double>* args_dev, const BatchBases&, int n, hipStream_t st) {
    const dim3 grid(k.wgs[0], n);
    const size_t lds = gk_rollout_rows_lds(k.O, k.h, k.d, sizeof(double));
    switch (k.O) {
#define ICEM_CASE(OV)                                                                                                          \
    case OV:                                                                                                                   \
        if (k.kind == ICEM_MODEL_TANH)                                                                                         \
            hipLaunchKernelGGL((rollout_cost_rows_batch_kernel<OV, ICEM_MODEL_TANH>), grid, dim3(WG), lds, st, args_dev);      \
        else                                                                                                                   \
            hipLaunchKernelGGL((rollout_cost_rows_batch_kernel<OV, ICEM_MODEL_LINEAR>), grid, dim3(WG), lds, st, args_dev);    \
        break;
        ICEM_GK_WIDTHS(ICEM_CASE)
#undef ICEM_CASE
        default:
            break;   // (the recording launcher admits these widths only)
    }
}

void launch_gk_rollout_thread_batch(const LaunchKey& k, const RolloutArgs<double>* args_dev, const BatchBases&, int n, hipStream_t st) {
    const dim3 grid(k.wgs[0], n);
    switch (k.O) {
#define ICEM_CASE(OV)                                                                                                          \
    case OV:                                                                                                                   \
        if (k.kind != ICEM_MODEL_TANH)                                                                                         \
            hipLaunchKernelGGL((rollout_cost_batch_kernel<OV, ICEM_MODEL_LINEAR>), grid, dim3(WG), 0, st, args_dev);           \
        else if constexpr (OV != 32)   /* gk_rollout_thread_batched: <32, tanh> spills registers and has no batched twin */    \
            hipLaunchKernelGGL((rollout_cost_batch_kernel<OV, ICEM_MODEL_TANH>), grid, dim3(WG), 0, st, args_dev);             \
        break;
        ICEM_GK_WIDTHS(ICEM_CASE)
#undef ICEM_CASE
        default:
            break;
    }
}

void launch_gk_select_batch(const LaunchKey& k, const SelectArgs<double>* args_dev, const BatchBases&, int n, hipStream_t st) {
    hipLaunchKernelGGL(select_refit_batch_kernel, dim3(1, n), dim3(SELECT_NT), (size_t)k.h * k.d * sizeof(double), st, args_dev);
}

}  // namespace icem
