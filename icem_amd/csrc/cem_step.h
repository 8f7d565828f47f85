// cem_step.h -- what the host side of icem_plan_step_cem (cem_step.hip) asks of its kernels (k_cem.hip).
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

// the step's sampler serves this handle's shape (its LDS holds the two probability tables and at least one row); where it does
// not, the step launches the operator's kernel
bool cem_sample_ok(const icem_handle* h);
int launch_cem_sample(const icem_handle* h, int n, const void* mean, const void* std, const void* lower, const void* upper,
                      uint64_t offset, void* out, hipStream_t st);
// selection + gather + refit + bounds (+ epilogue) in one workgroup: f32 on update_small_kernel's body, f64 on select_refit_kernel's
void launch_cem_update(const UpdateSmallArgs& u, const CemTailArgs<float>& t, hipStream_t st);
void launch_cem_update(const SelectArgs<double>& s, int* idx_out, const CemTailArgs<double>& t, hipStream_t st);

}  // namespace icem
