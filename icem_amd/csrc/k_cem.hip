// k_cem.hip -- the kernels of icem_plan_step_cem (cem_step.hip), the CEM baseline's MPC step (MpcCemStd.get_action,
// icem/controllers/mpc.py:200-262) as a chain of launches:
//   cem_sample_kernel      icem_sample_truncnorm's draw (mpc.py:188-198) with the two probability tables Phi(lower) and
//                          Phi(upper) - Phi(lower) -- functions of (t, j) alone -- computed once per workgroup into LDS, and a
//                          workgroup's rows staged in LDS and stored as one contiguous span
//   cem_update_*_kernel    one workgroup: selection + gather + refit (mpc.py:270-281) by the body of the operator's kernel --
//                          update_small_kernel's in f32, select_refit_kernel's in f64 --, then _update_bounds (mpc.py:290-301)
//                          and, behind the last iteration, get_action's epilogue (mpc.py:230-245): cem_dev.h::cem_tail
// The arithmetic of every value is a device function shared with the operator that computes it: the step's bits are theirs.
#include "update_small_body.h"
#include "generic_dev.h"
#include "cem_step.h"

namespace icem {

namespace {

// One thread per (trajectory, dim) row, as sample_truncnorm_kernel: word t of the row's stream is the uniform of step t.
// LDS: pa [h, d] | pd [h, d] | tile [tpw, h, d].
template <typename T, int ROUNDS>
__global__ __launch_bounds__(WG) void cem_sample_kernel(CemSampleArgs<T> a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int tid = threadIdx.x;
    const int hd = a.h * a.d;
    T* pa = reinterpret_cast<T*>(smem_raw);
    T* pd = pa + hd;
    T* tile = pd + hd;
    for (int e = tid; e < hd; e += WG) {
        const T p = std_normal_cdf(a.lower[e]), q = std_normal_cdf(a.upper[e]);
        pa[e] = p;
        pd[e] = q - p;
    }
    __syncthreads();
    const int n_base = blockIdx.x * a.tpw;
    const int n_here = min(a.tpw, a.n - n_base);
    if (tid < n_here * a.d) {
        const int nl = tid / a.d, j = tid - nl * a.d;
        Xoshiro128pp rng = row_stream<ROUNDS>((uint32_t)(n_base + nl), (uint32_t)j, a.off_lo, a.off_hi, a.seed_lo, a.seed_hi);
        T* row = tile + (size_t)nl * hd;
        for (int t = 0; t < a.h; ++t) {
            const int c = t * a.d + j;
            const uint32_t x = rng.next();
            const T z = truncnorm_quantile<T>(word_uniform<T>(x), pa[c], pd[c], a.lower[c], a.upper[c]);
            row[c] = fmad(z, a.std[c], a.mean[c]);
        }
    }
    __syncthreads();
    T* out = a.out + (size_t)n_base * hd;
    const int total = n_here * hd;
    for (int e = tid; e < total; e += WG) out[e] = tile[e];
}

__global__ __launch_bounds__(1024) void cem_update_f32_kernel(UpdateSmallArgs u, CemTailArgs<float> t) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    update_small_body<false>(u, nullptr);
    __syncthreads();
    cem_tail<float, 1024>(t, reinterpret_cast<float*>(smem_raw));
}

__global__ __launch_bounds__(SELECT_NT) void cem_update_f64_kernel(SelectArgs<double> s, int* idx_out, CemTailArgs<double> t) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];   // (the body's new_mean: unused, s.m.last == 0)
    select_refit_body<double>(s, idx_out);
    __syncthreads();
    cem_tail<double, SELECT_NT>(t, reinterpret_cast<double*>(smem_raw));
}

constexpr size_t CEM_SAMPLE_LDS_MAX = 64 * 1024;

// rows per workgroup: one thread per (row, dim), and the tile beside the two tables within the LDS bound (0: no room)
int cem_sample_tpw(const icem_handle* h) {
    const size_t row = (size_t)h->hd * h->tsize;
    if (row == 0 || 3 * row > CEM_SAMPLE_LDS_MAX) return 0;
    return (int)std::min<size_t>((size_t)(WG / h->cfg.act_dim), CEM_SAMPLE_LDS_MAX / row - 2);
}

}  // namespace

bool cem_sample_ok(const icem_handle* h) { return h->cfg.act_dim >= 1 && h->cfg.act_dim <= WG && cem_sample_tpw(h) >= 1; }

int launch_cem_sample(const icem_handle* h, int n, const void* mean, const void* std, const void* lower, const void* upper,
                      uint64_t offset, void* out, hipStream_t st) {
    const icem_config& c = h->cfg;
    const int tpw = cem_sample_tpw(h);
    const int grid = (n + tpw - 1) / tpw;
    const size_t lds = (size_t)(2 + tpw) * h->hd * h->tsize;
#define ICEM_CS(T, R)                                                                                                       \
    do {                                                                                                                    \
        CemSampleArgs<T> a{n, c.horizon, c.act_dim, tpw, (const T*)mean, (const T*)std, (const T*)lower, (const T*)upper,    \
                           (uint32_t)c.seed, (uint32_t)(c.seed >> 32), (uint32_t)offset, (uint32_t)(offset >> 32), (T*)out}; \
        hipLaunchKernelGGL((cem_sample_kernel<T, R>), dim3(grid), dim3(WG), lds, st, a);                                    \
    } while (0)
    if (c.dtype == ICEM_F64) {
        if (c.rng_rounds == 7) ICEM_CS(double, 7); else ICEM_CS(double, 10);
    } else {
        if (c.rng_rounds == 7) ICEM_CS(float, 7); else ICEM_CS(float, 10);
    }
#undef ICEM_CS
    ICEM_HIP_TRY(hipGetLastError());
    return ICEM_OK;
}

void launch_cem_update(const UpdateSmallArgs& u, const CemTailArgs<float>& t, hipStream_t st) {
    hipLaunchKernelGGL(cem_update_f32_kernel, dim3(1), dim3(1024), (size_t)t.h * t.d * sizeof(float), st, u, t);
}

void launch_cem_update(const SelectArgs<double>& s, int* idx_out, const CemTailArgs<double>& t, hipStream_t st) {
    hipLaunchKernelGGL(cem_update_f64_kernel, dim3(1), dim3(SELECT_NT), (size_t)t.h * t.d * sizeof(double), st, s, idx_out, t);
}

}  // namespace icem
