// k_cem.hip -- the kernels of icem_plan_step_cem and icem_plan_step_cem_batch (cem_step.hip), the CEM baseline's MPC step
// (MpcCemStd.get_action, icem/controllers/mpc.py:200-262) as a chain of launches, for one planner or for B (the *_batch_kernel
// twins: the same bodies, blockIdx.y / blockIdx.x = the problem, the argument blocks in a device array):
//   cem_sample_kernel      icem_sample_truncnorm's draw (mpc.py:188-198) with the three probability tables Phi(lower),
//                          Phi(-upper) and Phi(upper) - Phi(lower) -- functions of (t, j) alone -- computed once per workgroup
//                          into LDS, and a workgroup's rows staged in LDS and stored as one contiguous span
//   cem_update_*_kernel    one workgroup: selection + gather + refit (mpc.py:270-281) by the body of the operator's kernel --
//                          update_small_kernel's in f32, select_refit_kernel's in f64 --, then _update_bounds (mpc.py:290-301)
//                          and, behind the last iteration, get_action's epilogue (mpc.py:230-245): cem_dev.h::cem_tail
// The arithmetic of every value is a device function shared with the operator that computes it: the step's bits are theirs.
// icem_plan_step_cem_learned* (the same step through the declared RSSM) launches these kernels around the RSSM's rollout;
// its batch's first sampler launch is cem_sample_gather_batch_kernel, which also builds the batch's observation table.
// icem_plan_step_cem_learned_models' update kernel, which reduces an ensemble's member costs on the way to its keys, is
// k_cem_members.hip's: a unit of its own, so that the code of the kernels here is what it was.
#include "update_small_body.h"
#include "generic_dev.h"
#include "cem_step.h"
#include "cem_update_dev.h"   // from_device of the f32 update's blocks

namespace icem {

namespace {

// One thread per (trajectory, dim) row, as sample_truncnorm_kernel: word t of the row's stream is the uniform of step t.
// LDS: pa [h, d] | qb [h, d] | pd [h, d] | tile [tpw, h, d].
// (the body of cem_sample_kernel and of cem_sample_batch_kernel: one device function, the same device code)
template <typename T, int ROUNDS>
__device__ __forceinline__ void cem_sample_body(const CemSampleArgs<T>& a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int tid = threadIdx.x;
    const int hd = a.h * a.d;
    T* pa = reinterpret_cast<T*>(smem_raw);
    T* qb = pa + hd;
    T* pd = qb + hd;
    T* tile = pd + hd;
    for (int e = tid; e < hd; e += WG) {
        const T p = std_normal_cdf(a.lower[e]), q = std_normal_cdf(a.upper[e]);
        pa[e] = p;
        qb[e] = std_normal_cdf(-a.upper[e]);
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
            const T z = truncnorm_quantile<T>(word_uniform<T>(x), pa[c], qb[c], pd[c], a.lower[c], a.upper[c]);
            row[c] = fmad(z, a.std[c], a.mean[c]);
        }
    }
    __syncthreads();
    T* out = a.out + (size_t)n_base * hd;
    const int total = n_here * hd;
    for (int e = tid; e < total; e += WG) out[e] = tile[e];
}

template <typename T, int ROUNDS>
__global__ __launch_bounds__(WG) void cem_sample_kernel(CemSampleArgs<T> a) {
    cem_sample_body<T, ROUNDS>(a);
}

// ---- B problems per launch (icem_plan_step_cem_batch): the argument blocks in device memory, their pointers re-read as global
// addresses (fused_dev.h: gptr) ----
template <typename T>
__device__ __forceinline__ CemSampleArgs<T> from_device(const CemSampleArgs<T>& m) {
    CemSampleArgs<T> a = m;
    a.mean = gptr(m.mean), a.std = gptr(m.std), a.lower = gptr(m.lower), a.upper = gptr(m.upper), a.out = gptr(m.out);
    return a;
}
// (the CEM step's selection: every row a sampled one, no kept elites, nothing to wait for, never the step's "last")
__device__ __forceinline__ SelectArgs<double> from_device(const SelectArgs<double>& m) {
    SelectArgs<double> s = m;
    s.costs = gptr(m.costs), s.actions = gptr(m.actions), s.dbg = nullptr;
    MergeArgs<double>& a = s.m;
    a.records = nullptr, a.elites_cur = gptr(m.m.elites_cur), a.elites_cost_cur = gptr(m.m.elites_cost_cur);
    a.elites_next = gptr(m.m.elites_next), a.elites_cost_next = gptr(m.m.elites_cost_next);
    a.mean_in = gptr(m.m.mean_in), a.std_in = gptr(m.m.std_in), a.mean = gptr(m.m.mean), a.std = gptr(m.m.std);
    a.low = gptr(m.m.low), a.high = gptr(m.m.high), a.executed = gptr(m.m.executed), a.best_cost = gptr(m.m.best_cost);
    a.xw = XchgWait{};
    return s;
}

// blockIdx.y = the problem; the block's stream offset is relative to the step's base of that problem (BatchBases): it holds `it`
template <typename T, int ROUNDS>
__global__ __launch_bounds__(WG) void cem_sample_batch_kernel(const CemSampleArgs<T>* __restrict__ args, BatchBases bases) {
    CemSampleArgs<T> a = from_device(args[blockIdx.y]);
    add_base64(a.off_lo, a.off_hi, bases.v[blockIdx.y]);
    cem_sample_body<T, ROUNDS>(a);
}

// cem_sample_batch_kernel for the first iteration of icem_plan_step_cem_learned_batch: workgroup 0 of a problem also copies its
// observation into the batch's contiguous [n, og.width] table, which the batched RSSM rollout reads (as sample_folded_batch_kernel
// does for icem_plan_step_learned_batch, k_sample.hip) -- the callers' observation buffers need not be adjacent, and no launch
// is spent on it
template <typename T, int ROUNDS>
__global__ __launch_bounds__(WG) void cem_sample_gather_batch_kernel(const CemSampleArgs<T>* __restrict__ args, BatchBases bases, ObsGather og) {
    if (blockIdx.x == 0) {
        const float* src = og.src[blockIdx.y];
        for (int e = threadIdx.x; e < og.width; e += WG) og.dst[(size_t)blockIdx.y * og.width + e] = src[e];
    }
    CemSampleArgs<T> a = from_device(args[blockIdx.y]);
    add_base64(a.off_lo, a.off_hi, bases.v[blockIdx.y]);
    cem_sample_body<T, ROUNDS>(a);
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

// one workgroup per problem (blockIdx.x)
__global__ __launch_bounds__(1024) void cem_update_f32_batch_kernel(const CemUpdateF32Args* __restrict__ args) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const UpdateSmallArgs u = from_device(args[blockIdx.x].u);
    const CemTailArgs<float> t = from_device(args[blockIdx.x].t);
    update_small_body<false>(u, nullptr);
    __syncthreads();
    cem_tail<float, 1024>(t, reinterpret_cast<float*>(smem_raw));
}

__global__ __launch_bounds__(SELECT_NT) void cem_update_f64_batch_kernel(const CemUpdateF64Args* __restrict__ args) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const SelectArgs<double> s = from_device(args[blockIdx.x].s);
    int* idx_out = gptr(args[blockIdx.x].idx_out);
    const CemTailArgs<double> t = from_device(args[blockIdx.x].t);
    select_refit_body<double>(s, idx_out);
    __syncthreads();
    cem_tail<double, SELECT_NT>(t, reinterpret_cast<double*>(smem_raw));
}

constexpr size_t CEM_SAMPLE_LDS_MAX = 64 * 1024;

// rows per workgroup: one thread per (row, dim), and the tile beside the three tables within the LDS bound (0: no room)
int cem_sample_tpw(const icem_handle* h) {
    const size_t row = (size_t)h->hd * h->tsize;
    if (row == 0 || 4 * row > CEM_SAMPLE_LDS_MAX) return 0;
    return (int)std::min<size_t>((size_t)(WG / h->cfg.act_dim), CEM_SAMPLE_LDS_MAX / row - 3);
}

}  // namespace

bool cem_sample_ok(const icem_handle* h) { return h->cfg.act_dim >= 1 && h->cfg.act_dim <= WG && cem_sample_tpw(h) >= 1; }

int launch_cem_sample(const icem_handle* h, int n, const void* mean, const void* std, const void* lower, const void* upper,
                      uint64_t offset, void* out, hipStream_t st) {
    const icem_config& c = h->cfg;
    const int tpw = cem_sample_tpw(h);
    const int grid = (n + tpw - 1) / tpw;
    const size_t lds = (size_t)(3 + tpw) * h->hd * h->tsize;
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

size_t cem_sample_block_bytes(const icem_handle* h) { return h->cfg.dtype == ICEM_F64 ? sizeof(CemSampleArgs<double>) : sizeof(CemSampleArgs<float>); }

template <typename T>
static void sample_block_t(const icem_handle* h, int n, const void* mean, const void* std, const void* lower, const void* upper,
                           uint64_t offset_rel, void* out, void* dst) {
    const icem_config& c = h->cfg;
    CemSampleArgs<T>& a = *(CemSampleArgs<T>*)dst;   // (no padding: four ints, four pointers, four words, a pointer)
    a.n = n, a.h = c.horizon, a.d = c.act_dim, a.tpw = cem_sample_tpw(h);
    a.mean = (const T*)mean, a.std = (const T*)std, a.lower = (const T*)lower, a.upper = (const T*)upper;
    a.seed_lo = (uint32_t)c.seed, a.seed_hi = (uint32_t)(c.seed >> 32);
    a.off_lo = (uint32_t)offset_rel, a.off_hi = (uint32_t)(offset_rel >> 32);
    a.out = (T*)out;
}

void cem_sample_block(const icem_handle* h, int n, const void* mean, const void* std, const void* lower, const void* upper,
                      uint64_t offset_rel, void* out, void* dst) {
    if (h->cfg.dtype == ICEM_F64) sample_block_t<double>(h, n, mean, std, lower, upper, offset_rel, out, dst);
    else sample_block_t<float>(h, n, mean, std, lower, upper, offset_rel, out, dst);
}

// (the launch shape of launch_cem_sample for every problem: the handles of a batch share the configuration)
void launch_cem_sample_batch(const icem_handle* h, int n_rows, const void* args_dev, const BatchBases& bases, int n_problems, hipStream_t st) {
    const icem_config& c = h->cfg;
    const int tpw = cem_sample_tpw(h);
    const dim3 grid((n_rows + tpw - 1) / tpw, n_problems);
    const size_t lds = (size_t)(3 + tpw) * h->hd * h->tsize;
#define ICEM_CSB(T, R) hipLaunchKernelGGL((cem_sample_batch_kernel<T, R>), grid, dim3(WG), lds, st, (const CemSampleArgs<T>*)args_dev, bases)
    if (c.dtype == ICEM_F64) {
        if (c.rng_rounds == 7) ICEM_CSB(double, 7); else ICEM_CSB(double, 10);
    } else {
        if (c.rng_rounds == 7) ICEM_CSB(float, 7); else ICEM_CSB(float, 10);
    }
#undef ICEM_CSB
}

// (f32 handles: the learned-dynamics step serves no other)
void launch_cem_sample_gather_batch(const icem_handle* h, int n_rows, const void* args_dev, const BatchBases& bases, const ObsGather& og,
                                    int n_problems, hipStream_t st) {
    const int tpw = cem_sample_tpw(h);
    const dim3 grid((n_rows + tpw - 1) / tpw, n_problems);
    const size_t lds = (size_t)(3 + tpw) * h->hd * h->tsize;
    if (h->cfg.rng_rounds == 7)
        hipLaunchKernelGGL((cem_sample_gather_batch_kernel<float, 7>), grid, dim3(WG), lds, st, (const CemSampleArgs<float>*)args_dev, bases, og);
    else
        hipLaunchKernelGGL((cem_sample_gather_batch_kernel<float, 10>), grid, dim3(WG), lds, st, (const CemSampleArgs<float>*)args_dev, bases, og);
}

void launch_cem_update_batch(const CemUpdateF32Args* args_dev, int n_problems, int hd, hipStream_t st) {
    hipLaunchKernelGGL(cem_update_f32_batch_kernel, dim3(n_problems), dim3(1024), (size_t)hd * sizeof(float), st, args_dev);
}

void launch_cem_update_batch(const CemUpdateF64Args* args_dev, int n_problems, int hd, hipStream_t st) {
    hipLaunchKernelGGL(cem_update_f64_batch_kernel, dim3(n_problems), dim3(SELECT_NT), (size_t)hd * sizeof(double), st, args_dev);
}

void launch_cem_update(const UpdateSmallArgs& u, const CemTailArgs<float>& t, hipStream_t st) {
    hipLaunchKernelGGL(cem_update_f32_kernel, dim3(1), dim3(1024), (size_t)t.h * t.d * sizeof(float), st, u, t);
}

void launch_cem_update(const SelectArgs<double>& s, int* idx_out, const CemTailArgs<double>& t, hipStream_t st) {
    hipLaunchKernelGGL(cem_update_f64_kernel, dim3(1), dim3(SELECT_NT), (size_t)t.h * t.d * sizeof(double), st, s, idx_out, t);
}

}  // namespace icem
