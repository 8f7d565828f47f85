// k_random_learned.hip -- the kernels of icem_plan_step_random_learned_batch (random_step.hip): the random-shooting baseline's MPC
// step through the learned dynamics (the declared RSSM) for B planners at once.  The batched RSSM launch (launch_rssm_split_batch)
// scores rows that lie back to back, so problem p's rows are drawn into the slice [p * N, (p + 1) * N) of a pool owned by the first
// handle -- and, because a controller keeps its pool (MpcRandomHip._last_actions / _last_costs), into the problem's own buffers too:
//   random_sample_gather_batch_kernel   random_sample_body (random_dev.h) on the pool slice, every store mirrored into the problem's
//                                       own `actions`; the workgroups of blockIdx.x == 0 also copy their problem's observation into
//                                       the pool's [n, 230] table (as cem_sample_gather_batch_kernel, k_cem.hip)
//   random_select_pool_batch_kernel     random_select_body on the slice's costs and actions, every cost it reads stored into the
//                                       problem's own `costs`
// (icem_plan_step_random_learned_models' selection, which reduces an ensemble's member costs on the way to its keys, is
//  k_random_members.hip's: a unit of its own.)
// The argument blocks are byte for byte those of icem_plan_step_random_batch (the problem's OWN buffers); the pool's pointers travel
// by value and the slices follow from blockIdx.y.  The solo step launches the kernels of k_random.hip.
#include "random_dev.h"

namespace icem {

namespace {

// blockIdx.y = the problem; its call offset by value (the block holds 0).  A slice starts at p * total elements: 16-byte aligned
// or not as total goes (N = 17, h = 5, d = 6: 8 mod 16) whatever the problem's own buffer is -- random_sample_body decides the
// 16-byte store per destination
template <typename T, int ROUNDS>
__global__ __launch_bounds__(WG) void random_sample_gather_batch_kernel(const RandomSampleArgs<T>* __restrict__ args, BatchBases bases, ObsGather og,
                                                                        RandomPool<T> pool) {
    if (blockIdx.x == 0) {
        const float* src = og.src[blockIdx.y];
        for (int e = threadIdx.x; e < og.width; e += WG) og.dst[(size_t)blockIdx.y * og.width + e] = src[e];
    }
    RandomSampleArgs<T> a = from_device(args[blockIdx.y]);
    a.call_offset += (long long)bases.v[blockIdx.y];
    T* own = a.out;
    a.out = pool.actions + (size_t)blockIdx.y * (size_t)a.total;
    random_sample_body<T, ROUNDS, true>(a, own);
}

// blockIdx.y = the problem (gridDim.x = the slices of ONE problem: the handles of a batch share num_traj)
template <typename T>
__global__ __launch_bounds__(RANDOM_SELECT_NT) void random_select_pool_batch_kernel(const RandomSelectArgs<T>* __restrict__ args, RandomPool<T> pool) {
    RandomSelectArgs<T> a = from_device(args[blockIdx.y]);
    T* own_costs = const_cast<T*>(a.costs);
    a.costs = pool.costs + (size_t)blockIdx.y * (size_t)a.n;
    a.actions = pool.actions + (size_t)blockIdx.y * (size_t)a.n * (size_t)a.hd;
    random_select_body<T, true>(a, own_costs);
}

}  // namespace

void launch_random_sample_gather_batch(const icem_handle* h, const void* args_dev, const BatchBases& bases, const ObsGather& og,
                                       const RandomPool<float>& pool, int n_problems, hipStream_t st) {
    const long long total = (long long)h->cfg.num_traj * h->cfg.horizon * h->cfg.act_dim;
    const dim3 grid((unsigned)((total + RANDOM_SPAN - 1) / RANDOM_SPAN), n_problems);
    const size_t lds = random_table_elems(h->cfg.act_dim) * sizeof(float);
    if (h->cfg.rng_rounds == 7)
        hipLaunchKernelGGL((random_sample_gather_batch_kernel<float, 7>), grid, dim3(WG), lds, st, (const RandomSampleArgs<float>*)args_dev, bases, og, pool);
    else
        hipLaunchKernelGGL((random_sample_gather_batch_kernel<float, 10>), grid, dim3(WG), lds, st, (const RandomSampleArgs<float>*)args_dev, bases, og, pool);
}

void launch_random_select_pool_batch(const icem_handle* h, const void* args_dev, const RandomPool<float>& pool, int n_problems, hipStream_t st) {
    const dim3 grid(random_select_blocks(h->cfg.num_traj), n_problems);
    hipLaunchKernelGGL(random_select_pool_batch_kernel<float>, grid, dim3(RANDOM_SELECT_NT), 0, st, (const RandomSelectArgs<float>*)args_dev, pool);
}

}  // namespace icem
