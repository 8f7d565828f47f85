// k_random.hip -- the kernels of icem_plan_step_random and icem_plan_step_random_batch (random_step.hip), the random-shooting
// baseline's MPC step (MpcRandom.get_action, icem/controllers/mpc.py:114-138) as a chain of launches, for one planner or for B
// (the *_batch_kernel twins: the same bodies, blockIdx.y = the problem, the argument blocks in a device array):
//   random_sample_kernel   icem_sample_piecewise's pool (mpc.py:96-109).  sample_piecewise_kernel seeds a Philox / xoshiro stream
//                          per ELEMENT although change_freq + 1 consecutive sample() calls share one draw per dimension; here a
//                          workgroup owns RANDOM_SPAN consecutive elements, draws each (block, dimension) value they need once
//                          into LDS -- the operator's arithmetic, the same bits -- and stores its span from there, four
//                          elements per store
//   random_select_kernel   np.argmin(costs) (mpc.py:122) as icem_topk_sorted(costs, 1) gives it -- (cost, index) order, NaN = +inf
//                          -- and the gathers behind it.  A workgroup per RANDOM_SLICE costs; of several, each leaves its best
//                          pair and draws a ticket, and the one that draws the last merges them (no workgroup waits for another;
//                          tools/ubench/last_block.hip) and resets the ticket; the finisher copies the best row and writes result
#include "random_dev.h"   // the bodies (shared with k_random_learned.hip), from_device

namespace icem {

namespace {

template <typename T, int ROUNDS>
__global__ __launch_bounds__(WG) void random_sample_kernel(RandomSampleArgs<T> a) {
    random_sample_body<T, ROUNDS>(a);
}

// blockIdx.y = the problem; its call offset by value (the block holds 0)
template <typename T, int ROUNDS>
__global__ __launch_bounds__(WG) void random_sample_batch_kernel(const RandomSampleArgs<T>* __restrict__ args, BatchBases bases) {
    RandomSampleArgs<T> a = from_device(args[blockIdx.y]);
    a.call_offset += (long long)bases.v[blockIdx.y];
    random_sample_body<T, ROUNDS>(a);
}

template <typename T>
__global__ __launch_bounds__(RANDOM_SELECT_NT) void random_select_kernel(RandomSelectArgs<T> a) {
    random_select_body<T>(a);
}

// blockIdx.y = the problem (gridDim.x = the slices of ONE problem: the handles of a batch share num_traj)
template <typename T>
__global__ __launch_bounds__(RANDOM_SELECT_NT) void random_select_batch_kernel(const RandomSelectArgs<T>* __restrict__ args) {
    const RandomSelectArgs<T> a = from_device(args[blockIdx.y]);
    random_select_body<T>(a);
}

template <typename T>
void sample_block_t(const icem_handle* h, const icem_random_buffers& b, int change_freq, long long call_offset, long long first_block,
                    const void* u, void* dst) {
    const icem_config& c = h->cfg;
    RandomSampleArgs<T>& a = *(RandomSampleArgs<T>*)dst;   // (no padding: three 64-bit values, two ints, three pointers, two words, a pointer)
    a.total = (long long)c.num_traj * c.horizon * c.act_dim;
    a.call_offset = call_offset, a.first_block = first_block;
    a.d = c.act_dim, a.freq = change_freq;
    a.low = (const T*)b.low, a.high = (const T*)b.high, a.u = (const T*)u;
    a.seed_lo = (uint32_t)c.seed, a.seed_hi = (uint32_t)(c.seed >> 32);
    a.out = (T*)b.actions;
}

template <typename T>
void select_block_t(const icem_handle* h, const icem_random_buffers& b, void* result_row, void* dst) {
    const icem_config& c = h->cfg;
    RandomSelectArgs<T>& a = *(RandomSelectArgs<T>*)dst;   // (no padding: four ints, seven pointers)
    a.n = c.num_traj, a.hd = h->hd, a.d = c.act_dim;
    // which cost icem_topk_sorted(costs, 1) reports (abi.hip): its one-launch f32 form, or the generic partial + final pair
    a.canon = (h->use_fast && c.dtype == ICEM_F32 && topk_small_ok(c.num_traj, 1)) ? 1 : 0;
    a.costs = (const T*)b.costs, a.actions = (const T*)b.actions;
    a.best_actions = (T*)b.best_actions, a.result = (T*)b.result, a.result_row = (T*)result_row;
    const int nblk = random_select_blocks(c.num_traj);
    a.part = nblk > 1 ? (unsigned long long*)h->random_ws.dev : nullptr;
    a.ticket = nblk > 1 ? (unsigned*)((unsigned long long*)h->random_ws.dev + 2 * (size_t)nblk) : nullptr;
}

size_t sample_lds(const icem_handle* h) { return random_table_elems(h->cfg.act_dim) * h->tsize; }
int sample_grid(const icem_handle* h) {
    const long long total = (long long)h->cfg.num_traj * h->cfg.horizon * h->cfg.act_dim;
    return (int)((total + RANDOM_SPAN - 1) / RANDOM_SPAN);
}

}  // namespace

size_t random_sample_block_bytes(const icem_handle* h) {
    return h->cfg.dtype == ICEM_F64 ? sizeof(RandomSampleArgs<double>) : sizeof(RandomSampleArgs<float>);
}
size_t random_select_block_bytes(const icem_handle* h) {
    return h->cfg.dtype == ICEM_F64 ? sizeof(RandomSelectArgs<double>) : sizeof(RandomSelectArgs<float>);
}

void random_sample_block(const icem_handle* h, const icem_random_buffers& b, int change_freq, long long call_offset, long long first_block,
                         const void* u, void* dst) {
    if (h->cfg.dtype == ICEM_F64) sample_block_t<double>(h, b, change_freq, call_offset, first_block, u, dst);
    else sample_block_t<float>(h, b, change_freq, call_offset, first_block, u, dst);
}

void random_select_block(const icem_handle* h, const icem_random_buffers& b, void* result_row, void* dst) {
    if (h->cfg.dtype == ICEM_F64) select_block_t<double>(h, b, result_row, dst);
    else select_block_t<float>(h, b, result_row, dst);
}

void launch_random_sample(const icem_handle* h, const void* block, hipStream_t st) {
    const dim3 grid(sample_grid(h));
    const size_t lds = sample_lds(h);
#define ICEM_RS(T, R) hipLaunchKernelGGL((random_sample_kernel<T, R>), grid, dim3(WG), lds, st, *(const RandomSampleArgs<T>*)block)
    if (h->cfg.dtype == ICEM_F64) {
        if (h->cfg.rng_rounds == 7) ICEM_RS(double, 7); else ICEM_RS(double, 10);
    } else {
        if (h->cfg.rng_rounds == 7) ICEM_RS(float, 7); else ICEM_RS(float, 10);
    }
#undef ICEM_RS
}

void launch_random_sample_batch(const icem_handle* h, const void* args_dev, const BatchBases& bases, int n_problems, hipStream_t st) {
    const dim3 grid(sample_grid(h), n_problems);
    const size_t lds = sample_lds(h);
#define ICEM_RSB(T, R) hipLaunchKernelGGL((random_sample_batch_kernel<T, R>), grid, dim3(WG), lds, st, (const RandomSampleArgs<T>*)args_dev, bases)
    if (h->cfg.dtype == ICEM_F64) {
        if (h->cfg.rng_rounds == 7) ICEM_RSB(double, 7); else ICEM_RSB(double, 10);
    } else {
        if (h->cfg.rng_rounds == 7) ICEM_RSB(float, 7); else ICEM_RSB(float, 10);
    }
#undef ICEM_RSB
}

void launch_random_select(const icem_handle* h, const void* block, hipStream_t st) {
    const dim3 grid(random_select_blocks(h->cfg.num_traj));
    if (h->cfg.dtype == ICEM_F64)
        hipLaunchKernelGGL(random_select_kernel<double>, grid, dim3(RANDOM_SELECT_NT), 0, st, *(const RandomSelectArgs<double>*)block);
    else
        hipLaunchKernelGGL(random_select_kernel<float>, grid, dim3(RANDOM_SELECT_NT), 0, st, *(const RandomSelectArgs<float>*)block);
}

void launch_random_select_batch(const icem_handle* h, const void* args_dev, int n_problems, hipStream_t st) {
    const dim3 grid(random_select_blocks(h->cfg.num_traj), n_problems);
    if (h->cfg.dtype == ICEM_F64)
        hipLaunchKernelGGL(random_select_batch_kernel<double>, grid, dim3(RANDOM_SELECT_NT), 0, st, (const RandomSelectArgs<double>*)args_dev);
    else
        hipLaunchKernelGGL(random_select_batch_kernel<float>, grid, dim3(RANDOM_SELECT_NT), 0, st, (const RandomSelectArgs<float>*)args_dev);
}

}  // namespace icem
