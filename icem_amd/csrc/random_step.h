// random_step.h -- what the host side of icem_plan_step_random / icem_plan_step_random_batch (random_step.hip) asks of its
// kernels (k_random.hip).  Internal; not part of the public ABI.
#pragma once
#include "host_common.h"

namespace icem {

// random_sample_kernel: the pool's `total` = N * h * d elements of icem_sample_piecewise; workgroup w owns the elements
// [w * RANDOM_SPAN, (w + 1) * RANDOM_SPAN).  call_offset: the solo launch's; a batch's block holds 0 and the problem's offset
// arrives by value (BatchBases)
template <typename T>
struct RandomSampleArgs {
    long long total, call_offset, first_block;
    int d, freq;
    const T* low;
    const T* high;
    const T* u;
    uint32_t seed_lo, seed_hi;
    T* out;
};

// random_select_kernel: workgroup w reduces the costs [w * RANDOM_SLICE, (w + 1) * RANDOM_SLICE) to their smallest
// (cost, index) pair; of several, the one that arrives last merges the partials; the finisher gathers.
// part [2 * workgroups] (cost bits | index) and ticket: the handle's (RandomWs); unused by a pool of one slice
template <typename T>
struct RandomSelectArgs {
    int n, hd, d;
    int canon;              // the cost is reported as the f32 one-launch top-k reports it (-0 -> +0), else as the generic pair does
    const T* costs;
    const T* actions;
    T* best_actions;
    T* result;              // [d + 2]
    T* result_row;          // a batch's row of `results`, or nullptr
    unsigned long long* part;
    unsigned* ticket;
};

constexpr int RANDOM_SPAN = 1024;      // pool elements per sampler workgroup (4 per thread: one vector store each)
constexpr int RANDOM_SLICE = 16384;    // costs per selection workgroup
constexpr int RANDOM_SELECT_NT = 1024;
constexpr size_t RANDOM_BLOCK_MAX = 96;   // room of either block on the host stack (random_step.hip)
static_assert(sizeof(RandomSampleArgs<double>) <= RANDOM_BLOCK_MAX && sizeof(RandomSelectArgs<double>) <= RANDOM_BLOCK_MAX, "RANDOM_BLOCK_MAX");

inline int random_select_blocks(int n) { return (n + RANDOM_SLICE - 1) / RANDOM_SLICE; }
// bytes of a handle's RandomWs for a pool of n rows
inline size_t random_ws_bytes(int n) { return (size_t)random_select_blocks(n) * 2 * sizeof(unsigned long long) + 64; }

// the blocks of the handle's dtype -> dst (zeroed by the caller; every byte defined)
size_t random_sample_block_bytes(const icem_handle* h);
size_t random_select_block_bytes(const icem_handle* h);
void random_sample_block(const icem_handle* h, const icem_random_buffers& b, int change_freq, long long call_offset, long long first_block,
                         const void* u, void* dst);
void random_select_block(const icem_handle* h, const icem_random_buffers& b, void* result_row, void* dst);
// solo: the block by value
void launch_random_sample(const icem_handle* h, const void* block, hipStream_t st);
void launch_random_select(const icem_handle* h, const void* block, hipStream_t st);
// B problems of one configuration: blockIdx.y = the problem, the blocks in a device array, the call offsets by value
void launch_random_sample_batch(const icem_handle* h, const void* args_dev, const BatchBases& bases, int n_problems, hipStream_t st);
void launch_random_select_batch(const icem_handle* h, const void* args_dev, int n_problems, hipStream_t st);

// ---- icem_plan_step_random_learned_batch (k_random_learned.hip): the same blocks, the rows scored in a pool ----
// the pool of a batch's first handle (LearnedCtx), by value: problem p's slice is actions + p * N * hd, costs + p * N
template <typename T>
struct RandomPool {
    T* actions;
    T* costs;
};
// the batched sampler on the pool's slices, every store mirrored into the problem's own actions; the workgroups of
// blockIdx.x == 0 also copy their problem's observation og.src[p] [og.width] to og.dst + p * og.width (ObsGather: icem_fused.h)
void launch_random_sample_gather_batch(const icem_handle* h, const void* args_dev, const BatchBases& bases, const ObsGather& og,
                                       const RandomPool<float>& pool, int n_problems, hipStream_t st);
// the batched selection on the pool's slices, every cost it reads stored into the problem's own costs
void launch_random_select_pool_batch(const icem_handle* h, const void* args_dev, const RandomPool<float>& pool, int n_problems, hipStream_t st);
// ... whose costs are still the members' (icem_plan_step_random_learned_models): member e's cost of problem p's row i is
// member_costs[e * stride + p * N + i]; the selection reduces them (mean: ((c_0 + c_1) + ..) * inv, max: a NaN member wins),
// stores the reduced cost to the pool's slice and to the problem's own costs, and selects on it.  With one problem the pool may
// BE the problem's own actions / costs.
struct RandomMembers {
    const float* member_costs;   // [members, stride]
    int members, reduce;         // reduce: ICEM_RSSM_REDUCE_MEAN / _MAX
    int stride;                  // n * N
    float inv;                   // (float)(1.0 / members)
};
void launch_random_select_members_batch(const icem_handle* h, const void* args_dev, const RandomPool<float>& pool, const RandomMembers& mb,
                                        int n_problems, hipStream_t st);

}  // namespace icem
