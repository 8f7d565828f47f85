// update_small_body.h -- the body of update_small_kernel / update_small_batch_kernel (k_merge.hip) and of the f32 update
// kernel of icem_plan_step_cem (k_cem.hip): one device function, the same device code.  Internal; not part of the public ABI.
#pragma once
#include "fused_dev.h"
#include "refit.h"

namespace icem {

// icem_update_distribution: the reference's update_distributions in ONE launch for small f32 pools -- the sorted top-K
// over the pool's costs and the kept elites' (icem.py:143-145: appended behind the pool, index n + e), the gather of the
// K elite rows from pool / kept elites, the refit (refit.h: the arithmetic of gather_refit_kernel).  Phase 1 + 2 are
// topk_small_kernel's; the selection lands in LDS (wg_merge_emit's list 0 of 1, through a generic pointer).
// (the body of update_small_kernel and of update_small_batch_kernel: one device function.  FINISH: the step's epilogue behind
//  the refit -- the new mean goes through LDS and leaves shifted, std is reset (shift_kernel's arithmetic, icem.py:167-175),
//  executed = elites[0, 0, :], best_cost = elite_costs[0], and both once more as the problem's row of `results`.
//  Src: where candidate i < a.n gets its cost from -- PoolCosts, the plain load of a.costs[i], unless the caller says otherwise.)
struct PoolCosts {
    __device__ __forceinline__ float operator()(const UpdateSmallArgs& a, int i) const { return a.costs[i]; }
};

// ... or from the costs of an ensemble's members (update_small_members_batch_kernel; UpdateMembersArgs, icem_fused.h -- and the two
// baselines' cem_update_members_batch_kernel, k_cem_members.hip, and random_select_members_batch_kernel, random_dev.h), reduced here
// as rssm_ensemble_reduce_kernel reduces them -- the same float32 operations in the same order, no atomics, no division, the
// mean's one multiply a rounding of its own -- and written to costs[i] as well.  `members` is uniform across the workgroup: a
// row's loads are all requested before the first is consumed (one round trip to memory, not one per member), in a group of
// up to 8 members or of up to 32.
struct MemberCosts {
    const float* mc;   // member 0's cost of this problem's row 0
    float* out;
    unsigned stride;   // (members * stride <= 32 * 16 384 floats: 32-bit offsets from the one base)
    int members, reduce;
    float inv;
    template <int T>
    __device__ __forceinline__ float reduced(unsigned i) const {
        // (straight-line: a slot behind the last member loads the last member's cost again and is not consumed)
        // (typed as global memory: a pointer read from the argument block is generic, and its loads were flat_load)
        typedef const float __attribute__((address_space(1))) * GlobalF;
        const GlobalF g = (GlobalF)mc;
        float c[T];
#pragma unroll
        for (int e = 0; e < T; ++e) c[e] = g[(unsigned)(e < members ? e : members - 1) * stride + i];
        float acc = c[0];
        if (reduce == 0) {
#pragma unroll
            for (int e = 1; e < T; ++e) acc = e < members ? acc + c[e] : acc;
            return __fmul_rn(acc, inv);   // (__fmul_rn: never contracted into the key's `+ 0.0f`)
        }
#pragma unroll
        for (int e = 1; e < T; ++e) {
            const bool worse = (c[e] > acc) | (c[e] != c[e]);
            acc = ((e < members) & worse) ? c[e] : acc;
        }
        return acc;
    }
    // (Args: the argument block of the body that asks -- UpdateSmallArgs here, RandomSelectArgs<float> in random_dev.h; unused)
    template <class Args>
    __device__ __forceinline__ float operator()(const Args&, int i) const {
        const float r = members <= 8 ? reduced<8>((unsigned)i) : reduced<32>((unsigned)i);
        out[i] = r;
        return r;
    }
};

template <bool FINISH, class Src = PoolCosts>
__device__ __forceinline__ void update_small_body(const UpdateSmallArgs& a, const UpdateFinishArgs* f, const Src src = Src()) {
    __shared__ unsigned long long wg_keys[2][16][32];
    __shared__ unsigned long long sel[32];
    __shared__ float shifted[FINISH ? UPDATE_FINISH_MAX_HD : 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n_all = a.n + a.n_keep;
    unsigned long long run = KEY_SENTINEL;
    bool first = true;
    for (int base = wave * 64; base < n_all; base += 1024) {
        const int i = base + lane;
        unsigned long long key = KEY_SENTINEL;
        if (i < n_all) key = make_key(i < a.n ? src(a, i) : a.keep_costs[i - a.n], i);
        key = wave_sort64(key, lane);
        if (!first) {
            const unsigned long long prev = __shfl(run, lane - 32, 64);
            key = (lane >= 32 && lane < 32 + a.K) ? prev : (lane < a.K ? key : KEY_SENTINEL);
            key = wave_sort64(key, lane);
        }
        run = key;
        first = false;
    }
    FastRolloutArgs fr{};
    fr.part_k = sel;
    wg_merge_emit<16>(wg_keys, run, a.K, lane, wave, fr, 0, 1);
    __syncthreads();
    if (tid < a.K) {
        a.elite_costs_out[tid] = key_cost(sel[tid]);
        a.idx_out[tid] = key_idx(sel[tid]);
    }
    // a padded selection (fewer than K candidates: (+inf, INT_MAX)) repeats its best row, as icem_gather_refit does
    auto row = [&](int r) -> const float* {
        int i = key_idx(sel[r]);
        if (i < 0 || i == INT_MAX) i = key_idx(sel[0]);
        return i < a.n ? a.pool + (size_t)i * a.hd : a.keep_actions + (size_t)(i - a.n) * a.hd;
    };
    for (int e = tid; e < a.hd; e += 1024) {
        for (int r = 0; r < a.K; ++r) a.elites_out[(size_t)r * a.hd + e] = row(r)[e];
        float nm, ns;
        refit_element<float>(a.K, a.alpha, a.mean[e], a.std[e], [&](int r) { return row(r)[e]; }, nm, ns);
        if (FINISH) {
            shifted[e] = nm;
        } else {
            a.mean[e] = nm;
            a.std[e] = ns;
        }
    }
    if (FINISH) {
        __syncthreads();
        const int d = f->d;
        for (int e = tid; e < a.hd; e += 1024) {
            const int j = e % d;
            a.mean[e] = (e + d < a.hd) ? shifted[e + d] : shifted[e];
            a.std[e] = (f->high[j] - f->low[j]) / 2.f * f->init_std;
        }
        if (tid < d) {
            const float x = row(0)[tid];
            f->executed[tid] = x;
            if (f->result) f->result[tid] = x;
        }
        if (tid == 0) {
            const float c = key_cost(sel[0]);
            f->best_cost[0] = c;
            if (f->result) f->result[d] = c;
        }
    }
}

}  // namespace icem
