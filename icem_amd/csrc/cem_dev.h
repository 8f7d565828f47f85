// cem_dev.h -- device text of the CEM baseline (MpcCemStd, icem/controllers/mpc.py:142-327) that its stand-alone operators
// (generic_kernels.hip: sample_truncnorm_kernel, cem_bounds_kernel) and the kernels of icem_plan_step_cem (k_cem.hip) share:
// the truncated-normal quantile of one uniform, _update_bounds of one element, and the step's tail -- the bounds behind a
// refit and, on the last iteration, get_action's epilogue.  One text, one arithmetic: the step's bits are the operators'.
// Internal; not part of the public ABI.
#pragma once
#include "cost_terms_dev.h"   // fmad

namespace icem {

__device__ __forceinline__ double std_normal_cdf(double x) { return normcdf(x); }
__device__ __forceinline__ float std_normal_cdf(float x) { return normcdff(x); }
__device__ __forceinline__ double std_normal_icdf(double p) { return normcdfinv(p); }
__device__ __forceinline__ float std_normal_icdf(float p) { return normcdfinvf(p); }

// word x of a row's stream as a uniform in (0, 1): (x + 0.5) * 2^-32
template <typename T>
__device__ __forceinline__ T word_uniform(uint32_t x) {
    return ((T)x + (T)0.5) * (T)2.3283064365386963e-10;
}

// ppf(uu; lo_z, hi_z) of the truncated standard normal (scipy.stats.truncnorm.rvs, mpc.py:188-198) from pa = Phi(lo_z),
// qb = Phi(-hi_z) = 1 - Phi(hi_z) and pd = Phi(hi_z) - Phi(lo_z), two-sided: the probability below the quantile is
// p = pa + uu pd and the one above it q = qb + (1 - uu) pd; the smaller of the two, which the number format resolves to
// RELATIVE precision, is the one inverted (p + q = 1: p <= q is the lower half).  Through p alone the upper tail is resolved
// to 2^-24 of 1 only -- in f32 a uniform within 2^-24 of 1 at lo_z = 0 came back as hi_z, 5 sigma and more off.
// The quantile lies in [lo_z, hi_z] by definition, and ppf(1) = hi_z; an interval deep in one tail (pd == 0) or hi_z beyond
// the format's Phi(-hi_z) would otherwise come back as +-inf.  (mean inside the action box: lo_z <= 0 <= hi_z.)
template <typename T>
__device__ __forceinline__ T truncnorm_quantile(T uu, T pa, T qb, T pd, T lo_z, T hi_z) {
    const T p = fmad(uu, pd, pa), q = fmad((T)1 - uu, pd, qb);
    T z = std_normal_icdf(p <= q ? p : q);   // one inverse for both halves
    z = p <= q ? z : -z;
    z = z < lo_z ? lo_z : z;
    z = z > hi_z ? hi_z : z;
    return uu < (T)1 ? z : hi_z;
}

// MpcCemStd._update_bounds (mpc.py:290-301) of element e = (t, j): in place on std (like_levine) and into lower / upper
template <typename T>
__device__ __forceinline__ void cem_bounds_element(int e, int j, int like_levine, const T* mean, T* std, const T* low,
                                                   const T* high, T* lower, T* upper) {
    if (like_levine) {
        const T lb = (mean[e] - low[j]) / (T)2, ub = (high[j] - mean[e]) / (T)2;
        T s = lb < ub ? lb : ub;
        s = s < std[e] ? s : std[e];
        std[e] = s > (T)1e-8 ? s : (T)1e-8;
        lower[e] = (T)-2;
        upper[e] = (T)2;
    } else {
        lower[e] = (low[j] - mean[e]) / (std[e] + (T)1e-8);
        upper[e] = (high[j] - mean[e]) / (std[e] + (T)1e-8);
    }
}

// What follows the refit in an iteration of icem_plan_step_cem, for the ONE workgroup (NT threads) that refitted: element e of
// mean / std / elites was written by thread e % NT, which is the thread that reads it here.
template <typename T>
struct CemTailArgs {
    int h, d;
    int like_levine, shift_means, execute_best_elite;
    int last;                 // the step's last iteration: the epilogue below
    T init_std;
    T* mean;                  // [h, d] as refitted
    T* std;
    const T* low;             // [d]
    const T* high;
    T* lower;                 // [h, d]
    T* upper;
    const T* elites;          // [K, h, d] of this iteration (row 0: the best)
    const T* elite_costs;     // [K]
    T* executed;              // [d]
    T* best_cost;             // [1]
    T* result;                // [d + 1] executed | best_cost once more (a batch's row of `results`), or nullptr
};

// _update_bounds on the refitted rows (mpc.py:228); behind the last iteration executed / best_cost (mpc.py:230-233), the
// mean's shift (mpc.py:236-243 with the default compute_new_mean, mpc.py:265-269) or its reset to 0, the std reset
// (get_init_std(True), mpc.py:180-185: reset_kernel's expression) and _update_bounds again (mpc.py:244-245).
// stage: [h * d] of LDS (the mean's rows cross threads in the shift).
template <typename T, int NT>
__device__ __forceinline__ void cem_tail(const CemTailArgs<T>& c, T* stage) {
    const int tid = threadIdx.x;
    const int hd = c.h * c.d;
    for (int e = tid; e < hd; e += NT) cem_bounds_element<T>(e, e % c.d, c.like_levine, c.mean, c.std, c.low, c.high, c.lower, c.upper);
    if (!c.last) return;
    if (tid < c.d) {
        const T x = c.execute_best_elite ? c.elites[tid] : c.mean[tid];
        c.executed[tid] = x;
        if (c.result) c.result[tid] = x;
    }
    if (tid == 0) {
        const T bc = c.elite_costs[0];
        c.best_cost[0] = bc;
        if (c.result) c.result[c.d] = bc;
    }
    for (int e = tid; e < hd; e += NT) stage[e] = c.mean[e];
    __syncthreads();
    for (int e = tid; e < hd; e += NT) {
        const int j = e % c.d;
        T m = (T)0;
        if (c.shift_means) m = (e + c.d < hd) ? stage[e + c.d] : (c.like_levine ? (T)0 : stage[e]);
        c.mean[e] = m;
        c.std[e] = (c.high[j] - c.low[j]) / (T)2 * c.init_std;
        cem_bounds_element<T>(e, j, c.like_levine, c.mean, c.std, c.low, c.high, c.lower, c.upper);
    }
}

}  // namespace icem
