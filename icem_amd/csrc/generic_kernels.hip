// generic_kernels.hip -- the generic gfx950 kernels of the iCEM inner planning loop (f32 / f64, any h <= 64, d <= 64,
// o <= 32, external or device white noise) and their launchers (gk_*, host_common.h).  They serve the strict-parity
// f64 mode, shapes outside the compiled matrix-pipe list, and the stand-alone operators of the ABI.
//
// Data layout in HBM (all C-contiguous, T = float or double):
//   actions [n, h, d]   the reference's `action_sequences` (icem/controllers/icem.py:73-79)
//   costs   [n]
//   mean/std [h, d], low/high [d]
//   W [h, HMAX]         colored-noise synthesis table, row t holds the h coefficients that turn the
//                       h white draws of one (trajectory, action-dim) row into sample t (zero padded)
//   records [world*K, 2+h*d]   {cost, gidx, actions[h*d]} -- what the ranks exchange
//
// Kernels (one section each): sample_clip (K1), rollout_cost (K2), block top-k (K3),
// local_pack / merge_refit (K3+K4 of the fused step), small epilogue kernels.
#include "host_common.h"
#include "cost_terms_dev.h"
#include "exchange_dev.h"
#include "cem_dev.h"       // the CEM baseline's quantile, bounds and step tail (k_cem.hip)
#include "generic_dev.h"   // the bodies a batched float64 step shares (k_generic_batch.hip)
#include "philox.h"
#include "refit.h"

namespace icem {


// ---------------------------------------------------------------------------------------------
// K1  colored-noise sampling + affine + clip          (icem.py:61-82 + colorednoise)
// ---------------------------------------------------------------------------------------------
// One thread per (trajectory, action-dim) row: it owns the h white draws of that row, applies the
// [h x h] synthesis (inverse real DFT with f^(-beta/2)/sigma folded in) with the table row as a
// wave-uniform (scalar) operand, and parks the h samples in an LDS tile laid out like the output,
// so the workgroup's slab of `actions` (tpw consecutive trajectories = one contiguous span) goes
// out as coalesced stores.  The reference's transpose([0,2,1]) is absorbed by the tile indexing.

// (SampleArgs and the other argument blocks: generic_args.h)
struct ShiftSampleArgs {
    SampleArgs<float> s;        // n = the shifted rows, t_begin = h - 1, out = their first row, offset relative to the step's base
    const float* elites_src;    // [>= n, h, d]
};

template <typename T, int HMAX, int ROUNDS>
__device__ __forceinline__ void white_row(const SampleArgs<T>& a, int row_local, long long gi, int j, T (&g)[HMAX]) {
    if (a.zr != nullptr && a.white) {
#pragma unroll
        for (int m = 0; m < HMAX; ++m) g[m] = m < a.h ? a.zr[((size_t)row_local * a.h + m) * a.d + j] : (T)0;
    } else if (a.zr != nullptr) {
        const size_t base = ((size_t)row_local * a.d + j) * a.F;
#pragma unroll
        for (int m = 0; m < HMAX; ++m) {
            T v = (T)0;
            if (m < a.F)
                v = a.zr[base + m];
            else if (m < a.h)
                v = a.zi[base + (m - a.F + 1)];
            g[m] = v;
        }
    } else {
        Xoshiro128pp rng = row_stream<ROUNDS>((uint32_t)gi, (uint32_t)j, a.off_lo, a.off_hi, a.seed_lo, a.seed_hi);
#pragma unroll
        for (int m = 0; m < HMAX; m += 2) {
            if (m < a.h) {
                const uint32_t xa = rng.next();
                const uint32_t xb = rng.next();
                box_muller(xa, xb, g[m], g[m + 1]);
            } else {
                g[m] = g[m + 1] = (T)0;
            }
        }
    }
}

// (the body of sample_clip_kernel and of the thread form of shift_sample_batch_kernel: one device function, the same device code)
template <typename T, int HMAX, int ROUNDS>
__device__ __forceinline__ void sample_clip_body(const SampleArgs<T>& a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    T* tile = reinterpret_cast<T*>(smem_raw);
    const int tid = threadIdx.x;
    const int hd = a.h * a.d;
    const int n_base = blockIdx.x * a.tpw;
    const int n_here = min(a.tpw, a.n - n_base);
    const int rows = n_here * a.d;
    if (tid < rows) {
        const int nl = tid / a.d;
        const int j = tid - nl * a.d;
        T g[HMAX];
        white_row<T, HMAX, ROUNDS>(a, n_base + nl, a.first_index + n_base + nl, j, g);
        const T lo = a.low[j], hi = a.high[j];
        for (int t = a.t_begin; t < a.h; ++t) {
            const T* __restrict__ w = a.W + (size_t)t * HMAX;
            T acc = (T)0;
#pragma unroll
            for (int m = 0; m < HMAX; ++m) acc = fmad(g[m], w[m], acc);
            T v = fmad(acc, a.std[t * a.d + j], a.mean[t * a.d + j]);
            v = v < lo ? lo : v;
            v = v > hi ? hi : v;
            tile[nl * hd + t * a.d + j] = v;
        }
    }
    __syncthreads();
    if (a.row0_mean && a.first_index + n_base == 0) {  // icem.py:87-88
        for (int e = tid; e < hd; e += WG) tile[e] = a.mean[e];
        __syncthreads();
    }
    const size_t base = (size_t)n_base * hd;
    const int total = n_here * hd;
    const int e_begin = a.t_begin * a.d;
    for (int e = tid; e < total; e += WG) {
        if (e_begin == 0 || (e % hd) >= e_begin) a.out[base + e] = tile[e];
    }
}

template <typename T, int HMAX, int ROUNDS>
__global__ __launch_bounds__(WG) void sample_clip_kernel(SampleArgs<T> a) {
    sample_clip_body<T, HMAX, ROUNDS>(a);
}

template <typename T, int HMAX, int ROUNDS>
__global__ __launch_bounds__(WG) void sample_clip_quad_kernel(SampleArgs<T> a) {
    sample_clip_quad_body<T, HMAX, ROUNDS>(a);
}

// The shifted elites of B problems in one launch (icem_plan_step_learned*, learned_step.hip): blockIdx.y = the problem, its
// argument block in device memory, the stream offset stored relative to the step's base of that problem (BatchBases).  Rows
// [0, s.n) of s.out <- elites_src[e, 1:, :] (icem.py:97-100) and, behind them, the freshly drawn last action: the sampling
// call icem_sample_clip(t_begin = h - 1) makes for these rows -- the same body, so the same bits -- which writes the last
// time step only.  A problem without shifted elites (s.n == 0: its first MPC step) and surplus workgroups exit.
template <int HMAX, int ROUNDS, bool QUAD>
__global__ __launch_bounds__(WG) void shift_sample_batch_kernel(const ShiftSampleArgs* __restrict__ args, BatchBases bases) {
    ShiftSampleArgs g = args[blockIdx.y];
    SampleArgs<float>& a = g.s;
    const int n_base = blockIdx.x * a.tpw;
    if (n_base >= a.n) return;
    const unsigned long long off = (((unsigned long long)a.off_hi << 32) | a.off_lo) + bases.v[blockIdx.y];
    a.off_lo = (uint32_t)off;
    a.off_hi = (uint32_t)(off >> 32);
    const int hd = a.h * a.d;
    const int n_here = min(a.tpw, a.n - n_base);
    const int keep = hd - a.d;
    for (int x = threadIdx.x; x < n_here * keep; x += WG) {
        const int e = x / keep, r = x - e * keep;
        a.out[(size_t)(n_base + e) * hd + r] = g.elites_src[(size_t)(n_base + e) * hd + a.d + r];
    }
    if (QUAD) sample_clip_quad_body<float, HMAX, ROUNDS>(a);
    else sample_clip_body<float, HMAX, ROUNDS>(a);
}

// ---------------------------------------------------------------------------------------------
// MpcCemStd (the CEM baseline, icem/controllers/mpc.py:142-327): truncated-normal sampling and its bounds
// ---------------------------------------------------------------------------------------------
// (the quantile and _update_bounds of one element: cem_dev.h, shared with the kernels of icem_plan_step_cem)
// actions[i, t, j] = mean[t, j] + std[t, j] * ppf(u; lower[t, j], upper[t, j]) with the truncated standard normal's
// inverse CDF ppf(u; a, b) = Phi^-1(Phi(a) + u (Phi(b) - Phi(a)))  (scipy.stats.truncnorm.rvs, mpc.py:188-198), its upper
// half taken through the complement (cem_dev.h::truncnorm_quantile).
// u: the caller's uniforms [n, h, d] (parity: scipy draws exactly that array), or, if null, word t of row (i, j)'s
// Philox / xoshiro stream mapped to (x + 0.5) * 2^-32.  One thread per (trajectory, dim) row.
template <typename T, int ROUNDS>
__global__ __launch_bounds__(WG) void sample_truncnorm_kernel(int n, int h, int d, long long first_index, const T* mean,
                                                             const T* std, const T* lower, const T* upper, const T* u,
                                                             uint32_t seed_lo, uint32_t seed_hi, uint32_t off_lo,
                                                             uint32_t off_hi, T* out) {
    const int row = blockIdx.x * WG + threadIdx.x;
    if (row >= n * d) return;
    const int i = row / d, j = row - i * d;
    Xoshiro128pp rng = row_stream<ROUNDS>((uint32_t)(first_index + i), (uint32_t)j, off_lo, off_hi, seed_lo, seed_hi);
    for (int t = 0; t < h; ++t) {
        const size_t e = ((size_t)i * h + t) * d + j;
        const uint32_t x = rng.next();
        const T uu = u ? u[e] : word_uniform<T>(x);
        const T pa = std_normal_cdf(lower[t * d + j]), pb = std_normal_cdf(upper[t * d + j]), qb = std_normal_cdf(-upper[t * d + j]);
        const T z = truncnorm_quantile<T>(uu, pa, qb, pb - pa, lower[t * d + j], upper[t * d + j]);
        out[e] = fmad(z, std[t * d + j], mean[t * d + j]);
    }
}

// MpcRandom.sample_action_sequences (mpc.py:96-109): uniform actions held for a number of consecutive calls of
// sample() -- a call counter that runs over (trajectory, step) pairs and on across MPC steps.  Call c uses block
// 0 (the action drawn at construction) while c < freq, then block 1 + (c - freq) / (freq + 1).  u: the caller's
// uniforms [*, d] for blocks first_block.. (parity), or null: word 0 of block (b, j)'s Philox / xoshiro stream.
template <typename T, int ROUNDS>
__global__ __launch_bounds__(WG) void sample_piecewise_kernel(long long total, int d, long long call_offset, int freq,
                                                             long long first_block, const T* low, const T* high, const T* u,
                                                             uint32_t seed_lo, uint32_t seed_hi, T* out) {
    const long long e = (long long)blockIdx.x * WG + threadIdx.x;
    if (e >= total) return;
    const long long call = call_offset + e / d;
    const int j = (int)(e % d);
    const long long b = call < freq ? 0 : 1 + (call - freq) / (freq + 1);
    T uu;
    if (u) {
        uu = u[(b - first_block) * d + j];
    } else {
        Xoshiro128pp rng = row_stream<ROUNDS>((uint32_t)b, (uint32_t)j, (uint32_t)((unsigned long long)b >> 32), 0x52414E44u /* "RAND" */,
                                              seed_lo, seed_hi);
        uu = ((T)rng.next() + (T)0.5) * (T)2.3283064365386963e-10;
    }
    out[e] = fmad(high[j] - low[j], uu, low[j]);
}

// MpcCemStd._update_bounds (mpc.py:290-301), in place on std (like_levine) and into lower / upper [h, d]
template <typename T>
__global__ __launch_bounds__(WG) void cem_bounds_kernel(int hd, int d, int like_levine, const T* mean, T* std, const T* low,
                                                       const T* high, T* lower, T* upper) {
    const int e = blockIdx.x * WG + threadIdx.x;
    if (e >= hd) return;
    cem_bounds_element<T>(e, e % d, like_levine, mean, std, low, high, lower, upper);
}

// Raw Philox white noise in the reference's [n, d, F] x 2 layout (RNG known-answer tests).
template <typename T, int HMAX, int ROUNDS>
__global__ __launch_bounds__(WG) void philox_normals_kernel(SampleArgs<T> a, T* zr_out, T* zi_out) {
    const int row = blockIdx.x * WG + threadIdx.x;
    if (row >= a.n * a.d) return;
    const int nl = row / a.d;
    const int j = row - nl * a.d;
    T g[HMAX];
    white_row<T, HMAX, ROUNDS>(a, nl, a.first_index + nl, j, g);
    const size_t base = (size_t)row * a.F;
#pragma unroll
    for (int m = 0; m < HMAX; ++m) {
        if (m < a.F) {
            zr_out[base + m] = g[m];
            zi_out[base + m] = (T)0;
        }
    }
#pragma unroll
    for (int m = 0; m < HMAX; ++m) {
        if (m >= a.F && m < a.h) zi_out[base + (m - a.F + 1)] = g[m];
    }
}

// ---------------------------------------------------------------------------------------------
// K2  batched open-loop rollout + per-trajectory cost   (abstract_models.py:17-53,
//     abstract_controller.py:74-91, environments/mujoco.py:67-99 / 259-277)
// ---------------------------------------------------------------------------------------------
// One thread per trajectory; the observation lives in registers (O compile-time, zero padded),
// the model matrices are wave-uniform operands.  Cost is scored on the PRE-action observation.

template <typename T, int O, int KIND>
__global__ __launch_bounds__(WG) void rollout_cost_kernel(RolloutArgs<T> a) {
    rollout_cost_body<T, O, KIND>(a);
}

// ... and with a trajectory spread over a row of lanes (rollout_cost_rows_body, generic_dev.h)
template <typename T, int O, int KIND>
__global__ __launch_bounds__(WG) void rollout_cost_rows_kernel(RolloutArgs<T> a) {
    rollout_cost_rows_body<T, O, KIND>(a);
}

template <typename T>
__global__ __launch_bounds__(WG) void cost_reduce_kernel(int n, int h, int mode, const T* step, T* costs) {
    const int i = blockIdx.x * WG + threadIdx.x;
    if (i >= n) return;
    const T* row = step + (size_t)i * h;
    T acc = row[0];
    for (int t = 1; t < h; ++t) {
        const T c = row[t];
        if (mode == ICEM_COST_SUM)
            acc += c;
        else if (mode == ICEM_COST_BEST)
            acc = (c < acc || c != c) ? c : acc;  // np.amin: a NaN step cost makes the trajectory's cost NaN
        else
            acc = c;
    }
    costs[i] = acc;
}

// trajectory_cost_fn (abstract_controller.py:74-91) over rollouts an external model left in HBM: one wavefront
// per trajectory.  Phase A, only when a term needs every entry of the observation (finite check / state box):
// the rows are swept coalesced (lanes across the observation), one ballot per step leaves a bit mask of the bad
// steps.  Phase B: lane t scores step t (its actions and the handful of observation entries the terms read).
// The step costs are then reduced in t order.
template <typename T>
struct TrajCostArgs {
    int n, h, d, o;
    const T* obs;
    const T* nxt;     // nullable
    long long ts, ss;
    const T* actions;
    T* costs;
    CostArgs<T> cs;
    int cost_mode, sweep;
};

template <typename T>
__device__ __forceinline__ bool bad_entry(const TrajCostArgs<T>& a, T v, int k) {
    bool bad = !finite_val(v);
    if (a.cs.box_from >= 0 && k >= a.cs.box_from) bad |= !(a.cs.box_lo < v && v < a.cs.box_hi);
    return bad;
}

template <typename T>
__global__ __launch_bounds__(WG) void trajectory_cost_kernel(TrajCostArgs<T> a) {
    const int lane = threadIdx.x & 63;
    const int n = blockIdx.x * (WG / 64) + (threadIdx.x >> 6);
    if (n >= a.n) return;
    const T* __restrict__ traj = a.obs + (long long)n * a.ts;
    unsigned long long bad_steps = 0;   // h <= 64 (icem_create)
    if (a.sweep == 1) {
        // four rows x two 64-entry columns = eight unconditional loads in flight per lane; indices past the end
        // of a row / of the trajectory are clamped (a repeated entry changes nothing)
        for (int t = 0; t < a.h; t += 4) {
            const T* __restrict__ r0 = traj + (long long)min(t + 0, a.h - 1) * a.ss;
            const T* __restrict__ r1 = traj + (long long)min(t + 1, a.h - 1) * a.ss;
            const T* __restrict__ r2 = traj + (long long)min(t + 2, a.h - 1) * a.ss;
            const T* __restrict__ r3 = traj + (long long)min(t + 3, a.h - 1) * a.ss;
            bool b0 = false, b1 = false, b2 = false, b3 = false;
            for (int base = 0; base < a.o; base += 128) {
                const int k0 = min(base + lane, a.o - 1), k1 = min(base + 64 + lane, a.o - 1);
                const T v00 = r0[k0], v01 = r0[k1], v10 = r1[k0], v11 = r1[k1];
                const T v20 = r2[k0], v21 = r2[k1], v30 = r3[k0], v31 = r3[k1];
                b0 |= bad_entry(a, v00, k0);
                b0 |= bad_entry(a, v01, k1);
                b1 |= bad_entry(a, v10, k0);
                b1 |= bad_entry(a, v11, k1);
                b2 |= bad_entry(a, v20, k0);
                b2 |= bad_entry(a, v21, k1);
                b3 |= bad_entry(a, v30, k0);
                b3 |= bad_entry(a, v31, k1);
            }
            bad_steps |= (unsigned long long)(__ballot(b0) != 0) << (t & 63);
            bad_steps |= (unsigned long long)(__ballot(b1) != 0) << ((t + 1) & 63);   // rows past h repeat row h-1:
            bad_steps |= (unsigned long long)(__ballot(b2) != 0) << ((t + 2) & 63);   // their bits are never read
            bad_steps |= (unsigned long long)(__ballot(b3) != 0) << ((t + 3) & 63);
        }
    }
    T c = (T)0;
    if (lane < a.h) {
        const int t = lane;
        const T* __restrict__ row = traj + (long long)t * a.ss;
        const T* __restrict__ act = a.actions + ((long long)n * a.h + t) * a.d;
        T ctrl = (T)0;
        for (int j = 0; j < a.d; ++j) ctrl = fmad(act[j], act[j], ctrl);
        if (a.cs.flip_idx >= 0) {
            const T ang = row[a.cs.flip_idx];
            c += (ang > a.cs.flip_th) ? a.cs.flip_pen : (T)0;
            c += (ang < -a.cs.flip_th) ? a.cs.flip_pen : (T)0;
        }
        c += a.cs.ctrl_w * ctrl;
        if (a.cs.lin_w != (T)0) c += a.cs.lin_w * row[a.cs.lin_idx];
        if (a.cs.ext) {
            const T* __restrict__ nrow = a.nxt ? a.nxt + (long long)n * a.ts + (long long)t * a.ss : row;
            bool bad = (bad_steps >> t) & 1ull;
            if (a.sweep == 2)   // narrow observations: each lane checks its own row
                for (int k = 0; k < a.o; ++k) bad |= bad_entry(a, row[k], k);
            c += cost_terms<T>(a.cs, bad, [&](int idx) { return row[idx]; },
                               [&](int idx) { return nrow[idx]; });
        }
    }
    T acc = __shfl(c, 0);
    for (int t = 1; t < a.h; ++t) {
        const T ct = __shfl(c, t);
        if (a.cost_mode == ICEM_COST_SUM)
            acc += ct;
        else if (a.cost_mode == ICEM_COST_BEST)
            acc = (ct < acc || ct != ct) ? ct : acc;  // np.amin: NaN propagates
        else
            acc = ct;
    }
    if (lane == 0) a.costs[n] = acc;
}

// ---------------------------------------------------------------------------------------------
// K3  sorted top-k                                       (icem.py:199 argsort()[:K], :149 argmin)
// ---------------------------------------------------------------------------------------------
// Threshold selection: round r takes the smallest (cost, idx) key strictly greater than round
// r-1's winner, so nothing is mutated and the K winners come out already sorted.  Per round: a
// strided scan of the keys, a 64-lane butterfly, and one LDS hop across the 4 waves.

// Stage 1: each workgroup reduces TOPK_CHUNK costs to its K best -> part_c/part_i[block*K + r].
template <typename T>
__global__ __launch_bounds__(WG) void topk_partial_kernel(int n, int K, const T* costs, T* part_c, int* part_i) {
    __shared__ T keys[TOPK_CHUNK];
    __shared__ T red_c[WG / 64];
    __shared__ int red_i[WG / 64];
    __shared__ int red_e[WG / 64];
    const int base = blockIdx.x * TOPK_CHUNK;
    const int cnt = min(TOPK_CHUNK, n - base);
    for (int e = threadIdx.x; e < cnt; e += WG) keys[e] = nan_to_inf(costs[base + e]);
    __syncthreads();
    block_select_sorted<T>(
        cnt, K, [&](int e) { return keys[e]; }, [&](int e) { return base + e; }, part_c + (size_t)blockIdx.x * K,
        part_i + (size_t)blockIdx.x * K, nullptr, red_c, red_i, red_e);
}

// Stage 2 (stand-alone API): one workgroup merges the partial lists.
template <typename T>
__global__ __launch_bounds__(WG) void topk_final_kernel(int cnt, int K, const T* part_c, const int* part_i, T* out_c,
                                                        int* out_i) {
    __shared__ T red_c[WG / 64];
    __shared__ int red_i[WG / 64];
    __shared__ int red_e[WG / 64];
    block_select_sorted<T>(
        cnt, K, [&](int e) { return part_c[e]; }, [&](int e) { return part_i[e]; }, out_c, out_i, nullptr, red_c,
        red_i, red_e);
}

// ---------------------------------------------------------------------------------------------
// K4  gather + refit                                     (icem.py:201-211)
// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(WG) void gather_refit_kernel(int hd, int K, T alpha, const T* actions, const int* idx,
                                                          T* mean, T* std, T* elites_out) {
    // an index list padded by icem_topk_sorted (k > n: entries INT_MAX) repeats its best row instead of reading out of bounds
    auto row = [&](int r) -> size_t {
        const int i = idx[r];
        return (size_t)((i < 0 || i == INT_MAX) ? idx[0] : i);
    };
    for (int e = blockIdx.x * WG + threadIdx.x; e < hd; e += gridDim.x * WG) {
        if (elites_out != nullptr)
            for (int r = 0; r < K; ++r) elites_out[(size_t)r * hd + e] = actions[row(r) * hd + e];
        T nm, ns;
        refit_element<T>(K, alpha, mean[e], std[e], [&](int r) { return actions[row(r) * hd + e]; }, nm, ns);
        mean[e] = nm;
        std[e] = ns;
    }
}

// get_action epilogue (icem.py:167-175) and beginning_of_rollout (icem.py:48-59).
template <typename T>
__global__ __launch_bounds__(WG) void shift_kernel(int h, int d, T init_std, T* mean, T* std, const T* low,
                                                   const T* high) {
    // single workgroup: read every element before any is overwritten
    const int hd = h * d;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    T* tmp = reinterpret_cast<T*>(smem_raw);
    for (int e = threadIdx.x; e < hd; e += WG) tmp[e] = mean[e];
    __syncthreads();
    for (int e = threadIdx.x; e < hd; e += WG) {
        const int j = e % d;
        mean[e] = (e + d < hd) ? tmp[e + d] : tmp[e];
        std[e] = (high[j] - low[j]) / (T)2 * init_std;
    }
}

template <typename T>
__global__ __launch_bounds__(WG) void reset_kernel(int h, int d, T init_std, T* mean, T* std, const T* low,
                                                   const T* high) {
    const int hd = h * d;
    for (int e = blockIdx.x * WG + threadIdx.x; e < hd; e += gridDim.x * WG) {
        const int j = e % d;
        mean[e] = (high[j] + low[j]) / (T)2;
        std[e] = (high[j] - low[j]) / (T)2 * init_std;
    }
}

// ---------------------------------------------------------------------------------------------
// fused-step glue: shifted elites, local candidate packing, global merge + refit
// ---------------------------------------------------------------------------------------------

template <typename T>
__global__ __launch_bounds__(WG) void shift_elites_kernel(int n_reuse, int h, int d, const T* elites, T* dst) {
    shift_elites_body<T>(n_reuse, h, d, elites, dst);
}

template <typename T>
__device__ __forceinline__ int rec_gidx(const T* rec) {
    return reinterpret_cast<const int*>(rec + 1)[0];
}
template <typename T>
__device__ __forceinline__ void rec_set(T* rec, T cost, int gidx) {
    rec[0] = cost;
    rec[1] = (T)0;
    reinterpret_cast<int*>(rec + 1)[0] = gidx;
}

// One workgroup: pick this rank's K best among the block partials (sorted), translate local pool
// indices to global trajectory indices, and pack {cost, gidx, actions row} records.
//   local idx < n_loc           -> gidx = shard_lo + idx
//   local idx >= n_loc (shifted elites simulated at iteration 0) -> gidx = n_global + (idx - n_loc)
template <typename T>
__global__ __launch_bounds__(WG) void local_pack_kernel(int cnt, int K, int hd, int n_loc, int shard_lo, int n_global,
                                                        const T* part_c, const int* part_i, const T* actions,
                                                        T* records) {
    __shared__ T red_c[WG / 64];
    __shared__ int red_i[WG / 64];
    __shared__ int red_e[WG / 64];
    __shared__ T sel_c[ICEM_MAX_ELITES];
    __shared__ int sel_i[ICEM_MAX_ELITES];
    block_select_sorted<T>(
        cnt, K, [&](int e) { return part_c[e]; }, [&](int e) { return part_i[e]; }, sel_c, sel_i, nullptr, red_c,
        red_i, red_e);
    __syncthreads();
    const int rs = hd + 2;
    for (int r = 0; r < K; ++r) {
        const int li = sel_i[r];
        T* rec = records + (size_t)r * rs;
        if (li == INT_MAX) {  // fewer than K candidates on this rank
            if (threadIdx.x == 0) rec_set(rec, inf_v<T>(), INT_MAX);
            for (int e = threadIdx.x; e < hd; e += WG) rec[2 + e] = (T)0;
        } else {
            const int g = li < n_loc ? shard_lo + li : n_global + (li - n_loc);
            if (threadIdx.x == 0) rec_set(rec, sel_c[r], g);
            const T* src = actions + (size_t)li * hd;
            for (int e = threadIdx.x; e < hd; e += WG) rec[2 + e] = src[e];
        }
    }
}

// One workgroup: global sorted top-K over the gathered records (+ kept elites), new elite set,
// mean/std refit with momentum (icem.py:199-211); on the last iteration also the executed action,
// min cost, time shift of the mean and std reset (icem.py:163-177).
template <typename T>
__global__ __launch_bounds__(WG) void merge_refit_kernel(MergeArgs<T> a) {
    __shared__ T red_c[WG / 64];
    __shared__ int red_i[WG / 64];
    __shared__ int red_e[WG / 64];
    __shared__ T sel_c[ICEM_MAX_ELITES];
    __shared__ int sel_i[ICEM_MAX_ELITES];
    __shared__ int sel_e[ICEM_MAX_ELITES];
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    T* new_mean = reinterpret_cast<T*>(smem_raw);  // [hd]
    const int hd = a.h * a.d;
    const int rs = hd + 2;
    const int cnt = a.n_rec + a.n_keep;
    if (a.xw.flags != nullptr) {  // in-library exchange: the peers' records of this iteration have landed
        if (threadIdx.x < 64) xchg_wait(a.xw, threadIdx.x);
        __syncthreads();
    }
    block_select_sorted<T>(
        cnt, a.K,
        [&](int e) { return e < a.n_rec ? nan_to_inf(a.records[(size_t)e * rs]) : a.elites_cost_cur[e - a.n_rec]; },
        [&](int e) { return e < a.n_rec ? rec_gidx(a.records + (size_t)e * rs) : a.n_global + (e - a.n_rec); }, sel_c,
        sel_i, sel_e, red_c, red_i, red_e);
    __syncthreads();
    auto src_row = [&](int r) -> const T* {
        int e = sel_e[r];
        if (e < 0) e = sel_e[0];  // fewer than K live candidates (cannot happen for K <= N / 2): repeat the best
        return e < a.n_rec ? a.records + (size_t)e * rs + 2 : a.elites_cur + (size_t)(e - a.n_rec) * hd;
    };
    for (int e = threadIdx.x; e < hd; e += WG) {
        for (int r = 0; r < a.K; ++r) a.elites_next[(size_t)r * hd + e] = src_row(r)[e];
        T nm, ns;
        refit_element<T>(a.K, a.alpha, a.mean_in[e], a.std_in[e], [&](int r) { return src_row(r)[e]; }, nm, ns);
        if (!a.last) {
            a.mean[e] = nm;
            a.std[e] = ns;
        } else {
            new_mean[e] = nm;
        }
    }
    if ((int)threadIdx.x < a.K) a.elites_cost_next[threadIdx.x] = sel_c[threadIdx.x];
    if (a.last) {
        __syncthreads();
        for (int e = threadIdx.x; e < hd; e += WG) {
            const int j = e % a.d;
            a.mean[e] = (e + a.d < hd) ? new_mean[e + a.d] : new_mean[e];
            a.std[e] = (a.high[j] - a.low[j]) / (T)2 * a.init_std;
        }
        if ((int)threadIdx.x < a.d) a.executed[threadIdx.x] = src_row(0)[threadIdx.x];
        if (threadIdx.x == 0) a.best_cost[0] = sel_c[0];
    }
}


// K3 + K4 of a single-GPU step in ONE launch: threshold selection + gather + refit (select_refit_body, generic_dev.h)
template <typename T>
__global__ __launch_bounds__(SELECT_NT) void select_refit_kernel(SelectArgs<T> s) {
    select_refit_body<T>(s);
}


// =============================================================================================
// launchers
// =============================================================================================

template <typename T>
SampleArgs<T> make_sample_args(const icem_handle* h, int n, long long first_index, const void* mean, const void* std,
                               const void* low, const void* high, const void* zr, const void* zi, uint64_t offset,
                               int t_begin, int row0_mean, void* out) {
    SampleArgs<T> a;
    std::memset((void*)&a, 0, sizeof(a));   // (every byte defined: a batched step compares recorded blocks)
    a.n = n;
    a.h = h->cfg.horizon;
    a.d = h->cfg.act_dim;
    a.F = h->F;
    a.tpw = std::max(1, WG / a.d);
    a.first_index = first_index;
    a.W = (const T*)h->W_dev;
    a.mean = (const T*)mean;
    a.std = (const T*)std;
    a.low = (const T*)low;
    a.high = (const T*)high;
    a.zr = (const T*)zr;
    a.zi = (const T*)zi;
    a.seed_lo = (uint32_t)h->cfg.seed;
    a.seed_hi = (uint32_t)(h->cfg.seed >> 32);
    a.off_lo = (uint32_t)offset;
    a.off_hi = (uint32_t)(offset >> 32);
    a.t_begin = t_begin;
    a.row0_mean = row0_mean;
    a.white = h->cfg.noise_beta <= 0 ? 1 : 0;
    a.out = (T*)out;
    return a;
}

template <typename T>
int launch_sample(const icem_handle* h, const SampleArgs<T>& a_in, const LaunchCtx& cx) {
    if (a_in.n <= 0) return ICEM_OK;
    hipStream_t st = cx.st;
    SampleArgs<T> a = a_in;
    // four lanes per row where the population leaves the chip mostly empty (the one-thread-per-row form's 256 rows per
    // workgroup are then a few long chains per CU); option gk_sample = 0: never (A/B, tests; read per call)
    // (decided from the handle's GLOBAL population, never from a call's or a shard's row count: one summation order per handle)
    const bool quad = opt_i(OPT_GK_SAMPLE) != 0 && a.d <= WG / 4 && (long long)h->cfg.num_traj * a.d <= 262144;
    if (quad) a.tpw = std::max(1, (WG / 4) / a.d);
    const int grid = (a.n + a.tpw - 1) / a.tpw;
    size_t lds = (size_t)a.tpw * a.h * a.d * sizeof(T);
    ProfScope prof(h, ICEM_K_SAMPLE, (long long)a.n * (a.h - a.t_begin), st);
    const bool r7 = h->cfg.rng_rounds == 7;
    if (cx.rec) {   // a batched step: the float64 quad form on device noise has a batched twin (k_generic_batch.hip)
        LaunchKey key;
        key.family = LAUNCH_GK_SAMPLE;
        key.h = a.h, key.d = a.d, key.O = h->HMAX, key.waves = a.tpw, key.form = h->cfg.rng_rounds, key.wgs[0] = grid;
        if constexpr (std::is_same<T, double>::value)
            submit(cx, key, quad && a.zr == nullptr, [&](void* dst, unsigned long long base) { batch_form(a, base, dst); }, [] {});
        else
            cx.rec->unsupported = true;
        return ICEM_OK;
    }
    if (quad) {
        lds = gk_sample_quad_lds(a.tpw, a.h, a.d, h->HMAX, sizeof(T));
        if (h->HMAX == 32) {
            if (r7)
                hipLaunchKernelGGL((sample_clip_quad_kernel<T, 32, 7>), dim3(grid), dim3(WG), lds, st, a);
            else
                hipLaunchKernelGGL((sample_clip_quad_kernel<T, 32, 10>), dim3(grid), dim3(WG), lds, st, a);
        } else {
            if (r7)
                hipLaunchKernelGGL((sample_clip_quad_kernel<T, 64, 7>), dim3(grid), dim3(WG), lds, st, a);
            else
                hipLaunchKernelGGL((sample_clip_quad_kernel<T, 64, 10>), dim3(grid), dim3(WG), lds, st, a);
        }
        ICEM_HIP_TRY(hipGetLastError());
        return ICEM_OK;
    }
    if (h->HMAX == 32) {
        if (r7)
            hipLaunchKernelGGL((sample_clip_kernel<T, 32, 7>), dim3(grid), dim3(WG), lds, st, a);
        else
            hipLaunchKernelGGL((sample_clip_kernel<T, 32, 10>), dim3(grid), dim3(WG), lds, st, a);
    } else {
        if (r7)
            hipLaunchKernelGGL((sample_clip_kernel<T, 64, 7>), dim3(grid), dim3(WG), lds, st, a);
        else
            hipLaunchKernelGGL((sample_clip_kernel<T, 64, 10>), dim3(grid), dim3(WG), lds, st, a);
    }
    ICEM_HIP_TRY(hipGetLastError());
    return ICEM_OK;
}

template <typename T, int KIND>
int launch_rollout_k(const icem_handle* h, const RolloutArgs<T>& a, const LaunchCtx& cx) {
    hipStream_t st = cx.st;
    const int grid = (a.n + WG - 1) / WG;
    ProfScope prof(h, ICEM_K_ROLLOUT, (long long)a.n * a.h, st);
    if constexpr (std::is_same<T, double>::value) {
        if (h->f64_arith == ICEM_F64_MFMA) {   // the f64 matrix-core rollout (k_rollout_f64.hip): any width; no batched twin
            if (cx.rec) {
                cx.rec->unsupported = true;
                return ICEM_OK;
            }
            return launch_rollout_f64_mfma(h, a.n, a.obs0, a.actions, a.costs, a.observations, st);
        }
    }
    const bool thread_form = opt_i(OPT_GK_ROLLOUT_THREAD) != 0;   // read per call: the path-equivalence test flips it between planners
    const bool widths = h->O == 8 || h->O == 16 || h->O == 17 || h->O == 18 || h->O == 24 || h->O == 32;
    if (cx.rec) {   // a batched step: the float64 rollouts' batched twins (k_generic_batch.hip), costs only
        const bool rows = !thread_form && !a.cs.ext;
        constexpr bool f64 = std::is_same<T, double>::value;
        LaunchKey key;
        key.family = rows ? LAUNCH_GK_ROLLOUT_ROWS : LAUNCH_GK_ROLLOUT_THREAD;
        key.h = a.h, key.d = a.d, key.O = h->O, key.kind = KIND;
        key.wgs[0] = rows ? (a.n + WG / (h->O <= 16 ? 16 : 32) - 1) / (WG / (h->O <= 16 ? 16 : 32)) : grid;
        if constexpr (f64) {
            RolloutArgs<T> ar = a;
            ar.ch = rows ? gk_rollout_rows_ch(h->O, a.h, a.d, sizeof(T)) : 0;
            submit(cx, key, widths && a.observations == nullptr && (rows || gk_rollout_thread_batched(h->O, KIND)),
                   [&](void* dst, unsigned long long) { batch_form(ar, dst); }, [] {});
        } else {
            cx.rec->unsupported = true;
        }
        return ICEM_OK;
    }
    if (!thread_form && !a.cs.ext) {   // a trajectory's row of lanes (rollout_cost_rows_kernel); term lists: the thread form
        switch (h->O) {
#define ICEM_CASE(OV)                                                                                                          \
    case OV: {                                                                                                                 \
        constexpr int TPW = WG / (OV <= 16 ? 16 : 32);                                                                         \
        RolloutArgs<T> ar = a;                                                                                                 \
        ar.ch = gk_rollout_rows_ch(OV, a.h, a.d, sizeof(T));   /* at most 32 KB of actions */                                  \
        const size_t lds = gk_rollout_rows_lds(OV, a.h, a.d, sizeof(T));                                                       \
        hipLaunchKernelGGL((rollout_cost_rows_kernel<T, OV, KIND>), dim3((a.n + TPW - 1) / TPW), dim3(WG), lds, st, ar);      \
        break;                                                                                                                 \
    }
            ICEM_CASE(8)
            ICEM_CASE(16)
            ICEM_CASE(17)
            ICEM_CASE(18)
            ICEM_CASE(24)
            ICEM_CASE(32)
#undef ICEM_CASE
            default:
                return fail(ICEM_E_UNSUPPORTED, "the generic rollout is compiled for padded observation widths 8, 16, 17, 18, 24, 32 only");
        }
        ICEM_HIP_TRY(hipGetLastError());
        return ICEM_OK;
    }
    switch (h->O) {
#define ICEM_CASE(OV)                                                                                  \
    case OV:                                                                                           \
        hipLaunchKernelGGL((rollout_cost_kernel<T, OV, KIND>), dim3(grid), dim3(WG), 0, st, a);        \
        break;
        ICEM_CASE(8)
        ICEM_CASE(16)
        ICEM_CASE(17)
        ICEM_CASE(18)
        ICEM_CASE(24)
        ICEM_CASE(32)
#undef ICEM_CASE
        default:
            return fail(ICEM_E_UNSUPPORTED, "the generic rollout is compiled for padded observation widths 8, 16, 17, 18, 24, 32 only");
    }
    ICEM_HIP_TRY(hipGetLastError());
    return ICEM_OK;
}

// a cost spec + a term list (has_terms: the list is on) in kernel-argument form -- from a handle or from the pair itself
template <typename T>
void fill_cost_args_pair(const icem_cost_spec& cost, const icem_cost_terms& t, bool has_terms, CostArgs<T>& cs) {
    cs.ctrl_w = (T)cost.ctrl_weight;
    cs.lin_w = (T)cost.lin_weight;
    cs.flip_pen = (T)cost.flip_penalty;
    cs.flip_th = (T)cost.flip_thresh;
    cs.lin_idx = cost.lin_idx;
    cs.flip_idx = cost.flip_idx;
    cs.ext = has_terms ? 1 : 0;
    cs.diff_w = (T)t.diff_weight;
    cs.health_pen = (T)t.health_penalty;
    cs.health_lo = (T)t.health_lo;
    cs.health_hi = (T)t.health_hi;
    cs.box_lo = (T)t.box_lo;
    cs.box_hi = (T)t.box_hi;
    cs.diff_idx = has_terms ? t.diff_idx : -1;
    cs.health_idx = has_terms ? t.health_idx : -1;
    cs.health_closed = t.health_closed;
    cs.box_from = (has_terms && t.health_idx >= 0) ? t.box_from : -1;
    cs.n_terms = has_terms ? t.n_terms : 0;
    for (int j = 0; j < ICEM_MAX_COST_TERMS; ++j) {
        const icem_cost_term& tm = t.terms[j];
        cs.terms[j].w = (T)tm.weight;
        cs.terms[j].th = (T)tm.thresh;
        cs.terms[j].gate_th = (T)tm.gate_thresh;
        cs.terms[j].kind = tm.kind;
        cs.terms[j].a = tm.a;
        cs.terms[j].b = tm.b;
        cs.terms[j].len = tm.len;
        cs.terms[j].gate_idx = tm.gate_idx;
    }
}

template <typename T>
void fill_cost_args(const icem_handle* h, CostArgs<T>& cs) {
    fill_cost_args_pair<T>(h->cost, h->terms, h->has_terms, cs);
}

void fill_cost_args_f32(const icem_handle* h, CostArgs<float>& cs) { fill_cost_args<float>(h, cs); }
void fill_cost_args_f64(const icem_handle* h, CostArgs<double>& cs) { fill_cost_args<double>(h, cs); }

bool cost_terms_on(const icem_cost_terms* t) { return t != nullptr && (t->diff_idx >= 0 || t->health_idx >= 0 || t->n_terms > 0); }

void fill_cost_args_f32(const icem_cost_spec& cost, const icem_cost_terms* terms, CostArgs<float>& cs) {
    static const icem_cost_terms none = {};
    fill_cost_args_pair<float>(cost, terms ? *terms : none, cost_terms_on(terms), cs);
}

// every index a cost term reads lies inside an observation of width o
const char* cost_indices_error(const icem_handle* h, int o) { return cost_indices_error(h->cost, h->has_terms ? &h->terms : nullptr, o); }

const char* cost_indices_error(const icem_cost_spec& cost, const icem_cost_terms* terms, int o) {
    if (cost.lin_idx < 0 || cost.lin_idx >= o || cost.flip_idx >= o) return "cost index outside the observation";
    if (terms == nullptr) return nullptr;
    const icem_cost_terms& t = *terms;
    if (t.diff_idx >= o || t.health_idx >= o || t.box_from >= o) return "cost term index outside the observation";
    for (int j = 0; j < t.n_terms; ++j) {
        const icem_cost_term& tm = t.terms[j];
        if (tm.a < 0 || tm.a + tm.len > o || (tm.b >= 0 && tm.b + tm.len > o) || tm.gate_idx >= o)
            return "cost term slice outside the observation";
    }
    return nullptr;
}

template <typename T>
int launch_trajectory_cost(const icem_handle* h, int n, int o, const void* obs, const void* nxt, long long ts,
                           long long ss, const void* actions, void* costs, hipStream_t st) {
    TrajCostArgs<T> a;
    a.n = n;
    a.h = h->cfg.horizon;
    a.d = h->cfg.act_dim;
    a.o = o;
    a.obs = (const T*)obs;
    a.nxt = (const T*)nxt;
    a.ts = ts;
    a.ss = ss;
    a.actions = (const T*)actions;
    a.costs = (T*)costs;
    fill_cost_args<T>(h, a.cs);
    a.cost_mode = h->cfg.cost_mode;
    // all_finite(obs) / the state box are part of `unhealthy` only; 1: coalesced sweep, 2: per-lane rows (narrow obs)
    a.sweep = a.cs.health_idx < 0 ? 0 : (o <= 32 ? 2 : 1);
    hipLaunchKernelGGL((trajectory_cost_kernel<T>), dim3((n + WG / 64 - 1) / (WG / 64)), dim3(WG), 0, st, a);
    ICEM_HIP_TRY(hipGetLastError());
    return ICEM_OK;
}

template <typename T>
int launch_rollout(const icem_handle* h, int n, const void* obs0, const void* actions, void* costs, void* observations,
                   const LaunchCtx& cx) {
    if (n <= 0) return ICEM_OK;
    RolloutArgs<T> a;
    std::memset((void*)&a, 0, sizeof(a));   // (every byte defined: a batched step compares recorded blocks)
    a.n = n;
    a.h = h->cfg.horizon;
    a.d = h->cfg.act_dim;
    a.o = h->obs_dim;
    a.A = (const T*)h->A_dev;
    a.B = (const T*)h->B_dev;
    a.obs0 = (const T*)obs0;
    a.actions = (const T*)actions;
    a.costs = (T*)costs;
    a.observations = (T*)observations;
    fill_cost_args<T>(h, a.cs);
    a.cost_mode = h->cfg.cost_mode;
    a.ch = 0;
    a.dbg = h->dbg;
    return h->model_kind == ICEM_MODEL_TANH ? launch_rollout_k<T, ICEM_MODEL_TANH>(h, a, cx)
                                            : launch_rollout_k<T, ICEM_MODEL_LINEAR>(h, a, cx);
}



template <typename T>
int launch_topk(int n, int K, const void* costs, void* out_c, int* out_i, void* ws, hipStream_t st) {
    const int nblk = topk_blocks(n);
    T* pc;
    int* pi;
    split_partial_ws<T>(ws, nblk, K, &pc, &pi);
    hipLaunchKernelGGL((topk_partial_kernel<T>), dim3(nblk), dim3(WG), 0, st, n, K, (const T*)costs, pc, pi);
    hipLaunchKernelGGL((topk_final_kernel<T>), dim3(1), dim3(WG), 0, st, nblk * K, K, (const T*)pc, (const int*)pi,
                       (T*)out_c, out_i);
    ICEM_HIP_TRY(hipGetLastError());
    return ICEM_OK;
}

// ---- dtype-erased entry points (host_common.h) ---------------------------------------------------------------------

// ---- icem_plan_step_learned* (learned_step.hip): the shifted elites of n problems, one launch ----
size_t gk_shift_sample_block_bytes() { return sizeof(ShiftSampleArgs); }

// the argument block of one problem (every byte defined: the blocks are compared with the previous step's)
void gk_shift_sample_block(const icem_handle* h, int n_shift, const void* mean, const void* std, const void* low, const void* high,
                           uint64_t offset_rel, const void* elites_src, void* out, void* dst) {
    std::memset(dst, 0, sizeof(ShiftSampleArgs));
    ShiftSampleArgs& g = *(ShiftSampleArgs*)dst;
    const SampleArgs<float> a = make_sample_args<float>(h, n_shift, 0, mean, std, low, high, nullptr, nullptr, offset_rel, h->cfg.horizon - 1, 0, out);
    g.s.n = a.n, g.s.h = a.h, g.s.d = a.d, g.s.F = a.F;
    g.s.tpw = gk_shift_sample_quad(h) ? std::max(1, (WG / 4) / a.d) : a.tpw;
    g.s.first_index = 0;
    g.s.W = a.W, g.s.mean = a.mean, g.s.std = a.std, g.s.low = a.low, g.s.high = a.high, g.s.zr = nullptr, g.s.zi = nullptr;
    g.s.seed_lo = a.seed_lo, g.s.seed_hi = a.seed_hi, g.s.off_lo = a.off_lo, g.s.off_hi = a.off_hi;
    g.s.t_begin = a.t_begin, g.s.row0_mean = 0, g.s.white = a.white, g.s.out = a.out;
    g.elites_src = (const float*)elites_src;
}

// launch_sample's choice between its two forms (one summation order per handle)
bool gk_shift_sample_quad(const icem_handle* h) {
    return opt_i(OPT_GK_SAMPLE) != 0 && h->cfg.act_dim <= WG / 4 && (long long)h->cfg.num_traj * h->cfg.act_dim <= 262144;
}

// f32, HMAX = 32 (h <= 32), rng_rounds = 10: what icem_plan_step_learned_ok admits
int gk_shift_sample_batch(const icem_handle* h, int n_problems, int n_shift_max, const void* args_dev, const BatchBases& bases, hipStream_t st) {
    const bool quad = gk_shift_sample_quad(h);
    const int d = h->cfg.act_dim, hh = h->cfg.horizon;
    const int tpw = quad ? std::max(1, (WG / 4) / d) : std::max(1, WG / d);
    const dim3 grid((n_shift_max + tpw - 1) / tpw, n_problems);
    if (quad)
        hipLaunchKernelGGL((shift_sample_batch_kernel<32, 10, true>), grid, dim3(WG),
                           ((((size_t)tpw * hh * d + 1) & ~(size_t)1) + (size_t)hh * 32) * sizeof(float), st, (const ShiftSampleArgs*)args_dev, bases);
    else
        hipLaunchKernelGGL((shift_sample_batch_kernel<32, 10, false>), grid, dim3(WG), (size_t)tpw * hh * d * sizeof(float), st,
                           (const ShiftSampleArgs*)args_dev, bases);
    ICEM_HIP_TRY(hipGetLastError());
    return ICEM_OK;
}

int gk_sample(const icem_handle* h, int n, long long first_index, const void* mean, const void* std, const void* low,
              const void* high, const void* zr, const void* zi, uint64_t offset, int t_begin, int row0_mean, void* out,
              const LaunchCtx& cx) {
    return ICEM_DISPATCH(h,
                         launch_sample<float>(h, make_sample_args<float>(h, n, first_index, mean, std, low, high, zr, zi, offset, t_begin, row0_mean, out), cx),
                         launch_sample<double>(h, make_sample_args<double>(h, n, first_index, mean, std, low, high, zr, zi, offset, t_begin, row0_mean, out), cx));
}

int gk_sample_truncnorm(const icem_handle* h, int n, long long first_index, const void* mean, const void* std,
                        const void* lower, const void* upper, const void* u, uint64_t offset, void* actions, hipStream_t st) {
    const icem_config& c = h->cfg;
    const int grid = (n * c.act_dim + WG - 1) / WG;
    const uint32_t sl = (uint32_t)c.seed, sh = (uint32_t)(c.seed >> 32), ol = (uint32_t)offset, oh = (uint32_t)(offset >> 32);
#define ICEM_TN(T, R)                                                                                                    \
    hipLaunchKernelGGL((sample_truncnorm_kernel<T, R>), dim3(grid), dim3(WG), 0, st, n, c.horizon, c.act_dim,            \
                       (long long)first_index, (const T*)mean, (const T*)std, (const T*)lower, (const T*)upper,          \
                       (const T*)u, sl, sh, ol, oh, (T*)actions)
    if (c.dtype == ICEM_F64) {
        if (c.rng_rounds == 7) ICEM_TN(double, 7); else ICEM_TN(double, 10);
    } else {
        if (c.rng_rounds == 7) ICEM_TN(float, 7); else ICEM_TN(float, 10);
    }
#undef ICEM_TN
    ICEM_HIP_TRY(hipGetLastError());
    return ICEM_OK;
}

int gk_sample_piecewise(const icem_handle* h, int n, long long call_offset, int change_freq, long long first_block,
                        const void* low, const void* high, const void* u, void* actions, hipStream_t st) {
    const icem_config& c = h->cfg;
    const long long total = (long long)n * c.horizon * c.act_dim;
    const int grid = (int)((total + WG - 1) / WG);
    const uint32_t sl = (uint32_t)c.seed, sh = (uint32_t)(c.seed >> 32);
#define ICEM_PW(T, R)                                                                                              \
    hipLaunchKernelGGL((sample_piecewise_kernel<T, R>), dim3(grid), dim3(WG), 0, st, total, c.act_dim,             \
                       (long long)call_offset, change_freq, (long long)first_block, (const T*)low, (const T*)high, \
                       (const T*)u, sl, sh, (T*)actions)
    if (c.dtype == ICEM_F64) {
        if (c.rng_rounds == 7) ICEM_PW(double, 7); else ICEM_PW(double, 10);
    } else {
        if (c.rng_rounds == 7) ICEM_PW(float, 7); else ICEM_PW(float, 10);
    }
#undef ICEM_PW
    ICEM_HIP_TRY(hipGetLastError());
    return ICEM_OK;
}

int gk_cem_bounds(const icem_handle* h, int like_levine, const void* mean, void* std, const void* low, const void* high,
                  void* lower, void* upper, hipStream_t st) {
    const int grid = (h->hd + WG - 1) / WG;
    if (h->cfg.dtype == ICEM_F64)
        hipLaunchKernelGGL((cem_bounds_kernel<double>), dim3(grid), dim3(WG), 0, st, h->hd, h->cfg.act_dim, like_levine,
                           (const double*)mean, (double*)std, (const double*)low, (const double*)high, (double*)lower, (double*)upper);
    else
        hipLaunchKernelGGL((cem_bounds_kernel<float>), dim3(grid), dim3(WG), 0, st, h->hd, h->cfg.act_dim, like_levine,
                           (const float*)mean, (float*)std, (const float*)low, (const float*)high, (float*)lower, (float*)upper);
    ICEM_HIP_TRY(hipGetLastError());
    return ICEM_OK;
}

int gk_philox_normals(const icem_handle* h, int n, long long first_index, uint64_t offset, void* z_r, void* z_i,
                      hipStream_t st) {
    const int grid = (n * h->cfg.act_dim + WG - 1) / WG;
    const bool r7 = h->cfg.rng_rounds == 7;
#define ICEM_PN(T, HM, R)                                                                                           \
    hipLaunchKernelGGL((philox_normals_kernel<T, HM, R>), dim3(grid), dim3(WG), 0, st,                              \
                       make_sample_args<T>(h, n, first_index, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, \
                                           offset, 0, 0, nullptr),                                                  \
                       (T*)z_r, (T*)z_i)
    if (h->cfg.dtype == ICEM_F64) {
        if (h->HMAX == 32) { if (r7) ICEM_PN(double, 32, 7); else ICEM_PN(double, 32, 10); }
        else { if (r7) ICEM_PN(double, 64, 7); else ICEM_PN(double, 64, 10); }
    } else {
        if (h->HMAX == 32) { if (r7) ICEM_PN(float, 32, 7); else ICEM_PN(float, 32, 10); }
        else { if (r7) ICEM_PN(float, 64, 7); else ICEM_PN(float, 64, 10); }
    }
#undef ICEM_PN
    ICEM_HIP_TRY(hipGetLastError());
    return ICEM_OK;
}

int gk_rollout(const icem_handle* h, int n, const void* obs0, const void* actions, void* costs, void* observations,
               const LaunchCtx& cx) {
    return ICEM_DISPATCH(h, launch_rollout<float>(h, n, obs0, actions, costs, observations, cx),
                         launch_rollout<double>(h, n, obs0, actions, costs, observations, cx));
}

int gk_trajectory_cost(const icem_handle* h, int n, int o, const void* obs, const void* nxt, long long ts, long long ss,
                       const void* actions, void* costs, hipStream_t st) {
    return ICEM_DISPATCH(h, launch_trajectory_cost<float>(h, n, o, obs, nxt, ts, ss, actions, costs, st),
                         launch_trajectory_cost<double>(h, n, o, obs, nxt, ts, ss, actions, costs, st));
}

int gk_cost_reduce(const icem_handle* h, int n, const void* step_costs, void* costs, hipStream_t st) {
    const int grid = (n + WG - 1) / WG;
    if (h->cfg.dtype == ICEM_F64)
        hipLaunchKernelGGL((cost_reduce_kernel<double>), dim3(grid), dim3(WG), 0, st, n, h->cfg.horizon, h->cfg.cost_mode,
                           (const double*)step_costs, (double*)costs);
    else
        hipLaunchKernelGGL((cost_reduce_kernel<float>), dim3(grid), dim3(WG), 0, st, n, h->cfg.horizon, h->cfg.cost_mode,
                           (const float*)step_costs, (float*)costs);
    ICEM_HIP_TRY(hipGetLastError());
    return ICEM_OK;
}

int gk_topk(const icem_handle* h, int n, int K, const void* costs, void* out_c, int* out_i, void* ws, hipStream_t st) {
    return ICEM_DISPATCH(h, launch_topk<float>(n, K, costs, out_c, out_i, ws, st),
                         launch_topk<double>(n, K, costs, out_c, out_i, ws, st));
}

template <typename T>
static int topk_partial_t(const icem_handle* h, int n_cand, int K, const void* costs, void* ws, int nblk, hipStream_t st) {
    T* pc;
    int* pi;
    split_partial_ws<T>(ws, nblk, K, &pc, &pi);
    ProfScope prof(h, ICEM_K_TOPK_PARTIAL, n_cand, st);
    hipLaunchKernelGGL((topk_partial_kernel<T>), dim3(nblk), dim3(WG), 0, st, n_cand, K, (const T*)costs, pc, pi);
    return ICEM_OK;
}
int gk_topk_partial(const icem_handle* h, int n_cand, int K, const void* costs, void* ws, int nblk, hipStream_t st) {
    ICEM_DISPATCH(h, topk_partial_t<float>(h, n_cand, K, costs, ws, nblk, st), topk_partial_t<double>(h, n_cand, K, costs, ws, nblk, st));
    ICEM_HIP_TRY(hipGetLastError());
    return ICEM_OK;
}

template <typename T>
static int local_pack_t(const icem_handle* h, int nblk, int K, int n_loc, int shard_lo, int n_global, const void* ws,
                        const void* actions, void* records, hipStream_t st) {
    T* pc;
    int* pi;
    split_partial_ws<T>(const_cast<void*>(ws), nblk, K, &pc, &pi);
    ProfScope prof(h, ICEM_K_LOCAL_PACK, nblk * K, st);
    hipLaunchKernelGGL((local_pack_kernel<T>), dim3(1), dim3(WG), 0, st, nblk * K, K, h->hd, n_loc, shard_lo, n_global,
                       (const T*)pc, (const int*)pi, (const T*)actions, (T*)records);
    return ICEM_OK;
}
int gk_local_pack(const icem_handle* h, int nblk, int K, int n_loc, int shard_lo, int n_global, const void* ws,
                  const void* actions, void* records, hipStream_t st) {
    ICEM_DISPATCH(h, local_pack_t<float>(h, nblk, K, n_loc, shard_lo, n_global, ws, actions, records, st),
                  local_pack_t<double>(h, nblk, K, n_loc, shard_lo, n_global, ws, actions, records, st));
    ICEM_HIP_TRY(hipGetLastError());
    return ICEM_OK;
}

int gk_gather_refit(const icem_handle* h, const void* actions, const int32_t* idx, int k, void* mean, void* std,
                    void* elites_out, hipStream_t st) {
    const int grid = (h->hd + WG - 1) / WG;
    if (h->cfg.dtype == ICEM_F64)
        hipLaunchKernelGGL((gather_refit_kernel<double>), dim3(grid), dim3(WG), 0, st, h->hd, k, (double)h->cfg.alpha,
                           (const double*)actions, idx, (double*)mean, (double*)std, (double*)elites_out);
    else
        hipLaunchKernelGGL((gather_refit_kernel<float>), dim3(grid), dim3(WG), 0, st, h->hd, k, (float)h->cfg.alpha,
                           (const float*)actions, idx, (float*)mean, (float*)std, (float*)elites_out);
    ICEM_HIP_TRY(hipGetLastError());
    return ICEM_OK;
}

int gk_shift(const icem_handle* h, void* mean, void* std, const void* low, const void* high, hipStream_t st) {
    if (h->cfg.dtype == ICEM_F64)
        hipLaunchKernelGGL((shift_kernel<double>), dim3(1), dim3(WG), (size_t)h->hd * 8, st, h->cfg.horizon, h->cfg.act_dim,
                           (double)h->cfg.init_std, (double*)mean, (double*)std, (const double*)low, (const double*)high);
    else
        hipLaunchKernelGGL((shift_kernel<float>), dim3(1), dim3(WG), (size_t)h->hd * 4, st, h->cfg.horizon, h->cfg.act_dim,
                           (float)h->cfg.init_std, (float*)mean, (float*)std, (const float*)low, (const float*)high);
    ICEM_HIP_TRY(hipGetLastError());
    return ICEM_OK;
}

int gk_reset(const icem_handle* h, void* mean, void* std, const void* low, const void* high, hipStream_t st) {
    const int grid = (h->hd + WG - 1) / WG;
    if (h->cfg.dtype == ICEM_F64)
        hipLaunchKernelGGL((reset_kernel<double>), dim3(grid), dim3(WG), 0, st, h->cfg.horizon, h->cfg.act_dim,
                           (double)h->cfg.init_std, (double*)mean, (double*)std, (const double*)low, (const double*)high);
    else
        hipLaunchKernelGGL((reset_kernel<float>), dim3(grid), dim3(WG), 0, st, h->cfg.horizon, h->cfg.act_dim,
                           (float)h->cfg.init_std, (float*)mean, (float*)std, (const float*)low, (const float*)high);
    ICEM_HIP_TRY(hipGetLastError());
    return ICEM_OK;
}

int gk_shift_elites(const icem_handle* h, int n_extra, const void* elites, void* dst, const LaunchCtx& cx) {
    const icem_config& c = h->cfg;
    hipStream_t st = cx.st;
    if (cx.rec) {   // a batched step: one workgroup per problem (k_generic_batch.hip)
        LaunchKey key;
        key.family = LAUNCH_GK_SHIFT;
        key.h = c.horizon, key.d = c.act_dim, key.wgs[0] = 1;
        submit(cx, key, c.dtype == ICEM_F64, [&](void* blk, unsigned long long) {
            ShiftElitesArgs<double>& g = *(ShiftElitesArgs<double>*)blk;   // (zeroed)
            g.n_reuse = n_extra, g.h = c.horizon, g.d = c.act_dim;
            g.elites = (const double*)elites, g.dst = (double*)dst;
        }, [] {});
        return ICEM_OK;
    }
    if (c.dtype == ICEM_F64)
        hipLaunchKernelGGL((shift_elites_kernel<double>), dim3(1), dim3(WG), 0, st, n_extra, c.horizon, c.act_dim,
                           (const double*)elites, (double*)dst);
    else
        hipLaunchKernelGGL((shift_elites_kernel<float>), dim3(1), dim3(WG), 0, st, n_extra, c.horizon, c.act_dim,
                           (const float*)elites, (float*)dst);
    ICEM_HIP_TRY(hipGetLastError());
    return ICEM_OK;
}

template <typename T>
static void merge_refit_t(const icem_handle* h, const MergeArgsV& v, hipStream_t st) {
    MergeArgs<T> a;
    a.n_rec = v.n_rec;
    a.n_keep = v.n_keep;
    a.K = v.K;
    a.h = v.h;
    a.d = v.d;
    a.n_global = v.n_global;
    a.last = v.last;
    a.alpha = (T)v.alpha;
    a.init_std = (T)v.init_std;
    a.records = (const T*)v.records;
    a.elites_cur = (const T*)v.elites_cur;
    a.elites_cost_cur = (const T*)v.elites_cost_cur;
    a.elites_next = (T*)v.elites_next;
    a.elites_cost_next = (T*)v.elites_cost_next;
    a.mean_in = (const T*)v.mean_in;
    a.std_in = (const T*)v.std_in;
    a.mean = (T*)v.mean;
    a.std = (T*)v.std;
    a.low = (const T*)v.low;
    a.high = (const T*)v.high;
    a.executed = (T*)v.executed;
    a.best_cost = (T*)v.best_cost;
    a.xw = v.xw;
    ProfScope prof(h, ICEM_K_MERGE_REFIT, a.n_rec + a.n_keep, st);
    hipLaunchKernelGGL((merge_refit_kernel<T>), dim3(1), dim3(WG), (size_t)v.h * v.d * sizeof(T), st, a);
}
// world == 1: selection + gather + refit of an iteration in one launch (select_refit_kernel).  The worst case of the
// threshold -- K threads of each of the workgroup's waves hold ALL their keys at or below it -- must fit the candidate
// array; beyond that size the three-launch path runs.
bool gk_select_ok(const icem_handle* h, int n_cand, int n_keep, int K) {
    const bool off = opt_i(OPT_GK_SELECT) == 0;     // read per call (path-equivalence test)
    if (off || h->cfg.world != 1 || K < 1 || K > ICEM_MAX_ELITES) return false;
    const long long per_thread = ((long long)n_cand + n_keep + SELECT_NT - 1) / SELECT_NT;
    return (long long)(SELECT_NT / 64) * K * per_thread <= SELECT_CAP;
}

template <typename T>
static void select_refit_t(const icem_handle* h, int n_cand, int n_loc, const void* costs, const void* actions, const MergeArgsV& v,
                           const LaunchCtx& cx) {
    hipStream_t st = cx.st;
    SelectArgs<T> s;
    std::memset((void*)&s, 0, sizeof(s));   // (every byte defined: a batched step compares recorded blocks)
    s.n_cand = n_cand;
    s.n_loc = n_loc;
    s.cap = SELECT_CAP;
    s.costs = (const T*)costs;
    s.actions = (const T*)actions;
    s.dbg = h->dbg;
    MergeArgs<T>& a = s.m;
    a.n_rec = 0;
    a.n_keep = v.n_keep;
    a.K = v.K;
    a.h = v.h;
    a.d = v.d;
    a.n_global = v.n_global;
    a.last = v.last;
    a.alpha = (T)v.alpha;
    a.init_std = (T)v.init_std;
    a.records = nullptr;
    a.elites_cur = (const T*)v.elites_cur;
    a.elites_cost_cur = (const T*)v.elites_cost_cur;
    a.elites_next = (T*)v.elites_next;
    a.elites_cost_next = (T*)v.elites_cost_next;
    a.mean_in = (const T*)v.mean_in;
    a.std_in = (const T*)v.std_in;
    a.mean = (T*)v.mean;
    a.std = (T*)v.std;
    a.low = (const T*)v.low;
    a.high = (const T*)v.high;
    a.executed = (T*)v.executed;
    a.best_cost = (T*)v.best_cost;
    a.xw = XchgWait{};
    if (cx.rec) {   // a batched step: one workgroup per problem (k_generic_batch.hip)
        LaunchKey key;
        key.family = LAUNCH_GK_SELECT;
        key.h = v.h, key.d = v.d, key.wgs[0] = 1;
        if constexpr (std::is_same<T, double>::value)
            submit(cx, key, true, [&](void* dst, unsigned long long) { batch_form(s, dst); }, [] {});
        else
            cx.rec->unsupported = true;
        return;
    }
    ProfScope prof(h, ICEM_K_MERGE_REFIT, n_cand + v.n_keep, st);
    hipLaunchKernelGGL((select_refit_kernel<T>), dim3(1), dim3(SELECT_NT), (size_t)v.h * v.d * sizeof(T), st, s);
}
int gk_select_refit(const icem_handle* h, int n_cand, int n_loc, const void* costs, const void* actions, const MergeArgsV& a,
                    const LaunchCtx& cx) {
    if (h->cfg.dtype == ICEM_F64)
        select_refit_t<double>(h, n_cand, n_loc, costs, actions, a, cx);
    else
        select_refit_t<float>(h, n_cand, n_loc, costs, actions, a, cx);
    ICEM_HIP_TRY(hipGetLastError());
    return ICEM_OK;
}

int gk_merge_refit(const icem_handle* h, const MergeArgsV& a, hipStream_t st) {
    if (h->cfg.dtype == ICEM_F64)
        merge_refit_t<double>(h, a, st);
    else
        merge_refit_t<float>(h, a, st);
    ICEM_HIP_TRY(hipGetLastError());
    return ICEM_OK;
}

}  // namespace icem
