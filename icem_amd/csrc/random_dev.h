// random_dev.h -- the device bodies of the random-shooting step's kernels, shared by k_random.hip (the built-in model's step:
// icem_plan_step_random*), k_random_learned.hip (the step through the learned dynamics: icem_plan_step_random_learned_batch) and
// k_random_members.hip (that step through an ensemble's members: icem_plan_step_random_learned_models).
//   random_sample_body   icem_sample_piecewise's pool (mpc.py:96-109): a workgroup owns RANDOM_SPAN consecutive elements, draws
//                        each (block, dimension) value they need once into LDS -- the operator's arithmetic, the same bits --
//                        and stores its span from there, four elements per store
//   random_select_body   np.argmin(costs) (mpc.py:122) as icem_topk_sorted(costs, 1) gives it, the gathers behind it
// MIRROR (compile time, false in every kernel of k_random.hip): the body works on a slice of a pool and writes what it stores
// (the sampler) or reads (the selection's costs) into the problem's own buffer as well.
// Src (compile time, the plain load in every kernel but one): where the selection gets a row's cost from.
// Internal; device code only.
#pragma once
#include "fused_dev.h"     // gptr
#include "generic_dev.h"   // key_less, nan_to_inf, wave_min_key, fmad, row_stream
#include "random_step.h"
#include "update_small_body.h"   // MemberCosts

namespace icem {

namespace {

static_assert(RANDOM_SPAN % 4 == 0 && RANDOM_SPAN % WG == 0, "a thread stores groups of four elements");
// the table of a workgroup: at most RANDOM_SPAN / d + 2 sample() calls touch its span, each at most a block of its own
constexpr size_t random_table_elems(int d) { return (size_t)RANDOM_SPAN + 2 * (size_t)d; }
static_assert(random_table_elems(ICEM_MAX_ACT_DIM) * sizeof(double) <= 64 * 1024, "the block table fits LDS at every shape");

// the sampler's store of a thread's group of four elements, for its second destination (MIRROR): 16-byte stores where dst is
// 16-byte aligned (vec) and the group lies inside the span, else element by element
template <typename T>
__device__ __forceinline__ void random_mirror4(T* dst, bool vec, int q, int n_here, const T (&v)[4]) {
    if (vec && q + 4 <= n_here) {
        if constexpr (sizeof(T) == 4) {
            *reinterpret_cast<float4*>(dst + q) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
            *reinterpret_cast<double2*>(dst + q) = make_double2(v[0], v[1]);
            *reinterpret_cast<double2*>(dst + q + 2) = make_double2(v[2], v[3]);
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (q + k < n_here) dst[q + k] = v[k];
    }
}

// block of sample() call number (s + freq): 0 while s < 0 (the action drawn at construction), then 1 + s / (freq + 1).
// MIRROR: every element stored to a.out also goes to mirror (the same element index; the 16-byte store is decided per destination)
template <typename T, int ROUNDS, bool MIRROR = false>
__device__ __forceinline__ void random_sample_body(const RandomSampleArgs<T>& a, T* mirror = nullptr) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    T* tab = reinterpret_cast<T*>(smem_raw);
    const int tid = threadIdx.x;
    const int d = a.d, per = a.freq + 1;
    const long long e0 = (long long)blockIdx.x * RANDOM_SPAN;
    if (e0 >= a.total) return;
    const int n_here = (int)min((long long)RANDOM_SPAN, a.total - e0);
    // the span's first call, its dimension offset and its place among the held blocks: 64-bit once, 32-bit per element
    const long long call0 = a.call_offset + e0 / d;
    const int r0 = (int)(e0 % d);
    const long long s0 = call0 - a.freq;
    const long long m0 = s0 >= 0 ? s0 / per : 0;            // blocks 1 .. m0 lie wholly before the span's first call
    const int sl = s0 >= 0 ? (int)(s0 % per) : (int)s0;     // (s0 >= -freq > -64)
    const int rel0 = sl < 0 ? -1 : 0;                       // the first call's block is 1 + m0 + rel0
    auto rel_of = [&](int lc) { const int t = sl + lc; return t < 0 ? -1 : t / per; };   // local call -> block - (1 + m0)
    const int nb = rel_of((r0 + n_here - 1) / d) - rel0 + 1;
    const long long b_first = 1 + m0 + rel0;
    for (int x = tid; x < nb * d; x += WG) {
        const int bl = x / d, j = x - bl * d;
        const long long b = b_first + bl;
        T uu;
        if (a.u) {
            uu = a.u[(b - a.first_block) * d + j];
        } else {
            Xoshiro128pp rng = row_stream<ROUNDS>((uint32_t)b, (uint32_t)j, (uint32_t)((unsigned long long)b >> 32), 0x52414E44u /* "RAND" */,
                                                  a.seed_lo, a.seed_hi);
            uu = ((T)rng.next() + (T)0.5) * (T)2.3283064365386963e-10;
        }
        tab[x] = fmad(a.high[j] - a.low[j], uu, a.low[j]);
    }
    __syncthreads();
    T* out = a.out + e0;
    const bool vec = (reinterpret_cast<uintptr_t>(out) & 15) == 0;
    T* out_m = nullptr;
    bool vec_m = false;
    if constexpr (MIRROR) {
        out_m = mirror + e0;
        vec_m = (reinterpret_cast<uintptr_t>(out_m) & 15) == 0;
    }
    for (int q = tid * 4; q < n_here; q += WG * 4) {
        T v[4];
        // the group's first element: its local call, its dimension and the call's place among the blocks -- quotient tq and
        // remainder tr of (sl + lc) by the hold length, kept by increments from there (a call before the first drawn block,
        // sl + lc < 0 with |sl| <= freq, is tq = -1 with tr counting up to the hold length: the same carry)
        int lc = (r0 + q) / d, j = (r0 + q) - lc * d;
        const int t = sl + lc;
        int tq = t < 0 ? -1 : t / per, tr = t < 0 ? per + t : t - tq * per;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            v[k] = q + k < n_here ? tab[(tq - rel0) * d + j] : (T)0;   // (past the span: no table entry, nothing stored)
            if (++j == d) {
                j = 0;
                if (++tr == per) tr = 0, ++tq;
            }
        }
        if (vec && q + 4 <= n_here) {
            if constexpr (sizeof(T) == 4) {
                *reinterpret_cast<float4*>(out + q) = make_float4(v[0], v[1], v[2], v[3]);
            } else {
                *reinterpret_cast<double2*>(out + q) = make_double2(v[0], v[1]);
                *reinterpret_cast<double2*>(out + q + 2) = make_double2(v[2], v[3]);
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (q + k < n_here) out[q + k] = v[k];
        }
        if constexpr (MIRROR) random_mirror4(out_m, vec_m, q, n_here, v);
    }
}

template <typename T>
__device__ __forceinline__ RandomSampleArgs<T> from_device(const RandomSampleArgs<T>& m) {
    RandomSampleArgs<T> a = m;
    a.low = gptr(m.low), a.high = gptr(m.high), a.u = nullptr, a.out = gptr(m.out);   // (a batch offers no external uniforms)
    return a;
}

// ---- selection + epilogue ----
__device__ __forceinline__ unsigned long long cost_bits(float c) { return (unsigned long long)__float_as_uint(c); }
__device__ __forceinline__ unsigned long long cost_bits(double c) { return (unsigned long long)__double_as_longlong(c); }
__device__ __forceinline__ void bits_cost(unsigned long long b, float& c) { c = __uint_as_float((unsigned)b); }
__device__ __forceinline__ void bits_cost(unsigned long long b, double& c) { c = __longlong_as_double((long long)b); }

// the smallest (cost, index) pair of the workgroup's threads -> every thread (red_*: one entry per wave)
template <typename T>
__device__ __forceinline__ void wg_min_key(T& c, int& i, T* red_c, int* red_i) {
    constexpr int NW = RANDOM_SELECT_NT / 64;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    icem::wave_min_key(c, i);   // (generic_dev.h's pair form)
    if (lane == 0) red_c[wave] = c, red_i[wave] = i;
    __syncthreads();
    c = red_c[0], i = red_i[0];
#pragma unroll
    for (int w = 1; w < NW; ++w)
        if (key_less(red_c[w], red_i[w], c, i)) c = red_c[w], i = red_i[w];
    __syncthreads();
}

// where row i of the slice gets its cost from: the plain load of a.costs[i] ...
template <typename T>
struct SliceCosts {
    __device__ __forceinline__ T operator()(const RandomSelectArgs<T>& a, int i) const { return a.costs[i]; }
};
// ... or (random_select_members_batch_kernel, k_random_members.hip) the costs of an ensemble's members: MemberCosts
// (update_small_body.h), which reduces them as rssm_ensemble_reduce_kernel does -- all of a row's loads requested before the
// first is consumed -- and stores the reduced cost, as computed, where a.costs[i] would have been read

// MIRROR: every cost the source gives is stored, as given, at the same index of mirror_costs
template <typename T, bool MIRROR = false, class Src = SliceCosts<T>>
__device__ __forceinline__ void random_select_body(const RandomSelectArgs<T>& a, T* mirror_costs = nullptr, const Src src = Src()) {
    constexpr int NW = RANDOM_SELECT_NT / 64;
    __shared__ T red_c[NW];
    __shared__ int red_i[NW];
    __shared__ unsigned last;
    const int tid = threadIdx.x;
    const int nblk = (int)gridDim.x;
    const int lo = (int)blockIdx.x * RANDOM_SLICE, hi = (int)min((long long)a.n, (long long)lo + RANDOM_SLICE);
    T bc = inf_v<T>();
    int bi = INT_MAX;
    for (int i = lo + tid; i < hi; i += RANDOM_SELECT_NT) {
        const T raw = src(a, i);
        if constexpr (MIRROR) mirror_costs[i] = raw;
        const T c = nan_to_inf(raw);
        if (key_less(c, i, bc, bi)) bc = c, bi = i;
    }
    wg_min_key(bc, bi, red_c, red_i);
    if (nblk > 1) {
        // the pair leaves as two 8-byte agent-scope stores; release, ticket; the workgroup whose ticket is the last one
        // acquires and reads every pair with agent-scope loads
        if (tid == 0) {
            __hip_atomic_store(a.part + 2 * blockIdx.x, cost_bits(bc), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(a.part + 2 * blockIdx.x + 1, (unsigned long long)(unsigned)bi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __threadfence();
            const unsigned tk = __hip_atomic_fetch_add(a.ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
            last = tk == (unsigned)nblk - 1;
            if (last) {
                __hip_atomic_store(a.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // the next launch starts at 0
                __threadfence();
            }
        }
        __syncthreads();
        if (!last) return;
        bc = inf_v<T>(), bi = INT_MAX;
        for (int w = tid; w < nblk; w += RANDOM_SELECT_NT) {
            T c;
            bits_cost(__hip_atomic_load(a.part + 2 * w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), c);
            const int i = (int)(unsigned)__hip_atomic_load(a.part + 2 * w + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (key_less(c, i, bc, bi)) bc = c, bi = i;
        }
        wg_min_key(bc, bi, red_c, red_i);
    }
    // every pool has a row 0 and (+inf, 0) orders before the starting pair: bi is a row
    const T cost = a.canon ? bc + (T)0 : bc;   // (the f32 one-launch top-k reports its key's cost: -0 -> +0)
    const T* row = a.actions + (size_t)bi * a.hd;
    for (int e = tid; e < a.hd; e += RANDOM_SELECT_NT) {
        const T v = row[e];
        a.best_actions[e] = v;
        if (e < a.d) {
            a.result[e] = v;
            if (a.result_row) a.result_row[e] = v;
        }
    }
    if (tid == 0) {
        a.result[a.d] = cost, a.result[a.d + 1] = (T)bi;
        if (a.result_row) a.result_row[a.d] = cost, a.result_row[a.d + 1] = (T)bi;
    }
}

template <typename T>
__device__ __forceinline__ RandomSelectArgs<T> from_device(const RandomSelectArgs<T>& m) {
    RandomSelectArgs<T> a = m;
    a.costs = gptr(m.costs), a.actions = gptr(m.actions), a.best_actions = gptr(m.best_actions), a.result = gptr(m.result);
    a.result_row = gptr(m.result_row), a.part = gptr(m.part), a.ticket = gptr(m.ticket);
    return a;
}

}  // namespace

}  // namespace icem
