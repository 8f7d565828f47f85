// k_merge.hip -- K3 + K4 as a launch of its own: merge_single_kernel (global sorted top-K of the candidate lists or
// all-gathered records, elite gather, refit, last-iteration epilogue; one workgroup, wave 0 selects) and
// pack_records_kernel (sharded runs: this rank's K best as records for the exchange).
#include "fused_dev.h"
#include "refit.h"
#include "update_small_body.h"

namespace icem {

namespace {

// KX > 0 ("exact K"): the launcher has checked a.K == KX (merge_rows, refit_element_regs)
template <int KREG, bool REC, int KX = 0>
__device__ __forceinline__ void merge_single_body(const MergeSingleArgs& a, unsigned char* smem_raw) {
    __shared__ unsigned long long sel[64];
    __shared__ unsigned long long cand[64];
    __shared__ int slot[64];
    // (typed as LDS: written inside the lambda below through a generic pointer, the stores were flat_store)
    typedef float __attribute__((address_space(3))) * LdsF;
    const LdsF new_mean = (LdsF)smem_raw;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int hd = a.h * a.d;
    if (a.dbg && threadIdx.x == 0) a.dbg[0] = wall_clock64();
    // old mean/std of this thread's elements: issued now, consumed after the selection -- and, in the step's last merge, the
    // bounds its epilogue resets the std from (behind the final barrier they were one more memory round trip)
    constexpr int EPL = 4;
    const bool pre = hd <= MERGE_WG * EPL;
    float om[EPL], os[EPL], blo[EPL], bhi[EPL];
#pragma unroll
    for (int i = 0; i < EPL; ++i) {
        const int e = tid + i * MERGE_WG;
        om[i] = (pre && e < hd) ? a.mean[e] : 0.f;
        os[i] = (pre && e < hd) ? a.std[e] : 0.f;
    }
    // (the bounds' index is a division by d: the selecting wave asks for them BEHIND its selection, where they ride the
    // gather's round trip -- in front of it they put 0.4 us of address arithmetic and older loads before the keys')
    auto request_bounds = [&]() {
#pragma unroll
        for (int i = 0; i < EPL; ++i) {
            const int e = tid + i * MERGE_WG;
            blo[i] = (pre && a.last && e < hd) ? a.low[e % a.d] : 0.f;
            bhi[i] = (pre && a.last && e < hd) ? a.high[e % a.d] : 0.f;
        }
    };
    // who asks when: the records form and waves 1..3 of the lists form here, at entry; wave 0 of the lists form -- the one
    // that selects -- behind its selection, below.  Every thread asks exactly once, and only in the step's last merge.
    if (REC || tid >= 64) request_bounds();
    if constexpr (REC) {
        merge_select_records_wg(a, tid < 64, lane, tid, MERGE_WG, sel, slot);   // (all threads: the records' keys ranked by counting)
        if (a.dbg && threadIdx.x == 0) a.dbg[4] = wall_clock64();
    } else {
        if (tid < 64) merge_select_shallow<3>(a, lane, cand, sel);
        if (a.dbg && threadIdx.x == 0) a.dbg[4] = wall_clock64();
        if (tid < 64) request_bounds();   // (wave 0: in flight across the barrier, consumed in the epilogue)
        __syncthreads();
    }
    // ---- all 4 waves: gather + refit (icem.py:201-211); row pointers first, then all K loads in flight ----
    const float* rows[KREG];
    constexpr int NR = KX > 0 ? KX : KREG;   // rows gathered
    merge_rows<KREG, REC, KX>(a, sel, slot, rows);
    // (stores count on the same counter as loads here: a store between two of the gather's loads makes every later wait a
    // wait for that store's acknowledgement.  So: all K loads, ONE wait for them (the refit needs them all anyway), and only
    // then the K stores, back to back with nothing left to wait for.)
    float best0 = 0.f;   // element `tid` of the best row: the executed action's, where tid < d (the epilogue)
    auto finish_one = [&](int e, float old_mean, float old_std) {
        float xs[KREG];
#pragma unroll
        for (int r = 0; r < NR; ++r) xs[r] = rows[r][e];
#pragma unroll
        for (int r = 0; r < NR; ++r) asm volatile("" : "+v"(xs[r]));   // every row's value has arrived HERE
        float nm, ns;
        refit_element_regs<float, KREG, KX>(a.K, a.alpha, old_mean, old_std, xs, nm, ns);
#pragma unroll
        for (int r = 0; r < NR; ++r)
            if (KX > 0 || r < a.K) a.elites_next[(size_t)r * hd + e] = xs[r];
        if (!a.last) {
            a.mean_out[e] = nm;
            a.std_out[e] = ns;
        } else {
            new_mean[e] = nm;
        }
        if (e == tid) best0 = xs[0];
    };
    if (pre) {
#pragma unroll
        for (int i = 0; i < EPL; ++i) {
            const int e = tid + i * MERGE_WG;
            if (e < hd) finish_one(e, om[i], os[i]);
        }
    } else {
        for (int e = tid; e < hd; e += MERGE_WG) finish_one(e, a.mean[e], a.std[e]);
    }
    if (a.dbg && threadIdx.x == 0) a.dbg[5] = wall_clock64();
    if (tid < (KX > 0 ? KX : a.K)) a.elites_cost_next[tid] = key_cost(sel[tid]);
    if (a.last) {
        __syncthreads();
        if (pre) {   // (the bounds are in registers: request_bounds; the loop below is the same epilogue for hd > EPL * MERGE_WG)
#pragma unroll
            for (int i = 0; i < EPL; ++i) {
                const int e = tid + i * MERGE_WG;
                if (e < hd) {
                    a.mean_out[e] = (e + a.d < hd) ? new_mean[e + a.d] : new_mean[e];
                    a.std_out[e] = (bhi[i] - blo[i]) / 2.f * a.init_std;
                }
            }
        } else {
            for (int e = tid; e < hd; e += MERGE_WG) {
                const int j = e % a.d;
                a.mean_out[e] = (e + a.d < hd) ? new_mean[e + a.d] : new_mean[e];
                a.std_out[e] = (a.high[j] - a.low[j]) / 2.f * a.init_std;
            }
        }
        if (tid < a.d) a.executed[tid] = best0;   // rows[0][tid]: this thread gathered it (d <= hd: element tid is its first)
        if (tid == 0) a.best_cost[0] = key_cost(sel[0]);
    }
    if (a.dbg && threadIdx.x == 0) a.dbg[6] = wall_clock64();
}

template <int KREG, bool REC>
__global__ __launch_bounds__(MERGE_WG) void merge_single_kernel(MergeSingleArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    merge_single_body<KREG, REC>(a, smem_raw);
}

// ... for K == KX known at compile time (launch_merge_single picks it where a.K == KX): the same body, a name of its own
template <int KREG, int KX>
__global__ __launch_bounds__(MERGE_WG) void merge_single_exactk_kernel(MergeSingleArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    merge_single_body<KREG, false, KX>(a, smem_raw);
}

// The last merge of an MPC step with company (noise-ahead pipeline, plan.hip): workgroup 0 is merge_single_kernel, the
// other workgroups draw raw colored noise (noise_rows_kernel's work: sample_row into an LDS tile, coalesced copy-out) for
// iteration 0 of the NEXT MPC step -- the one launch of a step during which 255 of the 256 CUs had nothing to do.
// (KX > 0: workgroup 0 is the exact-K merge -- merge_noise_exactk_kernel below, the same body under a name of its own)
template <int H, int KREG, int KX>
__device__ __forceinline__ void merge_noise_body(const MergeSingleArgs& a, const FastSampleArgs& z1, const FastSampleArgs& z2, int wgs1,
                                                 unsigned char* smem_raw) {
    if (blockIdx.x == 0) {
        merge_single_body<KREG, false, KX>(a, smem_raw);
        return;
    }
    // workgroups 1 .. wgs1: the sampling call z1; behind them: z2 (a few rows of another stream)
    const bool second = (int)blockIdx.x > wgs1;
    const FastSampleArgs& z = second ? z2 : z1;
    float* tile = reinterpret_cast<float*>(smem_raw);
    const int d = z.d, hd = H * d, tpw = MERGE_WG / d, tid = threadIdx.x;
    const int n_base = ((int)blockIdx.x - 1 - (second ? wgs1 : 0)) * tpw;
    const int n_here = cmin(tpw, z.n - n_base);
    if (tid < n_here * d) {
        const int nl = tid / d;
        const int j = tid - nl * d;
        float* trow = tile + nl * hd + j;
        sample_row<H, 10>(z.W, (unsigned)(z.first_index + n_base + nl), (unsigned)j, z.off_lo, z.off_hi, z.seed_lo, z.seed_hi,
                          [&](int t, float y) { trow[t * d] = y; }, z.white != 0);
    }
    __syncthreads();
    float* gdst = z.out + (size_t)n_base * hd;
    const int total = n_here * hd;
    if ((hd & 3) == 0) {
        const float4* t4 = reinterpret_cast<const float4*>(tile);
        float4* g4 = reinterpret_cast<float4*>(gdst);
        for (int e = tid; e < total / 4; e += MERGE_WG) g4[e] = t4[e];
    } else {
        for (int e = tid; e < total; e += MERGE_WG) gdst[e] = tile[e];
    }
}
template <int H, int KREG>
__global__ __launch_bounds__(MERGE_WG) void merge_noise_kernel(MergeSingleArgs a, FastSampleArgs z1, FastSampleArgs z2, int wgs1) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    merge_noise_body<H, KREG, 0>(a, z1, z2, wgs1, smem_raw);
}
template <int H, int KREG, int KX>
__global__ __launch_bounds__(MERGE_WG) void merge_noise_exactk_kernel(MergeSingleArgs a, FastSampleArgs z1, FastSampleArgs z2, int wgs1) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    merge_noise_body<H, KREG, KX>(a, z1, z2, wgs1, smem_raw);
}

// The same launch for B problems at once (icem_plan_step_batch): blockIdx.y = the problem, its arguments in device memory,
// the noise calls' stream offsets relative to the step's base of that problem.  z1.n == 0 for every problem: merge only.
template <int H, int KREG>
__global__ __launch_bounds__(MERGE_WG) void merge_noise_batch_kernel(const MergeNoiseBatchArgs* __restrict__ args, BatchBases bases, int wgs1) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const MergeNoiseBatchArgs& g = args[blockIdx.y];
    if (blockIdx.x == 0) {
        const MergeSingleArgs a = from_device(g.a);
        merge_single_body<KREG, false>(a, smem_raw);
        return;
    }
    const bool second = (int)blockIdx.x > wgs1;
    const FastSampleArgs z = from_device(second ? g.z2 : g.z1);
    float* tile = reinterpret_cast<float*>(smem_raw);
    const int d = z.d, hd = H * d, tpw = MERGE_WG / d, tid = threadIdx.x;
    const int n_base = ((int)blockIdx.x - 1 - (second ? wgs1 : 0)) * tpw;
    const int n_here = cmin(tpw, z.n - n_base);
    if (n_here <= 0) return;
    uint32_t off_lo = z.off_lo, off_hi = z.off_hi;
    add_base64(off_lo, off_hi, bases.v[blockIdx.y]);
    if (tid < n_here * d) {
        const int nl = tid / d;
        const int j = tid - nl * d;
        float* trow = tile + nl * hd + j;
        sample_row<H, 10>(z.W, (unsigned)(z.first_index + n_base + nl), (unsigned)j, off_lo, off_hi, z.seed_lo, z.seed_hi,
                          [&](int t, float y) { trow[t * d] = y; }, z.white != 0);
    }
    __syncthreads();
    float* gdst = z.out + (size_t)n_base * hd;
    const int total = n_here * hd;
    if ((hd & 3) == 0) {
        const float4* t4 = reinterpret_cast<const float4*>(tile);
        float4* g4 = reinterpret_cast<float4*>(gdst);
        for (int e = tid; e < total / 4; e += MERGE_WG) g4[e] = t4[e];
    } else {
        for (int e = tid; e < total; e += MERGE_WG) gdst[e] = tile[e];
    }
}

// Sharded runs: this rank's K best candidates (same selection) packed as records (pack_records_body) -- a launch of
// its own where the pack cannot ride in the next iteration's launch (sample_rollout_kernel's workgroup 0).
// bytes of LDS the pack kernel may use to stage the K records for the push (larger records: separate push launch)
constexpr size_t PACK_STAGE_MAX = 48 * 1024;

template <int KREG>
__global__ __launch_bounds__(MERGE_WG) void pack_records_kernel(MergeSingleArgs a, int n_loc, int shard_lo, float* records, XchgPush px) {
    __shared__ unsigned long long sel[64];
    __shared__ unsigned long long cand[64];
    extern __shared__ __attribute__((aligned(16))) float stage[];  // [K, rs] when the kernel also pushes
    const int tid = threadIdx.x;
    if (tid < 64) merge_select<KREG>(a, tid, cand, sel);
    __syncthreads();
    pack_records_body<KREG>(a, n_loc, shard_lo, records, px, stage, sel, tid, MERGE_WG);
}

// ... and the step's LAST pack together with the records merge that waits for it (sharded runs): one launch instead of two
// one-workgroup launches back to back -- pack + push, then the wait for every rank's flag, selection over the gathered
// records, refit and the epilogue.  The dynamic LDS is the pack's stage first, the merge's new mean afterwards.
template <int KREG>
__global__ __launch_bounds__(MERGE_WG) void pack_merge_kernel(MergeSingleArgs pk, int n_loc, int shard_lo, float* records, XchgPush px,
                                                               MergeSingleArgs m) {
    __shared__ unsigned long long sel[64];
    __shared__ unsigned long long cand[64];
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int tid = threadIdx.x;
    if (tid < 64) merge_select<KREG>(pk, tid, cand, sel);
    __syncthreads();
    pack_records_body<KREG>(pk, n_loc, shard_lo, records, px, reinterpret_cast<float*>(smem_raw), sel, tid, MERGE_WG);
    __syncthreads();
    merge_single_body<KREG, true>(m, smem_raw);
}

// icem_topk_sorted for small f32 pools (the stage-wise controller paths: learned dynamics, host models, the CEM
// baselines) in ONE launch of one workgroup instead of the generic partial + final pair (12.4 + 9.2 us at n = 1 024):
// every wave keeps a running sorted top-K over its 64-key batches (batch sort, running list parked in lanes 32.., one
// more sort), the 16 lists meet in wg_merge_emit's tree.  Same keys as everywhere: (cost, index) order, NaN = +inf,
// (+inf, INT_MAX) padding behind the n real entries.
__global__ __launch_bounds__(1024) void topk_small_kernel(const float* costs, int n, int K, float* out_c, int* out_i) {
    __shared__ unsigned long long wg_keys[2][16][32];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long run = KEY_SENTINEL;
    bool first = true;
    for (int base = wave * 64; base < n; base += 1024) {
        const int i = base + lane;
        unsigned long long key = wave_sort64(i < n ? make_key(costs[i], i) : KEY_SENTINEL, lane);
        if (!first) {
            const unsigned long long prev = __shfl(run, lane - 32, 64);
            key = (lane >= 32 && lane < 32 + K) ? prev : (lane < K ? key : KEY_SENTINEL);
            key = wave_sort64(key, lane);
        }
        run = key;
        first = false;
    }
    FastRolloutArgs fr{};  // wg_merge_emit only looks at the candidate outputs: list 0 of 1 = the result
    fr.part_c = out_c;
    fr.part_i = out_i;
    wg_merge_emit<16>(wg_keys, run, K, lane, wave, fr, 0, 1);
}

// icem_update_distribution: update_small_body.h (the body is shared with the f32 update kernel of icem_plan_step_cem, k_cem.hip)
__global__ __launch_bounds__(1024) void update_small_kernel(UpdateSmallArgs a) {
    update_small_body<false>(a, nullptr);
}

// B problems in one launch (icem_plan_step_learned*): one workgroup per problem, its argument block in device memory; the
// step's last update carries the epilogue
template <bool FINISH>
__global__ __launch_bounds__(1024) void update_small_batch_kernel(const UpdateFinishArgs* __restrict__ args) {
    const UpdateFinishArgs g = args[blockIdx.x];
    update_small_body<FINISH>(g.u, &g);
}

// ... with the pool's costs still in the members' rows (icem_plan_step_learned_models): the same body, its keys out of the
// members' reduction (MemberCosts, update_small_body.h) -- the launch that reduced them first is gone
template <bool FINISH>
__global__ __launch_bounds__(1024) void update_small_members_batch_kernel(const UpdateMembersArgs* __restrict__ args) {
    const UpdateMembersArgs g = args[blockIdx.x];
    update_small_body<FINISH>(g.f.u, &g.f, MemberCosts{g.member_costs + g.row0, g.costs, (unsigned)g.stride, g.members, g.reduce, g.inv});
}

}  // namespace

void launch_update_small(const UpdateSmallArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(update_small_kernel, dim3(1), dim3(1024), 0, st, a);
}

void launch_update_small_batch(const UpdateFinishArgs* args_dev, int n, bool finish, hipStream_t st) {
    if (finish) hipLaunchKernelGGL(update_small_batch_kernel<true>, dim3(n), dim3(1024), 0, st, args_dev);
    else hipLaunchKernelGGL(update_small_batch_kernel<false>, dim3(n), dim3(1024), 0, st, args_dev);
}

void launch_update_small_members_batch(const UpdateMembersArgs* args_dev, int n, bool finish, hipStream_t st) {
    if (finish) hipLaunchKernelGGL(update_small_members_batch_kernel<true>, dim3(n), dim3(1024), 0, st, args_dev);
    else hipLaunchKernelGGL(update_small_members_batch_kernel<false>, dim3(n), dim3(1024), 0, st, args_dev);
}

bool topk_small_ok(int n, int K) { return n >= 1 && n <= 16384 && K >= 1 && K <= 32; }

void launch_topk_small(const float* costs, int n, int K, float* out_c, int* out_i, hipStream_t st) {
    hipLaunchKernelGGL(topk_small_kernel, dim3(1), dim3(1024), 0, st, costs, n, K, out_c, out_i);
}

bool pack_can_push(int K, int h, int d) { return (size_t)K * (h * d + 2) * sizeof(float) <= PACK_STAGE_MAX; }

void launch_pack_records(const MergeSingleArgs& a, int n_loc, int shard_lo, float* records, hipStream_t st, const XchgPush& px) {
    const size_t lds = px.peers ? (size_t)a.K * (a.h * a.d + 2) * sizeof(float) : 0;
    if (a.K + 1 <= 12)
        hipLaunchKernelGGL((pack_records_kernel<12>), dim3(1), dim3(MERGE_WG), lds, st, a, n_loc, shard_lo, records, px);
    else
        hipLaunchKernelGGL((pack_records_kernel<34>), dim3(1), dim3(MERGE_WG), lds, st, a, n_loc, shard_lo, records, px);
}

void launch_pack_merge(const MergeSingleArgs& pk, int n_loc, int shard_lo, float* records, const XchgPush& px, const MergeSingleArgs& m,
                       hipStream_t st) {
    const size_t lds = std::max(px.peers ? (size_t)pk.K * (pk.h * pk.d + 2) : (size_t)0, (size_t)m.h * m.d) * sizeof(float);
    if (pk.K + 1 <= 12)
        hipLaunchKernelGGL((pack_merge_kernel<12>), dim3(1), dim3(MERGE_WG), lds, st, pk, n_loc, shard_lo, records, px, m);
    else
        hipLaunchKernelGGL((pack_merge_kernel<34>), dim3(1), dim3(MERGE_WG), lds, st, pk, n_loc, shard_lo, records, px, m);
}

// lists form, K <= 11, default generator, a compiled sampler horizon (else: launch_merge_single + launch_noise_rows)
bool merge_noise_ok(const MergeSingleArgs& a, int rounds) {
    return a.records == nullptr && a.K + 1 <= 12 && rounds == 10 && fast_sample_supported(a.h, a.d);
}

// The last merge's launch, alone (wgs = {1, 0, 0}) or with noise workgroups beside it: key, and the one table of
// merge_noise_kernel / merge_noise_batch_kernel -- the key's horizon -> `f(H, grid, lds)`; false: not a compiled horizon
static LaunchKey merge_key(const MergeSingleArgs& a, const FastSampleArgs* z, const FastSampleArgs* z2) {
    LaunchKey k;
    k.family = LAUNCH_MERGE_NOISE;
    k.h = a.h, k.d = a.d, k.form = z ? 1 : 0;
    k.wgs[0] = 1;
    if (z) {
        const int tpw = MERGE_WG / z->d;
        k.wgs[1] = (z->n + tpw - 1) / tpw;
        k.wgs[2] = z2->n > 0 ? (z2->n + tpw - 1) / tpw : 0;
    }
    return k;
}
template <class F>
static bool merge_noise_dispatch(const LaunchKey& k, F&& f) {
    // workgroup 0 holds the new mean, a noise workgroup its [tpw, h, d] tile
    const size_t lds = std::max((size_t)k.h * k.d, k.form ? (size_t)(MERGE_WG / k.d) * k.h * k.d : (size_t)0) * sizeof(float);
    const int grid = k.wgs[0] + k.wgs[1] + k.wgs[2];
#define X(HH) \
    if (k.h == HH) return f(std::integral_constant<int, HH>{}, grid, lds), true;
    ICEM_FAST_HORIZONS(X)
#undef X
    return false;
}

void launch_merge_noise(const LaunchCtx& cx, const MergeSingleArgs& a, const FastSampleArgs& z, const FastSampleArgs& z2) {
    const LaunchKey k = merge_key(a, &z, &z2);
    submit(cx, k, true, [&](void* dst, unsigned long long base) { batch_form(a, &z, &z2, base, dst); }, [&] {
        merge_noise_dispatch(k, [&](auto H, int grid, size_t lds) {
            if (a.K == MERGE_EXACT_K && opt_i(OPT_MERGE_EXACT_K) != 0)
                hipLaunchKernelGGL((merge_noise_exactk_kernel<decltype(H)::value, 12, MERGE_EXACT_K>), dim3(grid), dim3(MERGE_WG), lds, cx.st, a, z, z2, k.wgs[1]);
            else
                hipLaunchKernelGGL((merge_noise_kernel<decltype(H)::value, 12>), dim3(grid), dim3(MERGE_WG), lds, cx.st, a, z, z2, k.wgs[1]);
        });
    });
}

// n problems' last merges (+ the next step's first noise) in one launch; the lists form with K <= 11 only
void launch_merge_batch(const LaunchKey& k, const MergeNoiseBatchArgs* args_dev, const BatchBases& bases, int n, hipStream_t st) {
    merge_noise_dispatch(k, [&](auto H, int grid, size_t lds) {
        hipLaunchKernelGGL((merge_noise_batch_kernel<decltype(H)::value, 12>), dim3(grid, n), dim3(MERGE_WG), lds, st, args_dev, bases, k.wgs[1]);
    });
}

// (alone, a solo step's merge is merge_single_kernel; a batch's is merge_noise_batch_kernel without noise workgroups)
void launch_merge_single(const LaunchCtx& cx, const MergeSingleArgs& a) {
    const LaunchKey k = merge_key(a, nullptr, nullptr);
    submit(cx, k, !a.records && a.K + 1 <= 12, [&](void* dst, unsigned long long base) { batch_form(a, nullptr, nullptr, base, dst); }, [&] {
        const size_t lds = (size_t)a.h * a.d * sizeof(float);
        if (a.records) {
            if (a.K + 1 <= 12)
                hipLaunchKernelGGL((merge_single_kernel<12, true>), dim3(1), dim3(MERGE_WG), lds, cx.st, a);
            else
                hipLaunchKernelGGL((merge_single_kernel<34, true>), dim3(1), dim3(MERGE_WG), lds, cx.st, a);
        } else if (a.K == MERGE_EXACT_K && opt_i(OPT_MERGE_EXACT_K) != 0) {
            hipLaunchKernelGGL((merge_single_exactk_kernel<12, MERGE_EXACT_K>), dim3(1), dim3(MERGE_WG), lds, cx.st, a);
        } else if (a.K + 1 <= 12) {
            hipLaunchKernelGGL((merge_single_kernel<12, false>), dim3(1), dim3(MERGE_WG), lds, cx.st, a);
        } else {
            hipLaunchKernelGGL((merge_single_kernel<34, false>), dim3(1), dim3(MERGE_WG), lds, cx.st, a);
        }
    });
}

}  // namespace icem
