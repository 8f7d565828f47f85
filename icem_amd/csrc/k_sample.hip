// k_sample.hip -- K1 for populations too large for the single-launch kernel.
// sample_folded_kernel<H, ROUNDS>: one thread per (trajectory, action-dim) row: per-row stream -> Box-Muller -> the h
//   white draws in registers; inverse real DFT folded on its cos/sin symmetry with the table rows as wave-uniform
//   scalar operands; affine (mean / std staged in LDS) + clip; samples parked in an LDS tile laid out like the
//   [n, h, d] output so the slab leaves as coalesced stores.
// sample_folded_merge_kernel: the same with the PREVIOUS iteration's top-K selection + refit in its prologue; in sharded
//   runs (records variant) workgroup 0 can be the previous iteration's record pack + push ("riding pack") and run the
//   launch's one records merge for everybody ("published merge"): DESIGN.md section 6.
#include "fused_dev.h"

namespace icem {

namespace {

// (the body of sample_folded_kernel and of sample_folded_batch_kernel: one device function, the same device code)
template <int H, int ROUNDS>
__device__ __forceinline__ void sample_folded_body(const FastSampleArgs& a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int d = a.d;
    const int hd = H * d;
    const int tpw = SWG / d;
    float* ms = smem;            // mean | std
    float* tile = smem + 2 * hd;  // [tpw, hd]
    const int tid = threadIdx.x;
    // mean / std are requested now and parked in LDS BEHIND the draws: the generator -- 60 % of a row's instructions --
    // needs neither, so the cold round trip of these loads hides under it instead of standing in front of it
    float mreg[2], sreg[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int e = tid + i * SWG;
        mreg[i] = a.mean[e < hd ? e : 0];
        sreg[i] = a.std[e < hd ? e : 0];
    }
    const int n_base = blockIdx.x * tpw;
    const int n_here = cmin(tpw, a.n - n_base);
    const bool shift_wg = a.n_shift > 0 && blockIdx.x == gridDim.x - 1;
    const bool has_row = !shift_wg && tid < n_here * d;
    const int nl = tid / d;
    const int j = tid - nl * d;
    const float lo = a.low[j < d ? j : 0], hi = a.high[j < d ? j : 0];
    float g[HMAX];
    if (has_row)
        row_normals<H, ROUNDS>((unsigned)(a.first_index + n_base + nl), (unsigned)j, a.off_lo, a.off_hi, a.seed_lo, a.seed_hi, g);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int e = tid + i * SWG;
        if (e < hd) {
            ms[e] = mreg[i];
            ms[hd + e] = sreg[i];
        }
    }
    for (int e = tid + 2 * SWG; e < hd; e += SWG) {
        ms[e] = a.mean[e];
        ms[hd + e] = a.std[e];
    }
    __syncthreads();
    if (shift_wg) {
        // the extra workgroup: shifted elites.  Row (e, j) keeps elites[e, 1:, j] and draws its last action
        // from the full (n_shift, d, h) noise batch of stream off2 (only t = h-1 is used, icem.py:102)
        if (tid < a.n_shift * d) {
            const int e = tid / d;
            const int js = tid - e * d;
            const float los = a.low[js], his = a.high[js];
            float last = 0.f;
            sample_row<H, ROUNDS>(a.W, (unsigned)e, (unsigned)js, a.off2_lo, a.off2_hi, a.seed_lo, a.seed_hi,
                                  [&](int t, float y) {
                                      if (t == H - 1) {
                                          float v = __builtin_fmaf(y, ms[hd + t * d + js], ms[t * d + js]);
                                          v = v < los ? los : v;
                                          last = v > his ? his : v;
                                      }
                                  }, a.white != 0);
            float* dst = a.out + (size_t)(a.n + e) * hd + js;
            const float* src = a.elites_src + (size_t)e * hd + js;
            for (int t = 0; t < H - 1; ++t) dst[t * d] = src[(t + 1) * d];
            dst[(H - 1) * d] = last;
        }
        return;
    }
    if (has_row) {
        float* trow = tile + nl * hd + j;
        const float* mrow = ms + j;
        row_synth<H>(a.W, g, [&](int t, float y) {
            const float v = __builtin_fmaf(y, mrow[hd + t * d], mrow[t * d]);
            trow[t * d] = __builtin_amdgcn_fmed3f(v, lo, hi);  // clip in one v_med3_f32
        }, a.white != 0);
    }
    __syncthreads();
    if (a.row0_mean && a.first_index + n_base == 0) {  // icem.py:87-88
        for (int e = tid; e < hd; e += SWG) tile[e] = ms[e];
        __syncthreads();
    }
    float* gdst = a.out + (size_t)n_base * hd;
    const int total = n_here * hd;
    if ((hd & 3) == 0) {
        const float4* t4 = reinterpret_cast<const float4*>(tile);
        float4* g4 = reinterpret_cast<float4*>(gdst);
        for (int e = tid; e < total / 4; e += SWG) g4[e] = t4[e];
    } else {
        for (int e = tid; e < total; e += SWG) gdst[e] = tile[e];
    }
}

template <int H, int ROUNDS>
__global__ __launch_bounds__(SWG) void sample_folded_kernel(FastSampleArgs a) {
    sample_folded_body<H, ROUNDS>(a);
}

// B problems in one launch (icem_plan_step_batch's two-kernel iterations of the TileHN shapes; icem_plan_step_learned*):
// blockIdx.y = the problem, its argument block in device memory (scalar loads: the index is uniform), the sampling calls'
// stream offsets stored relative to the step's base of that problem (BatchBases; the second offset is unused where
// n_shift == 0).  The grid's x extent is the largest problem's: a workgroup beyond its problem's rows that is not its shift
// workgroup (the launch's last, n_shift > 0) exits.  CONTRACT: ragged row counts require n_shift == 0 in every block -- else the
// last workgroup of a smaller problem would be a row workgroup and the shift workgroup at once (icem_plan_step_batch's problems
// have equal LaunchKeys, so equal row counts; the learned step's shifted elites are a launch of their own).  og.dst != nullptr:
// workgroup 0 of a problem also copies its observation into the batch's contiguous [n, og.width] array.
template <int H, int ROUNDS>
__global__ __launch_bounds__(SWG) void sample_folded_batch_kernel(const FastSampleArgs* __restrict__ args, BatchBases bases, ObsGather og) {
    FastSampleArgs s = from_device(args[blockIdx.y]);
    if (og.dst != nullptr && blockIdx.x == 0) {
        const float* src = og.src[blockIdx.y];
        for (int e = threadIdx.x; e < og.width; e += SWG) og.dst[(size_t)blockIdx.y * og.width + e] = src[e];
    }
    const bool shift_wg = s.n_shift > 0 && blockIdx.x == gridDim.x - 1;
    if ((int)blockIdx.x * (SWG / s.d) >= s.n && !shift_wg) return;
    const unsigned long long base = bases.v[blockIdx.y];
    add_base64(s.off_lo, s.off_hi, base);
    add_base64(s.off2_lo, s.off2_hi, base);
    sample_folded_body<H, ROUNDS>(s);
}

// -------------------------------------------------------------------------------------------------
// K1 without the distribution ("noise ahead"): the raw colored samples y [n, h, d] of one sampling call
// -------------------------------------------------------------------------------------------------
// powerlaw_psd_gaussian itself (icem.py:73-75) -- 95 % of the sampler's instructions -- needs only (seed, call offset,
// global row): it runs on a second stream while the PREVIOUS iteration's rollout is still busy, and the rollout of
// this iteration applies `* std + mean` and the clip to every vector it loads (Stream16::run_xf).  Same sample_row, so
// the same y; no mean / std staging, no shifted-elite workgroup.
// DT: the action dimension as a compile-time constant for the benchmark shapes (the tile offsets of the 30 stores of a
// row become immediates, the row / dimension split a constant division), 0 = run-time d.
template <int H, int ROUNDS, int DT>
__global__ __launch_bounds__(SWG) void noise_rows_kernel(FastSampleArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int d = DT > 0 ? DT : a.d;
    const int hd = H * d;
    const int tpw = SWG / d;
    float* tile = smem;  // [tpw, hd]
    const int tid = threadIdx.x;
    const int n_base = blockIdx.x * tpw;
    const int n_here = cmin(tpw, a.n - n_base);
    if (tid < n_here * d) {
        const int nl = tid / d;
        const int j = tid - nl * d;
        float* trow = tile + nl * hd + j;
        sample_row<H, ROUNDS>(a.W, (unsigned)(a.first_index + n_base + nl), (unsigned)j, a.off_lo, a.off_hi, a.seed_lo,
                              a.seed_hi, [&](int t, float y) { trow[t * d] = y; }, a.white != 0);
    }
    __syncthreads();
    float* gdst = a.out + (size_t)n_base * hd;
    const int total = n_here * hd;
    if ((hd & 3) == 0) {
        const float4* t4 = reinterpret_cast<const float4*>(tile);
        float4* g4 = reinterpret_cast<float4*>(gdst);
        for (int e = tid; e < total / 4; e += SWG) g4[e] = t4[e];
    } else {
        for (int e = tid; e < total; e += SWG) gdst[e] = tile[e];
    }
}

// -------------------------------------------------------------------------------------------------
// K1 with the PREVIOUS iteration's K3 + K4 in its prologue (populations too large for the single-launch kernel)
// -------------------------------------------------------------------------------------------------
// sample_folded_kernel plus one wavefront per workgroup that runs the low-register selection
// (merge_select_stream) on the previous iteration's candidate lists while the 4 sampling waves draw their noise
// into the LDS tile; then all 5 waves gather the K elite rows and refit, the affine map + clip is applied to the
// tile and the tile leaves as before.  Every workgroup redoes the same merge (L2 serves the 20 KB of keys and 7 KB
// of elite rows), workgroup 0 publishes it.  Saves the merge launch (8.6 + 2.6 us) for ~3 us more sampler time.
// (the body of sample_folded_merge_kernel and of sample_folded_merge_batch_kernel)
template <int H, int ROUNDS, int KREG, bool REC>
__device__ __forceinline__ void sample_folded_merge_body(const FastSampleArgs& a, const MergeSingleArgs& m, const PackPrev& p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    __shared__ unsigned long long sel[64];
    __shared__ unsigned long long cand[64];
    __shared__ int slot[64];
    constexpr int NTT = SWG + 64;
    const int d = a.d;
    const int hd = H * d;
    const int tpw = SWG / d;
    float* ms = smem;            // mean | std (computed here)
    float* tile = smem + 2 * hd;  // [tpw, hd]
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    // riding pack (sharded runs, PackPrev): workgroup 0 packs + pushes the previous iteration's records while the others
    // draw their noise; the launch has one workgroup more
    const bool has_pack = REC && p.part_k != nullptr;
    if constexpr (REC) {
        if (has_pack && blockIdx.x == 0) {
            MergeSingleArgs pk{};
            pk.n_lists = p.n_lists;
            pk.n_pool = p.n_pool;
            pk.n_global = p.n_global;
            pk.K = p.K;
            pk.h = H;
            pk.d = d;
            pk.part_k = p.part_k;
            pk.actions = p.actions;
            pk.n_keep = p.n_keep;
            pk.elites_cost_cur = p.keep_costs;
            pk.keep_base = p.n_loc;
            // everybody else's prologue waits for this workgroup's push: its waves go first on their SIMDs
            __builtin_amdgcn_s_setprio(3);
            if (tid >= SWG) merge_select_shallow<3>(pk, lane, cand, sel);
            __syncthreads();
            pack_records_body<KREG>(pk, p.n_loc, p.shard_lo, p.records, p.px, smem, sel, tid, NTT);
            if (p.pub != nullptr) {
                // Published merge: this workgroup also runs THE merge of the launch -- waits for every rank's records,
                // selects, gathers, refits -- and publishes the new mean | std to all the others (written through: the
                // XCDs' L2s are not coherent inside a launch; then one agent-scope flag).  Hundreds of workgroups each
                // reading the same 7 KB of records from uncached memory was the slowest part of this launch.
                __syncthreads();
                merge_select_records_wg(m, tid >= SWG, lane, tid, NTT, sel, slot);
                const float* rows[KREG];
                merge_rows<KREG, true>(m, sel, slot, rows);
                for (int e = tid; e < hd; e += NTT) {
                    float xs[KREG];
#pragma unroll
                    for (int r = 0; r < KREG; ++r) xs[r] = rows[r][e];
                    float nm, ns;
                    refit_element_regs<float, KREG>(m.K, m.alpha, m.mean[e], m.std[e], xs, nm, ns);
                    __hip_atomic_store(p.pub + e, nm, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    __hip_atomic_store(p.pub + hd + e, ns, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    m.mean_out[e] = nm;
                    m.std_out[e] = ns;
#pragma unroll
                    for (int r = 0; r < KREG; ++r)
                        if (r < m.K) m.elites_next[(size_t)r * hd + e] = xs[r];
                }
                if (tid < m.K) m.elites_cost_next[tid] = key_cost(sel[tid]);
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __syncthreads();
                if (tid == 0) __hip_atomic_store(p.pub_flag, p.pub_seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            return;
        }
    }
    const bool published = REC && has_pack && p.pub != nullptr;
    const int wg = blockIdx.x - (has_pack ? 1 : 0);
    const int n_base = wg * tpw;
    const int n_here = cmin(tpw, a.n - n_base);
    const bool has_row = tid < n_here * d;
    const int nl = tid / d;
    const int j = tid - nl * d;
    float* trow = tile + nl * hd + j;
    if (tid >= SWG) {
        if (published) {  // workgroup 0 merges for everybody: wait for its flag (bounded like every exchange wait)
            unsigned polls = 0;
            while (__hip_atomic_load(p.pub_flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != p.pub_seq &&
                   ++polls <= m.xw.max_polls)
                __builtin_amdgcn_s_sleep(16);
            if (polls > m.xw.max_polls && lane == 0 && m.xw.status)
                __hip_atomic_store(m.xw.status, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        } else if constexpr (!REC) {
            merge_select_shallow<3>(m, lane, cand, sel);
        }
    } else if (has_row) {
        sample_row<H, ROUNDS>(a.W, (unsigned)(a.first_index + n_base + nl), (unsigned)j, a.off_lo, a.off_hi, a.seed_lo,
                              a.seed_hi, [&](int t, float y) { trow[t * d] = y; }, a.white != 0);
    }
    if (REC && !published) merge_select_records_wg(m, tid >= SWG, lane, tid, NTT, sel, slot);   // (the records' keys ranked by all threads)
    else __syncthreads();
    if (published) {
        for (int e = tid; e < 2 * hd; e += NTT) ms[e] = __hip_atomic_load(p.pub + e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else {
        const float* rows[KREG];
        merge_rows<KREG, REC>(m, sel, slot, rows);
        for (int e = tid; e < hd; e += NTT) {
            float xs[KREG];
#pragma unroll
            for (int r = 0; r < KREG; ++r) xs[r] = rows[r][e];
            float nm, ns;
            refit_element_regs<float, KREG>(m.K, m.alpha, m.mean[e], m.std[e], xs, nm, ns);
            ms[e] = nm;
            ms[hd + e] = ns;
            if (wg == 0) {
                m.mean_out[e] = nm;
                m.std_out[e] = ns;
#pragma unroll
                for (int r = 0; r < KREG; ++r)
                    if (r < m.K) m.elites_next[(size_t)r * hd + e] = xs[r];
            }
        }
        if (wg == 0 && tid < m.K) m.elites_cost_next[tid] = key_cost(sel[tid]);
    }
    __syncthreads();
    if (has_row) {
        const float lo = a.low[j], hi = a.high[j];
        const float* mrow = ms + j;
        for (int t = 0; t < H; ++t) {
            const float v = __builtin_fmaf(trow[t * d], mrow[hd + t * d], mrow[t * d]);
            trow[t * d] = __builtin_amdgcn_fmed3f(v, lo, hi);
        }
    }
    __syncthreads();
    if (a.row0_mean && a.first_index + n_base == 0) {  // icem.py:87-88
        for (int e = tid; e < hd; e += NTT) tile[e] = ms[e];
        __syncthreads();
    }
    float* gdst = a.out + (size_t)n_base * hd;
    const int total = n_here * hd;
    if ((hd & 3) == 0) {
        const float4* t4 = reinterpret_cast<const float4*>(tile);
        float4* g4 = reinterpret_cast<float4*>(gdst);
        for (int e = tid; e < total / 4; e += NTT) g4[e] = t4[e];
    } else {
        for (int e = tid; e < total; e += NTT) gdst[e] = tile[e];
    }
}

template <int H, int ROUNDS, int KREG, bool REC>
__global__ __launch_bounds__(SWG + 64) void sample_folded_merge_kernel(FastSampleMergeArgs args) {
    sample_folded_merge_body<H, ROUNDS, KREG, REC>(args.s, args.m, args.p);
}

// ... and for B problems (the lists merge: world 1, no riding pack -- the block's PackPrev is all zero)
template <int H, int ROUNDS, int KREG>
__global__ __launch_bounds__(SWG + 64) void sample_folded_merge_batch_kernel(const FastSampleMergeArgs* __restrict__ args, BatchBases bases) {
    const FastSampleMergeArgs& g = args[blockIdx.y];
    FastSampleArgs s = from_device(g.s);
    add_base64(s.off_lo, s.off_hi, bases.v[blockIdx.y]);
    const MergeSingleArgs m = from_device(g.m);
    sample_folded_merge_body<H, ROUNDS, KREG, false>(s, m, g.p);
}

}  // namespace

bool fast_sample_supported(int h, int d) {
    if (d > SWG) return false;
#define X(HH) \
    if (h == HH) return true;
    ICEM_FAST_HORIZONS(X)
#undef X
    return false;
}

// sampler with the previous iteration's merge in its prologue (default generator only, K <= 11, no shifted elites)
bool sample_folded_merge_ok(int h, int d, int rounds, int K) {
    const int on = opt_i(OPT_MERGE_PROLOGUE);
    return on && rounds == 10 && K + 1 <= 12 && fast_sample_supported(h, d);
}

bool sample_folded_pack_ok(int h, int d, int rounds, int K) {
    const int on = opt_i(OPT_RIDING_PACK);
    const int tpw = SWG / d;
    return on && sample_folded_merge_ok(h, d, rounds, K) && K * (h * d + 2) <= (2 + tpw) * h * d;
}

// horizons at which a recorded sampling launch has a batched form: what a batch of TileHN handles reaches (ICEM_HN_SHAPES are
// all h = 30), and what a batch of GEMM-kernel handles is admitted at (plan.hip: batch_ineligible).
// sample_folded_merge_batch_kernel is compiled for these only; sample_folded_batch_kernel for every horizon of the folded sampler
// (the learned step's), but icem_plan_step_batch records a sampler only where BOTH exist
#define ICEM_SAMPLE_BATCH_HORIZONS(X) X(30)
bool sample_batch_compiled(int h) {
#define X(HH) \
    if (h == HH) return true;
    ICEM_SAMPLE_BATCH_HORIZONS(X)
#undef X
    return false;
}
int sample_row_workgroups(int n, int d) { return (n + SWG / d - 1) / (SWG / d); }
static size_t sample_lds(int h, int d) { return ((size_t)2 * h * d + (size_t)(SWG / d) * h * d) * sizeof(float); }

void launch_sample_folded_merge(const LaunchCtx& cx, const FastSampleMergeArgs& a) {
    const int tpw = SWG / a.s.d;
    const bool pack = a.m.records && a.p.part_k;
    LaunchKey k;
    k.family = LAUNCH_SAMPLE_MERGE;
    k.h = a.s.h, k.d = a.s.d, k.form = a.m.records ? 2 : 1;
    k.wgs[0] = (a.s.n + tpw - 1) / tpw;
    k.wgs[1] = pack ? 1 : 0;   // + workgroup 0: the riding pack
    const int grid = k.wgs[0] + k.wgs[1];
    const size_t lds = sample_lds(a.s.h, a.s.d);
    hipStream_t st = cx.st;
    submit(cx, k, k.form == 1 && sample_batch_compiled(k.h), [&](void* dst, unsigned long long base) { batch_form(a, base, dst); }, [&] {
#define X(HH)                                                                                                  \
    if (a.s.h == HH) {                                                                                         \
        if (a.m.records)                                                                                       \
            hipLaunchKernelGGL((sample_folded_merge_kernel<HH, 10, 12, true>), dim3(grid), dim3(SWG + 64), lds, st, a);  \
        else                                                                                                   \
            hipLaunchKernelGGL((sample_folded_merge_kernel<HH, 10, 12, false>), dim3(grid), dim3(SWG + 64), lds, st, a); \
        return;                                                                                                \
    }
        ICEM_FAST_HORIZONS(X)
#undef X
    });
}

void launch_sample_merge_batch(const LaunchKey& k, const FastSampleMergeArgs* args_dev, const BatchBases& bases, int n, hipStream_t st) {
#define X(HH)                                                                                                                   \
    if (k.h == HH) {                                                                                                            \
        hipLaunchKernelGGL((sample_folded_merge_batch_kernel<HH, 10, 12>), dim3(k.wgs[0], n), dim3(SWG + 64), sample_lds(k.h, k.d), st, \
                           args_dev, bases);                                                                                    \
        return;                                                                                                                 \
    }
    ICEM_SAMPLE_BATCH_HORIZONS(X)
#undef X
}

void launch_noise_rows(const FastSampleArgs& a, int rounds, hipStream_t st) {
    if (a.n <= 0) return;
    const int tpw = SWG / a.d;
    const int grid = (a.n + tpw - 1) / tpw;
    // The LDS request also bounds how many of these workgroups a CU takes (the tile is 30 KB at d = 6: five would fit and
    // leave a rollout workgroup of the noise-ahead pipeline -- 37 KB -- no room): at least 40.5 KB, i.e. three per CU.
    const size_t min_lds = (size_t)((opt(OPT_AHEAD_NOISE_LDS_KB) >= 0.0 ? opt(OPT_AHEAD_NOISE_LDS_KB) : 40.5) * 1024.0);   // (option ahead_noise_lds_kb: development)
    const size_t lds = std::max((size_t)tpw * a.h * a.d * sizeof(float), min_lds);
#define XS(HH, DD, OO)                                                                                \
    if (a.h == HH && a.d == DD && rounds == 10) {                                                     \
        hipLaunchKernelGGL((noise_rows_kernel<HH, 10, DD>), dim3(grid), dim3(SWG), lds, st, a);       \
        return;                                                                                       \
    }
    ICEM_FAST_SHAPES(XS)
#undef XS
#define X(HH)                                                                                         \
    if (a.h == HH) {                                                                                  \
        if (rounds == 7)                                                                              \
            hipLaunchKernelGGL((noise_rows_kernel<HH, 7, 0>), dim3(grid), dim3(SWG), lds, st, a);     \
        else                                                                                          \
            hipLaunchKernelGGL((noise_rows_kernel<HH, 10, 0>), dim3(grid), dim3(SWG), lds, st, a);    \
        return;                                                                                       \
    }
    ICEM_FAST_HORIZONS(X)
#undef X
}

void launch_sample_folded(const LaunchCtx& cx, const FastSampleArgs& a, int rounds) {
    LaunchKey k;
    k.family = LAUNCH_SAMPLE;
    k.h = a.h, k.d = a.d, k.form = rounds;
    k.wgs[0] = sample_row_workgroups(a.n, a.d);
    k.wgs[1] = a.n_shift > 0 ? 1 : 0;   // the last workgroup: the shifted elites
    const int grid = k.wgs[0] + k.wgs[1];
    const size_t lds = sample_lds(a.h, a.d);
    hipStream_t st = cx.st;
    submit(cx, k, rounds == 10 && sample_batch_compiled(k.h), [&](void* dst, unsigned long long base) { batch_form(a, base, dst); }, [&] {
#define X(HH)                                                                                        \
    if (a.h == HH) {                                                                                 \
        if (rounds == 7)                                                                             \
            hipLaunchKernelGGL((sample_folded_kernel<HH, 7>), dim3(grid), dim3(SWG), lds, st, a);    \
        else                                                                                         \
            hipLaunchKernelGGL((sample_folded_kernel<HH, 10>), dim3(grid), dim3(SWG), lds, st, a);   \
        return;                                                                                      \
    }
        ICEM_FAST_HORIZONS(X)
#undef X
    });
}

void launch_sample_batch(const LaunchKey& k, const FastSampleArgs* args_dev, const BatchBases& bases, const ObsGather& og, int n, hipStream_t st) {
#define X(HH)                                                                                                                       \
    if (k.h == HH) {                                                                                                                \
        hipLaunchKernelGGL((sample_folded_batch_kernel<HH, 10>), dim3(k.wgs[0] + k.wgs[1], n), dim3(SWG), sample_lds(k.h, k.d), st, \
                           args_dev, bases, og);                                                                                    \
        return;                                                                                                                     \
    }
    ICEM_FAST_HORIZONS(X)
#undef X
}

}  // namespace icem
