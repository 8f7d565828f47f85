// k_rollout_ahead.hip -- the noise-ahead iteration launch (large populations, world == 1; plan.hip::plan_step_ahead): ONE launch
// per CEM iteration whose workgroups play different roles,
//   rollout  (the first `n_roll` workgroups)  rollout16_kernel's work (one wavefront per 16 trajectories on
//            v_mfma_f32_16x16x4_f32, Tile16 / Stream16 of fused_dev.h) on a pool that holds RAW colored noise: the PREVIOUS
//            iteration's K3 + K4 (top-K of its candidate lists, elite gather, refit; icem.py:194-211) in the prologue, the
//            selection shared by all waves (merge_select_split: nothing hides it here), then every vector a wave loads
//            becomes clip(y * std + mean) (icem.py:79) between the prefetch registers and its LDS staging buffer
//            (Stream16::run_xf).  The last iteration writes the actions back in place (the caller's pool); the others
//            leave the noise where it is and the NEXT prologue maps the K elite rows once more (MergeSingleArgs::n_raw);
//   noise    (the next `n_noise` workgroups)  the raw colored noise of the NEXT sampling call (iteration i + 1, or
//            iteration 0 of the next MPC step) into the next pool: powerlaw_psd_gaussian needs no distribution
//            (icem.py:73-79), so it runs beside the rollout whose waves leave half of every SIMD's registers free;
//   shift    (one more workgroup, iteration 0 of every MPC step but the first)  the shifted elites (icem.py:91-104,
//            131-137): built like the sampler's extra workgroup builds them, rolled out by the workgroup's first wave, and
//            handed to the merge through the cost array (its kept-elite slot), as the single-launch kernel's tail rows.
// All roles in one launch on ONE stream: no events, no second queue (the two-stream form of this pipeline lost 10-15 us
// per cross-stream wait; profiles/r03_noise_ahead_*).  Same operations in the same order as sample_folded(_merge)_kernel +
// rollout16_kernel, so the same bits in every buffer (tests: test_noise_ahead_pipeline_equals_the_default_path).
#include "fused_dev.h"

namespace icem {

namespace {

constexpr int AHEAD_KREG = 12;

// LDS of a workgroup (dynamic, one buffer overlaid by the three roles), in floats
template <int H, int D, int O, int KIND, int WAVES>
struct AheadLds {
    using Stream = Stream16<H, D, O, KIND>;   // (the staging layout is the same for every tile arithmetic)
    using T16 = Tile16<H, D, O, KIND>;
    static constexpr int HD = H * D, NT = 64 * WAVES;
    // rollout role
    static constexpr int STAGE = 0;                                   // [WAVES][STG]; the selection's scratch lies over it
    static constexpr int KEYS = STAGE + WAVES * Stream::STG + (WAVES * Stream::STG) % 2;   // u64 [2][WAVES][32]
    static constexpr int DIST = KEYS + 2 * (2 * WAVES * 32);          // [2 HD]
    static constexpr int OBS = DIST + 2 * HD + (2 * HD) % 4;          // [32]
    static constexpr int SEL = OBS + 32;                              // u64 [64]
    static constexpr int WSEL = SEL + 2 * 64;                         // u64 [WAVES * 16]: every wave's K best, the kept elites behind them
    static constexpr int SLOT = WSEL + 2 * WAVES * 16;                // int [64]
    static_assert(WSEL % 4 == 0, "wsel is read two keys at a time");
    static constexpr int ROLL_END = SLOT + 64;
    static_assert(WAVES * 64 * 2 <= WAVES * Stream::STG, "per-wave compaction scratch fits the staging buffers");
    // noise role: [tpw, HD] tile of NT / D rows
    static constexpr int TPW = NT / D;
    static constexpr int NOISE_END = TPW * HD;
    // shift role: mean | std, then a 16-row tile the first wave rolls out
    static constexpr int SH_DIST = 0;
    static constexpr int SH_TILE = 2 * HD + (2 * HD) % 4;
    static constexpr int SHIFT_END = SH_TILE + T16::SLACK + 16 * HD + T16::TAIL + 32;
    static constexpr int FLOATS = ROLL_END > NOISE_END ? (ROLL_END > SHIFT_END ? ROLL_END : SHIFT_END) : (NOISE_END > SHIFT_END ? NOISE_END : SHIFT_END);
};

// (at most 128 registers whatever the workgroup size: the rollout waves share their SIMDs with the noise role's.  96 -- a
//  fifth wave per SIMD -- spills 32 registers in the rollout role: measured 220 instead of 185 us per MPC step at N = 65 536)
// PM: 0 = no merge (iteration 0), 1 = lists merge in every rollout workgroup's prologue, 2 = sharded: pack role + published
// records merge
template <int H, int D, int O, int KIND, int WAVES, int PM, int ARITH>
__global__ __launch_bounds__(64 * WAVES) __attribute__((amdgpu_waves_per_eu(4, 8))) void iter_ahead_kernel(IterAheadArgs args) {
#include "iter_ahead_body.h"
}

// B problems in one launch (blockIdx.y): the block of problem y from device memory, its pointers re-read as global addresses
// (fused_dev.h: from_device), the noise calls' stream offsets stored relative to the step's base of that problem
template <int H, int D, int O, int KIND, int WAVES, int PM, int ARITH>
__global__ __launch_bounds__(64 * WAVES) __attribute__((amdgpu_waves_per_eu(4, 8))) void iter_ahead_batch_kernel(
    const IterAheadArgs* __restrict__ arr, BatchBases bases) {
    static_assert(PM != 2, "sharded launches are not batched");
    const IterAheadArgs& g = arr[blockIdx.y];
    IterAheadArgs args = g;
    args.r = from_device(g.r);
    args.m = from_device(g.m);
    args.z = from_device(g.z);
    args.s = from_device(g.s);
    args.pool = gptr(g.pool);
    args.mean = gptr(g.mean);
    args.std = gptr(g.std);
    const unsigned long long base = bases.v[blockIdx.y];
    add_base64(args.z.off_lo, args.z.off_hi, base);
    add_base64(args.s.off2_lo, args.s.off2_hi, base);
#include "iter_ahead_body.h"
}

// Launch shape of the rollout role: rollout16's (one 16-trajectory tile per wave while they fit, at most FAST_MAX_LISTS
// workgroups), but at most 8 wavefronts per workgroup -- two per SIMD, each taking its tiles one after the other: the
// rollout leaves half of every SIMD's registers (and 100 of the CU's 160 KB of LDS) to a noise workgroup beside it.
void ahead_shape(const BatchHint& bh, int n_rows, int* grid, int* waves) {
    r16_shape(n_rows, grid, waves);
    if (*waves > 8) *waves = 8;
    if (bh.mult > 1 && bh.ahead) {
        // a batch of `mult` problems of this size in one launch (icem_plan_step_batch): waves per workgroup as for all their rows
        // together, the rollout workgroups of ONE problem (blockIdx.y is the problem)
        int g_all, w_all;
        r16_shape(n_rows * bh.mult, &g_all, &w_all);
        *waves = std::max(*waves, std::min(w_all, 8));
        *grid = (std::max(1, (n_rows + 15) / 16) + *waves - 1) / *waves;
    }
}

// The one table of this launch: key -> compiled instantiation, handed to `f` as a tag that knows its two launches
// (workgroups per role: key.wgs); false: nothing compiled for this key.
template <int H, int D, int O, int KIND, int WAVES, int PM, int ARITH>
struct AheadInst {
    using L = AheadLds<H, D, O, KIND, WAVES>;
    static constexpr bool BATCHED = PM != 2;   // (sharded launches are not batched)
    static void solo(int grid, hipStream_t st, const IterAheadArgs& a) {
        hipLaunchKernelGGL((iter_ahead_kernel<H, D, O, KIND, WAVES, PM, ARITH>), dim3(grid), dim3(64 * WAVES), L::FLOATS * sizeof(float), st, a);
    }
    static void batch(int grid, int n, hipStream_t st, const IterAheadArgs* args_dev, const BatchBases& bases) {
        hipLaunchKernelGGL((iter_ahead_batch_kernel<H, D, O, KIND, WAVES, PM, ARITH>), dim3(grid, n), dim3(64 * WAVES), L::FLOATS * sizeof(float), st,
                           args_dev, bases);
    }
};
template <int H, int D, int O, int WAVES, class F>
bool iter_ahead_pick(const LaunchKey& k, F& f) {
    if (k.waves != WAVES) return false;
    auto with = [&](auto kind, auto arith) {
        constexpr int KK = decltype(kind)::value, AA = decltype(arith)::value;
        if (k.form == 2) f(AheadInst<H, D, O, KK, WAVES, 2, AA>{});
        else if (k.form) f(AheadInst<H, D, O, KK, WAVES, 1, AA>{});
        else f(AheadInst<H, D, O, KK, WAVES, 0, AA>{});
        return true;
    };
    using I0 = std::integral_constant<int, 0>;
    using I1 = std::integral_constant<int, 1>;
    if (k.arith == 1) return k.kind == 1 ? with(I1{}, I1{}) : with(I0{}, I1{});
    return k.kind == 1 ? with(I1{}, I0{}) : with(I0{}, I0{});
}
template <class F>
bool iter_ahead_dispatch(const LaunchKey& k, F&& f) {
#define XR(HH, DD, OO)                                                                                        \
    if constexpr (OO <= 20) {                                                                                 \
        if (k.h == HH && k.d == DD && k.O == OO) return iter_ahead_pick<HH, DD, OO, 4>(k, f) || iter_ahead_pick<HH, DD, OO, 8>(k, f); \
    }
    ICEM_FAST_SHAPES(XR)
#undef XR
    return false;
}

}  // namespace

// populations whose rollout launch has at least 4 waves per workgroup (more than 512 tiles): below that the
// single-launch kernel of k_iter_small.hip is the shorter chain
// ... and one-tile observation widths (O <= 20) only: with two output tiles (O = 24: 26 MFMAs and twice the state per
// step) the rollout role does not fit the 128 registers it shares its SIMDs on -- 112-158 spilled VGPRs, and the launch
// LOSES to the sampler + rollout16 pair: 236.1 vs 171.4 us per MPC step at N = 16 384 (d = 17, 3 iterations), 657.7 vs
// 473.7 at 65 536 (EXPERIMENTS.md R4.6).  Those shapes are not instantiated.
bool rollout_ahead_ok(const BatchHint& bh, int h, int d, int O, int K, int n_rows) {
    int grid, waves;
    r16_shape(n_rows * ((bh.mult > 1 && bh.ahead) ? bh.mult : 1), &grid, &waves);   // (a batch: the rows of all its problems fill the chip)
    return O <= 20 && K + 1 <= AHEAD_KREG && waves >= 4 && fast_rollout_supported(h, d, O, K) && fast_sample_supported(h, d);
}

int ahead_roll_workgroups(const BatchHint& bh, int n_rows) {
    int grid, waves;
    ahead_shape(bh, n_rows, &grid, &waves);
    return grid;
}

void launch_iter_ahead(const LaunchCtx& cx, const IterAheadArgs& a_in, int h, int d, int O, int kind) {
    IterAheadArgs a = a_in;
    LaunchKey k;
    ahead_shape(cx.hint, a.r.n_rows, &a.n_roll, &k.waves);
    const int tpw = (64 * k.waves) / d;   // (AheadLds::TPW: rows of noise per workgroup)
    a.n_noise = a.z.n > 0 ? (a.z.n + tpw - 1) / tpw : 0;
    k.family = LAUNCH_ITER_AHEAD;
    k.h = h, k.d = d, k.O = O, k.kind = kind, k.arith = a.r.arith, k.form = a.has_merge;
    k.wgs[0] = a.n_roll, k.wgs[1] = a.n_noise, k.wgs[2] = (a.s.n_shift > 0 ? 1 : 0) + (a.has_merge == 2 ? 1 : 0);
    const bool compiled = iter_ahead_dispatch(k, [](auto) {});
    submit(cx, k, compiled && a.has_merge != 2, [&](void* dst, unsigned long long base) { batch_form(a, base, dst); },
           [&] { iter_ahead_dispatch(k, [&](auto inst) { inst.solo(k.wgs[0] + k.wgs[1] + k.wgs[2], cx.st, a); }); });
}

// ... and the same launch for n problems (blockIdx.y)
void launch_iter_ahead_batch(const LaunchKey& k, const IterAheadArgs* args_dev, const BatchBases& bases, int n, hipStream_t st) {
    iter_ahead_dispatch(k, [&](auto inst) {
        if constexpr (decltype(inst)::BATCHED) inst.batch(k.wgs[0] + k.wgs[1] + k.wgs[2], n, st, args_dev, bases);
    });
}

}  // namespace icem
