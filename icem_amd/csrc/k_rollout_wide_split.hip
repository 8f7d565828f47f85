// k_rollout_wide_split.hip -- K2 + K3 for WIDE observations (32 < o <= 384; HumanoidStandup's o = 378, d = 17:
// icem/environments/mujoco.py:241-277) with the model step on the bf16 matrix cores: rollout_wide_split_kernel.
//
// The step [n, o + d] x [o + d, o] is a GEMM three orders of magnitude above the f32 ridge, and the exact-f32 MFMA of
// k_rollout_wide.hip runs at 1/16 of the 16-bit rate.  Two splits of the f32 operands onto the 16-bit matrix cores, one
// kernel template (F16):
//   * fp16, two planes, THREE products (the default; icem_set_wide_exact 0).  x S = hi + lo with hi = f16(x S), lo =
//     f16(x S - hi), both round-to-nearest-even: 11 + 11 significant bits and lo's sign, x S to 2^-24 relative.  S is a
//     power of two per TRAJECTORY ROW and step, taken from the row's largest entry so that |x| S < 2^15 (fp16 ends at
//     65 504; found by four threads per row at the step's top), and one per model (pack_wide_model_split); both are taken
//     out of the accumulators again at the write-back, exactly.  A product x m = hi Hi + hi Lo + lo Hi (+ lo Lo, dropped:
//     below 2^-22 of hi Hi, i.e. 2^-24-class like the operands' own rounding), each of the three EXACT in the f32
//     accumulator's format (22 significant bits), summed smallest first on v_mfma_f32_16x16x32_f16.  The model is carried
//     EQUILIBRATED (pack_wide_model_split): row k as M[k][:] 2^-e_k with entry k as x_k 2^e_k, column j as M[:][j] 2^-f_j with
//     the accumulators x 2^f_j at the write-back -- rows, then columns, peak in [0.5, 1): one sweep of a matrix balancing,
//     exact (powers of two).  S therefore follows a row's largest CONTRIBUTION, and what fp16's subnormals cost -- an
//     entry 2^-r of the largest keeps 2^-24 relative up to r = 13, beyond that an ABSOLUTE 2^-40 of the largest -- is
//     relative to each output column's own scale: the same dynamics in other units (D^-1 A D: observation entries 10^6 apart
//     with weights to match) come out as they went in (test_wide_split_planes_in_mixed_units), and an entry the model
//     ignores takes no part.  What is left outside: contributions that differ by more than 2^13 inside a BALANCED model
//     (one state entry of 10^6 feeding a column beside entries of 1 feeding others): there the small columns see 1e-6
//     relative per step instead of 6e-8 -- the bf16 planes below (exact operands) are for such a model.  Measured against
//     the float64 oracle over 30 tanh steps at o = 378: 1-4 x 10^-6 relative, the exact-f32 kernel's own distance
//     (tools/dbg/split_tile_errors.py; tests: observations from 1e-30 to 1e9 in test_wide_fp16_planes_follow_the_magnitudes).
//   * bf16, three planes, SIX products (icem_set_wide_exact 2; round 4's first form).  x = hi + mid + lo EXACTLY (3 x 8
//     significant bits, no scale needed: bf16 has f32's exponent), products hi*Hi, hi*Mid, mid*Hi, hi*Lo, lo*Hi, mid*Mid
//     on v_mfma_f32_16x16x32_bf16; what is dropped is below 2^-31 of a product.  Two thirds of the fp16 form's speed.
// Either way the result is an f32 dot product with f32-class rounding, not the bits of an fmaf chain (error analysis:
// DESIGN.md section 4); a row's result depends on that row and the model only, wherever the row sits in a launch.
//
// Tiling (numbers for the bf16 form; the fp16 one has two planes where it has three, three products where it has six).  A
// 16-row tile per wave (k_rollout_wide.hip) streams the whole model through every wave every step; in three bf16 planes
// that is 958 KB per 16 rows and step -- more than a CU's L2 port delivers.  So a WORKGROUP owns up to 80
// trajectories (five 16-row tiles; four is the regular batch, the fifth takes the few rows a population leaves behind
// whole batches -- the shifted elites of iteration 0, icem.py:131-137 -- instead of a second round of workgroups):
//   * their contraction vectors [obs | action | 0-pad] live in LDS as f32 rows X[80][XS] (134 KB: one workgroup per CU);
//   * wave w of 8 (two per SIMD) owns the output column tiles NCT w .. NCT w + NCT - 1 for ALL the workgroup's
//     trajectories -- NCT x 4 (5) accumulator tiles -- and streams only ITS eighth of the model: per 32-deep contraction
//     block 3 planes x NCT 16-byte loads per lane into a second register set, requested BETWEEN the MFMAs of the block
//     before, one load per 8 MFMAs (all nine at the block's top queue up in front of the CU's one texture path, ~21 cycles
//     per 1 KB, and a wave whose load is not accepted yet does not issue the MFMAs behind it: 900 -> 823 us per launch);
//   * the B operand's planes are made ONCE per block for the whole workgroup -- thread u of the first 4 x rows splits
//     the 8 contraction entries (row u / 4, slot u % 4) -- and shared through a double-buffered 24 KB of LDS behind X: block
//     kb + 1 is split beside block kb's MFMAs, one barrier per block.  (Every wave splitting the same values for itself, the
//     first form of this kernel, asked the issue port for 3.3 VALU per MFMA where 3 fit: EXPERIMENTS R4.4.)
//   * per block a wave reads the planes of all its tiles (12 ds_read_b128) and runs column tile by column tile, 6 products x
//     4 tiles, consecutive MFMAs on different accumulators; per accumulator the order of the six products never changes
//     (Lo*hi, Hi*lo, Mid*mid, Mid*hi, Hi*mid, Hi*hi), so every form of this kernel returned the same bits;
//   * a launch in which some workgroup is left with FIVE tiles runs the FIVE instantiation: the five-tile batch in two tile
//     groups (3 + 2) with ONE operand set (requests over the operands just used).  Kept out of the regular kernel because
//     its 60 accumulators set the whole kernel's register allocation (+14 % on launches that never see a fifth tile), and
//     kept to one set because two spill > 100 VGPRs at 256 (11 with one);
//   * the step's actions are requested one step ahead and held in registers across the model loop;
//   * two workgroup barriers per step around the model loop's (X read by everybody -> X rewritten column block by column block);
//   * step cost, candidate lists and the running top-K as in k_rollout_wide.hip (trajectory tile tt is scored by wave tt's
//     lanes 0..15 from X); icem_cost_terms included (EXT).
// Model operand layout (pack_wide_model_split): Mb[kb][wave][ct][plane][lane] = 8 x 16 bits = M[32 kb + 8 (lane / 16) + v]
// [16 (NCT wave + ct) + lane % 16], planes in the order lo, (mid,) hi.
#include <cstring>
#include "wide_split_dev.h"

namespace icem {

namespace {

// (the body: wide_split_body.h, shared as text with the batched twin of k_rollout_wide_split_batch.hip)
// FIVE: some workgroup's tile count leaves a remainder of five (one batch instead of 4 + 1).  Its own instantiation: the
// five-tile batch's 60 accumulators set the register allocation of the whole kernel, and the four-tile batches of a launch
// that never sees one were 14 % slower for carrying it.
template <int NCT, int KIND, bool EXT, bool FIVE, bool F16>
__global__ __launch_bounds__(64 * SPLIT_WAVES) void rollout_wide_split_kernel(WideRolloutArgs a) {
#include "wide_split_body.h"
}

__host__ unsigned short bf16_rne(float x) {
    unsigned u;
    std::memcpy(&u, &x, 4);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (unsigned short)(u >> 16);
}
__host__ float bf16_f32(unsigned short b) {
    const unsigned u = (unsigned)b << 16;
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}

}  // namespace

int wide_split_kb(int o, int d) { return (o + d + 31) / 32; }
int wide_split_xs(int o, int d) { return 32 * wide_split_kb(o, d) + 4; }
// the workgroup's LDS: 80 rows of 32 kb + 4 floats, the planes' buffers and ~3 KB of static arrays in 160 KB: o + d <= 416
bool wide_split_fits(int o, int d) { return (size_t)16 * SPLIT_TT * wide_split_xs(o, d) * sizeof(float) + SPLIT_PLANE_BYTES + 4608 <= 160 * 1024 && 32 * wide_split_kb(o, d) <= SPLIT_KMAX; }
static int wide_split_nct(int o) { const int nt = (o + 15) / 16; return nt <= 8 ? 1 : nt <= 16 ? 2 : 3; }

// workgroups (= candidate lists): whole batches of four tiles, at most FAST_MAX_LISTS
int wide_split_lists(int n_rows) {
    const int tiles = std::max(1, (n_rows + 15) / 16);
    return std::min(std::max(1, tiles / (SPLIT_TT - 1)), FAST_MAX_LISTS);
}

// How far the EQUILIBRATED model (rows, then columns scaled by powers of two as pack_wide_model_split does for the fp16
// planes) stays from balanced: the largest log2(global max / line max) over its live rows and live columns.  0-1 for a
// model one sweep balances; a row or column whose LARGEST weight sits 2^13 below the model's largest has every entry where
// the fp16 pair no longer carries f32's 22+ bits relative to that line (the lo plane in fp16's subnormals) -- the model
// ICEM_WIDE_AUTO hands to the bf16 planes, whose operands are exact at any magnitude.  Incidental small entries inside a
// line that has a large one do not count (their error is absolute, 2^-40 of that line's largest; a dense random model has
// some 0.05 % of its entries 2^13 below its largest; the benchmark's 0.95 I + 0.05 N / sqrt(o) 3.5 % of every row) -- a
// STRUCTURAL spread does: a row or column in which MOST nonzero weights lie that far below its largest (a block of the
// model in other units than diagonal scaling can take out); the states that exercise those weights carry 10^-6 relative
// per step.  Returned: the larger of the two measures (log2 largest / weakest line's largest, log2 line's largest / its
// median nonzero weight, worst line).
int wide_model_imbalance_log2(int o, int d, const double* A, const double* B) {
    auto M = [&](int r, int c) -> double { return r < o ? A[(size_t)r * o + c] : B[(size_t)(r - o) * o + c]; };
    std::vector<int> ek((size_t)o + d, 0), fj((size_t)o, 0);
    std::vector<char> dead((size_t)o + d, 1);
    for (int r = 0; r < o + d; ++r) {
        float wmax = 0.f;
        bool any = false;
        for (int c = 0; c < o; ++c) {
            const float m = std::fabs((float)M(r, c));
            if (std::isfinite(m) && m > wmax) wmax = m;
            any = any || M(r, c) != 0.0;
        }
        if (!any) continue;
        int e = 0;
        if (wmax > 0.f) (void)std::frexp(wmax, &e);
        ek[r] = e < -100 ? -100 : (e > 100 ? 100 : e);
        dead[r] = 0;
    }
    std::vector<float> cmax((size_t)o, 0.f), rmax((size_t)o + d, 0.f);
    for (int c = 0; c < o; ++c) {
        for (int r = 0; r < o + d; ++r) {
            if (dead[r]) continue;
            const float m = std::fabs(std::ldexp((float)M(r, c), -ek[r]));
            if (std::isfinite(m) && m > cmax[c]) cmax[c] = m;
        }
        int f = 0;
        if (cmax[c] > 0.f) (void)std::frexp(cmax[c], &f);
        fj[c] = f < -100 ? -100 : (f > 100 ? 100 : f);
    }
    float gmax = 0.f;
    std::fill(cmax.begin(), cmax.end(), 0.f);
    for (int r = 0; r < o + d; ++r) {
        if (dead[r]) continue;
        for (int c = 0; c < o; ++c) {
            const float m = std::fabs(std::ldexp((float)M(r, c), -ek[r] - fj[c]));
            if (!std::isfinite(m)) continue;
            rmax[r] = std::max(rmax[r], m);
            cmax[c] = std::max(cmax[c], m);
            gmax = std::max(gmax, m);
        }
    }
    if (!(gmax > 0.f)) return 0;
    int worst = 0;
    {   // the structural spread: a line's largest weight over the MEDIAN of its nonzero weights
        std::vector<float> mags;
        auto spread = [&](int line_is_row, int idx) {
            mags.clear();
            float mx = 0.f;
            const int n = line_is_row ? o : o + d;
            for (int t = 0; t < n; ++t) {
                const int r = line_is_row ? idx : t, c = line_is_row ? t : idx;
                if (dead[r]) continue;
                const float m = std::fabs(std::ldexp((float)M(r, c), -ek[r] - fj[c]));
                if (std::isfinite(m) && m > 0.f) {
                    mags.push_back(m);
                    mx = std::max(mx, m);
                }
            }
            if (mags.size() < 2) return;
            std::nth_element(mags.begin(), mags.begin() + mags.size() / 2, mags.end());
            int em = 0, eq = 0;
            (void)std::frexp(mx, &em);
            (void)std::frexp(mags[mags.size() / 2], &eq);
            worst = std::max(worst, em - eq);
        };
        for (int r = 0; r < o + d; ++r)
            if (!dead[r]) spread(1, r);
        for (int c = 0; c < o; ++c) spread(0, c);
    }
    auto line = [&](float mx) {
        if (!(mx > 0.f)) return;   // (a column nothing feeds: zero in every arithmetic)
        int eg = 0, el = 0;
        (void)std::frexp(gmax, &eg);
        (void)std::frexp(mx, &el);
        worst = std::max(worst, eg - el);
    };
    for (int r = 0; r < o + d; ++r)
        if (!dead[r]) line(rmax[r]);
    for (int c = 0; c < o; ++c) line(cmax[c]);
    return worst;
}

// Mb[kb][wave][ct][plane][lane][v] = plane of (float)M[32 kb + 8 (lane / 16) + v][16 (NCT wave + ct) + lane % 16],
// M = [A ; B] ([o + d, o], zero padded).  planes = 3: bf16 lo, mid, hi.  planes = 2: fp16 lo, hi of M x 2^k, k such that the
// largest entry stays below 2^15; *minv = 2^-k.
void pack_wide_model_split(int o, int d, const double* A, const double* B, int planes, std::vector<unsigned short>& Mb, float* minv,
                           std::vector<float>* ksc, std::vector<float>* csc, float* sbound) {
    const int KB = wide_split_kb(o, d), NCT = wide_split_nct(o);
    Mb.assign((size_t)KB * SPLIT_WAVES * NCT * planes * 64 * 8, 0);
    auto M = [&](int r, int c) -> double {
        if (c >= o) return 0.0;
        if (r < o) return A[(size_t)r * o + c];
        if (r < o + d) return B[(size_t)(r - o) * o + c];
        return 0.0;
    };
    float SM = 1.f;
    // fp16 planes: contraction entry k (an observation / action entry) is carried as x_k 2^e_k and the model's row k as
    // M[k][:] 2^-e_k, 2^e_k the power of two of the row's largest weight -- every row of the scaled model peaks in [0.5, 1),
    // and the planes' per-trajectory scale follows the largest CONTRIBUTION x_k max|M[k][:]|, not the largest entry: an
    // observation in mixed units (positions of 1, forces of 10^4 with weights of 10^-4) keeps its small entries' bits, and an
    // entry the model ignores (a zero row: 2^e_k = 0) takes no part.  Exact: powers of two.
    std::vector<int> ek((size_t)32 * KB, 0);
    std::vector<char> dead((size_t)32 * KB, 1);
    if (planes == 2) {
        if (ksc) ksc->assign((size_t)32 * KB, 0.f);
        for (int r = 0; r < o + d; ++r) {
            float wmax = 0.f;
            for (int c = 0; c < o; ++c) {
                const float m = std::fabs((float)M(r, c));
                if (std::isfinite(m) && m > wmax) wmax = m;   // (a NaN / infinite weight: the scale of the finite ones, the weight stays what it is)
            }
            bool any = false;
            for (int c = 0; c < o; ++c) any = any || M(r, c) != 0.0;   // (NaN != 0: a row with a NaN weight is not dead)
            if (!any) continue;
            int e = 0;
            if (wmax > 0.f) (void)std::frexp(wmax, &e);
            e = e < -100 ? -100 : (e > 100 ? 100 : e);
            ek[r] = e;
            dead[r] = 0;
            if (ksc) (*ksc)[r] = std::ldexp(1.f, e);
        }
    }
    if (sbound) {   // the largest scaled state entry a tanh model can hand on: max over the observation entries of 2^e_k x 1
        *sbound = 0.f;
        if (planes == 2)
            for (int r = 0; r < o; ++r)
                if (!dead[r]) *sbound = std::max(*sbound, std::ldexp(1.f, ek[r]));
    }
    // ... and output column j as (sum) 2^f_j, 2^f_j the power of two of the column's largest (row-scaled) weight: the planes'
    // absolute accuracy (2^-40 of the row's largest contribution) is then relative to every COLUMN's own scale.  Rows, then
    // columns: the first sweep of a matrix balancing -- the same dynamics in other units (D^-1 A D) come out as A.
    std::vector<int> fj((size_t)o, 0);
    if (planes == 2) {
        if (csc) csc->assign((size_t)16 * SPLIT_WAVES * NCT, 1.f);
        for (int c = 0; c < o; ++c) {
            float cmax = 0.f;
            for (int r = 0; r < o + d; ++r) {
                if (dead[r]) continue;
                const float m = std::fabs(std::ldexp((float)M(r, c), -ek[r]));
                if (std::isfinite(m) && m > cmax) cmax = m;
            }
            int f = 0;
            if (cmax > 0.f) (void)std::frexp(cmax, &f);
            f = f < -100 ? -100 : (f > 100 ? 100 : f);
            fj[c] = f;
            if (csc) (*csc)[c] = std::ldexp(1.f, f);
        }
    }
    auto Ms = [&](int r, int c) -> float {   // the model as the fp16 planes see it
        if (r >= o + d || c >= o || dead[r]) return 0.f;
        return std::ldexp((float)M(r, c), -ek[r] - fj[c]);
    };
    if (planes == 2) {
        float mx = 0.f;
        for (int r = 0; r < o + d; ++r)
            for (int c = 0; c < o; ++c) {
                const float m = std::fabs(Ms(r, c));
                if (std::isfinite(m) && m > mx) mx = m;
            }
        int e = 0;
        if (mx > 0.f && std::isfinite(mx)) (void)std::frexp(mx, &e);   // mx = f x 2^e, f in [0.5, 1)
        else e = 1;
        SM = std::ldexp(1.f, 15 - e);
        if (minv) *minv = std::ldexp(1.f, e - 15);
    } else if (minv) {
        *minv = 1.f;
    }
    for (int kb = 0; kb < KB; ++kb)
        for (int w = 0; w < SPLIT_WAVES; ++w)
            for (int ct = 0; ct < NCT; ++ct)
                for (int lane = 0; lane < 64; ++lane)
                    for (int v = 0; v < 8; ++v) {
                        const float m = (float)M(32 * kb + 8 * (lane / 16) + v, 16 * (NCT * w + ct) + lane % 16);
                        if (planes == 2) {
                            const float ms = Ms(32 * kb + 8 * (lane / 16) + v, 16 * (NCT * w + ct) + lane % 16) * SM;
                            const _Float16 hi = (_Float16)ms;
                            const _Float16 lo = (_Float16)(ms - (float)hi);
                            const size_t at = ((((size_t)kb * SPLIT_WAVES + w) * NCT + ct) * 2) * 64 * 8 + (size_t)lane * 8 + v;
                            std::memcpy(&Mb[at], &lo, 2);
                            std::memcpy(&Mb[at + 64 * 8], &hi, 2);
                            continue;
                        }
                        const unsigned short hi = bf16_rne(m);
                        const float r1 = m - bf16_f32(hi);
                        const unsigned short mid = bf16_rne(r1);
                        const float r2 = r1 - bf16_f32(mid);
                        const unsigned short lo = bf16_rne(r2);
                        const size_t at = ((((size_t)kb * SPLIT_WAVES + w) * NCT + ct) * 3) * 64 * 8 + (size_t)lane * 8 + v;
                        Mb[at] = lo;
                        Mb[at + 64 * 8] = mid;
                        Mb[at + 2 * 64 * 8] = hi;
                    }
}

// the launch's key: everything that selects the instantiation and the grid (a batch issues ONE launch for problems of equal keys)
void launch_rollout_wide_split(const LaunchCtx& cx, const WideRolloutArgs& a, int kind) {
    const int grid = wide_split_lists(a.n_rows);
    // a batch of five: some workgroup holds 4 q + 1 tiles, q >= 1
    const int tiles = (a.n_rows + 15) / 16, base = tiles / grid, extra = tiles % grid;
    const bool five = (base >= SPLIT_TT && base % (SPLIT_TT - 1) == 1) || (extra > 0 && base + 1 >= SPLIT_TT && (base + 1) % (SPLIT_TT - 1) == 1);
    LaunchKey k;
    k.family = LAUNCH_ROLLOUT_WIDE_SPLIT;
    k.h = a.h, k.d = a.d, k.O = a.o, k.kind = kind == 1 ? 1 : 0, k.arith = a.planes == 2 ? 2 : 3;
    k.waves = wide_split_nct(a.o);
    k.form = (a.cs ? 1 : 0) | (five ? 2 : 0);
    k.wgs[0] = grid;
    hipStream_t st = cx.st;
    submit(cx, k, true, [&](void* dst, unsigned long long) { batch_form(a, dst); }, [&] {
        wide_split_dispatch(k, [&](auto nct, auto kd, auto ext, auto fv, auto f16) {
            auto kfn = rollout_wide_split_kernel<decltype(nct)::value, decltype(kd)::value, decltype(ext)::value, decltype(fv)::value, decltype(f16)::value>;
            const size_t lds = wide_split_lds_bytes(k);
            (void)hipFuncSetAttribute((const void*)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            hipLaunchKernelGGL(kfn, dim3(grid), dim3(64 * SPLIT_WAVES), lds, st, a);
        });
    });
}

}  // namespace icem
