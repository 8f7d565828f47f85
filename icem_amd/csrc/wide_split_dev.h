// wide_split_dev.h -- the device functions of the 16-bit-plane GEMM rollout (k_rollout_wide_split.hip: the arithmetic, the tiling
// and the measurements behind them), shared by the by-value kernel there and its batched twin (k_rollout_wide_split_batch.hip:
// blockIdx.y = the problem, the argument block read from a device array; the kernels' body: wide_split_body.h), and the dispatch
// table both launches pick their instantiation through.
#pragma once
#include <cmath>
#include <type_traits>
#include "fused_dev.h"
#include "wide_dev.h"

namespace icem {

namespace {

constexpr int SPLIT_TT = 5;      // trajectory tiles per workgroup batch (regular batches take 4)
constexpr int SPLIT_WAVES = 8;
constexpr int SPLIT_KMAX = 416;   // contraction length (o + d, padded to 32) the fp16 form's per-entry scales have LDS for
// the shared planes: two buffers of (up to) 3 planes x 64 rows x 32 x 16 bits for the regular batches (one of 80 rows for the five-tile batch fits inside)
constexpr size_t SPLIT_PLANE_BYTES = (size_t)2 * 3 * 16 * (SPLIT_TT - 1) * 64;
static_assert(SPLIT_PLANE_BYTES >= (size_t)3 * 16 * SPLIT_TT * 64 && SPLIT_PLANE_BYTES >= 2 * SPLIT_WAVES * 32 * sizeof(unsigned long long), "planes buffer");

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// x -> (hi, residual): hi = bf16(x) round-to-nearest-even, both of a pair in one v_cvt_pk_bf16_f32
__device__ __forceinline__ unsigned split_pair(float& a, float& b) {
    const bf16x2 h = __builtin_convertvector(f32x2{a, b}, bf16x2);
    const unsigned u = __builtin_bit_cast(unsigned, h);
    // exact: the residual has at most 16 significant bits.  (Spelled as two v_sub_f32: the compiler's v_pk_add_f32 is
    // an expensive neighbour of MFMAs -- MI355X guide, "price of one filler beside MFMAs".)
    const float fa = __uint_as_float(u << 16), fb = __uint_as_float(u & 0xFFFF0000u);
    asm volatile("v_sub_f32 %0, %0, %1" : "+v"(a) : "v"(fa));
    asm volatile("v_sub_f32 %0, %0, %1" : "+v"(b) : "v"(fb));
    return u;
}

struct Planes {
    u32x4 hi, mid, lo;
};
// the three bf16 planes of 8 f32 values (a lane's share of one 32-deep contraction block)
__device__ __forceinline__ Planes split8(float4 p, float4 q) {
    float x[8] = {p.x, p.y, p.z, p.w, q.x, q.y, q.z, q.w};
    Planes r;
#pragma unroll
    for (int i = 0; i < 4; ++i) r.hi[i] = split_pair(x[2 * i], x[2 * i + 1]);
#pragma unroll
    for (int i = 0; i < 4; ++i) r.mid[i] = split_pair(x[2 * i], x[2 * i + 1]);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const bf16x2 h = __builtin_convertvector(f32x2{x[2 * i], x[2 * i + 1]}, bf16x2);
        r.lo[i] = __builtin_bit_cast(unsigned, h);
    }
    return r;
}

// The two fp16 planes of 8 f32 values scaled by S (a power of two chosen per trajectory row so that |x| S < 2^15):
// hi = f16(x S), lo = f16(x S - hi), both round-to-nearest-even (v_cvt_pk_f16_f32).  hi + lo is x S to 2^-24 relative
// (11 + 11 significant bits and lo's sign), lo is a normal fp16 number for every entry within 2^-13 of the row's largest
// and carries an absolute error below 2^-40 of that largest entry otherwise.
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
__device__ __forceinline__ void split8h(float4 p, float4 q, float4 cp, float4 cq, float S, u32x4& hi, u32x4& lo) {
    const float x[8] = {p.x * cp.x, p.y * cp.y, p.z * cp.z, p.w * cp.w, q.x * cq.x, q.y * cq.y, q.z * cq.z, q.w * cq.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const f32x2 v = {x[2 * i] * S, x[2 * i + 1] * S};
        const f16x2 h = __builtin_convertvector(v, f16x2);
        const f32x2 b = __builtin_convertvector(h, f32x2);
        const f16x2 l = __builtin_convertvector(f32x2{v[0] - b[0], v[1] - b[1]}, f16x2);
        hi[i] = __builtin_bit_cast(unsigned, h);
        lo[i] = __builtin_bit_cast(unsigned, l);
    }
}

template <bool F16>
__device__ __forceinline__ f32x4 mma(u32x4 a, u32x4 b, f32x4 c) {
    if constexpr (F16) return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
    else return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

// One batch of NTT trajectory tiles (rows [row0, row0 + 16 ntt), ntt <= NTT: tiles beyond ntt are computed on whatever their
// LDS rows hold and dropped -- no predicate inside the model loop) through all H steps.  m0 holds contraction block 0 of the
// wave's share of the model on entry and on exit.
template <int NCT, int NTT, int KIND, bool EXT, bool ONESET, bool F16, typename Req>
__device__ __forceinline__ void split_batch(const WideRolloutArgs& a, float* X, unsigned char* P, float* rscale, float* rinv, const float* ksc, const float* csc,
                                            const CostArgs<float>& cs_s,
                                            int row0, int ntt, int tid, int lane, int wave, u32x4 (&m0)[NCT * (F16 ? 2 : 3)],
                                            u32x4 (&m1)[NCT * (F16 ? 2 : 3)], Req&& request1, unsigned long long& run_key, bool& first) {
    constexpr int NPL = F16 ? 2 : 3;   // planes per operand: fp16 (hi, lo) / bf16 (hi, mid, lo)
    const int j = lane & 15, g = lane >> 4;
    const int XS = a.xs, KB = a.kb, o = a.o, d = a.d, H = a.h;
    const WideCost wc{a.lin_idx, a.flip_idx, a.ctrl_w, a.lin_w, a.flip_pen, a.flip_th};
    const bool sweep = EXT && cs_s.health_idx >= 0, diff = EXT && cs_s.diff_idx >= 0;
    const int nrow = 16 * ntt;
    __syncthreads();   // (the previous batch's readers are done with X)
    for (int e = tid; e < 16 * NTT * XS; e += 64 * SPLIT_WAVES) {
        const int c = e % XS;
        X[e] = c < o ? a.obs0[c] : 0.f;
    }
    // cost bookkeeping of the trajectory tile this wave scores (tt = wave), in lanes 0..15
    constexpr int NS = (SPLIT_TT + SPLIT_WAVES - 1) / SPLIT_WAVES;
    float acc_c[NS] = {}, c_prev[NS] = {}, dold[NS] = {};
    auto score = [&](int t) {   // finish step t - 1 (its difference term reads the observation now in X), start step t
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int tt = wave + SPLIT_WAVES * s;
            if (tt >= ntt) continue;   // (wave-uniform)
            const float* xt = X + (size_t)(16 * tt) * XS;
            if (t > 0 && lane < 16) {
                float c = c_prev[s];
                if (diff) c += wide_diff_cost(cs_s, xt[lane * XS + cs_s.diff_idx], dold[s]);
                acc_c[s] = wide_accumulate(acc_c[s], c, t - 1, a.cost_mode);
            }
            if (t < H) {
                bool bad = false;
                if (sweep) {   // lane (j, g) sweeps entries g, g + 4, .. of row j
                    const float* xj = xt + j * XS;
                    bool b = false;
                    for (int k = g; k < o; k += 4) b |= wide_bad_entry(cs_s, xj[k], k);
                    const unsigned long long mk = __ballot(b);
                    bad = ((mk >> (lane & 15)) & 0x0001000100010001ull) != 0ull;
                }
                if (lane < 16) c_prev[s] = wide_step_cost(wc, EXT, cs_s, xt + lane * XS, o, d, bad, dold[s]);
            }
        }
    };
    // The step's actions -> X[:, o .. o + d): element e = tid + 256 i of the batch's [nrow, d] block.  Step t + 1's are
    // requested at the top of step t and stay in registers across the model loop (a load -> LDS store -> barrier sequence
    // per step would expose one global round trip per step and element: measured, a third of the launch).
    constexpr int AE = 4;   // elements per thread held ahead: covers d <= 25 at 80 rows, d <= 32 at 64
    const bool ahead = nrow * d <= 64 * SPLIT_WAVES * AE;
    int aoff[AE], xoff[AE];
    float an[AE];
#pragma unroll
    for (int i = 0; i < AE; ++i) {
        const int e = tid + 64 * SPLIT_WAVES * i;
        const int r = e / d, c = e - r * d;
        const bool in = e < nrow * d;
        xoff[i] = in ? r * XS + o + c : -1;
        aoff[i] = (in && row0 + r < a.n_rows) ? (r * H) * d + c : -1;   // relative to the batch's first row
    }
    const float* abase = a.actions + (size_t)row0 * H * d;
    auto load_actions = [&](int t) {
#pragma unroll
        for (int i = 0; i < AE; ++i) an[i] = aoff[i] >= 0 ? abase[aoff[i] + t * d] : 0.f;
    };
    auto store_actions = [&](int t) {
        if (ahead) {
#pragma unroll
            for (int i = 0; i < AE; ++i)
                if (xoff[i] >= 0) X[xoff[i]] = an[i];
        } else {
            for (int e = tid; e < nrow * d; e += 64 * SPLIT_WAVES) {
                const int r = e / d, c = e - r * d;
                const int row = row0 + r;
                X[r * XS + o + c] = row < a.n_rows ? a.actions[((size_t)row * H + t) * d + c] : 0.f;
            }
        }
    };
    if (ahead) load_actions(0);
    __syncthreads();   // the zeros above and the actions below meet in X's action slots, written by different threads
    store_actions(0);
    long long* st = (a.dbg && blockIdx.x == 3 && tid == 64) ? a.dbg : nullptr;   // development: phase stamps of step 5 (tools/dbg/split_stamps.py)
    for (int t = 0; t < H; ++t) {
        if (st && t == 5) st[0] = wall_clock64();
        __syncthreads();
        if (st && t == 5) st[1] = wall_clock64();
        score(t);
        if (st && t == 5) st[2] = wall_clock64();
        if (ahead && t + 1 < H) load_actions(t + 1);
        f32x4 acc[NCT][NTT];
#pragma unroll
        for (int c = 0; c < NCT; ++c)
#pragma unroll
            for (int tt = 0; tt < NTT; ++tt) acc[c][tt] = f32x4{0.f, 0.f, 0.f, 0.f};
        // the shared planes P[buffer][plane][row][32 bf16]: regular batches double-buffer (block kb + 1 is split while block kb
        // is multiplied, one barrier per block); the five-tile batch has room for one buffer (two barriers per block)
        constexpr bool DB = NTT < SPLIT_TT;
        constexpr int ROWS = 16 * NTT;
        float S = 1.f;   // (fp16 planes) the power of two of this splitter thread's row
        auto split_row = [&](int r, int gg, int kbn, int buf) {
            const float* xp = X + (size_t)r * XS + 32 * kbn + 8 * gg;
            unsigned char* q = P + ((size_t)(buf * NPL) * ROWS + r) * 64 + gg * 16;
            if constexpr (F16) {
                u32x4 hi, lo;
                const float* cp = ksc + 32 * kbn + 8 * gg;
                split8h(*reinterpret_cast<const float4*>(xp), *reinterpret_cast<const float4*>(xp + 4), *reinterpret_cast<const float4*>(cp),
                        *reinterpret_cast<const float4*>(cp + 4), S, hi, lo);
                *reinterpret_cast<u32x4*>(q) = hi;
                *reinterpret_cast<u32x4*>(q + (size_t)ROWS * 64) = lo;
            } else {
                const Planes b = split8(*reinterpret_cast<const float4*>(xp), *reinterpret_cast<const float4*>(xp + 4));
                *reinterpret_cast<u32x4*>(q) = b.hi;
                *reinterpret_cast<u32x4*>(q + (size_t)ROWS * 64) = b.mid;
                *reinterpret_cast<u32x4*>(q + (size_t)2 * ROWS * 64) = b.lo;
            }
        };
        // blocks 1 .. : bf16 planes by the first 4 x ROWS threads, 8 entries each; fp16 planes by ALL threads, 4 entries each
        // (EIGHT per row) -- with the entries' scales to read and apply, four waves splitting for eight made the block's
        // critical path: their MFMAs began when their SIMD partners' had ended (k-loop 13.3 -> 15.3 us per step)
        float S8[F16 ? (NTT < SPLIT_TT ? 1 : 2) : 1] = {};   // the power of two of this thread's row (rows: one per 512 threads' pass)
        auto splitn = [&](int kbn, int buf) {
            if constexpr (!F16) {
                if (tid < 4 * ROWS) split_row(tid >> 2, tid & 3, kbn, buf);
            } else {
#pragma unroll
                for (int ps = 0; ps < (NTT < SPLIT_TT ? 1 : 2); ++ps) {
                    const int u = tid + 64 * SPLIT_WAVES * ps;
                    if (u < 8 * ROWS) {
                        const int r = u >> 3, g8 = u & 7;
                        const float4 x4 = *reinterpret_cast<const float4*>(X + (size_t)r * XS + 32 * kbn + 4 * g8);
                        const float4 c4 = *reinterpret_cast<const float4*>(ksc + 32 * kbn + 4 * g8);
                        const float sc = S8[ps];
                        const f32x2 v0 = {x4.x * c4.x * sc, x4.y * c4.y * sc}, v1 = {x4.z * c4.z * sc, x4.w * c4.w * sc};
                        const f16x2 h0 = __builtin_convertvector(v0, f16x2), h1 = __builtin_convertvector(v1, f16x2);
                        const f32x2 b0 = __builtin_convertvector(h0, f32x2), b1 = __builtin_convertvector(h1, f32x2);
                        const f16x2 l0 = __builtin_convertvector(f32x2{v0[0] - b0[0], v0[1] - b0[1]}, f16x2);
                        const f16x2 l1 = __builtin_convertvector(f32x2{v1[0] - b1[0], v1[1] - b1[1]}, f16x2);
                        unsigned char* q = P + ((size_t)(buf * NPL) * ROWS + r) * 64 + g8 * 8;
                        *reinterpret_cast<uint2*>(q) = uint2{__builtin_bit_cast(unsigned, h0), __builtin_bit_cast(unsigned, h1)};
                        *reinterpret_cast<uint2*>(q + (size_t)ROWS * 64) = uint2{__builtin_bit_cast(unsigned, l0), __builtin_bit_cast(unsigned, l1)};
                    }
                }
            }
        };
        // Block 0 of a step.  bf16 planes: like every block.  fp16 planes: by the threads four waves on (the waves that
        // score nothing at the step's top), which first find the row's scale -- four threads per row scan it, S = 2^(141 - e)
        // for a largest entry 1.m x 2^(e - 127), so |x| S < 2^15 (fp16 holds 65 504), exact powers of two throughout;
        // 1 / (S x the model's scale) waits in rinv[] for the write-back.  A NaN entry does not move the maximum and poisons
        // its own trajectory only (one B-operand row = one output column); an infinite one makes S 2^-114 and stays infinite.
        auto split_first = [&](int t) {
            if constexpr (!F16) {
                splitn(0, 0);
            } else {
                const int u = (tid + 4 * 64) & (64 * SPLIT_WAVES - 1);
                if (u < 4 * ROWS) {
                    const int r = u >> 2, gg = u & 3;
                    const float* xr = X + (size_t)r * XS + 4 * gg;
                    const float* cr = ksc + 4 * gg;
                    // (tanh model, t > 0: the state entries are below 1 -- their scaled bound a.sbound stands in for them, only
                    //  the actions behind them are scanned: an upper bound of the largest contribution is all S needs)
                    const bool bounded = KIND == 1 && t > 0;
                    float mx = bounded ? a.sbound : 0.f;
                    for (int k = bounded ? ((o / 4) & ~3) : 0; k < 8 * KB; k += 4) {   // float4s gg, gg + 4, ..: the row's 32 KB entries, a quarter each
                        if (4 * (gg + k) < 32 * KB) {
                            float4 v = *reinterpret_cast<const float4*>(xr + 4 * k);
                            const float4 c = *reinterpret_cast<const float4*>(cr + 4 * k);
                            v.x *= c.x; v.y *= c.y; v.z *= c.z; v.w *= c.w;
                            mx = __builtin_fmaxf(__builtin_fmaxf(mx, __builtin_fabsf(v.x)), __builtin_fmaxf(__builtin_fabsf(v.y), __builtin_fmaxf(__builtin_fabsf(v.z), __builtin_fabsf(v.w))));
                        }
                    }
                    mx = __builtin_fmaxf(mx, __shfl_xor(mx, 1));
                    mx = __builtin_fmaxf(mx, __shfl_xor(mx, 2));
                    int e = (int)(__float_as_uint(mx) >> 23);
                    e = e < 40 ? 40 : e;   // (an all-zero row: any scale)
                    const float Sr = __uint_as_float((unsigned)(268 - e) << 23);
                    if (gg == 0) {
                        rscale[r] = Sr;
                        rinv[r] = __uint_as_float((unsigned)(e - 14) << 23) * a.minv;
                    }
                    const float keep = S;
                    S = Sr;
                    split_row(r, gg, 0, 0);
                    S = keep;
                }
            }
        };
        // A block: the planes of all NTT tiles are read once, then column tile by column tile -- 6 products x NTT tiles on NTT
        // different accumulators -- with the NEXT block's operands of that column tile requested between its MFMAs (two sets:
        // every operand is asked for exactly one block before its use; one set: over itself, behind its last use).
        static_assert(ONESET || NTT < SPLIT_TT, "the two-set form has one tile group");
        auto block = [&](const u32x4 (&m)[NCT * NPL], int buf, u32x4 (&mn)[NCT * NPL], int kbn) {
            const unsigned char* q0 = P + ((size_t)(buf * NPL) * ROWS + j) * 64 + g * 16;
            auto feed = [&](int e) {
                __builtin_amdgcn_sched_barrier(0);
                mn[e] = request1(kbn, e);
                __builtin_amdgcn_sched_barrier(0);
            };
            // (the five-tile batch in two groups of tiles, 3 + 2: see the head of the file)
            constexpr int T0 = NTT < SPLIT_TT ? NTT : 3;
            auto group = [&](auto t_lo, auto t_n, bool first, bool last) {
                constexpr int TL = decltype(t_lo)::value, TN = decltype(t_n)::value;
                // planes of the group's tiles: [0] hi, [1] mid (bf16) / lo (fp16), [2] lo (bf16)
                u32x4 bp[NPL][TN];
                if (!first) __builtin_amdgcn_sched_barrier(0);   // (or the second group's planes are read beside the first's)
#pragma unroll
                for (int pl = 0; pl < NPL; ++pl) {
                    const int src = pl == 0 ? 0 : (NPL - pl);   // read order hi, lo, (mid): the order the products want them in
#pragma unroll
                    for (int tt = 0; tt < TN; ++tt) bp[src][tt] = *reinterpret_cast<const u32x4*>(q0 + (size_t)(16 * (TL + tt) + src * ROWS) * 64);
                }
                // products, smallest first; model operands m[NPL c + ..]: planes in the order lo, (mid), hi
                constexpr int NPROD = F16 ? 3 : 6;
                constexpr int PA[6] = {0, NPL - 1, F16 ? 1 : 1, 1, 2, 2};          // A: Lo, Hi, [Hi] | Mid, Mid, Hi, Hi
                constexpr int PB[6] = {0, NPL - 1, F16 ? 0 : 1, 0, 1, 0};          // B: hi, lo, [hi] | mid, hi, mid, hi
#pragma unroll
                for (int c = 0; c < NCT; ++c) {
#pragma unroll
                    for (int p = 0; p < NPROD; ++p) {
                        // product by product over the group's tiles: consecutive MFMAs write different accumulators
#pragma unroll
                        for (int tt = 0; tt < TN; ++tt) acc[c][TL + tt] = mma<F16>(m[NPL * c + PA[p]], bp[PB[p]][tt], acc[c][TL + tt]);
                        if (!ONESET && first && last) {   // the next block's operands of this column tile, spread over its products
#pragma unroll
                            for (int i = 0; i < NPL; ++i)
                                if (p == (i + 1) * NPROD / NPL - 1) feed(NPL * c + i);
                        }
                    }
                    if (ONESET && last) {   // over the operands just used for the last time
#pragma unroll
                        for (int i = 0; i < NPL; ++i) feed(NPL * c + i);
                    }
                }
            };
            group(std::integral_constant<int, 0>{}, std::integral_constant<int, T0>{}, true, T0 == NTT);
            if constexpr (T0 < NTT) group(std::integral_constant<int, T0>{}, std::integral_constant<int, NTT - T0>{}, false, true);
        };
        // behind a block: everybody is done with its planes (and the next block's are complete, if they were made beside it)
        auto behind = [&](int kbn) {
            __syncthreads();
            if (!DB && kbn >= 0) {
                splitn(kbn, 0);
                __syncthreads();
            }
        };
        split_first(t);
        __syncthreads();
        if constexpr (F16) {
#pragma unroll
            for (int ps = 0; ps < (NTT < SPLIT_TT ? 1 : 2); ++ps)
                if (tid + 64 * SPLIT_WAVES * ps < 8 * ROWS) S8[ps] = rscale[(tid + 64 * SPLIT_WAVES * ps) >> 3];
        }
        int kb = 0;
        if constexpr (!ONESET) {
            // two register sets of model operands, a block's requested while the block before it runs; beside the last block: block 0 of the NEXT step
#pragma unroll 1
            for (; kb + 1 < KB; kb += 2) {
                splitn(kb + 1, 1);
                block(m0, 0, m1, kb + 1);
                behind(kb + 1);
                if (kb + 2 < KB) splitn(kb + 2, 0);
                block(m1, 1, m0, kb + 2 < KB ? kb + 2 : 0);
                behind(kb + 2 < KB ? kb + 2 : -1);
            }
            if (kb < KB) {   // odd block count: the last one (outside the loop: a conditional block inside it costs a copy of every accumulator per trip)
                block(m0, 0, m1, 0);   // (the next step's block 0 lands in m1: moved to m0 at the step's end, when it has long arrived)
            }
        } else {
#pragma unroll 1
            for (; kb < KB; ++kb) {
                if (DB && kb + 1 < KB) splitn(kb + 1, (kb + 1) & 1);
                block(m0, DB ? (kb & 1) : 0, m0, kb + 1 < KB ? kb + 1 : 0);
                behind(kb + 1 < KB ? kb + 1 : -1);
            }
        }
        if (st && t == 5) st[3] = wall_clock64();
        if (a.dbg && blockIdx.x == 3 && lane == 0 && t == 5) a.dbg[8 + wave] = wall_clock64();   // every wave's loop end
        __syncthreads();   // everybody has read X: the new observation may go in
        if (st && t == 5) st[4] = wall_clock64();
#pragma unroll
        for (int c = 0; c < NCT; ++c) {
            const int col = 16 * (NCT * wave + c) + 4 * g;
#pragma unroll
            for (int tt = 0; tt < NTT; ++tt) {
                f32x4 v = acc[c][tt];
                if constexpr (F16) {   // the row's, the model's and the column's powers of two taken out again (exact)
                    const float iv = rinv[16 * tt + j];
                    const float4 cs4 = *reinterpret_cast<const float4*>(csc + col);
                    v[0] *= iv * cs4.x;
                    v[1] *= iv * cs4.y;
                    v[2] *= iv * cs4.z;
                    v[3] *= iv * cs4.w;
                }
                if (KIND == 1) {
#pragma unroll
                    for (int k = 0; k < 4; ++k) v[k] = fast_tanh(v[k]);
                }
                float* dst = X + (size_t)(16 * tt + j) * XS + col;
                if (col + 3 < o) {
                    *reinterpret_cast<f32x4*>(dst) = v;
                } else {   // the column group that straddles o: the action slots behind it belong to other threads
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (col + k < o) dst[k] = v[k];
                }
            }
        }
        if (st && t == 5) st[5] = wall_clock64();
        if (t + 1 < H) store_actions(t + 1);
        if (!ONESET && (KB & 1)) {
#pragma unroll
            for (int e = 0; e < NCT * NPL; ++e) m0[e] = m1[e];
        }
        if (st && t == 5) st[6] = wall_clock64();
        if (st && t == 6) st[7] = wall_clock64();
    }
    __syncthreads();
    score(H);
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const int tt = wave + SPLIT_WAVES * s;
        if (tt >= ntt) continue;
        const int row = row0 + 16 * tt + (lane & 15);
        const bool live = row < a.n_rows;
        if (live && lane < 16) a.costs[row] = acc_c[s];
        if (a.K > 0) {
            const unsigned long long key = (lane < 16 && live && row < a.n_cand) ? make_key(acc_c[s], row) : KEY_SENTINEL;
            run_key = topk_push16(run_key, key, first, a.K, lane);
            first = false;
        }
    }
}

// The one table of the plane kernel: key -> compiled instantiation, handed to `f` as (NCT, KIND, EXT, FIVE, F16) constants -- the
// by-value launch and the batched one pick their kernel through it
template <class F>
bool wide_split_dispatch(const LaunchKey& k, F&& f) {
    using std::integral_constant;
#define X5(NV, KV, EV, FV)                                                                                                                          \
    if (k.arith == 2) return f(integral_constant<int, NV>{}, integral_constant<int, KV>{}, integral_constant<bool, EV>{}, integral_constant<bool, FV>{}, std::true_type{}), true; \
    return f(integral_constant<int, NV>{}, integral_constant<int, KV>{}, integral_constant<bool, EV>{}, integral_constant<bool, FV>{}, std::false_type{}), true;
#define X4(NV, KV, EV)       \
    if (k.form & 2) {        \
        X5(NV, KV, EV, true) \
    } else {                 \
        X5(NV, KV, EV, false) \
    }
#define X3(NV, KV)           \
    if (k.form & 1) {        \
        X4(NV, KV, true)     \
    } else {                 \
        X4(NV, KV, false)    \
    }
#define X2(NV)               \
    if (k.waves == NV) {     \
        if (k.kind == 1) {   \
            X3(NV, 1)        \
        } else {             \
            X3(NV, 0)        \
        }                    \
    }
    X2(1) X2(2) X2(3)
#undef X2
#undef X3
#undef X4
#undef X5
    return false;
}
// the workgroup's dynamic LDS: 80 contraction rows and the planes' buffers
inline size_t wide_split_lds_bytes(const LaunchKey& k) { return (size_t)16 * SPLIT_TT * wide_split_xs(k.O, k.d) * sizeof(float) + SPLIT_PLANE_BYTES; }

}  // namespace

}  // namespace icem
