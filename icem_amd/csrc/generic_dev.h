// generic_dev.h -- the bodies of the generic kernels an MPC step runs in the strict-parity arithmetic, each written ONCE as a
// __device__ function: the four-lanes-per-row sampler, the two rollouts (a thread / a row of lanes per trajectory), the shifted
// elites' copy and the one-launch selection + refit.  generic_kernels.hip wraps them in the __global__ kernels that take their
// arguments by value (a solo step); k_generic_batch.hip in the ones that read the block of problem blockIdx.y from a device array
// (icem_plan_step_batch_f64).  One text, one summation order: a problem's bits do not depend on which of the two launched it.
// Argument blocks: generic_args.h.  Internal; not part of the public ABI.
#pragma once
#include "host_common.h"
#include "cost_terms_dev.h"
#include "philox.h"
#include "refit.h"

namespace icem {

template <typename T>
__device__ __forceinline__ T inf_v() {
    return (T)INFINITY;
}

// (cost, index) lexicographic order; the index breaks ties (np.argmin / stable argsort semantics).
template <typename T>
__device__ __forceinline__ bool key_less(T ca, int ia, T cb, int ib) {
    return ca < cb || (ca == cb && ia < ib);
}

// ---- K1: the four-lanes-per-row sampler ------------------------------------------------------------------------------
// The same sampler with FOUR lanes per (trajectory, dim) row (WG / 4 rows per workgroup): in float64 a row is one thread's chain of
// HMAX / 2 libm-grade Box-Muller transforms and h x HMAX dependent fused multiply-adds -- 19 us per launch at N = 4096 with the
// chip all but empty.  Lane q of a row's quad runs the row's generator like the others (integer work: cheap), transforms only
// the pairs p = q, q + 4, .. of its words (or loads only those entries of the caller's z), multiplies them into partial sums
// over ITS table columns (W staged in LDS) and the quad adds the four partial sums (two DPP swaps).  Not the thread form's
// summation order: results agree with it to rounding (a few 1e-16 relative), inside the strict-parity bar of 1e-10.
template <int CTRL>
__device__ __forceinline__ float quad_swap(float x) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, 0xF, 0xF, false));
}
template <int CTRL>
__device__ __forceinline__ double quad_swap(double x) {
    const long long b = __double_as_longlong(x);
    const int lo = __builtin_amdgcn_update_dpp(0, (int)b, CTRL, 0xF, 0xF, false);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), CTRL, 0xF, 0xF, false);
    return __longlong_as_double((long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned long long)(unsigned)lo));
}

template <typename T, int HMAX, int ROUNDS>
__device__ __forceinline__ void sample_clip_quad_body(const SampleArgs<T>& a) {
    constexpr int PAIRS = HMAX / 8;   // Box-Muller pairs per lane
    typedef T T2 __attribute__((ext_vector_type(2)));
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    T* tile = reinterpret_cast<T*>(smem_raw);              // [tpw][h * d]
    const int hd = a.h * a.d;
    T* Wl = tile + (((size_t)a.tpw * hd + 1) & ~(size_t)1);   // [h][HMAX]
    const int tid = threadIdx.x;
    const int q = tid & 3, rowi = tid >> 2;
    const int n_base = blockIdx.x * a.tpw;
    const int n_here = min(a.tpw, a.n - n_base);
    const int rows = n_here * a.d;
    for (int e = tid; e < a.h * HMAX; e += WG) Wl[e] = a.W[e];
    const bool on = rowi < rows;
    const int nl = on ? rowi / a.d : 0;
    const int j = on ? rowi - nl * a.d : 0;
    T g[2 * PAIRS];   // entries m = 8 i + 2 q, 8 i + 2 q + 1 of the row's white draws
    {
        const int row_local = n_base + nl;
        if (a.zr != nullptr && a.white) {
#pragma unroll
            for (int i = 0; i < PAIRS; ++i)
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const int m = 8 * i + 2 * q + u;
                    g[2 * i + u] = m < a.h ? a.zr[((size_t)row_local * a.h + m) * a.d + j] : (T)0;
                }
        } else if (a.zr != nullptr) {
            const size_t base = ((size_t)row_local * a.d + j) * a.F;
#pragma unroll
            for (int i = 0; i < PAIRS; ++i)
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const int m = 8 * i + 2 * q + u;
                    T v = (T)0;
                    if (m < a.F)
                        v = a.zr[base + m];
                    else if (m < a.h)
                        v = a.zi[base + (m - a.F + 1)];
                    g[2 * i + u] = v;
                }
        } else {
            Xoshiro128pp rng = row_stream<ROUNDS>((uint32_t)(a.first_index + row_local), (uint32_t)j, a.off_lo, a.off_hi, a.seed_lo, a.seed_hi);
            // every lane of the quad walks the row's whole word stream (integer work) and KEEPS the words of its own pairs
            // (selects, no branch); the transforms -- the float64 work -- then run on all lanes at once, a quarter each
            uint32_t wa[PAIRS], wb[PAIRS];
#pragma unroll
            for (int p = 0; p < HMAX / 2; ++p) {
                const uint32_t xa = rng.next();
                const uint32_t xb = rng.next();
                if ((p & 3) == 0) {   // (p is a constant of the unrolled loop) the group's first pair: lane 0's, a placeholder for the others
                    wa[p >> 2] = xa;
                    wb[p >> 2] = xb;
                } else {
                    const bool mine = (p & 3) == q;
                    wa[p >> 2] = mine ? xa : wa[p >> 2];
                    wb[p >> 2] = mine ? xb : wb[p >> 2];
                }
            }
#pragma unroll
            for (int i = 0; i < PAIRS; ++i) {
                if (2 * (4 * i) < a.h)   // (wave-uniform up to the quad's offset: pairs past the horizon are zero)
                    box_muller(wa[i], wb[i], g[2 * i], g[2 * i + 1]);
                if (!(2 * (4 * i + q) < a.h)) g[2 * i] = g[2 * i + 1] = (T)0;
            }
        }
    }
    __syncthreads();
    const T lo = a.low[j], hi = a.high[j];
    for (int t = a.t_begin; t < a.h; ++t) {
        const T* __restrict__ w = Wl + (size_t)t * HMAX + 2 * q;
        T acc = (T)0;
#pragma unroll
        for (int i = 0; i < PAIRS; ++i) {
            const T2 wv = *reinterpret_cast<const T2*>(w + 8 * i);
            acc = fmad(g[2 * i], wv[0], acc);
            acc = fmad(g[2 * i + 1], wv[1], acc);
        }
        acc = acc + quad_swap<0xB1>(acc);   // quad_perm [1, 0, 3, 2]
        acc = acc + quad_swap<0x4E>(acc);   // quad_perm [2, 3, 0, 1]
        if (on && (t & 3) == q) {
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

// ---- K2: rollout + cost, one thread per trajectory / a row of lanes per trajectory -------------------------------------
__device__ __forceinline__ float act_tanh(float x) { return tanhf(x); }
__device__ __forceinline__ double act_tanh(double x) { return tanh(x); }

template <typename T, int O, int KIND>
__device__ __forceinline__ void rollout_cost_body(const RolloutArgs<T>& a) {
    const int n = blockIdx.x * WG + threadIdx.x;
    if (n >= a.n) return;
    T obs[O];
#pragma unroll
    for (int k = 0; k < O; ++k) obs[k] = k < a.o ? a.obs0[k] : (T)0;
    const T* __restrict__ act = a.actions + (size_t)n * a.h * a.d;
    const T* __restrict__ A = a.A;
    const T* __restrict__ B = a.B;
    T acc = (T)0;
    for (int t = 0; t < a.h; ++t) {
        T nxt[O];
#pragma unroll
        for (int i = 0; i < O; ++i) nxt[i] = (T)0;
#pragma unroll
        for (int k = 0; k < O; ++k) {
            const T ok = obs[k];
#pragma unroll
            for (int i = 0; i < O; ++i) nxt[i] = fmad(ok, A[k * O + i], nxt[i]);
        }
        T ctrl = (T)0;
        for (int j = 0; j < a.d; ++j) {
            const T aj = act[t * a.d + j];
            ctrl = fmad(aj, aj, ctrl);
#pragma unroll
            for (int i = 0; i < O; ++i) nxt[i] = fmad(aj, B[j * O + i], nxt[i]);
        }
        T lin = (T)0, ang = (T)0;
#pragma unroll
        for (int k = 0; k < O; ++k) {
            lin = (k == a.cs.lin_idx) ? obs[k] : lin;
            ang = (k == a.cs.flip_idx) ? obs[k] : ang;
        }
        T c = (T)0;
        if (a.cs.flip_idx >= 0) {
            c += (ang > a.cs.flip_th) ? a.cs.flip_pen : (T)0;
            c += (ang < -a.cs.flip_th) ? a.cs.flip_pen : (T)0;
        }
        c += a.cs.ctrl_w * ctrl;
        if (a.cs.lin_w != (T)0) c += a.cs.lin_w * lin;
        if (a.cs.ext) {
            bool bad = false;
#pragma unroll
            for (int k = 0; k < O; ++k) {
                if (k >= a.o) continue;
                bad |= !finite_val(obs[k]);
                if (a.cs.box_from >= 0 && k >= a.cs.box_from) bad |= !(a.cs.box_lo < obs[k] && obs[k] < a.cs.box_hi);
            }
            auto pick = [&](const T* v, int idx) {
                T r = (T)0;
#pragma unroll
                for (int k = 0; k < O; ++k) r = (k == idx) ? v[k] : r;
                return r;
            };
            T post[O];
#pragma unroll
            for (int i = 0; i < O; ++i) post[i] = (KIND == ICEM_MODEL_TANH) ? act_tanh(nxt[i]) : nxt[i];
            c += cost_terms<T>(a.cs, bad, [&](int idx) { return pick(obs, idx); }, [&](int idx) { return pick(post, idx); });
        }
        if (t == 0 || a.cost_mode == ICEM_COST_FINAL)
            acc = c;
        else if (a.cost_mode == ICEM_COST_SUM)
            acc += c;
        else
            acc = (c < acc || c != c) ? c : acc;  // np.amin: a NaN step cost makes the trajectory's cost NaN
        if (a.observations != nullptr) {
            T* dst = a.observations + ((size_t)n * a.h + t) * a.o;
#pragma unroll
            for (int k = 0; k < O; ++k)
                if (k < a.o) dst[k] = obs[k];
        }
#pragma unroll
        for (int i = 0; i < O; ++i) obs[i] = (KIND == ICEM_MODEL_TANH) ? act_tanh(nxt[i]) : nxt[i];
    }
    a.costs[n] = acc;
}

// The same rollout with a trajectory spread over LPT lanes (lane = observation column) instead of one thread per trajectory:
// in float64 a thread's horizon is 30 x (O + d) x O dependent 8-cycle FMAs -- 214 us per launch at N = 4096, three quarters
// of a strict-parity MPC step -- while 250 of the chip's 256 CUs hold one wave each.  Here lane c of a trajectory's row keeps
// column c of A in registers and accumulates output c over the SAME chain (k = 0 .. O - 1, then the actions, fused
// multiply-adds in that order: bit-identical to the thread form), the state goes from step to step through two LDS rows per
// trajectory (written by its lanes, read back as broadcasts by the same wave: no workgroup barrier in the loop), B sits in
// LDS, a chunk of the row's actions is staged in LDS.  Costs (icem_cost_spec's form; a term list keeps the thread form) are
// computed redundantly by every lane of the row (same instructions); lane 0 stores.  ICEM_GK_ROLLOUT=thread brings the thread
// form back (A/B, tests).
template <typename T, int O, int KIND>
__device__ __forceinline__ void rollout_cost_rows_body(const RolloutArgs<T>& a) {
    constexpr int LPT = O <= 16 ? 16 : 32;   // lanes per trajectory
    constexpr int TPW = WG / LPT;            // trajectories per workgroup
    constexpr int OS = (O + 1) & ~1;         // LDS row stride: pairs of entries are read as one 2 x T vector
    constexpr int BREG = 8;                  // action dims whose row of B stays in registers
    typedef T T2 __attribute__((ext_vector_type(2)));
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    T* xs = reinterpret_cast<T*>(smem_raw);  // [2][TPW][OS]: the state before / behind the running step
    T* Bs = xs + 2 * TPW * OS;               // [d][OS]
    const int ds = a.d <= BREG ? BREG : ((a.d + 1) & ~1);   // a step's actions in LDS, zero padded (to BREG: read whole, unconditionally)
    T* As = Bs + a.d * OS;                   // [TPW][ch * ds]: the next `ch` steps' actions of every trajectory of the workgroup
    const int tid = threadIdx.x, col = tid % LPT, tl = tid / LPT;
    const bool live_col = col < O;
    const int cc = live_col ? col : 0;
    const int n = blockIdx.x * TPW + tl;
    const bool live = n < a.n;
    long long* const dbg = (blockIdx.x == 0 && tid == 0) ? a.dbg : nullptr;
    if (dbg) dbg[24] = wall_clock64();
    for (int e = tid; e < a.d * O; e += WG) Bs[(e / O) * OS + e % O] = a.B[e];
    T Acol[O];
#pragma unroll
    for (int k = 0; k < O; ++k) Acol[k] = live_col ? a.A[k * O + cc] : (T)0;
    T Bcol[BREG];
#pragma unroll
    for (int j = 0; j < BREG; ++j) Bcol[j] = (live_col && j < a.d) ? a.B[j * O + cc] : (T)0;
    if (tid < TPW * OS) xs[tid] = (T)0;
    __syncthreads();
    if (live_col) xs[tl * OS + col] = col < a.o ? a.obs0[col] : (T)0;
    if (O < OS && col == 0) xs[TPW * OS + tl * OS + O] = (T)0;   // (the pad entry of the second buffer: read, never written)
    __syncthreads();
    if (dbg) dbg[25] = wall_clock64();
    const T* __restrict__ act_g = a.actions + (size_t)(live ? n : a.n - 1) * a.h * a.d;
    const int lane = tid & 63;
    const unsigned long long row_mask = (LPT == 64 ? ~0ull : ((1ull << LPT) - 1ull)) << ((lane / LPT) * LPT);
    const int ch = a.ch;                     // steps per staged chunk (host: the whole horizon where it fits)
    T* my_acts = As + (size_t)tl * ch * ds;
    const bool b_regs = a.d <= BREG;
    // (the cost's scalars as locals: the argument block's term list must not be live across the loop -- with it in reach the
    //  step restored 600 spilled scalar registers through v_readlane, 1.1 us per step whatever the arithmetic.  Costs with a
    //  term list -- cs.ext -- keep the thread form: launch_rollout_k)
    const T flip_th = a.cs.flip_th, flip_pen = a.cs.flip_pen, ctrl_w = a.cs.ctrl_w, lin_w = a.cs.lin_w;
    const int lin_idx = a.cs.lin_idx, flip_idx = a.cs.flip_idx, cost_mode = a.cost_mode, hh = a.h, dd = a.d, oo = a.o;
    T* const obs_out = a.observations;
    T acc = (T)0;
    for (int t = 0; t < hh; ++t) {
        if (t % ch == 0) {
            // the row's lanes fetch their trajectory's next chunk (one coalesced span: a step's actions straight from HBM were
            // a cold miss every other step -- 1.5 us per step, 44 us per launch); same wave writes and reads: no workgroup barrier
            const int cnt = (hh - t < ch ? hh - t : ch) * dd;
            // (eight loads in flight per lane: one at a time, each a cold miss, was 0.6 us per step of the horizon)
            for (int e0 = col; e0 < cnt; e0 += 8 * LPT) {
                T v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) v[u] = act_g[t * dd + (e0 + u * LPT < cnt ? e0 + u * LPT : 0)];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int e = e0 + u * LPT;
                    if (e < cnt) my_acts[(e / dd) * ds + e % dd] = v[u];
                }
            }
            for (int e = col; e < ch * (ds - dd); e += LPT) my_acts[(e / (ds - dd)) * ds + dd + e % (ds - dd)] = (T)0;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
        if (dbg && t < 3) dbg[26 + t] = wall_clock64();
        const T* act = my_acts + (t % ch) * ds;
        const T* pre = xs + ((t & 1) * TPW + tl) * OS;
        T* post = xs + (((t + 1) & 1) * TPW + tl) * OS;
        // the whole state and the step's actions in a few wide broadcast reads, THEN the chain (the LDS pipe of a CU that
        // holds eight such waves was the bound with one read per entry: 0.4 us of every step)
        T xk[OS], av[BREG];
#pragma unroll
        for (int k = 0; k < OS; k += 2) {
            const T2 v = *reinterpret_cast<const T2*>(pre + k);
            xk[k] = v[0];
            xk[k + 1] = v[1];
        }
        if (b_regs) {   // the step's actions ride the same wait (the row is padded to BREG entries)
#pragma unroll
            for (int j = 0; j < BREG; j += 2) {
                const T2 v = *reinterpret_cast<const T2*>(act + j);
                av[j] = v[0];
                av[j + 1] = v[1];
            }
        }
        T nx = (T)0;
#pragma unroll
        for (int k = 0; k < O; ++k) nx = fmad(xk[k], Acol[k], nx);
        T ctrl = (T)0;
        if (b_regs) {
#pragma unroll
            for (int j = 0; j < BREG; ++j) {
                if (j < dd) {   // (wave-uniform; the padding entries take no part: an exact zero keeps its sign)
                    ctrl = fmad(av[j], av[j], ctrl);
                    nx = fmad(av[j], Bcol[j], nx);
                }
            }
        } else {
            for (int j = 0; j < dd; ++j) {
                const T aj = act[j];
                ctrl = fmad(aj, aj, ctrl);
                nx = fmad(aj, Bs[j * OS + cc], nx);
            }
        }
        const T pv = (KIND == ICEM_MODEL_TANH) ? act_tanh(nx) : nx;
        if (live_col) post[col] = pv;
        // (two more LDS reads, not a select chain over the registers: 34 compare masks do not fit the scalar registers)
        const T lin = (lin_idx >= 0 && lin_idx < O) ? pre[lin_idx] : (T)0;
        const T ang = (flip_idx >= 0 && flip_idx < O) ? pre[flip_idx] : (T)0;
        T c = (T)0;
        if (flip_idx >= 0) {
            c += (ang > flip_th) ? flip_pen : (T)0;
            c += (ang < -flip_th) ? flip_pen : (T)0;
        }
        c += ctrl_w * ctrl;
        if (lin_w != (T)0) c += lin_w * lin;
        if (t == 0 || cost_mode == ICEM_COST_FINAL)
            acc = c;
        else if (cost_mode == ICEM_COST_SUM)
            acc += c;
        else
            acc = (c < acc || c != c) ? c : acc;  // np.amin: a NaN step cost makes the trajectory's cost NaN
        if (obs_out != nullptr && live && live_col && col < oo)
            obs_out[((size_t)n * hh + t) * oo + col] = pre[col];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    if (live && col == 0) a.costs[n] = acc;
    if (dbg) dbg[29] = wall_clock64();
}

// ---- K3: sorted top-k helpers ------------------------------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ void wave_min_key(T& c, int& i) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        const T oc = __shfl_xor(c, s, 64);
        const int oi = __shfl_xor(i, s, 64);
        if (key_less(oc, oi, c, i)) {
            c = oc;
            i = oi;
        }
    }
}

// getc(e)/geti(e) expose `cnt` keys; winners go to out_c/out_i[0..K) (any address space),
// `slot(e)` is returned through out_e (position of the winner in the key array) when non-null.
template <typename T, typename GetC, typename GetI>
__device__ __forceinline__ void block_select_sorted(int cnt, int K, GetC getc, GetI geti, T* out_c, int* out_i,
                                                    int* out_e, T* red_c, int* red_i, int* red_e) {
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    T pc = -inf_v<T>();
    int pi = -1;
    for (int r = 0; r < K; ++r) {
        T bc = inf_v<T>();
        int bi = INT_MAX, be = -1;
        for (int e = tid; e < cnt; e += WG) {
            const T c = getc(e);
            const int i = geti(e);
            const bool after_prev = c > pc || (c == pc && i > pi);
            if (after_prev && key_less(c, i, bc, bi)) {
                bc = c;
                bi = i;
                be = e;
            }
        }
        // reduce (bc, bi); carry `be` along with the winner
        T wc = bc;
        int wi = bi;
        wave_min_key(wc, wi);
        const bool mine = (wc == bc && wi == bi);
        // several lanes can hold the sentinel; the lowest such lane reports
        const unsigned long long m = __ballot(mine);
        if (mine && lane == __ffsll((long long)m) - 1) {
            red_c[wave] = bc;
            red_i[wave] = bi;
            red_e[wave] = be;
        }
        __syncthreads();
        T fc = red_c[0];
        int fi = red_i[0], fe = red_e[0];
#pragma unroll
        for (int w = 1; w < WG / 64; ++w) {
            if (key_less(red_c[w], red_i[w], fc, fi)) {
                fc = red_c[w];
                fi = red_i[w];
                fe = red_e[w];
            }
        }
        if (tid == 0) {
            out_c[r] = fc;
            out_i[r] = fi;
            if (out_e != nullptr) out_e[r] = fe;
        }
        pc = fc;
        pi = fi;
        __syncthreads();
    }
}

template <typename T>
__device__ __forceinline__ T nan_to_inf(T c) {
    return c != c ? inf_v<T>() : c;
}

// ---- fused-step glue -----------------------------------------------------------------------------------------------------
// icem.py:97-100: rows [0, n_reuse) of dst <- elites[e, 1:, :] (the last time step is sampled after).
template <typename T>
__device__ __forceinline__ void shift_elites_body(int n_reuse, int h, int d, const T* elites, T* dst) {
    const int hd = h * d;
    const int total = n_reuse * (hd - d);
    for (int x = blockIdx.x * WG + threadIdx.x; x < total; x += gridDim.x * WG) {
        const int e = x / (hd - d);
        const int r = x - e * (hd - d);
        dst[(size_t)e * hd + r] = elites[(size_t)e * hd + d + r];
    }
}

// ---------------------------------------------------------------------------------------------
// K3 + K4 of a single-GPU step in ONE launch: threshold selection + gather + refit
// ---------------------------------------------------------------------------------------------
// topk_partial -> local_pack -> merge_refit are three launches of K rounds of a workgroup-wide minimum each (two barriers
// per round): 46 us per iteration in float64 for work that is a few hundred compares.  One workgroup, the selection by
// THRESHOLD (as the f32 merges do): every thread's best key, the K-th smallest of a wave's 64 bests (K rounds of a wave
// minimum over order-preserving 64-bit images of the costs) is an upper bound of the K-th smallest key overall, the tightest
// of the waves' bounds is T; the keys at or below T (K .. a few dozen) are collected and PLACED by counting -- a key's place
// is the number of smaller keys (cost, then global index: np.argsort's order on distinct indices) -- and the K rows are
// gathered and refitted exactly as merge_refit_kernel does (same refit_element, same epilogue).  Same elites, same bits.
__device__ __forceinline__ unsigned long long order_image(double c) {   // monotone: c1 < c2  <=>  image(c1) < image(c2); -0 == +0
    c = c == 0.0 ? 0.0 : c;
    const unsigned long long b = (unsigned long long)__double_as_longlong(c);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ unsigned long long order_image(float c) { return order_image((double)c); }   // (exact widening)

__device__ __forceinline__ unsigned long long wave_min_u64_shfl(unsigned long long x) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        const unsigned long long o = __shfl_xor(x, s, 64);
        x = o < x ? o : x;
    }
    return x;
}

// idx_out (icem_plan_step_cem, k_cem.hip): where the K selected global indices go as well; the step kernels pass none.
template <typename T>
__device__ __forceinline__ void select_refit_body(const SelectArgs<T>& s, int* idx_out = nullptr) {
    constexpr int NW = SELECT_NT / 64;
    __shared__ unsigned long long wave_T[NW];
    __shared__ unsigned long long wave_best[NW][64];
    __shared__ T cand_c[SELECT_CAP];
    __shared__ int cand_i[SELECT_CAP];
    __shared__ int cand_e[SELECT_CAP];
    __shared__ int n_c;
    __shared__ T sel_c[ICEM_MAX_ELITES];
    __shared__ int sel_i[ICEM_MAX_ELITES];
    __shared__ int sel_e[ICEM_MAX_ELITES];
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    T* new_mean = reinterpret_cast<T*>(smem_raw);  // [hd]
    const MergeArgs<T>& a = s.m;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int total = s.n_cand + a.n_keep;
    auto cost_of = [&](int e) -> T { return e < s.n_cand ? nan_to_inf(s.costs[e]) : a.elites_cost_cur[e - s.n_cand]; };
    auto gidx_of = [&](int e) -> int { return e < s.n_loc ? e : a.n_global + (e < s.n_cand ? e - s.n_loc : e - s.n_cand); };
    if (s.dbg && tid == 0) s.dbg[16] = wall_clock64();
    if (tid == 0) n_c = 0;
    if (tid < ICEM_MAX_ELITES) {
        sel_c[tid] = inf_v<T>();
        sel_i[tid] = INT_MAX;
        sel_e[tid] = -1;
    }
    // every thread's best cost (image), then the K-th smallest of the wave's 64
    // (loads in batches of eight, all requested before the first is used: one thread's keys are 2 KB apart -- a cold miss
    //  each, and a loop of dependent misses was 16 us of this kernel)
    unsigned long long best = ~0ull;
    constexpr int KEEP = 16;             // a thread's first keys stay in registers for the second pass (all of them up to 4096 keys)
    T kept[KEEP];
#pragma unroll
    for (int b = 0; b < KEEP / 8; ++b) {
        const int e0 = tid + b * 8 * SELECT_NT;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int e = e0 + u * SELECT_NT;
            kept[b * 8 + u] = cost_of(e < total ? e : 0);
        }
    }
#pragma unroll
    for (int q = 0; q < KEEP; ++q) {
        const unsigned long long v = tid + q * SELECT_NT < total ? order_image(kept[q]) : ~0ull;
        best = v < best ? v : best;
    }
    for (int e0 = tid + KEEP * SELECT_NT; e0 < total; e0 += 8 * SELECT_NT) {
        T cv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int e = e0 + u * SELECT_NT;
            cv[u] = cost_of(e < total ? e : tid);
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const unsigned long long v = e0 + u * SELECT_NT < total ? order_image(cv[u]) : ~0ull;
            best = v < best ? v : best;
        }
    }
    if (s.dbg && tid == 0) s.dbg[17] = wall_clock64();
    // ... by counting: a lane's rank among the wave's 64 (value, then lane) is the number of smaller ones -- 64 broadcast
    // reads, no dependent cross-lane chain (K rounds of a shuffled 64-bit minimum cost 5 us)
    wave_best[wave][lane] = best;
    if (lane == 0) wave_T[wave] = ~0ull;   // fewer than K threads with a key: everything is a candidate
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    int rank = 0;
#pragma unroll 8
    for (int j = 0; j < 64; ++j) {
        const unsigned long long o = wave_best[wave][j];
        rank += (o < best || (o == best && j < lane)) ? 1 : 0;
    }
    if (rank == a.K - 1 && best != ~0ull) wave_T[wave] = best;
    __syncthreads();
    if (s.dbg && tid == 0) s.dbg[18] = wall_clock64();
    unsigned long long Tt = wave_T[0];
#pragma unroll
    for (int w = 1; w < NW; ++w) Tt = wave_T[w] < Tt ? wave_T[w] : Tt;
    // the keys at or below the threshold (costs that tie with it all survive)
#pragma unroll
    for (int q = 0; q < KEEP; ++q) {
        const int e = tid + q * SELECT_NT;
        if (e < total && order_image(kept[q]) <= Tt) {
            const int pos = atomicAdd(&n_c, 1);
            if (pos < s.cap) {
                cand_c[pos] = kept[q];
                cand_i[pos] = gidx_of(e);
                cand_e[pos] = e;
            }
        }
    }
    for (int e0 = tid + KEEP * SELECT_NT; e0 < total; e0 += 8 * SELECT_NT) {
        T cv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int e = e0 + u * SELECT_NT;
            cv[u] = cost_of(e < total ? e : tid);
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int e = e0 + u * SELECT_NT;
            if (e < total && order_image(cv[u]) <= Tt) {
                const int pos = atomicAdd(&n_c, 1);
                if (pos < s.cap) {
                    cand_c[pos] = cv[u];
                    cand_i[pos] = gidx_of(e);
                    cand_e[pos] = e;
                }
            }
        }
    }
    __syncthreads();
    if (s.dbg && tid == 0) s.dbg[19] = wall_clock64();
    // More keys at or below the threshold than the candidate array holds: costs that TIE with it in bulk (a collapsed
    // distribution -- every trajectory the same --, a population of NaNs).  Which of them landed in the array is a race, and
    // np.argsort's order among equal costs is by index: take the three-launch path's selection instead (K rounds of a
    // workgroup-wide minimum over all keys: deterministic, slow, rare).
    if (n_c > s.cap) {
        __shared__ T red_c[SELECT_NT / 64];
        __shared__ int red_i[SELECT_NT / 64];
        __shared__ int red_e[SELECT_NT / 64];
        static_assert(SELECT_NT == WG, "block_select_sorted strides by WG");
        block_select_sorted<T>(total, a.K, cost_of, gidx_of, sel_c, sel_i, sel_e, red_c, red_i, red_e);
        __syncthreads();
    }
    const int nc = n_c <= s.cap ? n_c : 0;   // (overflow: the selection above stands, nothing is placed)
    for (int i = tid; i < nc; i += SELECT_NT) {
        const T c = cand_c[i];
        const int g = cand_i[i];
        int place = 0;
#pragma unroll 8
        for (int j = 0; j < nc; ++j) place += key_less(cand_c[j], cand_i[j], c, g) ? 1 : 0;
        if (place < a.K) {
            sel_c[place] = c;
            sel_i[place] = g;
            sel_e[place] = cand_e[i];
        }
    }
    __syncthreads();
    if (s.dbg && tid == 0) {
        s.dbg[20] = wall_clock64();
        s.dbg[23] = nc;
    }
    const int hd = a.h * a.d;
    auto src_row = [&](int r) -> const T* {
        int e = sel_e[r];
        if (e < 0) e = sel_e[0];  // fewer than K live candidates (cannot happen for K <= N / 2): repeat the best
        return e < s.n_cand ? s.actions + (size_t)e * hd : a.elites_cur + (size_t)(e - s.n_cand) * hd;
    };
    constexpr int KR = 16;   // elite rows gathered into registers at once (K <= KR: every load requested before the first use)
    for (int e = tid; e < hd; e += SELECT_NT) {
        T nm, ns;
        if (a.K <= KR) {
            T xr[KR];
#pragma unroll
            for (int r = 0; r < KR; ++r) xr[r] = src_row(r < a.K ? r : 0)[e];
            const T om = a.mean_in[e], os = a.std_in[e];
#pragma unroll
            for (int r = 0; r < KR; ++r)
                if (r < a.K) a.elites_next[(size_t)r * hd + e] = xr[r];
            refit_element_regs<T, KR>(a.K, a.alpha, om, os, xr, nm, ns);
        } else {
            for (int r = 0; r < a.K; ++r) a.elites_next[(size_t)r * hd + e] = src_row(r)[e];
            refit_element<T>(a.K, a.alpha, a.mean_in[e], a.std_in[e], [&](int r) { return src_row(r)[e]; }, nm, ns);
        }
        if (!a.last) {
            a.mean[e] = nm;
            a.std[e] = ns;
        } else {
            new_mean[e] = nm;
        }
    }
    if (tid < a.K) a.elites_cost_next[tid] = sel_c[tid];
    if (idx_out != nullptr && tid < a.K) idx_out[tid] = sel_i[tid];
    if (s.dbg && tid == 0) s.dbg[21] = wall_clock64();
    if (a.last) {
        __syncthreads();
        for (int e = tid; e < hd; e += SELECT_NT) {
            const int j = e % a.d;
            a.mean[e] = (e + a.d < hd) ? new_mean[e + a.d] : new_mean[e];
            a.std[e] = (a.high[j] - a.low[j]) / (T)2 * a.init_std;
        }
        if (tid < a.d) a.executed[tid] = src_row(0)[tid];
        if (tid == 0) a.best_cost[0] = sel_c[0];
    }
}

}  // namespace icem
