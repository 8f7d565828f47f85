// See icem_mlp.h.  The structure of icem_rssm.hip's fused kernel: one workgroup (8 wavefronts) per tile of 16 trajectories, every
// layer D = W-block . X^T with v_mfma_f32_16x16x32_bf16 (A operand: a 16 x 32 block of the weight, streamed from L2; B operand:
// the activations of the 16 trajectories from LDS; lane (j, g) is left with outputs 4g .. 4g+3 of trajectory j and writes
// them -- bias added, activation applied, rounded to bf16 -- to the LDS row the next layer reads).  The state lives in LDS in f32,
// twice: s_t and s_{t+1}, so that the step cost c(s_t, a_t, s_{t+1}) is evaluated per row in f32 by ONE wave while the others
// already run the input layer of the next step.  State and hidden activations are rounded to bf16 only as matrix operands.
#include "icem_mlp.h"
#include "rssm_dev.h"
#include "cost_terms_dev.h"

namespace icem {
namespace {
using namespace rssm_dev;
static_assert(mlp::HIDB == HIDB && mlp::HIDK == HIDK && mlp::BLK == BLK, "the hidden layers use the RSSM's 13 x 7 block shape");

constexpr int SS = 68;   // f32 row stride of the state (64 + 4: rows start in different banks)
constexpr int AS = 32;   // f32 row stride of a step's actions

// The rollout of ONE tile of 16 trajectories -- rows base .. base + 15 of a problem of n rows -- by one workgroup: the body of
// both kernels below.  Pg, obs0, actions, costs and obs_out are the PROBLEM's: its parameter buffer, its start observation, its
// first action row, its first cost (and first state row).  Everything is wave-uniform.
// SK: the 32-wide K blocks of the state (1: obs_dim <= 32, 2: <= 64); ACTV: mlp::RELU / mlp::SWISH.  Everything else is a
// runtime value: o = obs_dim, d = act_dim, L = the number of hidden layers, the horizon, the cost, `observations`.
template <int SK, int ACTV>
__device__ __forceinline__ void mlp_rollout_tile(const int base, const int n, const int horizon, const int o, const int d, const int L,
                                                 const int cost_mode, const CostArgs<float>& cs_arg, const unsigned short* __restrict__ Pg,
                                                 const float* __restrict__ obs0, const float* __restrict__ actions,
                                                 float* __restrict__ costs, float* __restrict__ obs_out) {
    // the cost's argument block goes to LDS once: left in the kernel arguments its term list stays live in scalar registers
    // across the whole step loop (500 of them spilled to lanes of vector registers and restored every step)
    __shared__ CostArgs<float> cs;
    if (threadIdx.x == 0) cs = cs_arg;
    const bool reads_last = cs_arg.ext && cs_arg.diff_idx >= 0;   // the difference term reads s_h
    constexpr int K1 = SK + 1;            // K blocks of [s | a]
    constexpr int XS = 32 * K1 + 8;       // bf16 row stride of [s | a]
    __shared__ __attribute__((aligned(16))) unsigned short sA[16 * XS];      // [s_t | a_t] as the input layer's operand
    __shared__ __attribute__((aligned(16))) unsigned short xb[2][16 * RS];   // hidden activations, ping-pong
    __shared__ __attribute__((aligned(16))) float s32[2][16 * SS];           // s_t (buffer t & 1) and s_{t+1} in f32
    __shared__ __attribute__((aligned(16))) float aF[2][16 * AS];            // a_t in f32 (buffer t & 1): the control cost
    __shared__ __attribute__((aligned(16))) float bs[16 * HIDB * mlp::LAYERS_MAX + mlp::OBS_MAX];   // all biases
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform: block addresses stay scalar
    const int j = lane & 15, g = lane >> 4;
    const int OB = mlp::state_oblocks(o);
    const size_t first = mlp::first_units(SK), hid = mlp::hidden_units();
    const size_t wout = first + (size_t)(L - 1) * hid;        // Wout's offset; its bias sits OB * HIDK * BLK behind
    // padding trajectories of the last tile repeat row n - 1 and are never stored
    const int row = base + j;
    const size_t arow = (size_t)(row < n ? row : n - 1) * horizon * d;
    // ---- initial state: every trajectory starts from obs0 ----
    for (int e = tid; e < 16 * RS; e += NTHR) xb[0][e] = xb[1][e] = 0;
    for (int e = tid; e < 16 * SS; e += NTHR) {
        const int k = e % SS;
        s32[0][e] = k < o ? obs0[k] : 0.f;
        s32[1][e] = 0.f;
    }
    for (int e = tid; e < 16 * XS; e += NTHR) {
        const int k = e % XS, jj = e / XS;
        float v = 0.f;
        if (k < o) v = obs0[k];
        else if (k >= 32 * SK && k < 32 * SK + d) v = actions[(size_t)(base + jj < n ? base + jj : n - 1) * horizon * d + (k - 32 * SK)];
        sA[e] = to_bf16(v);
    }
    for (int e = tid; e < 16 * AS; e += NTHR) {
        const int k = e % AS, jj = e / AS;
        aF[0][e] = k < d ? actions[(size_t)(base + jj < n ? base + jj : n - 1) * horizon * d + k] : 0.f;
        aF[1][e] = 0.f;
    }
    for (int l = 0; l < L; ++l) {
        const float* b = reinterpret_cast<const float*>(Pg + (l == 0 ? first : first + (size_t)l * hid) - 2 * 16 * HIDB);
        for (int e = tid; e < 16 * HIDB; e += NTHR) bs[l * 16 * HIDB + e] = b[e];
    }
    {
        const float* b = reinterpret_cast<const float*>(Pg + wout + (size_t)OB * HIDK * BLK);
        for (int e = tid; e < 16 * OB; e += NTHR) bs[L * 16 * HIDB + e] = b[e];
    }
    if (obs_out != nullptr)
        for (int e = tid; e < 16 * o; e += NTHR) {
            const int jj = e / o, k = e - jj * o;
            if (base + jj < n) obs_out[(size_t)(base + jj) * (horizon + 1) * o + k] = obs0[k];
        }
    __syncthreads();
    const int xr = j * RS + 8 * g, zr = j * XS + 8 * g;   // operand reads: 8 bf16 of a 32-wide k-block
    const int xo = j * RS + 4 * g;                        // result writes: 4 outputs of a 16-wide block
    // ---- the cost of step t, by wave WAVES - 1 (it owns one block less than waves 0 .. 4): c(s_t, a_t, s_{t+1}) per row in f32,
    //      icem_cost_spec's form in generic_dev.h's spelling + the term list; the four lanes of a row share the sweep for `bad`
    //      and compute everything else alike, lane (j, 0) keeps the result ----
    float acc_cost = 0.f;
    auto score = [&](int t) {
        const float* pre = s32[t & 1] + j * SS;
        const float* post = s32[(t + 1) & 1] + j * SS;
        const float* af = aF[t & 1] + j * AS;
        float ctrl = 0.f;
        for (int k = 0; k < d; ++k) ctrl = fmad(af[k], af[k], ctrl);
        float c = 0.f;
        if (cs.flip_idx >= 0) {
            const float ang = pre[cs.flip_idx];
            c += (ang > cs.flip_th) ? cs.flip_pen : 0.f;
            c += (ang < -cs.flip_th) ? cs.flip_pen : 0.f;
        }
        c += cs.ctrl_w * ctrl;
        if (cs.lin_w != 0.f) c += cs.lin_w * pre[cs.lin_idx];
        if (cs.ext) {
            int bad = 0;
            for (int k = g; k < o; k += 4) {
                const float v = pre[k];
                bad |= !finite_val(v);
                if (cs.box_from >= 0 && k >= cs.box_from) bad |= !(cs.box_lo < v && v < cs.box_hi);
            }
            bad |= __shfl_xor(bad, 16, 64);
            bad |= __shfl_xor(bad, 32, 64);
            c += cost_terms<float>(cs, bad != 0, [&](int idx) { return pre[idx]; }, [&](int idx) { return post[idx]; });
        }
        if (t == 0 || cost_mode == ICEM_COST_FINAL) acc_cost = c;
        else if (cost_mode == ICEM_COST_SUM) acc_cost += c;
        else acc_cost = (c < acc_cost || c != c) ? c : acc_cost;   // np.amin: a NaN step cost makes the trajectory's cost NaN
    };
    // The last transition is computed only where something reads s_h: the difference term, or the caller.
    const int steps = (obs_out != nullptr || reads_last) ? horizon : horizon - 1;
    v4i A1[NOB][K1], Ah[NOB][HIDK];
    // what follows the input layer: hidden layer 2, or the output layer (waves without a block of it ask for block 0)
    auto req_next = [&](gptr Plane, int next /* 1 .. L: the layer's 0-based index, L = the output layer */) {
        __builtin_amdgcn_sched_barrier(0);
        if (next < L) {
#pragma unroll
            for (int i = 0; i < NOB; ++i) request<HIDK>(Plane + first + (size_t)(next - 1) * hid + (size_t)own_block(w, i) * HIDK * BLK, Ah[i]);
        } else {
#pragma unroll
            for (int i = 0; i < NOB; ++i) request<HIDK>(Plane + wout + (size_t)(w < OB ? w : 0) * HIDK * BLK, Ah[i]);
        }
        __builtin_amdgcn_sched_barrier(0);
    };
    req_own<K1>((gptr)Pg + lane * 8, 0, w, A1);
    for (int t = 0; t < steps; ++t) {
        // the parameters do not depend on t: re-derive the pointer behind an opaque barrier every step, or the optimizer
        // keeps whatever fits of them in registers across steps (icem_rssm.hip)
        gptr P = (gptr)Pg;
        asm volatile("" : "+s"(P));
        gptr Plane = P + lane * 8;   // this lane's 8 bf16 inside every A-operand block
        // the next step's actions: asked for now, staged behind the output layer
        float an[4] = {0.f, 0.f, 0.f, 0.f};
        const int e0 = (w - 4) * 16 + 4 * g;
        if ((w == 4 || w == 5) && t + 1 < horizon) {
#pragma unroll
            for (int r = 0; r < 4; ++r) an[r] = e0 + r < d ? actions[arow + (size_t)(t + 1) * d + e0 + r] : 0.f;
        }
        // ---- input layer (reads [s_t | a_t]): x1 = act(W1 [s | a] + b1); the cost of step t - 1 beside it ----
        req_next(Plane, 1);   // in flight across the barrier
        if (w == WAVES - 1 && t > 0) score(t - 1);
        fin_dense_act<K1, 1, ACTV>(bs, A1, sA + zr, 0, xb[0] + xo, w, g);
        __syncthreads();
        int p = 0;
        for (int l = 1; l < L; ++l) {   // ---- hidden layer l + 1 ----
            fin_dense_act<HIDK, 1, ACTV>(bs + l * 16 * HIDB, Ah, xb[p] + xr, 0, xb[p ^ 1] + xo, w, g);
            req_next(Plane, l + 1);
            __syncthreads();
            p ^= 1;
        }
        // ---- output layer (waves 0 .. OB - 1): s_{t+1} = s_t + Wout x + bout in f32; waves 4, 5: a_{t+1} -> [s | a] ----
        req_own<K1>(Plane, 0, w, A1);   // the next step's input layer (always: a request that is always made leaves nothing to keep alive)
        if (w < OB) {
            const int k0 = w * 16 + 4 * g;
            const v4f b = *reinterpret_cast<const v4f*>(bs + L * 16 * HIDB + k0);
            const v4f a = mma<HIDK>(Ah[0], xb[p] + xr, b);
            const v4f old = *reinterpret_cast<const v4f*>(s32[t & 1] + j * SS + k0);
            v4f nw;
#pragma unroll
            for (int r = 0; r < 4; ++r) nw[r] = old[r] + a[r];
            *reinterpret_cast<v4f*>(s32[(t + 1) & 1] + j * SS + k0) = nw;
            *reinterpret_cast<v4s*>(sA + j * XS + k0) = pack4(nw[0], nw[1], nw[2], nw[3]);
            if (obs_out != nullptr && row < n) {
                float* dst = obs_out + ((size_t)row * (horizon + 1) + (t + 1)) * o;
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (k0 + r < o) dst[k0 + r] = nw[r];
            }
        } else if ((w == 4 || w == 5) && t + 1 < horizon) {
            *reinterpret_cast<v4s*>(sA + j * XS + 32 * SK + e0) = pack4(an[0], an[1], an[2], an[3]);
            *reinterpret_cast<v4f*>(aF[(t + 1) & 1] + j * AS + e0) = v4f{an[0], an[1], an[2], an[3]};
        }
        __syncthreads();
    }
    if (w == WAVES - 1) {
        for (int t = steps > 0 ? steps - 1 : 0; t < horizon; ++t) score(t);
        if (g == 0 && row < n) costs[row] = acc_cost;
    }
}

// One problem: workgroup b rolls out rows 16 b .. 16 b + 15 of the launch's n.
template <int SK, int ACTV>
__global__ __launch_bounds__(NTHR) void mlp_rollout_kernel(int n, int horizon, int o, int d, int L, int cost_mode, CostArgs<float> cs_arg,
                                                          const unsigned short* __restrict__ Pg, const float* __restrict__ obs0,
                                                          const float* __restrict__ actions, float* __restrict__ costs,
                                                          float* __restrict__ obs_out) {
    mlp_rollout_tile<SK, ACTV>(blockIdx.x * 16, n, horizon, o, d, L, cost_mode, cs_arg, Pg, obs0, actions, costs, obs_out);
}

// The problems of a launch in which every problem names its OWN model, by value in the kernel arguments (icem_rssm_split.hip's
// ModelsTable; 1152 bytes).  Problem p owns the workgroups wg0[p] .. wg0[p] + ceil(rows[p] / 16) - 1; its rows[p] trajectories are
// the ACTION rows arow0[p] .. (several problems may name the same rows: an ensemble's members score one population) and the
// COST rows crow0[p] .. (back to back in problem order, not rounded to 16; the rows of `observations` alike); it starts from
// row obs[p] of the observation table and runs through the packed parameter buffer params[p].
struct MlpTable {
    gptr params[mlp::PROBLEMS_MAX];   // (declared global: read out of the kernel arguments as generic ones, every access behind them would be FLAT)
    long long arow0[mlp::PROBLEMS_MAX], crow0[mlp::PROBLEMS_MAX];
    int wg0[mlp::PROBLEMS_MAX], rows[mlp::PROBLEMS_MAX], obs[mlp::PROBLEMS_MAX];
};

// mlp_rollout_kernel with a problem table in front.  A workgroup finds its problem ONCE, here: a wave-uniform scan over the
// (at most 32) first workgroups, kept scalar; behind it only the problem's five values are live -- its parameters, its
// observation, its first action row, its row count, its first cost row -- and mlp_rollout_tile runs on them as it does on the
// solo kernel's arguments: a tile holds 16 rows of ONE problem in the problem's own order (the padding rows of a problem's
// last tile repeat ITS last row and are never stored), so every cost and state is bit for bit the solo launch's.
template <int SK, int ACTV>
__global__ __launch_bounds__(NTHR) void mlp_rollout_models_kernel(const MlpTable tab, int n_problems, int horizon, int o, int d, int L,
                                                                 int cost_mode, CostArgs<float> cs_arg, const float* __restrict__ obs0,
                                                                 const float* __restrict__ actions, float* __restrict__ costs,
                                                                 float* __restrict__ obs_out) {
    const int b = blockIdx.x;
    int p = 0;
    for (int q = 1; q < n_problems; ++q) p = b >= tab.wg0[q] ? q : p;
    p = __builtin_amdgcn_readfirstlane(p);
    const long long crow0 = tab.crow0[p];
    mlp_rollout_tile<SK, ACTV>((b - tab.wg0[p]) * 16, tab.rows[p], horizon, o, d, L, cost_mode, cs_arg, (const unsigned short*)tab.params[p],
                               obs0 + (size_t)tab.obs[p] * o, actions + (size_t)tab.arow0[p] * horizon * d, costs + crow0,
                               obs_out != nullptr ? obs_out + (size_t)crow0 * (horizon + 1) * o : nullptr);
}
}  // namespace

hipError_t launch_mlp_rollout(int n, int horizon, int obs_dim, int act_dim, int layers, int activation, int cost_mode,
                              const CostArgs<float>& cs, const unsigned short* params, const float* obs0, const float* actions,
                              float* costs, float* observations, hipStream_t st) {
    if (!mlp::shape_ok(obs_dim, act_dim, layers) || horizon < 1 || (activation != mlp::RELU && activation != mlp::SWISH))
        return hipErrorInvalidValue;
    if (n <= 0) return hipSuccess;
    const dim3 grid((n + 15) / 16), block(NTHR);
    const int sk = mlp::state_kblocks(obs_dim);
#define ICEM_MLP_LAUNCH(SKV, AV)                                                                                                   \
    hipLaunchKernelGGL((mlp_rollout_kernel<SKV, AV>), grid, block, 0, st, n, horizon, obs_dim, act_dim, layers, cost_mode, cs, params, \
                       obs0, actions, costs, observations)
    if (sk == 1 && activation == mlp::RELU) ICEM_MLP_LAUNCH(1, mlp::RELU);
    else if (sk == 1) ICEM_MLP_LAUNCH(1, mlp::SWISH);
    else if (activation == mlp::RELU) ICEM_MLP_LAUNCH(2, mlp::RELU);
    else ICEM_MLP_LAUNCH(2, mlp::SWISH);
#undef ICEM_MLP_LAUNCH
    return hipGetLastError();
}

hipError_t launch_mlp_rollout_models(int n_problems, const mlp::Problem* problems, int horizon, int obs_dim, int act_dim, int layers,
                                     int activation, int cost_mode, const CostArgs<float>& cs, const float* obs0, const float* actions,
                                     float* costs, float* observations, hipStream_t st) {
    if (!mlp::shape_ok(obs_dim, act_dim, layers) || horizon < 1 || (activation != mlp::RELU && activation != mlp::SWISH) ||
        n_problems < 1 || n_problems > mlp::PROBLEMS_MAX)
        return hipErrorInvalidValue;
    MlpTable tab{};
    long long wgs = 0, row = 0;
    for (int p = 0; p < n_problems; ++p) {
        const mlp::Problem& q = problems[p];
        if (!q.params || q.rows < 1 || q.action_row0 < 0 || q.obs_row < 0) return hipErrorInvalidValue;
        tab.params[p] = (gptr)q.params; tab.arow0[p] = q.action_row0; tab.obs[p] = q.obs_row;
        tab.wg0[p] = (int)wgs; tab.crow0[p] = row; tab.rows[p] = q.rows;
        wgs += ((long long)q.rows + 15) / 16; row += q.rows;
        if (wgs > mlp::WORKGROUPS_MAX) return hipErrorInvalidValue;
    }
    const dim3 grid((unsigned)wgs), block(NTHR);
    const int sk = mlp::state_kblocks(obs_dim);
#define ICEM_MLP_LAUNCH(SKV, AV)                                                                                                      \
    hipLaunchKernelGGL((mlp_rollout_models_kernel<SKV, AV>), grid, block, 0, st, tab, n_problems, horizon, obs_dim, act_dim, layers,  \
                       cost_mode, cs, obs0, actions, costs, observations)
    if (sk == 1 && activation == mlp::RELU) ICEM_MLP_LAUNCH(1, mlp::RELU);
    else if (sk == 1) ICEM_MLP_LAUNCH(1, mlp::SWISH);
    else if (activation == mlp::RELU) ICEM_MLP_LAUNCH(2, mlp::RELU);
    else ICEM_MLP_LAUNCH(2, mlp::SWISH);
#undef ICEM_MLP_LAUNCH
    return hipGetLastError();
}
}  // namespace icem
