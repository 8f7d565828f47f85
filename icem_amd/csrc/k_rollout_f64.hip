// k_rollout_f64.hip -- the float64 rollout + cost on the f64 matrix cores (icem_set_f64_arith(ICEM_F64_MFMA)): every observation
// width up to 384 in the strict-parity dtype.  One kernel family, runtime o / d / h; instantiated on the model kind, on whether
// the cost carries a term list and on whether the observations are written -- never on a width.
//
// A workgroup owns a tile of 16 trajectories.  Its contraction vector [state (o) | actions of the step (d) | zeros to a multiple
// of 4] lives as f64 rows in dynamic LDS, double buffered: the step reads buffer t & 1 and writes the new state (and the next
// step's actions) into the other one.  The model [A ; B] is in HBM as f64, row-major, zero-padded to Kp = ceil4(o + d) rows and
// Op = ceil16(o) columns (abi.hip: sync_f64_mfma), so the B operand of a 4-deep block is one 128-byte line per 16 lanes.
// v_mfma_f64_16x16x4_f64: A operand lane l = X[row l & 15][k0 + (l >> 4)], B operand lane l = M[k0 + (l >> 4)][col l & 15],
// result register r of lane l = row (l >> 4) + 4 r, column l & 15  (NOT the f32 forms' row formula).
// The column tiles are dealt over the four waves, a wave keeps up to three tiles' accumulators in flight (independent MFMAs
// back to back; one A-operand read serves the three).  Padding is zero in BOTH operands: the rows of a ragged last tile start
// at zero and stay there (tanh(0) = 0), columns >= o are never written back, k >= o + d is zero in the rows and in the model.
// The step's cost is evaluated from the LDS rows by the code the generic kernels use (cost_terms_dev.h), in their order.
#include "host_common.h"
#include "cost_terms_dev.h"

namespace icem {

namespace {

constexpr int F64_ROWS = 16;   // trajectories per workgroup
constexpr int F64_TIF = 3;     // column tiles in flight per wave
constexpr int F64_PRE = 4;     // action entries a thread fetches ahead: 16 rows x d <= 64 entries over 256 threads

typedef double f64x4 __attribute__((ext_vector_type(4)));

struct F64RolloutArgs {
    int n, h, d, o;
    int Op, Kp, xs;              // padded model columns / rows; LDS row stride in doubles
    int cost_mode;
    const double* M;             // [Kp][Op]
    const double* obs0;
    const double* actions;
    double* costs;
    double* observations;        // nullable [n, h, o]
    const CostArgs<double>* cs;  // device copy (by value it costs hundreds of scalar registers)
};

__device__ __forceinline__ double act_tanh64(double x) { return tanh(x); }

template <int KIND, bool TERMS, bool OBS>
__global__ __launch_bounds__(WG) void rollout_f64_mfma_kernel(F64RolloutArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    double* X = reinterpret_cast<double*>(smem_raw);   // [2][16][xs]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int o = a.o, d = a.d, hh = a.h, xs = a.xs, Op = a.Op, Kp = a.Kp;
    const int n_base = blockIdx.x * F64_ROWS;
    const int n_here = min(F64_ROWS, a.n - n_base);
    const int buf = F64_ROWS * xs;
    const int nct = Op >> 4;
    for (int e = tid; e < 2 * buf; e += WG) X[e] = 0.0;
    __syncthreads();
    for (int e = tid; e < n_here * o; e += WG) X[(e / o) * xs + e % o] = a.obs0[e % o];
    for (int e = tid; e < n_here * d; e += WG) {
        const int r = e / d, j = e - r * d;
        X[r * xs + o + j] = a.actions[(size_t)(n_base + r) * hh * d + j];
    }
    __syncthreads();
    // the cost of trajectory row `crow` is evaluated by the first lane of its group of 16 (four evaluators per wave); the
    // group's lanes sweep the row for the health term's finite / box check
    const int crow = tid >> 4, csub = tid & 15;
    const CostArgs<double>& cs = *a.cs;
    double acc = 0.0;
    const int mrow = lane & 15, mk = lane >> 4;
    for (int t = 0; t < hh; ++t) {
        const double* Xc = X + (t & 1) * buf;
        double* Xn = X + ((t + 1) & 1) * buf;
        // the next step's actions: fetched before the contraction, parked in LDS behind it
        double pre[F64_PRE];
#pragma unroll
        for (int u = 0; u < F64_PRE; ++u) {
            const int e = tid + u * WG;
            pre[u] = 0.0;
            if (t + 1 < hh && e < n_here * d) {
                const int r = e / d, j = e - r * d;
                pre[u] = a.actions[((size_t)(n_base + r) * hh + (t + 1)) * d + j];
            }
        }
        f64x4 res[(ICEM_MAX_OBS_DIM / 16 / 4 + F64_TIF - 1) / F64_TIF][F64_TIF];
        constexpr int GROUPS = (ICEM_MAX_OBS_DIM / 16 / 4 + F64_TIF - 1) / F64_TIF;
#pragma unroll
        for (int g = 0; g < GROUPS; ++g) {
            const int ct0 = wave + 4 * (g * F64_TIF);
            if (ct0 < nct) {   // (wave-uniform)
                const int ntl = min(F64_TIF, (nct - ct0 + 3) >> 2);
                f64x4 c[F64_TIF];
#pragma unroll
                for (int j = 0; j < F64_TIF; ++j) c[j] = f64x4{0.0, 0.0, 0.0, 0.0};
                const double* __restrict__ xa = Xc + mrow * xs + mk;
                const double* __restrict__ mb = a.M + (size_t)mk * Op + ct0 * 16 + mrow;
#pragma unroll 2
                for (int k0 = 0; k0 < Kp; k0 += 4) {
                    const double av = xa[k0];
                    double bv[F64_TIF];
#pragma unroll
                    for (int j = 0; j < F64_TIF; ++j) bv[j] = j < ntl ? mb[(size_t)k0 * Op + j * 64] : 0.0;
#pragma unroll
                    for (int j = 0; j < F64_TIF; ++j)
                        if (j < ntl) c[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv[j], c[j], 0, 0, 0);
                }
#pragma unroll
                for (int j = 0; j < F64_TIF; ++j) res[g][j] = c[j];
            }
        }
        // (every read of Xn by the previous step's cost phase is behind that step's closing barrier)
#pragma unroll
        for (int g = 0; g < GROUPS; ++g) {
            const int ct0 = wave + 4 * (g * F64_TIF);
            if (ct0 < nct) {
                const int ntl = min(F64_TIF, (nct - ct0 + 3) >> 2);
#pragma unroll
                for (int j = 0; j < F64_TIF; ++j) {
                    const int col = (ct0 + 4 * j) * 16 + mrow;
                    if (j < ntl && col < o) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const double v = res[g][j][r];
                            Xn[(mk + 4 * r) * xs + col] = (KIND == ICEM_MODEL_TANH) ? act_tanh64(v) : v;
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int u = 0; u < F64_PRE; ++u) {
            const int e = tid + u * WG;
            if (t + 1 < hh && e < n_here * d) {
                const int r = e / d, j = e - r * d;
                Xn[r * xs + o + j] = pre[u];
            }
        }
        __syncthreads();
        // ---- the step's cost, scored on the PRE-action observation (rollout_cost_body's order, generic_dev.h) ----
        const double* row = Xc + crow * xs;
        const double* nrow = Xn + crow * xs;
        bool bad = false;
        if (TERMS) {
            if (cs.health_idx >= 0) {   // (uniform) all_finite(obs) / the state box: part of `unhealthy` only
                bool b = false;
                for (int k = csub; k < o; k += 16) {
                    const double v = row[k];
                    b |= !finite_val(v);
                    if (cs.box_from >= 0 && k >= cs.box_from) b |= !(cs.box_lo < v && v < cs.box_hi);
                }
                const unsigned long long m = __ballot(b);
                bad = ((m >> (16 * (lane >> 4))) & 0xFFFFull) != 0ull;
            }
        }
        if (csub == 0 && crow < n_here) {
            const double* act = row + o;
            double ctrl = 0.0;
            for (int j = 0; j < d; ++j) ctrl = fmad(act[j], act[j], ctrl);
            double c = 0.0;
            if (cs.flip_idx >= 0) {
                const double ang = row[cs.flip_idx];
                c += (ang > cs.flip_th) ? cs.flip_pen : 0.0;
                c += (ang < -cs.flip_th) ? cs.flip_pen : 0.0;
            }
            c += cs.ctrl_w * ctrl;
            if (cs.lin_w != 0.0) c += cs.lin_w * row[cs.lin_idx];
            if (TERMS) {
                if (cs.ext) c += cost_terms<double>(cs, bad, [&](int idx) { return row[idx]; }, [&](int idx) { return nrow[idx]; });
            }
            if (t == 0 || a.cost_mode == ICEM_COST_FINAL)
                acc = c;
            else if (a.cost_mode == ICEM_COST_SUM)
                acc += c;
            else
                acc = (c < acc || c != c) ? c : acc;  // np.amin: a NaN step cost makes the trajectory's cost NaN
        }
        if (OBS) {
            double* dst = a.observations + ((size_t)n_base * hh + t) * o;
            for (int e = tid; e < n_here * o; e += WG) {
                const int r = e / o, k = e - r * o;
                dst[(size_t)r * hh * o + k] = Xc[r * xs + k];
            }
        }
        __syncthreads();   // the next step overwrites Xc
    }
    if (csub == 0 && crow < n_here) a.costs[n_base + crow] = acc;
}

}  // namespace

// LDS row stride: Kp entries, padded so that the 16 rows of an A-operand read start four doubles apart modulo the 64 banks
int f64_mfma_row_stride(int Kp) { return Kp + ((4 - Kp % 32) + 32) % 32; }

size_t f64_mfma_lds_bytes(int o, int d) {
    const int Kp = (o + d + 3) & ~3;
    return (size_t)2 * F64_ROWS * f64_mfma_row_stride(Kp) * sizeof(double);
}

int launch_rollout_f64_mfma(const icem_handle* h, int n, const void* obs0, const void* actions, void* costs, void* observations,
                            hipStream_t st) {
    if (!h->f64_model_ready || !h->f64_cs_dev || !h->M64_dev)
        return fail(ICEM_E_STATE, "ICEM_F64_MFMA: the model / cost of this handle have no device copy (icem_set_model / icem_set_cost first)");
    F64RolloutArgs a;
    a.n = n;
    a.h = h->cfg.horizon;
    a.d = h->cfg.act_dim;
    a.o = h->obs_dim;
    a.Op = (a.o + 15) & ~15;
    a.Kp = (a.o + a.d + 3) & ~3;
    a.xs = f64_mfma_row_stride(a.Kp);
    a.cost_mode = h->cfg.cost_mode;
    a.M = (const double*)h->M64_dev;
    a.obs0 = (const double*)obs0;
    a.actions = (const double*)actions;
    a.costs = (double*)costs;
    a.observations = (double*)observations;
    a.cs = (const CostArgs<double>*)h->f64_cs_dev;
    const size_t lds = f64_mfma_lds_bytes(a.o, a.d);
    if (lds > 160 * 1024 || a.o > ICEM_MAX_OBS_DIM || F64_ROWS * a.d > F64_PRE * WG)
        return fail(ICEM_E_UNSUPPORTED, "ICEM_F64_MFMA: the tile's rows do not fit the 160 KB of LDS");
    const dim3 grid((n + F64_ROWS - 1) / F64_ROWS), block(WG);
    const bool terms = h->has_terms, obs = observations != nullptr;
#define ICEM_F64_LAUNCH(KIND, TERMS, OBS)                                                                                   \
    do {                                                                                                                    \
        static std::atomic<bool> attr_set{false};                                                                           \
        if (!attr_set.load(std::memory_order_acquire)) {                                                                    \
            ICEM_HIP_TRY(hipFuncSetAttribute((const void*)rollout_f64_mfma_kernel<KIND, TERMS, OBS>,                        \
                                             hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));                      \
            attr_set.store(true, std::memory_order_release);                                                                \
        }                                                                                                                   \
        hipLaunchKernelGGL((rollout_f64_mfma_kernel<KIND, TERMS, OBS>), grid, block, lds, st, a);                           \
    } while (0)
#define ICEM_F64_PICK(KIND)                                       \
    do {                                                          \
        if (terms && obs) ICEM_F64_LAUNCH(KIND, true, true);      \
        else if (terms) ICEM_F64_LAUNCH(KIND, true, false);       \
        else if (obs) ICEM_F64_LAUNCH(KIND, false, true);         \
        else ICEM_F64_LAUNCH(KIND, false, false);                 \
    } while (0)
    if (h->model_kind == ICEM_MODEL_TANH) ICEM_F64_PICK(ICEM_MODEL_TANH);
    else ICEM_F64_PICK(ICEM_MODEL_LINEAR);
#undef ICEM_F64_PICK
#undef ICEM_F64_LAUNCH
    ICEM_HIP_TRY(hipGetLastError());
    return ICEM_OK;
}

}  // namespace icem
