// k_rollout_wide.hip -- K2 + K3 for WIDE observations (32 < o <= 384, e.g. HumanoidStandup's real o = 378, d = 17:
// icem/environments/mujoco.py:241-277): rollout_wide_kernel.
//
// At this width the model step is a real GEMM: per step [n, o + d] x [o + d, o], 2 (o + d) o = 299 kflop per
// trajectory-step at o = 378 against 68 bytes of actions -- compute bound by three orders of magnitude (SURVEY
// 7.3-11), so the kernel is built around keeping the f32 matrix pipe fed, not around HBM:
//   * one wavefront owns 16 trajectories; their contraction vectors [obs | action | 0-pad] live in the wave's own LDS
//     rows X[16][XS] (f32; 25.6 KB at o = 378), the new observation of all NT = ceil(o / 16) column tiles in 4 * NT
//     accumulator registers (96 at o = 378);
//   * per 4-wide contraction block kb: ONE ds_read of the B operand (X[j][4 kb + g]: trajectory j = lane % 16, slot
//     g = lane / 16), then NT v_mfma_f32_16x16x4_f32 (exact f32, same fmaf chain as scalar code) on independent
//     accumulators, their A operands (the 16 x 4 blocks of the model) coming as 16-byte loads from a host-packed copy
//     of [A ; B] in exactly that order: Mp[kb][ct / 4][lane][ct % 4] = M[4 kb + lane / 16][16 ct + lane % 16] -- 6
//     coalesced dwordx4 loads per 24 MFMAs, shared by every wave of the chip through L2 (the 608 KB model stays
//     L2-resident);
//   * after the last block lane (j, g) holds columns 16 ct + 4 g .. + 3 of trajectory j in accumulator ct: activation,
//     then one 16-byte LDS store per tile back into X (the wave's LDS traffic executes in order: no barrier);
//   * the step cost (icem_cost_spec: control cost + linear + flip terms of the PRE-action observation) is read from X
//     by lanes 0..15; costs and the wave's running sorted top-K as in k_rollout.hip; one candidate list per workgroup.
// The arithmetic is exact f32, so the tolerance against the float64 oracle is the 1e-5 of every other f32 kernel.
// (A bf16 x 3-plane split on v_mfma_f32_16x16x32_bf16 would need 94 B/clk of model operands per CU at this tiling --
// more than the L2 port delivers: DESIGN.md section 4.)
#include "wide_rollout_dev.h"

namespace icem {

namespace {

// (the bodies: wide_rollout_body.h / wide_rows_body.h, shared as text with the batched twins of k_rollout_wide_batch.hip)
// EXT: icem_cost_terms on.  Its own instantiation: the model loop below is scheduled to the register -- with the terms'
// code merely PRESENT (never executed) the allocator moved an in-flight model operand, which is a wait for all requests
// in flight, and every launch was 9 % slower (1 358 -> 1 466 us at o = 378, N = 16 384), whatever was tried to keep the
// terms out of the loop's live set.
template <int NT, int KIND, int WAVES, bool EXT>
__global__ __launch_bounds__(64 * WAVES) void rollout_wide_kernel(WideRolloutArgs a) {
#include "wide_rollout_body.h"
}

// A few single rows at the same widths: one workgroup per trajectory, thread c owns observation column c and runs the
// contraction as ONE fmaf chain over k = 0 .. o + d - 1 from the row-major model -- the chain an f32 MFMA executes over
// its slots, blocks in rollout_wide_kernel's order, so the costs are the bits the tile kernel would produce for the row
// (the zero padding blocks add exact zeros).  For the handful of shifted elites (icem.py:131-137) that would otherwise
// open a 16-row tile of their own: at N = 16 384 that tile is number 1 025 on 1 024 wavefront slots and doubles the
// launch (2.47 instead of 1.26 ms); these rows take ~0.1 ms.
// (WideRowsArgs: icem_fused.h)
template <int KIND>
__global__ __launch_bounds__(384) void rollout_rows_wide_kernel(WideRowsArgs a) {
#include "wide_rows_body.h"
}

}  // namespace

bool wide_rollout_supported(int o, int d, int K) { return o > 32 && o <= 384 && d >= 1 && d <= 64 && K <= 32; }
bool gemm_rollout_supported(int o, int d, int K) { return o >= 1 && o <= 384 && d >= 1 && d <= 64 && K <= 32; }

int wide_rollout_lists(int n_rows) { return std::min(std::max(1, (n_rows + 15) / 16), FAST_MAX_LISTS); }

// contraction rows of the packed model: [obs (o) | act (d)] padded to whole 4-blocks; X row stride in floats
// (a multiple of 3: rollout_wide_kernel's block loop is unrolled by three; the padding blocks are zero)
int wide_kb(int o, int d) { return ((o + d + 3) / 4 + 2) / 3 * 3; }
int wide_xs(int o, int d) { return 4 * wide_kb(o, d) + 4; }
int wide_nt(int o) { const int nt = (o + 15) / 16; return nt <= 4 ? 4 : nt <= 8 ? 8 : nt <= 16 ? 16 : 24; }

// Mp[kb][q][lane][v] = M[4 kb + lane / 16][16 (4 q + v) + lane % 16], M = [A ; B] ([o + d, o], zero padded)
void pack_wide_model(int o, int d, const double* A, const double* B, std::vector<float>& Mp) {
    const int KB = wide_kb(o, d), NT = wide_nt(o), NQ = NT / 4;
    Mp.assign((size_t)KB * NQ * 64 * 4, 0.f);
    auto M = [&](int r, int c) -> double {
        if (c >= o) return 0.0;
        if (r < o) return A[(size_t)r * o + c];
        if (r < o + d) return B[(size_t)(r - o) * o + c];
        return 0.0;
    };
    for (int kb = 0; kb < KB; ++kb)
        for (int q = 0; q < NQ; ++q)
            for (int lane = 0; lane < 64; ++lane)
                for (int v = 0; v < 4; ++v)
                    Mp[(((size_t)kb * NQ + q) * 64 + lane) * 4 + v] = (float)M(4 * kb + lane / 16, 16 * (4 * q + v) + lane % 16);
}

// the launch's key: everything that selects the instantiation and the grid (a batch issues ONE launch for problems of equal keys)
void launch_rollout_wide(const LaunchCtx& cx, const WideRolloutArgs& a, int kind) {
    LaunchKey k;
    k.family = LAUNCH_ROLLOUT_WIDE;
    k.h = a.h, k.d = a.d, k.O = a.o, k.kind = kind == 1 ? 1 : 0, k.arith = 1;
    k.waves = wide_nt(a.o);
    k.form = a.cs ? 1 : 0;
    k.wgs[0] = wide_rollout_lists(a.n_rows);
    hipStream_t st = cx.st;
    submit(cx, k, true, [&](void* dst, unsigned long long) { batch_form(a, dst); }, [&] {
        wide_dispatch(k, [&](auto nt, auto kd, auto ext) {
            auto kfn = rollout_wide_kernel<decltype(nt)::value, decltype(kd)::value, WIDE_WAVES, decltype(ext)::value>;
            const size_t lds = wide_lds_bytes(k);
            (void)hipFuncSetAttribute((const void*)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            hipLaunchKernelGGL(kfn, dim3(k.wgs[0]), dim3(64 * WIDE_WAVES), lds, st, a);
        });
    });
}

void launch_rollout_rows_wide(const LaunchCtx& cx, const WideRolloutArgs& w, int row0, int n_tail, const float* A, const float* B, int kind) {
    if (n_tail <= 0) return;
    WideRowsArgs a{row0, n_tail, w.o, w.d, w.h, w.cost_mode, WideCost{w.lin_idx, w.flip_idx, w.ctrl_w, w.lin_w, w.flip_pen, w.flip_th},
                   w.cs, A, B, w.obs0, w.actions, w.costs};
    LaunchKey k;
    k.family = LAUNCH_ROLLOUT_ROWS_WIDE;
    k.h = w.h, k.d = w.d, k.O = w.o, k.kind = kind == 1 ? 1 : 0, k.arith = 1;
    k.form = w.cs ? 1 : 0;
    k.wgs[0] = n_tail;
    hipStream_t st = cx.st;
    submit(cx, k, true, [&](void* dst, unsigned long long) { batch_form(a, dst); }, [&] {
        if (k.kind == 1) hipLaunchKernelGGL((rollout_rows_wide_kernel<1>), dim3(n_tail), dim3(384), 0, st, a);
        else hipLaunchKernelGGL((rollout_rows_wide_kernel<0>), dim3(n_tail), dim3(384), 0, st, a);
    });
}

}  // namespace icem
