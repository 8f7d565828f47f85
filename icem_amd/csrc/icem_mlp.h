// Fused rollout of a feed-forward learned dynamics model (icem_amd/models.py::declared_mlp) with the environment's parametric
// cost (icem_cost_spec + icem_cost_terms) on the bf16 matrix cores, in ONE launch.  Architecture:
//   x1 = act(W1 [s | a] + b1)                            200
//   xk = act(Wk x(k-1) + bk),  k = 2 .. layers           200
//   s' = s + Wout x_layers + bout                        obs_dim      (the residual add and the state itself in f32)
// act = relu or swish (x sigmoid(x)); obs_dim 1 .. 64, act_dim 1 .. 32, layers 1 .. 4, hidden 200.
// Output widths are padded to multiples of 16 (200 -> 208, obs_dim -> 16 OB), contraction widths to multiples of 32
// (200 -> 224, obs_dim -> 32 SK, act_dim -> 32) with SK = ceil(obs_dim / 32), OB = ceil(obs_dim / 16).  The packed parameter
// buffer (16-bit units; packer: icem_amd.models.pack_mlp) holds, per layer, the weight as v_mfma_f32_16x16x32_bf16
// A-operand blocks [out block][k block][lane 64][8 bf16] (lane = 16 g + i holds W[16 ob + i][32 kb + 8 g + 0 .. 7]) followed
// by the f32 bias (two units per entry):
//   W1    [13][SK + 1]   state columns at 0 .. obs_dim - 1, action columns at 32 SK .. 32 SK + act_dim - 1, zeros elsewhere
//   b1    208 f32
//   Wk    [13][7], bk 208 f32                            for k = 2 .. layers
//   Wout  [OB][7], bout 16 OB f32
// Padded hidden units have zero weights and zero biases (both activations map 0 to 0), padded state rows of Wout likewise:
// whatever is padding stays an exact zero through the rollout.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include "cost_args.h"

namespace icem {
namespace mlp {
constexpr int HID = 200, HIDB = 13, HIDK = 7;   // hidden width, its 16-wide output blocks and 32-wide K blocks
constexpr int OBS_MAX = 64, ACT_MAX = 32, LAYERS_MAX = 4;
constexpr int BLK = 64 * 8;                     // bf16 elements of one 16 x 32 A-operand block (rssm::BLK)
constexpr int RELU = 0, SWISH = 1;              // ICEM_MLP_RELU / ICEM_MLP_SWISH
constexpr int PROBLEMS_MAX = 32;                // problems of one launch (ICEM_MLP_MAX_PROBLEMS): their table travels in the kernel arguments
constexpr long long WORKGROUPS_MAX = 0x7fffffffLL;   // of one launch: the grid's x extent
__host__ __device__ constexpr int state_kblocks(int o) { return (o + 31) / 32; }
__host__ __device__ constexpr int state_oblocks(int o) { return (o + 15) / 16; }
// sizes in 16-bit units: the input layer with its bias, a further hidden layer with its bias, the output layer with its bias
__host__ __device__ constexpr size_t first_units(int sk) { return (size_t)HIDB * (sk + 1) * BLK + 2 * 16 * HIDB; }
__host__ __device__ constexpr size_t hidden_units() { return (size_t)HIDB * HIDK * BLK + 2 * 16 * HIDB; }
__host__ __device__ constexpr size_t out_units(int ob) { return (size_t)ob * HIDK * BLK + 2 * 16 * ob; }
inline bool shape_ok(int o, int d, int layers) {
    return o >= 1 && o <= OBS_MAX && d >= 1 && d <= ACT_MAX && layers >= 1 && layers <= LAYERS_MAX;
}
inline size_t param_units(int o, int d, int layers) {
    if (!shape_ok(o, d, layers)) return 0;
    return first_units(state_kblocks(o)) + (size_t)(layers - 1) * hidden_units() + out_units(state_oblocks(o));
}
// one problem of a launch of problems with a model each (icem_mlp_problem)
struct Problem {
    const unsigned short* params;   // its packed parameter buffer
    long long action_row0;          // its first row of `actions`
    int rows;                       // >= 1
    int obs_row;                    // its start observation: row of obs0 [n_obs, obs_dim]
};
}  // namespace mlp

// costs[i] = reduce_t c(s_t, a_t, s_{t+1}) along s_{t+1} = s_t + f(s_t, a_t) from s_0 = obs0 (cost_mode: 0 sum, 1 best, 2 final;
// c: `cs`, evaluated per row in f32 on the f32 states).  observations: NULL, or [n, horizon + 1, obs_dim] for s_0 .. s_h.
// The shape must satisfy mlp::shape_ok and 1 <= horizon (hipErrorInvalidValue otherwise); allocates nothing.
hipError_t launch_mlp_rollout(int n, int horizon, int obs_dim, int act_dim, int layers, int activation, int cost_mode,
                              const CostArgs<float>& cs, const unsigned short* params, const float* obs0, const float* actions,
                              float* costs, float* observations, hipStream_t st);

// launch_mlp_rollout for n_problems (1 .. mlp::PROBLEMS_MAX) problems with a MODEL EACH in one launch: problem p rolls the action
// rows action_row0 .. action_row0 + rows - 1 out from row obs_row of obs0 [n_obs, obs_dim] through its own params, on
// ceil(rows / 16) workgroups of its own.  costs [sum rows] and observations (NULL, or [sum rows, horizon + 1, obs_dim]): the
// problems back to back in problem order, each bit for bit what launch_mlp_rollout gives for it alone.  The shape, the
// activation, the horizon, cost_mode and the cost are the launch's.  `problems` is read before the call returns (the table
// travels by value in the kernel arguments); allocates nothing.  hipErrorInvalidValue: what launch_mlp_rollout refuses, a
// problem without params or rows, more than mlp::WORKGROUPS_MAX workgroups.  The caller checks the rows against the buffers.
hipError_t launch_mlp_rollout_models(int n_problems, const mlp::Problem* problems, int horizon, int obs_dim, int act_dim, int layers,
                                     int activation, int cost_mode, const CostArgs<float>& cs, const float* obs0, const float* actions,
                                     float* costs, float* observations, hipStream_t st);
}  // namespace icem
