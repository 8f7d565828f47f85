// icem_fused.h -- interface between the host-side translation units (plan.hip, abi.hip) and the f32 throughput
// kernels (k_sample.hip, k_rollout.hip, k_rollout_ahead.hip, k_rollout_wide.hip, k_iter_small.hip, k_merge.hip):
// argument blocks and launchers; the launch context of a step and what a batched step (icem_plan_step_batch, and for its sampler
// icem_plan_step_learned*) needs of a launch family -- LAUNCH_FAMILIES, one row per family.  Internal; not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <cstddef>
#include <cstring>
#include <vector>
#include "cost_args.h"
#include "options.h"
#include "tile_scales.h"

namespace icem {

constexpr int FAST_MAX_LISTS = 256;  // candidate lists (one per rollout workgroup) the merge accepts
struct BatchHint;   // how many problems share the step's launches ...
struct LaunchCtx;   // ... and stream + hint + recorder, what the step's launchers take (both below: "the step's launch context")

// In-library elite exchange (exchange.hip): what a merge needs to wait for the ranks' records of one exchange.
constexpr int XCHG_MAX_WORLD = 16;
struct XchgWait {
    const unsigned* flags = nullptr;  // [world] sequence flags of the exchange's parity in THIS rank's block; nullptr: no wait
    unsigned* status = nullptr;       // set to 1 when a wait times out
    unsigned seq = 0;                 // the value every flag must reach
    int world = 0;
    unsigned max_polls = 0;           // bound of the wait (polls of ~0.5 us); then status = 1 and the wait gives up
    const void* records = nullptr;    // [world * K] gathered records of that parity (handle dtype)
};
// ... and what the producer needs to push its K records into every rank's block from inside the pack kernel
struct XchgPush {
    unsigned char* const* peers = nullptr;  // [world] device pointers of the ranks' blocks; nullptr: no push
    size_t rec_byte_off = 0;                // byte offset of this rank's slot (parity applied) inside a block
    int world = 0;
    int flag_idx = 0;                       // flag word of (parity, this rank)
    unsigned seq = 0;
};

// K1 fast: colored-noise sampling with the inverse real DFT folded on its symmetry (f32, Philox).
struct FastSampleArgs {
    int n, h, d;
    long long first_index;
    const float* W;  // [h, 32]
    const float* mean;
    const float* std;
    const float* low;
    const float* high;
    uint32_t seed_lo, seed_hi, off_lo, off_hi;
    int row0_mean;
    float* out;  // [n (+ n_shift), h, d]
    // optional shifted elites (icem.py:91-104), handled by one extra workgroup of the same launch:
    // rows [n, n + n_shift) <- elites_src[e, 1:, :] ++ one freshly sampled last action (stream off2)
    int n_shift;
    const float* elites_src;  // [>= n_shift, h, d]
    uint32_t off2_lo, off2_hi;
    int white;  // noise_beta <= 0 (icem.py:77): normal t of a row is its sample at step t, no synthesis
    // single-launch kernel, iteration 0 only: the raw colored noise of this call -- rows [0, n) and, behind them, the
    // n_shift shifted elites' rows of stream off2 -- was drawn ahead (beside the previous MPC step's last merge,
    // merge_noise_kernel) and only has to be mapped; nullptr: draw it here
    const float* raw_src = nullptr;
};
bool fast_sample_supported(int h, int d);
int sample_row_workgroups(int n, int d);   // workgroups of the folded sampler that draw n rows
void launch_sample_folded(const LaunchCtx& cx, const FastSampleArgs& a, int rounds);

// K2+K3 fast: rollout on the matrix pipe (v_mfma_f32_16x16x4, exact f32), cost on the VALU, and a
// sorted top-K per workgroup; one wavefront per 16 trajectories.
struct FastRolloutArgs {
    int n_rows;   // trajectories to roll out (rows of `actions`)
    int n_cand;   // rows [0, n_cand) enter the top-K
    int K;        // 0 = no candidate output
    int o;        // true observation width (<= O)
    int cost_mode;
    const float* Mp;    // [O + D + 1, 4*ceil(O/4)] permuted, zero padded model [A ; B], then one zero row
    const int* perm;    // [32] permuted column k holds observation entry perm[k]; 31 (a zero slot) for k >= o
    const float* obs0;
    float ctrl_w, lin_w, flip_pen, flip_th;
    int flip_col;       // column holding obs[flip_idx] after the permutation, -1 = no flip term
    const float* actions;
    float* costs;
    float* part_c;  // [grid, K] sorted candidate costs / row indices of every workgroup ...
    int* part_i;
    unsigned long long* part_k;  // ... or, if not null, their packed keys, key r of workgroup w at [r * grid + w]
    int list_wgs = 0;   // > 0: only the first list_wgs workgroups emit a list (sample_rollout_lists' tail rows)
    long long* dbg;  // development: [waves, 8] cycle stamps, nullptr in production
    // which arithmetic the model step of the 16-trajectory tile runs in (icem_set_tile_arith; fused_dev.h):
    // 0 = v_mfma_f32_16x16x4_f32, bitwise an fmaf chain (Tile16; Tile4 is its VALU twin); 1 = two fp16 planes of every f32
    // operand, three products per multiply-add on v_mfma_f32_16x16x32_f16 (Tile16H; one-tile observation widths only)
    int arith = 0;
    float act_mag = 1.f;   // arith 1: magnitude of the action bounds, max(|low|, |high|) -- with |obs0| it fixes the launch's scale
    float m_scale = 1.f, b_scale = 1.f;   // arith 1: powers of two that put the largest |entry| of A / of B into [64, 128)
    float inv_m_scale = 1.f, inv_b_scale = 1.f;   // ... and their reciprocals, exact (update_paths; tile_scales.h): the kernels multiply
    unsigned* nonfinite = nullptr;        // counts the trajectories whose cost came out NaN (icem_nonfinite_costs); never NULL in a launch
};
bool fast_rollout_supported(int h, int d, int O, int K);
void launch_rollout16(const LaunchCtx& cx, const FastRolloutArgs& a, int h, int d, int O, int kind);
// workgroups (= candidate lists) the rollout of n_rows trajectories is launched with
int rollout_lists(int h, int d, int O, int n_rows);

// K2+K3 for the narrow shapes beside HalfCheetah that the reference ships (Door, Relocate, FetchPickAndPlace: k_rollout_hn.hip):
// TileHN -- up to three output tiles on the 16-bit matrix cores (the fp16-plane arithmetic of Tile16H), icem_cost_terms
// evaluated across the four lanes of a trajectory.  A [o, lda], B [d, ldb]: the row-major f32 model; cs: device copy of the
// cost terms (nullptr: none).  r: n_rows / n_cand / K / o / cost_mode / obs0 / actions / costs / part_* / the cost spec's
// weights / act_mag, m_scale, b_scale.
template <typename T> struct CostArgs;
bool hn_rollout_supported(int h, int d, int o, int K);
// (bh: a batch of bh.mult problems of this size in one launch -- waves per workgroup as for all their tiles together, the
//  workgroups of ONE problem, always the one-wave-per-tile kernel, no tail workgroups)
int hn_rollout_lists(const BatchHint& bh, int n_rows);
int hn_tail_rows(const BatchHint& bh, int n_rows, int n_tail);   // trailing shifted-elite rows scored through the cost array (0: none)
// the icem_cost_spec part of a step cost as the GEMM and TileHN kernels take it (wide_dev.h)
struct WideCost {
    int lin_idx, flip_idx;
    float ctrl_w, lin_w, flip_pen, flip_th;
};
// the TileHN kernels' argument block: by value, or -- a batch -- one per problem in a device array
struct HnArgs {
    FastRolloutArgs r;           // n_rows, n_cand, K, o, cost_mode, obs0, actions, costs, part_*, ctrl_w, act_mag, m_scale, b_scale
    const float* A;              // [o, lda] row-major f32
    const float* B;              // [d, ldb]
    int lda, ldb;
    WideCost wc;
    const CostArgs<float>* cs;   // device copy of the cost terms, nullptr: none
};
// cs: terms sorted into the program prog = (N32, N4, NP) and padded with null terms (kind -1): hn_cost_program says whether a
// list of n32 long slices (5 .. 32 entries), n4 short ones and np point terms has a compiled program, and which
bool hn_cost_program(int n32, int n4, int np, int* prog);
void launch_rollout_hn(const LaunchCtx& cx, const FastRolloutArgs& r, int h, int d, int o, int kind, const float* A, int lda, const float* B, int ldb,
                       int lin_idx, int flip_idx, const CostArgs<float>* cs, const int* prog);

// K2+K3 for wide observations (32 < o <= 384; k_rollout_wide.hip): the model step as an f32 matrix-pipe GEMM per
// 16-trajectory tile, contraction vectors in LDS; same candidate-list outputs as the kernels above.
struct WideRolloutArgs {
    int n_rows, n_cand, K;
    int o, d, h;
    int kb, xs;           // contraction blocks of 4, LDS row stride (wide_kb / wide_xs)
    int planes;           // rollout_wide_split_kernel: 3 = bf16 planes (six products per multiply-add), 2 = fp16 planes (three)
    float minv;           // ... fp16 planes: 1 / the model's power-of-two scale (pack_wide_model_split)
    const float* ksc;     // ... the contraction entries' powers of two, [32 kb] (device memory)
    const float* csc;     // ... and the output columns', [16 x 8 x NCT]
    float sbound;         // ... the largest scaled state entry of a tanh model (max over the observation entries of their power of two)
    int cost_mode;
    int lin_idx, flip_idx;
    float ctrl_w, lin_w, flip_pen, flip_th;
    const CostArgs<float>* cs;   // icem_cost_terms on: the same + the terms, in device memory (NULL: off)
    long long* dbg;       // development: 8 wall_clock64 phase stamps of one wave (rollout_wide_split_kernel; tools/dbg/split_stamps.py), nullptr in production
    const float* Mp;      // pack_wide_model / pack_wide_model_split
    const float* obs0;
    const float* actions;
    float* costs;
    float* part_c;
    int* part_i;
    unsigned long long* part_k;
};
bool wide_rollout_supported(int o, int d, int K);
bool gemm_rollout_supported(int o, int d, int K);   // the same kernels at ANY observation width 1..384 (narrow models the tile kernels do not serve)
int wide_rollout_lists(int n_rows);
int wide_kb(int o, int d);
int wide_xs(int o, int d);
void pack_wide_model(int o, int d, const double* A, const double* B, std::vector<float>& Mp);
void launch_rollout_wide(const LaunchCtx& cx, const WideRolloutArgs& a, int kind);
// ... the same on the bf16 matrix cores (k_rollout_wide_split.hip): every f32 operand as three bf16 planes, six products
// per MAC, up to 80 trajectories per workgroup; a.Mp = pack_wide_model_split's planes, a.kb / a.xs = wide_split_kb / _xs
int wide_split_kb(int o, int d);
int wide_split_xs(int o, int d);
int wide_split_lists(int n_rows);
bool wide_split_fits(int o, int d);   // the workgroup's rows + planes in 160 KB of LDS (o + d <= 416); else the exact-f32 kernel
int wide_model_imbalance_log2(int o, int d, const double* A, const double* B);   // ICEM_WIDE_AUTO's criterion (k_rollout_wide_split.hip)
void pack_wide_model_split(int o, int d, const double* A, const double* B, int planes, std::vector<unsigned short>& Mb, float* minv,
                           std::vector<float>* ksc, std::vector<float>* csc, float* sbound);
void launch_rollout_wide_split(const LaunchCtx& cx, const WideRolloutArgs& a, int kind);
// rows [row0, row0 + n_tail) of the same pool one workgroup each, from the row-major f32 model (A [o, o], B [d, o]); costs only
struct WideRowsArgs {
    int row0, n_tail, o, d, h, cost_mode;
    WideCost wc;
    const CostArgs<float>* cs;
    const float* A;  // [o, o] row-major
    const float* B;  // [d, o]
    const float* obs0;
    const float* actions;
    float* costs;
};
void launch_rollout_rows_wide(const LaunchCtx& cx, const WideRolloutArgs& a, int row0, int n_tail, const float* A, const float* B, int kind);

// world == 1: global sorted top-K straight from the waves' candidate lists (+ kept elites), gather of
// the elite rows from the pool, refit, and the last-iteration epilogue.
struct MergeSingleArgs {
    int n_lists;   // candidate lists, each K long and sorted
    int n_keep;    // kept elites appended as candidates (icem.py:143-145), gidx = n_global + e
    int keep_base = -1;  // >= 0: index of kept candidate 0 in its key instead of n_global (pack of a sharded rank: n_loc)
    int n_pool;    // sampled + shifted rows in `actions` this iteration (local == global, world 1)
    int n_global;  // N_it: index offset of shifted (it == 0) or kept (it > 0) elites
    int K, h, d, last;
    float alpha, init_std;
    const unsigned long long* part_k;  // [K, n_lists] packed candidate keys (FastRolloutArgs::part_k)
    // sharded runs (merge prologues only): the candidates are the all-gathered records {cost, gidx, actions[h*d]}
    // instead of lists + pool (part_k / actions / n_lists / n_pool unused)
    const float* records;  // [n_rec, 2 + h*d] or nullptr
    int n_rec;
    XchgWait xw;           // records arrive through the in-library exchange: wait for them first (flags == nullptr: no)
    const float* actions;
    const float* elites_cur;
    const float* elites_cost_cur;
    float* elites_next;
    float* elites_cost_next;
    const float* mean;  // distribution before the refit (momentum term)
    const float* std;
    float* mean_out;    // ... and after (may alias mean / std)
    float* std_out;
    const float* low;
    const float* high;
    float* executed;
    float* best_cost;
    long long* dbg;  // development: 8 wall_clock64 stamps (100 MHz) of thread 0, nullptr in production
    // noise-ahead pipeline, non-last iterations (iter_ahead_kernel's prologue only): pool rows [0, n_raw) still hold the
    // RAW colored noise y -- the launch that rolled them out did not write the actions back -- and an elite row among
    // them is clip(y * std + mean, xf_lo, xf_hi) with THIS merge's input distribution (mean / std above: what the
    // iteration sampled from).  0: the pool holds actions.
    int n_raw = 0;
    float xf_lo = 0.f, xf_hi = 0.f;
};
void launch_merge_single(const LaunchCtx& cx, const MergeSingleArgs& a);
// ... with noise workgroups beside it (noise-ahead pipeline: z.n rows of raw colored noise -> z.out; see merge_noise_kernel)
bool merge_noise_ok(const MergeSingleArgs& a, int rounds);
// z2 (z2.n > 0): a second, small sampling call in one more workgroup (the next step's shifted elites' noise)
void launch_merge_noise(const LaunchCtx& cx, const MergeSingleArgs& a, const FastSampleArgs& z, const FastSampleArgs& z2);
// icem_update_distribution for small f32 pools (topk_small_ok(n + n_keep, K)): top-K over [costs | keep_costs], gather from
// [pool | keep_actions], refit of mean / std in place -- one launch
struct UpdateSmallArgs {
    const float* costs;         // [n]
    const float* pool;          // [n, hd]
    const float* keep_costs;    // [n_keep] or nullptr
    const float* keep_actions;  // [n_keep, hd]
    int n, n_keep, K, hd;
    float alpha;
    float* mean;                // [hd], in place
    float* std;
    float* elites_out;          // [K, hd] (must not alias keep_actions)
    float* elite_costs_out;     // [K]
    int* idx_out;               // [K] indices into [pool | kept elites]
};
void launch_update_small(const UpdateSmallArgs& a, hipStream_t st);
// ... for B problems in one launch (one workgroup each, args[n] in DEVICE memory), and -- finish -- with the MPC step's
// epilogue behind the refit: shift of the new mean, reset of std (icem_shift's arithmetic), executed = elites[0, 0, :],
// best_cost = elite_costs[0], both also as `result` [d + 1] (nullptr: not wanted).  hd <= UPDATE_FINISH_MAX_HD: the new mean
// passes through that many floats of LDS (2 KB; the learned-dynamics step at h = 12 / 13 and the RSSM's widest action, 32,
// needs 384 / 416 of them).
constexpr int UPDATE_FINISH_MAX_HD = 512;
struct UpdateFinishArgs {
    UpdateSmallArgs u;
    int d;
    float init_std;
    const float* low;
    const float* high;
    float* executed;
    float* best_cost;
    float* result;
};
void launch_update_small_batch(const UpdateFinishArgs* args_dev, int n, bool finish, hipStream_t st);
// ... whose pool costs are not in memory yet: the update reduces them itself from the members' (icem_plan_step_learned_models).
// Candidate i of the problem costs reduce_e member_costs[e * stride + row0 + i], e = 0 .. members - 1, in the arithmetic of
// rssm_ensemble_reduce_kernel operation for operation (mean: ((c_0 + c_1) + ..) * inv with inv = (float)(1.0 / members) from the
// host; max: (c > acc || c != c) ? c : acc; a NaN member makes the row NaN); the reduced cost is also written to costs[i], where
// the single-model step leaves it.  Everything behind the keys is launch_update_small_batch's.  members in [1, 32].
struct UpdateMembersArgs {
    UpdateFinishArgs f;          // (f.u.costs: unused -- the costs come from member_costs)
    const float* member_costs;   // [members, stride]
    float* costs;                // [f.u.n] out: the reduced costs
    int members, reduce;         // reduce: ICEM_RSSM_REDUCE_MEAN / _MAX
    int stride, row0;            // the member stride (all problems' rows of this iteration) and this problem's first row
    float inv;                   // (float)(1.0 / members)
};
void launch_update_small_members_batch(const UpdateMembersArgs* args_dev, int n, bool finish, hipStream_t st);
// sorted top-K of a small f32 cost array in one launch (icem_topk_sorted's fast path)
bool topk_small_ok(int n, int K);
void launch_topk_small(const float* costs, int n, int K, float* out_c, int* out_i, hipStream_t st);
// sharded runs: the rank's K best of its candidate lists (part_k / actions / n_lists / n_keep = 0 of `a`) -> records [K, 2 + h*d]
// px.peers != nullptr (allowed when pack_can_push): the records also go into every rank's exchange block, followed by the
// flags -- pack and push in one launch
bool pack_can_push(int K, int h, int d);
void launch_pack_records(const MergeSingleArgs& a, int n_loc, int shard_lo, float* records, hipStream_t st,
                         const XchgPush& px = XchgPush());
// the same + the records merge `m` that waits for this pack's records (the step's last iteration), one launch
void launch_pack_merge(const MergeSingleArgs& pk, int n_loc, int shard_lo, float* records, const XchgPush& px, const MergeSingleArgs& m,
                       hipStream_t st);

// Sharded runs, "riding pack": the PREVIOUS iteration's record pack + push as one extra workgroup (index 0) of this
// iteration's launch, running while the other workgroups draw their noise; their merge prologue then waits for the
// exchange's flags (this rank's own among them) as always.  Reads the previous launch's lists and pool, which this
// launch overwrites only behind those flags.
struct PackPrev {
    const unsigned long long* part_k = nullptr;  // previous launch's candidate lists; nullptr: no pack in this launch
    const float* actions = nullptr;              // ... and pool
    int n_lists = 0, n_pool = 0, n_global = 0, K = 0;
    int n_loc = 0, shard_lo = 0;
    int n_keep = 0;                              // shifted-elite rows behind the lists (rank 0, iteration 0), scored through
    const float* keep_costs = nullptr;           // ... their costs (the cost array from row n_loc on)
    float* records = nullptr;                    // this rank's [K, 2 + h*d] records
    XchgPush px;
    // sample_folded_merge_kernel only ("published merge"): workgroup 0 also runs the launch's one records merge and
    // publishes mean | std here (written through), then stores pub_seq to pub_flag; the other workgroups wait for that
    float* pub = nullptr;                        // [2 * h*d]; nullptr: every workgroup merges for itself
    unsigned* pub_flag = nullptr;
    unsigned pub_seq = 0;
};
// may the merge-prologue launch of an iteration with n_rows local rows carry the previous iteration's pack? (the
// single-launch kernel or the sampler of the two-kernel path; the records must fit the workgroup's tile)
bool sample_rollout_pack_ok(const BatchHint& bh, int h, int d, int O, int rounds, int n_rows, int K);
bool sample_folded_pack_ok(int h, int d, int rounds, int K);

// ---- noise-ahead pipeline (large populations, world == 1; plan.hip::plan_step_ahead) -----------------------
// The colored noise of an iteration does not depend on the distribution (icem.py:73-79: powerlaw_psd_gaussian first,
// `* std + mean` after), so it is drawn AHEAD: every iteration is ONE launch (iter_ahead_kernel, k_rollout_ahead.hip)
// whose workgroups split into a rollout role (previous iteration's merge in the prologue, affine map + clip applied to
// every vector it loads from the raw-noise pool and written back in place), a noise role (the NEXT sampling call's raw
// y [n, h, d] into the next pool) and, at iteration 0, a shifted-elites role.  Same operations in the same order as the
// sampler + rollout pair: same bits in every buffer.
void launch_noise_rows(const FastSampleArgs& a, int rounds, hipStream_t st);  // uses n, first_index, W, seed / offset, out, white
struct IterAheadArgs {
    // rollout role
    FastRolloutArgs r;   // r.actions == pool
    MergeSingleArgs m;   // has_merge: the PREVIOUS iteration's merge (last == 0) -- 1: lists form, in every rollout
    int has_merge;       // workgroup's prologue (world 1); 2: records form, once, by the pack role (sharded runs)
    int n_xf;            // rows [0, n_xf) of the pool hold raw noise
    int row0_mean;       // icem.py:87-88
    int store_back;      // write the actions back over the noise (the last iteration: the caller's pool; the others leave
                         // the noise in place and the next prologue maps the K elite rows again, MergeSingleArgs::n_raw)
    float* pool;         // [n_rows, h, d]
    const float* mean;   // the distribution when has_merge == 0 (else the prologue computes it from m)
    const float* std;
    float lo, hi;        // the action bounds, equal in every action dimension (plan.hip checks before taking this path)
    // noise role: z.n rows of the sampling call (z.off_*) -> z.out (z.n == 0: no such workgroups)
    FastSampleArgs z;
    // shift role: s.n_shift shifted elites from s.elites_src (stream s.off2_*, distribution s.mean / s.std) -> rows
    // [s.n, s.n + s.n_shift) of s.out (== pool) and their costs -> r.costs[s.n ...] (s.n_shift == 0: no such workgroup)
    FastSampleArgs s;
    // sharded runs (world > 1; has_merge == 2): the PREVIOUS iteration's record pack + push rides as workgroup 0, which
    // then runs the launch's one records merge (m: records form) and publishes mean | std (p.pub / p.pub_flag / p.pub_seq,
    // as in sample_folded_merge_kernel); the rollout workgroups wait for that flag instead of merging themselves
    PackPrev p;
    int n_roll, n_noise;  // workgroups per role (filled by the launcher)
    int dbg_slot = 0;     // development: which 16-word block of r.dbg this launch stamps (the iteration)
};
bool rollout_ahead_ok(const BatchHint& bh, int h, int d, int O, int K, int n_rows);
int ahead_roll_workgroups(const BatchHint& bh, int n_rows);  // = candidate lists of that launch
void launch_iter_ahead(const LaunchCtx& cx, const IterAheadArgs& a, int h, int d, int O, int kind);

// K1 with the previous iteration's merge (last == 0) in its prologue, see sample_folded_merge_kernel
struct FastSampleMergeArgs {
    FastSampleArgs s;  // n_shift must be 0
    MergeSingleArgs m;
    PackPrev p;        // sharded runs: the previous iteration's pack rides as workgroup 0
};
bool sample_folded_merge_ok(int h, int d, int rounds, int K);
void launch_sample_folded_merge(const LaunchCtx& cx, const FastSampleMergeArgs& a);
bool sample_batch_compiled(int h);   // do the batched forms of BOTH sampling launches exist at this horizon? (ICEM_SAMPLE_BATCH_HORIZONS)

// K1+K2+K3 in one launch (small populations): r.actions == s.out, r.n_rows == s.n + s.n_shift.
struct FastIterArgs {
    FastSampleArgs s;
    FastRolloutArgs r;
    MergeSingleArgs m;  // merge prologue only: the PREVIOUS iteration's merge (last == 0), see sample_rollout_kernel
    PackPrev p;         // ... and its pack (sharded runs)
};
}  // namespace icem
#include "generic_args.h"   // the generic kernels' argument blocks (MergeArgs holds an XchgWait): families 7-11 below
namespace icem {
// ---- the step's launch context, and batched planners (icem_plan_step_batch, icem_plan_step_batch_f64; plan.hip) ------------
// B independent MPC problems of the same configuration advance together: every launch of the small-population path
// (sample_rollout_kernel x opt_iters, then the last merge) is ONE launch for all of them -- blockIdx.y = the problem, its
// argument block read from an array in device memory instead of the kernel-argument segment.  The host side of every
// handle runs as for a solo step under a LaunchCtx that carries a recorder: a launcher computes its launch (LaunchKey: the
// family's dispatch key and workgroup counts) and either issues it or, recording, appends key + argument block to the
// recorder; plan.hip then issues one batched launch per recorded one.  Same device code (the kernels' bodies are shared),
// same bits per problem.
constexpr int ICEM_MAX_BATCH = 32;
struct BatchBases {          // by value in the kernel-argument segment: the noise stream offset of this MPC step per problem
    unsigned long long v[ICEM_MAX_BATCH];   // (the offsets in the argument blocks are stored RELATIVE to it: the blocks of a
};                                          //  steady-state step are the previous same-parity step's, and are not uploaded again)
// How many problems share the step's launches: the shape rules choose launch shapes for mult x the rows ...
struct BatchHint {
    int mult = 1;
    bool ahead = false;   // ... and the batch may take the noise-ahead launches where all its rows together fill them
};
// What a dispatch table maps to a compiled instantiation and a grid (all ints, no padding: compared as bytes)
// (LAUNCH_SAMPLE / _SAMPLE_MERGE / _ROLLOUT_HN: the sampler, the sampler with the previous merge in its prologue and the TileHN
//  rollout -- the two-kernel iterations of the Door / Relocate / FetchPickAndPlace shapes)
// (LAUNCH_GK_*: the generic kernels of a float64 step, icem_plan_step_batch_f64 -- the quad sampler, the shifted elites' copy, the
//  rollout with a row of lanes / a thread per trajectory, the one-launch selection + refit; generic_kernels.hip, k_generic_batch.hip)
// (LAUNCH_ROLLOUT_WIDE / _WIDE_SPLIT / _ROWS_WIDE: the GEMM-path rollouts -- exact f32 tiles, the 16-bit planes, the row-by-row tail
//  behind the exact kernel; k_rollout_wide_batch.hip, k_rollout_wide_split_batch.hip.  A batch keeps each problem's SOLO launch shape)
// (LAUNCH_ROLLOUT16: rollout16_kernel alone, the rollout of a tile shape's two-kernel iteration -- icem_plan_step_cem_batch; k_rollout.hip.
//  Each problem's solo launch shape)
enum LaunchFamily : int { LAUNCH_SAMPLE_ROLLOUT = 1, LAUNCH_ITER_AHEAD = 2, LAUNCH_MERGE_NOISE = 3, LAUNCH_SAMPLE = 4, LAUNCH_SAMPLE_MERGE = 5,
                          LAUNCH_ROLLOUT_HN = 6, LAUNCH_GK_SAMPLE = 7, LAUNCH_GK_SHIFT = 8, LAUNCH_GK_ROLLOUT_ROWS = 9, LAUNCH_GK_ROLLOUT_THREAD = 10,
                          LAUNCH_GK_SELECT = 11, LAUNCH_ROLLOUT_WIDE = 12, LAUNCH_ROLLOUT_WIDE_SPLIT = 13, LAUNCH_ROLLOUT_ROWS_WIDE = 14,
                          LAUNCH_ROLLOUT16 = 15 };
struct LaunchKey {
    int family = 0;
    int h = 0, d = 0, O = 0, kind = 0, arith = 0;   // (rollout_hn: O = the observation width o)
    int waves = 0;     // rollout waves per workgroup (sample_rollout: RW; iter_ahead, rollout_hn: WAVES)
    // sample_rollout: 0 = plain, 1 = lists merge in the prologue, 2 = records merge; iter_ahead: PM; merge_noise: 1 = with noise;
    // sample: the generator's rounds; sample_merge: 1 = lists merge, 2 = records merge; rollout_hn: the term program, N32 << 16 | N4 << 8 | NP
    // gk_sample: O = HMAX, waves = trajectories per workgroup, form = the generator's rounds; gk_rollout_*: O = the padded width
    // rollout_wide: O = o, arith = 1 (exact f32), waves = NT, form = EXT; rollout_wide_split: arith = 2 (fp16 planes) / 3 (bf16),
    // waves = NCT, form = EXT | FIVE << 1; rollout_rows_wide: O = o, form = EXT, wgs[0] = the tail's rows
    // rollout16: arith = 1 the fp16 planes (Tile16H), 0 exact f32 (Tile16); waves = WAVES
    int form = 0;
    int wgs[3] = {0, 0, 0};   // workgroups per role (of ONE problem); the grid is their sum
    bool operator==(const LaunchKey& o) const { return std::memcmp(this, &o, sizeof(LaunchKey)) == 0; }
};
struct MergeNoiseBatchArgs {
    MergeSingleArgs a;
    FastSampleArgs z1, z2;
};
// One recorded launch of one problem: the key and the family's argument block in its device-array form
struct LaunchDesc {
    LaunchKey key;
    static constexpr size_t BLOCK = sizeof(IterAheadArgs) > sizeof(RolloutArgs<double>) ? sizeof(IterAheadArgs) : sizeof(RolloutArgs<double>);
    static_assert(sizeof(SelectArgs<double>) <= BLOCK && sizeof(SampleArgs<double>) <= BLOCK, "LaunchDesc::block");
    // (every family's block is held to BLOCK by family_row's static_assert below: WideRolloutArgs, WideRowsArgs included)
    alignas(8) unsigned char block[BLOCK];
};
struct LaunchRecorder {
    unsigned long long base = 0;        // noise stream base of the recorded problem's step (BatchBases::v)
    std::vector<LaunchDesc> launches;
    bool unsupported = false;           // a launch without a batched form was reached (nothing was launched for it)
    const char* who = "icem_plan_step_batch: ";   // the recording entry's name, for the message of such a refusal
    void* add(const LaunchKey& key) {   // -> the new record's block, zeroed
        launches.emplace_back();
        launches.back().key = key;
        std::memset(launches.back().block, 0, sizeof(launches.back().block));
        return launches.back().block;
    }
};
// What the MPC step's call tree passes down instead of a bare stream
struct LaunchCtx {
    hipStream_t st = nullptr;
    BatchHint hint;
    LaunchRecorder* rec = nullptr;      // != nullptr: launches are recorded, not issued
};
// A launcher's one exit: `issue` launches now; recording, `form(block, base)` writes the device-array form of the arguments
template <class Form, class Issue>
void submit(const LaunchCtx& cx, const LaunchKey& key, bool batched_form, Form&& form, Issue&& issue) {
    if (!cx.rec) return issue();
    if (!batched_form) cx.rec->unsupported = true;
    else form(cx.rec->add(key), cx.rec->base);
}
// The device-array form of an argument block -> dst: sampling offsets relative to `base` (the kernels' add_base64, fused_dev.h,
// undoes it), unused offsets and dbg zero, the struct's tail padding zero -- a steady-state step's blocks compare equal as bytes
inline void sub_base(uint32_t& lo, uint32_t& hi, unsigned long long base) {
    const unsigned long long v = (((unsigned long long)hi << 32) | lo) - base;
    lo = (uint32_t)v;
    hi = (uint32_t)(v >> 32);
}
inline void batch_form(const FastIterArgs& a, unsigned long long base, void* dst) {
    std::memcpy(dst, &a, sizeof(a));
    FastSampleArgs& s = ((FastIterArgs*)dst)->s;
    if (s.n_shift == 0) s.off2_lo = s.off2_hi = 0;   // (unused)
    else sub_base(s.off2_lo, s.off2_hi, base);
    sub_base(s.off_lo, s.off_hi, base);
}
inline void batch_form(const IterAheadArgs& a, unsigned long long base, void* dst) {
    constexpr size_t defined = offsetof(IterAheadArgs, dbg_slot) + sizeof(int);   // (copies do not carry the tail padding)
    std::memcpy(dst, &a, defined);
    IterAheadArgs& g = *(IterAheadArgs*)dst;
    g.r.dbg = nullptr;
    if (g.z.n > 0) sub_base(g.z.off_lo, g.z.off_hi, base);
    else g.z.off_lo = g.z.off_hi = 0;
    if (g.s.n_shift > 0) {
        sub_base(g.s.off_lo, g.s.off_hi, base);
        sub_base(g.s.off2_lo, g.s.off2_hi, base);
    } else {
        g.s.off_lo = g.s.off_hi = g.s.off2_lo = g.s.off2_hi = 0;
    }
}
inline void batch_form(const MergeSingleArgs& a, const FastSampleArgs* z1, const FastSampleArgs* z2, unsigned long long base, void* dst) {
    MergeNoiseBatchArgs& g = *(MergeNoiseBatchArgs*)dst;   // (zeroed: a merge alone has z1.n == z2.n == 0)
    std::memcpy(&g.a, &a, sizeof(a));
    if (!z1) return;
    std::memcpy(&g.z1, z1, sizeof(*z1));
    std::memcpy(&g.z2, z2, sizeof(*z2));
    for (FastSampleArgs* z : {&g.z1, &g.z2}) {
        if (z->n > 0) sub_base(z->off_lo, z->off_hi, base);
        else z->off_lo = z->off_hi = 0;
        z->off2_lo = z->off2_hi = 0;
    }
}
// (dst is zeroed and the blocks are copied member by member: every byte of a recorded block is defined, whatever the padding of
//  the launcher's own copy held)
inline void batch_form(const FastSampleArgs& a, unsigned long long base, void* dst) {
    std::memcpy(dst, &a, sizeof(a));
    FastSampleArgs& s = *(FastSampleArgs*)dst;
    if (s.n_shift == 0) s.off2_lo = s.off2_hi = 0;   // (unused)
    else sub_base(s.off2_lo, s.off2_hi, base);
    sub_base(s.off_lo, s.off_hi, base);
}
inline void batch_form(const FastSampleMergeArgs& a, unsigned long long base, void* dst) {   // (world 1: no riding pack, PackPrev stays zero)
    FastSampleMergeArgs& g = *(FastSampleMergeArgs*)dst;
    batch_form(a.s, base, &g.s);
    std::memcpy(&g.m, &a.m, sizeof(a.m));
    g.m.dbg = nullptr;
}
// (member by member into the zeroed block: the padding behind planes / sbound / flip_th stays zero)
inline void batch_form(const WideRolloutArgs& a, void* dst) {
    WideRolloutArgs& g = *(WideRolloutArgs*)dst;
    g.n_rows = a.n_rows, g.n_cand = a.n_cand, g.K = a.K, g.o = a.o, g.d = a.d, g.h = a.h, g.kb = a.kb, g.xs = a.xs;
    g.planes = a.planes, g.minv = a.minv, g.ksc = a.ksc, g.csc = a.csc, g.sbound = a.sbound, g.cost_mode = a.cost_mode;
    g.lin_idx = a.lin_idx, g.flip_idx = a.flip_idx, g.ctrl_w = a.ctrl_w, g.lin_w = a.lin_w, g.flip_pen = a.flip_pen, g.flip_th = a.flip_th;
    g.cs = a.cs, g.dbg = nullptr, g.Mp = a.Mp, g.obs0 = a.obs0, g.actions = a.actions, g.costs = a.costs;
    g.part_c = a.part_c, g.part_i = a.part_i, g.part_k = a.part_k;
}
inline void batch_form(const WideRowsArgs& a, void* dst) {
    WideRowsArgs& g = *(WideRowsArgs*)dst;
    g.row0 = a.row0, g.n_tail = a.n_tail, g.o = a.o, g.d = a.d, g.h = a.h, g.cost_mode = a.cost_mode, g.wc = a.wc;
    g.cs = a.cs, g.A = a.A, g.B = a.B, g.obs0 = a.obs0, g.actions = a.actions, g.costs = a.costs;
}
inline void batch_form(const FastRolloutArgs& a, void* dst) {   // (member by member into the zeroed block: the padding stays zero)
    FastRolloutArgs& g = *(FastRolloutArgs*)dst;
    g.n_rows = a.n_rows, g.n_cand = a.n_cand, g.K = a.K, g.o = a.o, g.cost_mode = a.cost_mode;
    g.Mp = a.Mp, g.perm = a.perm, g.obs0 = a.obs0;
    g.ctrl_w = a.ctrl_w, g.lin_w = a.lin_w, g.flip_pen = a.flip_pen, g.flip_th = a.flip_th, g.flip_col = a.flip_col;
    g.actions = a.actions, g.costs = a.costs, g.part_c = a.part_c, g.part_i = a.part_i, g.part_k = a.part_k;
    g.list_wgs = a.list_wgs, g.dbg = nullptr, g.arith = a.arith, g.act_mag = a.act_mag, g.m_scale = a.m_scale, g.b_scale = a.b_scale;
    g.inv_m_scale = a.inv_m_scale, g.inv_b_scale = a.inv_b_scale;
    g.nonfinite = a.nonfinite;
}
inline void batch_form(const HnArgs& a, void* dst) {
    HnArgs& g = *(HnArgs*)dst;
    std::memcpy(&g.r, &a.r, sizeof(a.r));
    g.r.dbg = nullptr;
    g.A = a.A, g.B = a.B, g.lda = a.lda, g.ldb = a.ldb, g.wc = a.wc, g.cs = a.cs;
}
// The generic kernels' blocks (float64).  Their launchers fill a ZEROED block member by member (generic_kernels.hip), so a copy
// carries defined bytes throughout; the sampler's offset goes relative to the step's base, external noise and dbg are never batched
inline void batch_form(const SampleArgs<double>& a, unsigned long long base, void* dst) {
    SampleArgs<double>& g = *(SampleArgs<double>*)dst;   // (dst is zeroed)
    g.n = a.n, g.h = a.h, g.d = a.d, g.F = a.F, g.tpw = a.tpw;
    g.first_index = a.first_index;
    g.W = a.W, g.mean = a.mean, g.std = a.std, g.low = a.low, g.high = a.high;
    g.zr = nullptr, g.zi = nullptr;
    g.seed_lo = a.seed_lo, g.seed_hi = a.seed_hi, g.off_lo = a.off_lo, g.off_hi = a.off_hi;
    sub_base(g.off_lo, g.off_hi, base);
    g.t_begin = a.t_begin, g.row0_mean = a.row0_mean, g.white = a.white;
    g.out = a.out;
}
inline void batch_form(const RolloutArgs<double>& a, void* dst) {
    std::memcpy(dst, &a, sizeof(a));
    ((RolloutArgs<double>*)dst)->dbg = nullptr;
}
inline void batch_form(const SelectArgs<double>& a, void* dst) {
    std::memcpy(dst, &a, sizeof(a));
    ((SelectArgs<double>*)dst)->dbg = nullptr;
}
// the batched launches: args[n] in DEVICE memory (the problems' keys are equal: plan.hip checked)
// The batched sampler also serves the learned-dynamics step (icem_plan_step_learned*), which builds its key itself (family
// LAUNCH_SAMPLE, form 10, wgs[0] for the LARGEST problem, wgs[1] = 0) at any horizon fast_sample_supported admits: problem p
// draws args[p].n rows, surplus workgroups exit -- ragged row counts require n_shift == 0 in every block.  og.dst != nullptr:
// problem p's observation og.src[p] [og.width] is also copied to og.dst + p * og.width
struct ObsGather {
    const float* src[ICEM_MAX_BATCH];
    float* dst;
    int width;
};
void launch_sample_batch(const LaunchKey& key, const FastSampleArgs* args_dev, const BatchBases& bases, const ObsGather& og, int n, hipStream_t st);
void launch_sample_merge_batch(const LaunchKey& key, const FastSampleMergeArgs* args_dev, const BatchBases& bases, int n, hipStream_t st);
void launch_rollout_hn_batch(const LaunchKey& key, const HnArgs* args_dev, const BatchBases& bases, int n, hipStream_t st);   // (draws nothing: bases unused)
void launch_sample_rollout_batch(const LaunchKey& key, const FastIterArgs* args_dev, const BatchBases& bases, int n, hipStream_t st);
void launch_merge_batch(const LaunchKey& key, const MergeNoiseBatchArgs* args_dev, const BatchBases& bases, int n, hipStream_t st);
void launch_iter_ahead_batch(const LaunchKey& key, const IterAheadArgs* args_dev, const BatchBases& bases, int n, hipStream_t st);
// k_generic_batch.hip (float64; gk_sample_batch adds each problem's base to its block's offset, the others draw nothing)
void launch_gk_sample_batch(const LaunchKey& key, const SampleArgs<double>* args_dev, const BatchBases& bases, int n, hipStream_t st);
void launch_gk_shift_batch(const LaunchKey& key, const ShiftElitesArgs<double>* args_dev, const BatchBases& bases, int n, hipStream_t st);
void launch_gk_rollout_rows_batch(const LaunchKey& key, const RolloutArgs<double>* args_dev, const BatchBases& bases, int n, hipStream_t st);
void launch_gk_rollout_thread_batch(const LaunchKey& key, const RolloutArgs<double>* args_dev, const BatchBases& bases, int n, hipStream_t st);
void launch_gk_select_batch(const LaunchKey& key, const SelectArgs<double>* args_dev, const BatchBases& bases, int n, hipStream_t st);
// k_rollout_wide_batch.hip, k_rollout_wide_split_batch.hip (draw nothing: bases unused; grid = key.wgs[0] x n, the problem's own)
void launch_rollout_wide_batch(const LaunchKey& key, const WideRolloutArgs* args_dev, const BatchBases& bases, int n, hipStream_t st);
void launch_rollout_wide_split_batch(const LaunchKey& key, const WideRolloutArgs* args_dev, const BatchBases& bases, int n, hipStream_t st);
void launch_rollout_rows_wide_batch(const LaunchKey& key, const WideRowsArgs* args_dev, const BatchBases& bases, int n, hipStream_t st);
// k_rollout.hip (draws nothing: bases unused; grid = key.wgs[0] x n, the problem's own)
void launch_rollout16_batch(const LaunchKey& key, const FastRolloutArgs* args_dev, const BatchBases& bases, int n, hipStream_t st);
// is there a batched instantiation of the thread-form rollout at this width and model kind?  (rollout_cost_kernel<double, 32, tanh>
// spills registers -- tests/test_register_hygiene_cpu.py carries it -- and gets no twin)
inline bool gk_rollout_thread_batched(int O, int kind) { return !(O == 32 && kind == ICEM_MODEL_TANH); }
// LDS of the row-of-lanes rollout and the steps of actions it stages at a time: one rule for the solo and the batched launch
inline int gk_rollout_rows_ch(int O, int h, int d, size_t tsize) {
    const int tpw = 256 / (O <= 16 ? 16 : 32), ds = d <= 8 ? 8 : ((d + 1) & ~1);
    const int ch = (int)(32768 / ((size_t)tpw * ds * tsize));   /* at most 32 KB of actions */
    return ch < 1 ? 1 : (ch > h ? h : ch);
}
inline size_t gk_rollout_rows_lds(int O, int h, int d, size_t tsize) {
    const int tpw = 256 / (O <= 16 ? 16 : 32), os = (O + 1) & ~1, ds = d <= 8 ? 8 : ((d + 1) & ~1);
    return ((size_t)2 * tpw * os + (size_t)d * os + (size_t)tpw * gk_rollout_rows_ch(O, h, d, tsize) * ds) * tsize;
}
inline size_t gk_sample_quad_lds(int tpw, int h, int d, int hmax, size_t tsize) {
    return ((((size_t)tpw * h * d + 1) & ~(size_t)1) + (size_t)h * hmax) * tsize;
}
inline void launch_sample_batch_recorded(const LaunchKey& key, const FastSampleArgs* args_dev, const BatchBases& bases, int n, hipStream_t st) {
    launch_sample_batch(key, args_dev, bases, ObsGather{}, n, st);
}

// The launch families, each written once: the size of the family's argument block and its batched launch.  A recorded launch
// whose family has no row here is refused by every batched entry (launch_family -> nullptr; RecordedBatch::check, recorded_batch.h).
struct LaunchFamilyRow {
    int family;
    size_t block_bytes;
    void (*launch)(const LaunchKey& key, const void* args_dev, const BatchBases& bases, int n, hipStream_t st);
};
template <class Args, void (*Fn)(const LaunchKey&, const Args*, const BatchBases&, int, hipStream_t)>
void launch_typed(const LaunchKey& key, const void* args_dev, const BatchBases& bases, int n, hipStream_t st) {
    Fn(key, (const Args*)args_dev, bases, n, st);
}
template <class Args, void (*Fn)(const LaunchKey&, const Args*, const BatchBases&, int, hipStream_t)>
constexpr LaunchFamilyRow family_row(int family) {
    static_assert(sizeof(Args) <= sizeof(LaunchDesc::block), "LaunchDesc::block");
    return {family, sizeof(Args), &launch_typed<Args, Fn>};
}
constexpr LaunchFamilyRow LAUNCH_FAMILIES[] = {
    family_row<FastIterArgs, launch_sample_rollout_batch>(LAUNCH_SAMPLE_ROLLOUT),
    family_row<IterAheadArgs, launch_iter_ahead_batch>(LAUNCH_ITER_AHEAD),
    family_row<MergeNoiseBatchArgs, launch_merge_batch>(LAUNCH_MERGE_NOISE),
    family_row<FastSampleArgs, launch_sample_batch_recorded>(LAUNCH_SAMPLE),
    family_row<FastSampleMergeArgs, launch_sample_merge_batch>(LAUNCH_SAMPLE_MERGE),
    family_row<HnArgs, launch_rollout_hn_batch>(LAUNCH_ROLLOUT_HN),
    family_row<SampleArgs<double>, launch_gk_sample_batch>(LAUNCH_GK_SAMPLE),
    family_row<ShiftElitesArgs<double>, launch_gk_shift_batch>(LAUNCH_GK_SHIFT),
    family_row<RolloutArgs<double>, launch_gk_rollout_rows_batch>(LAUNCH_GK_ROLLOUT_ROWS),
    family_row<RolloutArgs<double>, launch_gk_rollout_thread_batch>(LAUNCH_GK_ROLLOUT_THREAD),
    family_row<SelectArgs<double>, launch_gk_select_batch>(LAUNCH_GK_SELECT),
    family_row<WideRolloutArgs, launch_rollout_wide_batch>(LAUNCH_ROLLOUT_WIDE),
    family_row<WideRolloutArgs, launch_rollout_wide_split_batch>(LAUNCH_ROLLOUT_WIDE_SPLIT),
    family_row<WideRowsArgs, launch_rollout_rows_wide_batch>(LAUNCH_ROLLOUT_ROWS_WIDE),
    family_row<FastRolloutArgs, launch_rollout16_batch>(LAUNCH_ROLLOUT16),
};
inline const LaunchFamilyRow* launch_family(int family) {
    for (const LaunchFamilyRow& r : LAUNCH_FAMILIES)
        if (r.family == family) return &r;
    return nullptr;
}

// workgroups (= candidate lists) of that launch; 0 if this shape / generator / size has no single-launch kernel
// (n_tail trailing shifted-elite rows; *tail_out > 0: that many rows behind the lists are scored through the cost array)
int sample_rollout_lists(const BatchHint& bh, int h, int d, int O, int rounds, int n_rows, int n_tail = 0, int* tail_out = nullptr);
// may iteration `it >= 1` with n_rows rows fold the previous iteration's merge into its own launch?
bool sample_rollout_merge_ok(const BatchHint& bh, int h, int d, int O, int rounds, int n_rows, int K);
void launch_sample_rollout(const LaunchCtx& cx, const FastIterArgs& a, int h, int d, int O, int kind, bool merge_prologue);

}  // namespace icem
