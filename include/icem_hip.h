/*
 * icem_hip.h -- C ABI of libicem_hip.so: the MI355X-native iCEM inner planning loop.
 *
 * This is the drop-in boundary for ONE hot path of martius-lab/iCEM: everything inside the
 * `for i in range(opt_iter)` loop of MpcICem.get_action (reference icem/controllers/icem.py:106-189).
 * The whole loop is one call for the built-in models (icem_plan_step, icem_plan_step_batch, icem_get_action) and for the
 * learned-dynamics model (icem_plan_step_learned, icem_plan_step_learned_batch); its stages are calls of their own too.
 * The reference is pure Python/NumPy and has no FFI; each entry point below names the reference
 * call site (file:line, relative to /root/reference) whose arithmetic it replaces.  The binding a
 * reference maintainer would add is a ctypes stub -- see INTEGRATION.md.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no C++/torch types.
 *   - Every pointer is a DEVICE pointer owned by the caller (e.g. torch tensor.data_ptr())
 *     unless its name ends in `_host`.  `stream` is a hipStream_t passed as void*
 *     (torch.cuda.current_stream().cuda_stream); all work is enqueued on it and nothing
 *     synchronises unless stated.
 *   - `dtype` selects the arithmetic/storage type of every floating tensor of a call:
 *     ICEM_F32 (throughput) or ICEM_F64 (the reference's type; strict-parity mode).
 *   - Return value: 0 on success, <0 on error (ICEM_E_*); icem_last_error() returns a
 *     thread-local message.  No exceptions cross the boundary.
 *   - Tensor layouts are C-contiguous: actions [n, h, d]; mean/std [h, d]; low/high [d];
 *     white noise z_r/z_i [n, d, F] with F = h/2+1 (the layout of the reference's draws).
 *   - A handle is not thread-safe; different handles may be used concurrently.
 */
#ifndef ICEM_HIP_H
#define ICEM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ICEM_ABI_VERSION 6 /* 6: icem_step_status removed (icem_rssm_rollout_cost_batch and the learned-dynamics step -- icem_plan_step_learned, icem_plan_step_learned_batch, icem_plan_step_learned_ok, icem_learned_step_launches -- were added without a new number: an added symbol breaks no caller); 5: ICEM_TILE_AUTO serves the fp16 planes only where no state can leave their range (icem_tile_growth), icem_nonfinite_costs / ICEM_E_RANGE, icem_set_option (the library reads no environment variable), icem_plan_step_batch; 2: icem_build_hash, icem_allgather_elites / icem_rccl_*, noise-ahead planning; ICEM_MAX_OBS_DIM 384; 3: icem_set_tile_arith; 4: icem_set_wide_arith (default AUTO), ICEM_TILE_AUTO = planes at every population */

enum { ICEM_F32 = 0, ICEM_F64 = 1 };
enum { ICEM_COST_SUM = 0, ICEM_COST_BEST = 1, ICEM_COST_FINAL = 2 }; /* abstract_controller.py:82-87 */
enum { ICEM_MODEL_LINEAR = 0, ICEM_MODEL_TANH = 1 };

enum {
    ICEM_OK = 0,
    ICEM_E_INVALID = -1,      /* bad argument (the reference raises ValueError/AttributeError)   */
    ICEM_E_UNSUPPORTED = -2,  /* shape outside the compiled kernels (NotImplementedError)          */
    ICEM_E_HIP = -3,          /* a HIP runtime call failed                                         */
    ICEM_E_NO_DEVICE = -4,    /* no gfx950 device visible                                          */
    ICEM_E_STATE = -5,        /* call order violated (e.g. rollout before icem_set_model)          */
    ICEM_E_RANGE = -6         /* icem_get_action: the step's outputs are returned, but trajectories came back with a
                                 non-finite cost from a finite observation (a state left the arithmetic's range)       */
};

#define ICEM_MAX_HORIZON 64
#define ICEM_MAX_ACT_DIM 64
#define ICEM_MAX_OBS_DIM 384
#define ICEM_MAX_ELITES 64

/* Constructor kwargs of MpcICem (icem.py:213-233, mpc.py:22, abstract_controller.py:64-65). */
typedef struct icem_config {
    int32_t horizon;              /* h                                                   */
    int32_t act_dim;              /* d  = env.action_space.shape[0] (icem.py:245)        */
    int32_t num_traj;             /* N  = num_simulated_trajectories (GLOBAL, all ranks) */
    int32_t num_elites;           /* K  = min(elites_size, N/2), >= 2 (icem.py:235-240)  */
    int32_t elites_size;          /* raw elites_size (the N-decay floor is 2*elites_size, icem.py:127) */
    int32_t opt_iters;            /* opt_iterations                                      */
    int32_t cost_mode;            /* ICEM_COST_*  (cost_along_trajectory)                */
    int32_t use_mean_actions;     /* icem.py:87-88                                       */
    int32_t keep_previous_elites; /* icem.py:143-145                                     */
    int32_t shift_elites;         /* icem.py:131-137                                     */
    int32_t dtype;                /* ICEM_F32 / ICEM_F64                                 */
    int32_t rng_rounds;           /* Philox4x32 rounds: 10 (default) or 7                */
    int32_t rank;                 /* this process' shard of the N dimension              */
    int32_t world;                /* number of shards (GPUs)                             */
    double factor_decrease;       /* gamma = factor_decrease_num                         */
    double alpha;                 /* momentum                                            */
    double init_std;              /* relative to (high-low)/2 (icem.py:55-59)            */
    double fraction_reused;       /* xi = fraction_elites_reused                         */
    double noise_beta;            /* colored-noise exponent; <= 0: white noise (icem.py:77) */
    uint64_t seed;                /* Philox key                                          */
} icem_config;

/* Parametric form of the shipped cost functions (environments/mujoco.py:67-99 HalfCheetah,
 * :259-277 HumanoidStandup):
 *   cost_t = ctrl_weight*sum_j a_j^2 + lin_weight*obs[lin_idx]
 *            + flip_penalty*([obs[flip_idx] > flip_thresh] + [obs[flip_idx] < -flip_thresh])
 * with the flip term dropped when flip_idx < 0 and the linear term when lin_weight == 0 (lin_idx must still be a
 * valid index).  `obs` is the PRE-action observation. */
typedef struct icem_cost_spec {
    double ctrl_weight;
    double lin_weight;
    double flip_penalty;
    double flip_thresh;
    int32_t lin_idx;
    int32_t flip_idx;
} icem_cost_spec;

/* The remaining parametric cost functions of the reference's environments, as extra terms on top of
 * icem_cost_spec (a zero-initialised struct with diff_idx = health_idx = box_from = -1 and n_terms = 0 is "off"):
 *   + diff_weight * (next_obs[diff_idx] - obs[diff_idx])            Ant, Hopper: -x_velocity = -(x' - x)/dt
 *                                                                    (environments/mujoco.py:164, 218)
 *   + health_penalty * unhealthy(obs),  unhealthy = 1 - all_finite(obs) * [lo <(=) obs[health_idx] <(=) hi]
 *                                                   * [box_lo < obs[k] < box_hi for all k >= box_from]
 *       Ant :146-149,166 (closed range), Hopper :189-203,221 (open range + healthy_state_range over obs[2:];
 *       its healthy_angle is dropped by the reference itself, :199), Humanoid :302-315,338 (open range)
 *   + sum over terms[0 .. n_terms) of  weight * gate * f,  gate = [obs[gate_idx] > gate_thresh] (1 if gate_idx < 0;
 *     a product as in the reference, so a non-finite f is not masked by a closed gate),
 *     with r = || obs[a .. a+len) - obs[b .. b+len) ||  (b < 0: the norm of the slice itself) and f by kind:
 *       ICEM_TERM_NORM       r                    Reacher :366-368, FetchPickAndPlace / FetchReach
 *                                                 environments/robotics.py:150-164, 286-295, Door / Relocate
 *                                                 environments/mjenvs.py:64, 161, 166 (the latter gated on the lift)
 *       ICEM_TERM_NORM_GT    [r > thresh]         the sparse robotics costs robotics.py:159-161, 291-292
 *       ICEM_TERM_NORM_LT    [r < thresh]         Relocate's closeness bonuses mjenvs.py:170-172
 *       ICEM_TERM_SQ_OFFSET  (obs[a] - thresh)^2  Door's hinge target mjenvs.py:68
 *       ICEM_TERM_SUMSQ      sum_k obs[a+k]^2     Door's velocity cost mjenvs.py:70
 *       ICEM_TERM_STEP_GT    [obs[a] > thresh]    Door's opening bonuses :74-76, Relocate's lift bonus :162 */
enum { ICEM_TERM_NORM = 0, ICEM_TERM_NORM_GT = 1, ICEM_TERM_NORM_LT = 2, ICEM_TERM_SQ_OFFSET = 3, ICEM_TERM_SUMSQ = 4,
       ICEM_TERM_STEP_GT = 5 };
#define ICEM_MAX_COST_TERMS 8
#define ICEM_MAX_TERM_LEN 64

typedef struct icem_cost_term {
    double weight, thresh, gate_thresh;
    int32_t kind;
    int32_t a, b, len;      /* b = -1: no second slice; len <= ICEM_MAX_TERM_LEN (1 for the scalar kinds) */
    int32_t gate_idx;       /* -1: not gated */
    int32_t reserved;
} icem_cost_term;

typedef struct icem_cost_terms {
    double diff_weight;
    double health_penalty, health_lo, health_hi;
    double box_lo, box_hi;
    int32_t diff_idx;        /* -1: off */
    int32_t health_idx;      /* -1: off */
    int32_t health_closed;   /* 1: lo <= z <= hi, 0: lo < z < hi */
    int32_t box_from;        /* -1: off */
    int32_t n_terms;
    int32_t reserved;
    icem_cost_term terms[ICEM_MAX_COST_TERMS];
} icem_cost_terms;

typedef struct icem_handle icem_handle;

/* ---- library / handle ------------------------------------------------------------------ */

int icem_abi_version(void);
const char* icem_last_error(void);
/* Hash (16 hex digits) of the sources this binary was built from -- what `python -m icem_amd.build` compares with the
 * tree to tell a stale library from a current one (no reference counterpart: the reference is interpreted Python). */
const char* icem_build_hash(void);

/* Number of visible HIP devices (0 on a CPU-only host); never fails. */
int icem_device_count(void);

/* Creates a planner for one controller instance (replaces MpcICem.__init__ state, icem.py:22-29).
 * Builds the colored-noise synthesis table on the current device. */
int icem_create(const icem_config* cfg, icem_handle** out);
int icem_destroy(icem_handle* h);

/* Episode number of the rollout being planned, folded into the device noise streams (high word of the stream offset,
 * the sampling call number mpc_step*(opt_iters+1)+it is the low word): the reference draws from one np.random stream
 * that runs on across episodes (icem.py:73-77), so consecutive episodes must not replay the same exploration noise.
 * 0 after icem_create; the host mirror advances it in beginning_of_rollout (icem.py:31-43).  episode < 2^32. */
int icem_set_episode(icem_handle* h, uint64_t episode);

/* Sequence of population sizes N_i the loop will use (icem.py:123-127); out_host[opt_iters]. */
int icem_population_sizes(const icem_handle* h, int32_t* out_host);

/* Colored-noise synthesis matrices (float64, host): y[t] = sum_k z_r[k]*cr[k*h+t] + z_i[k]*ci[k*h+t]
 * restating colorednoise.powerlaw_psd_gaussian (third-party; call site icem.py:73-75). */
int icem_noise_tables_host(int32_t horizon, double beta, double* cr_host, double* ci_host);

/* Built-in batched forward model o' = act(o.A + a.B) (the `predict` contract of
 * models/abstract_models.py:17-26).  A [obs_dim, obs_dim], B [act_dim, obs_dim] are HOST float64
 * arrays; they are converted to the handle dtype and copied to the device.  `kind` = ICEM_MODEL_*.
 * obs_dim <= 32: every kernel family (f32 / f64).  32 < obs_dim <= 384 (HumanoidStandup's o = 378,
 * environments/mujoco.py:241-252): dtype f32 only, the model step runs as an exact-f32 GEMM on the matrix pipe
 * (icem_rollout_cost without `observations`, icem_plan_*); cost = icem_set_cost's form + icem_set_cost_terms
 * (Ant's o = 111/113, Humanoid's 376, Door / Relocate's 39: mujoco.py:151-171, 317-343, mjenvs.py:57-78, 155-174). */
int icem_set_model(icem_handle* h, int32_t kind, int32_t obs_dim, const double* A_host, const double* B_host);
int icem_set_cost(icem_handle* h, const icem_cost_spec* spec);
/* Extra cost terms (NULL switches them off again).  With any of them on, icem_rollout_cost / icem_plan_* evaluate
 * the cost in the general rollout kernel (one thread per trajectory) for obs_dim <= 32 and inside the matrix-pipe
 * rollout of k_rollout_wide.hip for 32 < obs_dim <= 384. */
int icem_set_cost_terms(icem_handle* h, const icem_cost_terms* terms);

/* ---- stateless operators (each replaces one NumPy call site) ------------------------------ */

/* K1  MpcICem.sample_action_sequences (icem.py:61-82) + colorednoise.powerlaw_psd_gaussian:
 *   actions[i, t, j] = clip(colored(i, j)[t] * std[t, j] + mean[t, j], low[j], high[j]),  i < n.
 * White noise: if z_r/z_i are non-NULL they are the [n, d, F] standard-normal draws (parity mode:
 * the same draws the reference takes from np.random); otherwise Philox4x32 keyed by
 * (cfg.seed, offset, first_index + i, j).  Only time steps t >= t_begin are written
 * (t_begin = h-1 restates the time_slice=slice(-1, None) call of icem.py:102).
 * cfg.noise_beta <= 0 is the reference's white branch (np.random.randn(num_traj, h, d), icem.py:77): no synthesis,
 * draw t of row (i, j) is its sample at step t; an external draw is then passed as z_r = randn [n, h, d], z_i NULL.
 * If row0_mean != 0 and first_index == 0, row 0 is overwritten with `mean` (icem.py:87-88). */
int icem_sample_clip(icem_handle* h, int32_t n, int64_t first_index, const void* mean, const void* std,
                     const void* low, const void* high, const void* z_r, const void* z_i,
                     uint64_t offset, int32_t t_begin, int32_t row0_mean, void* actions, void* stream);

/* MpcCemStd.sample_action_sequences (the CEM baseline, icem/controllers/mpc.py:188-198):
 *   actions[i, t, j] = mean[t, j] + std[t, j] * truncnorm.ppf(u[i, t, j]; lower[t, j], upper[t, j])
 * (scipy.stats.truncnorm.rvs draws ONE uniform(size=(n, h, d)) per call).  u: those uniforms [n, h, d] (parity mode),
 * or NULL: word t of the Philox / xoshiro stream of row (first_index + i, j), offset as in icem_sample_clip.
 * lower / upper are [h, d] in standard-normal units, as MpcCemStd keeps them. */
int icem_sample_truncnorm(icem_handle* h, int32_t n, int64_t first_index, const void* mean, const void* std,
                          const void* lower, const void* upper, const void* u, uint64_t offset, void* actions,
                          void* stream);
/* MpcCemStd._update_bounds (mpc.py:290-301): like_levine != 0 caps std at half the distance to the action bounds
 * (in place, floor 1e-8) and sets lower / upper = -2 / +2; otherwise lower / upper = (low|high - mean) / (std + 1e-8). */
int icem_cem_bounds(icem_handle* h, int32_t like_levine, const void* mean, void* std, const void* low, const void* high,
                    void* lower, void* upper, void* stream);

/* MpcCemStd.get_action (mpc.py:200-262) as ONE call: the loop a caller would otherwise drive operator by operator
 * (icem_sample_truncnorm, icem_rollout_cost, icem_update_distribution or icem_topk_sorted + icem_gather_refit,
 * icem_cem_bounds), a chain of launches with no host round trip.  Per CEM iteration i of MPC step s (mpc.py:207-228):
 *   - cfg.num_traj rows are drawn with icem_sample_truncnorm's arithmetic from (mean, std, lower, upper) at stream offset
 *     (episode << 32) + s * opt_iters + i (mpc.py:188-198; device uniforms);
 *   - they are rolled out by the launch icem_rollout_cost picks for this handle (mpc.py:56-67: every model width, tile / wide /
 *     f64 arithmetic and cost-term list the operator serves);
 *   - the K = cfg.num_elites best rows in (cost, index) order go to elites / elite_costs / elite_idx and mean / std are
 *     refitted with cfg.alpha (mpc.py:270-281), then lower / upper -- and std under like_levine -- follow as icem_cem_bounds
 *     writes them (_update_bounds, mpc.py:290-301).
 * Behind the last iteration: executed = elites[0, 0, :] under execute_best_elite, else mean[0, :] as refitted and before the
 * shift (mpc.py:230-233); best_cost = elite_costs[0]; with shift_means the mean's rows move up one and the last row keeps its
 * value, or is zero under like_levine (mpc.py:236-243 with the default compute_new_mean, mpc.py:265-269), without it the
 * mean is set to 0; std is reset to what icem_reset_distribution writes and lower / upper follow once more (mpc.py:244-245).
 * actions / costs hold the last iteration's pool afterwards.  3 launches per iteration, none in between; no host
 * synchronisation; no allocation after the first call.  Every output is bit for bit what the operators give.
 *   Served: f32 handles where icem_update_distribution_ok(num_traj, K); f64 handles whose pool the one-launch selection
 * admits; world == 1, rng_rounds 7 and 10, profiling off, factor_decrease == 1, keep_previous_elites and shift_elites off
 * (MpcCemStd has neither, mpc.py:142-327); development option cem_step = 0 switches the entry off.  Anything else is
 * ICEM_E_UNSUPPORTED; a NULL argument or a negative mpc_step ICEM_E_INVALID; no model or cost set ICEM_E_STATE.  Whatever
 * is refused is refused before anything is launched. */
typedef struct icem_cem_params { int32_t like_levine, shift_means, execute_best_elite, reserved; } icem_cem_params; /* mpc.py:303-327 */
typedef struct icem_cem_buffers {   /* all device, handle dtype */
    void *mean, *std;        /* [h,d] in/out, persistent (mpc.py:158-170)      */
    void *lower, *upper;     /* [h,d] in/out, standard-normal units (mpc.py:290-301) */
    void *low, *high;        /* [d]                                            */
    void *obs0;              /* [obs_dim]                                      */
    void *actions, *costs;   /* [N,h,d], [N]: the last iteration's pool        */
    void *elites, *elite_costs; int32_t* elite_idx;   /* [K,h,d], [K], [K] (mpc.py:270-271) */
    void *executed, *best_cost;                        /* [d], [1] (mpc.py:230-233) */
    void *workspace;         /* icem_topk_workspace_bytes(N, K), may be unused */
} icem_cem_buffers;
int     icem_plan_step_cem_ok(const icem_handle* h);   /* 1 if THIS handle is served, else 0 */
int     icem_plan_step_cem(icem_handle* h, const icem_cem_buffers* b, const icem_cem_params* p, int32_t mpc_step, void* stream);
int64_t icem_cem_step_launches(const icem_handle* h);  /* kernel launches of the last such step of this handle; measurement */
/* The same step for n planners of ONE configuration at once: the reference compares the CEM baseline with iCEM over many
 * episodes and seeds and runs those controllers side by side (icem/misc/rollout_utils.py:46-58, 129-152), each its own
 * MpcCemStd.get_action (mpc.py:200-262).  One problem leaves the chip mostly empty and its step is a chain of 3 * opt_iters
 * launch latencies; n problems share those launches: the sampler, the rollout and the update of an iteration are each ONE
 * launch for all of them (blockIdx.y = the problem, its argument block read from device memory) -- 3 launches per iteration
 * whatever n, no host round trip, no allocation after the first call of a batch size.
 *   handles[n], n in [1, 32]: no NULL, no handle twice, one configuration -- everything but the seed equal (as for
 * icem_plan_step_learned_batch); models, costs, observations, seeds, episodes differ.  p: one set of flags for the batch.
 * mpc_steps_host[n]: the MPC step of every problem (a controller that was reset later than its neighbours steps with them).
 * buffers[i]: problem i's, as for icem_plan_step_cem (workspace may be NULL).  results: NULL, or a device buffer [n, d + 1]
 * of the handle dtype -- row i is executed | best_cost of problem i, written by the last update in addition to the
 * problem's own executed / best_cost (one device-to-host copy fetches the batch).
 *   Every output of problem i -- mean, std, lower, upper, elites, elite_costs, elite_idx, executed, best_cost, the last
 * pool and its costs -- is bit for bit what icem_plan_step_cem gives for that handle alone at the same seed, episode and
 * step: the batched kernels run the solo kernels' bodies.
 *   Served: handles icem_plan_step_cem serves whose rollout launch has a batched twin -- the tile shapes (HalfCheetah ...), the
 * TileHN shapes, the GEMM-kernel shapes, the float64 generic rollouts -- and whose rollout launches are equal in shape (tile /
 * wide / f64 arithmetic, cost-term program).  ICEM_E_INVALID: n outside [1, 32], a NULL argument, handle or buffer, a handle
 * twice, unequal configurations, a negative step; ICEM_E_UNSUPPORTED: a handle icem_plan_step_cem refuses, a rollout without a
 * batched form (the f32 thread-per-trajectory kernel, the float64 matrix-core rollout, the float64 thread form at padded width 32
 * with a tanh model), and for n > 1 a shape whose row does not fit the step's sampler; ICEM_E_STATE: no model or cost set, or the
 * problems' rollout launches differ.  Whatever is refused is refused before anything is launched.  n == 1 is
 * icem_plan_step_cem (+ the results row).  Development option cem_step = 0 switches this entry off too. */
int     icem_plan_step_cem_batch(icem_handle* const* handles, int32_t n, const icem_cem_buffers* buffers, const icem_cem_params* p,
                                 const int32_t* mpc_steps_host, void* results, void* stream);
int64_t icem_cem_batch_launches(const icem_handle* h); /* kernel launches of the last such batch this handle led as handles[0]; measurement */
/* The same step through the LEARNED dynamics -- the declared RSSM of icem_rssm_rollout_cost, BASELINE configs[4]; the planner
 * PlaNet itself uses and the baseline of the reference's "iCEM with PlaNet" column -- for one planner and for n planners at once.
 * The step is icem_plan_step_cem's in every respect but the rollout: per iteration cfg.num_traj rows drawn with
 * icem_sample_truncnorm's arithmetic at stream offset (episode << 32) + s * opt_iters + i, rolled out through the RSSM (params:
 * the packed parameter buffer of icem_rssm_rollout_cost, shared by the problems of a batch) under the handle's cost_mode, the K
 * best rows in (cost, index) order gathered and refitted with alpha, the bounds as icem_cem_bounds writes them, the epilogue
 * behind the last iteration.  icem_cem_buffers and icem_cem_params are icem_plan_step_cem's: b->obs0 is [ICEM_RSSM_OBS_DIM] f32,
 * workspace is unused.  No built-in model or cost need be set on the handle.  The stream offsets are the operator loop's and
 * icem_plan_step_cem's: a caller may alternate freely between the loop, the solo entry and the batched entry.
 *   3 launches per iteration whatever n (3 * opt_iters in all; reported by icem_cem_step_launches for the solo entry and by
 * icem_cem_batch_launches of handles[0] for the batched one), no host synchronisation, no allocation after the first call of a
 * batch size on a stream.  Every output of the solo entry -- mean, std, lower, upper, elites, elite_costs, elite_idx, executed,
 * best_cost, the last pool in actions / costs -- is bit for bit what the operator loop gives (icem_sample_truncnorm,
 * icem_rssm_rollout_cost, icem_update_distribution, icem_cem_bounds).  Every problem of a batch is bit for bit its own solo step
 * on the first nine of those and on its row of results ([n, act_dim + 1] f32: executed | best cost; may be NULL).  A batch scores
 * its rows back to back in a pool owned by handles[0] (the batched RSSM launch wants them contiguous): for n > 1 A PROBLEM'S OWN
 * actions / costs ARE SCRATCH -- they must be valid, their contents afterwards are unspecified.  The problems' obs0 buffers need
 * not be adjacent: the first iteration's sampler launch gathers them into the pool's [n, 230] table.  The batch's argument blocks
 * live in a device array of handles[0] and are uploaded only when a byte changed (icem_batch_uploads: the steady state uploads
 * nothing).  n == 1 is the solo step plus the results row.
 *   Served: f32 handles, world == 1, act_dim == the RSSM's action width (6, or the handle's own 1 .. 32 once icem_set_rssm_act_dim has bound it),
 * rng_rounds 7 or 10, profiling off, factor_decrease == 1, keep_previous_elites and
 * shift_elites off, icem_update_distribution_ok(num_traj, K), a row that fits the step's sampler, a population the RSSM's split
 * launch takes (for a batch: all problems' tiles together), any horizon the handle and that launch accept.  Development option
 * cem_step = 0 switches these entries off too.  ICEM_E_INVALID: a NULL handle / buffers / flags / params, a negative step, a NULL
 * buffer other than workspace, n outside [1, 32], a handle twice, unequal configurations; ICEM_E_UNSUPPORTED: anything not served;
 * ICEM_E_STATE: the learned-dynamics rollout's own rules (its staging area's first call of a size must not be under capture; its
 * host-visible status word, looked at before the step's first launch).  Whatever is refused is refused before anything is
 * launched or any handle touched.
 *   Measured (EXPERIMENTS R15.1; N = 1024, h = 12, K = 10, 5 iterations, MpcCemStdHip.get_action): 0.50 ms against 0.57 ms for the
 * operator loop in the same process (1.14 x: the rollout's 74 us of every iteration are the same in both; sampler 12 us, update +
 * bounds 23 us); batched, per step of the batch against B solo steps: B = 2 0.52 / 0.96 ms, B = 4 0.68 / 1.89, B = 8 1.01 / 3.76,
 * B = 16 1.71 / 7.47 ms (1.9 x to 4.4 x). */
int     icem_plan_step_cem_learned_ok(const icem_handle* h);   /* 1 if THIS handle is served, else 0 */
int     icem_plan_step_cem_learned(icem_handle* h, const icem_cem_buffers* b, const icem_cem_params* p, const void* params,
                                   int32_t mpc_step, void* stream);
int     icem_plan_step_cem_learned_batch(icem_handle* const* handles, int32_t n, const icem_cem_buffers* buffers,
                                         const icem_cem_params* p, const void* params, const int32_t* mpc_steps_host, void* results,
                                         void* stream);

/* MpcRandom.sample_action_sequences (icem/controllers/mpc.py:96-109, random shooting): actions[i, t, :] = low +
 * (high - low) * U(block), uniform draws held for consecutive calls of MpcRandom.sample() (mpc.py:96-102) -- one call
 * per (trajectory, step) pair in row-major order, the call counter running on across MPC steps: call c =
 * call_offset + i*h + t uses block 0 (the action drawn at construction) while c < change_freq, then block
 * 1 + (c - change_freq) / (change_freq + 1).  u: uniforms [*, d] for blocks first_block, first_block + 1, ...
 * (parity mode: env.action_space.sample()'s draws), or NULL for the Philox path (keyed by the block index). */
int icem_sample_piecewise(icem_handle* h, int32_t n, int64_t call_offset, int32_t change_freq, int64_t first_block,
                          const void* low, const void* high, const void* u, void* actions, void* stream);

/* MpcRandom.get_action (mpc.py:114-138) as ONE call: the chain a caller would otherwise drive operator by operator
 * (icem_sample_piecewise, icem_rollout_cost, icem_topk_sorted(costs, 1) and the gathers behind it), with no host round trip:
 *   - actions [N, h, d] <- icem_sample_piecewise(N = cfg.num_traj, call_offset, change_freq, first_block, low, high, u), drawn by
 *     the step's own sampler: a workgroup draws every held (block, dimension) value its elements need ONCE into LDS and stores
 *     its span of the pool from there -- the generator work of a launch falls by about change_freq + 1; the same bits;
 *   - costs [N] <- the launch icem_rollout_cost picks for this handle (every model width, tile / wide / f64 arithmetic and
 *     cost-term list the operator serves);
 *   - ONE selection launch: best = the row of the smallest (cost, index) pair, NaN counted as +inf (np.argmin, mpc.py:122, as
 *     icem_topk_sorted(costs, 1) gives it); best_actions = actions[best]; result = actions[best, 0, :] | the cost
 *     icem_topk_sorted reports for that row | best -- the index stored as a value of the handle dtype (exact: f32 handles with
 *     num_traj > 2^24 are refused).  One device-to-host copy of result fetches all a controller needs.
 * 3 launches on the one-launch rollouts, no host synchronisation, no allocation after the first call.  call_offset is
 * MpcRandom's counter of sample() calls (mpc.py:95-102) and is the caller's: the entry keeps no per-handle step state, so
 * the operator chain and the entry may alternate.  u != NULL is icem_sample_piecewise's parity mode (the caller's uniforms
 * for blocks first_block ..).
 *   Served: world == 1, profiling and debug stamps off, rng_rounds 7 and 10, f32 and f64, whatever icem_rollout_cost serves
 * for the handle; development option random_step = 0 switches both entries off.  ICEM_E_INVALID: a NULL argument or buffer,
 * change_freq < 0 or >= horizon, a negative call_offset; ICEM_E_STATE: no model or cost set; ICEM_E_UNSUPPORTED: anything
 * else.  Whatever is refused is refused before anything is launched or the handle touched. */
typedef struct icem_random_buffers {      /* all device, handle dtype */
    void *low, *high;                     /* [d]                                             */
    void *obs0;                           /* [obs_dim]                                       */
    void *actions, *costs;                /* [N,h,d], [N]: the step's pool (mpc.py:120-123)  */
    void *best_actions;                   /* [h,d]: the cheapest row (mpc.py:129-131)        */
    void *result;                         /* [d+2]: executed | best_cost | best index        */
} icem_random_buffers;
int     icem_plan_step_random_ok(const icem_handle* h);   /* 1 if THIS handle is served, else 0 */
int     icem_plan_step_random(icem_handle* h, const icem_random_buffers* b, int32_t change_freq, int64_t call_offset,
                              int64_t first_block, const void* u, void* stream);
int64_t icem_random_step_launches(const icem_handle* h);  /* kernel launches of the last such step of this handle; measurement */
/* The same step for n planners of ONE configuration at once (the reference runs its baseline episodes side by side,
 * icem/misc/rollout_utils.py:46-58, 129-152): the sampler, the rollout and the selection are each ONE launch for all of them
 * (blockIdx.y = the problem, its argument block read from a device array of handles[0]).  Admission is
 * icem_plan_step_cem_batch's: n in [1, 32], no NULL, no handle twice, everything but the seed equal, rollout launches equal in
 * shape and each with a batched twin; models, costs, seeds, observations and call offsets (call_offsets_host[n]) are per problem;
 * external uniforms are not offered.  The call offsets travel by value, not in the blocks: a batch whose buffers stay put
 * uploads its blocks once (icem_batch_uploads of handles[0]).  results: NULL, or [n, d + 2] of the handle dtype -- row i is
 * problem i's result.  Every output of problem i is bit for bit that of its solo step at the same seed and offset.  n == 1 is
 * the solo step (+ the results row).  ICEM_E_STATE also where the problems' rollout launches differ.
 *   Measured (EXPERIMENTS R16.1; HalfCheetah shape, change_freq 4, f32, MpcRandomHip.get_action): 0.05 ms at N = 512 and at
 * N = 4096 against 0.10 ms for the operator chain in the same process and on the parent commit's library (2.0 x: the chain's three
 * device-to-host reads and its allocations are gone; the kernels are about 5 + 9 + 5 us of it).  The step's sampler is NOT faster
 * than the operator's at these sizes -- both sit at the floor of a launch: 3.6-5.0 against 3.1 us at N = 512, 5.4-5.8 against
 * 5.5-5.6 us at N = 4096 over two traces -- and is at N = 65 536 (29.7 against 40.2 us; the step 0.09 against 0.14 ms).
 * Batched, per step of the batch against B solo steps: B = 8 0.08 / 0.18 ms at N = 512, 0.10 / 0.19 ms at N = 4096 (1.9 x to 2.3 x),
 * B = 16 2.2 x to 2.8 x. */
int     icem_plan_step_random_batch(icem_handle* const* handles, int32_t n, const icem_random_buffers* buffers,
                                    int32_t change_freq, const int64_t* call_offsets_host, void* results, void* stream);
int64_t icem_random_batch_launches(const icem_handle* h); /* kernel launches of the last such batch this handle led as handles[0]; measurement */

/* The same MPC step through the LEARNED dynamics (the declared RSSM): the chain icem_sample_piecewise (the device's own uniforms),
 * icem_rssm_rollout_cost(params: its packed parameter buffer, shared by the problems of a batch) under the handle's cost_mode,
 * icem_topk_sorted(costs, 1) and the gathers behind it, as ONE call for one planner or for n planners of one configuration.
 * icem_random_buffers is icem_plan_step_random's: b->obs0 is [ICEM_RSSM_OBS_DIM] f32.  External uniforms are not offered.  No
 * built-in model or cost need be set on the handle.  call_offset(s) are the caller's, as above: the chain, the solo entry and the
 * batched entry may alternate freely, and so may these entries and icem_plan_step_random* on one handle.
 *   3 launches whatever n (icem_random_step_launches for the solo entry, icem_random_batch_launches of handles[0] for the batched
 * one), no host synchronisation, no allocation after the first call of a batch size on a stream.  Every output of the solo entry
 * -- actions, costs, best_actions, result -- is bit for bit what the chain leaves.  A batch scores its rows back to back in a pool
 * owned by handles[0] (the batched RSSM launch wants them contiguous); its sampler writes every row into the pool AND into the
 * problem's own actions, its selection leaves every cost in the problem's own costs: EVERY buffer of EVERY problem -- actions,
 * costs, best_actions, result, its row of results ([n, d + 2] f32; may be NULL) -- is bit for bit its solo step's at the same seed
 * and offset (a controller keeps its pool; icem_plan_step_cem_learned_batch, whose pools are scratch, promises less).  The
 * problems' obs0 buffers need not be adjacent: the sampler launch gathers them into the pool's [n, 230] table.  The argument blocks
 * are those of icem_plan_step_random_batch, in the same device array of handles[0], uploaded only when a byte changed.  n == 1 is
 * the solo step plus the results row.
 *   Served: whatever icem_plan_step_random_ok asks of the handle, f32,
 * act_dim == the RSSM's action width (6, or the handle's own 1 .. 32 once icem_set_rssm_act_dim has bound it), a population the RSSM's split launch takes (for
 * a batch: all problems' tiles together; development option rssm_split = 0 switches the entries off, as random_step = 0 does), any
 * horizon that launch accepts.  ICEM_E_INVALID: a NULL handle / buffers / params, a NULL buffer, change_freq < 0 or >= horizon, a
 * negative call offset, n outside [1, 32], a handle twice, unequal configurations; ICEM_E_UNSUPPORTED: anything not served;
 * ICEM_E_STATE: the learned-dynamics rollout's own rules (icem_plan_step_cem_learned).  Whatever is refused is refused before
 * anything is launched or any handle touched.
 *   Measured (EXPERIMENTS R22.1; N = 1024, h = 12, change_freq 4, MpcRandomHip.get_action): 0.123 ms against 0.148 ms for the
 * operator chain in the same process and 0.145 ms on the parent commit's library (1.2 x: the chain's three device-to-host reads and its
 * allocations are gone; the rollout's 74 us are the same in both, the three launches together 82 us).  Batched, per step of the
 * batch against B solo steps: B = 2 0.12 / 0.19 ms, B = 4 0.19 / 0.36, B = 8 0.29 / 0.69, B = 16 0.43 / 1.34 ms (1.5 x to 3.2 x); on
 * the device B = 16 is 376 us, 23.5 us per problem, 332 us of them the batched rollout (20.8 us per problem). */
int     icem_plan_step_random_learned_ok(const icem_handle* h);   /* 1 if THIS handle is served, else 0 */
int     icem_plan_step_random_learned(icem_handle* h, const icem_random_buffers* b, const void* params, int32_t change_freq,
                                      int64_t call_offset, void* stream);
int     icem_plan_step_random_learned_batch(icem_handle* const* handles, int32_t n, const icem_random_buffers* buffers,
                                            const void* params, int32_t change_freq, const int64_t* call_offsets_host,
                                            void* results, void* stream);

/* Raw white noise of the Philox path (for RNG known-answer tests): z_r, z_i [n, d, F]. */
int icem_philox_normals(icem_handle* h, int32_t n, int64_t first_index, uint64_t offset,
                        void* z_r, void* z_i, void* stream);

/* K2  MpcController.simulate_trajectories (mpc.py:56-67) through the batched model loop
 * (abstract_models.py:17-53) + trajectory_cost_fn (abstract_controller.py:74-91) with the built-in
 * model/cost:  costs[i] = reduce_t cost(o_t, a_t),  o_{t+1} = model(o_t, a_t),  o_0 = obs0[obs_dim].
 * If observations != NULL the pre-action observations [n, h, obs_dim] are also stored. */
int icem_rollout_cost(icem_handle* h, int32_t n, const void* obs0, const void* actions, void* costs,
                      void* observations, void* stream);

/* trajectory_cost_fn's reduction alone (abstract_controller.py:82-87) for step costs [n, h]
 * produced by an external (e.g. torch) model. */
int icem_cost_reduce(icem_handle* h, int32_t n, const void* step_costs, void* costs, void* stream);

/* trajectory_cost_fn as a whole (abstract_controller.py:74-91) for rollouts produced by an external model and
 * held as tensors: costs[i] = reduce_t cost(observations[i, t, :], actions[i, t, :], next_observations[i, t, :])
 * with the cost set by icem_set_cost (+ icem_set_cost_terms) and the handle's cost_mode.  Any obs_dim.
 * observations / next_observations: element (i, t, k) at ptr[i*traj_stride + t*step_stride + k] (so [n, h, o] and
 * step-major [h, n, o] both work); next_observations may be NULL unless diff_idx >= 0.  actions [n, h, d] dense. */
int icem_trajectory_cost(icem_handle* h, int32_t n, int32_t obs_dim, const void* observations,
                         const void* next_observations, int64_t traj_stride, int64_t step_stride,
                         const void* actions, void* costs, void* stream);

/* K3  costs.argsort()[:k] (icem.py:199) and argmin (icem.py:149): the k smallest (cost, index)
 * pairs in ascending order, ties broken by index, NaN treated as +inf.
 * out_cost [k] (handle dtype), out_idx [k] int32 (k > n: entries n.. are (+inf, INT_MAX)).  workspace:
 * icem_topk_workspace_bytes(n, k). */
size_t icem_topk_workspace_bytes(const icem_handle* h, int32_t n, int32_t k);
int icem_topk_sorted(icem_handle* h, int32_t n, const void* costs, int32_t k, void* out_cost,
                     int32_t* out_idx, void* workspace, void* stream);

/* K3 + K4 in one launch for small pools (the stage-wise controller loop: learned dynamics, host models, the CEM
 * baselines): update_distributions (icem.py:194-211) with the previous elites appended behind the pool
 * (icem.py:143-145) -- the k best of [costs (n) | keep_costs (n_keep)] in (cost, index) order, index n + e = kept elite e;
 * their rows from [pool | keep_actions] into elites_out [k, h, d] (must not alias keep_actions), elite_costs_out [k],
 * idx_out [k]; mean / std refitted in place as icem_gather_refit does (same arithmetic, same bits as icem_topk_sorted
 * over the concatenation + icem_gather_refit).  f32 handles, n + n_keep <= 16384, k <= 32; otherwise
 * ICEM_E_UNSUPPORTED: use the two operators. */
int icem_update_distribution(icem_handle* h, int32_t n, const void* costs, const void* pool, int32_t n_keep,
                             const void* keep_costs, const void* keep_actions, int32_t k, void* mean, void* std,
                             void* elites_out, void* elite_costs_out, int32_t* idx_out, void* stream);
/* 1 if THIS handle serves icem_update_distribution for a pool of n_all = n + n_keep candidates and k elites (the handle's
 * dtype and the fast-path switch it latched at icem_create decide, not the caller's environment), else 0. */
int icem_update_distribution_ok(const icem_handle* h, int32_t n_all, int32_t k);

/* K4  update_distributions (icem.py:201-211): gather the k elite rows of `actions` [*, h, d] in
 * `idx` order into elites_out [k, h, d]; mean <- (1-alpha)*mean_k + alpha*mean,
 * std <- (1-alpha)*std_k(ddof=0) + alpha*std (in place).  An entry INT_MAX (padding of icem_topk_sorted) repeats row idx[0]. */
int icem_gather_refit(icem_handle* h, const void* actions, const int32_t* idx, int32_t k, void* mean,
                      void* std, void* elites_out, void* stream);

/* Epilogue of get_action (icem.py:167-175): mean[:-1] = mean[1:] (last row kept);
 * std = (high-low)/2*init_std. */
int icem_shift(icem_handle* h, void* mean, void* std, const void* low, const void* high, void* stream);

/* beginning_of_rollout (icem.py:31-59): mean = (high+low)/2, std = (high-low)/2*init_std.  The action bounds are
 * read when this is called and, on the f32 large-population path, once more per (low, high) buffer pair at the next
 * step: a caller that rewrites the bounds IN PLACE does so between episodes, in front of this call. */
int icem_reset_distribution(icem_handle* h, void* mean, void* std, const void* low, const void* high,
                            void* stream);

/* ---- fused MPC step ------------------------------------------------------------------------ */

/* Device buffers of one planner; all owned by the caller, sized by icem_plan_buffer_bytes(). */
typedef struct icem_plan_buffers {
    void* mean;        /* [h, d]              in/out: persistent across MPC steps               */
    void* std;         /* [h, d]              in/out                                            */
    void* low;         /* [d]                                                                   */
    void* high;        /* [d]                                                                   */
    void* obs0;        /* [obs_dim]           current observation                               */
    void* actions;     /* [n_local_max + r, h, d]  sampled pool of this rank (r = reused elites)*/
    void* costs;       /* [n_local_max + r]                                                     */
    void* elites;      /* 2 x [K, h, d] + 2 x [K] costs: persistent elite set (double buffered) */
    void* records;     /* [world*K + r] candidate records {cost, gidx, actions[h*d]}            */
    void* workspace;   /* scratch for the block-level top-k                                     */
    void* executed;    /* [d]   out: first action of the best trajectory (icem.py:163)          */
    void* best_cost;   /* [1]   out: min(costs) of the last iteration (icem.py:177)             */
    /* Optional external white noise for the CURRENT iteration (parity mode, NULL = Philox):
     * z_r/z_i [n_local, d, F] for the main batch; z_r_shift/z_i_shift [r, d, F] for the
     * shifted elites' last action (iteration 0 only).  noise_beta <= 0: z_r = randn [n_local, h, d] and
     * z_r_shift = randn [r, h, d] (icem.py:77), z_i / z_i_shift NULL.                           */
    const void* z_r;
    const void* z_i;
    const void* z_r_shift;
    const void* z_i_shift;
} icem_plan_buffers;

enum {
    ICEM_BUF_MEAN = 0, ICEM_BUF_STD, ICEM_BUF_LOW, ICEM_BUF_HIGH, ICEM_BUF_OBS0, ICEM_BUF_ACTIONS,
    ICEM_BUF_COSTS, ICEM_BUF_ELITES, ICEM_BUF_RECORDS, ICEM_BUF_WORKSPACE, ICEM_BUF_EXECUTED,
    ICEM_BUF_BEST_COST, ICEM_BUF_COUNT
};
/* Bytes required for buffer `which` (ICEM_BUF_*) of icem_plan_buffers. */
size_t icem_plan_buffer_bytes(const icem_handle* h, int32_t which);

/* One CEM iteration `it` (0..opt_iters-1) of MPC step number `mpc_step` (0 = first after
 * beginning_of_rollout), local part: sample this rank's shard of N_it (+ shifted / kept elites),
 * roll out, cost, block-level top-k, and pack this rank's sorted local top-K candidate records
 * into records[rank*K .. rank*K+K).  icem.py:124-147. */
int icem_plan_iter_local(icem_handle* h, const icem_plan_buffers* b, int32_t mpc_step, int32_t it,
                         void* stream);
/* After the ranks' records have been all-gathered in place (world > 1; nothing to do for world == 1):
 * merge world*K candidates (+ kept elites), take the global sorted top-K, refit mean/std, store the
 * new elite set; on the last iteration also write executed/best_cost and shift mean/std
 * (icem.py:149-175, 194-211). */
int icem_plan_iter_merge(icem_handle* h, const icem_plan_buffers* b, int32_t mpc_step, int32_t it,
                         void* stream);
/* Sharded runs (world > 1): allow icem_plan_iter_merge of a non-last iteration to postpone its work into the next
 * icem_plan_iter_local launch of the same MPC step (the merge of the gathered records then runs in that launch's
 * prologue, next to the sampling; one kernel launch less per iteration).  While on, mean / std / elites in the plan
 * buffers are current only after the LAST icem_plan_iter_merge of an MPC step.  Off by default. */
int icem_set_merge_deferral(icem_handle* h, int32_t on);

/* ---- in-library elite exchange (world > 1) ------------------------------------------------------------------
 * The all-gather of every rank's K candidate records {cost, gidx, actions[h*d]} before the replicated refit (the
 * reference's only data parallelism gathers its workers' results over pipes, icem/models/gt_par_model.py:77-94).
 * Each rank owns an exchange block in its HBM and maps the blocks of all others (HIP IPC); a rank's records reach its
 * peers as peer-to-peer stores over xGMI from ONE launch behind its local kernels, and every merge waits on flags in
 * its own block -- no host call and no collective between icem_plan_iter_local and icem_plan_iter_merge.
 *   1. icem_exchange_create on every rank: allocates the block, returns its IPC handle (ICEM_IPC_HANDLE_BYTES bytes);
 *   2. the caller moves the handles between the ranks' processes once (any channel: torch.distributed, MPI, a file);
 *   3. icem_exchange_connect with all `world` handles in rank order.  Ranks living in the CALLER'S process are passed
 *      as device pointers instead (local_blocks[r] = icem_exchange_block(peer handle); NULL entries use the IPC handle;
 *      handles_host may be NULL when every peer is local).
 * From then on icem_plan_iter_local ends with the push and icem_plan_iter_merge reads the gathered records from the
 * block (b->records then only receives this rank's own K records).  Every device-side wait is bounded (~seconds); a
 * timeout sets the block's status word, which icem_exchange_status returns and clears (0 = fine). */
#define ICEM_IPC_HANDLE_BYTES 64
int icem_exchange_create(icem_handle* h, void* ipc_handle_out_host);
int icem_exchange_connect(icem_handle* h, const void* handles_host, void* const* local_blocks);
void* icem_exchange_block(icem_handle* h);
/* Back to caller-driven exchanges (frees the block, unmaps the peers'): every rank must do the same. */
int icem_exchange_disable(icem_handle* h);
/* finegrained_host (may be NULL): 1 if the block is fine-grained device memory (what multi-GPU runs want). */
int icem_exchange_status(icem_handle* h, int32_t* status_host, int32_t* finegrained_host);
/* Measurement only (collective: every rank calls it at the same time): average latency [us] of one exchange -- this
 * rank's K records to every rank's block, then the wait for all ranks' -- over `rounds` back-to-back exchanges inside
 * one launch.  Synchronises the stream. */
int icem_exchange_probe(icem_handle* h, int32_t rounds, void* stream, double* us_out);
/* ---- the same all-gather on RCCL (world > 1) -------------------------------------------------------------------
 * SURVEY 8(b)'s icem_allgather_elites: ncclAllGather of the ranks' K records, in place in `records`
 * [world*K, 2 + h*d] (this rank's slot written by icem_plan_iter_local), enqueued on the launch stream between the
 * record pack and the merge.  It is the fallback of the exchange above -- for ranks whose peer blocks do not map or
 * whose self-test fails -- and keeps an MPC step ONE C call with zero host-side collectives (icem_plan_step_sharded).
 * Same reference analogue: the pipe gather of icem/models/gt_par_model.py:77-94.  RCCL is bound at run time (dlopen:
 * the copy already loaded in the process, else icem_rccl_load's path / $ICEM_RCCL_LIB / librccl.so.1); nothing here is
 * needed, or loaded, on one GPU.
 *   icem_rccl_unique_id   rank 0: a fresh ncclUniqueId (ICEM_RCCL_ID_BYTES bytes) for the caller to hand to every rank
 *   icem_rccl_connect     every rank, together: ncclCommInitRank(world, id, rank) -- the handle owns the communicator
 *   icem_rccl_adopt       or: use a communicator the caller already has (an ncclComm_t; size / rank must match)
 *   icem_allgather_elites the collective itself (every rank, same stream order)
 *   icem_rccl_disconnect  destroys an owned communicator / forgets an adopted one */
#define ICEM_RCCL_ID_BYTES 128
int icem_rccl_load(const char* path_or_null);
const char* icem_rccl_library(void); /* which library was bound ("" = none yet) */
int icem_rccl_unique_id(void* id_out_host);
int icem_rccl_connect(icem_handle* h, const void* id_host);
int icem_rccl_adopt(icem_handle* h, void* nccl_comm);
int icem_rccl_disconnect(icem_handle* h);
int icem_allgather_elites(icem_handle* h, void* records, void* stream);

/* Whole MPC step of one rank of a sharded run (world > 1, device noise) as ONE call, no host synchronisation and no
 * host-side collective: opt_iters x (local launch, pack, exchange, merge -- every merge but the last in the next local
 * launch's prologue).  The exchange is the in-library one when it is connected (pack + push in one launch), else
 * icem_allgather_elites when a communicator is connected; neither: ICEM_E_STATE.  world == 1: icem_plan_step. */
int icem_plan_step_sharded(icem_handle* h, const icem_plan_buffers* b, int32_t mpc_step, void* stream);

/* Whole MPC step for world == 1: opt_iters x (local + merge), no host synchronisation
 * (the body of MpcICem.get_action, icem.py:123-175). */
int icem_plan_step(icem_handle* h, const icem_plan_buffers* b, int32_t mpc_step, void* stream);

/* B independent planners of ONE configuration -- the reference's parallel episodes, each its own get_action
 * (icem/misc/rollout_utils.py:46-58, 129-152; icem.py:106-189) -- advanced by one MPC step together: every launch of the step
 * is one launch for all of them (grid.y = the problem, the argument blocks in a device array), so the step's chain of launch
 * latencies is paid once per batch instead of once per problem.  handles[i] with buffers[i]: exactly the arguments
 * icem_plan_step takes; every problem's outputs (executed action, best cost, mean, std, elites, pool, costs) are bit for bit
 * those of its own icem_plan_step.  The handles must share horizon, act_dim, populations, elites, flags, model width / kind and
 * tile arithmetic (else ICEM_E_INVALID); models, costs, seeds, bounds and observations are per problem.  Served, at world == 1,
 * f32, device noise and at most 8192 rows per iteration:
 *   - the o <= 20 tile shapes (HalfCheetah ...), whose iterations are the single-launch kernel.  (From 49 152 rows of all
 *     problems together the batch takes the noise-ahead launches of large populations -- k_rollout_ahead.hip -- instead:
 *     measured faster from there on.)
 *   - the TileHN shapes -- Door (d = 28, o = 39), Relocate (d = 30, o = 39), FetchPickAndPlace (d = 4, o = 28) at h = 30 --
 *     whose iterations are a sampler (from the second iteration on with the previous merge in its prologue: num_elites <= 11
 *     and the default generator, rng_rounds = 10) and a rollout.  The handles must also share the observation width and the
 *     compiled term program of their icem_cost_terms (a Door planner beside one without its term list: ICEM_E_INVALID).  A
 *     batch's rollout is always the one-wave-per-tile arrangement (rollout_hn_kernel's), with the waves per workgroup chosen
 *     for the tiles of all problems together: the two- and several-waves-per-tile arrangements that serve one small
 *     population alone are not batched.  At the benchmark's populations that is the arrangement that fills the chip from four
 *     problems on; for where a batch pays against stepping alone see EXPERIMENTS.md R7.4 (tools/hn_batch_bench.py).
 *   - the GEMM-kernel shapes at h = 30 -- wide observations (HumanoidStandup o = 378, Humanoid o = 376, Ant o = 113 with its term
 *     list, any 32 < o <= 384) on the 16-bit planes or the exact-f32 kernel, and the narrow shapes no tile kernel serves (Hopper,
 *     Reacher, FetchReach; a term list outside the compiled programs; ICEM_TILE_F32 on a TileHN shape) on the exact-f32 kernel --
 *     whose iterations are the same sampler pair and a GEMM rollout (rollout_wide_split_kernel, or rollout_wide_kernel with
 *     rollout_rows_wide_kernel behind it for trailing shifted elites): num_elites <= 11, rng_rounds = 10, shifted elites that fit
 *     the sampling launch (rows * act_dim <= 256).  Every problem keeps the launch shape it has alone (grid.x = its own
 *     workgroups, grid.y = the problem), so one problem's four or sixteen workgroups become 4 n or 16 n on the chip's 256 CUs.
 *     The handles must also share the observation width, the wide arithmetic IN EFFECT (icem_wide_arith: a model that
 *     ICEM_WIDE_AUTO sends to the bf16 planes beside one on the fp16 planes is refused) and all or none carry icem_cost_terms
 *     (else ICEM_E_INVALID).  Not served (ICEM_E_UNSUPPORTED): another horizon (the batched merge-prologue sampler is compiled
 *     for h = 30); a TileHN handle beside a GEMM-kernel handle.  (Every instantiation of the three rollout kernels has its
 *     batched twin: none had to be left out for its registers.)  Where a batch pays, per population and n: EXPERIMENTS.md R9.1 (tools/wide_batch_bench.py).
 * Anything else -- f64, external noise, sharded handles, num_elites > 11, other generators, populations above 8192 rows per
 * iteration (they fill the chip alone), profiling or debug stamps switched on -- is ICEM_E_UNSUPPORTED.  Whatever is refused is
 * refused before anything is launched, and every handle is left as it was.  n in [1, 32]; n == 1 is icem_plan_step.  No host
 * synchronisation; one small host-to-device copy on `stream` when the argument blocks changed (the first steps: the blocks of
 * step s are those of step s - 6).  Solo and batched steps may alternate on a handle. */
int icem_plan_step_batch(icem_handle* const* handles, int32_t n, const icem_plan_buffers* buffers, int32_t mpc_step, void* stream);
int64_t icem_batch_uploads(const icem_handle* h); /* how often handles[0]'s argument array was (re)written (measurement) */

/* The same for planners in the strict-parity arithmetic (dtype f64, the generic kernels): arguments and contract are those of
 * icem_plan_step_batch -- n in [1, 32] (n == 1 is icem_plan_step), one configuration, and also one padded model width, one model
 * kind, and either every handle with icem_cost_terms or none (else ICEM_E_INVALID: the term list decides the rollout kernel, so a
 * planner with a term list beside one without is refused); models, costs (the parametric spec and the term lists), seeds, bounds,
 * episodes and observations are per problem.  Every problem's outputs -- executed action, best cost, mean, std, both elite halves
 * and their costs, the last pool and its costs -- are bit for bit those of its own icem_plan_step: the batched kernels run the
 * solo kernels' bodies (csrc/generic_dev.h) on the argument block of problem blockIdx.y.  A step launches what a solo step
 * launches, whatever n: sampler, rollout and the one-launch selection + refit per iteration (3 * opt_iters), and in a step with
 * shifted elites their copy and their last action's sampler in front (2 more).  No host synchronisation; no allocation after
 * the first call of a batch size; one small host-to-device copy on `stream` when the argument blocks changed (the first steps;
 * icem_batch_uploads counts them for this entry too).
 *   Served: dtype f64, world == 1, device noise (colored, and white at noise_beta <= 0), rng_rounds 7 and 10, every horizon,
 * act_dim, cost mode and flag combination of the generic path, padded observation widths 8 / 16 / 17 / 18 / 24 / 32 (linear and
 * tanh), at most 8192 rows per iteration: the row-of-lanes rollout for the parametric cost, the thread-per-trajectory rollout
 * where the handles carry icem_cost_terms.
 *   ICEM_E_UNSUPPORTED, before anything is launched and with every handle left as it was: f32 handles (icem_plan_step_batch is
 * theirs), a non-NULL z_*, sharded handles, profiling or debug stamps switched on, a population above 8192 rows, an iteration
 * whose pool the one-launch selection does not admit (it would take the three-launch selection), a development option
 * gk_sample / gk_rollout_thread / gk_select away from its default, num_traj * act_dim > 262144 (the sampler's one-thread-per-row
 * form), and icem_cost_terms on a tanh model of padded width 32 (that instantiation of the thread-form rollout spills registers
 * and has no batched twin).  Where a batch pays against stepping alone: EXPERIMENTS.md R8.1 (tools/f64_batch_bench.py). */
int icem_plan_step_batch_f64(icem_handle* const* handles, int32_t n, const icem_plan_buffers* buffers, int32_t mpc_step, void* stream);
int64_t icem_batch_f64_launches(const icem_handle* h); /* kernel launches of the last f64 batch step this handle led (handles[0]); measurement */

/* The MPC step of the learned-dynamics configuration (the declared RSSM of the learned-dynamics rollout below; BASELINE
 * configs[4]) as ONE call, for one planner or for n planners at once: the loop a caller would otherwise drive operator by
 * operator.  Per CEM iteration i of MPC step s: sample population_sizes[i] rows at stream offset
 * (episode << 32) + s * (opt_iters + 1) + i (row 0 = the mean on the last iteration under use_mean_actions); at i == 0, with
 * shift_elites, s > 0 and n_reuse > 0, append the n_reuse shifted elites, their last action drawn at offset ... + opt_iters with
 * the arithmetic of the sampling operator at t_begin = h - 1; roll all rows out through the RSSM under the handle's cost_mode; select the
 * top K over [pool | kept elites] (kept for i > 0 under keep_previous_elites), gather, refit; behind the last iteration shift
 * mean and std and write executed = elites[0, 0, :] and best_cost = elite_costs[0].  Every stage is one launch for all
 * problems: 3 launches per iteration, one more in a step that shifts elites.
 *   Buffers: b->obs0 is [ICEM_RSSM_OBS_DIM] f32 and the CALLER sizes it (the buffer-size query knows no model width for a
 * handle without a built-in model); mean, std, low, high, actions, costs, elites, executed, best_cost as the fused step uses them
 * (actions / costs are scratch; a batch scores its rows in a pool of handles[0]'s instead).  records, workspace: unused.
 * A non-NULL z_*: ICEM_E_UNSUPPORTED.  Elite halves: iteration i of step s writes half (s * opt_iters + i + 1) & 1 of
 * `elites` and reads the other one, so the current set behind step s is half ((s + 1) * opt_iters) & 1.
 *   params: the packed parameter buffer of the learned-dynamics rollout, shared by all problems.  mpc_step is the caller's
 * count since the last reset -- per problem in a batch (mpc_steps_host[n], host memory): a planner reset later than its peers
 * has no shifted elites and fewer rows.  results (device, may be NULL): [n, act_dim + 1] f32, row p = problem p's executed
 * action | best cost.
 *   Served: f32, world == 1, act_dim == the RSSM's action width (6, or the handle's own 1 .. 32 once icem_set_rssm_act_dim has bound it),
 * horizon * act_dim <= 512, the handle's fast path on, profiling off, rng_rounds 10, a horizon of the folded
 * sampler (30, 12, 13, 10), at most 16 384 candidates and 32 elites per update, and all problems' 16-row tiles together within
 * the split launch's limit; development option learned_step = 0 switches the entries off.  Anything else is
 * ICEM_E_UNSUPPORTED; mismatched configurations (everything but the seed must agree), the same handle twice, n outside
 * [1, 32] or a NULL argument ICEM_E_INVALID.  Whatever is refused is refused before anything is launched.  The staging,
 * first-call-not-under-capture and ICEM_E_STATE rules of the learned-dynamics rollout apply; its host-visible status word is
 * looked at BEFORE the step's first launch, so a step refused with ICEM_E_STATE has launched nothing.  No host
 * synchronisation; no allocation after the first call of a batch size on a stream; one small host-to-device copy when the
 * argument blocks changed (the first steps).  Each problem's outputs in a batch are bit for bit those of its own solo step;
 * n == 1 is the solo entry. */
#define ICEM_RSSM_OBS_DIM 230
int icem_plan_step_learned_ok(const icem_handle* h);   /* 1 if THIS handle is served, else 0 */
int icem_plan_step_learned(icem_handle* h, const icem_plan_buffers* b, const void* params, int32_t mpc_step, void* stream);
int icem_plan_step_learned_batch(icem_handle* const* handles, int32_t n, const icem_plan_buffers* buffers, const void* params,
                                 const int32_t* mpc_steps_host, void* results, void* stream);
int64_t icem_learned_step_launches(const icem_handle* h); /* kernel launches of the last learned step this handle led (handles[0]); measurement */
/* icem_plan_step_learned_batch for problems that roll out through MODELS OF THEIR OWN: an ensemble whose members score every
 * plan together (the model loop of icem/models/abstract_models.py:17-53), parallel episodes that each own a trained model
 * (icem/misc/rollout_utils.py:46-58, 129-152), or both.  params_host [n * members] (host array of device pointers, problem-major,
 * read before the call returns): problem p's members are params_host[p * members .. (p + 1) * members), each a packed buffer
 * as icem_rssm_rollout_cost_models takes it.  A shared ensemble repeats the same `members` pointers for every problem; a model
 * each is members == 1 with n pointers; an ensemble each names n * members buffers.  A plan's cost is the members'
 * icem_rssm_ensemble_reduce (`reduce`: ICEM_RSSM_REDUCE_MEAN or _MAX; a NaN member makes the row NaN).
 *   Semantics: icem_plan_step_learned_batch's -- noise offsets, elite halves, the shifted rows of a problem reset later than
 * its peers, the epilogue, `results`, the buffers (n == 1 works in the problem's own actions / costs, a batch in a pool of
 * handles[0]'s), option learned_step -- with two differences.  The rollout of an iteration is ONE launch of n * members problems
 * in member-major order (problem e * n + p reads problem p's action rows and observation), so the members' costs land as
 * [members, the iteration's rows of all problems]: the layout icem_rssm_rollout_cost_models gives such a launch.  And the
 * update reduces them itself: problem p's candidate i costs the reduction over e of member_costs[e * stride + row0 + i]
 * (stride: the iteration's rows of all problems, row0: p's first), in icem_rssm_ensemble_reduce's arithmetic operation for
 * operation, and the reduced cost is written where the single-model step leaves its costs.  So still 3 launches per
 * iteration, + 1 in a step that shifts elites, whatever n and members.  Every buffer of every problem is bit for bit what the
 * stage-wise operators (sample, icem_rssm_rollout_cost_ensemble / _models, update, shift) give; members == 1 with equal pointers
 * gives icem_plan_step_learned_batch's bits, with n == 1 icem_plan_step_learned's.
 *   member_costs (device f32, may be NULL): at least members * n * (the largest iteration's rows of one problem) floats; after the
 * call it holds the LAST iteration's [members, rows of all problems].  NULL: scratch of handles[0] (no allocation after the
 * first call of a size).  Its address sits in the step's argument blocks: keep one buffer and the steady state uploads nothing.
 *   ICEM_E_INVALID: a NULL argument or a NULL entry of params_host, n or members outside [1, 32], a bad reduce, the same handle
 * twice, unequal configurations or RSSM widths.  ICEM_E_UNSUPPORTED: n * members > 32 (the launch's table travels in the
 * kernel arguments); the tiles of an iteration (members x the sum over the problems of ceil(rows / 16)) beyond the split
 * launch's limit; whatever icem_plan_step_learned_batch does not serve; a non-NULL z_*.  All of it before anything is launched
 * or any handle touched; the learned-dynamics rollout's status word is looked at before the first launch (ICEM_E_STATE: nothing
 * was launched).  icem_plan_step_learned_models_ok: would n handles like this one be served with `members` models each (every
 * problem counted with its shifted elites)?  icem_learned_step_launches counts this entry's launches too. */
int icem_plan_step_learned_models_ok(const icem_handle* h, int32_t n, int32_t members);
int icem_plan_step_learned_models(icem_handle* const* handles, int32_t n, const icem_plan_buffers* buffers, int32_t members,
                                  const void* const* params_host, int32_t reduce, const int32_t* mpc_steps_host, void* member_costs,
                                  void* results, void* stream);

/* The two baselines' MPC steps through MODELS OF THEIR OWN -- the planners the ensemble literature uses (PETS: CEM or random
 * shooting through a probabilistic ensemble; PlaNet's planner is this CEM): icem_plan_step_cem_learned_batch and
 * icem_plan_step_random_learned_batch with params_host, members, reduce and member_costs as icem_plan_step_learned_models takes
 * them (a shared ensemble, a model each with members == 1, an ensemble each; member_costs NULL or at least members * n * num_traj
 * floats, afterwards the LAST rollout's [members, rows of all problems]).
 *   Semantics: those of the *_learned_batch entry -- stream offsets, call_offsets, the results rows ([n, d + 1] / [n, d + 2]), the
 * argument array of handles[0] uploaded only when a byte changed, free alternation with the other entries on one handle -- with
 * two differences.  The rollout is ONE launch of n * members problems in member-major order (icem_plan_step_learned_models'
 * arrangement: member e's cost of problem p's row i at member_costs[e * n * num_traj + p * num_traj + i]).  And the launch behind
 * it reduces the members' costs itself, in icem_rssm_ensemble_reduce's arithmetic operation for operation (a NaN member makes the
 * row NaN), and writes the reduced cost where the single-model step leaves its costs: the CEM step's update
 * (cem_update_members_batch_kernel) while it builds its keys, the random-shooting step's selection
 * (random_select_members_batch_kernel) while it looks for the smallest (cost, index) pair with NaN counted as +inf.  So 3 launches
 * per CEM iteration (icem_cem_batch_launches of handles[0]) and 3 launches per random-shooting step (icem_random_batch_launches of
 * handles[0]) whatever n and members, no host synchronisation, no allocation after the first call of a size on a stream.
 * n == 1 works in the problem's own actions / costs, n > 1 in the pool of handles[0].
 *   CEM: every problem's mean, std, lower, upper, elites, elite_costs, elite_idx, executed, best_cost and its results row are bit
 * for bit the operator loop's (icem_sample_truncnorm, icem_rssm_rollout_cost_ensemble / _models, icem_update_distribution,
 * icem_cem_bounds); for n == 1 the last pool in actions / costs too, for n > 1 a problem's own pool is scratch.  Random shooting:
 * EVERY buffer of every problem (actions, costs, best_actions, result, its results row) is bit for bit the chain's
 * (icem_sample_piecewise, icem_rssm_rollout_cost_ensemble / _models, icem_topk_sorted(costs, 1), the gathers).  Both: members == 1
 * with equal pointers gives the *_learned_batch entry's bits, with n == 1 the solo entry's.
 *   ICEM_E_INVALID: a NULL argument or a NULL entry of params_host, n or members outside [1, 32], a bad reduce, a handle twice,
 * unequal configurations or RSSM widths, and what the *_learned entries call invalid (a negative step or offset, change_freq < 0
 * or >= horizon, a NULL buffer).  ICEM_E_UNSUPPORTED: n * members > 32; the tiles of a rollout (members x the sum over the
 * problems of ceil(num_traj / 16)) beyond the split launch's limit; whatever icem_plan_step_cem_learned_ok /
 * icem_plan_step_random_learned_ok does not serve (options cem_step / random_step / rssm_split = 0 among it).  ICEM_E_STATE: the
 * learned-dynamics rollout's staging and status-word rules, looked at before the first launch.  All of it before anything is
 * launched or any handle touched.  *_models_ok: would n handles like this one be served with `members` models each? */
int icem_plan_step_cem_learned_models_ok(const icem_handle* h, int32_t n, int32_t members);
int icem_plan_step_cem_learned_models(icem_handle* const* handles, int32_t n, const icem_cem_buffers* buffers, const icem_cem_params* p,
                                      int32_t members, const void* const* params_host, int32_t reduce, const int32_t* mpc_steps_host,
                                      void* member_costs, void* results, void* stream);
int icem_plan_step_random_learned_models_ok(const icem_handle* h, int32_t n, int32_t members);
int icem_plan_step_random_learned_models(icem_handle* const* handles, int32_t n, const icem_random_buffers* buffers, int32_t members,
                                         const void* const* params_host, int32_t reduce, int32_t change_freq,
                                         const int64_t* call_offsets_host, void* member_costs, void* results, void* stream);

/* Wide observations (32 < obs_dim <= 384; HumanoidStandup's o = 378, environments/mujoco.py:241-277): which matrix-pipe
 * arithmetic the rollout's model step (the GEMM of abstract_models.py:31-53's predict at this width) runs in.  The modes
 * are NAMES, not an accuracy order:
 *   ICEM_WIDE_F32 (1): v_mfma_f32_16x16x4_f32 -- bitwise an f32 fmaf chain, a quarter of the speed.  What strict-parity
 *     callers pass; the only arithmetic at widths the split kernel's LDS does not hold (o + d > 416).
 *   ICEM_WIDE_F16X2 (0): every f32 operand x 2^k (k per trajectory row / per model, so that nothing exceeds 2^15) as the
 *     sum of two fp16 numbers, three fp16 products per multiply-add with f32 accumulation on v_mfma_f32_16x16x32_f16 --
 *     f32-class rounding (operands to 2^-24 relative, the dropped lo x lo product below 2^-24 of a product), NOT the bits
 *     of an f32 fmaf chain; a tanh model's state is bounded by the equilibrated scales instead of scanned.  The model is
 *     carried equilibrated -- rows and columns scaled by powers of two -- so observations in mixed units keep their
 *     accuracy; contributions more than 2^13 apart inside the balanced model keep an absolute, not a relative, accuracy:
 *     2^-40 of a row's largest.
 *   ICEM_WIDE_BF16X3 (2): three bf16 numbers and six products (operands exact whatever their magnitudes, dropped products
 *     below 2^-31), two thirds of F16X2's speed.
 *   ICEM_WIDE_AUTO (-1, THE DEFAULT since ABI 4; ABI 3 defaulted to F16X2 unconditionally, ABI 2 to F32): F16X2 where one
 *     sweep of balancing leaves every row and column of the model with its largest weight within 2^13 of the model's
 *     largest AND its median nonzero weight within 2^13 of its own largest (icem_wide_imbalance_log2 <= 13: the larger of
 *     the two measures over all lines), BF16X3 otherwise -- decided per model at icem_set_model.  A caller that needs the
 *     fmaf chain's bits (golden vectors recorded at this width in f32) must ask for ICEM_WIDE_F32; the parity bar of
 *     north_star (1e-5 relative, identical elite sets) holds in all three (tests/test_gpu_parity_sizes.py).
 * icem_wide_arith: the arithmetic in effect for the handle's current model (never AUTO).  Takes effect at the next
 * rollout; no effect at obs_dim <= 32 (narrow models on the GEMM kernel always compute in exact f32: icem_wide_arith = 1).
 * Other values: ICEM_E_INVALID.  icem_set_wide_exact(h, on) is the ABI <= 3 spelling of icem_set_wide_arith(h, on), on in {0, 1, 2}. */
enum { ICEM_WIDE_AUTO = -1, ICEM_WIDE_F16X2 = 0, ICEM_WIDE_F32 = 1, ICEM_WIDE_BF16X3 = 2 };
int icem_set_wide_arith(icem_handle* h, int32_t mode);
int icem_wide_arith(const icem_handle* h);
int icem_wide_imbalance_log2(const icem_handle* h); /* of the balanced model: max over rows / columns of log2(model max / line max) and log2(line max / line median) */
/* the same measure for any model (host arrays as icem_set_model takes them; no handle, no device): -1 on bad arguments */
int icem_wide_model_imbalance_log2(int32_t obs_dim, int32_t act_dim, const double* A_host, const double* B_host);
int icem_set_wide_exact(icem_handle* h, int32_t on);

/* Narrow observations (the 16-trajectory tile kernels, 16 <= padded obs_dim <= 20: HalfCheetah's o = 17 / 18): which
 * arithmetic the model step (abstract_models.py:17-26's predict) runs in.
 *   ICEM_TILE_F32 (0): v_mfma_f32_16x16x4_f32 -- bitwise an f32 fmaf chain; the single-launch kernel of small populations
 *     runs the same chain on the VALU, so every launch shape gives the same bits.
 *   ICEM_TILE_F16X2 (1): every f32 operand x S (S one power of two per launch, from max(|obs0|, action bound)) as the sum
 *     of two fp16 numbers, three fp16 products per multiply-add with f32 accumulation on v_mfma_f32_16x16x32_f16 -- f32-class
 *     rounding (operands to 2^-24 relative down to 2^-7 of the largest, 2^-29 of the largest below), a quarter of the
 *     matrix-pipe time of the exact form; NOT the bits of an fmaf chain.  fp16 ends at 65 504 = 2^11 x the scaled magnitude,
 *     so the planes are SERVED ONLY WHERE NO STATE CAN GET THERE: for a linear model the reachable maximum of
 *     |state entry| / max(|obs0|, action bound) over the horizon -- over every start observation and every action sequence
 *     inside the bounds; icem_tile_growth returns it -- must not exceed 2^10 (a tanh model's state is bounded by 1), and the
 *     largest |entry| of B must not exceed 2^10 x A's (the action operand's scale).  Every other model keeps the
 *     exact form whatever is asked -- with A = 1.5 I over 30 steps the reference ranks finite costs of 1e5 (icem.py:147-159,
 *     199) and so does this library -- and icem_tile_arith tells which arithmetic a handle's launches use.
 *   ICEM_TILE_AUTO (-1, the default): F16X2 wherever it is served (the widths, models and thresholds above), at every
 *     population -- since ABI 4; ABI 3 kept configurations with an iteration of at most 8192 rows on F32, which measured
 *     SLOWER there too (N = 4096 x 5 iterations: 66.7 -> 61.9 us per MPC step).  Decided from the configuration alone -- the
 *     handle's, never the process environment's: every rank of a sharded run and every iteration of a decaying population
 *     computes in the same arithmetic.  Strict-parity callers pass ICEM_TILE_F32.
 * The same setting governs the Door / Relocate / FetchPickAndPlace shapes' TileHN rollout (o = 28 / 39; k_rollout_hn.hip --
 * fp16 planes by default under the same range rules; ICEM_TILE_F32, and at o = 39 also icem_set_wide_arith(ICEM_WIDE_F32),
 * puts them on the exact-f32 GEMM kernel).
 * Takes effect at the next launch (not between icem_plan_iter_local and its merge).  No reference counterpart.
 * The scale S takes the action bound from the (low, high) buffers of the plan calls and of icem_reset_distribution (fetched
 * once per buffer pair and again at every reset -- the first such call on a stream must not be inside a stream capture);
 * icem_rollout_cost on actions OUTSIDE those bounds can still leave the planes' range: see icem_nonfinite_costs. */
enum { ICEM_TILE_AUTO = -1, ICEM_TILE_F32 = 0, ICEM_TILE_F16X2 = 1 };
int icem_set_tile_arith(icem_handle* h, int32_t mode);
int icem_tile_arith(const icem_handle* h); /* the arithmetic in effect: ICEM_TILE_F32 or ICEM_TILE_F16X2 */
double icem_tile_growth(const icem_handle* h); /* reachable max of |state| / max(|obs0|, action bound) over the horizon (1: tanh) */

/* Float64 handles (dtype ICEM_F64, the reference's own arithmetic): which arithmetic the model step of the rollout
 * (abstract_models.py:17-26's predict) runs in.
 *   ICEM_F64_CHAIN (0, the default): one fma chain per output (k = 0 .. o - 1, then the actions) on the vector ALU, the
 *     generic kernels; observation widths up to 32.
 *   ICEM_F64_MFMA (1): v_mfma_f64_16x16x4_f64 -- sixteen trajectories per workgroup, the contraction over [state | actions]
 *     summed in blocks of four on the f64 matrix cores: float64 rounding in another summation order, NOT the chain's bits
 *     (the float64 oracle's bar, 1e-10 relative, holds with a factor 100 in hand at every shipped cost).  Under it
 *     icem_set_model accepts 1 <= obs_dim <= 384 with either model kind, the num_elites <= 32 limit of the f32 wide
 *     kernels does not apply (selection runs on the cost array), external noise (z_r / z_i) works at every width and
 *     icem_rollout_cost returns `observations` at every width.  One kernel serves the stand-alone operator, icem_plan_step,
 *     icem_plan_iter_local (sharded or not) and icem_get_action; it has no batched twin: icem_plan_step_batch_f64 refuses
 *     such handles with ICEM_E_UNSUPPORTED, nothing launched.  The development option gk_rollout_thread does not apply.
 * Other values: ICEM_E_INVALID.  An f32 handle: ICEM_E_UNSUPPORTED.  Back to ICEM_F64_CHAIN while the handle's model is
 * wider than 32: ICEM_E_UNSUPPORTED.  A refused call leaves the handle as it was.  Takes effect at the next launch (not
 * between icem_plan_iter_local and its merge).  icem_f64_arith: the arithmetic in effect (ICEM_F64_CHAIN on an f32
 * handle).  No reference counterpart. */
enum { ICEM_F64_CHAIN = 0, ICEM_F64_MFMA = 1 };
int icem_set_f64_arith(icem_handle* h, int32_t mode);
int icem_f64_arith(const icem_handle* h);

/* Status word of the tile rollouts (every launch of the o <= 48 kernels counts into it): the number of trajectories since
 * icem_create whose cost came out NaN -- a state that left the arithmetic's range (f32's; the fp16 planes' for actions
 * outside the bounds their scale was taken from) or non-finite inputs.  Such a trajectory ranks last, as a NaN does under
 * icem.py:199's argsort; the reference's float64 would have ranked a finite cost, so a caller that fed finite inputs must
 * not trust the step: icem_get_action returns ICEM_E_RANGE (outputs filled) when its own step raised the count from a finite
 * observation; icem_plan_step callers read it here.  Copies one word back and synchronises `stream`. */
int icem_nonfinite_costs(icem_handle* h, int64_t* count_out, void* stream);

/* Development options: which of several BIT-IDENTICAL launch arrangements serves a call, tuning fractions, the bound of the
 * exchange's device-side waits (names and defaults: icem_amd/csrc/options.h; icem_option_name(i) enumerates them, NULL
 * behind the last).  One process-wide table; the library reads NO environment variable -- tools map ICEM_<NAME> variables
 * onto it explicitly (icem_amd._lib.apply_env_options).  No option selects an arithmetic. */
int icem_set_option(const char* name, double value);
int icem_get_option(const char* name, double* value_out);
int icem_reset_options(void);
const char* icem_option_name(int32_t index);

/* ---- per-kernel timing (measurement only) ------------------------------------------------- */
enum {
    ICEM_K_SAMPLE = 0, ICEM_K_ROLLOUT, ICEM_K_TOPK_PARTIAL, ICEM_K_LOCAL_PACK, ICEM_K_MERGE_REFIT,
    ICEM_K_SAMPLE_ROLLOUT, ICEM_K_COUNT
};
/* While enabled, every kernel launch of this handle is bracketed by hipEventRecord on the
 * caller's stream.  icem_profile_read synchronises those events, returns per kernel class the
 * summed duration [ms], the number of launches and the units processed (traj-steps for
 * SAMPLE/ROLLOUT/SAMPLE_ROLLOUT, keys for the top-k kernels), and clears the log. */
int icem_profile_enable(icem_handle* h, int32_t on);
/* Development aid: [grid, 8] int64 device buffer a kernel under study may fill with per-workgroup phase
 * cycle stamps (NULL disables; no production kernel writes it).  h = NULL addresses the stateless
 * icem_rssm_rollout_cost instead: 16 int64 of wall_clock64 stamps of tile 0 (icem_rssm_split.hip). */
int icem_debug_stamps(icem_handle* h, void* dev_ptr);
int icem_profile_read(icem_handle* h, double* total_ms, int64_t* launches, int64_t* units);
/* What an event pair adds to the kernel it brackets (measurement only; stateless).  Times `reps` event pairs on `stream`
 * around a one-wave kernel that spins for spin_us of the 100 MHz wall clock and reports how long it really ran:
 * *pair_us = median event-pair time, *kernel_us = median in-kernel duration.  pair_us - kernel_us is the part of every
 * icem_profile_read span that is the bracket (dispatch in front, the closing event behind), not the kernel; bench.py
 * subtracts it so that the per-kernel times sum to the step they were taken from. */
int icem_profile_overhead(void* stream, int32_t reps, double spin_us, double* pair_us, double* kernel_us);

/* Byte size / layout of one candidate record: {cost (T), gidx (int32, padded to sizeof(T)),
 * actions[h*d] (T)}; all-gather moves K records per rank. */
size_t icem_record_bytes(const icem_handle* h);

/* Learned-dynamics rollout (BASELINE configs[4]; the reference has no model code for it, README.md:21-29): the
 * recurrent state-space model declared in icem_amd/models.py::declared_rssm, rolled out on its prior mean from
 * obs0 = [h (200) | z (30)] (f32) along actions [n, horizon, 6] (f32; any other width 1 .. 32: icem_rssm_rollout_cost_w below) in ONE launch on the bf16 matrix cores
 * (f32 accumulation, f32 recurrent state); costs[i] (f32) = reduce_t -reward(state_t) with cost_mode = ICEM_COST_*.
 * params: the packed bf16 parameter buffer of icem_rssm_param_elems() elements (layout: icem_amd/csrc/icem_rssm.h;
 * packer: icem_amd.models.pack_rssm).  No handle.  Populations of up to 65 536 rows take a launch in which the
 * recurrence and the reward head are separate workgroups exchanging the states through a staging area in device
 * memory (8 KB per 16 trajectories and step: 25 MB up to 4096 rows at h = 12, grown on demand to 403 MB at 65 536); the
 * library keeps one such area per (device, stream), allocated at the
 * first call on that stream -- which therefore must not be inside a stream capture (later ones may be: the launch
 * leaves its flags as it found them).  A reward workgroup whose bounded wait for its recurrence times out reports NaN
 * costs and raises a host-visible word: every later launch on that stream reports NaN too until the NEXT call of this
 * function, which resets the flags, launches nothing and returns ICEM_E_STATE once.  icem_rssm_trim() frees the staging
 * areas (no launch of this path may be in flight). */
size_t icem_rssm_param_elems(void);
int icem_rssm_trim(void);
int icem_rssm_rollout_cost(int32_t n, int32_t horizon, int32_t cost_mode, const void* params, const void* obs0,
                           const void* actions, void* costs, void* stream);
/* B planners' populations through the declared RSSM in ONE launch (the reference's parallel episodes, each with its own
 * start state: icem/misc/rollout_utils.py:46-58, 129-152).  rows_host[p] >= 1 trajectories of problem p, back to back in
 * actions [sum rows, horizon, 6] (another width: icem_rssm_rollout_cost_batch_w) / costs [sum rows]; obs0 [n_problems, 230] (f32, device); one params buffer for all.
 * costs of problem p: bit for bit icem_rssm_rollout_cost(rows_host[p], ..., obs0 + 230 p, its actions).
 * n_problems in [1, 32].  Served by the split launch only: the sum over p of ceil(rows/16) tiles beyond its limit, or the
 * split launch switched off: ICEM_E_UNSUPPORTED, nothing launched.  Staging / capture / ICEM_E_STATE rules of
 * icem_rssm_rollout_cost. */
int icem_rssm_rollout_cost_batch(int32_t n_problems, const int32_t* rows_host, int32_t horizon, int32_t cost_mode,
                                 const void* params, const void* obs0, const void* actions, void* costs, void* stream);
/* The two entries above at any action width act_dim in [1, ICEM_RSSM_MAX_ACT_DIM] (the other sizes stay 200 / 30 / 200):
 * actions is [n, horizon, act_dim] resp. [sum rows, horizon, act_dim], params a buffer packed from a model of THAT width --
 * the same icem_rssm_param_elems() elements, the action columns of the input layer at 32 .. 32 + act_dim of its [z | a]
 * contraction, zeros behind them (pack_rssm).  Only the act_dim entries a row owns per step are ever read.  act_dim outside
 * the range: ICEM_E_UNSUPPORTED, nothing launched.  The entries above are these at act_dim = 6, bit for bit. */
#define ICEM_RSSM_MAX_ACT_DIM 32
int icem_rssm_rollout_cost_w(int32_t n, int32_t horizon, int32_t act_dim, int32_t cost_mode, const void* params, const void* obs0,
                             const void* actions, void* costs, void* stream);
int icem_rssm_rollout_cost_batch_w(int32_t n_problems, const int32_t* rows_host, int32_t horizon, int32_t act_dim, int32_t cost_mode,
                                   const void* params, const void* obs0, const void* actions, void* costs, void* stream);
/* Binds a handle to an RSSM of action width act_dim for the learned-dynamics steps (icem_plan_step_learned*,
 * icem_plan_step_cem_learned*, icem_plan_step_random_learned* and their *_ok): the width of the model whose packed `params` the
 * caller will pass.  act_dim must equal the handle's cfg.act_dim (ICEM_E_INVALID) and lie in [1, ICEM_RSSM_MAX_ACT_DIM]
 * (ICEM_E_UNSUPPORTED); a refused call leaves the handle as it was.  A handle never bound is served at the declared width 6
 * only -- the library cannot see the width of a `params` buffer, so it is never guessed from cfg.act_dim.  A batch shares one
 * model: handles of one batch that are bound to different widths are an unequal configuration (ICEM_E_INVALID).
 * icem_rssm_act_dim: the bound width (6 for a handle never bound, 0 for a null handle). */
int icem_set_rssm_act_dim(icem_handle* h, int32_t act_dim);
int32_t icem_rssm_act_dim(const icem_handle* h);

/* Problems with a MODEL EACH in one launch of the learned-dynamics rollout: the reference's parallel episodes
 * (icem/misc/rollout_utils.py:46-58, 129-152) when every episode owns its trained model, and the members of a model
 * ensemble, which the reference's model loop (icem/models/abstract_models.py:17-53) would visit one after the other.
 * Problem p rolls the rows action_row0 .. action_row0 + rows of actions [n_action_rows, horizon, act_dim] (f32, device; the
 * rows of different problems may overlap or coincide, and are only read) out from row obs_row of obs0 [n_obs, 230] (f32,
 * device) through its own packed parameter buffer (device; icem_rssm_param_elems() 16-bit words packed at width act_dim).
 * costs [sum rows] (f32): problem p's rows back to back in problem order, each bit for bit what icem_rssm_rollout_cost_w
 * gives for that problem alone with its params.  n_problems in [1, 32]; problems_host is read before the call returns.
 *   ICEM_E_INVALID: a NULL pointer or a NULL params entry, n_problems outside [1, 32], rows < 1, action_row0 < 0 or
 * action_row0 + rows > n_action_rows, obs_row outside [0, n_obs), horizon < 1, a bad cost_mode.  ICEM_E_UNSUPPORTED:
 * act_dim outside [1, ICEM_RSSM_MAX_ACT_DIM]; all problems' tiles together (the sum of ceil(rows / 16)) beyond the split
 * launch's limit, or the split launch switched off.  Whatever is refused is refused before anything is launched.  Staging /
 * capture / ICEM_E_STATE rules of icem_rssm_rollout_cost (the first call of a size not inside a stream capture). */
typedef struct icem_rssm_problem {
    const void* params;   /* this problem's packed RSSM (icem_rssm_param_elems() 16-bit words) */
    int64_t action_row0;  /* its first row of `actions`; problems may overlap or coincide */
    int32_t rows;         /* >= 1 */
    int32_t obs_row;      /* its start state: row of obs0 [n_obs, 230] */
} icem_rssm_problem;
int icem_rssm_rollout_cost_models(int32_t n_problems, const icem_rssm_problem* problems_host, int32_t horizon, int32_t act_dim,
                                  int32_t cost_mode, const void* obs0, int32_t n_obs, const void* actions, int64_t n_action_rows,
                                  void* costs, void* stream);
/* costs [n] (f32, device) out of member_costs [members, n] (f32, device), the members visited in the order 0 .. members - 1
 * (the model loop of icem/models/abstract_models.py:17-53, reduced): ICEM_RSSM_REDUCE_MEAN is ((c_0 + c_1) + ...) * inv with
 * inv = (float)(1.0 / members) computed on the host -- no division on the device, no atomics: float32 arithmetic restates
 * it bit for bit; ICEM_RSSM_REDUCE_MAX is the worst member, and a NaN member makes the row NaN under both.  members in
 * [1, 32], n >= 1, otherwise (or a NULL pointer, a bad reduce) ICEM_E_INVALID. */
enum { ICEM_RSSM_REDUCE_MEAN = 0, ICEM_RSSM_REDUCE_MAX = 1 };
int icem_rssm_ensemble_reduce(int32_t members, int64_t n, int32_t reduce, const void* member_costs, void* costs, void* stream);
/* An ensemble of `members` models (params_host [members]: host array of device pointers, read before the call returns)
 * scores the SAME n rows of actions [n, horizon, act_dim] from one observation obs0 [230]: ONE split launch of
 * members problems that share the action rows, then the reduction.  member_costs [members, n] is an OUTPUT (row e: member
 * e alone, bit for bit icem_rssm_rollout_cost_w with its params), costs [n] their icem_rssm_ensemble_reduce.  members == 1
 * gives the solo launch's bits in both.  Refusals as above (members outside [1, 32], n < 1: ICEM_E_INVALID; members x
 * ceil(n / 16) tiles beyond the limit: ICEM_E_UNSUPPORTED), before anything is launched. */
int icem_rssm_rollout_cost_ensemble(int32_t members, const void* const* params_host, int32_t n, int32_t horizon, int32_t act_dim,
                                    int32_t cost_mode, int32_t reduce, const void* obs0, const void* actions, void* member_costs,
                                    void* costs, void* stream);

/* Feed-forward learned dynamics (PETS / MBPO style; no reference counterpart: the reference's cost_fns presuppose such a
 * model, it ships none): an observation-space MLP that predicts the next observation as a residual,
 *   x1 = act(W1 [s | a] + b1), xk = act(Wk x(k-1) + bk) for k = 2 .. layers, s' = s + Wout x_layers + bout,
 * hidden width 200, act = relu (ICEM_MLP_RELU) or swish x sigmoid(x) (ICEM_MLP_SWISH), obs_dim in [1, 64], act_dim in [1, 32],
 * layers in [1, 4].  params: the packed bf16 parameter buffer (device) of icem_mlp_param_elems(obs_dim, act_dim, layers) 16-bit
 * words (layout: icem_amd/csrc/icem_mlp.h; packer: icem_amd.models.pack_mlp); the function returns 0 for a shape outside the
 * ranges. */
#define ICEM_MLP_MAX_OBS_DIM 64
#define ICEM_MLP_MAX_ACT_DIM 32
#define ICEM_MLP_MAX_LAYERS 4
enum { ICEM_MLP_RELU = 0, ICEM_MLP_SWISH = 1 };
size_t icem_mlp_param_elems(int32_t obs_dim, int32_t act_dim, int32_t layers);
/* costs [n] (f32, device) of actions [n, horizon, act_dim] (f32, device) rolled out through that model from obs0 [obs_dim]
 * (f32, device) in ONE launch on the bf16 matrix cores, scored by the parametric cost:
 *   costs[i] = reduce_t c(s_t, a_t, s_{t+1}),  s_{t+1} = s_t + f(s_t, a_t),  s_0 = obs0,
 * c = icem_set_cost's form (*cost) plus icem_set_cost_terms' list (*terms; NULL: none), reduced by cost_mode as
 * icem_rollout_cost does -- its semantics with the MLP in the model's place.  Weights, the state and the hidden activations
 * enter the matrix products rounded to bf16; the state itself, the residual add and the cost are f32.  observations: NULL, or
 * [n, horizon + 1, obs_dim] (f32, device) for s_0 .. s_h; the costs do not depend on it bit for bit.  No handle, no state,
 * nothing allocated: the call may be captured into a graph from the first one on.
 *   ICEM_E_INVALID: a NULL cost / params / obs0 / actions / costs, n < 0, a cost_mode or activation outside its enum, a term
 * list icem_set_cost_terms refuses, a cost or term index outside obs_dim.  ICEM_E_UNSUPPORTED: obs_dim, act_dim or layers
 * outside the ranges above, horizon outside [1, ICEM_MAX_HORIZON].  Whatever is refused is refused before anything is
 * launched.  n == 0: ICEM_OK, nothing launched. */
int icem_mlp_rollout_cost(int32_t n, int32_t horizon, int32_t obs_dim, int32_t act_dim, int32_t layers, int32_t activation,
                          int32_t cost_mode, const icem_cost_spec* cost, const icem_cost_terms* terms, const void* params,
                          const void* obs0, const void* actions, void* costs, void* observations, void* stream);
/* Problems with an MLP EACH in one launch of that rollout (icem_rssm_rollout_cost_models' layout with the MLP in the model's
 * place): parallel episodes that each own a trained model, and the members of a PETS-style ensemble.  Problem p rolls the rows
 * action_row0 .. action_row0 + rows of actions [n_action_rows, horizon, act_dim] (f32, device; the rows of different problems may
 * overlap or coincide, and are only read) out from row obs_row of obs0 [n_obs, obs_dim] (f32, device) through its own packed
 * parameter buffer (device; icem_mlp_param_elems() 16-bit words; the same buffer may serve several problems).  obs_dim, act_dim,
 * layers, activation, horizon, cost_mode and the cost pair are the launch's, shared by all problems.  costs [sum rows] (f32):
 * problem p's rows back to back in problem order (not rounded to tiles), observations (NULL, or [sum rows, horizon + 1, obs_dim])
 * alike; every cost and every state bit for bit what icem_mlp_rollout_cost gives for that problem alone with its params.
 * n_problems in [1, ICEM_MLP_MAX_PROBLEMS]; problems_host is read before the call returns (the problem table travels in the
 * kernel arguments).  Nothing is allocated: the call may be captured into a graph from the first one on.
 *   ICEM_E_INVALID: a NULL pointer or a NULL params entry, n_problems outside [1, 32], rows < 1, action_row0 < 0 or
 * action_row0 + rows > n_action_rows, obs_row outside [0, n_obs), and what icem_mlp_rollout_cost calls invalid about
 * cost_mode, the activation and the cost pair.  ICEM_E_UNSUPPORTED: its shape and horizon ranges (and 2^31 tiles or more).
 * Whatever is refused is refused before anything is launched. */
#define ICEM_MLP_MAX_PROBLEMS 32
typedef struct icem_mlp_problem {
    const void* params;   /* this problem's packed MLP (icem_mlp_param_elems() 16-bit words) */
    int64_t action_row0;  /* its first row of `actions`; problems may overlap or coincide */
    int32_t rows;         /* >= 1 */
    int32_t obs_row;      /* its start observation: row of obs0 [n_obs, obs_dim] */
} icem_mlp_problem;
int icem_mlp_rollout_cost_models(int32_t n_problems, const icem_mlp_problem* problems_host, int32_t horizon, int32_t obs_dim,
                                 int32_t act_dim, int32_t layers, int32_t activation, int32_t cost_mode, const icem_cost_spec* cost,
                                 const icem_cost_terms* terms, const void* obs0, int32_t n_obs, const void* actions, int64_t n_action_rows,
                                 void* costs, void* observations /* NULL or [sum rows, h + 1, obs_dim] */, void* stream);
/* An ensemble of `members` MLPs (params_host [members]: host array of device pointers, read before the call returns) scores
 * the SAME n rows of actions [n, horizon, act_dim] from one observation obs0 [obs_dim]: ONE models launch of `members` problems
 * that share the action rows, then icem_rssm_ensemble_reduce (which knows nothing of the model; `reduce`: ICEM_RSSM_REDUCE_MEAN
 * or _MAX).  member_costs [members, n] is an OUTPUT (row e: member e alone, bit for bit icem_mlp_rollout_cost with its params),
 * costs [n] their reduction.  members == 1 gives the solo launch's bits in both.  Refusals as above (members outside [1, 32],
 * n < 1, a bad reduce: ICEM_E_INVALID), before anything is launched; nothing is allocated. */
int icem_mlp_rollout_cost_ensemble(int32_t members, const void* const* params_host, int32_t n, int32_t horizon, int32_t obs_dim,
                                   int32_t act_dim, int32_t layers, int32_t activation, int32_t cost_mode, int32_t reduce,
                                   const icem_cost_spec* cost, const icem_cost_terms* terms, const void* obs0, const void* actions,
                                   void* member_costs /* [members, n], output */, void* costs /* [n] */, void* stream);
/* The iCEM MPC step through that model as ONE call: icem_plan_step_learned_models (above) with the MLP launch in the rollout's
 * place -- for one planner or n, through one model, a model each, one shared ensemble or an ensemble each.  params_host
 * [n * members] (host array of device pointers, problem-major, read before the call returns): problem p's members are
 * params_host[p * members .. (p + 1) * members), each a packed buffer of icem_mlp_param_elems(model->obs_dim, act_dim,
 * model->layers) words.  A shared model is members == 1 with the same pointer n times, a shared ensemble repeats its `members`
 * pointers per problem, a model each / an ensemble each name distinct buffers.  *model: the shape and activation all of them share
 * and the cost pair that scores every problem (act_dim, the horizon and cost_mode are the handles').
 *   Semantics: icem_plan_step_learned_models' in every point -- noise offsets, elite halves, the shifted rows of a problem reset
 * later than its peers, the epilogue, `results` [n, act_dim + 1], member_costs (NULL, or at least members * n * the largest
 * iteration's rows of one problem; afterwards the LAST iteration's [members, rows of all problems]), the argument blocks with
 * handles[0] uploaded only when a byte changed, free alternation with the other steps and the stage-wise operators on one
 * handle.  b->obs0 is [model->obs_dim] f32.  The rollout of an iteration is ONE icem_mlp_rollout_cost_models launch of
 * n * members problems in member-major order over the observation table [n, obs_dim] (n == 1: b->obs0 itself, and the
 * problem's own actions / costs; n > 1: a pool of handles[0]'s); the update reduces the members' costs in
 * icem_rssm_ensemble_reduce's arithmetic.  3 launches per iteration, + 1 in a step that shifts elites, whatever n and members
 * (icem_mlp_step_launches of handles[0]); no host synchronisation; no staging area, no status word, no
 * icem_set_rssm_act_dim binding.  Every problem's mean, std, both elite halves with their costs, executed, best_cost and its
 * results row are bit for bit what the stage-wise operators (icem_sample_clip, icem_mlp_rollout_cost_ensemble / _models,
 * icem_update_distribution, icem_shift) give, for n == 1 the last pool in actions / costs too; members == 1 gives the bits of
 * the loop through icem_mlp_rollout_cost.
 *   Served: what icem_plan_step_learned asks of a handle except the RSSM's action width and the split launch's limit (f32,
 * world == 1, the fast path on, profiling off, rng_rounds 10, a horizon of the folded sampler, horizon * act_dim <= 512, at
 * most 16 384 candidates and 32 elites per update), act_dim <= 32, n * members <= 32; development option mlp_step = 0
 * switches the entry off.  ICEM_E_INVALID: a NULL argument, cost or params_host entry, n or members outside [1, 32], a bad
 * reduce or activation, a negative step, a NULL required buffer, the same handle twice, unequal configurations, a cost pair
 * icem_mlp_rollout_cost calls invalid (a term index outside obs_dim among it).  ICEM_E_UNSUPPORTED: n * members > 32, obs_dim
 * or layers outside the MLP's ranges (these, like the counts, before any handle is looked at), act_dim > 32, a non-NULL z_*,
 * a handle that is not served.  All of it before anything is launched or any handle touched.  icem_plan_step_mlp_ok: would n
 * handles like this one be served with `members` models each (the model's own shape is not asked)? */
typedef struct icem_mlp_step_model {
    int32_t obs_dim, layers, activation;     /* act_dim and cost_mode are the handles' */
    const icem_cost_spec*  cost;             /* required */
    const icem_cost_terms* terms;            /* may be NULL */
} icem_mlp_step_model;
int icem_plan_step_mlp_ok(const icem_handle* h, int32_t n, int32_t members);
int icem_plan_step_mlp(icem_handle* const* handles, int32_t n, const icem_plan_buffers* buffers, const icem_mlp_step_model* model,
                       int32_t members, const void* const* params_host, int32_t reduce, const int32_t* mpc_steps_host,
                       void* member_costs, void* results, void* stream);
int64_t icem_mlp_step_launches(const icem_handle* h); /* kernel launches of the last icem_plan_step_mlp this handle led (handles[0]); measurement */

/* MpcICem.get_action (icem/controllers/icem.py:106-189) as ONE call for a host caller: obs_host [obs_dim] float64
 * goes to b->obs0 through a pinned staging buffer of the handle, icem_plan_step runs, and the executed action
 * [act_dim] (+ the best cost of the last pool, if best_cost_host != NULL) comes back as float64 after ONE stream
 * synchronisation.  world == 1, device noise (b->z_* must be NULL). */
int icem_get_action(icem_handle* h, const icem_plan_buffers* b, int32_t mpc_step, const double* obs_host,
                    double* action_host, double* best_cost_host, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ICEM_HIP_H */
