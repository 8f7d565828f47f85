// generic_args.h -- the argument blocks of the generic kernels (generic_kernels.hip, k_generic_batch.hip; bodies in generic_dev.h):
// what a solo launch passes by value in the kernel-argument segment and a batched launch (icem_plan_step_batch_f64) reads from a
// device array, one block per problem.  Included by icem_fused.h (behind XchgWait), whose LAUNCH_FAMILIES table sizes the blocks;
// no device code.  Internal; not part of the public ABI.
#pragma once
#include <stdint.h>
#include "cost_args.h"

namespace icem {

template <typename T>
struct SampleArgs {
    int n, h, d, F, tpw;
    long long first_index;
    const T* W;
    const T* mean;
    const T* std;
    const T* low;
    const T* high;
    const T* zr;
    const T* zi;
    uint32_t seed_lo, seed_hi, off_lo, off_hi;
    int t_begin, row0_mean;
    int white;  // noise_beta <= 0 (icem.py:77): zr is randn[n, h, d], zi unused; W is the identity
    T* out;
};

template <typename T>
struct RolloutArgs {
    int n, h, d, o;
    const T* A;  // [O, O] padded
    const T* B;  // [d, O] padded
    const T* obs0;
    const T* actions;
    T* costs;
    T* observations;  // nullable [n, h, o]
    CostArgs<T> cs;
    int cost_mode;
    int ch;  // (rows kernel) steps of actions staged in LDS at a time
    long long* dbg;  // icem_debug_stamps: phase stamps [24..29] of workgroup 0 (tools/dbg/f64_stamps.py), else null
};

template <typename T>
struct MergeArgs {
    int n_rec;        // world*K candidate records
    int n_keep;       // kept elites appended as candidates (icem.py:143-145)
    int K, h, d;
    int n_global;     // N_it: kept elite e gets gidx = n_global + e
    int last;         // last CEM iteration of the MPC step
    T alpha, init_std;
    const T* records;
    const T* elites_cur;       // [K, hd]
    const T* elites_cost_cur;  // [K]
    T* elites_next;
    T* elites_cost_next;
    const T* mean_in;  // distribution before the refit (momentum term)
    const T* std_in;
    T* mean;           // ... and where the new one goes (may alias)
    T* std;
    const T* low;
    const T* high;
    T* executed;
    T* best_cost;
    XchgWait xw;  // in-library exchange: wait for the ranks' records first (flags == nullptr: they are in place)
};

template <typename T>
struct SelectArgs {
    int n_cand;   // pool rows with a cost: the sampled rows, then (iteration 0) the shifted elites
    int n_loc;    // ... of which sampled rows (global index = pool row); the others: n_global + (row - n_loc)
    int cap;      // candidate capacity (host: SELECT_CAP)
    const T* costs;
    const T* actions;
    long long* dbg;   // icem_debug_stamps: phase stamps [16..22] (tools/dbg/f64_stamps.py), else null
    MergeArgs<T> m;   // records / n_rec / xw unused: the rows come from the pool
};

constexpr int SELECT_NT = 256;
constexpr int SELECT_CAP = 3072;

// shift_elites_kernel's arguments as a block (the solo launch passes them one by one)
template <typename T>
struct ShiftElitesArgs {
    int n_reuse, h, d, pad_;
    const T* elites;
    T* dst;
};

}  // namespace icem
