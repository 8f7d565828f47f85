// recorded_batch.h -- the recorded-launch plan of a batched MPC step, written once for icem_plan_step_batch / _batch_f64
// (plan.hip), icem_plan_step_cem_batch (cem_step.hip) and icem_plan_step_random_batch (random_step.hip).  Every problem's launches
// run under a LaunchRecorder (icem_fused.h: nothing is launched, a launch leaves its key and its argument block).  Recording is
// the caller's -- that is where the entries differ -- as are the blob's slot and room, the handles' state and the launch counters.
// Internal; not part of the public ABI.
#pragma once
#include "block_layout.h"
#include "host_common.h"

namespace icem {

struct RecordedBatch {
    std::vector<LaunchRecorder> recs;   // one per problem (none: a step without recorded launches -- every method then does nothing)
    std::vector<size_t> at;             // place(): each recorded launch's section

    explicit RecordedBatch(int n) : recs((size_t)n) {}
    size_t launches() const { return recs.empty() ? 0 : recs[0].launches.size(); }
    const LaunchKey& key(size_t l) const { return recs[0].launches[l].key; }
    size_t block_bytes(size_t l) const { return launch_family(key(l).family)->block_bytes; }   // (behind check())
    // the refusals, all of them before anything is launched: the problems took the same launches (their number, then LaunchKey
    // equality against problem 0), and every one's family has a row in LAUNCH_FAMILIES
    int check(const std::string& who) const {
        const size_t L = launches();
        for (const LaunchRecorder& r : recs) {
            if (r.launches.size() != L || L == 0) return fail(ICEM_E_STATE, who + "the problems' steps took different launches");
            for (size_t l = 0; l < L; ++l)
                if (!(r.launches[l].key == key(l))) return fail(ICEM_E_STATE, who + "the problems' launches differ in shape");
        }
        for (size_t l = 0; l < L; ++l)
            if (!launch_family(key(l).family)) return fail(ICEM_E_STATE, who + "a recorded launch's family has no batched launch");
        return ICEM_OK;
    }
    // one section of the caller's layout per recorded launch ...
    void place(BlockLayout& layout) {
        at.resize(launches());
        for (size_t l = 0; l < at.size(); ++l) at[l] = layout.add(block_bytes(l));
    }
    // ... problem i's blocks into a part of the host blob laid out so ...
    void copy(int i, unsigned char* part) const {
        for (size_t l = 0; l < at.size(); ++l) {
            const size_t one = block_bytes(l);
            std::memcpy(part + at[l] + one * (size_t)i, recs[i].launches[l].block, one);
        }
    }
    // ... and one batched launch per recorded launch on the device copy of that part.  *count += the launches issued
    int launch(const unsigned char* dev_part, const BatchBases& bases, hipStream_t st, long long* count) const {
        for (size_t l = 0; l < at.size(); ++l) {
            launch_family(key(l).family)->launch(key(l), dev_part + at[l], bases, (int)recs.size(), st);
            ICEM_HIP_TRY(hipGetLastError());
            ++*count;
        }
        return ICEM_OK;
    }
};

// Problem i's rollout as icem_rollout_cost would launch it for the handle, recorded: what the CEM and the random-shooting step put
// between their own two launches.  A handle whose rollout kernel has no batched twin is refused here, before the comparison.
inline int record_rollout(RecordedBatch& rb, int i, icem_handle* h, const void* obs0, const void* actions, void* costs, hipStream_t st,
                          const std::string& who) {
    BatchHint hint;
    hint.mult = (int)rb.recs.size();   // (TileHN: a batch's launches are the one-wave-per-tile kernel's; the other families keep the solo shape)
    rb.recs[i].who = who.c_str();
    if (int rc = rollout_cost_launch(h, h->cfg.num_traj, obs0, actions, costs, nullptr, LaunchCtx{st, hint, &rb.recs[i]})) return rc;
    if (rb.recs[i].unsupported)
        return fail(ICEM_E_UNSUPPORTED, who + "a launch without a batched form was reached (this handle's rollout kernel has no batched twin)");
    return ICEM_OK;
}

}  // namespace icem
