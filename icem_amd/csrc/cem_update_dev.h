// cem_update_dev.h -- the f32 CEM update's argument blocks read from DEVICE memory (fused_dev.h: gptr), shared by the update
// kernels of k_cem.hip and k_cem_members.hip.  Internal; device code only.
#pragma once
#include "fused_dev.h"
#include "cem_step.h"

namespace icem {

namespace {

template <typename T>
__device__ __forceinline__ CemTailArgs<T> from_device(const CemTailArgs<T>& m) {
    CemTailArgs<T> t = m;
    t.mean = gptr(m.mean), t.std = gptr(m.std), t.low = gptr(m.low), t.high = gptr(m.high), t.lower = gptr(m.lower), t.upper = gptr(m.upper);
    t.elites = gptr(m.elites), t.elite_costs = gptr(m.elite_costs), t.executed = gptr(m.executed), t.best_cost = gptr(m.best_cost);
    t.result = gptr(m.result);
    return t;
}
__device__ __forceinline__ UpdateSmallArgs from_device(const UpdateSmallArgs& m) {
    UpdateSmallArgs u = m;
    u.costs = gptr(m.costs), u.pool = gptr(m.pool), u.keep_costs = gptr(m.keep_costs), u.keep_actions = gptr(m.keep_actions);
    u.mean = gptr(m.mean), u.std = gptr(m.std), u.elites_out = gptr(m.elites_out), u.elite_costs_out = gptr(m.elite_costs_out);
    u.idx_out = gptr(m.idx_out);
    return u;
}

}  // namespace

}  // namespace icem
