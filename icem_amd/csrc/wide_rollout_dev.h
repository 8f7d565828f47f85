// wide_rollout_dev.h -- what the by-value kernels of the exact-f32 GEMM rollout (k_rollout_wide.hip) and their batched twins
// (k_rollout_wide_batch.hip: blockIdx.y = the problem, the argument block read from a device array) share besides the kernel
// bodies (wide_rollout_body.h, wide_rows_body.h: one text, the same bits): the waves per workgroup, the dispatch table, the LDS.
#pragma once
#include <type_traits>
#include "fused_dev.h"
#include "wide_dev.h"

namespace icem {

namespace {

constexpr int WIDE_WAVES = 4;

// The one table of the exact kernel: key -> compiled instantiation, handed to `f` as (NT, KIND, EXT) constants -- the by-value
// launch and the batched one pick their kernel through it
template <class F>
bool wide_dispatch(const LaunchKey& k, F&& f) {
#define XE(NTV, KV)                                                                                                              \
    if (k.form & 1) return f(std::integral_constant<int, NTV>{}, std::integral_constant<int, KV>{}, std::true_type{}), true;     \
    return f(std::integral_constant<int, NTV>{}, std::integral_constant<int, KV>{}, std::false_type{}), true;
#define XN(NTV)                 \
    if (k.waves == NTV) {       \
        if (k.kind == 1) {      \
            XE(NTV, 1)          \
        } else {                \
            XE(NTV, 0)          \
        }                       \
    }
    XN(4) XN(8) XN(16) XN(24)
#undef XN
#undef XE
    return false;
}
inline size_t wide_lds_bytes(const LaunchKey& k) { return (size_t)WIDE_WAVES * 16 * wide_xs(k.O, k.d) * sizeof(float); }

}  // namespace

}  // namespace icem
