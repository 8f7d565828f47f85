// tile_scales.h -- the launch scalars of the fp16-plane tiles (Tile16H: fused_dev.h; TileHN / TileHNc: k_rollout_hn.hip), for
// host and device code alike: plain f32 arithmetic on bit patterns, no device intrinsics (tests/units/tile_scales_host.cpp
// runs it on the CPU).
//
// A launch fixes ONE power of two S = 2^(4 - ex) from the magnitude every trajectory shares -- max(|obs0| entries, the action
// bound, 1 for a tanh model), 2^ex <= magnitude < 2^(ex + 1), ex clamped to [-100, 100] -- and carries four scalars made of
// it and of the model's scales sM / sB (FastRolloutArgs::m_scale / b_scale):
//     T = S sM,    invT = 2^(ex - 4) / sM,    invM = 1 / sM,    sact = T / sB.
// sM and sB are powers of two by construction (update_paths: 2^(7 - e) with e the frexp exponent of the model's largest
// |entry|, which lies in (1e-30, 1e30): 2^-93 .. 2^106), so 1 / sM and 1 / sB are f32 numbers too (2^-106 .. 2^93, all
// normal) and the host passes them along (FastRolloutArgs::inv_m_scale / inv_b_scale).  With an EXACT reciprocal r = 1 / s
// the quotient x / s and the product x r are the correctly rounded f32 of the same real number, for every x: the same bits,
// including where that number leaves f32's range (2^(ex - 4) r < 2^-149 rounds to zero in both forms, T r > 2^127 to
// infinity in both -- and T itself is the same rounded product in both).  No range argument beyond "r is exact" is needed;
// tile_scale_is_pow2 is the check that it is, and the host test walks every (ex, e(sM), e(sB)) all the same.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ICEM_TS_FN __host__ __device__ inline
#else
#define ICEM_TS_FN inline
#endif

namespace icem {

ICEM_TS_FN uint32_t ts_bits(float x) {
    uint32_t u;
    __builtin_memcpy(&u, &x, 4);
    return u;
}
ICEM_TS_FN float ts_float(uint32_t u) {
    float x;
    __builtin_memcpy(&x, &u, 4);
    return x;
}

// |x|, a NaN counted as 0 (a NaN observation poisons every cost anyway: the scale stays finite).  Non-negative floats order
// like their bit patterns, so the wave-wide maximum of these is an unsigned maximum of ts_bits().
ICEM_TS_FN float tile_obs_magnitude(float x) {
    const float a = ts_float(ts_bits(x) & 0x7FFFFFFFu);
    return a != a ? 0.f : a;
}

// ex of the launch: obs_max = the largest tile_obs_magnitude over obs0
ICEM_TS_FN int tile_scale_exponent(float obs_max, float act_mag, bool tanh_model) {
    float mm = obs_max > act_mag ? obs_max : act_mag;
    if (tanh_model) mm = mm > 1.f ? mm : 1.f;
    const int ex = (int)((ts_bits(mm) >> 23) & 0xFF) - 127;   // 2^ex <= mm < 2^(ex+1); mm == 0 or subnormal: -127
    return ex < -100 ? -100 : (ex > 100 ? 100 : ex);
}

// a normal power of two whose reciprocal is a normal f32 as well (exponent field 1 .. 253, no mantissa bits, positive)
ICEM_TS_FN bool tile_scale_is_pow2(float s) {
    const uint32_t u = ts_bits(s);
    return (u & 0x807FFFFFu) == 0u && (u >> 23) >= 1u && (u >> 23) <= 253u;
}
// ... and that reciprocal, exactly: 2^-e
ICEM_TS_FN float tile_scale_reciprocal(float s) { return ts_float((254u - (ts_bits(s) >> 23)) << 23); }

struct TileScales {
    float T;      // the accumulators' (and the kept state's) scale: S sM
    float invT;   // 1 / T
    float invM;   // 1 / sM: accumulators -> the B operand's scale S
    float sact;   // T / sB: an action's scale into the B operand (B sB) x (a T / sB) = T B a
};

// the product form the kernels run: inv_sM = 1 / sM, inv_sB = 1 / sB from the host
ICEM_TS_FN TileScales tile_scales(int ex, float sM, float inv_sM, float inv_sB) {
    TileScales s;
    s.T = ts_float((uint32_t)(127 + 4 - ex) << 23) * sM;
    s.invT = ts_float((uint32_t)(127 - 4 + ex) << 23) * inv_sM;
    s.invM = inv_sM;
    s.sact = s.T * inv_sB;
    return s;
}

// the division form the kernels ran before the reciprocals travelled with the arguments: the reference of the host test
ICEM_TS_FN TileScales tile_scales_by_division(int ex, float sM, float sB) {
    TileScales s;
    s.T = ts_float((uint32_t)(127 + 4 - ex) << 23) * sM;
    s.invT = ts_float((uint32_t)(127 - 4 + ex) << 23) / sM;
    s.invM = 1.f / sM;
    s.sact = s.T / sB;
    return s;
}

}  // namespace icem
