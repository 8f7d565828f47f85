// The launch scalars of the fp16-plane tiles (icem_amd/csrc/tile_scales.h) on the CPU: the product form the kernels run
// against the division form they ran before, bit for bit.  tests/test_tile_scales_cpu.py builds and runs this.
//
//  1. every triple (ex, e(sM), e(sB)): ex over the whole clamped range [-100, 100] (reached through tile_scale_exponent from a
//     magnitude, the clamp's edges from magnitudes beyond them), the scales over EVERY exponent tile_scale_is_pow2 accepts
//     ([-126, 126]: a superset of what update_paths produces, 2^-93 .. 2^106) -- T, invT, invM, sact compared as bit patterns;
//  2. x * (1 / s) against x / s for operands that are no powers of two (what load() scales by 1 / sM);
//  3. observation vectors: all zeros, subnormals, one NaN entry, magnitudes of 2^+-100 and beyond -- the exponent against
//     an independent one (ilogb), then both forms of the scalars;
//  4. tile_scale_is_pow2 refuses what has no exact normal reciprocal.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>
#include "tile_scales.h"

using namespace icem;

static long failures = 0;
static void fail(const char* what, double a, double b, double c) {
    if (failures < 20) std::printf("FAIL %s (%g, %g, %g)\n", what, a, b, c);
    ++failures;
}
static bool same(float a, float b) { return ts_bits(a) == ts_bits(b); }
static bool same(const TileScales& a, const TileScales& b) {
    return same(a.T, b.T) && same(a.invT, b.invT) && same(a.invM, b.invM) && same(a.sact, b.sact);
}

// the wave-wide maximum as the kernels take it: the unsigned minimum of the complemented bit patterns
static float obs_max(const std::vector<float>& obs) {
    uint32_t mn = ~0u;
    for (float v : obs) {
        const uint32_t c = ~ts_bits(tile_obs_magnitude(v));
        mn = c < mn ? c : mn;
    }
    return ts_float(~mn);
}
// ... and the exponent it has to give, worked out another way
static int ref_exponent(const std::vector<float>& obs, float act_mag, bool tanh_model) {
    double mm = act_mag;
    for (float v : obs)
        if (!std::isnan(v)) mm = std::fmax(mm, std::fabs((double)v));
    if (tanh_model) mm = std::fmax(mm, 1.0);
    if (mm < (double)std::numeric_limits<float>::min()) return -100;   // zero or subnormal: the clamp
    if (std::isinf(mm)) return 100;
    const int e = std::ilogb(mm);
    return e < -100 ? -100 : (e > 100 ? 100 : e);
}

int main() {
    long triples = 0;
    // 1. (magnitude exponents -126 .. 127 reach every ex and both clamp edges)
    for (int me = -126; me <= 127; ++me) {
        const float mag = std::ldexp(1.5f, me);
        const int ex = tile_scale_exponent(mag, 0.f, false);
        const int want = me < -100 ? -100 : (me > 100 ? 100 : me);
        if (ex != want) fail("exponent of a magnitude", me, ex, want);
        if (me < -101 || me > 101) continue;   // (the clamped ones repeat ex = +-100: one each is enough)
        for (int em = -126; em <= 126; ++em) {
            const float sM = std::ldexp(1.f, em);
            if (!tile_scale_is_pow2(sM)) fail("a power of two refused", em, 0, 0);
            const float iM = tile_scale_reciprocal(sM);
            if (!same(iM, 1.f / sM)) fail("reciprocal", em, iM, 1.f / sM);
            for (int eb = -126; eb <= 126; ++eb) {
                const float sB = std::ldexp(1.f, eb);
                const float iB = tile_scale_reciprocal(sB);
                if (!same(tile_scales(ex, sM, iM, iB), tile_scales_by_division(ex, sM, sB))) fail("triple", ex, em, eb);
                ++triples;
            }
        }
    }
    // 2.
    const float xs[] = {1.f, 0.95f, 0.05f, -3.1415927f, 1e-38f, 1e-42f, 3e38f, 0.f, -0.f, std::numeric_limits<float>::infinity()};
    for (int e = -126; e <= 126; ++e) {
        const float s = std::ldexp(1.f, e), r = tile_scale_reciprocal(s);
        for (float x : xs)
            if (!same(x * r, x / s)) fail("x / s", x, e, 0);
    }
    // 3.
    const float nan = std::numeric_limits<float>::quiet_NaN();
    std::vector<std::vector<float>> cases;
    cases.push_back(std::vector<float>(32, 0.f));
    cases.push_back(std::vector<float>(32, -0.f));
    {
        std::vector<float> v(32, 0.f);
        v[3] = 1e-40f, v[17] = -2e-45f;   // subnormals only
        cases.push_back(v);
    }
    {
        std::vector<float> v(32, 0.f);
        for (int i = 0; i < 17; ++i) v[i] = 0.1f * (float)(i - 8);
        v[5] = nan;   // one NaN entry beside ordinary ones
        cases.push_back(v);
        v[5] = -nan;
        cases.push_back(v);
    }
    cases.push_back(std::vector<float>(32, nan));
    for (int k : {-126, -120, -101, -100, -99, -30, -8, 0, 8, 30, 99, 100, 101, 120, 127})
        for (float f : {1.f, -1.9999999f}) {
            std::vector<float> v(32, 0.f);
            v[16] = std::ldexp(f, k);
            v[0] = std::ldexp(0.75f, k);
            cases.push_back(v);
        }
    {
        std::vector<float> v(32, 0.f);
        v[2] = std::numeric_limits<float>::infinity();
        cases.push_back(v);
    }
    const float act_mags[] = {0.f, 1.f, 0.4f, 1e-35f, 5e30f};
    const int scale_exps[] = {-93, -10, 0, 7, 13, 106};
    for (const auto& obs : cases)
        for (float am : act_mags)
            for (int tanh_model = 0; tanh_model < 2; ++tanh_model) {
                const int ex = tile_scale_exponent(obs_max(obs), am, tanh_model != 0);
                const int want = ref_exponent(obs, am, tanh_model != 0);
                if (ex != want) fail("exponent of an observation", ex, want, am);
                for (int em : scale_exps)
                    for (int eb : scale_exps) {
                        const float sM = std::ldexp(1.f, em), sB = std::ldexp(1.f, eb);
                        const TileScales p = tile_scales(ex, sM, tile_scale_reciprocal(sM), tile_scale_reciprocal(sB));
                        if (!same(p, tile_scales_by_division(ex, sM, sB))) fail("observation case", ex, em, eb);
                        if (std::isnan(p.T) || std::isnan(p.invT) || std::isnan(p.sact)) fail("a NaN scalar", ex, em, eb);
                    }
            }
    // 4.
    const float bad[] = {0.f, -0.f, 1e-40f, 3.f, -2.f, 0.75f, std::ldexp(1.f, 127), std::numeric_limits<float>::infinity(), nan};
    for (float b : bad)
        if (tile_scale_is_pow2(b)) fail("accepted as a power of two", b, 0, 0);
    std::printf("%ld triples, %zu observation cases, %ld failures\n", triples, cases.size(), failures);
    return failures ? 1 : 0;
}
