// vx_pool.h — the march only the pooled soft-shadow instantiations of k_render
// use (EXT 3, VX_FLAG_SOFT_POOL, and EXT 4, VX_FLAG_SOFT_BRICK; vx_render.h):
// the LDS brick march.  Both modes are bit-exact, opt-in and measured slower
// than the per-lane march, so it stands apart from the marches
// that ship (vx_march.h).  The pooled pass that calls it is still text of
// k_render: as a function, in every form tried, it changed the pooled kernels'
// machine code and timed slower (profiles/pool_header_ab.txt).
#pragma once
#include "vx_loads.h"
#include "vx_march.h"
#include "vx_math.h"

namespace vx {
namespace {

// march_pad with an LDS brick (VX_FLAG_SOFT_BRICK, the EXT 4 instantiation:
// north_star's "8^3 brick staging"): the pooled pass stages, per fragment, the
// 8x8x8 block of the march channel around its start cell in LDS (origin at or
// one cell behind the start on a positive axis, four to seven cells behind on a
// negative one, x aligned to 4 bytes, so the first steps toward the sun stay
// inside), and a step reads LDS when its cell lies in that brick, the global
// channel otherwise.  Same step arithmetic as
// march_pad (fract peel, exact cells), cells kept per axis for the brick test:
// local = cell - origin as exact fp32 integers, inside iff the largest of the
// three bit patterns is below bits(8.0f) (a negative local has its sign bit set).
template <int SG>
__device__ __forceinline__ bool march_brick(const KernelArgs &a, const SunRay &S, const int8_t *sun,
                                            const int8_t *brick, int ox, int oy, int oz, float c0, float c1, float c2,
                                            float f0, float f1, float f2, Counters &cnt) {
    const float r0 = S.r[0], r1 = S.r[1], r2 = S.r[2];
    const int maxs = a.fc.max_steps;
    if (maxs <= 0) return maxs == 0;
    constexpr float kBias = 8388608.0f;
    const float xpf = a.SXpf;
    const int8_t *sunb = sun - 0x4B000000;
    float e0 = (c0 + a.SBf) + kBias, e1 = c1 + a.SBf, e2 = (c2 + a.SBf) + kBias;
    // brick origin (padded cells, same biases as the cells)
    const float b0 = (float)ox + kBias, b1 = (float)oy, b2 = (float)oz + kBias;
    const unsigned sxpyp = a.SXpYp;
    float len = march_len_sg<SG>(S, f0, f1, f2);
    int tv = 1;
    int step = 0;
    const unsigned nl = active_lanes();
    bool first = true;
    do {
        const float safe = cvt_f32_ubyte0((uint32_t)tv);
        f0 = f0 + (r0 * safe) * len;                                              // :118
        f1 = f1 + (r1 * safe) * len;
        f2 = f2 + (r2 * safe) * len;
        const float fl0 = floorf(f0), fl1 = floorf(f1), fl2 = floorf(f2);
        f0 = f0 - fl0; f1 = f1 - fl1; f2 = f2 - fl2;                              // :120
        e0 += fl0; e1 += fl1; e2 += fl2;                                          // :119
        const float l0 = e0 - b0, l1 = e1 - b1, l2 = e2 - b2;                     // exact small integers
        const unsigned m = max(max(__float_as_uint(l0), __float_as_uint(l1)), __float_as_uint(l2));
        int t;
        if (m < 0x41000000u) {                                                    // inside the brick
            t = brick[(int)__builtin_fmaf(l2, 64.0f, __builtin_fmaf(l1, 8.0f, l0))];
        } else {
            const unsigned off = __umul24(__float_as_uint(e2), sxpyp) + __float_as_uint(__builtin_fmaf(e1, xpf, e0));
            t = (int)ld_off(sunb, off);
        }
        len = first ? march_len_sg<SG>(S, f0, f1, f2) : march_len_fract<SG>(S, f0, f1, f2);
        first = false;
        cnt.shadow_fetch += t >= 0 ? 1u : 0u;
        tv = t;
        cnt.march_witers += once_per_wave(1u);
        cnt.march_slots += once_per_wave(nl);
    } while (tv > 0 && ++step < maxs);
    // lit: left the grid (-1), or the MAX_STEPS-th step taken whatever it read
    // (render.frag:234: a block on the last step still ends with step == MAX_STEPS);
    // a block found earlier ends the loop with step + 1 < maxs
    return tv != 0 || step + 1 >= maxs;
}

}  // namespace
}  // namespace vx
