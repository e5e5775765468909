// vx_math.h — the arithmetic of the numerical contract as
// device helpers: the GLSL built-ins spelled out, the proven hardware forms of
// min / max / clamp, the exact quotient, reciprocal and square root rewrites,
// vexp2 and the GL blend stage.  fp32, IEEE div/sqrt, no FMA contraction
// (-ffp-contract=off): every helper returns what the scalar oracle
// (oracle/vxo_render.c) computes, bit for bit.  No field data, no KernelArgs.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vx {
namespace {

constexpr int kWG = 256;      // threads per render workgroup (4 waves)
constexpr int kGlass = 21;  // render.vert:21, sdf.cpp:337
constexpr float kInf = __builtin_inff();

// ---------------- GLSL built-ins (GLSL ES 3.00 §8) ----------------
__device__ __forceinline__ float gmin(float x, float y) { return y < x ? y : x; }
__device__ __forceinline__ float gmax(float x, float y) { return x < y ? y : x; }
__device__ __forceinline__ float gclamp(float x, float a, float b) { return gmin(gmax(x, a), b); }
__device__ __forceinline__ float gmix(float x, float y, float a) { return x * (1.0f - a) + y * a; }
// The proven forms: one v_min_f32 / v_max_f32, or the result clamp of the op
// that produces x, where gmin / gmax / gclamp are a v_cmp + v_cndmask pair
// each.  The selects and the hardware ops differ only on a NaN operand (the
// select returns its first argument, the hardware the other one) and in the
// sign of a zero result when the operands are zeros of both signs, so
//   fmin_fin, fmax_fin: neither operand is NaN, and they are not +0 and -0;
//   clamp01: x is not NaN and not -0 -- or the value is only packed into a
//            byte (pack_rgba8), which takes NaN and both zeros to 0 either way.
// Each call site states why its operands qualify; tools/micro/clamp_check.hip
// runs both forms over every float (profiles/r07_clamp_check.txt).  The
// clamp of a NaN is 0 by DX10_CLAMP, which every kernel here has set
// (kernel_meta.check reads the kernel descriptors).
__device__ __forceinline__ float fmin_fin(float x, float y) { return __builtin_fminf(x, y); }
__device__ __forceinline__ float fmax_fin(float x, float y) { return __builtin_fmaxf(x, y); }
__device__ __forceinline__ float clamp01(float x) { return __builtin_amdgcn_fmed3f(x, 0.0f, 1.0f); }
// ivec(float) of the contract: NaN -> 0, saturate at +-2^24 (branch-free)
__device__ __forceinline__ int f2i(float x) {
    const float c = __builtin_fminf(__builtin_fmaxf(x, -16777216.0f), 16777216.0f);
    const int r = (int)c;
    return x == x ? r : 0;
}

// a / b, b a per-frame constant with y = RN(1/b), a > 0 (no signed zero):
// exactly the IEEE quotient.  q0 = RN(a*y) is faithful and one Markstein
// correction q1 = RN(q0 + fma(-q0, b, a)*y) is already correctly rounded
// (Markstein's theorem for y = RN(1/b); tools/markstein_check.c: 0 mismatches
// over every numerator in [1e-4, 1.0002] for thousands of divisors, random
// and adversarial mantissas; tools/micro/markstein_all.hip: every pair of
// significands).
__device__ __forceinline__ float div_const(float a, float b, float y) {
    const float q0 = a * y;
    const float r0 = __builtin_fmaf(-q0, b, a);
    return __builtin_fmaf(r0, y, q0);
}

// a / b for any sign of a (b > 0, y = RN(1/b)): div_const with the sign of a
// copied onto the result, so a = -0 gives -0 as the IEEE quotient does.
// One correction is exact for every pair of significands
// (tools/micro/markstein_all.hip, profiles/r01_markstein_all.txt), so the
// divisor may vary per pixel.
__device__ __forceinline__ float div_shared(float a, float b, float y) {
    return __builtin_copysignf(div_const(a, b, y), a);
}

// RN(1/l) for l with |l| in [2^-40, 2^41): v_rcp + one Newton step equals the
// IEEE reciprocal on every such input (tools/micro/rcp_check.hip, exhaustive
// over exponents -40..40, both signs: profiles/r01_rcp_check.txt).  Callers
// guarantee the range.
__device__ __forceinline__ float rcp_ranged(float l) {
    const float r = __builtin_amdgcn_rcpf(l);
    return __builtin_fmaf(__builtin_fmaf(-l, r, 1.0f), r, r);
}


// Correctly rounded sqrt without the wrapper hipcc puts around it.  sqrtf
// (-fhip-fp32-correctly-rounded-divide-sqrt) is v_sqrt_f32 plus a one-ulp
// residual correction, wrapped in a 2^32 input scaling for x < 2^-96 and a
// class test for zero / inf; sqrt_ranged is the correction alone, bit-identical
// to sqrtf on +-0 and on [2^-96, FLT_MAX] (tools/micro/sqrt_ranged_check.hip,
// every float of that domain: profiles/r03_sqrt_ranged_check.txt).
__device__ __forceinline__ float sqrt_ranged(float x) {
    const float s = __builtin_amdgcn_sqrtf(x);
    const float dn = __uint_as_float(__float_as_uint(s) - 1u), up = __uint_as_float(__float_as_uint(s) + 1u);
    float r = __builtin_fmaf(-dn, s, x) <= 0.0f ? dn : s;
    r = __builtin_fmaf(-up, s, x) > 0.0f ? up : r;
    return r;
}

// exp2 by the fixed degree-9 polynomial of the numerical contract.
__device__ __forceinline__ float vexp2(float x) {
    if (x != x) return x;
    if (x >= 128.0f) return kInf;
    if (x < -126.0f) return 0.0f;
    const float n = floorf(x);
    const float f = x - n;
    float p = 1.0178086e-07f;
    p = p * f + 1.3215487e-06f;
    p = p * f + 1.5252734e-05f;
    p = p * f + 1.5403530e-04f;
    p = p * f + 1.3333558e-03f;
    p = p * f + 9.6181291e-03f;
    p = p * f + 5.5504109e-02f;
    p = p * f + 2.4022651e-01f;
    p = p * f + 6.9314718e-01f;
    p = p * f + 1.0f;
    return ldexpf(p, (int)n);
}
__device__ __forceinline__ float vexp(float x) { return vexp2(x * 1.44269504f); }

// The GL blend stage (oracle blend_canvas).  Every draw blends SRC_ALPHA /
// ONE_MINUS_SRC_ALPHA (render.js:84-86) into an RGBA8 canvas (map.js:7): for a
// fixed-point buffer GLES 3.0 §4.1.7 clamps source, destination and blend
// factors to [0, 1], and the destination is the byte the canvas holds for the
// colour written before (pack_rgba8's floor(clamp(v) * 255 + 0.5)), read back
// as RN(byte / 255).  A pane over dst: clamp(src) * a + canvas8(dst) * (1 - a)
// with a = clamp(src.a); the next pane reads that back through canvas8 again.
constexpr float kRcp255 = 1.0f / 255.0f;     // RN(1/255): div_const's reciprocal
__device__ __forceinline__ float canvas8(float v) {
    return div_const(floorf(gclamp(v, 0.0f, 1.0f) * 255.0f + 0.5f), 255.0f, kRcp255);   // exactly RN(q / 255)
}
__device__ __forceinline__ void blend_canvas(const float src[4], const float dst[3], float out[3]) {
    const float al = gclamp(src[3], 0.0f, 1.0f);
#pragma unroll
    for (int i = 0; i < 3; i++) out[i] = gclamp(src[i], 0.0f, 1.0f) * al + canvas8(dst[i]) * (1.0f - al);
}

}  // namespace
}  // namespace vx
