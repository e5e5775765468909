// Exhaustive check on gfx950 of vx_math.h's proven forms against the GLSL
// select forms they replace, over all 2^32 float bit patterns x:
//   pack   the RGBA8 byte (uint)(c(x) * 255 + 0.5) with c = gclamp(x, 0, 1)
//          (two v_cmp + v_cndmask pairs) against c = clamp01 (v_med3 / the clamp
//          output modifier, as the compiler chooses) and against the clamp
//          modifier spelled out (v_max_f32 x, x clamp): equal for EVERY x, NaN
//          and -0 included -- pack_rgba8's claim;
//   clamp  the clamped VALUES bit for bit for every x that is not NaN and not
//          -0 -- the sky colour's claim (sky_clear<true>); and how the forms
//          treat NaN (the select keeps it, the clamp gives 0: DX10_CLAMP);
//   minmax gmin / gmax against v_min_f32 / v_max_f32 (fmin_fin, fmax_fin) for
//          every x that is not NaN, against each y of a list that spans the
//          classes (zeros, subnormals, the AO cap 0.8, 1, 255, FLT_MAX, inf, both
//          signs), skipping the pairs the claim excludes: zeros of both signs;
//   sqrt   sqrt_ranged of every NaN is a NaN (what the sky's outer roots, whose
//          arguments are in sqrt_ranged's checked domain or NaN, would need;
//          they stay literal).
// A tool, not a test: run by hand, output kept in profiles/r07_clamp_check.txt.
#include <hip/hip_runtime.h>
#include <cstdio>

__device__ __forceinline__ float gmin(float x, float y) { return y < x ? y : x; }
__device__ __forceinline__ float gmax(float x, float y) { return x < y ? y : x; }
__device__ __forceinline__ float gclamp(float x, float a, float b) { return gmin(gmax(x, a), b); }
__device__ __forceinline__ float fmin_fin(float x, float y) { return __builtin_fminf(x, y); }
__device__ __forceinline__ float fmax_fin(float x, float y) { return __builtin_fmaxf(x, y); }
__device__ __forceinline__ float clamp01(float x) { return __builtin_amdgcn_fmed3f(x, 0.0f, 1.0f); }
__device__ __forceinline__ float clamp_mod(float x) {
    float r;
    asm("v_max_f32 %0, %1, %1 clamp" : "=v"(r) : "v"(x));
    return r;
}
__device__ __forceinline__ unsigned byte_of(float c) { return (unsigned)(c * 255.0f + 0.5f); }

__device__ __forceinline__ float sqrt_ranged(float x) {   // vx_math.h
    const float s = __builtin_amdgcn_sqrtf(x);
    const float dn = __uint_as_float(__float_as_uint(s) - 1u), up = __uint_as_float(__float_as_uint(s) + 1u);
    float r = __builtin_fmaf(-dn, s, x) <= 0.0f ? dn : s;
    r = __builtin_fmaf(-up, s, x) > 0.0f ? up : r;
    return r;
}

enum { PACK = 0, PACK_MOD, CLAMP, NAN_SEL_KEEPS, NAN_CLAMP_ZERO, NAN_SQRT_RANGED, MIN, MAX, N_SLOTS };

__constant__ float kY[18] = {0.0f, -0.0f, 1e-45f, -1e-45f, 1e-40f, 0x1p-126f, 0x1p-73f, 0.8f, -0.8f, 1.0f, -1.0f, 255.0f,
                             -15.0f, 3.40282347e38f, -3.40282347e38f, __builtin_inff(), -__builtin_inff(), 0x1p-96f};

__global__ void k_check(unsigned hi, unsigned long long *bad, unsigned *first) {
    const unsigned u = (hi << 23) | (blockIdx.x * blockDim.x + threadIdx.x);   // 2^23 patterns per launch
    const float x = __uint_as_float(u);
    auto fail = [&](int slot) {
        if (atomicAdd(&bad[slot], 1ull) == 0ull) first[slot] = u;
    };
    const float sel = gclamp(x, 0.0f, 1.0f), cl = clamp01(x), cm = clamp_mod(x);
    if (byte_of(sel) != byte_of(cl)) fail(PACK);
    if (byte_of(sel) != byte_of(cm)) fail(PACK_MOD);
    if (x != x) {
        const float sr = sqrt_ranged(x);
        if (sr != sr) atomicAdd(&bad[NAN_SQRT_RANGED], 1ull);
        if (sel != sel) atomicAdd(&bad[NAN_SEL_KEEPS], 1ull);
        if (__float_as_uint(cl) == 0u && __float_as_uint(cm) == 0u) atomicAdd(&bad[NAN_CLAMP_ZERO], 1ull);
        return;
    }
    if (u != 0x80000000u && (__float_as_uint(sel) != __float_as_uint(cl) || __float_as_uint(sel) != __float_as_uint(cm)))
        fail(CLAMP);
#pragma unroll
    for (int i = 0; i < 18; i++) {
        const float y = kY[i];
        if (x == 0.0f && y == 0.0f && __float_as_uint(x) != __float_as_uint(y)) continue;
        if (__float_as_uint(gmin(x, y)) != __float_as_uint(fmin_fin(x, y))) fail(MIN);
        if (__float_as_uint(gmin(y, x)) != __float_as_uint(fmin_fin(y, x))) fail(MIN);
        if (__float_as_uint(gmax(x, y)) != __float_as_uint(fmax_fin(x, y))) fail(MAX);
        if (__float_as_uint(gmax(y, x)) != __float_as_uint(fmax_fin(y, x))) fail(MAX);
    }
}

int main() {
    unsigned long long *d, bad[N_SLOTS];
    unsigned *f, first[N_SLOTS];
    if (hipMalloc(&d, sizeof bad) != hipSuccess || hipMalloc(&f, sizeof first) != hipSuccess) return 2;
    (void)hipMemset(d, 0, sizeof bad);
    (void)hipMemset(f, 0, sizeof first);
    for (unsigned hi = 0; hi < 512; hi++) hipLaunchKernelGGL(k_check, dim3((1u << 23) / 256), dim3(256), 0, 0, hi, d, f);
    if (hipMemcpy(bad, d, sizeof bad, hipMemcpyDeviceToHost) != hipSuccess) return 2;
    (void)hipMemcpy(first, f, sizeof first, hipMemcpyDeviceToHost);
    const unsigned long long nan = 2ull * ((1ull << 23) - 1ull);
    printf("clamp_check on gfx950, all 4294967296 float bit patterns x (%llu of them NaN)\n", nan);
    printf("pack byte, gclamp(x, 0, 1) vs clamp01 (fmed3):        %llu mismatches\n", bad[PACK]);
    printf("pack byte, gclamp(x, 0, 1) vs v_max_f32 x, x clamp:   %llu mismatches\n", bad[PACK_MOD]);
    printf("clamped value bits, x not NaN and not -0, all forms:  %llu mismatches\n", bad[CLAMP]);
    printf("NaN x: the select form keeps NaN on %llu, both clamp forms give +0 on %llu\n", bad[NAN_SEL_KEEPS],
           bad[NAN_CLAMP_ZERO]);
    printf("NaN x: sqrt_ranged(x) is a NaN on %llu (the sky's roots of a NaN direction stay NaN)\n", bad[NAN_SQRT_RANGED]);
    printf("gmin vs v_min_f32, x not NaN, 18 second operands, both orders, no +0/-0 pairs: %llu mismatches\n", bad[MIN]);
    printf("gmax vs v_max_f32, same pairs:                                                %llu mismatches\n", bad[MAX]);
    const int slots[] = {PACK, PACK_MOD, CLAMP, MIN, MAX};
    int rc = 0;
    for (int s : slots)
        if (bad[s]) {
            printf("slot %d: first mismatch at x bits 0x%08x\n", s, first[s]);
            rc = 1;
        }
    if (bad[NAN_SEL_KEEPS] != nan || bad[NAN_CLAMP_ZERO] != nan || bad[NAN_SQRT_RANGED] != nan) rc = 1;
    printf(rc ? "FAILED\n" : "-> the forms agree wherever vx_render.h uses them\n");
    return rc;
}
