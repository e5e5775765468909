// Exhaustive check on gfx950 of vx_math.h's sqrt_ranged: hipcc's
// correctly rounded sqrtf (-fhip-fp32-correctly-rounded-divide-sqrt) is
// v_sqrt_f32 plus a one-ulp residual correction, wrapped in a 2^32 scaling for
// inputs below 2^-96 and a class test for zero / inf.  sqrt_ranged keeps the
// correction and drops the wrapper; the kernels call it for x = +-0 or
// 2^-96 <= x <= FLT_MAX and take sqrtf otherwise.  This compares the two on
// every float of that domain (2^31 - 2^23*31 normal values, both zeros).
#include <hip/hip_runtime.h>
#include <cstdio>

__device__ __forceinline__ float sqrt_ranged(float x) {
    const float s = __builtin_amdgcn_sqrtf(x);
    const float dn = __uint_as_float(__float_as_uint(s) - 1u), up = __uint_as_float(__float_as_uint(s) + 1u);
    float r = __builtin_fmaf(-dn, s, x) <= 0.0f ? dn : s;
    r = __builtin_fmaf(-up, s, x) > 0.0f ? up : r;
    return r;
}

__global__ void k_check(unsigned hi_bits, unsigned long long *bad, unsigned *first) {
    const unsigned lo = blockIdx.x * blockDim.x + threadIdx.x;          // 2^23 per launch
    const unsigned u = (hi_bits << 23) | lo;                            // sign | exponent = hi_bits
    const float x = __uint_as_float(u);
    const bool in = x == 0.0f || (x >= 0x1p-96f && x <= 3.40282347e38f);
    if (!in) return;
    const float q = sqrtf(x);
    const float s = sqrt_ranged(x);
    if (__float_as_uint(s) != __float_as_uint(q)) {
        if (atomicAdd(bad, 1ull) == 0ull) *first = u;
    }
}

int main() {
    unsigned long long *d;
    unsigned *f;
    (void)hipMalloc(&d, 8);
    (void)hipMalloc(&f, 4);
    (void)hipMemset(d, 0, 8);
    unsigned long long checked = 0;
    // exponents 31..254 (x >= 2^-96) of positive floats, and the two zero slices (hi 0 and 256)
    for (unsigned e = 0; e < 512; e++) {
        const unsigned ex = e & 255;
        if (ex != 0 && (ex < 31 || ex == 255)) continue;
        hipLaunchKernelGGL(k_check, dim3((1u << 23) / 256), dim3(256), 0, 0, e, d, f);
        checked += ex == 0 ? 1 : (1ull << 23);
    }
    unsigned long long bad = 0;
    unsigned first = 0;
    (void)hipMemcpy(&bad, d, 8, hipMemcpyDeviceToHost);
    (void)hipMemcpy(&first, f, 4, hipMemcpyDeviceToHost);
    printf("sqrt_ranged vs sqrtf on gfx950: %llu inputs (+-0 and every float in [2^-96, FLT_MAX] of both signs' "
           "positive range), %llu mismatches%s\n", checked, bad, bad ? "" : " -> exact");
    if (bad) printf("first mismatch at bits 0x%08x\n", first);
    return bad ? 1 : 0;
}
