// Check on gfx950 of the mask forms in vx_walk.h's primary() against the select
// forms they replace, bit for bit.  For every exit axis
// ax, every sign triple hp and every in-face offset pair (lo, hi) in 0..31 x 0..31:
//   place   uv_offsets' select ladder against qcopy_place's two products per axis,
//           from a packed word with other bits in the fields of the other axes;
//   nidx    2 * ax + hpos against (int)fma(m2, 4, fma(m1, 2, hpf)), and the face
//           plane's step hpos ? 0 : 1 against 1 - hpf;
//   plane   (x + (ax == i ? upf : 0)) against fma(upf, m_i, x) over a dense set of
//           x: every finite exponent with 64 random mantissas, both signs, +-0,
//           and the integers around 2^22, 2^23 and 2^24 the host admits as r + cam;
//   fract   ax == i ? 0 : v against fma(-v, m_i, v) over the same set: where they
//           differ (v = -0 off the axis) is counted and reported, not an error --
//           primary() keeps the select there;
//   sign    s = hp ? 1 : -1 against fma(hp, 2, -1);
//   index   the fetch's per-lane constants: (kx4 - 4 ip0) + 2^23 against
//           fma(hp0, -4, kx4 + 2^23) for camera cells up to +-2^21 and pads up to 255,
//           and the former kz against kz_neg + the three selected terms, mod 2^32;
//   stop    col != prev && col != 0 && col != 21 against a non-zero
//           min3(col ^ prev, col, col ^ 21) for every byte pair.
// A tool, not a test: run by hand, output kept in profiles/axis_mask_check.txt.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>

enum { PLACE = 0, NIDX, UPF, PLANE, FRACT_DIFF, FRACT_OTHER, SIGN, KX4, KZ, STOP, N_SLOTS };

__device__ __forceinline__ unsigned mix(unsigned x) {      // a 32-bit hash (random mantissas and words)
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}
__device__ __forceinline__ bool same(float a, float b) { return __float_as_uint(a) == __float_as_uint(b); }

__device__ __forceinline__ void uv_offsets(int ax, float lo, float hi, float &o0, float &o1, float &o2) {
    o0 = ax == 2 ? lo : (ax == 1 ? hi : 0.0f);
    o1 = ax == 0 ? lo : (ax == 2 ? hi : 0.0f);
    o2 = ax == 1 ? lo : (ax == 0 ? hi : 0.0f);
}
__device__ __forceinline__ void qcopy_offsets(uint32_t w, int ax, float &o0, float &o1, float &o2) {
    const unsigned q = (w >> (10 * ax)) & 0x3ffu;
    uv_offsets(ax, (float)(q & 31u), (float)(q >> 5), o0, o1, o2);
}
__device__ __forceinline__ void qcopy_place(uint32_t w, unsigned sh, float m0, float m1, float m2, float &o0, float &o1,
                                            float &o2) {
    const unsigned q = w >> sh;
    const float lo = (float)(q & 31u), hi = (float)((q >> 5) & 31u);
    o0 = __builtin_fmaf(hi, m1, lo * m2);
    o1 = __builtin_fmaf(hi, m2, lo * m0);
    o2 = __builtin_fmaf(hi, m0, lo * m1);
}

// the dense set: index -> a float
__device__ float dense(unsigned i, unsigned n_rand) {
    const float special[] = {0.0f, -0.0f, 4194303.0f, -4194303.0f, 4194304.0f, -4194304.0f, 8388607.0f, -8388607.0f,
                             8388608.0f, -8388608.0f, 12582911.0f, -12582911.0f, 16777215.0f, -16777215.0f, 16777216.0f,
                             -16777216.0f, 1.0f, -1.0f, 0.5f, -0.5f, 31.0f, -31.0f, 1e-45f, -1e-45f};
    if (i >= n_rand) return special[(i - n_rand) % 24];
    const unsigned e = (i >> 7) % 255u, sg = (i >> 6) & 1u;                 // exponent 0..254: every finite one
    return __uint_as_float((sg << 31) | (e << 23) | (mix(i) & 0x7fffffu));
}

__global__ void k_values(unsigned n_rand, unsigned long long *bad) {
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_rand + 24) return;
    const float v = dense(i, n_rand);
    for (int ax = 0; ax < 3; ax++)
        for (int oct = 0; oct < 8; oct++) {
            const float hp[3] = {oct & 1 ? 0.0f : 1.0f, oct & 2 ? 0.0f : 1.0f, oct & 4 ? 0.0f : 1.0f};
            const bool x0 = ax == 0, x1 = ax == 1;
            const float m0 = x0 ? 1.0f : 0.0f, m1 = x1 ? 1.0f : 0.0f, m2 = (1.0f - m0) - m1;
            const float m[3] = {m0, m1, m2};
            const bool hpos = hp[ax] != 0.0f;
            const float hpf = __builtin_fmaf(m0, hp[0], __builtin_fmaf(m1, hp[1], m2 * hp[2]));
            const float upf_sel = hpos ? 0.0f : 1.0f, upf = 1.0f - hpf;
            for (int k = 0; k < 3; k++) {
                if (!same(v + (ax == k ? upf_sel : 0.0f), __builtin_fmaf(upf, m[k], v))) atomicAdd(&bad[PLANE], 1ull);
                const float fs = ax == k ? 0.0f : v, fm = __builtin_fmaf(-v, m[k], v);
                if (!same(fs, fm))
                    atomicAdd(&bad[(__float_as_uint(v) == 0x80000000u && ax != k) ? FRACT_DIFF : FRACT_OTHER], 1ull);
            }
        }
}

__global__ void k_cases(unsigned long long *bad) {
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;       // lo | hi << 5 | ax << 10 | oct << 12 | salt << 15
    const unsigned lo = i & 31u, hi = (i >> 5) & 31u, oct = (i >> 12) & 7u, salt = i >> 15;
    const int ax = (int)((i >> 10) & 3u);
    // the loop's stop flag, every (col, prev) byte pair (the low 16 bits of i)
    const unsigned col = i & 255u, prev = (i >> 8) & 255u;
    const bool stop = col != prev && col != 0u && col != 21u;
    if (stop != (min(min(col ^ prev, col), col ^ 21u) != 0u)) atomicAdd(&bad[STOP], 1ull);
    if (ax > 2) return;
    const bool x0 = ax == 0, x1 = ax == 1;
    const float m0 = x0 ? 1.0f : 0.0f, m1 = x1 ? 1.0f : 0.0f, m2 = (1.0f - m0) - m1;
    const float hp[3] = {oct & 1 ? 0.0f : 1.0f, oct & 2 ? 0.0f : 1.0f, oct & 4 ? 0.0f : 1.0f};
    // the word: (lo, hi) in the axis's field, hashed bits in the two others and above them
    const uint32_t field = (lo | (hi << 5)) << (10 * ax);
    const uint32_t w = (mix(i ^ (salt * 0x9e3779b9u)) & ~(0x3ffu << (10 * ax))) | field;
    float a0, a1, a2, b0, b1, b2;
    qcopy_offsets(w, ax, a0, a1, a2);
    qcopy_place(w, x0 ? 0u : (x1 ? 10u : 20u), m0, m1, m2, b0, b1, b2);
    if (!same(a0, b0) || !same(a1, b1) || !same(a2, b2)) atomicAdd(&bad[PLACE], 1ull);
    qcopy_place(w & 0u, x0 ? 0u : (x1 ? 10u : 20u), m0, m1, m2, b0, b1, b2);        // the unit split: all +0
    if (__float_as_uint(b0) | __float_as_uint(b1) | __float_as_uint(b2)) atomicAdd(&bad[PLACE], 1ull);
    const bool hpos = hp[ax] != 0.0f;
    const float hpf = __builtin_fmaf(m0, hp[0], __builtin_fmaf(m1, hp[1], m2 * hp[2]));
    if ((int)__builtin_fmaf(m2, 4.0f, __builtin_fmaf(m1, 2.0f, hpf)) != 2 * ax + (hpos ? 1 : 0)) atomicAdd(&bad[NIDX], 1ull);
    if (!same(1.0f - hpf, hpos ? 0.0f : 1.0f)) atomicAdd(&bad[UPF], 1ull);
    for (int k = 0; k < 3; k++)
        if (!same(__builtin_fmaf(hp[k], 2.0f, -1.0f), hp[k] != 0.0f ? 1.0f : -1.0f)) atomicAdd(&bad[SIGN], 1ull);
    // the fetch constants, for a hashed camera cell inside the fp32 index's bounds and at them
    const int pads[4] = {1, 17, 64, 255};
    const int edge[4] = {(1 << 21) - 1, -((1 << 21) - 1), 0, -1};
    const int pad = pads[lo & 3u];
    const int cx = (hi & 3u) == 0u ? edge[(hi >> 2) & 3u] : (int)(mix(i * 3u + 1u) % ((1u << 22) - 1u)) - ((1 << 21) - 1);
    const int ip0 = hp[0] != 0.0f, ip1 = hp[1] != 0.0f, ip2 = hp[2] != 0.0f;
    const float kx4 = (float)(4 * (cx + pad));
    if (!same(kx4 - (float)(4 * ip0) + 8388608.0f, __builtin_fmaf(hp[0], -4.0f, kx4 + 8388608.0f))) atomicAdd(&bad[KX4], 1ull);
    const unsigned kz = mix(i * 5u + 2u), XpYp = mix(i * 7u + 3u) >> 9, texels = mix(i * 11u + 4u);
    const unsigned XpYp4 = 4u * XpYp;
    const unsigned old_kz = kz - XpYp4 * (unsigned)ip2 + ((oct * texels) << 2) - 0x4B000000u - (XpYp4 << 22);
    const unsigned kz_neg = kz - 0x4B000000u - (XpYp4 << 22) + (texels << 4), kz_up = 0u - (texels << 4) - XpYp4;
    const unsigned new_kz = kz_neg + ((ip0 ? 0u : texels << 2) + (ip1 ? 0u : texels << 3) + (ip2 ? kz_up : 0u));
    if (old_kz != new_kz) atomicAdd(&bad[KZ], 1ull);
}

int main() {
    unsigned long long *d, bad[N_SLOTS];
    if (hipMalloc(&d, sizeof bad) != hipSuccess) return 2;
    (void)hipMemset(d, 0, sizeof bad);
    const unsigned n_rand = 255u * 128u, n_cases = 1u << 19;       // 16 salts of the 2^15 (lo, hi, ax, octant) cases
    hipLaunchKernelGGL(k_values, dim3((n_rand + 24 + 255) / 256), dim3(256), 0, 0, n_rand, d);
    hipLaunchKernelGGL(k_cases, dim3(n_cases / 256), dim3(256), 0, 0, d);
    if (hipMemcpy(bad, d, sizeof bad, hipMemcpyDeviceToHost) != hipSuccess) return 2;
    printf("axis_mask_check on gfx950: 3 axes x 8 sign triples x 32 x 32 offsets x 16 words; %u values x 3 axes x 8 sign triples\n",
           n_rand + 24);
    printf("quad offsets, select ladder vs two products per axis:          %llu mismatches\n", bad[PLACE]);
    printf("normal index 2 ax + hpos vs (int)fma(m2, 4, fma(m1, 2, hpf)):   %llu mismatches\n", bad[NIDX]);
    printf("plane step hpos ? 0 : 1 vs 1 - hpf:                            %llu mismatches\n", bad[UPF]);
    printf("face plane x + (ax == i ? upf : 0) vs fma(upf, m_i, x):        %llu mismatches\n", bad[PLANE]);
    printf("sign hp ? 1 : -1 vs fma(hp, 2, -1):                            %llu mismatches\n", bad[SIGN]);
    printf("fetch constant kx4, two roundings vs one fma:                  %llu mismatches\n", bad[KX4]);
    printf("fetch constant kz, octant multiply vs selected terms:          %llu mismatches\n", bad[KZ]);
    printf("stop flag, two compares and a select vs min3 != 0:             %llu mismatches\n", bad[STOP]);
    printf("fraction ax == i ? 0 : v vs fma(-v, m_i, v): differs %llu times for v = -0 off the axis (the select stays in\n"
           "primary()), %llu times elsewhere\n", bad[FRACT_DIFF], bad[FRACT_OTHER]);
    const int slots[] = {PLACE, NIDX, UPF, PLANE, SIGN, KX4, KZ, STOP, FRACT_OTHER};
    unsigned long long total = 0;
    for (int s : slots) total += bad[s];
    printf("mismatches: %llu\n", total);
    printf(total ? "FAILED\n" : "-> the mask forms equal the select forms wherever primary() uses them\n");
    return total ? 1 : 0;
}
