// vx_sample.h — the texture samples of render.frag (the AO trilinear sample,
// the noise fbm and white), normalize, and the sky branch of main().
#pragma once
#include "vx_loads.h"
#include "vx_math.h"

namespace vx {
namespace {

// ---------------- sampling ----------------
// (fsize = (float)size, from the host: KernelArgs::Xf ..)
__device__ __forceinline__ void lin_axis(float coord, int size, float fsize, int &i0, int &i1, float &w) {
    const float u = coord * fsize - 0.5f;
    const float fl = floorf(u);
    w = u - fl;
    // AO coordinates are finite and far inside +-2^24 ((cell + fract) of a
    // fragment next to the grid): ivec3()'s NaN / saturation rules never
    // apply, so a plain convert is f2i here
    const int i = (int)fl;
    const int j = i + 1;
    i0 = min(max(i, 0), size - 1);
    i1 = min(max(j, 0), size - 1);
}

// sdf(ivec3, vec3) (render.frag:55-58) = min of trilinear R, G at LOD 0.
// The x-neighbours come in pairs (a.rg2): entry p of a row holds (R, G) of
// cells clamp(p - 1) and clamp(p), so the lerp's two x corners i0 =
// clamp(i), i1 = clamp(i + 1) are ONE typed load at p = clamp(i, -1, X - 1) + 1
// (i <= -1: (0, 0); i >= X - 1: (X - 1, X - 1); else (i, i + 1) -- exactly
// lin_axis's CLAMP_TO_EDGE pair).  Four 8_8_8_8 UNORM loads per sample
// instead of eight 8_8 ones, the same RN(b / 255) values, the same lerps.
__device__ __forceinline__ float sdf_lin(const KernelArgs &a, float c0, float c1, float c2, float f0, float f1, float f2) {
    const FrameConsts &F = a.fc;
    int y0, y1, z0, z1;
    float wx, wy, wz;
    const float ux = (c0 + f0) * F.sf[0] * a.Xf - 0.5f;
    const float flx = floorf(ux);
    wx = ux - flx;
    const int px = min(max((int)flx, -1), a.X - 1) + 1;     // pair index (AO coordinates are far inside +-2^24)
    lin_axis((c1 + f1) * F.sf[1], a.Y, a.Yf, y0, y1, wy);
    lin_axis((c2 + f2) * F.sf[2], a.Z, a.Zf, z0, z1, wz);
    // one byte offset and two deltas (0 or one row / plane: the clamped corners
    // differ by at most one cell per axis)
    const unsigned row = (unsigned)a.X + 1u;
    const unsigned b00 = ((unsigned)px + __umul24(row, (unsigned)y0) + __umul24(__umul24(row, (unsigned)a.Y), (unsigned)z0)) << 2;
    const unsigned dy = __umul24((unsigned)(y1 - y0), 4u * row), dz = __umul24((unsigned)(z1 - z0), 4u * row * (unsigned)a.Y);
    const u32x4 rs = buf_rsrc(a.rg2, kRsrcRGBA);
    const f32x4 u00 = ld_fmt4(rs, b00), u10 = ld_fmt4(rs, b00 + dy);
    const f32x4 u01 = ld_fmt4(rs, b00 + dz), u11 = ld_fmt4(rs, b00 + dy + dz);
    float res[2];
#pragma unroll
    for (int ch = 0; ch < 2; ch++) {
        const float v00 = gmix(u00[ch], u00[2 + ch], wx);
        const float v01 = gmix(u10[ch], u10[2 + ch], wx);
        const float v10 = gmix(u01[ch], u01[2 + ch], wx);
        const float v11 = gmix(u11[ch], u11[2 + ch], wx);
        const float w0 = gmix(v00, v01, wy);
        const float w1 = gmix(v10, v11, wy);
        res[ch] = gmix(w0, w1, wz) * 255.0f;
    }
    // fmin_fin: each res is a chain of lerps of texels k/255 with weights in
    // [0, 1], times 255 -- finite, and >= +0 (products and sums of values >= +0
    // are never -0)
    return fmin_fin(res[0], res[1]);
}

// REPEAT wrap of an integer-valued float onto [0, n), n a power of two:
// |fl| < 2^24 (every cloud lookup; a mountain lookup unless r1 ~ 0): fl - q*n
// is exact and in [0, n), i.e. (int)fl mod n = (int)fl & (n - 1).  The literal
// form only for the lanes outside that range (NaN included): floor(fl / n)
// with the IEEE quotient by n = 2^k, which is exactly fl * 2^-k (fl is 0 or
// |fl| >= 1: no underflow).
__device__ __forceinline__ int wrap_idx(float fl, int n, float fn) {   // fn = (float)n (KernelArgs::noise_wf, _hf)
    int r = (int)fl & (n - 1);
    if (!(fabsf(fl) < 16777216.0f)) {
        // 1/n from fn = 2^k, which the caller's hot path holds in a register already:
        // its exponent mirrored, 2^-k = bits(2^0) * 2 - bits(2^k), one scalar
        // subtraction (a division of two scalars would run on the vector unit).  Not
        // from a kernel argument of its own: a load sunk into this rare block would be
        // tail-merged across the u/v calls into a pointer phi -- a KernelArgs copy to scratch
        const float rn = __uint_as_float(0x7F000000u - __float_as_uint(fn));
        const float q = floorf(fl * rn);
        r = f2i(fl - q * fn) & (n - 1);
    }
    return r;
}

// fbm(p) = 1 - 2*texture(u_noise, p).a (render.frag:16-24), bilinear, REPEAT, LOD 0.
// The four A texels of the bilinear footprint are one typed load from the quad
// texture a.noise4 (entry (x, y) = A of (x, y), (x+1, y), (x, y+1), (x+1, y+1),
// REPEAT-wrapped when it was built): the same RN(b / 255) values.
__device__ __forceinline__ float fbm(const KernelArgs &a, float px, float py) {
    const int W = a.noise_w, H = a.noise_h;
    const float u = px * a.noise_wf - 0.5f, v = py * a.noise_hf - 0.5f;
    const float fu = floorf(u), fv = floorf(v);
    const float wa = u - fu, wb = v - fv;
    const int x0 = wrap_idx(fu, W, a.noise_wf), y0 = wrap_idx(fv, H, a.noise_hf);
    const u32x4 rs = buf_rsrc(a.noise4, kRsrcRGBA);
    const f32x4 t = ld_fmt4(rs, (((unsigned)y0 << a.noise_lw) | (unsigned)x0) << 2);
    const float r0 = gmix(t.x, t.y, wa), r1 = gmix(t.z, t.w, wa);
    return 1.0f - 2.0f * gmix(r0, r1, wb);
}

// normalize3 of a vector whose length lies in [2^-40, 2^41) (exactly the IEEE result)
__device__ __forceinline__ void normalize3_ranged(float v0, float v1, float v2, float &o0, float &o1, float &o2) {
    const float l = sqrt_ranged(v0 * v0 + v1 * v1 + v2 * v2);   // callers: |v|^2 in [2^-80, 2^82)
    const float y = rcp_ranged(l);
    o0 = div_shared(v0, l, y); o1 = div_shared(v1, l, y); o2 = div_shared(v2, l, y);
}
__device__ __forceinline__ void normalize3(float v0, float v1, float v2, float &o0, float &o1, float &o2) {
    const float l = sqrtf(v0 * v0 + v1 * v1 + v2 * v2);
    const float y = 1.0f / l;       // one IEEE reciprocal, three exact corrections
    o0 = div_shared(v0, l, y); o1 = div_shared(v1, l, y); o2 = div_shared(v2, l, y);
}

// ---------------- render.frag main(), sky branch (render.frag:148-205) ----------------
// The sky's ray direction and clear-sky colour (render.frag:152-176).  RANGED:
// the length of d is known to lie in [2^-40, 2^41) (a view ray of a frame
// whose FrameConsts::rays_ranged is set), so normalize3_ranged is the IEEE
// result and r is finite, |r_i| <= 1.
template <bool RANGED>
__device__ __forceinline__ void sky_clear(const FrameConsts &F, float d0, float d1, float d2, float &r0, float &r1,
                                          float &r2, float sky[3]) {
    if (RANGED) normalize3_ranged(d0, d1, d2, r0, r1, r2);
    else normalize3(d0, d1, d2, r0, r1, r2);     // skybox modelled at infinity
    // reflect(rayDir, (-1,0,0)) (render.frag:155); only .z is read.  RANGED (r finite): k is
    // finite, k * 0 a zero, so r2 - k * 0 is r2, or for r2 = +-0 a zero of either sign -- and
    // gmax(0, z) below returns its +0 for both zeros: r2 itself gives the same rz
    const float k = 2.0f * ((-1.0f * r0 + 0.0f * r1) + 0.0f * r2);
    const float refl_z = RANGED ? r2 : r2 - k * 0.0f;
    const float sunCol[3] = {1.4f, 1.0f, 0.5f};
    float sunFactor = gmax(0.0f, F.sun[0] * r0 + F.sun[1] * r1 + F.sun[2] * r2) - 1.0f;
    const float glow = vexp2(8.0f * sunFactor);
    sunFactor = vexp2(4000.0f * sunFactor) + 0.3f * glow;
    const float rz = sqrtf(gmax(0.0f, refl_z));   // (literal: r2 = d2 / |d| can lie below sqrt_ranged's 2^-96)
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const float atm = gmix(F.scatterCol[i], F.spaceCol[i], rz);
        // clamp01 where r is finite: the sun term is then finite and >= +0 (a
        // vexp2 result is), and atm, a lerp with rz in [0, 1] of two colours
        // >= 0.2, is positive -- the sum is neither NaN nor -0.  A NaN
        // direction (normalize(0), the mirror ray of a t = 0 hit) must stay
        // NaN through the clamp: the select form.
        const float v = sunCol[i] * sunFactor + atm;
        sky[i] = RANGED ? clamp01(v) : gclamp(v, 0.0f, 1.0f);
    }
}

// ranged: wave-uniform (FrameConsts::rays_ranged for a view ray, false for any
// other direction) -- one scalar branch, no per-wave test of the lengths
// (a per-wave guard costs what it saves)
// org: the ray's own origin (k_ortho), whose sky offset stands in for the frame's
__device__ __forceinline__ void shade_sky(const KernelArgs &a, float d0, float d1, float d2, float o[4],
                          Counters &cnt, bool ranged = false, const RayOrigin *org = nullptr) {
    const FrameConsts &F = a.fc;
    const float sunCol[3] = {1.4f, 1.0f, 0.5f};
    float r0, r1, r2;
    float sky[3];
    if (ranged) sky_clear<true>(F, d0, d1, d2, r0, r1, r2, sky);
    else sky_clear<false>(F, d0, d1, d2, r0, r1, r2, sky);
    r2 = fabsf(r2);                                                               // :179
    if (F.flags & VX_FLAG_NO_CLOUDS) {
        o[0] = sky[0]; o[1] = sky[1]; o[2] = sky[2]; o[3] = 1.0f;
        return;
    }
    cnt.noise_px++;
    const float ct = F.cloudTime;
    const float den = sqrt_ranged(fabsf(r2) + 0.03f);   // in [0.03, 1.03]
    float sx, sy;                                                                 // :184
    {
        const float y = rcp_ranged(den);    // den = sqrt(|r2| + 0.03) in [0.17, 1.02]
        sx = div_shared(r0, den, y); sy = div_shared(r1, den, y);
    }
    sx = sx * 0.1f; sy = sy * 0.1f;
    // (literal roots: the ranged forms hold here too -- the outer argument is +0, >= 2^-75
    // or NaN, the cloud factor in [2^-12, 1] or NaN -- but measured within noise on C3
    // and, together with axis_normal, +1 % on C5: profiles/r07_ab.txt)
    const float sl = sqrtf(sqrtf(sx * sx + sy * sy));
    sx = sx * sl; sy = sy * sl;
    // render.frag:184-203 computes both the clouds and the mountains and keeps
    // one (:199-203).  The three samples that decide or feed the first step of
    // either (the mountain height, the two cloud warps) load together; then only
    // the kept branch's last sample is taken (the mountain factor or the cloud
    // factor): the same values, one noise sample less per sky pixel.
    const float n0 = fbm(a, 2.0f * sx + ct, 2.0f * sy + ct);
    const float n1 = fbm(a, 2.0f * sx - ct, 2.0f * sy - ct);
    const float mountainPos = r0 / r1;                                            // :195
    float mountainHeight = 1.0f - fbm(a, 0.3f * mountainPos, 0.3f * mountainPos);
    mountainHeight = mountainHeight / (vexp(0.3f * mountainPos * mountainPos) * 6.0f);
    if (mountainHeight > r2 && r1 > 0.0f && r2 > 0.0f) {
        const float mountainFactor = 2.0f - fbm(a, 2.0f * (mountainPos + r1), 2.0f * (mountainPos + r2));
        const float mt[3] = {0.7f, 0.8f, 0.7f};
        const float w = mountainFactor * r2;
#pragma unroll
        for (int i = 0; i < 3; i++) sky[i] = gmix(sky[i], sky[i] * mt[i], w);
    } else {
        sx = sx * (3.0f + n0); sy = sy * (3.0f + n1);
        sx = sx + (org ? org->sky0 : F.skyOff[0]);
        sy = sy + (org ? org->sky1 : F.skyOff[1]);
        const float cloudFactor = vexp2(6.0f * (fbm(a, sx + 2.0f * ct, sy + -9.0f * ct) - 1.0f));
        const float scf = sqrtf(cloudFactor);
#pragma unroll
        for (int i = 0; i < 3; i++) sky[i] = gmix(sky[i], gmix(sunCol[i], 0.8f, scf), cloudFactor);
    }
    o[0] = sky[0]; o[1] = sky[1]; o[2] = sky[2]; o[3] = 1.0f;
}

// ---------------- extensions (DESIGN.md §3 "Extensions") ----------------
// white(p) = 1 - 2*texture(u_noise, p).rgb (render.frag:16-21), bilinear REPEAT LOD 0.
// The bilinear footprint's four texels of each channel are one typed load
// from that channel's plane of the quad texture (a.noise4 planes 1..3).
__device__ __forceinline__ void white(const KernelArgs &a, float px, float py, float &w0, float &w1, float &w2) {
    const int W = a.noise_w, H = a.noise_h;
    const float u = px * a.noise_wf - 0.5f, v = py * a.noise_hf - 0.5f;
    const float fu = floorf(u), fv = floorf(v);
    const float wa = u - fu, wb = v - fv;
    const int x0 = wrap_idx(fu, W, a.noise_wf), y0 = wrap_idx(fv, H, a.noise_hf);
    const unsigned off = (((unsigned)y0 << a.noise_lw) | (unsigned)x0) << 2, plane = ((unsigned)W * (unsigned)H) << 2;
    const u32x4 rs = buf_rsrc(a.noise4, kRsrcRGBA);
    const f32x4 tr = ld_fmt4(rs, off + plane), tg = ld_fmt4(rs, off + 2u * plane), tb = ld_fmt4(rs, off + 3u * plane);
    auto bil = [&](const f32x4 &t) { return 1.0f - 2.0f * gmix(gmix(t.x, t.y, wa), gmix(t.z, t.w, wa), wb); };
    w0 = bil(tr); w1 = bil(tg); w2 = bil(tb);
}

constexpr float kRoughScale = 0.00390625f;   // 1/256: 4 noise texels per voxel
constexpr float kRoughAmp = 0.1f;

// The axis normal of normal index ni (render.vert:14-17: 2 * axis, + 1 for the
// negative direction): +-1 on its axis, +0 on the others.  The sign from the low
// bit (bits(1.0f) | ni << 31) and one select per axis on ni >> 1, the compares
// shared with the in-face axis selects, instead of two compare / select pairs
// per axis: the same three values.
__device__ __forceinline__ void axis_normal(int ni, float &n0, float &n1, float &n2) {
    const float s = __uint_as_float(0x3f800000u | ((unsigned)ni << 31));
    const int ax = ni >> 1;
    n0 = ax == 0 ? s : 0.0f;
    n1 = ax == 1 ? s : 0.0f;
    n2 = ax == 2 ? s : 0.0f;
}

}  // namespace
}  // namespace vx
