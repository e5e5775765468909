// vx_shade.h — the block branch of render.frag main() (shade_block), the
// colour a mirror reflection sees (reflect_color) and the glass chain.
#pragma once
#include "vx_march.h"
#include "vx_sample.h"
#include "vx_walk.h"

namespace vx {
namespace {

// ---------------- render.frag main(), block branch (render.frag:148-176, 207-251) ----------------
// EXT: the extension instantiation (rough normals, soft shadows); has_ray:
// rayDir is given (a surface seen in a reflection) instead of the camera ray
// to the fragment (:154).  ray_out receives the rayDir used.
// The sun-facing factor of render.frag:228-229 with the (ext ROUGH) shading
// normal, exactly as shade_block computes it: the soft-shadow pass of k_render
// asks it first, to know which fragments march.
template <int EXT>
__device__ __forceinline__ float block_shade_factor(const KernelArgs &a, const Surf &g) {
    const FrameConsts &F = a.fc;
    const int ni = g.nidx;
    if (!(EXT && (F.flags & VX_FLAG_ROUGH))) return F.shadeFactor[ni];
    float n0, n1, n2;
    axis_normal(ni, n0, n1, n2);
    const int ax = ni >> 1;
    const float u = ax == 0 ? g.c1 + g.f1 : g.c0 + g.f0;
    const float v = ax == 2 ? g.c1 + g.f1 : g.c2 + g.f2;
    float w0, w1, w2, m0, m1, m2;
    white(a, u * kRoughScale, v * kRoughScale, w0, w1, w2);
    normalize3_ranged(n0 + kRoughAmp * w0, n1 + kRoughAmp * w1, n2 + kRoughAmp * w2, m0, m1, m2);
    return F.sun_down ? 0.0f : sqrtf(gmax(0.0f, (m0 * F.sun[0] + m1 * F.sun[1]) + m2 * F.sun[2]));
}

// lit_given >= 0 (EXT 2): the soft-shadow samples of this fragment were
// marched by k_render's wave pass, lit_given of them lit.
template <int EXT>
__device__ __forceinline__ void shade_block(const KernelArgs &a, const Surf &g, float o[4], Counters &cnt,
                            bool has_ray = false, float q0 = 0.0f, float q1 = 0.0f, float q2 = 0.0f,
                            float *ray_out = nullptr, int lit_given = -1) {
    const FrameConsts &F = a.fc;
    const int ni = g.nidx;
    float n0, n1, n2;
    axis_normal(ni, n0, n1, n2);
    float r0, r1, r2;
    if (EXT && has_ray) {
        r0 = q0; r1 = q1; r2 = q2;
    } else {
        normalize3((g.c0 - F.cam_cell_f[0]) + (g.f0 - F.cam_fract[0]),        // exact cell differences
                   (g.c1 - F.cam_cell_f[1]) + (g.f1 - F.cam_fract[1]),
                   (g.c2 - F.cam_cell_f[2]) + (g.f2 - F.cam_fract[2]), r0, r1, r2);   // :154
    }
    if (EXT && ray_out) { ray_out[0] = r0; ray_out[1] = r1; ray_out[2] = r2; }
    // shading normal: geometric, or (ext ROUGH) jittered by white() noise
    float m0 = n0, m1 = n1, m2 = n2;
    const bool rough = EXT && (F.flags & VX_FLAG_ROUGH);
    if (rough) {
        cnt.rough++;
        const int ax = ni >> 1;
        const float u = ax == 0 ? g.c1 + g.f1 : g.c0 + g.f0;   // first in-face axis
        const float v = ax == 2 ? g.c1 + g.f1 : g.c2 + g.f2;   // second
        float w0, w1, w2;
        white(a, u * kRoughScale, v * kRoughScale, w0, w1, w2);
        // |n + 0.1 w| lies in [0.89, 1.11] (unit axis n, |w_i| <= 1): rcp_ranged is exact
        normalize3_ranged(n0 + kRoughAmp * w0, n1 + kRoughAmp * w1, n2 + kRoughAmp * w2, m0, m1, m2);
    }
    float base0, base1, base2;
    palette(g.color, base0, base1, base2);
    float amb0 = 1.0f, amb1 = 1.0f, amb2 = 1.0f;
    if (!(F.flags & VX_FLAG_NO_AO)) {                                                  // :223-225
        cnt.ao++;
        const float ambDist = sdf_lin(a, g.c0 + n0, g.c1 + n1, g.c2 + n2, g.f0, g.f1, g.f2);
        // sqrt_ranged: ambDist is 0 or >= 2^-73, inside its checked domain.  The
        // sample is 255 times three nested lerps x * (1 - w) + y * w of texels
        // that are 0 or >= RN(1/255) > 2^-8.  A weight w = u - floor(u) of
        // u = p - 0.5 (p the rounded coordinate) is exact, and 0 or >= 2^-24:
        // for p in [0.5, 1) u is a multiple of ulp(p) = 2^-24 and w = u; for
        // p < 0.5, w = u + 1 >= 0.5; for |u| >= 0.5, w is a multiple of
        // ulp(u) >= 2^-24.  w <= 1, so 1 - w is 0 or >= 2^-24 too.  All terms
        // are >= +0, so a lerp is 0 or >= 2^-24 times its smallest non-zero
        // input (RN is monotone, nothing is near underflow): >= 2^-32, 2^-56,
        // 2^-80 after the three levels, times 255.  At most 255, so
        // 1 - sqrt lies in [-15, 1], finite and never -0: fmin_fin.
        const float ambFactor = fmin_fin(1.0f - sqrt_ranged(ambDist), 0.8f);
        amb0 = gmix(1.0f, F.shadeCol[0], ambFactor);
        amb1 = gmix(1.0f, F.shadeCol[1], ambFactor);
        amb2 = gmix(1.0f, F.shadeCol[2], ambFactor);
    }
    // (a default that ROUGH overwrites, on purpose: as an if / else the compiler splits the
    // march below by `rough` and its step loop spills -- 51 spill instructions in EXT 1's)
    float shadeFactor = F.shadeFactor[ni];                                             // :228-229
    if (rough)
        shadeFactor = F.sun_down ? 0.0f : sqrtf(gmax(0.0f, (m0 * F.sun[0] + m1 * F.sun[1]) + m2 * F.sun[2]));
    if (shadeFactor > 0.0f && !(F.flags & VX_FLAG_NO_SHADOW)) {                        // :232-235
        // the exit copy every sample reads (sunc, or the octant's orthant copy
        // when they share one sign pattern): a first step into a marked block is lit
        const int sg0 = F.sun_sg[0];
        const int8_t *xch = EXT != 2 || !a.sunp || !F.sun_k[0].fast ? nullptr
                          : a.sunc ? a.sunc
                          : a.sunx && F.soft_sg >= 0 ? a.sunx + (size_t)sg0 * a.sunp_texels : nullptr;
        const bool first_exit = xch && lit_given < 0 && first_step_exit(a, xch, sg0, g);
        if (EXT != 2) {                // the reference's hard shadow: one sun ray
            cnt.shadow_rays++;
            const bool lit = march_sun(a, F.sun_k[0], sg0, g.c0, g.c1, g.c2, g.f0, g.f1, g.f2, cnt);
            shadeFactor = shadeFactor * (lit ? 1.0f : 0.0f);
        } else if (lit_given >= 0) {   // marched by the wave pass (k_render)
            shadeFactor = shadeFactor * ((float)lit_given / (float)F.n_sun);
        } else if (first_exit) {       // every sample's first step lands in the marked block
            cnt.shadow_rays += (unsigned)F.n_sun;
            cnt.shadow_resolved += (unsigned)F.n_sun;
        } else {                       // ext soft shadows (EXT == 2): lit fraction of the sun samples
            int lit = 0;
            if (xch) {                 // one sign pattern, one copy: the shared-start loop
                switch (sg0) {
#define VX_SGS(K) case K: lit = march_soft<K>(a, xch, g.c0, g.c1, g.c2, g.f0, g.f1, g.f2, cnt); break;
                    VX_SGS(0) VX_SGS(1) VX_SGS(2) VX_SGS(3) VX_SGS(4) VX_SGS(5) VX_SGS(6)
                    default: lit = march_soft<7>(a, xch, g.c0, g.c1, g.c2, g.f0, g.f1, g.f2, cnt);
#undef VX_SGS
                }
            } else {
                for (int k = 0; k < F.n_sun; k++) {
                    cnt.shadow_rays++;
                    lit += march_sun(a, F.sun_k[k], F.sun_sg[k], g.c0, g.c1, g.c2, g.f0, g.f1, g.f2, cnt) ? 1 : 0;
                }
            }
            // ((float)F.n_sun stays a convert on the vector unit, once per shaded wave: from the host
            // as a float it measured C5 +1.0 %, DESIGN.md §3 "Round 8" step 7)
            shadeFactor = shadeFactor * ((float)lit / (float)F.n_sun);
        }
    }
    const float l0 = F.shadeCol[0] + 0.4f * shadeFactor;                               // :238
    const float l1 = F.shadeCol[1] + 0.35f * shadeFactor;
    const float l2 = F.shadeCol[2] + 0.3f * shadeFactor;
    o[0] = base0; o[1] = base1; o[2] = base2; o[3] = 1.0f;
    if (F.quality > 0) {                                                               // :242-244
        float nc0, nc1, nc2;
        if (rough) {                                                                   // :211-217 per fragment
            const float an0 = fabsf(m0), an1 = fabsf(m1), an2 = fabsf(m2);
            nc0 = (0.90f * an0 + 0.95f * an1) + 1.0f * an2;
            nc1 = (0.90f * an0 + 0.95f * an1) + 1.0f * an2;
            nc2 = (0.95f * an0 + 1.00f * an1) + 1.0f * an2;
            if (m2 < 0.0f) { nc0 = nc0 * 0.8f; nc1 = nc1 * 0.8f; nc2 = nc2 * 0.8f; }
        } else {                                                                       // per axis normal: the host's table
            nc0 = F.normalCol[ni][0]; nc1 = F.normalCol[ni][1]; nc2 = F.normalCol[ni][2];
        }
        o[0] = o[0] * ((nc0 * l0) * amb0);
        o[1] = o[1] * ((nc1 * l1) * amb1);
        o[2] = o[2] * ((nc2 * l2) * amb2);
    }
    if (g.id == 2) {                                                                   // :246-249
        const float k = 2.0f * ((m0 * r0 + m1 * r1) + m2 * r2);
        const float rz = sqrtf(gmax(0.0f, r2 - k * m2));
        o[3] = 0.8f * vexp2((r0 * m0 + r1 * m1) + r2 * m2);
#pragma unroll
        for (int i = 0; i < 3; i++) {
            const float atm = gmix(F.scatterCol[i], F.spaceCol[i], rz);
            o[i] = o[i] * (0.2f * atm);
        }
    }
}

// ext REFLECT: colour seen along the mirror reflection at glass record gl
// (rd = the camera rayDir at the fragment; R = rd with the face-axis
// component negated = reflect(rd, n) exactly), oracle reflect_color().
// org: the view ray's own origin (k_ortho): the mirror ray's sky takes its offset.
template <int EXT>
__device__ __forceinline__ void reflect_color(const KernelArgs &a, const Surf &gl, const float rd[3], float out[3],
                              Counters &cnt, const RayOrigin *org = nullptr) {
    const int ax = gl.nidx >> 1;
    const float R0 = ax == 0 ? -rd[0] : rd[0], R1 = ax == 1 ? -rd[1] : rd[1], R2 = ax == 2 ? -rd[2] : rd[2];
    const float fl0 = floorf(gl.f0), fl1 = floorf(gl.f1), fl2 = floorf(gl.f2);
    const int B0 = (int)(ax == 0 ? gl.c0 : gl.c0 + fl0);                // exact integers
    const int B1 = (int)(ax == 1 ? gl.c1 : gl.c1 + fl1);
    const int B2 = (int)(ax == 2 ? gl.c2 : gl.c2 + fl2);
    const float o0 = ax == 0 ? 0.0f : gl.f0 - fl0;
    const float o1 = ax == 1 ? 0.0f : gl.f1 - fl1;
    const float o2 = ax == 2 ? 0.0f : gl.f2 - fl2;
    const int s0 = ax == 0 ? (R0 > 0.0f ? 0 : -1) : 0;
    const int s1 = ax == 1 ? (R1 > 0.0f ? 0 : -1) : 0;
    const int s2 = ax == 2 ? (R2 > 0.0f ? 0 : -1) : 0;
    cnt.refl_rays++;
    Surf h;
    float rgba[4];
    if (walk_reflect(a, B0, B1, B2, o0, o1, o2, R0, R1, R2, s0, s1, s2, h, cnt))
        shade_block<EXT>(a, h, rgba, cnt, true, R0, R1, R2);
    else
        shade_sky(a, R0, R1, R2, rgba, cnt, false, org);
    out[0] = rgba[0]; out[1] = rgba[1]; out[2] = rgba[2];
}

// rayDir of fragment g seen from origin L (render.frag:154), as shade_block forms
// it from the frame's camera: exact cell differences, one normalize3
__device__ __forceinline__ void origin_ray(const RayOrigin &L, const Surf &g, float &r0, float &r1, float &r2) {
    normalize3((g.c0 - (float)L.cc0) + (g.f0 - L.o0), (g.c1 - (float)L.cc1) + (g.f1 - L.o1),
               (g.c2 - (float)L.cc2) + (g.f2 - L.o2), r0, r1, r2);
}

// Glass in draw order (render.js:82-91; DESIGN.md §5 "Glass"): the reference
// draws the glass quads after every opaque one, in vertex.bin order, depth test
// LESS with writes on, SRC_ALPHA blending -- a pane is blended iff it is
// nearer than the last surface written when its quad is drawn.  The nearest
// pane P1 of a ray is nearer than every other surface, so it always passes and
// is always the last pane blended: the pixel is P1 over dst', where dst' is the
// surface behind the panes with the panes drawn before P1 (key order, each
// nearer than the last one written) blended over it.  glass_chain turns dst
// (the surface behind, depth its depth) into dst'; k_render's one-blend path
// then blends P1 (g[0]) over it.  It runs for pixels whose ray crosses two or
// more panes in front of its surface (primary()'s multi): with one pane dst' =
// dst.
// org: the ray's own origin (k_ortho, XE != 0) in the camera's place: the scan
// walks from it, and each pane's rayDir is taken from it.
template <int XE>
__device__ __forceinline__ void glass_chain(const KernelArgs &a, float d0, float d1, float d2, float dst[4], float depth,
                                            Counters &cnt, const RayOrigin *org = nullptr) {
    const FrameConsts &F = a.fc;
    unsigned long long klast = 0;
    bool have_last = false, nearest = false;
    Surf cur;
    float tc;
    unsigned long long kc;
    while (glass_scan(a, d0, d1, d2, have_last, klast, depth, cur, tc, kc, nearest, org) && !nearest) {
        depth = tc; klast = kc; have_last = true;
        float src[4], rd[3];
        if (org) {
            origin_ray(*org, cur, rd[0], rd[1], rd[2]);
            shade_block<XE>(a, cur, src, cnt, true, rd[0], rd[1], rd[2]);
        } else {
            shade_block<XE>(a, cur, src, cnt, false, 0.0f, 0.0f, 0.0f, rd);
        }
        if (XE && (F.flags & (VX_FLAG_REFLECT | VX_FLAG_REFLECT_ALL))) {   // ext REFLECT: panes mirror
            float refl[3];
            reflect_color<XE>(a, cur, rd, refl, cnt, org);
            const int ax = cur.nidx >> 1;
            const float cs = gmin(fabsf(ax == 0 ? rd[0] : (ax == 1 ? rd[1] : rd[2])), 1.0f);
            const float x = 1.0f - cs, x2 = x * x;
            const float fr = 0.04f + 0.96f * ((x2 * x2) * x);
#pragma unroll
            for (int i = 0; i < 3; i++) src[i] = src[i] + fr * refl[i];
        }
        blend_canvas(src, dst, dst);        // the pane over the canvas (render.js:84-86)
    }
}

}  // namespace
}  // namespace vx
