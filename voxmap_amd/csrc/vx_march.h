// vx_march.h — the sun march of render.frag:75-142 in its variants (unpadded
// fast, padded with typed loads and doom codes, soft, literal), the first-step
// exit test and march_sun, which picks one per frame.  (The LDS brick march of
// the pooled modes: vx_pool.h.)
#pragma once
#include "vx_loads.h"
#include "vx_math.h"

namespace vx {
namespace {

// ---------------- sun march: render.frag:75-142 ----------------
// Fast exact path for sun directions with every |r_i| >= 2^-10 (no zero
// component, so no 0*inf NaN; every t finite and < 1025).  `sun` is the
// channel sdf_dir reads (R "up" for r.z > 0, else G "down").  Returns "lit"
// (step == MAX_STEPS, render.frag:234).
//
// Loop shape: rotated so that the step length of the NEXT step (fract,
// three divisions, min3: it depends only on f) is computed while the texel
// load of this step is in flight; the dependent chain of a step is then just
// safe -> f -> floor -> cell -> address -> load.  One exit test per step
// (sky, safe == 0 or the step budget); cells kept as exact fp32 integers; the
// three-way min and its tie test as min3/med3 (two or more axes share the
// minimum iff med3 == min3, then the literal length of render.frag:105-116).
// the step length from the distance terms d_i = fract(-f_i*s_i) + 1e-4 (:94-116):
// the one place that holds the quotients, the minimum and the tie rule
__device__ __forceinline__ float march_len_d(const SunRay &S, float d0, float d1, float d2) {
    const float t0 = div_const(d0, S.abs[0], S.rcp[0]);                                // :97
    const float t1 = div_const(d1, S.abs[1], S.rcp[1]);
    const float t2 = div_const(d2, S.abs[2], S.rcp[2]);
    float len = __builtin_fminf(__builtin_fminf(t0, t1), t2);                         // :100-105, one axis
    if (__builtin_amdgcn_fmed3f(t0, t1, t2) == len) {                                  // ties: literal length
        const float v0 = t0 == len ? t0 : 0.0f, v1 = t1 == len ? t1 : 0.0f, v2 = t2 == len ? t2 : 0.0f;
        len = sqrtf(v0 * v0 + v1 * v1 + v2 * v2);
    }
    return len;
}

__device__ __forceinline__ float march_len(const SunRay &S, float f0, float f1, float f2) {
    const float x0 = -f0 * S.sign[0], x1 = -f1 * S.sign[1], x2 = -f2 * S.sign[2];     // :94
    return march_len_d(S, (x0 - floorf(x0)) + 1e-4f, (x1 - floorf(x1)) + 1e-4f, (x2 - floorf(x2)) + 1e-4f);
}

// The distance terms with the sun's axis signs known at compile time (SG bit i:
// r_i > 0; the fast paths have no zero component): fract(-f*s) + 1e-4 without
// the multiply -- for s > 0 it is (-f) - floor(-f) = ceil(f) - f, the same single
// IEEE subtraction (floor(-f) = -ceil(f)); for s < 0, f - floor(f).
template <int SG>
__device__ __forceinline__ void march_terms_sg(float f0, float f1, float f2, float &d0, float &d1, float &d2) {
    d0 = ((SG & 1) ? ceilf(f0) - f0 : f0 - floorf(f0)) + 1e-4f;
    d1 = ((SG & 2) ? ceilf(f1) - f1 : f1 - floorf(f1)) + 1e-4f;
    d2 = ((SG & 4) ? ceilf(f2) - f2 : f2 - floorf(f2)) + 1e-4f;
}

// march_len with those terms
template <int SG>
__device__ __forceinline__ float march_len_sg(const SunRay &S, float f0, float f1, float f2) {
    float d0, d1, d2;
    march_terms_sg<SG>(f0, f1, f2, d0, d1, d2);
    return march_len_d(S, d0, d1, d2);
}

// march_len_sg inside the march loop, where every f_i is a step's
// f - floor(f), so f_i in [0, 1]: each fract term is one v_fract_f32 (a
// 4-cycle op, against floor/ceil + subtract = 6).  v_fract(x) is x - floor(x)
// clamped below 1.0; the two uses never reach the clamp:
//   s < 0: v_fract(f) = f for f in [0, 1), 0 for f = 1 -- exactly f - floor(f);
//   s > 0: v_fract(-f) = RN(1 - f) for f in (0, 1], 0 for f = 0 -- exactly
//          ceil(f) - f, unless RN(1 - f) = 1.0, i.e. 0 < f <= 2^-25.  That f
//          never occurs after a step taken from an f >= 0 (every step after
//          the first): the axis moves by RN(RN(r*safe)*len) >= 2^-10 * 1e-4
//          (|r_i| >= 2^-10 on the fast path, safe >= 1, len >= 1e-4 since
//          every d >= 1e-4 and |r| <= 1), so f_u >= 9.7e-8 and its fraction
//          is f_u itself or a multiple of ulp(1) = 2^-23.
// The first step starts from the surface's fract, which can be slightly
// negative (the hit point's rounding), so march_pad keeps march_len_sg there.
template <int SG>
__device__ __forceinline__ float march_len_fract(const SunRay &S, float f0, float f1, float f2) {
    return march_len_d(S, __builtin_amdgcn_fractf((SG & 1) ? -f0 : f0) + 1e-4f,
                       __builtin_amdgcn_fractf((SG & 2) ? -f1 : f1) + 1e-4f,
                       __builtin_amdgcn_fractf((SG & 4) ? -f2 : f2) + 1e-4f);
}

__device__ __forceinline__ bool march_fast(const KernelArgs &a, const SunRay &S, const uint8_t *sun, float c0, float c1, float c2, float f0,
                           float f1, float f2, Counters &cnt) {
    const FrameConsts &F = a.fc;
    const float r0 = S.r[0], r1 = S.r[1], r2 = S.r[2];
    const int maxs = F.max_steps;
    if (maxs <= 0) return maxs == 0;
    float safe = 1.0f;
    float e0 = c0, e1 = c1, e2 = c2;
    float len = march_len(S, f0, f1, f2);
    int step = 0;
    const unsigned nl = active_lanes();
    do {
        f0 = f0 + (r0 * safe) * len;                                             // :118
        f1 = f1 + (r1 * safe) * len;
        f2 = f2 + (r2 * safe) * len;
        const float fl0 = floorf(f0), fl1 = floorf(f1), fl2 = floorf(f2);
        e0 += fl0; e1 += fl1; e2 += fl2;                                         // :119 (exact)
        f0 = f0 - fl0; f1 = f1 - fl1; f2 = f2 - fl2;                             // :120
        const int i0 = (int)e0, i1 = (int)e1, i2 = (int)e2;
        const bool sky = (unsigned)i0 >= (unsigned)a.X || (unsigned)i1 >= (unsigned)a.Y || (unsigned)i2 >= (unsigned)a.Z;
        const uint32_t t = sun[sky ? 0u : lin_index(a, i0, i1, i2)];             // :123-128
        cnt.shadow_fetch += sky ? 0u : 1u;
        cnt.march_witers += once_per_wave(1u);
        cnt.march_slots += once_per_wave(nl);
        len = march_len(S, f0, f1, f2);                                          // next step, under the load
        // safe < 0 marks "lit": left the grid (:123-126), or the step that
        // reaches MAX_STEPS, whatever it read (:234 tests step, not safe)
        safe = sky ? -1.0f : (float)t;
        if (++step >= maxs) safe = -1.0f;
    } while (safe > 0.0f);
    return safe < 0.0f;
}

// The same march over the int8 sun channels inside a border of -1 cells
// (vx_scene_create, Z <= 126): a step moves at most safe + 1 <= Z + 1 cells
// per axis, so the texel a lane loads after leaving the grid is a border
// cell and its -1 is the exit ("lit", render.frag:123-126) -- no bounds test.
// The last step (step MAX_STEPS-1 -> MAX_STEPS) is lit whatever it reads
// (:234), so the loop runs MAX_STEPS-1 steps with the step test on the scalar
// unit, and a lane still marching afterwards is lit.
//
// Cells as fp32 integers, x and z biased by 2^23 (exact below 2^24): the bit
// pattern of 2^23 + n is 0x4B000000 + n, so the x + Xp*y part of the offset is
// the bit pattern of one exact fma and the low 24 bits of the z pattern are z
// itself -- no float -> int converts in the loop:
//   bits(fma(y, Xp, 2^23 + x)) + u24(bits(2^23 + z)) * XpYp
//     = 0x4B000000 + x + Xp*y + XpYp*z,
// read from the channel base moved down by 0x4B000000 (vx_scene_create checks
// Xp*Yp < 2^23 and the sum < 2^32).  The x + Xp*y part is carried as one
// biased fp32 integer exy (2^23 <= exy < 2^24) and moved by fma(fl1, Xp, fl0)
// per step.  The texel arrives as a float (kRsrcS8): safe directly, -1 = left
// the grid.
// march_pad's loop from a start state: exy, e2 = the start cell's biased
// offset terms, len = the first step's length (march_len_sg), rsrc = the
// channel's typed-load descriptor (march_pad; march_soft shares these across
// the samples of a fragment).
// A doom code (a frame's cone copy, launch_sun_doom: kDoomBase - C)
// read at landing j: the cell is one from which every ray of the frame's window
// meets a solid cell after at most C boundary crossings, so the march lands on
// a 0 texel within 2 C landings -- unlit (0) if that is before MAX_STEPS, else
// the march goes on from the cell's texel T, read from the plain channel
// (oracle march_ex).  Anything else is returned as read.
__device__ __forceinline__ float doom_resolve(const KernelArgs &a, float t, int j, int maxs, unsigned off) {
    if (t <= -8.5f) {
        const int c = (int)(-8.0f - t);                                           // C
        t = j + 2 * c < maxs ? 0.0f : ld_fmt1(buf_rsrc(a.sunp - 0x4B000000, kRsrcS8), off);
    }
    return t;
}

// DOOM (kDoomAfter): the copy may hold doom codes.  The peeled first landing
// resolves its own; a code read in the loop ends the loop like any negative
// value and is resolved after it (landing j), a late one marching on in a
// per-lane loop of its own, so the main loop keeps its scalar step count.
// (Resolving in the loop at the wave's landing instead measured slower on C5
// and C3, though it keeps the hard units' step loop free of spills:
// profiles/r06_ab_doom3_c5.txt, r06_ab_doom10_*.txt.)
constexpr int kDoomNone = 0, kDoomAfter = 1;
template <int SG, int DOOM = kDoomNone>
__device__ __forceinline__ bool march_pad_from(const KernelArgs &a, const SunRay &S, u32x4 rsrc, float exy, float e2,
                                               float len, float f0, float f1, float f2, Counters &cnt) {
    const float r0 = S.r[0], r1 = S.r[1], r2 = S.r[2];
    const int maxs = a.fc.max_steps;
    if (maxs <= 0) return maxs == 0;
    const float xpf = a.SXpf;
    const unsigned sxpyp = a.SXpYp;
    float tv = 1.0f;                            // texel of the current cell = safe (render.frag:86: 1)
    // one step of :94-128 -> the offset of the texel to load
    auto advance = [&]() -> unsigned {
        f0 = f0 + (r0 * tv) * len;                                                // :118
        f1 = f1 + (r1 * tv) * len;
        f2 = f2 + (r2 * tv) * len;
        const float fl0 = floorf(f0), fl1 = floorf(f1), fl2 = floorf(f2);
        f0 = f0 - fl0; f1 = f1 - fl1; f2 = f2 - fl2;                              // :120
        exy += __builtin_fmaf(fl1, xpf, fl0); e2 += fl2;                          // :119 (exact)
        return __umul24(__float_as_uint(e2), sxpyp) + __float_as_uint(exy);
    };
    // the offset of the cell the last step landed in
    auto cell_off = [&]() -> unsigned { return __umul24(__float_as_uint(e2), sxpyp) + __float_as_uint(exy); };
    int step = 0;                                                                // wave-uniform
    const unsigned nl = active_lanes();
    if (maxs > 1) {                            // the first step, peeled: its len from march_len_sg
        float t = ld_fmt1(rsrc, advance());                                        // :123-128
        len = march_len_sg<SG>(S, f0, f1, f2);  // next step, under the load
        cnt.shadow_fetch += t >= 0.0f ? 1u : 0u;
        if constexpr (DOOM != kDoomNone) t = doom_resolve(a, t, 1, maxs, cell_off());
        tv = t;
        cnt.march_witers += once_per_wave(1u);
        cnt.march_slots += once_per_wave(nl);
        ++step;
    }
    if (maxs > 1 && tv > 0.0f && step < maxs - 1) {
        int j = 1;                             // DOOM: the lane's landings (the loop's exit leaves step behind)
        do {
            float t = ld_fmt1(rsrc, advance());
            len = march_len_fract<SG>(S, f0, f1, f2);   // next step, under the load
            cnt.shadow_fetch += t >= 0.0f ? 1u : 0u;
            tv = t;
            if constexpr (DOOM == kDoomAfter) ++j;
            cnt.march_witers += once_per_wave(1u);   // counted in the loop: step stays a scalar
            cnt.march_slots += once_per_wave(nl);
        } while (tv > 0.0f && ++step < maxs - 1);
        if constexpr (DOOM == kDoomAfter) {
            if (tv <= -8.5f) {                 // a doom code at landing j
                tv = doom_resolve(a, tv, j, maxs, cell_off());
                while (tv > 0.0f && j < maxs - 1) {   // late: on from the cell's texel (rare)
                    const unsigned o = advance();
                    const float t2 = ld_fmt1(rsrc, o);
                    len = march_len_fract<SG>(S, f0, f1, f2);
                    cnt.shadow_fetch += t2 >= 0.0f ? 1u : 0u;
                    cnt.march_witers += once_per_wave(1u);
                    cnt.march_slots += once_per_wave(nl);
                    tv = doom_resolve(a, t2, ++j, maxs, o);
                }
            }
        }
    }
    if (tv > 0.0f) {                           // the MAX_STEPS-th step: only its fetch (stats) matters
        const float t = ld_fmt1(rsrc, advance());   // (dropped unless counted)
        cnt.shadow_fetch += t >= 0.0f ? 1u : 0u;
    }
    return tv != 0.0f;
}

template <int SG, int DOOM = kDoomNone>   // the sun's axis signs (bit i: r_i > 0); DOOM: see march_pad_from
__device__ __forceinline__ bool march_pad(const KernelArgs &a, const SunRay &S, const int8_t *sun, float c0, float c1,
                                          float c2, float f0, float f1, float f2, Counters &cnt) {
    const float xpf = a.SXpf;
    constexpr float kBias = 8388608.0f;
    const float exy = __builtin_fmaf(c1 + a.SBf, xpf, (c0 + a.SBf) + kBias);   // exact integers
    const float e2 = (c2 + a.SBf) + kBias;
    const u32x4 rsrc = buf_rsrc(sun - 0x4B000000, kRsrcS8);   // (pointer arithmetic: keeps the global address space)
    return march_pad_from<SG, DOOM>(a, S, rsrc, exy, e2, march_len_sg<SG>(S, f0, f1, f2), f0, f1, f2, cnt);
}

// The soft-shadow samples of one fragment (every sample on the padded path with
// sign pattern SG, all reading `sun`): the start cell's offset terms, the
// descriptor and the first step's fract terms d_i are the same for every
// sample, so they are formed once; only the three quotients by |r_k| differ.
template <int SG>
__device__ __forceinline__ int march_soft(const KernelArgs &a, const int8_t *sun, float c0, float c1, float c2, float f0,
                                          float f1, float f2, Counters &cnt) {
    const FrameConsts &F = a.fc;
    const float xpf = a.SXpf;
    constexpr float kBias = 8388608.0f;
    const float exy = __builtin_fmaf(c1 + a.SBf, xpf, (c0 + a.SBf) + kBias);
    const float e2 = (c2 + a.SBf) + kBias;
    const u32x4 rsrc = buf_rsrc(sun - 0x4B000000, kRsrcS8);
    float d0, d1, d2;
    march_terms_sg<SG>(f0, f1, f2, d0, d1, d2);
    int lit = 0;
    for (int k = 0; k < F.n_sun; k++) {
        cnt.shadow_rays++;
        const SunRay S = F.sun_k[k];
        lit += march_pad_from<SG, kDoomAfter>(a, S, rsrc, exy, e2, march_len_d(S, d0, d1, d2), f0, f1, f2, cnt) ? 1 : 0;
    }
    return lit;
}

// Literal path for any other sun direction (zero or tiny components: the
// 0*inf = NaN and ivec3(floor(NaN)) := 0 rules of the contract apply).
__device__ __forceinline__ bool march_literal(const KernelArgs &a, const SunRay &S, const uint8_t *sun, float cf0, float cf1,
                                              float cf2, float f0, float f1, float f2, Counters &cnt) {
    int c0 = (int)cf0, c1 = (int)cf1, c2 = (int)cf2;      // exact integers
    const FrameConsts &F = a.fc;
    const float s0 = S.sign[0], s1 = S.sign[1], s2 = S.sign[2];
    const float a0 = S.abs[0], a1 = S.abs[1], a2 = S.abs[2];
    const float r0 = S.r[0], r1 = S.r[1], r2 = S.r[2];
    const int maxs = F.max_steps;
    float safe = 1.0f;
    int step = 0;
    const unsigned nl = active_lanes();
    while (step < maxs && safe != 0.0f) {
        const float x0 = -f0 * s0, x1 = -f1 * s1, x2 = -f2 * s2;
        const float d0 = (x0 - floorf(x0)) + 1e-4f;
        const float d1 = (x1 - floorf(x1)) + 1e-4f;
        const float d2 = (x2 - floorf(x2)) + 1e-4f;
        const float t0 = d0 / a0, t1 = d1 / a1, t2 = d2 / a2;
        const float m0 = t0 <= gmin(t1, t2) ? 1.0f : 0.0f;
        const float m1 = t1 <= gmin(t2, t0) ? 1.0f : 0.0f;
        const float m2 = t2 <= gmin(t0, t1) ? 1.0f : 0.0f;
        const float v0 = m0 * t0, v1 = m1 * t1, v2 = m2 * t2;
        const float len = sqrtf(v0 * v0 + v1 * v1 + v2 * v2);
        f0 = f0 + (r0 * safe) * len;
        f1 = f1 + (r1 * safe) * len;
        f2 = f2 + (r2 * safe) * len;
        const float fl0 = floorf(f0), fl1 = floorf(f1), fl2 = floorf(f2);
        c0 += f2i(fl0); c1 += f2i(fl1); c2 += f2i(fl2);
        f0 = f0 - fl0; f1 = f1 - fl1; f2 = f2 - fl2;
        cnt.march_witers += once_per_wave(1u);
        cnt.march_slots += once_per_wave(nl);
        if (c0 >= a.X || c1 >= a.Y || c2 >= a.Z || c0 < 0 || c1 < 0 || c2 < 0) return true;
        const uint32_t t = sun[lin_index(a, c0, c1, c2)];
        cnt.shadow_fetch++;
        safe = (float)t;
        step++;
    }
    return step == maxs;
}

// The first step of a march from a face (DESIGN.md §3 "Sun exit tables", the
// first step).  A fragment starts on its face plane (f = 0 on the face axis a)
// at in-face cells c_j + floor(f_j), c_k + floor(f_k) with fractions in
// [0, 1) (RN(f + d) is monotone in d, so the step's cell moves by floor(f) +
// 0 or 1 toward the sun on each in-face axis); when the sun lies on the face's normal
// side, the first step -- len <= sqrt(3) * 1e-4/|r_a| (a tie takes the literal
// length), so it moves under 0.2 cell on the other axes -- lands in the air
// cell on the normal side or a neighbour of it toward the sun on the in-face
// axes (f_j, f_k in [0, 1)): the 2 x 2 block of bit a.  If the air cell's value
// in the exit copy carries bit a, every cell the step can land in is marked,
// so the march ends there, lit, with no fetch counted: the same lit flag and
// counters without its setup, first step and load.  Used for the soft-shadow
// samples of a fragment (one test for all of them); for the single hard
// shadow it measured +-0 on C3.  ch = the exit copy every sample reads (sg =
// their sign pattern, fast path); true = lit.
__device__ __forceinline__ bool first_step_exit(const KernelArgs &a, const int8_t *ch, int sg, const Surf &g) {
    if (a.fc.max_steps < 1) return false;
    const int ax = g.nidx >> 1;
    const bool nneg = (g.nidx & 1) != 0;                   // face normal -e_a (render.vert:14-17)
    const bool spos = (sg >> ax) & 1;                      // sun toward +e_a
    // the in-face start: cell c + floor(f), fraction f - floor(f) (a quad-relative
    // v_fractPos spans the quad: f up to CHUNK); a fraction that rounds to 1
    // (f just below 0) fails the test and the samples march
    const float fl0 = floorf(g.f0), fl1 = floorf(g.f1), fl2 = floorf(g.f2);
    const float fj = ax == 0 ? g.f1 - fl1 : g.f0 - fl0, fk = ax == 2 ? g.f1 - fl1 : g.f2 - fl2;
    const bool ok = spos != nneg && fj >= 0.0f && fj < 1.0f && fk >= 0.0f && fk < 1.0f;
    const float nb = nneg ? -1.0f : 0.0f;
    const int x = (int)(g.c0 + (ax == 0 ? nb : fl0)), y = (int)(g.c1 + (ax == 1 ? nb : fl1)),
              z = (int)(g.c2 + (ax == 2 ? nb : fl2));                 // exact integers
    // the air cell is inside the padded copy (a face lies inside the grid or on its edge)
    const unsigned off = (unsigned)(x + a.SB) + (unsigned)a.SXp * (unsigned)(y + a.SB) + a.SXpYp * (unsigned)(z + a.SB);
    const float v = ok ? ld_fmt1(buf_rsrc(ch, kRsrcS8), off) : 0.0f;
    return v <= -2.0f && v >= -8.5f && (((int)(-1.0f - v) >> ax) & 1);   // face bits, not a doom code
}

// march(cell, fract, S.r) of render.frag:233 -> "lit" (step == MAX_STEPS, :234).
// sg: S's axis-sign pattern (FrameConsts::sun_sg), read only where S.fast.
// S by value: the soft-shadow loop indexes sun_k[k] dynamically, and a
// reference into the kernel argument there made the compiler copy the whole
// KernelArgs (1.5 KB) to scratch.
// (the per-sample soft loop runs only where no cone copy serves every sample,
// so it never reads a doom code; it keeps the same form, which measured faster)
template <int DOOM = kDoomAfter>
__device__ __forceinline__ bool march_sun(const KernelArgs &a, const SunRay S, int sg, float c0, float c1, float c2, float f0,
                                          float f1, float f2, Counters &cnt) {
    if (S.fast && a.sunp) {
        // wave-uniform switch on the sun's axis signs (sg = FrameConsts::sun_sg of S, from the host: a
        // scalar integer, where three float compares of S.sign ran on the vector unit): one specialised loop each
        // the frame's cone copy, else the octant's orthant copy, else the plain channel
        const int8_t *ch = a.sunc ? a.sunc
                         : a.sunx ? a.sunx + (size_t)sg * a.sunp_texels : S.up ? a.sunp : a.sunp + a.sunp_texels;
        switch (sg) {
        // (DOOM: the frame's cone copy may hold doom codes, launch_sun_doom)
#define VX_SG(K) case K: return march_pad<K, DOOM>(a, S, ch, c0, c1, c2, f0, f1, f2, cnt);
            VX_SG(0) VX_SG(1) VX_SG(2) VX_SG(3) VX_SG(4) VX_SG(5) VX_SG(6)
            default: return march_pad<7, DOOM>(a, S, ch, c0, c1, c2, f0, f1, f2, cnt);
#undef VX_SG
        }
    }
    const uint8_t *ch = S.up ? a.sun : a.sun + a.XYZ;
    return S.fast ? march_fast(a, S, ch, c0, c1, c2, f0, f1, f2, cnt)
                  : march_literal(a, S, ch, c0, c1, c2, f0, f1, f2, cnt);
}

}  // namespace
}  // namespace vx
