// vx_walk.h — the walks through the octant box copies: the quad offsets a hit
// carries, the reciprocal of a ray, the primary walk (the build's replacement
// for rasterising vertex.bin), the mirror ray's walk
// (walk_reflect, primary()'s step in scalar form) and the glass draw-order scan.
#pragma once
#include "vx_loads.h"
#include "vx_math.h"
#ifndef VX_QSPEC
#define VX_QSPEC 1
#endif

namespace vx {
namespace {

// a quad's in-face offsets (lo along u = (ax+1)%3, hi along v = (ax+2)%3) per axis
__device__ __forceinline__ void uv_offsets(int ax, float lo, float hi, float &o0, float &o1, float &o2) {
    o0 = ax == 2 ? lo : (ax == 1 ? hi : 0.0f);
    o1 = ax == 0 ? lo : (ax == 2 ? hi : 0.0f);
    o2 = ax == 1 ? lo : (ax == 0 ? hi : 0.0f);
}

// The offset (per axis, as exact fp32 integers) of the face with normal index
// nidx of cell (x, y, z) from the origin of the greedy quad covering it
// (a.qface: du along u = (ax+1)%3, dv along v = (ax+2)%3, 0 on the face axis);
// a cell without that face (never a primary hit) counts as its own origin,
// as in the oracle.
__device__ __forceinline__ void quad_offsets(const KernelArgs &a, int ax, int nidx, int x, int y, int z, float &o0,
                                             float &o1, float &o2) {
    unsigned q = a.qface[(size_t)nidx * a.XYZ + lin_index(a, x, y, z)];
    q = q == 0xFFFFu ? 0u : q;
    uv_offsets(ax, (float)(q & 0xffu), (float)(q >> 8), o0, o1, o2);
}

// The same offsets from a qcopy word (the octant's entry faces, 10 bits per
// face axis ax: du | dv << 5, launch_qcopy) -- chunks of at most 32 cells.
__device__ __forceinline__ void qcopy_offsets(uint32_t w, int ax, float &o0, float &o1, float &o2) {
    const unsigned q = (w >> (10 * ax)) & 0x3ffu;
    uv_offsets(ax, (float)(q & 31u), (float)(q >> 5), o0, o1, o2);
}

// qcopy_offsets with the axis given as its field's shift (0, 10, 20) and as the
// float masks m_i = (ax == i ? 1 : 0): each offset is the sum of two products
// of which at most one is non-zero, lo and hi are integers 0..31 and the masks
// 0 or 1, so every product and the sum are exact, and a zero is +0 as the
// select form's (no factor is negative).
__device__ __forceinline__ void qcopy_place(uint32_t w, unsigned sh, float m0, float m1, float m2, float &o0, float &o1,
                                            float &o2) {
    const unsigned q = w >> sh;
    const float lo = (float)(q & 31u), hi = (float)((q >> 5) & 31u);
    o0 = __builtin_fmaf(hi, m1, lo * m2);
    o1 = __builtin_fmaf(hi, m2, lo * m0);
    o2 = __builtin_fmaf(hi, m0, lo * m1);
}

// iv = RN(1/d) (kInf for d = 0, a positive axis as -0 is) of a walk outside
// primary(), which fuses its slab products into the fast branch: rcp_ranged is
// exact for |d| in [2^-40, 2^41) -- every lane of nearly every wave; a wave with
// a lane outside it (a zero or tiny component) takes the IEEE division.
__device__ __forceinline__ void ray_rcp(float d0, float d1, float d2, float &iv0, float &iv1, float &iv2) {
    const unsigned lo_b = 0x2B800000u, span = 0x54000000u - 0x2B800000u;   // 2^-40, 2^41
    const bool ok = (__float_as_uint(fabsf(d0)) - lo_b) < span && (__float_as_uint(fabsf(d1)) - lo_b) < span &&
                    (__float_as_uint(fabsf(d2)) - lo_b) < span;
    if (__builtin_expect(__ballot(!ok) == 0, 1)) {
        iv0 = rcp_ranged(d0); iv1 = rcp_ranged(d1); iv2 = rcp_ranged(d2);
    } else {
        iv0 = d0 != 0.0f ? 1.0f / d0 : kInf;
        iv1 = d1 != 0.0f ? 1.0f / d1 : kInf;
        iv2 = d2 != 0.0f ? 1.0f / d2 : kInf;
    }
}

// ---------------- primary visibility ----------------
// The nearest front face of the greedy mesh of sdf.cpp:281-356 after back-face
// culling = the first step along the view ray that ENTERS a meshed cell (vis
// colour 1..21, vx_scene_create) from a cell of another colour.  Air (map.bin
// B = pal_size = 22, sdf.cpp:229-233) is never meshed (sdf.cpp:284), so a
// glass -> air step is no surface: glass blends over the next entry behind
// it.  The walk records the nearest glass entry and the surface behind it;
// a second glass entry before that surface sets `multi` (the panes' draw
// order then decides the pixel: k_render's stacked pass, glass_scan).  Box-exit
// stepping (oracle/vxo_render.c vxo_primary): in the ray octant's field copy
// the extents E of a cell say the box [c, c + E*s] ahead of it is air, so one
// step goes to the face where the ray leaves that box (E = 0: an exact DDA
// step).  Returns 0 sky, 1 surface, 2 glass + what is behind.
//
// The loop runs on camera-relative cells held as fp32 integers (exact: the
// host keeps |cam_cell| < 2^22), with x and y in packed-fp32 pairs:
//   h = c + hp (hp = 1 on a positive axis, 0 on a negative one), s = +-1;
//   far face    A  = c + (s > 0 ? E + 1 : -E) = fma(s, E, h)       (exact, per axis)
//   crossing    tb = (A - o) * iv                                   (= oracle)
//   exit axis   next h = A + s; others med3(floor(o + te*d) + hp, h, A)
// d == 0 is a positive axis with iv = +inf: A - o >= 1 - o > 0 (0 <= o < 1 is
// checked by vx_render), so tb = +inf exactly as the oracle's.  The box
// [c, c + E*s] lies ahead of the ray: h and A bracket it on every axis.
template <bool F32IDX>
__device__ __forceinline__ int primary(const KernelArgs &a, int oct, float d0, float d1, float d2, Surf &g0, Surf &g1,
                       Counters &cnt, float &t_hit, int &multi) {
    const FrameConsts &F = a.fc;
    const float o0 = F.cam_fract[0], o1 = F.cam_fract[1], o2 = F.cam_fract[2];
    const int cc0 = F.cam_cell[0], cc1 = F.cam_cell[1], cc2 = F.cam_cell[2];
    // iv = RN(1/d) (kInf for d = 0): rcp_ranged is exact for |d| in [2^-40,
    // 2^41) -- every lane of nearly every wave (|d| = O(1)); a wave with a lane
    // outside it (a zero or tiny component) takes the IEEE division
    // grid slabs (bounds per frame: FrameConsts::slab_lo/hi); a zero component
    // misses unless the camera lies inside that slab
    float iv0, iv1, iv2;
    float tlo = 0.0f, thi = kInf;
    bool miss = false;
    {
        const unsigned lo_b = 0x2B800000u, span = 0x54000000u - 0x2B800000u;   // 2^-40, 2^41
        const bool ok = (__float_as_uint(fabsf(d0)) - lo_b) < span && (__float_as_uint(fabsf(d1)) - lo_b) < span &&
                        (__float_as_uint(fabsf(d2)) - lo_b) < span;
        if (__builtin_expect(__ballot(!ok) == 0, 1)) {
            iv0 = rcp_ranged(d0); iv1 = rcp_ranged(d1); iv2 = rcp_ranged(d2);
            // no zero component: every slab crossing lo*iv, hi*iv is finite, and
            // the running max / min below is the general form's (a select of one
            // of its finite inputs; the sign of a zero t changes neither the
            // entry point o + t*d nor tlo < thi)
            const float a0 = F.slab_lo[0] * iv0, b0 = F.slab_hi[0] * iv0;
            const float a1 = F.slab_lo[1] * iv1, b1 = F.slab_hi[1] * iv1;
            const float a2 = F.slab_lo[2] * iv2, b2 = F.slab_hi[2] * iv2;
            tlo = __builtin_fmaxf(__builtin_fmaxf(__builtin_fminf(a0, b0), __builtin_fminf(a1, b1)),
                                  __builtin_fmaxf(__builtin_fminf(a2, b2), 0.0f));
            thi = __builtin_fminf(__builtin_fminf(__builtin_fmaxf(a0, b0), __builtin_fmaxf(a1, b1)),
                                  __builtin_fmaxf(a2, b2));
        } else {
            iv0 = d0 != 0.0f ? 1.0f / d0 : kInf;
            iv1 = d1 != 0.0f ? 1.0f / d1 : kInf;
            iv2 = d2 != 0.0f ? 1.0f / d2 : kInf;
#define VX_SLAB(D, IV, I)                                                     \
            {                                                                 \
                const float lo = F.slab_lo[I], hi = F.slab_hi[I];             \
                const float t0 = lo * IV, t1 = hi * IV;                       \
                const bool sw = t0 > t1, nz = D != 0.0f;                      \
                tlo = nz ? gmax(tlo, sw ? t1 : t0) : tlo;                     \
                thi = nz ? gmin(thi, sw ? t0 : t1) : thi;                     \
                miss |= !nz && !(lo <= 0.0f && 0.0f < hi);                    \
            }
            VX_SLAB(d0, iv0, 0)
            VX_SLAB(d1, iv1, 1)
            VX_SLAB(d2, iv2, 2)
#undef VX_SLAB
        }
    }
    if (miss || !(tlo < thi)) return 0;
    // entry cell, camera-relative, as exact fp32 integers: floor, then clamped
    // into the grid (the former int convert + clamp; o + tlo*d is finite)
    const float cf0 = __builtin_amdgcn_fmed3f(floorf(o0 + tlo * d0), F.cell_lo[0], F.cell_hi[0]);
    const float cf1 = __builtin_amdgcn_fmed3f(floorf(o1 + tlo * d1), F.cell_lo[1], F.cell_hi[1]);
    const float cf2 = __builtin_amdgcn_fmed3f(floorf(o2 + tlo * d2), F.cell_lo[2], F.cell_hi[2]);
    const bool p0 = !(d0 < 0.0f), p1 = !(d1 < 0.0f), p2 = !(d2 < 0.0f);
    // one select per axis: hp is exactly 1 or 0, so s = 2*hp - 1 is exactly +-1
    // (the fma written out: its product 2*hp is exact, one rounding of an
    // exact +-1 -- the select form's value, and never a zero)
    float hp0 = p0 ? 1.0f : 0.0f, hp1 = p1 ? 1.0f : 0.0f, hp2 = p2 ? 1.0f : 0.0f;
    asm volatile("" : "+v"(hp0), "+v"(hp1), "+v"(hp2));   // (or the compiler folds s back into a select of its own)
    const float s0 = __builtin_fmaf(hp0, 2.0f, -1.0f), s1 = __builtin_fmaf(hp1, 2.0f, -1.0f),
                s2 = __builtin_fmaf(hp2, 2.0f, -1.0f);
    float h0 = cf0 + hp0, h1 = cf1 + hp1, h2 = cf2 + hp2;
    // padded index of h: kray + hx + Xp*hy + XpYp*hz, mod 2^32 with 24-bit
    // signed products (|h| < 2^23); the octant's terms are scalars the sign
    // compares select
    const uint32_t *ppad = a.prim + (size_t)oct * a.copy_texels;
    const int kray = (int)a.kcam - (p0 ? 1 : 0) - (p1 ? a.Xp : 0) - (p2 ? (int)a.XpYp : 0);
    // F32IDX (a.prim_f32): the byte offset 4*(x + Xp*y) in fp32 (exact, <
    // 2^23), z by a 24-bit multiply-add, 32 bits from a.prim, all without
    // float -> int converts: the x/y sum is biased by 2^23 (its bit pattern is
    // 0x4B000000 + the sum) and z by 2^23 + 2^22 (|z| < 2^21: the low 24 bits
    // of the pattern are 2^22 + z); kz takes both constants back, mod 2^32.
    // The octant terms come from the host as scalars (KernelArgs::kx4b ..):
    // kx4b - 4*hp0 has integer terms that are multiples of 4 below 2^25, so the
    // fma's one rounding is exact, as the former two were; kz sums, mod 2^32,
    // what the sign compares select of 4*copy_texels << bit per negative axis
    // and of the z term (the former oct * copy_texels * 4 - 4*XpYp * ip2)
    const float kx4 = __builtin_fmaf(hp0, -4.0f, a.kx4b), ky = a.ky - hp1;
    const float fXp4 = a.Xp4f;
    const unsigned XpYp4 = 4u * a.XpYp;
    // (each select has 0 for one arm: a select between two arguments becomes a
    // load through a selected pointer into the kernel arguments)
    const unsigned kz = a.kz_neg + ((p0 ? 0u : a.koct0) + (p1 ? 0u : a.koct1) + (p2 ? a.kz_up : 0u));
    // QSPEC (the fp32-index path, a.qcopy): every step also loads the cell's
    // entry-face quad offsets from a.qcopy at the same byte offset (the copy has
    // the prim layout), so the hit's offsets arrive with its colour instead of
    // by one more dependent load after the walk (quad_offsets)
    constexpr bool QSPEC = F32IDX && VX_QSPEC;
    uint32_t qw = 0, gqw = 0;
    auto fetch = [&](float x, float y, float z) -> uint32_t {
        if (F32IDX) {
            const float xy = __builtin_fmaf(fXp4, y + ky, __builtin_fmaf(4.0f, x, kx4));
            const unsigned off = __umul24(__float_as_uint(z + 12582912.0f), XpYp4) + __float_as_uint(xy) + kz;
            if (QSPEC) qw = ld_off(a.qcopy, off);
            return ld_off(a.prim, off);
        }
        const int idx = kray + (int)x + __mul24(a.Xp, (int)y) + __mul24((int)a.XpYp, (int)z);
        return ppad[(unsigned)idx];
    };
    uint32_t t = fetch(h0, h1, h2);
    cnt.prim_fetch++;
    cnt.prim_witers += once_per_wave(1u);          // the entry fetch is a wave iteration too
    int prev = t & 0xff;
    float E0 = cvt_f32_ubyte1(t), E1 = cvt_f32_ubyte2(t), E2 = cvt_f32_ubyte3(t);
    // gmark: the colour whose entry is "the first glass" -- glass until a glass
    // entry is recorded, then 256 (matches nothing).  The sentinel's colour
    // byte 0xFF is no vis colour (those are 0..21), so leaving the grid is an
    // entry that stops the walk.
    int gmark = kGlass, stop, col, mul = 0;
    float g0h = 0.0f, g1h = 0.0f, g2h = 0.0f, gt = 0.0f, te;
    float tb0, tb1, tb2;
    int gax = 0;
    const int cap = 4 * (a.X + a.Y + a.Z);
    int it = 0;
    do {
        // far face of the air box [c, c + E*s] ahead: A = h + s*E (exact)
        const float A0 = __builtin_fmaf(s0, E0, h0), A1 = __builtin_fmaf(s1, E1, h1), A2 = __builtin_fmaf(s2, E2, h2);
        tb0 = (A0 - o0) * iv0;
        tb1 = (A1 - o1) * iv1;
        tb2 = (A2 - o2) * iv2;
        te = __builtin_fminf(__builtin_fminf(tb0, tb1), tb2);
        const bool e0 = tb0 == te;
        const bool e1 = !e0 && tb1 == te;
        // other axes: floor(o + te*d) as h, clamped into the box, whose h
        // range is [h, A] (positive axis) or [A, h] (negative): med3(q, h, A)
        const float q0 = floorf(o0 + te * d0) + hp0;
        const float q1 = floorf(o1 + te * d1) + hp1;
        const float q2 = floorf(o2 + te * d2) + hp2;
        h0 = e0 ? A0 + s0 : __builtin_amdgcn_fmed3f(q0, h0, A0);
        h1 = e1 ? A1 + s1 : __builtin_amdgcn_fmed3f(q1, h1, A1);
        h2 = (!e0 && !e1) ? A2 + s2 : __builtin_amdgcn_fmed3f(q2, h2, A2);
        t = fetch(h0, h1, h2);
        cnt.prim_fetch += t >= kSentinel ? 0u : 1u;
        col = t & 0xff;
        // a face of the mesh: entering a meshed cell (vis colour != 0) from a
        // cell of another colour; air is never meshed (sdf.cpp:229-233,284)
        // (enter = col != prev && col != 0.)  The lane's stop flag is enter &&
        // col != kGlass -- later glass entries are passed, the stacked pass blends
        // them -- as a value that is non-zero exactly then: the unsigned minimum
        // of col ^ prev, col and col ^ kGlass, one 3-operand minimum in place of
        // two compares and a select, tested once by the loop
        const unsigned dprev = (unsigned)(col ^ prev), dglass = (unsigned)(col ^ kGlass);
        if (dglass == 0 && dprev != 0) {               // a glass entry (rare, divergent)
            if (gmark == kGlass) {                     // the first: blend over the next surface
                gmark = 256;
                g0h = h0; g1h = h1; g2h = h2; gt = te;
                gax = e0 ? 0 : (e1 ? 1 : 2);
                if (QSPEC) gqw = qw;
            } else {
                mul = 1;                               // a second pane in front of the surface
            }
        }
        stop = (int)min(min(dprev, (unsigned)col), dglass);
        asm volatile("" : "+v"(stop));                 // keep the lane flag in a VGPR
        prev = col;
        E0 = cvt_f32_ubyte1(t); E1 = cvt_f32_ubyte2(t); E2 = cvt_f32_ubyte3(t);
        cnt.prim_witers += once_per_wave(1u);      // counted in the loop: it stays a scalar
    } while (stop == 0 && ++it < cap);
    // opaque after the loop: otherwise the compiler keeps the loop's compare
    // masks (stop, tb == te) alive past it, at 3 SALU merges per mask per step
    asm volatile("" : "+v"(col), "+v"(stop), "+v"(tb0), "+v"(tb1), "+v"(te), "+v"(mul));
    multi = mul;
    if (stop == 0) cnt.cap_hit++;
    const bool hit = stop != 0 && t < kSentinel;
    // exit axis of the last step (ties x < y < z), as the float masks m_i = 1 on
    // it and 0 off it that place the record's values: m2 = (1 - m0) - m1, exact
    const bool x0 = tb0 == te, x1 = !x0 && tb1 == te;
    const int hax = x0 ? 0 : (x1 ? 1 : 2);
    const float m0 = x0 ? 1.0f : 0.0f, m1 = x1 ? 1.0f : 0.0f, m2 = (1.0f - m0) - m1;
    // G-buffer records as the raster hands them over (render.vert:25-28):
    // v_cellPos = the origin of the greedy quad covering the face (the face
    // axis: its plane), v_fractPos = the hit point minus it, rounded once --
    // p - (c - off) with c the entered cell and off its offset in the quad
    // (a.qface; 0 with VX_FLAG_UNIT_GBUF: the unit cell's split p - c).  Both
    // tables are read before either record is formed.
    int nrec = 0;
    const bool gl = gmark != kGlass;
    // the hit axis's hp (1: the ray goes up it), as the one non-zero product of
    // 0/1 factors (exact), and the normal index 2*axis + hp as an exact small
    // fp32 integer, converted once
    const float hpf = __builtin_fmaf(m0, hp0, __builtin_fmaf(m1, hp1, m2 * hp2));
    const int hnidx = (int)__builtin_fmaf(m2, 4.0f, __builtin_fmaf(m1, 2.0f, hpf));
    const float hr0 = h0 - hp0, hr1 = h1 - hp1, hr2 = h2 - hp2;      // relative cells
    float gq0 = 0.0f, gq1 = 0.0f, gq2 = 0.0f, hq0 = 0.0f, hq1 = 0.0f, hq2 = 0.0f;
    if (QSPEC) {
        // the loaded entry-face word of the recorded step, 10 bits per face axis
        // (all zero with VX_FLAG_UNIT_GBUF: one AND with a scalar, no branch);
        // the glass record's word is taken apart where that record is formed
        qcopy_place(qw & (a.quad_gbuf ? ~0u : 0u), x0 ? 0u : (x1 ? 10u : 20u), m0, m1, m2, hq0, hq1, hq2);
    } else if (a.quad_gbuf) {
        if (gl) {
            const bool gpos = gax == 0 ? p0 : (gax == 1 ? p1 : p2);
            quad_offsets(a, gax, 2 * gax + (gpos ? 1 : 0), (int)(g0h - hp0) + cc0, (int)(g1h - hp1) + cc1,
                         (int)(g2h - hp2) + cc2, gq0, gq1, gq2);
        }
        if (hit) quad_offsets(a, hax, hnidx, (int)hr0 + cc0, (int)hr1 + cc1, (int)hr2 + cc2, hq0, hq1, hq2);
    }
    if (gl) {
        const bool gpos = gax == 0 ? p0 : (gax == 1 ? p1 : p2);
        const float upf = gpos ? 0.0f : 1.0f;
        const float gr0 = g0h - hp0, gr1 = g1h - hp1, gr2 = g2h - hp2;
        if (QSPEC && a.quad_gbuf) qcopy_offsets(gqw, gax, gq0, gq1, gq2);
        const float r0 = gr0 - gq0, r1 = gr1 - gq1, r2 = gr2 - gq2;   // quad origin (exact small integers)
        g0.id = 2;
        g0.color = kGlass;
        g0.nidx = 2 * gax + (gpos ? 1 : 0);
        g0.c0 = (r0 + F.cam_cell_f[0]) + (gax == 0 ? upf : 0.0f);      // exact integers
        g0.c1 = (r1 + F.cam_cell_f[1]) + (gax == 1 ? upf : 0.0f);
        g0.c2 = (r2 + F.cam_cell_f[2]) + (gax == 2 ? upf : 0.0f);
        g0.f0 = gax == 0 ? 0.0f : (o0 + gt * d0) - r0;
        g0.f1 = gax == 1 ? 0.0f : (o1 + gt * d1) - r1;
        g0.f2 = gax == 2 ? 0.0f : (o2 + gt * d2) - r2;
        nrec = 1;
    }
    if (hit) {
        const float upf = 1.0f - hpf;                                  // 1 on a face entered going down its axis
        const float r0 = hr0 - hq0, r1 = hr1 - hq1, r2 = hr2 - hq2;
        const int id = col == kGlass ? 2 : 0;
        const int nidx = hnidx;
        // the face's plane: upf added on the hit axis alone.  upf * m_i is exactly
        // +0 or 1 (both factors are), so the fma rounds (r + cam) + that once, as
        // the select form's add did, with the same +0 off the axis
        const float c0 = __builtin_fmaf(upf, m0, r0 + F.cam_cell_f[0]);
        const float c1 = __builtin_fmaf(upf, m1, r1 + F.cam_cell_f[1]);
        const float c2 = __builtin_fmaf(upf, m2, r2 + F.cam_cell_f[2]);
        // (a select stays here: fma(-v, m, v) would turn v = -0 off the axis into
        // +0, and v is -0 for cam_fract = -0 with te * d = -0, which the host admits)
        const float f0 = x0 ? 0.0f : (o0 + te * d0) - r0;
        const float f1 = x1 ? 0.0f : (o1 + te * d1) - r1;
        const float f2 = (!x0 && !x1) ? 0.0f : (o2 + te * d2) - r2;
        // The record goes behind a glass record if the lane has one.  A wave
        // without any (nearly all: glass is 0.2 % of the headline frame's pixels)
        // writes g0 with no select per field; in the others every lane writes
        // g1, which only a lane with a glass record reads, and a lane without
        // one also g0.  (Values selected, never the reference: stores through a
        // selected reference keep both records in scratch.)
        if (__builtin_expect(__ballot(gl) == 0, 1)) {
            g0.id = id; g0.color = (int)col; g0.nidx = nidx;
            g0.c0 = c0; g0.c1 = c1; g0.c2 = c2;
            g0.f0 = f0; g0.f1 = f1; g0.f2 = f2;
        } else {
            g1.id = id; g1.color = (int)col; g1.nidx = nidx;
            g1.c0 = c0; g1.c1 = c1; g1.c2 = c2;
            g1.f0 = f0; g1.f1 = f1; g1.f2 = f2;
            g0.id = gl ? g0.id : id; g0.color = gl ? g0.color : (int)col; g0.nidx = gl ? g0.nidx : nidx;
            g0.c0 = gl ? g0.c0 : c0; g0.c1 = gl ? g0.c1 : c1; g0.c2 = gl ? g0.c2 : c2;
            g0.f0 = gl ? g0.f0 : f0; g0.f1 = gl ? g0.f1 : f1; g0.f2 = gl ? g0.f2 : f2;
        }
        nrec++;
    }
    t_hit = te;
    return nrec;
}

// ext REFLECT: octant-cube walk of a reflection ray B + o + t*d (B integer,
// 0 <= o < 1, start cell B + c) to the first colour change (oracle walk()
// with glass_layer = 0).  Scalar form of primary(): reflection rays are few.
// Returns 1 and the surface record, or 0 (sky: left the grid, or the start
// cell is outside it).
__device__ __forceinline__ int walk_reflect(const KernelArgs &a, int B0, int B1, int B2, float o0, float o1, float o2, float d0,
                            float d1, float d2, int c0, int c1, int c2, Surf &h, Counters &cnt) {
    // primary()'s stepping on exact fp32 cells relative to B, h = c + hp (hp = 1
    // on a positive axis, d = 0 counting positive), far face A = fma(s, E, h),
    // crossing (A - o) * iv (iv = +inf for d = 0: A - o > 0, so +inf, as the
    // integer form's explicit infinity), exit axis ties x < y < z, next h = A + s
    // on it and med3(floor(o + te*d) + hp, h, A) on the others (= the integer
    // form's clamp of floor(o + te*d) into [c, c+e] or [c-e, c]).  The octant
    // copy's sentinel border (colour 0xFF) marks leaving the grid: no fetch
    // counted, no hit, as the integer form's bounds test.
    const int oct = (d0 < 0.0f ? 1 : 0) | (d1 < 0.0f ? 2 : 0) | (d2 < 0.0f ? 4 : 0);
    const uint32_t *pp = a.prim + (size_t)oct * a.copy_texels;
    float iv0, iv1, iv2;
    ray_rcp(d0, d1, d2, iv0, iv1, iv2);
    const bool p0 = !(d0 < 0.0f), p1 = !(d1 < 0.0f), p2 = !(d2 < 0.0f);
    const float s0 = p0 ? 1.0f : -1.0f, s1 = p1 ? 1.0f : -1.0f, s2 = p2 ? 1.0f : -1.0f;
    const float hp0 = p0 ? 1.0f : 0.0f, hp1 = p1 ? 1.0f : 0.0f, hp2 = p2 ? 1.0f : 0.0f;
    float h0 = (float)c0 + hp0, h1 = (float)c1 + hp1, h2 = (float)c2 + hp2;
    // element index of the padded cell B + pad + h - hp: the x + Xp*y part as the
    // bits of one exact fp32 fma biased by 2^23 (Xp*Yp < 2^23), z by a 24-bit
    // multiply of the biased bits (their low 24 bits are z)
    const float bx = (float)(B0 + a.pad) - hp0 + 8388608.0f, by = (float)(B1 + a.pad) - hp1,
                bz = (float)(B2 + a.pad) - hp2 + 8388608.0f;
    const float fXp = a.Xpf;
    auto fetch = [&]() -> uint32_t {
        const unsigned xy = __float_as_uint(__builtin_fmaf(h1 + by, fXp, h0 + bx)) - 0x4B000000u;
        return pp[xy + __umul24(__float_as_uint(h2 + bz), a.XpYp)];
    };
    uint32_t t = fetch();
    // a direction that is not finite (a hit at t = 0: rayDir = normalize(0) = NaN) is not walked: sky
    // along it with no fetch counted, like a start outside the grid (oracle reflect_color())
    const bool finite = fabsf(d0) < kInf && fabsf(d1) < kInf && fabsf(d2) < kInf;
    if (t >= kSentinel || !finite) return 0;
    cnt.refl_fetch++;
    int prev = t & 0xff;
    float E0 = cvt_f32_ubyte1(t), E1 = cvt_f32_ubyte2(t), E2 = cvt_f32_ubyte3(t);
    const int cap = 4 * (a.X + a.Y + a.Z);
    for (int it = 0; it < cap; it++) {
        const float A0 = __builtin_fmaf(s0, E0, h0), A1 = __builtin_fmaf(s1, E1, h1), A2 = __builtin_fmaf(s2, E2, h2);
        const float tb0 = (A0 - o0) * iv0, tb1 = (A1 - o1) * iv1, tb2 = (A2 - o2) * iv2;
        const float te = __builtin_fminf(__builtin_fminf(tb0, tb1), tb2);
        const bool e0 = tb0 == te;
        const bool e1 = !e0 && tb1 == te;
        const int ax = e0 ? 0 : (e1 ? 1 : 2);
        h0 = e0 ? A0 + s0 : __builtin_amdgcn_fmed3f(floorf(o0 + te * d0) + hp0, h0, A0);
        h1 = e1 ? A1 + s1 : __builtin_amdgcn_fmed3f(floorf(o1 + te * d1) + hp1, h1, A1);
        h2 = (!e0 && !e1) ? A2 + s2 : __builtin_amdgcn_fmed3f(floorf(o2 + te * d2) + hp2, h2, A2);
        t = fetch();
        if (t >= kSentinel) return 0;
        cnt.refl_fetch++;
        const int col = t & 0xff;
        E0 = cvt_f32_ubyte1(t); E1 = cvt_f32_ubyte2(t); E2 = cvt_f32_ubyte3(t);
        if (col != prev && col != 0) {                 // entering a meshed cell (air never is)
            const bool pos = ax == 0 ? p0 : (ax == 1 ? p1 : p2);
            const float r0 = h0 - hp0, r1 = h1 - hp1, r2 = h2 - hp2;   // relative cells (exact)
            h.color = col;
            h.id = col == kGlass ? 2 : 0;
            h.nidx = 2 * ax + (pos ? 1 : 0);
            h.c0 = ((float)B0 + r0) + (ax == 0 && !pos ? 1.0f : 0.0f);
            h.c1 = ((float)B1 + r1) + (ax == 1 && !pos ? 1.0f : 0.0f);
            h.c2 = ((float)B2 + r2) + (ax == 2 && !pos ? 1.0f : 0.0f);
            h.f0 = ax == 0 ? 0.0f : (o0 + te * d0) - r0;
            h.f1 = ax == 1 ? 0.0f : (o1 + te * d1) - r1;
            h.f2 = ax == 2 ? 0.0f : (o2 + te * d2) - r2;
            return 1;
        }
        prev = col;
    }
    cnt.cap_hit++;
    return 0;
}

// ---------------- glass in draw order (VX_FLAG_GLASS_ORDER) ----------------
// The reference draws the glass quads after every opaque one, in vertex.bin
// order, with depth test LESS and depth writes on, blending SRC_ALPHA
// (render.js:82-91, sdf.cpp:284,337).  face_key is that order for a glass
// face (oracle vxo_face_order): forChunkXYZ chunk, axis d, normal, slice, quad
// origin row j, column i; a face on an interior chunk plane is emitted first
// by the lower chunk (its slice CH-1).
__device__ __forceinline__ unsigned long long face_key(const KernelArgs &a, int x, int y, int z, int nidx,
                                                       unsigned q) {
    const int CH = a.chunk;
    const int d = nidx >> 1, normal = nidx & 1;
    const int cd_ = d == 0 ? x : (d == 1 ? y : z);                  // cell along d, u, v
    const int cu = d == 0 ? y : (d == 1 ? z : x);
    const int cv = d == 0 ? z : (d == 1 ? x : y);
    const int plane = cd_ + (normal ? 0 : 1);
    int kd = plane / CH, pd = plane % CH - 1;
    if (pd < 0) { kd -= 1; pd = CH - 1; }
    const int ou = cu - (int)(q & 0xffu), ov = cv - (int)(q >> 8);
    const int ku = ou / CH, kv = ov / CH;
    const int kx = d == 0 ? kd : (d == 1 ? kv : ku);
    const int ky = d == 1 ? kd : (d == 2 ? kv : ku);
    const int kz = d == 2 ? kd : (d == 0 ? kv : ku);
    const unsigned long long ny = (unsigned long long)((a.Y + CH - 1) / CH), nz = (unsigned long long)((a.Z + CH - 1) / CH);
    const unsigned long long S = (unsigned long long)CH + 1;
    const unsigned long long chunk = ((unsigned long long)kx * ny + (unsigned long long)ky) * nz + (unsigned long long)kz;
    return ((((chunk * 3 + (unsigned long long)d) * 2 + (unsigned long long)normal) * S + (unsigned long long)(pd + 1)) * S +
            (unsigned long long)(ov - kv * CH)) * S + (unsigned long long)(ou - ku * CH);
}

// One pass over the view ray's glass faces (the walk of primary visibility in
// the oracle's integer form, not the fp32 step of primary / walk_reflect: a cold
// path compiled into every timed kernel, whose register footprint sets EXT 0's
// scratch size; oracle walk() with glass_layer 3): of the
// front-facing glass entries before the first opaque entry, the one drawn
// first after key `klast` (none: have_last false) among those nearer than
// tmax.  Returns false if there is none; else its G-buffer record
// (quad-relative unless a.quad_gbuf is 0), depth and key, and whether it is
// the ray's nearest pane.  No storage per pane, so a pixel blends every pane
// its ray crosses, as the raster does.  Its fetches repeat the primary walk's
// and are not counted again.
__device__ __forceinline__ bool glass_scan(const KernelArgs &a, float d0, float d1, float d2, bool have_last,
                                           unsigned long long klast, float tmax, Surf &h, float &t_out,
                                           unsigned long long &k_out, bool &nearest,
                                           const RayOrigin *org = nullptr) {
    const FrameConsts &F = a.fc;
    // org: the ray's own origin (k_ortho) in the camera's place, its slabs by frame_consts' expressions
    const float o0 = org ? org->o0 : F.cam_fract[0], o1 = org ? org->o1 : F.cam_fract[1],
                o2 = org ? org->o2 : F.cam_fract[2];
    const int cc0 = org ? org->cc0 : F.cam_cell[0], cc1 = org ? org->cc1 : F.cam_cell[1],
              cc2 = org ? org->cc2 : F.cam_cell[2];
    const float iv0 = d0 != 0.0f ? 1.0f / d0 : 0.0f, iv1 = d1 != 0.0f ? 1.0f / d1 : 0.0f,
                iv2 = d2 != 0.0f ? 1.0f / d2 : 0.0f;
    float tlo = 0.0f, thi = kInf;
    bool miss = false;
    // (the origin's slab bounds in a lambda of their own, called only where org is given: written into
    // slab's body they changed every frame kernel's code, tools/isa_diff.py)
    auto org_slab = [&](int i, int edge) {
        const int cc = i == 0 ? cc0 : (i == 1 ? cc1 : cc2);
        return (float)(edge - cc) - (i == 0 ? o0 : (i == 1 ? o1 : o2));
    };
    auto slab = [&](float d, float iv, int i) {
        const float lo = org ? org_slab(i, 0) : F.slab_lo[i],
                    hi = org ? org_slab(i, i == 0 ? a.X : (i == 1 ? a.Y : a.Z)) : F.slab_hi[i];
        if (d != 0.0f) {
            float t0 = lo * iv, t1 = hi * iv;
            if (t0 > t1) { const float tt = t0; t0 = t1; t1 = tt; }
            tlo = gmax(tlo, t0);
            thi = gmin(thi, t1);
        } else if (!(lo <= 0.0f && 0.0f < hi)) {
            miss = true;
        }
    };
    slab(d0, iv0, 0); slab(d1, iv1, 1); slab(d2, iv2, 2);
    if (miss || !(tlo < thi)) return false;
    auto entry = [&](float o, float d, int cc, int dim) {
        const int c = f2i(floorf(o + tlo * d));
        return min(max(c, -cc), dim - cc - 1);
    };
    int c0 = entry(o0, d0, cc0, a.X), c1 = entry(o1, d1, cc1, a.Y), c2 = entry(o2, d2, cc2, a.Z);
    const int oct = (d0 < 0.0f ? 1 : 0) | (d1 < 0.0f ? 2 : 0) | (d2 < 0.0f ? 4 : 0);
    const uint32_t *pp = a.prim + (size_t)oct * a.copy_texels;
    auto fetch = [&](int x, int y, int z) -> uint32_t {
        return pp[(unsigned)(x + a.pad) + (unsigned)a.Xp * (unsigned)(y + a.pad) + a.XpYp * (unsigned)(z + a.pad)];
    };
    const int st0 = d0 > 0.0f ? 1 : -1, st1 = d1 > 0.0f ? 1 : -1, st2 = d2 > 0.0f ? 1 : -1;
    uint32_t t = fetch(c0 + cc0, c1 + cc1, c2 + cc2);
    int prev = t & 0xff, e0 = (int)((t >> 8) & 0xff), e1 = (int)((t >> 16) & 0xff), e2 = (int)(t >> 24);
    bool found = false, bfirst = false, first = true;
    int bx = 0, by = 0, bz = 0, bax = 0, bst = 0;
    unsigned bq = 0;
    float bt = 0.0f;
    unsigned long long bk = 0;
    const int cap = 4 * (a.X + a.Y + a.Z);
    for (int it = 0; it < cap; it++) {
        const float tb0 = d0 != 0.0f ? ((float)(c0 + (st0 > 0 ? e0 + 1 : -e0)) - o0) * iv0 : kInf;
        const float tb1 = d1 != 0.0f ? ((float)(c1 + (st1 > 0 ? e1 + 1 : -e1)) - o1) * iv1 : kInf;
        const float tb2 = d2 != 0.0f ? ((float)(c2 + (st2 > 0 ? e2 + 1 : -e2)) - o2) * iv2 : kInf;
        const int ax = (tb0 <= tb1 && tb0 <= tb2) ? 0 : (tb1 <= tb2 ? 1 : 2);
        const float te = ax == 0 ? tb0 : (ax == 1 ? tb1 : tb2);
        // the walk's crossings never decrease, and a pane qualifies only nearer
        // than tmax: past it no later entry can, so the scan ends there (each
        // scan of the chain walks only up to the last surface written)
        if (!(te < tmax)) break;
        auto side = [&](int c, float o, float d, int e) {
            const int v = f2i(floorf(o + te * d));
            const int lo = d < 0.0f ? c - e : c, hi = d < 0.0f ? c : c + e;
            return v < lo ? lo : (v > hi ? hi : v);
        };
        const int n0 = ax == 0 ? c0 + st0 * (e0 + 1) : side(c0, o0, d0, e0);
        const int n1 = ax == 1 ? c1 + st1 * (e1 + 1) : side(c1, o1, d1, e1);
        const int n2 = ax == 2 ? c2 + st2 * (e2 + 1) : side(c2, o2, d2, e2);
        c0 = n0; c1 = n1; c2 = n2;
        const int x = c0 + cc0, y = c1 + cc1, z = c2 + cc2;
        if ((unsigned)x >= (unsigned)a.X || (unsigned)y >= (unsigned)a.Y || (unsigned)z >= (unsigned)a.Z) break;
        t = fetch(x, y, z);
        const int col = t & 0xff;
        e0 = (int)((t >> 8) & 0xff); e1 = (int)((t >> 16) & 0xff); e2 = (int)(t >> 24);
        if (col != prev && col != 0) {             // a front face
            if (col != kGlass) break;              // the opaque surface: no glass behind it is drawn
            const int stp = ax == 0 ? st0 : (ax == 1 ? st1 : st2);
            const int nidx = 2 * ax + (stp > 0 ? 1 : 0);
            unsigned q = a.qface[(size_t)nidx * a.XYZ + lin_index(a, x, y, z)];
            q = q == 0xFFFFu ? 0u : q;
            const unsigned long long k = face_key(a, x, y, z, nidx, q);
            if ((!have_last || k > klast) && te < tmax && (!found || k < bk)) {
                found = true;
                bfirst = first;
                bk = k; bt = te; bq = q; bax = ax; bst = stp;
                bx = c0; by = c1; bz = c2;
            }
            first = false;
        }
        prev = col;
    }
    if (!found) return false;
    // the record (primary()'s rule): face axis on its plane, the others quad-relative
    unsigned q = a.quad_gbuf ? bq : 0u;
    const int lo = (int)(q & 0xffu), hi = (int)(q >> 8);
    const int of0 = bax == 2 ? lo : (bax == 1 ? hi : 0);
    const int of1 = bax == 0 ? lo : (bax == 2 ? hi : 0);
    const int of2 = bax == 1 ? lo : (bax == 0 ? hi : 0);
    const int up = bst > 0 ? 0 : 1;
    h.id = 2;
    h.color = kGlass;
    h.nidx = 2 * bax + (bst > 0 ? 1 : 0);
    h.c0 = (float)(bx - of0 + cc0 + (bax == 0 ? up : 0));
    h.c1 = (float)(by - of1 + cc1 + (bax == 1 ? up : 0));
    h.c2 = (float)(bz - of2 + cc2 + (bax == 2 ? up : 0));
    h.f0 = bax == 0 ? 0.0f : (o0 + bt * d0) - (float)(bx - of0);
    h.f1 = bax == 1 ? 0.0f : (o1 + bt * d1) - (float)(by - of1);
    h.f2 = bax == 2 ? 0.0f : (o2 + bt * d2) - (float)(bz - of2);
    t_out = bt;
    k_out = bk;
    nearest = bfirst;
    return true;
}

}  // namespace
}  // namespace vx
