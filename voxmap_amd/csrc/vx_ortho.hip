// vx_ortho.hip — orthographic frames (vx_render_ortho): every pixel's ray has
// the frame's one direction ray_fwd and an origin of its own on the image
// plane, camera + nx * ray_right + ny * ray_up.  A translation unit of its own:
// kernel_meta.check() budgets every kernel whose name holds k_render, and this
// one shares with them the device helpers only (the stage headers below).
//
// The definition (include/voxmap.h): pixel (x, y) is the one pixel of the 1 x 1
// frame vx_render makes of the same parameters with the camera at that pixel's
// origin and ray_right = ray_up = 0.  So per lane: the origin by
// vx_pixel_ray_ortho's fp32 formula; the primary walk in k_query's form from it
// (grid slabs of the origin, entry cell clamped into the grid, box-exit steps on
// exact fp32 cells relative to the origin cell, biased fp32 index with a
// per-lane base), recording as primary() does the first glass entry, a second
// one (multi) and the first opaque entry, with primary()'s quad-relative split
// (a.qface; the unit cell's with VX_FLAG_UNIT_GBUF); then k_render's one-blend
// shading through shade_block<1> (rayDir given: the fragment minus the lane's
// origin), reflect_color<1>, glass_chain<1> and shade_sky with the lane's
// RayOrigin in the camera's place.  Lane = pixel, wave = 8 x 8 tile, as k_render.
// What the whole frame shares comes from the host (OrthoArgs): the direction,
// RN(1/d), the axis signs, the octant copy, whether |d| is in normalize's fast range.
//
// Every index formed lies inside its array, for every frame vx_render_ortho's
// checks let through (|origin cell| < 2^22, 0 <= fract < 1, a finite non-zero
// direction):
//   the walk, as vx_query.hip: the entry cell is clamped into the grid, a
//   fetched cell that is not the sentinel lies in the grid, and one step leaves
//   such a cell c for A + s on the exit axis (|A + s - c| = E + 1 <= cap, the
//   extents being <= cap - 1) and for a cell of [c, A] on the others (med3
//   returns one of its bounds even for a NaN first operand): at most cap cells
//   outside the grid on any axis, and the border is pad = cap cells wide.  A
//   border cell is the sentinel and ends the walk; the iteration cap, 4 * (X +
//   Y + Z), ends anything else.
//   a.qface is read at a recorded cell: one that was fetched and was no sentinel.
//   the sun march and the AO sample start from a record's fragment, which lies
//   on a face of a grid cell, as in k_render: the march returns before reading
//   outside the padded channel and the AO sample clamps; glass_scan tests the
//   grid's bounds before each fetch; the mirror walk is walk_reflect's own.
//   the noise lookups wrap.
// A lane off the frame (a partial edge tile, or a row past the launch's range)
// neither loads nor stores: it only takes part in the counters' wave sums.
#include "vx_math.h"
#include "vx_loads.h"
#include "vx_march.h"
#include "vx_walk.h"
#include "vx_sample.h"
#include "vx_shade.h"
#include "vx_pixel.h"

namespace vx {
namespace {

// The primary walk of one orthographic ray: primary()'s results (0 sky, 1
// surface, 2 glass + what is behind; g0 the first record, g1 the second;
// t_hit the last crossing; multi: a second pane in front of the surface) by
// k_query's stepping from the lane's origin L.
__device__ __forceinline__ int ortho_primary(const OrthoArgs &oa, const RayOrigin &L, Surf &g0, Surf &g1, Counters &cnt,
                                             float &t_hit, int &multi) {
    const KernelArgs &a = oa.k;
    const float d0 = oa.d[0], d1 = oa.d[1], d2 = oa.d[2];
    const float iv0 = oa.iv[0], iv1 = oa.iv[1], iv2 = oa.iv[2];
    const float hp0 = oa.hp[0], hp1 = oa.hp[1], hp2 = oa.hp[2];
    const float s0 = oa.sg[0], s1 = oa.sg[1], s2 = oa.sg[2];
    const float o0 = L.o0, o1 = L.o1, o2 = L.o2;
    const int B0 = L.cc0, B1 = L.cc1, B2 = L.cc2;
    multi = 0;
    t_hit = 0.0f;
    // grid slabs from the lane's origin (frame_consts' slab_lo / slab_hi of the 1 x 1
    // frame); a zero component misses unless the origin lies inside that slab
    float tlo = 0.0f, thi = kInf;
    bool miss = false;
#define VX_SLAB(D, IV, B, O, DIM)                                         \
    {                                                                     \
        const float lo = (float)(0 - B) - O, hi = (float)(DIM - B) - O;   \
        const float t0 = lo * IV, t1 = hi * IV;                           \
        const bool sw = t0 > t1, nz = D != 0.0f;                          \
        tlo = nz ? gmax(tlo, sw ? t1 : t0) : tlo;                         \
        thi = nz ? gmin(thi, sw ? t0 : t1) : thi;                         \
        miss |= !nz && !(lo <= 0.0f && 0.0f < hi);                        \
    }
    VX_SLAB(d0, iv0, B0, o0, a.X)
    VX_SLAB(d1, iv1, B1, o1, a.Y)
    VX_SLAB(d2, iv2, B2, o2, a.Z)
#undef VX_SLAB
    if (miss || !(tlo < thi)) return 0;
    // entry cell relative to the origin cell, as exact fp32 integers, clamped into the grid
    const float cf0 = __builtin_amdgcn_fmed3f(floorf(o0 + tlo * d0), (float)(-B0), (float)(a.X - B0 - 1));
    const float cf1 = __builtin_amdgcn_fmed3f(floorf(o1 + tlo * d1), (float)(-B1), (float)(a.Y - B1 - 1));
    const float cf2 = __builtin_amdgcn_fmed3f(floorf(o2 + tlo * d2), (float)(-B2), (float)(a.Z - B2 - 1));
    float h0 = cf0 + hp0, h1 = cf1 + hp1, h2 = cf2 + hp2;
    // element index of the padded cell B + pad + h - hp in the frame's octant copy, as
    // k_query forms it (Xp*Yp < 2^23, |B| < 2^22)
    const uint32_t *pp = a.prim + (size_t)oa.oct * a.copy_texels;
    const float bx = (float)(B0 + a.pad) - hp0 + 8388608.0f, by = (float)(B1 + a.pad) - hp1,
                bz = (float)(B2 + a.pad) - hp2 + 8388608.0f;
    const float fXp = a.Xpf;
    auto fetch = [&]() -> uint32_t {
        const unsigned xy = __float_as_uint(__builtin_fmaf(h1 + by, fXp, h0 + bx)) - 0x4B000000u;
        return pp[xy + __umul24(__float_as_uint(h2 + bz), a.XpYp)];
    };
    uint32_t t = fetch();                          // in the grid by the clamp: never the sentinel
    cnt.prim_fetch++;
    cnt.prim_witers += once_per_wave(1u);
    int prev = t & 0xff;
    float E0 = cvt_f32_ubyte1(t), E1 = cvt_f32_ubyte2(t), E2 = cvt_f32_ubyte3(t);
    bool gl = false, hit = false;
    float g0h = 0.0f, g1h = 0.0f, g2h = 0.0f, gt = 0.0f, te = 0.0f;
    int gax = 0, hax = 0, col = 0;
    const int cap = 4 * (a.X + a.Y + a.Z);
    int it = 0;
    for (; it < cap; it++) {
        const float A0 = __builtin_fmaf(s0, E0, h0), A1 = __builtin_fmaf(s1, E1, h1), A2 = __builtin_fmaf(s2, E2, h2);
        const float tb0 = (A0 - o0) * iv0, tb1 = (A1 - o1) * iv1, tb2 = (A2 - o2) * iv2;
        te = __builtin_fminf(__builtin_fminf(tb0, tb1), tb2);
        const bool e0 = tb0 == te;
        const bool e1 = !e0 && tb1 == te;
        hax = e0 ? 0 : (e1 ? 1 : 2);
        h0 = e0 ? A0 + s0 : __builtin_amdgcn_fmed3f(floorf(o0 + te * d0) + hp0, h0, A0);
        h1 = e1 ? A1 + s1 : __builtin_amdgcn_fmed3f(floorf(o1 + te * d1) + hp1, h1, A1);
        h2 = (!e0 && !e1) ? A2 + s2 : __builtin_amdgcn_fmed3f(floorf(o2 + te * d2) + hp2, h2, A2);
        t = fetch();
        cnt.prim_witers += once_per_wave(1u);
        if (t >= kSentinel) break;                 // left the grid: no fetch counted, no surface
        cnt.prim_fetch++;
        col = t & 0xff;
        E0 = cvt_f32_ubyte1(t); E1 = cvt_f32_ubyte2(t); E2 = cvt_f32_ubyte3(t);
        // a face of the mesh: entering a meshed cell from a cell of another colour
        if (col != prev && col != 0) {
            if (col != kGlass) {
                hit = true;
                break;
            }
            if (!gl) {                             // the first glass entry: recorded, the walk goes on
                gl = true;
                g0h = h0; g1h = h1; g2h = h2; gt = te; gax = hax;
            } else {
                multi = 1;                         // a second pane in front of the surface
            }
        }
        prev = col;
    }
    if (it >= cap) cnt.cap_hit++;
    // The records, as primary() forms them: v_cellPos = the origin of the greedy quad
    // covering the face (the face axis: its plane), v_fractPos = the hit point minus it,
    // rounded once; q = the entered cell + hp
    const float ccf0 = (float)B0, ccf1 = (float)B1, ccf2 = (float)B2;      // exact: |B| < 2^22
    auto record = [&](Surf &s, int color, int ax, float q0, float q1, float q2, float tt) {
        const bool pos = (ax == 0 ? hp0 : (ax == 1 ? hp1 : hp2)) != 0.0f;
        const float upf = pos ? 0.0f : 1.0f;
        const int nidx = 2 * ax + (pos ? 1 : 0);
        const float c0 = q0 - hp0, c1 = q1 - hp1, c2 = q2 - hp2;          // the entered cell, relative (exact)
        float f0 = 0.0f, f1 = 0.0f, f2 = 0.0f;
        if (a.quad_gbuf) quad_offsets(a, ax, nidx, B0 + (int)c0, B1 + (int)c1, B2 + (int)c2, f0, f1, f2);
        const float r0 = c0 - f0, r1 = c1 - f1, r2 = c2 - f2;             // quad origin (exact small integers)
        s.id = color == kGlass ? 2 : 0;
        s.color = color;
        s.nidx = nidx;
        s.c0 = (r0 + ccf0) + (ax == 0 ? upf : 0.0f);
        s.c1 = (r1 + ccf1) + (ax == 1 ? upf : 0.0f);
        s.c2 = (r2 + ccf2) + (ax == 2 ? upf : 0.0f);
        s.f0 = ax == 0 ? 0.0f : (o0 + tt * d0) - r0;
        s.f1 = ax == 1 ? 0.0f : (o1 + tt * d1) - r1;
        s.f2 = ax == 2 ? 0.0f : (o2 + tt * d2) - r2;
    };
    int nrec = 0;
    if (gl) {
        record(g0, kGlass, gax, g0h, g1h, g2h, gt);
        nrec = 1;
    }
    if (hit) {
        if (gl) record(g1, col, hax, h0, h1, h2, te);
        else record(g0, col, hax, h0, h1, h2, te);
        nrec++;
    }
    t_hit = te;
    return nrec;
}

template <int FMT, bool STATS>
__global__ __launch_bounds__(kWG) void k_ortho(const OrthoArgs oa) {
    const KernelArgs &a = oa.k;
    const FrameConsts &F = a.fc;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lx = ((wave % kWX) << 3) | (lane & 7);
    const int ly = ((wave / kWX) << 3) | (lane >> 3);
    const int px = (int)(blockIdx.x << kBXS) + lx;
    const int ry = (int)(blockIdx.y << kBYS) + ly;     // the row within the launch's range: where it is written
    const int py = oa.row0 + ry;                       // the row of the frame: what it shows
    const bool inframe = px < a.w && ry < oa.rows;
    Counters cnt = {};
    unsigned n_sky = 0, n_block = 0, n_glass = 0, n_px = 0;
    if (inframe) {
        // the pixel's origin (vx_pixel_ray_ortho): nx, ny as view_ray's, then per axis
        // s = cam_fract + (nx * right + ny * up), cell = cam_cell + floor(s), fract = s - floor(s)
        // clamped below 1 (s - floor(s) rounds to 1 for a tiny negative s)
        const float nx = div_const((float)(2 * px + 1), F.fw, F.rcp_w) - 1.0f;
        const float ny = 1.0f - div_const((float)(2 * py + 1), F.fh, F.rcp_h);
        RayOrigin L;
        {
            const float s0 = F.cam_fract[0] + ((nx * F.right[0]) + (ny * F.up[0]));
            const float s1 = F.cam_fract[1] + ((nx * F.right[1]) + (ny * F.up[1]));
            const float s2 = F.cam_fract[2] + ((nx * F.right[2]) + (ny * F.up[2]));
            const float fl0 = floorf(s0), fl1 = floorf(s1), fl2 = floorf(s2);
            L.cc0 = F.cam_cell[0] + (int)fl0; L.cc1 = F.cam_cell[1] + (int)fl1; L.cc2 = F.cam_cell[2] + (int)fl2;
            L.o0 = __builtin_fminf(s0 - fl0, 0x1.fffffep-1f);
            L.o1 = __builtin_fminf(s1 - fl1, 0x1.fffffep-1f);
            L.o2 = __builtin_fminf(s2 - fl2, 0x1.fffffep-1f);
            // the sky's offset of the pixel's own 1 x 1 frame (frame_consts' skyOff)
            L.sky0 = 1e-4f * ((float)L.cc0 + L.o0);
            L.sky1 = 1e-4f * ((float)L.cc1 + L.o1);
        }
        const float d0 = oa.d[0], d1 = oa.d[1], d2 = oa.d[2];
        Surf g[2];
        float t_hit;
        int multi;
        const int n = ortho_primary(oa, L, g[0], g[1], cnt, t_hit, multi);
        const bool stacked = multi != 0 && !(F.flags & (VX_FLAG_GLASS_SINGLE | VX_FLAG_PRIMARY_ONLY));
        float rgba[4];
        if (F.flags & VX_FLAG_PRIMARY_ONLY) {
            primary_only_colour(n, g[0], rgba);
            n_sky = n == 0;
            n_glass = n != 0 && g[0].id == 2;
            n_block = n != 0 && g[0].id != 2;
        } else if (n == 0) {
            n_sky = 1;
            shade_sky(a, d0, d1, d2, rgba, cnt, oa.ranged != 0, &L);
        } else {
            // k_render's one-blend path: what a pane blends over is shaded first
            float dst[4], r0, r1, r2;
            if (g[0].id == 2) {
                if (n == 2) {
                    origin_ray(L, g[1], r0, r1, r2);
                    shade_block<1>(a, g[1], dst, cnt, true, r0, r1, r2);
                } else {
                    shade_sky(a, d0, d1, d2, dst, cnt, oa.ranged != 0, &L);
                }
                if (__builtin_expect(__ballot(stacked) != 0, 0) && stacked)
                    glass_chain<1>(a, d0, d1, d2, dst, n == 2 ? t_hit : kInf, cnt, &L);
            }
            origin_ray(L, g[0], r0, r1, r2);
            shade_block<1>(a, g[0], rgba, cnt, true, r0, r1, r2);
            if (g[0].id == 2) {
                n_glass = 1;
                if (F.flags & VX_FLAG_REFLECT) {
                    const float rd[3] = {r0, r1, r2};
                    float refl[3];
                    reflect_color<1>(a, g[0], rd, refl, cnt, &L);
                    const int ax = g[0].nidx >> 1;
                    const float cs = gmin(fabsf(ax == 0 ? rd[0] : (ax == 1 ? rd[1] : rd[2])), 1.0f);
                    const float x = 1.0f - cs, x2 = x * x;
                    const float fr = 0.04f + 0.96f * ((x2 * x2) * x);
#pragma unroll
                    for (int i = 0; i < 3; i++) rgba[i] = rgba[i] + fr * refl[i];
                }
                blend_canvas(rgba, dst, rgba);      // the nearest pane over the canvas
            } else {
                n_block = 1;
            }
        }
        rgba[3] = 1.0f;
        if constexpr (FMT == VX_PIXEL_RGBA8)
            store_rgba8_frame(a, px, ry, rgba);
        else
            store_pixel<FMT>(a, (size_t)ry * a.w + px, rgba);
        n_px = 1;
    }
    if (STATS) flush_counters(a, cnt, n_px, n_sky, n_block, n_glass);
}

}  // namespace

int launch_ortho(const OrthoArgs &a, int fmt, void *stream) {
    const hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)((a.k.w + kBX - 1) / kBX), (unsigned)((a.rows + kBY - 1) / kBY));
    launch_variant(fmt, a.k.stats != nullptr, false, [&](auto F, auto S, auto) {
        hipLaunchKernelGGL((k_ortho<F(), S()>), grid, dim3(kWG), 0, s, a);
    });
    int rc = (int)hipGetLastError();
    if (!rc && a.k.stats) rc = launch_reduce_stats(a.k.stats, stream);
    return rc;
}

}  // namespace vx
