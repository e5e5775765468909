// vx_pixel.h — a pixel's way in and out of a render kernel: the block shape,
// the view ray, packing and stores, the primary-only colour, the counters'
// flush, the host's (format, stats, tiled) launch ladder, and the 2D mode's
// shading (k_render_2d, vx_dispatch.hip).  Shared by k_render (vx_render.h)
// and the dispatch unit, which does not include k_render.
#pragma once
#include <type_traits>
#include "vx_loads.h"
#include "vx_math.h"
#include "vx_sample.h"

namespace vx {
namespace {

// Workgroup = 256 threads = four 8x8-pixel waves side by side: a 32x8 pixel
// block.  Each wave stores its own 8x8 tile (32-B row pieces): staging the
// block in LDS for whole 128-B rows needs a block barrier, and the waves of a
// block finish at very different times (round 5: per-wave stores C3 full
// quality -1.7 %, v1 -1.1 %, C5 -0.5..-1.2 %, profiles/r05_ab_wave_store_*.txt).
constexpr int kBX = 32;                    // block width in pixels
constexpr int kBY = kWG / kBX;             // block height
constexpr int kBXS = 5;                    // log2(kBX)
constexpr int kBYS = 3;                    // log2(kBY)
constexpr int kWX = kBX / 8;               // waves per block row
static_assert(kBX == 1 << kBXS && kBY == 1 << kBYS, "block shape");

__device__ __forceinline__ uint32_t pack_rgba8(const float rgba[4]) {
    uint32_t pk = 0;
#pragma unroll
    // clamp01 for gclamp(x, 0, 1): the value only feeds * 255 + 0.5 and the
    // truncating convert, so the two cases where the forms differ give one
    // byte: -0 and +0 both 0.5 -> 0; a NaN stays NaN through the select form and
    // converts to 0, and clamps to 0 (every float: profiles/r07_clamp_check.txt)
    for (int i = 0; i < 4; i++) pk |= (uint32_t)(clamp01(rgba[i]) * 255.0f + 0.5f) << (8 * i);
    return pk;
}

template <int FMT>
__device__ __forceinline__ void store_pixel(const KernelArgs &a, size_t idx, const float rgba[4]) {
    if (FMT == VX_PIXEL_RGBA32F)
        reinterpret_cast<float4 *>(a.out)[idx] = make_float4(rgba[0], rgba[1], rgba[2], rgba[3]);
    else
        reinterpret_cast<uint32_t *>(a.out)[idx] = pack_rgba8(rgba);
}
// The RGBA8 pixel of an untiled frame at a 32-bit byte offset from a.out (the
// saddr form, as ld_off: no 64-bit multiply-add and shifts per pixel): a frame
// is at most 32768 x 32768 pixels (check_frame), so 4 * (py * w + px) <= 2^32 - 4.
__device__ __forceinline__ void store_rgba8_frame(const KernelArgs &a, int px, int py, const float rgba[4]) {
    const unsigned off = ((unsigned)py * (unsigned)a.w + (unsigned)px) << 2;
    *reinterpret_cast<uint32_t *>(reinterpret_cast<char *>(a.out) + off) = pack_rgba8(rgba);
}

// output index of pixel (px, py), at (x, y) inside tile k of a tiled launch:
// compact tile-major (tile k at k * tile_h * pitch, rows pitch apart) or,
// tile_inplace, the pixel's own place in the w-wide frame
template <bool TILED>
__device__ __forceinline__ size_t out_index(const KernelArgs &a, int k, int x, int y, int px, int py) {
    if (TILED && !a.tile_inplace) return (size_t)k * a.tile_h * a.tile_pitch + (size_t)y * a.tile_pitch + x;
    return (size_t)py * a.w + px;
}

// view ray of pixel (px, py): nx = (2px+1)/w - 1, ny = 1 - (2py+1)/h with exact quotients
// (FC: FrameConsts, or GbufArgs, which carries the same seven constants under the same names)
template <class FC>
__device__ __forceinline__ void view_ray(const FC &F, int px, int py, float &d0, float &d1, float &d2) {
    const float nx = div_const((float)(2 * px + 1), F.fw, F.rcp_w) - 1.0f;
    const float ny = 1.0f - div_const((float)(2 * py + 1), F.fh, F.rcp_h);
    d0 = (F.fwd[0] + nx * F.right[0]) + ny * F.up[0];
    d1 = (F.fwd[1] + nx * F.right[1]) + ny * F.up[1];
    d2 = (F.fwd[2] + nx * F.right[2]) + ny * F.up[2];
}

__device__ __forceinline__ void primary_only_colour(int n, const Surf &g0, float rgba[4]) {
    const int pc = n == 0 ? 0 : g0.color;
    palette(pc, rgba[0], rgba[1], rgba[2]);
    rgba[3] = 1.0f;
}

// The counters' way out of a STATS kernel (k_render, k_render_2d): each wave
// sums a pixel's counters and the four pixel counts over its lanes, and lane 0
// adds the sums that are not zero to the block's row of a.stats
// (k_reduce_stats, vx_dispatch.hip, then sums the rows).
__device__ __forceinline__ void flush_counters(const KernelArgs &a, const Counters &cnt, unsigned n_px, unsigned n_sky,
                                               unsigned n_block, unsigned n_glass) {
    unsigned long long v[ST_COUNT];
    v[ST_PIXELS] = wave_sum(n_px);
    v[ST_SKY] = wave_sum(n_sky);
    v[ST_BLOCK] = wave_sum(n_block);
    v[ST_GLASS] = wave_sum(n_glass);
    v[ST_PRIM_FETCH] = wave_sum(cnt.prim_fetch);
    v[ST_SHADOW_RAYS] = wave_sum(cnt.shadow_rays);
    v[ST_SHADOW_FETCH] = wave_sum(cnt.shadow_fetch);
    v[ST_AO] = wave_sum(cnt.ao);
    v[ST_NOISE_PX] = wave_sum(cnt.noise_px);
    v[ST_CAP_HITS] = wave_sum(cnt.cap_hit);
    v[ST_REFL_RAYS] = wave_sum(cnt.refl_rays);
    v[ST_REFL_FETCH] = wave_sum(cnt.refl_fetch);
    v[ST_ROUGH] = wave_sum(cnt.rough);
    v[ST_PRIM_WITERS] = wave_sum(cnt.prim_witers);
    v[ST_MARCH_WITERS] = wave_sum(cnt.march_witers);
    v[ST_MARCH_SLOTS] = wave_sum(cnt.march_slots);
    v[ST_SHADOW_RESOLVED] = wave_sum(cnt.shadow_resolved);
    if ((threadIdx.x & 63) == 0) {
        // spread the adds over 64 slot rows to avoid one hot line per counter
        unsigned long long *row = a.stats + (size_t)((blockIdx.x + blockIdx.y * 7) & 63) * ST_COUNT;
#pragma unroll
        for (int i = 0; i < ST_COUNT; i++)
            if (v[i]) atomicAdd(row + i, v[i]);
    }
}

// A launch's (pixel format, stats, tiled) as template arguments: calls
// f(FMT, STATS, TILED) with three std::integral_constant values (FMT an int,
// VX_PIXEL_*; the other two bools), so the caller writes its kernel once:
//   launch_variant(fmt, st, tiled, [&](auto F, auto S, auto T) { ... k<F(), S(), T()> ... });
template <typename Fn>
void launch_variant(int fmt, bool stats, bool tiled, Fn f) {
    const auto pick = [](bool v, auto g) {
        if (v) g(std::true_type{});
        else g(std::false_type{});
    };
    pick(fmt == VX_PIXEL_RGBA32F, [&](auto f32) {
        pick(stats, [&](auto S) {
            pick(tiled, [&](auto T) {
                f(std::integral_constant<int, f32() ? VX_PIXEL_RGBA32F : VX_PIXEL_RGBA8>{}, S, T);
            });
        });
    });
}

// ---------------- 2D mode (u_quality = 0) ----------------
// drawScene binds the vertex2d mesh when mode == MODE_2D and sets u_quality = 0
// (render.js:278, 287): the footprint quads of sdf.cpp:362-401 on the z = 0
// plane (vert2d: normal byte 0 -> v_normal = (1, 0, 0), render.vert:16; id 2
// for glass), front-facing from above (tri2d winding, culled from below,
// render.js:88-91), over the clear colour (0.9, 0.9, 0.9) (render.js:274-275:
// from the second frame on).  render.frag with u_quality = 0 outputs the
// palette colour (:241-244); glass: alpha 0.8 exp2(dot(rayDir, n)), rgb *=
// 0.2 atmCol (:246-249), blended over the clear colour.  The march and the
// AO sample the reference also runs there do not reach the output (:244): not
// run.  Oracle: vxo_render.c shade_2d.
constexpr float kClear2d = 0.9f;
__device__ __forceinline__ void shade_2d(const KernelArgs &a, float d0, float d1, float d2, float rgba[4], Counters &cnt,
                         unsigned &n_sky, unsigned &n_block, unsigned &n_glass) {
    const FrameConsts &F = a.fc;
    rgba[0] = rgba[1] = rgba[2] = kClear2d;
    rgba[3] = 1.0f;
    const float zr = (float)(0 - F.cam_cell[2]) - F.cam_fract[2];      // the plane, camera-relative
    int c = 0, x = 0, y = 0;
    float hx = 0.0f, hy = 0.0f;
    if (zr < 0.0f && d2 < 0.0f) {                                       // camera above, ray going down
        const float t = zr / d2;
        hx = F.cam_fract[0] + t * d0;
        hy = F.cam_fract[1] + t * d1;
        x = F.cam_cell[0] + f2i(floorf(hx));
        y = F.cam_cell[1] + f2i(floorf(hy));
        if ((unsigned)x < (unsigned)a.X && (unsigned)y < (unsigned)a.Y) {
            c = (int)a.fp2d[2 * ((size_t)y * a.X + x)];
            cnt.prim_fetch++;
        }
    }
    if (c == 0) {
        n_sky = 1;
        return;
    }
    const uint32_t org = a.fp2d[2 * ((size_t)y * a.X + x) + 1];
    const int x0 = (int)(org & 0xffffu), y0 = (int)(org >> 16);
    const float pc0 = kPalette[c][0], pc1 = kPalette[c][1], pc2 = kPalette[c][2];
    if (c != kGlass) {
        n_block = 1;
        rgba[0] = pc0; rgba[1] = pc1; rgba[2] = pc2;
        return;
    }
    n_glass = 1;
    // v_cellPos = the quad corner (x0, y0, 0), v_fractPos = hit - corner (render.vert:27-28)
    const float f0 = (float)(F.cam_cell[0] - x0) + hx, f1 = (float)(F.cam_cell[1] - y0) + hy;
    float r0, r1, r2;
    normalize3((float)(x0 - F.cam_cell[0]) + (f0 - F.cam_fract[0]), (float)(y0 - F.cam_cell[1]) + (f1 - F.cam_fract[1]),
               (float)(0 - F.cam_cell[2]) + (0.0f - F.cam_fract[2]), r0, r1, r2);     // render.frag:154
    const float k = 2.0f * ((1.0f * r0 + 0.0f * r1) + 0.0f * r2);                  // reflect(rayDir, n)
    const float rz = sqrtf(gmax(0.0f, r2 - k * 0.0f));
    float src[4];
    src[3] = 0.8f * vexp2((r0 * 1.0f + r1 * 0.0f) + r2 * 0.0f);
    const float pc[3] = {pc0, pc1, pc2};
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const float atm = gmix(F.scatterCol[i], F.spaceCol[i], rz);
        src[i] = pc[i] * (0.2f * atm);
    }
    blend_canvas(src, rgba, rgba);          // over the clear colour in the canvas
}

}  // namespace
}  // namespace vx
