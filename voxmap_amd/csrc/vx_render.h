// vx_render.h — the fused render kernel of the Voxmap shading path (gfx950),
// shared by the translation units that instantiate it.
//
// One fused kernel per frame: primary visibility (the build's replacement for
// rasterising vertex.bin) -> render.frag main() shading with
// the sun march() (render.frag:75-142) -> glass blend -> framebuffer store.
// Lane = pixel; a wave64 covers an 8x8 pixel tile, a 256-thread workgroup a
// 32x8 block, so the rays of a wave march through neighbouring cells.
//
// Each EXT mode's instantiations are compiled in a translation unit of their
// own (vx_render_e*.hip): the same template text, so every mode's code is what
// it would be in one file, the units build in parallel, and the general shading
// modes (EXT 5/6) get a register budget of their own (VX_OCC_ATTR) without a
// shared body function for the others.
//
// The device code the kernel calls lives in one header per stage, included
// below in the order the stages run: vx_math.h, vx_loads.h, vx_march.h,
// vx_walk.h, vx_sample.h, vx_shade.h, vx_pool.h (the pooled modes' brick
// march), vx_pixel.h.  The kernel is tuned to the register; moving text
// between those headers is free (every kernel's machine code is compared,
// tools/isa_diff.py), folding it is not, nor is a new function boundary
// (DESIGN.md §3).
//
// Numerical contract: fp32, IEEE div/sqrt, no FMA contraction
// (built with -ffp-contract=off), GLSL built-ins spelled out, vexp2
// (vx_math.h), so every pixel matches the scalar oracle (oracle/vxo_render.c)
// bit for bit.
// Exactness-preserving rewrites used here (each justified in DESIGN.md §5):
//   * a / b with b a per-frame constant -> one Markstein correction from
//     y = RN(1/b) computed on the host (exhaustively checked:
//     tools/micro/markstein_all.hip): div_const, div_shared, vx_math.h;
//   * length(m*t) with a single selected axis -> t (sqrt(RN(t*t)) == t):
//     march_len_d, vx_march.h;
//   * unorm8 decode b/255 -> typed UNORM buffer loads (the texture data unit
//     returns RN(b/255) for every byte, tools/micro/unorm_check.hip): ld_fmt4,
//     vx_loads.h;
//   * per-frame uniform-only expressions -> host (vx_frame.cpp);
//   * min / max / clamp as v_min / v_max / the clamp modifier, and sqrtf /
//     normalize without their range handling, where the operands are proven
//     (fmin_fin, fmax_fin, clamp01, sqrt_ranged: vx_math.h; normalize3_ranged:
//     vx_sample.h; the view rays' lengths by a per-frame bit from the host,
//     FrameConsts::rays_ranged).
// Rejected experiments (bricked layouts, LDS r*k tables, hand-batched sky
// loads, typed primary loads, ...) are measured in profiles/ and kept in git
// history, not here.
#pragma once
#include "vx_math.h"
#include "vx_loads.h"
#include "vx_march.h"
#include "vx_walk.h"
#include "vx_sample.h"
#include "vx_shade.h"
#include "vx_pool.h"
#include "vx_pixel.h"

namespace vx {
namespace {

// Lane = pixel, wave = 8x8 tile, workgroup = 32x8 pixels.
// EXT: 0 = v1 (the reference's shader), 1 = extensions (REFLECT, ROUGH,
// REFLECT_ALL) with the hard shadow, 2 = extensions with soft shadows (n sun
// samples), 3 = 2 with the first surface's samples marched by the pooled wave
// pass (VX_FLAG_SOFT_POOL), 4 = 3 with LDS brick staging (VX_FLAG_SOFT_BRICK,
// march_brick: vx_pool.h), 5 / 6 = 1 / 2 with glass in draw order
// (VX_FLAG_GLASS_ORDER); named kExt* in vx_internal.h.  Each
// instantiation carries only its own code and registers; soft shadows in a
// kernel of their own also keep the sun_k[0] / sun_k[k] addresses apart (a
// pointer phi between them makes the compiler copy KernelArgs to scratch).
// Occupancy: 8 waves/SIMD needs <= 64 VGPRs and <= 80 SGPRs (8 256-thread
// blocks per CU, MI355X_MICROARCH.md "Residency"); every instantiation is held
// to that budget explicitly (left alone the EXT ones take 66 VGPRs + 100 SGPRs
// and run at 6 waves/SIMD).
// The counting (STATS) instantiations are not timed and keep 13 more per-lane
// counters live through every walk and march loop: at the 64-VGPR budget they
// spilled 300-500 VGPRs, so they take the registers they need instead
// (VX_OCC_WAVES(n): n waves/SIMD for the frames' kernels, no floor for STATS).
#define VX_OCC_WAVES(n) amdgpu_waves_per_eu(STATS ? 1 : (n), STATS ? 8 : (n))
#ifndef VX_OCC_ATTR
#define VX_OCC_ATTR __attribute__((VX_OCC_WAVES(8), amdgpu_num_sgpr(80)))
#endif

// F32IDX: the fp32 primary index (a.prim_f32) -- a kernel of its own: two
// inlined primary() copies in one kernel make the compiler copy KernelArgs
// to scratch.
template <int FMT, bool STATS, bool TILED, int EXT, bool F32IDX>
__global__ __launch_bounds__(kWG) VX_OCC_ATTR
void k_render(KernelArgs a) {
    // the shading instantiation: EXT 3/4 shade as 2; 5/6 are 1/2 with the general
    // shading block (glass in draw order, REFLECT_ALL)
    constexpr int XE = EXT == 5 ? 1 : (EXT >= 2 ? 2 : EXT);
    constexpr bool kPool = EXT == 3 || EXT == 4;   // VX_FLAG_SOFT_POOL: the pooled wave pass
    constexpr bool kBrick = EXT == 4;              // VX_FLAG_SOFT_BRICK: + LDS brick staging
    constexpr bool kGeneral = EXT >= 5;            // VX_FLAG_GLASS_ORDER / VX_FLAG_REFLECT_ALL
    // pooled pass: the frame's sun samples (r, |r|, RN(1/|r|)) and per wave
    // the compacted marching fragments' start (fract, cell) and lit counts
    __shared__ float4 s_sunk[kPool ? 3 * VX_MAX_SHADOW_SAMPLES : 1];
    __shared__ float4 s_pf[kPool ? kWG : 1];
    __shared__ float4 s_pc[kPool ? kWG : 1];
    __shared__ int s_plit[kPool ? kWG : 1];
    __shared__ int s_brick[kBrick ? 4 * 4 * 128 : 1];      // per wave: 4 bricks of 8x8x8 int8 (dwords)
    if (kPool) {
        for (int k = 0; k < a.fc.n_sun; k++) {          // uniform k: scalar loads of the kernel argument
            if (threadIdx.x == k) {
                const SunRay &Sk = a.fc.sun_k[k];
                s_sunk[3 * k] = make_float4(Sk.r[0], Sk.r[1], Sk.r[2], 0.0f);
                s_sunk[3 * k + 1] = make_float4(Sk.abs[0], Sk.abs[1], Sk.abs[2], 0.0f);
                s_sunk[3 * k + 2] = make_float4(Sk.rcp[0], Sk.rcp[1], Sk.rcp[2], 0.0f);
            }
        }
        __syncthreads();
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lx = ((wave % kWX) << 3) | (lane & 7);
    const int ly = ((wave / kWX) << 3) | (lane >> 3);
    int ox, oy, tx0 = 0, ty0 = 0, tile_k = 0;
    if (TILED) {
        // tiles of tile_w x tile_h pixels (multiples of the block), tile k of the
        // list at k * tile_w * tile_h in the compact output (or at its own
        // place in a w-wide frame: tile_inplace)
        // (launch_render_ext: a grid of (block columns, block rows, tiles), so no
        // integer division; a list of more than 65535 tiles takes a 1-D grid)
        const int perx = a.tile_w >> kBXS;
        int sx, sy;
        if (gridDim.y > 1 || gridDim.z > 1) {
            tile_k = blockIdx.z;
            sx = blockIdx.x;
            sy = blockIdx.y;
        } else {
            const int bpt = perx * (a.tile_h >> kBYS);
            tile_k = blockIdx.x / bpt;
            const int sub = blockIdx.x % bpt;
            sx = sub % perx;
            sy = sub / perx;
        }
        const int tid = a.tile_ids[tile_k];
        tx0 = sx << kBXS;
        ty0 = sy << kBYS;
        if (a.tiles_x == 1) {               // bands (vx_render_bands): one tile spans the row
            ox = tx0;
            oy = tid * a.tile_h + ty0;
        } else {
            ox = (tid % a.tiles_x) * a.tile_w + tx0;
            oy = (tid / a.tiles_x) * a.tile_h + ty0;
        }
    } else {
        ox = blockIdx.x << kBXS;
        // diagnostics (VX_FLAG_ROWS_BOTTOM_UP): block rows dispatched bottom row first
        oy = ((a.fc.flags & VX_FLAG_ROWS_BOTTOM_UP) ? gridDim.y - 1 - blockIdx.y : blockIdx.y) << kBYS;
    }
    const int px = ox + lx, py = oy + ly;
    const bool inframe = px < a.w && py < a.h;
    // the tiled launch's output index, formed once: only it stays live across the
    // shading instead of the tile's coordinates (the host keeps it below 2^32)
    const unsigned toidx = TILED ? (unsigned)out_index<TILED>(a, tile_k, tx0 + lx, ty0 + ly, px, py) : 0u;
    const FrameConsts &F = a.fc;
    Counters cnt = {};
#ifdef VX_BLOCK_TIMING
    // diagnostics build only (tools/block_times.py): the block's start and end
    // on the 100 MHz constant clock
    const unsigned long long t_blk0 = __builtin_amdgcn_s_memrealtime();
#endif
    unsigned n_sky = 0, n_block = 0, n_glass = 0, n_px = 0;
    // The pooled pass deals work over all 64 lanes of a wave, so there every
    // lane runs: a lane off the frame (a partial edge wave) takes the nearest
    // in-frame pixel's ray, marches for the others, and neither counts its own
    // primary work nor shades nor stores.
    if (kPool || inframe) {
        float d0, d1, d2;
        view_ray(F, kPool ? min(px, a.w - 1) : px, kPool ? min(py, a.h - 1) : py, d0, d1, d2);
        // the field copy of this ray's octant (zero components count positive)
        const int oct = (d0 < 0.0f ? 1 : 0) | (d1 < 0.0f ? 2 : 0) | (d2 < 0.0f ? 4 : 0);
        Surf g[2];
        float t_hit;
        int multi;
        const int n = primary<F32IDX>(a, oct, d0, d1, d2, g[0], g[1], cnt, t_hit, multi);
        // glass in draw order (render.js:82-91): the nearest pane is blended last,
        // over what is behind it; a ray that crosses two or more panes in front
        // of its surface first blends the panes drawn before the nearest one over
        // that (glass_chain), with one pane there are none.  VX_FLAG_GLASS_SINGLE:
        // the nearest pane only (diagnostic).  The general modes (VX_FLAG_GLASS_ORDER,
        // REFLECT_ALL) are instantiations of their own (EXT 5, 6), so their mirror
        // walk per surface adds no code or registers here.
        const bool order = !(F.flags & VX_FLAG_GLASS_SINGLE);
        const bool stacked = multi != 0 && order && !(F.flags & VX_FLAG_PRIMARY_ONLY) && inframe;
        int lit0 = -1;
        if (kPool && !inframe) cnt = Counters{};
        if (kPool && F.soft_sg >= 0 && a.sunp) {
            // Pooled soft shadows: the fragments of the wave that march are
            // compacted by a ballot, and each pass deals 64 / G of them with
            // G = 2^soft_lg lanes per fragment, lane k of a group marching sample
            // k.  A wave load then touches the few cache lines around 64 / G
            // surface points instead of one line per pixel, and lanes whose own
            // pixel does not march (sky, faces turned from the sun) march for
            // the others.  Same exact march_pad, lit counted per fragment in LDS.
            // (a glass pixel in draw order may shade other panes first: it marches in shade_block)
            const bool need = inframe && n != 0 && !(F.flags & (VX_FLAG_PRIMARY_ONLY | VX_FLAG_NO_SHADOW)) &&
                              block_shade_factor<XE>(a, g[0]) > 0.0f;
            const unsigned long long mask = __ballot(need);
            if (mask) {
                const int wb = threadIdx.x & ~63;                // this wave's 64 slots
                const int nf = __popcll(mask);
                const int slot = __popcll(mask & ((1ull << lane) - 1ull));
                if (need) {
                    s_pf[wb + slot] = make_float4(g[0].f0, g[0].f1, g[0].f2, 0.0f);
                    s_pc[wb + slot] = make_float4(g[0].c0, g[0].c1, g[0].c2, 0.0f);
                    s_plit[wb + slot] = 0;
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                const int lg = F.soft_lg;
                const int k = lane & ((1 << lg) - 1);
                const bool klane = k < F.n_sun;
                SunRay S;                                         // this lane's sample (per-lane values)
                const float4 q0 = s_sunk[3 * k], q1 = s_sunk[3 * k + 1], q2 = s_sunk[3 * k + 2];
                S.r[0] = q0.x; S.r[1] = q0.y; S.r[2] = q0.z;
                S.abs[0] = q1.x; S.abs[1] = q1.y; S.abs[2] = q1.z;
                S.rcp[0] = q2.x; S.rcp[1] = q2.y; S.rcp[2] = q2.z;
                const int8_t *ch = a.sunc ? a.sunc
                                         : a.sunx ? a.sunx + (size_t)F.soft_sg * a.sunp_texels
                                         : F.sun_k[0].up ? a.sunp : a.sunp + a.sunp_texels;
                // EXT 4 is launched only when the bricks fit (launch_render): <= 4 fragments per
                // pass, 4-byte aligned rows, a border of >= 9 cells around the grid
                const int sgv = F.soft_sg;
                const int bx = (sgv & 1) ? 0 : 4, by = (sgv & 2) ? 1 : 6, bz = (sgv & 4) ? 1 : 6;
                const int fpp = 64 >> lg;
                for (int base = 0; base < nf; base += fpp) {          // wave-uniform passes
                    const int fs = base + (lane >> lg);
                    if (kBrick) {
                        // stage the pass's bricks: 4 x 64 rows x 2 dwords, 8 dword loads per lane
                        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                        __builtin_amdgcn_wave_barrier();
                        int *wbrick = s_brick + (wb >> 6) * 512;
#pragma unroll
                        for (int j = 0; j < 8; j++) {
                            const int d = lane + 64 * j, bi = d >> 7, row = (d & 127) >> 1, half = d & 1;
                            const int fb = min(base + bi, nf - 1);
                            const float4 pc = s_pc[wb + fb];
                            const float4 pf = s_pf[wb + fb];     // anchor: the start's unit cell c + floor(f)
                            const int ox = ((int)(pc.x + floorf(pf.x)) + a.SB - bx) & ~3,
                                      oy = (int)(pc.y + floorf(pf.y)) + a.SB - by, oz = (int)(pc.z + floorf(pf.z)) + a.SB - bz;
                            const size_t off = (size_t)(unsigned)ox + 4u * half +
                                               (size_t)(unsigned)a.SXp * (unsigned)(oy + (row & 7)) +
                                               (size_t)a.SXpYp * (unsigned)(oz + (row >> 3));
                            wbrick[d] = *reinterpret_cast<const int *>(ch + off);
                        }
                        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                        __builtin_amdgcn_wave_barrier();
                    }
                    if (klane && fs < nf) {
                        const float4 pf = s_pf[wb + fs];
                        const float4 pc = s_pc[wb + fs];
                        cnt.shadow_rays++;
                        bool lit;
                        if constexpr (kBrick) {
                            const int8_t *br = reinterpret_cast<const int8_t *>(s_brick + (wb >> 6) * 512) +
                                               512 * (lane >> lg);
                            const int ox = ((int)(pc.x + floorf(pf.x)) + a.SB - bx) & ~3,
                                      oy = (int)(pc.y + floorf(pf.y)) + a.SB - by, oz = (int)(pc.z + floorf(pf.z)) + a.SB - bz;
                            switch (sgv) {
#define VX_SGB(K) case K: lit = march_brick<K>(a, S, ch, br, ox, oy, oz, pc.x, pc.y, pc.z, pf.x, pf.y, pf.z, \
                                               cnt); break;
                                VX_SGB(0) VX_SGB(1) VX_SGB(2) VX_SGB(3) VX_SGB(4) VX_SGB(5) VX_SGB(6)
                                default: lit = march_brick<7>(a, S, ch, br, ox, oy, oz, pc.x, pc.y, pc.z, pf.x, pf.y,
                                                              pf.z, cnt);
#undef VX_SGB
                            }
                        } else {
                            switch (sgv) {
#define VX_SGP(K) case K: lit = march_pad<K, kDoomAfter>(a, S, ch, pc.x, pc.y, pc.z, pf.x, pf.y, pf.z, \
                                                   cnt); break;
                                VX_SGP(0) VX_SGP(1) VX_SGP(2) VX_SGP(3) VX_SGP(4) VX_SGP(5) VX_SGP(6)
                                default: lit = march_pad<7, kDoomAfter>(a, S, ch, pc.x, pc.y, pc.z, pf.x, pf.y, pf.z,
                                                                  cnt);
#undef VX_SGP
                            }
                        }
                        if (lit) atomicAdd(&s_plit[wb + fs], 1);
                    }
                }
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                if (need) lit0 = s_plit[wb + slot];
            }
        }
        if (!kPool || inframe) {
            float rgba[4];
            if (F.flags & VX_FLAG_PRIMARY_ONLY) {
                primary_only_colour(n, g[0], rgba);
                n_sky = n == 0;
                n_glass = n != 0 && g[0].id == 2;
                n_block = n != 0 && g[0].id != 2;
            } else if (n == 0) {
                n_sky = 1;
                shade_sky(a, d0, d1, d2, rgba, cnt, F.rays_ranged != 0);
            } else {
                // what a glass pane blends over is shaded FIRST: only its colour
                // then stays live across the pane's shading (the record g[1]
                // itself would be: 9 registers, spilled to scratch at the
                // 64-VGPR budget).  Shading has no side effects besides the
                // counters (sums), so the order changes no result.
if constexpr (!kGeneral) {
                float dst[4];
                if (g[0].id == 2) {
                    if (n == 2) shade_block<XE>(a, g[1], dst, cnt);
                    else shade_sky(a, d0, d1, d2, dst, cnt);
                    // two or more panes (rare: a wave-uniform branch): the panes drawn
                    // before the nearest one, in draw order, over what is behind
                    if (__builtin_expect(__ballot(stacked) != 0, 0) && stacked)
                        glass_chain<XE>(a, d0, d1, d2, dst, n == 2 ? t_hit : kInf, cnt);
                }
                float rd[3];
                shade_block<XE>(a, g[0], rgba, cnt, false, 0.0f, 0.0f, 0.0f, rd, lit0);
                if (g[0].id == 2) {
                    n_glass = 1;
                    if (XE && (F.flags & VX_FLAG_REFLECT)) {
                        float refl[3];
                        reflect_color<XE>(a, g[0], rd, refl, cnt);
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
                (void)t_hit;
} else {
                // the general modes (REFLECT_ALL, VX_FLAG_GLASS_ORDER): every first
                // surface may mirror the scene; glass as in the one-blend path
                float dst[4];
                const bool glass = g[0].id == 2;
                if (glass) {
                    if (n == 2) shade_block<XE>(a, g[1], dst, cnt);
                    else shade_sky(a, d0, d1, d2, dst, cnt);
                    if (__builtin_expect(__ballot(stacked) != 0, 0) && stacked)
                        glass_chain<XE>(a, d0, d1, d2, dst, n == 2 ? t_hit : kInf, cnt);
                }
                float rd[3];
                shade_block<XE>(a, g[0], rgba, cnt, false, 0.0f, 0.0f, 0.0f, rd, lit0);
                // ext REFLECT (glass panes) / REFLECT_ALL (every first surface and pane)
                if (XE && (F.flags & (glass ? (VX_FLAG_REFLECT | VX_FLAG_REFLECT_ALL) : VX_FLAG_REFLECT_ALL))) {
                    // Schlick Fresnel, F0 = 0.04, on the geometric normal (cos = |rayDir| on the face axis)
                    float refl[3];
                    reflect_color<XE>(a, g[0], rd, refl, cnt);
                    const int ax = g[0].nidx >> 1;
                    const float cs = gmin(fabsf(ax == 0 ? rd[0] : (ax == 1 ? rd[1] : rd[2])), 1.0f);
                    const float x = 1.0f - cs, x2 = x * x;
                    const float fr = 0.04f + 0.96f * ((x2 * x2) * x);
#pragma unroll
                    for (int i = 0; i < 3; i++) rgba[i] = rgba[i] + fr * refl[i];
                }
                if (glass) {
                    n_glass = 1;
                    blend_canvas(rgba, dst, rgba);
                } else {
                    n_block = 1;
                }
}
            }
            rgba[3] = 1.0f;
            // each wave stores its own 8x8 tile (eight 32-B row pieces per RGBA8 wave
            // store): no block barrier, so a wave that finishes early frees its slot
            if constexpr (!TILED && FMT == VX_PIXEL_RGBA8)
                store_rgba8_frame(a, px, py, rgba);
            else
                store_pixel<FMT>(a, TILED ? (size_t)toidx : out_index<TILED>(a, tile_k, tx0 + lx, ty0 + ly, px, py), rgba);
            n_px = 1;
        }
    }
#ifdef VX_BLOCK_TIMING
    __syncthreads();
    if (threadIdx.x == 0 && a.blk_time) {
        const size_t b = (size_t)blockIdx.x + (size_t)blockIdx.y * gridDim.x;
        a.blk_time[2 * b] = t_blk0;
        a.blk_time[2 * b + 1] = __builtin_amdgcn_s_memrealtime();
    }
#endif
    if (STATS) flush_counters(a, cnt, n_px, n_sky, n_block, n_glass);
}

// One EXT mode's render launches: every (format, stats, tiled, primary index)
// instantiation of that mode, compiled in the unit that calls it.
template <int F, bool S, bool T, int E>
void launch_k(const KernelArgs &a, dim3 grid, hipStream_t s) {
    if constexpr (E >= 5) {           // the general shading modes: the integer primary index only
        hipLaunchKernelGGL((k_render<F, S, T, E, false>), grid, dim3(kWG), 0, s, a);
    } else {
        if (a.prim_f32)
            hipLaunchKernelGGL((k_render<F, S, T, E, true>), grid, dim3(kWG), 0, s, a);
        else
            hipLaunchKernelGGL((k_render<F, S, T, E, false>), grid, dim3(kWG), 0, s, a);
    }
}

template <int E>
int launch_render_ext(const KernelArgs &a, int fmt, unsigned gx, unsigned gy, void *stream) {
    const hipStream_t s = (hipStream_t)stream;
    // a tiled launch as (block columns, block rows, tiles) while the list fits the z dimension
    const bool t3 = a.tile_ids != nullptr && a.n_tiles <= 65535;
    const dim3 grid = t3 ? dim3((unsigned)(a.tile_w >> kBXS), (unsigned)(a.tile_h >> kBYS), (unsigned)a.n_tiles)
                         : dim3(gx, gy);
    const bool st = a.stats != nullptr, tiled = a.tile_ids != nullptr;
    launch_variant(fmt, st, tiled, [&](auto F, auto S, auto T) { launch_k<F(), S(), T(), E>(a, grid, s); });
    return (int)hipGetLastError();
}

}  // namespace
}  // namespace vx
