// vx_gbuffer.hip — the frame's depth and surface planes (vx_render_gbuffer):
// per pixel what vx_query_rays answers for vx_pixel_ray's ray with t_max =
// INFINITY, as 4 to 12 bytes instead of 48 in and 88 out.  A translation unit
// of its own, like vx_query.hip and for the same reason: kernel_meta.check()
// budgets every kernel whose name holds k_render, and tests/test_query.py
// counts the kernels and code objects that hold k_query.
//
// One lane per pixel in the render kernel's mapping (vx_pixel.h: 32x8-pixel
// blocks of four 8x8 waves), so neighbouring rays walk neighbouring cells.
// The ray is view_ray's, bit for bit.  The walk is k_query's (vx_query.hip)
// restated with t_max = +inf, statement for statement, so that unit's machine
// code is untouched; what differs is where the origin comes from: the camera
// is one origin for the whole frame, so the slabs, the entry cell's range and
// the padded origin cell are wave-uniform kernel arguments (gbuffer_frame,
// vx_frame.cpp: frame_consts' expressions) instead of per-lane converts.  The
// record's cell and fract are never formed: a plane takes t, or the packed
// (n, normal, colour) word.
//
// Every index the walk forms lies inside the padded copy, for every camera
// vx_render_gbuffer's check lets through (|cam_cell| < 2^22, 0 <= cam_fract <
// 1, finite basis) and every direction the per-lane test lets through (finite,
// not all zero; a sum of finite basis terms can overflow): k_query's argument
// with its ray origin = the camera.  The entry cell is clamped into the grid
// (cell_lo, cell_hi are exact: |cam_cell| and the dimensions are below 2^23),
// a fetched cell that is not the sentinel lies in the grid, and one step leaves
// such a cell c for A + s on the exit axis (|A + s - c| = E + 1 <= cap) and for
// a cell of [c, A] on the others (med3 returns one of its bounds even for a NaN
// first operand): at most cap cells outside the grid, inside the border of pad
// = cap sentinel cells, which ends the walk; the iteration cap ends anything
// else.  A store goes to word py * w + px < w * h of a plane of w * h words.
#include "vx_pixel.h"
#include "vx_walk.h"

namespace vx {
namespace {

__device__ __forceinline__ bool finite(float d) { return fabsf(d) < kInf; }

template <bool STATS>
__global__ __launch_bounds__(kWG) void k_gbuffer(const GbufArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int px = (int)(blockIdx.x << kBXS) + (((wave % kWX) << 3) | (lane & 7));
    const int py = (int)(blockIdx.y << kBYS) + (((wave / kWX) << 3) | (lane >> 3));
    unsigned n_invalid = 0, n_hits = 0, n_glass = 0, n_fetch = 0, n_cap = 0;
    if (px < a.w && py < a.h) {                        // lanes outside the frame neither walk nor store
        float d0, d1, d2;
        view_ray(a, px, py, d0, d1, d2);
        const float o0 = a.o[0], o1 = a.o[1], o2 = a.o[2];
        const bool valid = finite(d0) && finite(d1) && finite(d2) && !(d0 == 0.0f && d1 == 0.0f && d2 == 0.0f);
        // results: the first glass entry and the entry that ended the walk: crossing time, axis; its colour
        bool gl = false, hit = false;
        float gt = 0.0f, te = 0.0f, hp0 = 0.0f, hp1 = 0.0f, hp2 = 0.0f;
        int gax = 0, hax = 0, col = 0;
        if (valid) {
            float iv0, iv1, iv2;
            ray_rcp(d0, d1, d2, iv0, iv1, iv2);
            // grid slabs from the camera; a zero component misses unless the camera lies inside that slab
            float tlo = 0.0f, thi = kInf;
            bool miss = false;
#define VX_SLAB(D, IV, K)                                                     \
            {                                                                 \
                const float lo = a.slab_lo[K], hi = a.slab_hi[K];             \
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
            if (!miss && tlo < thi) {
                // entry cell relative to the camera cell, as exact fp32 integers, clamped into the grid
                const float cf0 = __builtin_amdgcn_fmed3f(floorf(o0 + tlo * d0), a.cell_lo[0], a.cell_hi[0]);
                const float cf1 = __builtin_amdgcn_fmed3f(floorf(o1 + tlo * d1), a.cell_lo[1], a.cell_hi[1]);
                const float cf2 = __builtin_amdgcn_fmed3f(floorf(o2 + tlo * d2), a.cell_lo[2], a.cell_hi[2]);
                const bool p0 = !(d0 < 0.0f), p1 = !(d1 < 0.0f), p2 = !(d2 < 0.0f);
                const float s0 = p0 ? 1.0f : -1.0f, s1 = p1 ? 1.0f : -1.0f, s2 = p2 ? 1.0f : -1.0f;
                hp0 = p0 ? 1.0f : 0.0f; hp1 = p1 ? 1.0f : 0.0f; hp2 = p2 ? 1.0f : 0.0f;
                float h0 = cf0 + hp0, h1 = cf1 + hp1, h2 = cf2 + hp2;
                // element index of the padded cell cam_cell + pad + h - hp in the ray octant's copy, as k_query
                // forms it: x + Xp*y as the bits of one exact fp32 fma biased by 2^23, z by a 24-bit multiply
                const int oct = (p0 ? 0 : 1) | (p1 ? 0 : 2) | (p2 ? 0 : 4);
                const uint32_t *pp = a.prim + (size_t)oct * a.copy_texels;
                const float bx = a.padded[0] - hp0 + 8388608.0f, by = a.padded[1] - hp1,
                            bz = a.padded[2] - hp2 + 8388608.0f;
                const float fXp = a.Xpf;
                auto fetch = [&]() -> uint32_t {
                    const unsigned xy = __float_as_uint(__builtin_fmaf(h1 + by, fXp, h0 + bx)) - 0x4B000000u;
                    return pp[xy + __umul24(__float_as_uint(h2 + bz), a.XpYp)];
                };
                uint32_t t = fetch();                  // in the grid by the clamp: never the sentinel
                n_fetch++;
                int prev = t & 0xff;
                float E0 = cvt_f32_ubyte1(t), E1 = cvt_f32_ubyte2(t), E2 = cvt_f32_ubyte3(t);
                int it = 0;
                for (; it < a.cap; it++) {
                    const float A0 = __builtin_fmaf(s0, E0, h0), A1 = __builtin_fmaf(s1, E1, h1), A2 = __builtin_fmaf(s2, E2, h2);
                    const float tb0 = (A0 - o0) * iv0, tb1 = (A1 - o1) * iv1, tb2 = (A2 - o2) * iv2;
                    te = __builtin_fminf(__builtin_fminf(tb0, tb1), tb2);
                    if (te >= kInf) break;             // k_query's te >= t_max with t_max = +inf
                    const bool e0 = tb0 == te;
                    const bool e1 = !e0 && tb1 == te;
                    hax = e0 ? 0 : (e1 ? 1 : 2);
                    h0 = e0 ? A0 + s0 : __builtin_amdgcn_fmed3f(floorf(o0 + te * d0) + hp0, h0, A0);
                    h1 = e1 ? A1 + s1 : __builtin_amdgcn_fmed3f(floorf(o1 + te * d1) + hp1, h1, A1);
                    h2 = (!e0 && !e1) ? A2 + s2 : __builtin_amdgcn_fmed3f(floorf(o2 + te * d2) + hp2, h2, A2);
                    t = fetch();
                    if (t >= kSentinel) break;         // left the grid: no fetch counted, no surface
                    n_fetch++;
                    col = t & 0xff;
                    E0 = cvt_f32_ubyte1(t); E1 = cvt_f32_ubyte2(t); E2 = cvt_f32_ubyte3(t);
                    // a face of the mesh: entering a meshed cell from a cell of another colour
                    if (col != prev && col != 0) {
                        if (col != kGlass) {
                            hit = true;
                            break;
                        }
                        if (!gl) {                     // the first glass entry: recorded, the walk goes on
                            gl = true;
                            gt = te; gax = hax;
                        }
                    }
                    prev = col;
                }
                if (it >= a.cap) n_cap++;
            }
        } else {
            n_invalid = 1;
        }
        // normal index of an entry through axis ax: 2 * ax, + 1 for a ray going up that axis (render.vert:14-17)
        auto normal_idx = [&](int ax) -> unsigned {
            const bool pos = (ax == 0 ? hp0 : (ax == 1 ? hp1 : hp2)) != 0.0f;
            return (unsigned)(2 * ax + (pos ? 1 : 0));
        };
        const unsigned half_g = normal_idx(gax) << 2 | (unsigned)kGlass << 8;
        const unsigned half_h = hit ? normal_idx(hax) << 2 | (unsigned)col << 8 : 0u;
        n_glass = gl ? 1u : 0u;
        n_hits = n_glass + (hit ? 1u : 0u);
        const unsigned idx = (unsigned)py * (unsigned)a.w + (unsigned)px;   // w * h <= 2^26
        if (a.depth) a.depth[idx] = gl ? gt : (hit ? te : kInf);
        if (a.opaque_depth) a.opaque_depth[idx] = hit ? te : kInf;
        if (a.surface) a.surface[idx] = n_hits | (gl ? half_g : half_h) | half_h << 16;
    }
    if (STATS) {
        // every lane of the wave is here again: one atomicAdd per wave and counter
        const unsigned long long v[QS_COUNT] = {wave_sum(n_invalid), wave_sum(n_hits), wave_sum(n_glass), wave_sum(n_fetch),
                                                wave_sum(n_cap)};
        if ((threadIdx.x & 63) == 0) {
#pragma unroll
            for (int k = 0; k < QS_COUNT; k++)
                if (v[k]) atomicAdd(a.stats + k, v[k]);
        }
    }
}

}  // namespace

int launch_gbuffer(const GbufArgs &a, void *stream) {
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)((a.w + kBX - 1) >> kBXS), (unsigned)((a.h + kBY - 1) >> kBYS)), block(kWG);
    if (a.stats) hipLaunchKernelGGL(k_gbuffer<true>, grid, block, 0, s, a);
    else hipLaunchKernelGGL(k_gbuffer<false>, grid, block, 0, s, a);
    return (int)hipGetLastError();
}

}  // namespace vx
