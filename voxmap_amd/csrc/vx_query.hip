// vx_query.hip — batched ray queries (vx_query_rays): picking and place-label
// visibility on the primary traversal's octant copies.  A translation unit of
// its own: kernel_meta.check() budgets every kernel whose name holds k_render,
// and this one shares nothing with them but device helpers: the arithmetic
// (vx_math.h), the byte converts and loads (vx_loads.h), ray_rcp (vx_walk.h).
//
// One lane per ray.  Per ray, exactly the oracle's primary_walk + walk(...,
// glass_layer = 1, ...) (oracle/vxo_render.c) with the ray's own origin in the
// place of cam_cell / cam_fract and the unit-cell split: grid slabs, entry cell
// clamped into the grid, box-exit stepping in walk_reflect()'s form (exact
// fp32 cells relative to the origin cell, h = c + hp, A = fma(s, E, h),
// crossing (A - o) * iv, ties x < y < z, med3 clamp on the other axes, biased
// fp32 index with a per-lane base), the first glass entry recorded and passed,
// later glass entries passed, the first opaque entry or the sentinel border
// ending the walk.
//
// Every index the walk forms lies inside the padded copy, for every ray the
// validation lets through: the entry cell is clamped into the grid, a fetched
// cell that is not the sentinel lies in the grid, and one step leaves such a
// cell c for A + s on the exit axis (|A + s - c| = E + 1 <= cap, the extents
// being <= cap - 1) and for a cell of [c, A] on the others (med3 returns one
// of its bounds even for a NaN first operand) -- at most cap cells outside the
// grid on any axis, and the border is pad = cap cells wide.  A border cell is
// the sentinel and ends the walk; the iteration cap ends anything else.
#include "vx_math.h"
#include "vx_loads.h"
#include "vx_walk.h"

namespace vx {
namespace {

typedef uint32_t u32x4u __attribute__((ext_vector_type(4), aligned(4)));   // a 16-byte store at dword alignment
typedef uint32_t u32x2u __attribute__((ext_vector_type(2), aligned(4)));

constexpr int kHitWords = sizeof(vx_ray_hit) / 4;
static_assert(sizeof(vx_ray) == 48 && sizeof(vx_surface) == 40 && sizeof(vx_ray_hit) == 88, "query record layout");

__device__ __forceinline__ bool cell_ok(int c) { return c > -(1 << 22) && c < (1 << 22); }
__device__ __forceinline__ bool fract_ok(float f) { return f >= 0.0f && f < 1.0f; }
__device__ __forceinline__ bool finite(float d) { return fabsf(d) < kInf; }

template <bool STATS>
__global__ __launch_bounds__(kWG) void k_query(const QueryArgs a) {
    const unsigned i = blockIdx.x * (unsigned)kWG + threadIdx.x;
    unsigned n_invalid = 0, n_hits = 0, n_glass = 0, n_fetch = 0, n_cap = 0;
    if (i < (unsigned)a.n) {                           // tail lanes neither load nor store
        const u32x4 *rp = static_cast<const u32x4 *>(a.rays) + 3 * (size_t)i;
        const u32x4 r0 = rp[0], r1 = rp[1], r2 = rp[2];
        const int B0 = (int)r0.x, B1 = (int)r0.y, B2 = (int)r0.z;
        const float o0 = __uint_as_float(r0.w), o1 = __uint_as_float(r1.x), o2 = __uint_as_float(r1.y);
        const float d0 = __uint_as_float(r1.z), d1 = __uint_as_float(r1.w), d2 = __uint_as_float(r2.x);
        const float tmax = __uint_as_float(r2.y);
        const bool valid = cell_ok(B0) && cell_ok(B1) && cell_ok(B2) && fract_ok(o0) && fract_ok(o1) && fract_ok(o2) &&
                           finite(d0) && finite(d1) && finite(d2) && !(d0 == 0.0f && d1 == 0.0f && d2 == 0.0f) &&
                           tmax == tmax;
        // results: the glass record (first glass entry) and the record that ended the walk
        bool gl = false, hit = false;
        float g0h = 0.0f, g1h = 0.0f, g2h = 0.0f, gt = 0.0f, te = 0.0f;
        float h0 = 0.0f, h1 = 0.0f, h2 = 0.0f, hp0 = 0.0f, hp1 = 0.0f, hp2 = 0.0f;
        int gax = 0, hax = 0, col = 0;
        if (valid) {
            // iv = RN(1/d), +inf for d = 0 (a positive axis, as -0 is): rcp_ranged where
            // the whole wave is in its range, the IEEE division otherwise
            float iv0, iv1, iv2;
            ray_rcp(d0, d1, d2, iv0, iv1, iv2);
            // grid slabs from the ray's own origin; a zero component misses unless
            // the origin lies inside that slab
            float tlo = 0.0f, thi = kInf;
            bool miss = false;
#define VX_SLAB(D, IV, B, O, DIM)                                             \
            {                                                                 \
                const float lo = (float)(0 - B) - O, hi = (float)(DIM - B) - O; \
                const float t0 = lo * IV, t1 = hi * IV;                       \
                const bool sw = t0 > t1, nz = D != 0.0f;                      \
                tlo = nz ? gmax(tlo, sw ? t1 : t0) : tlo;                     \
                thi = nz ? gmin(thi, sw ? t0 : t1) : thi;                     \
                miss |= !nz && !(lo <= 0.0f && 0.0f < hi);                    \
            }
            VX_SLAB(d0, iv0, B0, o0, a.X)
            VX_SLAB(d1, iv1, B1, o1, a.Y)
            VX_SLAB(d2, iv2, B2, o2, a.Z)
#undef VX_SLAB
            if (!miss && tlo < thi) {
                // entry cell relative to the origin cell, as exact fp32 integers,
                // clamped into the grid
                const float cf0 = __builtin_amdgcn_fmed3f(floorf(o0 + tlo * d0), (float)(-B0), (float)(a.X - B0 - 1));
                const float cf1 = __builtin_amdgcn_fmed3f(floorf(o1 + tlo * d1), (float)(-B1), (float)(a.Y - B1 - 1));
                const float cf2 = __builtin_amdgcn_fmed3f(floorf(o2 + tlo * d2), (float)(-B2), (float)(a.Z - B2 - 1));
                const bool p0 = !(d0 < 0.0f), p1 = !(d1 < 0.0f), p2 = !(d2 < 0.0f);
                const float s0 = p0 ? 1.0f : -1.0f, s1 = p1 ? 1.0f : -1.0f, s2 = p2 ? 1.0f : -1.0f;
                hp0 = p0 ? 1.0f : 0.0f; hp1 = p1 ? 1.0f : 0.0f; hp2 = p2 ? 1.0f : 0.0f;
                h0 = cf0 + hp0; h1 = cf1 + hp1; h2 = cf2 + hp2;
                // element index of the padded cell B + pad + h - hp in the ray octant's
                // copy: x + Xp*y as the bits of one exact fp32 fma biased by 2^23
                // (Xp*Yp < 2^23, |B| < 2^22), z by a 24-bit multiply of the biased bits
                const int oct = (p0 ? 0 : 1) | (p1 ? 0 : 2) | (p2 ? 0 : 4);
                const uint32_t *pp = a.prim + (size_t)oct * a.copy_texels;
                const float bx = (float)(B0 + a.pad) - hp0 + 8388608.0f, by = (float)(B1 + a.pad) - hp1,
                            bz = (float)(B2 + a.pad) - hp2 + 8388608.0f;
                const float fXp = a.Xpf;
                auto fetch = [&]() -> uint32_t {
                    const unsigned xy = __float_as_uint(__builtin_fmaf(h1 + by, fXp, h0 + bx)) - 0x4B000000u;
                    return pp[xy + __umul24(__float_as_uint(h2 + bz), a.XpYp)];
                };
                uint32_t t = fetch();                  // in the grid by the clamp: never the sentinel
                n_fetch++;
                int prev = t & 0xff;
                float E0 = cvt_f32_ubyte1(t), E1 = cvt_f32_ubyte2(t), E2 = cvt_f32_ubyte3(t);
                const int cap = 4 * (a.X + a.Y + a.Z);
                int it = 0;
                for (; it < cap; it++) {
                    const float A0 = __builtin_fmaf(s0, E0, h0), A1 = __builtin_fmaf(s1, E1, h1), A2 = __builtin_fmaf(s2, E2, h2);
                    const float tb0 = (A0 - o0) * iv0, tb1 = (A1 - o1) * iv1, tb2 = (A2 - o2) * iv2;
                    te = __builtin_fminf(__builtin_fminf(tb0, tb1), tb2);
                    if (te >= tmax) break;             // nothing from here on can count (t < t_max)
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
                            g0h = h0; g1h = h1; g2h = h2; gt = te; gax = hax;
                        }
                    }
                    prev = col;
                }
                if (it >= cap) n_cap++;
                gl = gl && gt < tmax;
                hit = hit && te < tmax;
            }
        } else {
            n_invalid = 1;
        }
        // the result: n, reserved, s[0], s[1]; unused records are zero
        constexpr int kRec = sizeof(vx_surface) / 4;
        auto record = [&](uint32_t (&r)[kRec], int id, int color, int ax, float q0, float q1, float q2, float t) {
            // q = the entered cell + hp; on the face axis the record holds the
            // face's plane, elsewhere the cell and the hit point minus it
            const float r0 = q0 - hp0, r1 = q1 - hp1, r2 = q2 - hp2;
            const bool pos = (ax == 0 ? hp0 : (ax == 1 ? hp1 : hp2)) != 0.0f;
            const int up = pos ? 0 : 1;
            r[0] = (uint32_t)id;
            r[1] = (uint32_t)color;
            r[2] = (uint32_t)(2 * ax + (pos ? 1 : 0));
            r[3] = (uint32_t)(B0 + (int)r0 + (ax == 0 ? up : 0));
            r[4] = (uint32_t)(B1 + (int)r1 + (ax == 1 ? up : 0));
            r[5] = (uint32_t)(B2 + (int)r2 + (ax == 2 ? up : 0));
            r[6] = __float_as_uint(ax == 0 ? 0.0f : (o0 + t * d0) - r0);
            r[7] = __float_as_uint(ax == 1 ? 0.0f : (o1 + t * d1) - r1);
            r[8] = __float_as_uint(ax == 2 ? 0.0f : (o2 + t * d2) - r2);
            r[9] = __float_as_uint(t);
        };
        uint32_t rg[kRec], rh[kRec];
        record(rg, 2, kGlass, gax, g0h, g1h, g2h, gt);
        record(rh, 0, col, hax, h0, h1, h2, te);
        const int nrec = (gl ? 1 : 0) + (hit ? 1 : 0);
        n_glass = gl ? 1u : 0u;
        n_hits = (unsigned)nrec;
        uint32_t w[kHitWords];
        w[0] = valid ? (uint32_t)nrec : (uint32_t)VX_RAY_INVALID;
        w[1] = 0u;
#pragma unroll
        for (int k = 0; k < kRec; k++) {               // selects, not indexed stores: w stays in registers
            w[2 + k] = gl ? rg[k] : (hit ? rh[k] : 0u);
            w[2 + kRec + k] = (gl && hit) ? rh[k] : 0u;
        }
        uint32_t *out = static_cast<uint32_t *>(a.hits) + (size_t)kHitWords * i;
#pragma unroll
        for (int k = 0; k + 4 <= kHitWords; k += 4) {
            u32x4u v;
            v.x = w[k]; v.y = w[k + 1]; v.z = w[k + 2]; v.w = w[k + 3];
            *reinterpret_cast<u32x4u *>(out + k) = v;
        }
        {
            u32x2u v;
            v.x = w[kHitWords - 2]; v.y = w[kHitWords - 1];
            *reinterpret_cast<u32x2u *>(out + kHitWords - 2) = v;
        }
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

int launch_query(const QueryArgs &a, void *stream) {
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)((a.n + kWG - 1) / kWG)), block(kWG);
    if (a.stats) hipLaunchKernelGGL(k_query<true>, grid, block, 0, s, a);
    else hipLaunchKernelGGL(k_query<false>, grid, block, 0, s, a);
    return (int)hipGetLastError();
}

}  // namespace vx
