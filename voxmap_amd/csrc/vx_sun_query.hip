// vx_sun_query.hip — batched sunlight queries (vx_query_sun): for n points and k
// sun directions, lit(i, j) of include/voxmap.h.  A translation unit of its
// own, as vx_query.hip is: kernel_meta.check() budgets every kernel whose name
// holds k_render, and this one shares with them only the march of vx_march.h,
// which it calls as the frames do (march_sun with no cone copy: the orthant exit
// copy of the sun's octant, else the plain channel; never a doom code).
//
// One lane per point, the wave loops over the suns.  A sun's constants (SunQ:
// sun_ray()'s, its sign pattern and its face-test mask, filled by the host)
// come through scalar loads at a wave-uniform address, so the choice of march
// variant and the switch into the specialised march_pad<SG> loops are
// wave-uniform; the face test and a point's validity are per-lane predicates.
//
// Every index a march forms lies inside the copy it reads, for every point the
// validation lets through (every cell axis inside the grid, -1 <= fract < 2,
// finite):
//   * march_literal and march_fast (suns off the fast path; scenes without
//     padded copies) test the cell against the grid before every load.
//   * march_pad reads the query's own padded copies (launch_sun_widen), whose
//     border is SBq = sun_query_border(Z) cells of -1.  A step moves axis i by
//     |r_i| * safe * len.  With one axis at the minimum, len = min_j t_j <= t_i
//     = RN(d_i / |r_i|), so the axis moves by at most d_i * safe, d_i <= 1.0001;
//     where axes tie, len is the literal length of render.frag:105-116, at most
//     sqrt(3) times that.  The first step has safe = 1: from a fract in [-1, 2)
//     it ends in (-2.74, 3.74), so it lands within 3 cells of an in-grid cell,
//     and SBq >= 3.  Every later step starts from a fract in [0, 1) in a cell
//     whose texel was positive, i.e. an in-grid cell with safe <= Z (a scene has
//     padded copies only if every R, G <= Z), and moves by less than
//     1.7324 * Z cells: it lands at most floor(1.7324 * Z) + 1 = SBq - 1 cells
//     outside the grid.  A border cell reads -1 and ends the march, lit.
//     (The frames' copies have a border of Z + 2, which a tie step with safe >=
//     2 could overrun; a frame's marches start on faces, a query's anywhere, so
//     the query does not read them.)
//   * fast-path rule of this entry point: every 2^-10 <= |r_i| <= 1
//     (sun_query_entry).  The upper bound is what march_len_fract's exactness
//     note and the bound above assume; a query's suns need not be normalised.
#include "vx_march.h"

namespace vx {
namespace {

static_assert(sizeof(vx_sun_point) == 32 && sizeof(SunQ) == 64, "sun query record layout");

// a load from the constant address space at a wave-uniform address is a scalar load
#define VX_CONST_AS __attribute__((address_space(4)))

__device__ __forceinline__ bool sun_fract_ok(float f) { return f >= -1.0f && f < 2.0f; }   // false for NaN

template <bool STATS>
__global__ __launch_bounds__(kWG) void k_sun_query(const SunQueryArgs a) {
    const unsigned i = blockIdx.x * (unsigned)kWG + threadIdx.x;
    const bool live = i < (unsigned)a.n;               // tail lanes neither load nor store
    Counters cnt = {};
    unsigned n_invalid = 0, n_rays = 0, n_culled = 0, n_lit = 0;
    bool valid = false;
    float c0 = 0.0f, c1 = 0.0f, c2 = 0.0f, f0 = 0.0f, f1 = 0.0f, f2 = 0.0f;
    unsigned face = 0u;                                // bit normal_idx, 0 for -1: tested against SunQ::cull
    if (live) {
        const u32x4 *pp = static_cast<const u32x4 *>(a.points) + 2 * (size_t)i;
        const u32x4 p0 = pp[0], p1 = pp[1];
        const int x = (int)p0.x, y = (int)p0.y, z = (int)p0.z, nidx = (int)p1.z;
        f0 = __uint_as_float(p0.w); f1 = __uint_as_float(p1.x); f2 = __uint_as_float(p1.y);
        valid = (unsigned)x < (unsigned)a.k.X && (unsigned)y < (unsigned)a.k.Y && (unsigned)z < (unsigned)a.k.Z &&
                sun_fract_ok(f0) && sun_fract_ok(f1) && sun_fract_ok(f2) && nidx >= -1 && nidx <= 5;
        c0 = (float)x; c1 = (float)y; c2 = (float)z;   // exact (dimensions < 2^16)
        face = nidx >= 0 ? 1u << (nidx & 7) : 0u;
        n_invalid = valid ? 0u : 1u;
    }
    uint32_t *out = a.out + (size_t)a.words * i;
    for (int j0 = 0; j0 < a.nsuns; j0 += 32) {         // one mask word: wave-uniform loop bounds
        const int nb = a.nsuns - j0 < 32 ? a.nsuns - j0 : 32;
        unsigned bits = 0u;
        for (int b = 0; b < nb; b++) {
            const uint32_t VX_CONST_AS *q = (const uint32_t VX_CONST_AS *)(a.suns + (j0 + b));
            const bool culled = ((unsigned)q[15] & face) != 0u;
            n_culled += valid && culled ? 1u : 0u;
            if (valid && !culled) {
                SunRay S;                              // SunQ::S, word by word: scalar registers
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    S.r[c] = __uint_as_float(q[c]); S.sign[c] = __uint_as_float(q[3 + c]);
                    S.abs[c] = __uint_as_float(q[6 + c]); S.rcp[c] = __uint_as_float(q[9 + c]);
                }
                S.up = (int)q[12]; S.fast = (int)q[13];
                n_rays++;
                if (march_sun<kDoomNone>(a.k, S, (int)q[14], c0, c1, c2, f0, f1, f2, cnt)) bits |= 1u << b;
            }
        }
        n_lit += (unsigned)__popc(bits);
        if (live) out[1 + (j0 >> 5)] = bits;           // 0 for an invalid point
    }
    if (live) out[0] = valid ? n_lit : VX_SUN_INVALID;
    if (STATS) {
        // every lane of the wave is here again: one atomicAdd per wave and counter
        const unsigned long long v[SS_COUNT] = {wave_sum(n_invalid), wave_sum(n_rays), wave_sum(n_culled), wave_sum(n_lit),
                                                wave_sum(cnt.shadow_fetch)};
        if ((threadIdx.x & 63) == 0) {
#pragma unroll
            for (int k = 0; k < SS_COUNT; k++)
                if (v[k]) atomicAdd(a.stats + k, v[k]);
        }
    }
}

// one thread per texel of the wide copies: the grid's texels from src, -1 around them
__global__ void k_sun_widen(const int8_t *src, int8_t *dst, int X, int Y, int Z, int SB, int SBq, int channels) {
    const size_t Xq = (size_t)X + 2 * SBq, Yq = (size_t)Y + 2 * SBq, Zq = (size_t)Z + 2 * SBq, nq = Xq * Yq * Zq;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nq * (size_t)channels) return;
    const size_t ch = i / nq, t = i % nq;
    const int x = (int)(t % Xq) - SBq, y = (int)((t / Xq) % Yq) - SBq, z = (int)(t / (Xq * Yq)) - SBq;
    int8_t v = -1;
    if ((unsigned)x < (unsigned)X && (unsigned)y < (unsigned)Y && (unsigned)z < (unsigned)Z) {
        const size_t Xp = (size_t)X + 2 * SB, Yp = (size_t)Y + 2 * SB, Zp = (size_t)Z + 2 * SB;
        v = src[ch * Xp * Yp * Zp + (size_t)(x + SB) + Xp * ((size_t)(y + SB) + Yp * (size_t)(z + SB))];
    }
    dst[i] = v;
}

}  // namespace

int launch_sun_query(const SunQueryArgs &a, void *stream) {
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)((a.n + kWG - 1) / kWG)), block(kWG);
    if (a.stats) hipLaunchKernelGGL(k_sun_query<true>, grid, block, 0, s, a);
    else hipLaunchKernelGGL(k_sun_query<false>, grid, block, 0, s, a);
    return (int)hipGetLastError();
}

int launch_sun_widen(const int8_t *src, int8_t *dst, int X, int Y, int Z, int SB, int SBq, int channels, void *stream) {
    const size_t n = ((size_t)X + 2 * SBq) * ((size_t)Y + 2 * SBq) * ((size_t)Z + 2 * SBq) * (size_t)channels;
    hipLaunchKernelGGL(k_sun_widen, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, src, dst, X, Y, Z,
                       SB, SBq, channels);
    return (int)hipGetLastError();
}

}  // namespace vx
