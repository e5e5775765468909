// vx_loads.h — what the render path's stages hand each other and how they read
// the field: the palette, the G-buffer record (Surf), the per-lane counters,
// the byte converts, the wave-wide helpers, and the loads (32-bit offsets from a wave-uniform base,
// typed buffer loads whose texture data unit converts the texel).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vx_internal.h"

namespace vx {
namespace {

// (row 22: what a colour past the palette shades as, white -- palette() clamps to it)
__constant__ float kPalette[23][3] = {
    {0.0f, 0.0f, 0.0f},
    {0.0431373f, 0.0627451f, 0.0745098f},
    {0.133333f, 0.490196f, 0.317647f},
    {0.321569f, 0.262745f, 0.239216f},
    {0.337255f, 0.423529f, 0.45098f},
    {0.392157f, 0.211765f, 0.235294f},
    {0.396078f, 0.403922f, 0.396078f},
    {0.439216f, 0.486275f, 0.454902f},
    {0.454902f, 0.403922f, 0.243137f},
    {0.52549f, 0.65098f, 0.592157f},
    {0.52549f, 0.756863f, 0.4f},
    {0.568627f, 0.596078f, 0.623529f},
    {0.647059f, 0.870588f, 0.894118f},
    {0.666667f, 0.666667f, 0.666667f},
    {0.741176f, 0.752941f, 0.729412f},
    {0.768627f, 0.384314f, 0.262745f},
    {0.780392f, 0.243137f, 0.227451f},
    {0.854902f, 0.788235f, 0.65098f},
    {0.964706f, 0.772549f, 0.333333f},
    {0.984314f, 0.886275f, 0.317647f},
    {1.0f, 1.0f, 1.0f},
    {0.505882f, 0.780392f, 0.831373f},
    {1.0f, 1.0f, 1.0f},
};

struct Surf {            // one G-buffer record (what render.vert hands render.frag)
    int id;              // 0 block, 1 sky, 2 glass
    int color;           // palette index
    int nidx;            // normal index 0..5 (render.vert:14-17)
    float c0, c1, c2;    // v_cellPos (exact integers: fp32 keeps the consumers' arithmetic convert-free)
    float f0, f1, f2;    // v_fractPos
};

struct Counters {
    unsigned prim_fetch, shadow_rays, shadow_fetch, ao, noise_px, cap_hit;
    unsigned refl_rays, refl_fetch, rough;   // extensions
    unsigned prim_witers, march_witers;      // loop iterations per wave (diagnostic: lane utilisation)
    unsigned march_slots;                    // per march wave iteration: the lanes that began that march
    unsigned shadow_resolved;                // shadow rays resolved by the first-step table test (not marched)
};

// A ray's own origin, for a kernel whose pixels do not share the frame's camera
// (k_ortho): what FrameConsts::cam_cell, cam_fract and skyOff are to k_render.
// The helpers that read the camera take one as an optional last argument; the
// frame kernels pass none, and their code is what it was without it.
struct RayOrigin {
    int cc0, cc1, cc2;       // the origin's cell (|cell| < 2^22)
    float o0, o1, o2;        // and fraction, in [0, 1)
    float sky0, sky1;        // 1e-4 * (cell.xy + fract.xy) (render.frag:191)
};

// (float)((t >> 8k) & 0xff) as one v_cvt_f32_ubyteK (left to itself the
// compiler may fold the mask away and emit a shift + convert)
__device__ __forceinline__ float cvt_f32_ubyte0(uint32_t t) {
    float r;
    asm("v_cvt_f32_ubyte0 %0, %1" : "=v"(r) : "v"(t));
    return r;
}
__device__ __forceinline__ float cvt_f32_ubyte1(uint32_t t) {
    float r;
    asm("v_cvt_f32_ubyte1 %0, %1" : "=v"(r) : "v"(t));
    return r;
}
__device__ __forceinline__ float cvt_f32_ubyte2(uint32_t t) {
    float r;
    asm("v_cvt_f32_ubyte2 %0, %1" : "=v"(r) : "v"(t));
    return r;
}
__device__ __forceinline__ float cvt_f32_ubyte3(uint32_t t) {
    float r;
    asm("v_cvt_f32_ubyte3 %0, %1" : "=v"(r) : "v"(t));
    return r;
}

// v counted once per wave: by the first active lane (wave-uniform loop counts)
__device__ __forceinline__ unsigned once_per_wave(unsigned v) {
    const unsigned long long act = __ballot(1);
    return __lane_id() == (unsigned)(__ffsll((unsigned long long)act) - 1) ? v : 0u;
}
// the lanes of the wave that run this code (a march's marching lanes, taken at its start)
__device__ __forceinline__ unsigned active_lanes() { return (unsigned)__popcll(__ballot(1)); }
// v summed over the wave's 64 lanes, in every lane (the counters' way out: k_render, k_render_2d, k_query)
__device__ __forceinline__ unsigned long long wave_sum(unsigned v) {
    unsigned long long s = v;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    return s;
}

// Field data in HBM, each array shaped for the loop that
// reads it, so a cache line holds as many useful cells as possible:
//   prim  8 copies, one per ray octant, u32 per cell: vis colour | ex << 8 |
//         ey << 16 | ez << 24 (vis colour = map.bin B if it is a meshed palette
//         index 1..21, else 0 = never a surface; extents of the all-unmeshed box
//         ahead, vxo_field_box), inside a border of P = cap sentinel cells
//         (0xFFFFFFFF: colour 0xFF is no vis colour, extents are <= cap - 1 <=
//         254), so the primary traversal detects leaving the grid from the value
//         it loads;
//   sunp  map.bin's R ("up") and G ("down") channels, int8 each, inside a
//         border of -1 cells: the sun march reads one of them;
//   sun   the same channels u8, unpadded (the literal march);
//   rg    R | G << 8, u16, linear: the AO trilinear sample.
// Every read is in bounds: the traversal stays within P of the grid, march()
// returns before reading outside it, the AO sample clamps.
constexpr uint32_t kSentinel = 0xFFFFFFFFu;   // border cells: colour 0xFF, extents 255

// Loads at a 32-bit byte offset from a wave-uniform base: lets the compiler
// use the saddr form (SGPR base + VGPR offset) instead of 64-bit per-lane
// address arithmetic.  Offsets here are < 2^31 (vx_scene_create limits).
template <typename T>
__device__ __forceinline__ T ld_off(const T *base, unsigned byte_off) {
    return *reinterpret_cast<const T *>(reinterpret_cast<const char *>(base) + byte_off);
}

// The base colour of palette index c (render.frag: c < 22 ? palette[c] : white):
// the index clamped onto the table's white row 22 instead of a divergent
// branch around the fetch, at a 32-bit offset from the table's base.
__device__ __forceinline__ void palette(int c, float &r, float &g, float &b) {
    const unsigned off = __umul24(min((unsigned)c, 22u), 12u);
    const float *base = &kPalette[0][0];
    r = ld_off(base, off); g = ld_off(base, off + 4u); b = ld_off(base, off + 8u);
}

// Typed buffer loads: the texture data unit converts the texel.
//   * the march texel: descriptor "8-bit, SSCALED" (DATA_FORMAT 1, NUM_FORMAT
//     3, DST_SEL_X = X) returns (float)(int8)texel, so the loop has no
//     byte -> float convert; base = the channel moved down by the offset bias
//     (0x4B000000, march_pad), num_records = 2^32 - 1 (offsets are in bounds
//     by the -1 border);
//   * AO and noise texels: NUM_FORMAT UNORM returns RN(b / 255) for every
//     byte b, the exact render.frag:38 decode (tools/micro/unorm_check.hip: all
//     256 bytes, 8, 8_8 and 8_8_8_8 formats, profiles/r02_unorm_check.txt).
// All of them through the LLVM intrinsic: the compiler sees the loads, places
// the waits, schedules independent work under them and never copies or spills
// a register a load has not written yet.
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ u32x4 buf_rsrc(const void *base, unsigned w3) {
    const unsigned long long p = (unsigned long long)base;
    u32x4 r;
    r.x = __builtin_amdgcn_readfirstlane((unsigned)p);
    r.y = __builtin_amdgcn_readfirstlane((unsigned)(p >> 32) & 0xffffu);
    r.z = 0xffffffffu;
    r.w = w3;
    return r;
}
constexpr unsigned kRsrcS8 = 0x0000B004u;  // 8, SSCALED, dst X: the march texel
constexpr unsigned kRsrcRGBA = 0x50FACu;   // 8_8_8_8, UNORM, dst (X, Y, Z, W): AO pairs, noise quads
__device__ float vx_ld_format_f32(u32x4 rsrc, unsigned voff, int soff, int aux)
    __asm("llvm.amdgcn.raw.buffer.load.format.f32");
__device__ f32x4 vx_ld_format_v4f32(u32x4 rsrc, unsigned voff, int soff, int aux)
    __asm("llvm.amdgcn.raw.buffer.load.format.v4f32");
__device__ __forceinline__ float ld_fmt1(u32x4 rsrc, unsigned off) { return vx_ld_format_f32(rsrc, off, 0, 0); }
__device__ __forceinline__ f32x4 ld_fmt4(u32x4 rsrc, unsigned off) { return vx_ld_format_v4f32(rsrc, off, 0, 0); }

// x + X*y + XY*z; X*Y < 2^23 (vx_scene_create): full-rate 24-bit multiplies
__device__ __forceinline__ unsigned lin_index(const KernelArgs &a, int x, int y, int z) {
    return (unsigned)x + __umul24((unsigned)a.X, (unsigned)y) + __umul24(a.XY, (unsigned)z);
}

}  // namespace
}  // namespace vx
