// vx_resolve.hip — the resolve of vx_render_aa (include/voxmap.h "antialiasing"):
// output pixel (x, y) from the S x S block at (S*x, S*y) of a chunk of the
// hi-res frame.  Streaming and bandwidth-bound: a lane reads 16-byte pieces of S
// consecutive hi-res rows, and a wave's loads and stores cover contiguous row
// pieces.  No load is misaligned or reaches past the chunk's S * rows rows of
// S * w pixels: every lane's pieces lie inside the pixels its own output covers.
//
// RGBA8: per channel (sum of the S*S bytes + S*S/2) / (S*S).  The bytes are
// summed as even / odd bytes in 16-bit halves of a dword (16 bytes sum to at
// most 4080), no floating point.  RGBA32F: ((H(0,0) + H(1,0)) + (H(0,1) +
// H(1,1))) * 0.25f, for S = 4 applied twice; the unit compiles with
// -ffp-contract=off like every other (build.py), which the definition needs.
//
// Row alignment: a hi-res row is S * w pixels.  RGBA32F pixels are 16 bytes and
// S = 4 RGBA8 rows are 16 * w bytes: always aligned.  S = 2 RGBA8 rows are 8 * w
// bytes: with w odd every other row sits 8 bytes off, so that case (and an out
// that is not 8-byte aligned) takes the narrow shape, 8-byte loads that give one
// output pixel per lane, instead of 16-byte loads that give two.
#include <hip/hip_runtime.h>

#include "vx_internal.h"

namespace vx {
namespace {

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kResolveWG = 256;

// The intermediate is read once.  Non-temporal loads measured no faster than plain
// ones here (DESIGN.md §3 "Antialiasing"), so plain is the default; -DVX_RESOLVE_NT=1
// builds the variant for an A/B run.
#ifndef VX_RESOLVE_NT
#define VX_RESOLVE_NT 0
#endif
template <class T> __device__ __forceinline__ T load_once(const T *p) {
#if VX_RESOLVE_NT
    return __builtin_nontemporal_load(p);
#else
    return *p;
#endif
}

// byte sums of RGBA8 pixels: R, B in the 16-bit halves of e, G, A in those of o
struct Sum8 {
    unsigned e = 0, o = 0;
    __device__ __forceinline__ void add(unsigned p) {
        e += p & 0x00FF00FFu;
        o += (p >> 8) & 0x00FF00FFu;
    }
    // (sum + n/2) / n per channel, n = S*S a power of two; a half's quotient is at most 255, and
    // the mask drops what the shift brings down from the upper half
    template <int S> __device__ __forceinline__ unsigned mean() const {
        constexpr unsigned sh = S == 2 ? 2 : 4, half = (unsigned)(S * S / 2) * 0x00010001u;
        return (((e + half) >> sh) & 0x00FF00FFu) | ((((o + half) >> sh) & 0x00FF00FFu) << 8);
    }
};

__device__ __forceinline__ f32x4 resolve2(f32x4 h00, f32x4 h10, f32x4 h01, f32x4 h11) {
    return ((h00 + h10) + (h01 + h11)) * 0.25f;
}

// One output row per blockIdx.y, one unit per lane along it: two output pixels
// (RGBA8, S = 2, wide) or one.  src: the chunk's first hi-res row, rows
// src_row_bytes apart; dst: the chunk's first output row, rows of w pixels.
template <int FMT, int S>
__global__ void __launch_bounds__(kResolveWG) k_resolve(const char *__restrict__ src, char *__restrict__ dst, int w,
                                                        int units, size_t src_row_bytes, int narrow) {
    const int u = blockIdx.x * kResolveWG + threadIdx.x;
    if (u >= units) return;
    const size_t y = blockIdx.y;
    const char *r0 = src + (size_t)S * y * src_row_bytes;
    if constexpr (FMT == VX_PIXEL_RGBA8) {
        unsigned *out = reinterpret_cast<unsigned *>(dst + y * (size_t)w * 4);
        if constexpr (S == 2) {
            if (narrow) {
                const u32x2 a = load_once(reinterpret_cast<const u32x2 *>(r0) + u);
                const u32x2 b = load_once(reinterpret_cast<const u32x2 *>(r0 + src_row_bytes) + u);
                Sum8 s;
                s.add(a.x); s.add(a.y); s.add(b.x); s.add(b.y);
                out[u] = s.mean<2>();
            } else {
                const u32x4 a = load_once(reinterpret_cast<const u32x4 *>(r0) + u);
                const u32x4 b = load_once(reinterpret_cast<const u32x4 *>(r0 + src_row_bytes) + u);
                Sum8 s0, s1;
                s0.add(a.x); s0.add(a.y); s0.add(b.x); s0.add(b.y);
                s1.add(a.z); s1.add(a.w); s1.add(b.z); s1.add(b.w);
                u32x2 r;
                r.x = s0.mean<2>();
                r.y = s1.mean<2>();
                reinterpret_cast<u32x2 *>(out)[u] = r;
            }
        } else {
            Sum8 s;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const u32x4 a = load_once(reinterpret_cast<const u32x4 *>(r0 + (size_t)j * src_row_bytes) + u);
                s.add(a.x); s.add(a.y); s.add(a.z); s.add(a.w);
            }
            out[u] = s.mean<4>();
        }
    } else {
        f32x4 *out = reinterpret_cast<f32x4 *>(dst + y * (size_t)w * 16);
        if constexpr (S == 2) {
            const f32x4 *a = reinterpret_cast<const f32x4 *>(r0) + 2 * (size_t)u;
            const f32x4 *b = reinterpret_cast<const f32x4 *>(r0 + src_row_bytes) + 2 * (size_t)u;
            out[u] = resolve2(load_once(a), load_once(a + 1), load_once(b), load_once(b + 1));
        } else {
            f32x4 q[2][2];   // q[j][i]: the 2 x 2 block at (2i, 2j) of the lane's 4 x 4
#pragma unroll
            for (int j = 0; j < 2; j++) {
                const f32x4 *a = reinterpret_cast<const f32x4 *>(r0 + (size_t)(2 * j) * src_row_bytes) + 4 * (size_t)u;
                const f32x4 *b = reinterpret_cast<const f32x4 *>(r0 + (size_t)(2 * j + 1) * src_row_bytes) + 4 * (size_t)u;
#pragma unroll
                for (int i = 0; i < 2; i++)
                    q[j][i] = resolve2(load_once(a + 2 * i), load_once(a + 2 * i + 1), load_once(b + 2 * i),
                                       load_once(b + 2 * i + 1));
            }
            out[u] = resolve2(q[0][0], q[0][1], q[1][0], q[1][1]);
        }
    }
}

template <int FMT, int S>
void launch_k(const void *src, void *dst, int w, int rows, int units, size_t src_row_bytes, int narrow, hipStream_t s) {
    const dim3 grid((unsigned)((units + kResolveWG - 1) / kResolveWG), (unsigned)rows);
    hipLaunchKernelGGL((k_resolve<FMT, S>), grid, dim3(kResolveWG), 0, s, static_cast<const char *>(src),
                       static_cast<char *>(dst), w, units, src_row_bytes, narrow);
}

}  // namespace

int launch_resolve(const void *src, void *dst, int w, int rows, int ss, int src_pitch, int fmt, void *stream) {
    const hipStream_t s = (hipStream_t)stream;
    const bool f32 = fmt == VX_PIXEL_RGBA32F;
    const size_t row_bytes = (size_t)src_pitch * (f32 ? 16u : 4u);
    // what the vector accesses need; rows is a grid dimension
    const bool wide8 = !f32 && ss == 2 && !(row_bytes & 15u) && !(w & 1) && !((uintptr_t)dst & 7u);
    const bool narrow8 = !f32 && ss == 2 && !wide8;
    if (w <= 0 || rows <= 0 || rows > 65535 || (ss != 2 && ss != 4) || src_pitch < ss * w || ((uintptr_t)src & 15u) ||
        (row_bytes & (narrow8 ? 7u : 15u)) || ((uintptr_t)dst & (f32 ? 15u : 3u)))
        return (int)hipErrorInvalidValue;
    if (f32) {
        if (ss == 2) launch_k<VX_PIXEL_RGBA32F, 2>(src, dst, w, rows, w, row_bytes, 0, s);
        else launch_k<VX_PIXEL_RGBA32F, 4>(src, dst, w, rows, w, row_bytes, 0, s);
    } else {
        if (ss == 2) launch_k<VX_PIXEL_RGBA8, 2>(src, dst, w, rows, wide8 ? w / 2 : w, row_bytes, narrow8 ? 1 : 0, s);
        else launch_k<VX_PIXEL_RGBA8, 4>(src, dst, w, rows, w, row_bytes, 0, s);
    }
    return (int)hipGetLastError();
}

}  // namespace vx
