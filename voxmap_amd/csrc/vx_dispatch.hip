// vx_dispatch.hip — the per-frame render dispatch (gfx950): launch_render picks
// the frame's EXT mode and calls that mode's unit (vx_render_e*.hip; the 3D
// kernel, vx_render.h, is not included here), the 2D mode's kernel, the stats
// reduction and the de-tile pass.
#include "vx_pixel.h"

namespace vx {
namespace {

// 2D mode frames (quality 0) in a kernel of their own: the 3D kernel keeps its
// code and registers (a third user of the frame constants in k_render made
// the compiler copy KernelArgs to scratch).  Same pixel mapping and stores.
template <int FMT, bool STATS, bool TILED>
__global__ __launch_bounds__(kWG) void k_render_2d(KernelArgs a) {
    __shared__ uint32_t s_px[kBY][kBX];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lx = ((wave % kWX) << 3) | (lane & 7);
    const int ly = ((wave / kWX) << 3) | (lane >> 3);
    int ox, oy, tx0 = 0, ty0 = 0, tile_k = 0;
    if (TILED) {
        const int perx = a.tile_w >> kBXS, pery = a.tile_h >> kBYS;
        const int bpt = perx * pery;
        tile_k = blockIdx.x / bpt;
        const int sub = blockIdx.x % bpt;
        const int tid = a.tile_ids[tile_k];
        tx0 = (sub % perx) << kBXS;
        ty0 = (sub / perx) << kBYS;
        ox = (tid % a.tiles_x) * a.tile_w + tx0;
        oy = (tid / a.tiles_x) * a.tile_h + ty0;
    } else {
        ox = blockIdx.x << kBXS;
        oy = blockIdx.y << kBYS;
    }
    const int px = ox + lx, py = oy + ly;
    Counters cnt = {};
    unsigned n_sky = 0, n_block = 0, n_glass = 0, n_px = 0;
    if (px < a.w && py < a.h) {
        float d0, d1, d2, rgba[4];
        view_ray(a.fc, px, py, d0, d1, d2);
        shade_2d(a, d0, d1, d2, rgba, cnt, n_sky, n_block, n_glass);
        if (FMT == VX_PIXEL_RGBA8)
            s_px[ly][lx] = pack_rgba8(rgba);
        else
            store_pixel<FMT>(a, out_index<TILED>(a, tile_k, tx0 + lx, ty0 + ly, px, py), rgba);
        n_px = 1;
    }
    if (FMT == VX_PIXEL_RGBA8) {
        __syncthreads();
        const int sx = threadIdx.x & (kBX - 1), sy = threadIdx.x >> kBXS;
        if (ox + sx < a.w && oy + sy < a.h)
            reinterpret_cast<uint32_t *>(a.out)[out_index<TILED>(a, tile_k, tx0 + sx, ty0 + sy, ox + sx, oy + sy)] =
                s_px[sy][sx];
    }
    if (STATS) flush_counters(a, cnt, n_px, n_sky, n_block, n_glass);   // (only prim_fetch is counted here)
}

// Scatter compact tile-major pixels into a frame.
template <typename T>
__global__ void k_detile(const T *tiles, T *frame, int w, int h, int ts, int tiles_x, const int *ids, int n_tiles) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t per = (size_t)ts * ts;
    if (i >= per * n_tiles) return;
    const int k = (int)(i / per), r = (int)(i % per);
    const int tid = ids[k];
    const int x = (tid % tiles_x) * ts + r % ts, y = (tid / tiles_x) * ts + r / ts;
    if (x >= 0 && y >= 0 && x < w && y < h) frame[(size_t)y * w + x] = tiles[i];
}

__global__ void k_reduce_stats(unsigned long long *stats) {
    const int i = threadIdx.x;
    if (i < ST_COUNT) {
        unsigned long long s = 0;
        for (int r = 0; r < 64; r++) s += stats[r * ST_COUNT + i];
        stats[i] = s;
    }
}

}  // namespace

int launch_render(const KernelArgs &a, int fmt, void *stream) {
    hipStream_t s = (hipStream_t)stream;
    const bool tiled = a.tile_ids != nullptr;
    const bool st = a.stats != nullptr;
    dim3 block(kWG);
    dim3 grid = tiled ? dim3(a.n_tiles * (a.tile_w >> kBXS) * (a.tile_h >> kBYS))
                      : dim3((a.w + kBX - 1) / kBX, (a.h + kBY - 1) / kBY);
    if (a.fc.quality == 0) {          // MODE_2D: the vertex2d mesh (render.js:278, 287)
        launch_variant(fmt, st, tiled, [&](auto F, auto S, auto T) {
            hipLaunchKernelGGL((k_render_2d<F(), S(), T()>), grid, block, 0, s, a);
        });
        if (st) hipLaunchKernelGGL(k_reduce_stats, dim3(1), dim3(64), 0, s, a.stats);
        return (int)hipGetLastError();
    }
    const bool brick_ok = a.fc.soft_sg >= 0 && a.sunp && a.fc.soft_lg >= 4 && (a.SXp & 3) == 0 && a.SB >= 9;
    // the general shading block (glass in draw order, REFLECT_ALL): EXT 5 / 6 (not with the pooled pass)
    const bool general = (a.fc.flags & (VX_FLAG_GLASS_ORDER | VX_FLAG_REFLECT_ALL)) != 0;
    const unsigned fl = a.fc.flags;
    const int ext = a.fc.n_sun > 1 ? (general ? kExtGeneralSoft : (fl & VX_FLAG_SOFT_BRICK) && brick_ok ? kExtSoftBrick
                                      : (fl & (VX_FLAG_SOFT_POOL | VX_FLAG_SOFT_BRICK)) ? kExtSoftPool : kExtSoft)
                                   : (general ? kExtGeneralHard : (fl & (VX_FLAG_REFLECT | VX_FLAG_ROUGH)) ? kExtHard
                                      : kExtV1);
    int rc;
    switch (ext) {
        case kExtV1: rc = launch_render_e0(a, fmt, grid.x, grid.y, stream); break;
        case kExtHard: rc = launch_render_e1(a, fmt, grid.x, grid.y, stream); break;
        case kExtSoft: rc = launch_render_e2(a, fmt, grid.x, grid.y, stream); break;
        case kExtSoftPool: rc = launch_render_e3(a, fmt, grid.x, grid.y, stream); break;
        case kExtSoftBrick: rc = launch_render_e4(a, fmt, grid.x, grid.y, stream); break;
        default: rc = launch_render_e56(ext, a, fmt, grid.x, grid.y, stream); break;
    }
    if (rc) return rc;
    if (st) hipLaunchKernelGGL(k_reduce_stats, dim3(1), dim3(64), 0, s, a.stats);
    return (int)hipGetLastError();
}

int launch_reduce_stats(unsigned long long *stats, void *stream) {
    hipLaunchKernelGGL(k_reduce_stats, dim3(1), dim3(64), 0, (hipStream_t)stream, stats);
    return (int)hipGetLastError();
}

int launch_detile(const void *tiles, void *frame, int w, int h, int ts, int tiles_x, const int *ids,
                  int n_tiles, int fmt, void *stream) {
    const size_t n = (size_t)ts * ts * n_tiles;
    dim3 grid((unsigned)((n + 255) / 256));
    hipStream_t s = (hipStream_t)stream;
    if (fmt == VX_PIXEL_RGBA32F)
        hipLaunchKernelGGL(k_detile<float4>, grid, dim3(256), 0, s, (const float4 *)tiles, (float4 *)frame, w, h, ts,
                           tiles_x, ids, n_tiles);
    else
        hipLaunchKernelGGL(k_detile<uint32_t>, grid, dim3(256), 0, s, (const uint32_t *)tiles, (uint32_t *)frame, w,
                           h, ts, tiles_x, ids, n_tiles);
    return (int)hipGetLastError();
}

}  // namespace vx
