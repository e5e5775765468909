// vx_api.cpp — the C ABI (include/voxmap.h) over the HIP kernels.
//
// Replaces the WebGL host of the reference (src/web/render.js): texture
// upload (render.js:134-206) becomes vx_scene_create (field + noise resident
// in HBM, A channel filled on the GPU), drawScene (render.js:267-298) becomes
// vx_render / vx_render_tiles.  The camera/sun helpers restate map.js:349-402
// and math.js:16-49 in double precision, as the JS computes them.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "vx_device.h"
#include "vx_internal.h"

using namespace vx;

#ifndef VX_QSPEC   // as vx_walk.h: the fp32-index walk loads its quad offsets beside every prim word (d_qcopy)
#define VX_QSPEC 1
#endif

// Every device resource is a holder (vx_device.h), destroyed in reverse order
// of declaration: the stream and the stats events, declared first, outlive
// every buffer, cone copy and list (vx_scene_destroy).
struct vx_scene {
    int device = 0;
    int X = 0, Y = 0, Z = 0;
    int noise_w = 0, noise_h = 0;
    Stream stream;
    Event ev0, ev1;
    DevBuf<uint32_t> d_prim;      // 8 padded octant copies (vx_internal.h FieldLayout)
    DevBuf<uint8_t> d_sun;        // R, G channels
    DevBuf<int8_t> d_sunp;        // R, G channels, int8, -1 border (Z <= 126)
    DevBuf<int8_t> d_sunx;        // 8 orthant-exit copies of the march channel (launch_sun_exit)
    // cone copies of the march channel, built on first use for a frame's sun
    // samples {octant, kx, ky} (exit_plan) and kept: the sun moves slowly
    // (map.js:399-402), so one serves many frames
    struct Cone {
        int oct = -1, kx = -1, ky = -1;
        bool doom = false;            // the doom table is in (launch_sun_doom, window `plan`)
        int plan[7] = {0, 0, 0, 0, 0, 0, 0};
        DevBuf<int8_t> d;
        Event ready;                  // recorded on the build's stream after the build
        unsigned long long used = 0;
        bool ready_seen = false;      // the build's `ready` event observed complete
    } cones[2];
    unsigned long long cone_tick = 0;
    std::mutex cone_mu;
    // the sun queries' own march copies (sun_query_copies): sunp's two channels, then the orthant copies
    // where the scene has them, inside a border of sun_query_border(Z) cells; built by the first vx_query_sun
    struct SunQueryCopies {
        int state = 0;                // 0: not tried yet, 1: built, -1: none (no padded copies, or they do not fit)
        int SB = 0, SXp = 0, SYp = 0, SZp = 0;
        bool exits = false;
        DevBuf<int8_t> d;
        Event ready;                  // recorded on the build's stream after the build
        bool ready_seen = false;
    } sunq;
    std::mutex sunq_mu;
    // band / tile-id lists (vx_render_tiles / _bands, vx_detile), uploaded once
    // per distinct list and never rewritten while cached (list_acquire)
    struct ListBuf {
        std::vector<int> ids;         // the list d holds (also the upload's source)
        unsigned long long hash = 0;
        DevBuf<int> d;
        Event ready;                  // recorded after the upload
        bool ready_seen = false;
        int pins = 0;                 // renders between lookup and enqueue
        unsigned long long used = 0;
    };
    std::vector<std::unique_ptr<ListBuf>> lists;
    std::mutex lists_mu;
    unsigned long long list_tick = 0;
    int SB = 0, SXp = 0, SYp = 0, SZp = 0;
    DevBuf<uint16_t> d_rg;        // R | G << 8
    DevBuf<uint32_t> d_rg2;       // AO x-pairs: (R, G) of cells x and x + 1, clamped, (X + 1) per row
    DevBuf<uint8_t> d_bcol;       // map.bin's B channel as uploaded (vx_scene_read_field)
    DevBuf<uint16_t> d_qface;     // greedy mesh per face: 6 planes of X*Y*Z offsets from the quad origin
    DevBuf<uint32_t> d_qcopy;     // per octant, prim layout: entry faces' offsets (CHUNK <= 32), or null
    int chunk = 0;                // its CHUNK (sdf.cpp:284, voxmap.h:9)
    DevBuf<uint32_t> d_fp2d;      // 2D mode: per column vis colour + quad corner (KernelArgs::fp2d)
    std::vector<Quad2d> quads2d;  // 2D mode: the footprint's greedy quads (vx_scene_vertex2d)
    DevBuf<uint32_t> d_noise;
    DevBuf<uint32_t> d_noise4;    // noise quads, 4 planes (A, R, G, B): a channel of texels (x, y), (x+1, y), (x, y+1), (x+1, y+1), wrapped
    DevBuf<unsigned long long> d_stats;
    FieldLayout L;
    DevBuf<unsigned long long> d_blk;   // VX_BLOCK_TIMING builds: the last launch's block times
    size_t blk_cap = 0, blk_n = 0;
    bool f32_scene = false;       // the scene's half of the fp32-index predicate (do_render adds the camera's)
    KernelArgs ka;                // what no frame changes of do_render's arguments, filled once (scene_consts)
    QueryArgs qa;                 // and of do_query's
    GbufArgs ga;                  // and of do_gbuffer's
};

#define VX_HIP(call)                                                                                 \
    do {                                                                                             \
        hipError_t e_ = (call);                                                                      \
        if (e_ != hipSuccess)                                                                        \
            return set_error(VX_EDEVICE, std::string(#call " failed: ") + hipGetErrorString(e_));     \
    } while (0)

// early returns: of a hipError_t (a launcher's int is one) in a function that returns one, of a VX_E* code
#define VX_TRY(call) do { const hipError_t e_ = (hipError_t)(call); if (e_ != hipSuccess) return e_; } while (0)
#define VX_CHECK(call) do { const int rc_ = (call); if (rc_ != VX_OK) return rc_; } while (0)

int vx::scene_device(const vx_scene *s) { return s->device; }
void *vx::scene_stream(const vx_scene *s) { return (void *)s->stream.get(); }

// the stream an entry point works on: the caller's, or the scene's own
static hipStream_t stream_of(const vx_scene *s, void *stream) { return stream ? (hipStream_t)stream : s->stream.get(); }
static size_t pixel_bytes(int fmt) { return fmt == VX_PIXEL_RGBA32F ? 16 : 4; }

// every id of a tile / band list in [0, limit), or VX_EINVAL with the entry point's message
static int check_ids(const int *ids, int n, int limit, const char *message) {
    for (int i = 0; i < n; i++)
        if (ids[i] < 0 || ids[i] >= limit) return set_error(VX_EINVAL, message);
    return VX_OK;
}

// an optional table: one that does not fit leaves its buffer null and no HIP error behind
template <class T> static bool alloc_optional(DevBuf<T> &b, size_t n) {
    if (b.alloc(n) != hipSuccess) (void)hipGetLastError();
    return (bool)b;
}

// A cached copy (cone, list) read on stream st: st waits for the build's event
// until the host has seen it complete (a no-op on the build's own stream).
static int wait_ready(hipEvent_t ready, bool &seen, hipStream_t st) {
    if (seen) return VX_OK;
    const hipError_t q = hipEventQuery(ready);
    if (q == hipSuccess) seen = true;
    else if (q == hipErrorNotReady) VX_HIP(hipStreamWaitEvent(st, ready, 0));
    else VX_HIP(q);
    return VX_OK;
}

// A stats launch on stream st, bracketed: stats_begin zeroes n of the scene's counters and records ev0;
// stats_end records ev1, copies n counters to v, waits for st and gives the kernel time.  Events only
// for a stats launch: two more stream packets per frame widen the gap between back-to-back frames.
static int stats_begin(vx_scene *s, size_t n, hipStream_t st) {
    VX_HIP(hipMemsetAsync(s->d_stats.get(), 0, sizeof(unsigned long long) * n, st));
    VX_HIP(hipEventRecord(s->ev0.get(), st));
    return VX_OK;
}
static int stats_end(vx_scene *s, unsigned long long *v, size_t n, hipStream_t st, float *ms) {
    VX_HIP(hipEventRecord(s->ev1.get(), st));
    VX_HIP(hipMemcpyAsync(v, s->d_stats.get(), sizeof(unsigned long long) * n, hipMemcpyDeviceToHost, st));
    VX_HIP(hipStreamSynchronize(st));
    VX_HIP(hipEventElapsedTime(ms, s->ev0.get(), s->ev1.get()));
    return VX_OK;
}

// ---- vx_scene_create in stages: each returns the first hipError_t.  Their order is
// fixed: the allocations' order decides the device addresses, those the frame time (face_tables).
// The stages' temporaries, freed as build_scene returns: psum, ga, gb, lin (reverse of declaration)
struct Scratch {
    DevBuf<uint32_t> lin;     // the linear RGBA upload, B -> vis colour, A rewritten per octant
    DevBuf<uint8_t> gb, ga;   // launch_field_octant's, and launch_sun_exit's flags
    DevBuf<int> psum;         // prefix sums of solid cells for the octant boxes
};

// stream, events, the first allocations and the host's bytes on their way
static hipError_t upload(vx_scene *s, const SceneInputs &in, Scratch &sc) {
    const size_t N = (size_t)in.X * in.Y * in.Z, NN = (size_t)in.NW * in.NH;
    VX_TRY(s->stream.create());
    VX_TRY(s->ev0.create()); VX_TRY(s->ev1.create());
    VX_TRY(sc.lin.alloc(N));
    VX_TRY(s->d_noise.alloc(NN));
    VX_TRY(s->d_noise4.alloc(4 * NN));
    VX_TRY(s->d_stats.alloc((size_t)ST_COUNT * 64));
    VX_TRY(s->d_bcol.alloc(N));
    VX_TRY(sc.ga.alloc(N));
    VX_TRY(sc.gb.alloc(N));
    if (!in.from_grid)
        VX_TRY(hipMemcpyAsync(sc.lin.get(), in.field.data(), 4 * N, hipMemcpyHostToDevice, s->stream.get()));
    return hipMemcpyAsync(s->d_noise.get(), in.noise.data(), 4 * NN, hipMemcpyHostToDevice, s->stream.get());
}

// VX_FORMAT_GRID: sdf.cpp:405-470 on the device, into the linear RGBA upload buffer.  The palette
// grid's device copy is freed on return, before the kernels' arrays are allocated.
static hipError_t grid_field(vx_scene *s, const void *grid, Scratch &sc) {
    const size_t N = (size_t)s->X * s->Y * s->Z;
    DevBuf<uint8_t> d_col;
    VX_TRY(d_col.alloc(N));
    VX_TRY(hipMemcpyAsync(d_col.get(), grid, N, hipMemcpyHostToDevice, s->stream.get()));
    return (hipError_t)field_build_device(d_col.get(), sc.lin.get(), s->X, s->Y, s->Z, s->stream.get());
}

// 2D mode data (DESIGN.md §3 "2D mode"): the footprint of the field (each column's top block
// with z >= 1, sdf.cpp:201-204) meshed by the greedy 2D mesher of sdf.cpp:362-401 on the host,
// uploaded as {colour, quad corner} per column.
static hipError_t build_2d(vx_scene *s, const uint32_t *d_lin) {
    const size_t n = (size_t)s->X * s->Y;
    std::vector<uint8_t> c2d(n);
    {
        DevBuf<uint8_t> d_c2d;   // freed before d_fp2d is allocated
        VX_TRY(d_c2d.alloc(n));
        VX_TRY(launch_footprint(d_lin, d_c2d.get(), s->X, s->Y, s->Z, s->stream.get()));
        VX_TRY(hipMemcpyAsync(c2d.data(), d_c2d.get(), n, hipMemcpyDeviceToHost, s->stream.get()));
        VX_TRY(hipStreamSynchronize(s->stream.get()));
    }
    std::vector<uint32_t> origin(n, 0), fp(2 * n);
    mesh2d(c2d.data(), s->X, s->Y, s->quads2d, origin.data());
    for (size_t i = 0; i < n; i++) {
        fp[2 * i] = c2d[i];
        fp[2 * i + 1] = origin[i];
    }
    VX_TRY(s->d_fp2d.alloc(fp.size()));
    return hipMemcpy(s->d_fp2d.get(), fp.data(), fp.size() * 4, hipMemcpyHostToDevice);
}

// the kernels' arrays that every step reads: sun channels and
// AO arrays from the upload, the noise quads, and the prefix sums for the boxes
static hipError_t step_arrays(vx_scene *s, const SceneInputs &in, Scratch &sc) {
    const int X = s->X, Y = s->Y, Z = s->Z;
    const size_t N = (size_t)X * Y * Z;
    hipStream_t st = s->stream.get();
    VX_TRY(s->d_prim.alloc(8 * s->L.texels));
    VX_TRY(s->d_sun.alloc(2 * N));
    VX_TRY(s->d_rg.alloc(N));
    VX_TRY(s->d_rg2.alloc(N + (size_t)Y * Z));
    VX_TRY(sc.psum.alloc((size_t)(X + 1) * (Y + 1) * (Z + 1)));
    VX_TRY(hipMemsetD32Async((hipDeviceptr_t)s->d_prim.get(), 0xFFFFFFFF, 8 * s->L.texels, st));   // border = sentinel
    // B -> vis colour first: the boxes and prim copies classify by it
    VX_TRY(launch_field_vis(sc.lin.get(), s->d_bcol.get(), X, Y, Z, st));
    VX_TRY(build_2d(s, sc.lin.get()));
    VX_TRY(launch_field_pack(sc.lin.get(), s->d_sun.get(), s->d_rg.get(), X, Y, Z, st));
    VX_TRY(launch_ao_pairs(s->d_rg.get(), s->d_rg2.get(), X, Y, Z, st));
    VX_TRY(launch_noise_quads(s->d_noise.get(), s->d_noise4.get(), in.NW, in.NH, st));
    return (hipError_t)launch_field_psum(sc.lin.get(), sc.psum.get(), X, Y, Z, st);
}

// march copy of the sun channels: int8 inside a border of -1 ("left the grid"), so the
// march's loaded value carries the exit test (vx_march.h march_pad_from); values <= Z <= 126
static hipError_t march_copies(vx_scene *s, const SceneInputs &in, Scratch &sc) {
    const int X = s->X, Y = s->Y, Z = s->Z;
    hipStream_t st = s->stream.get();
    const size_t sxy = (size_t)(X + 2 * (Z + 2)) * (Y + 2 * (Z + 2));
    // the march's byte offset is 0x4B000000 + x + Xp*y + XpYp*z from fp32 bit patterns
    // (vx_march.h march_pad): the padded plane below 2^23, the sum below 2^32
    if (!(Z <= 126 && in.max_rg <= Z && sxy < (1u << 23) && sxy * (Z + 2 * (Z + 2) + 3) + 0x4B000000ull < (1ull << 32)))
        return hipSuccess;
    s->SB = Z + 2;
    s->SXp = X + 2 * s->SB; s->SYp = Y + 2 * s->SB; s->SZp = Z + 2 * s->SB;
    const size_t np = (size_t)s->SXp * s->SYp * s->SZp;
    VX_TRY(s->d_sunp.alloc(2 * np));
    VX_TRY(hipMemsetAsync(s->d_sunp.get(), 0xFF, 2 * np, st));
    VX_TRY(launch_sun_pad(sc.lin.get(), s->d_sunp.get(), X, Y, Z, s->SB, st));
    // per ray octant, the channel with every cell whose orthant ahead holds no block marked -1:
    // the march exits "lit" there (DESIGN.md §3 "Orthant exit").  The exit tables are an optimisation
    // (the kernel marches the plain channel when a.sunx is null): a copy that does not fit leaves them off
    if (!alloc_optional(s->d_sunx, 8 * np)) return hipSuccess;
    VX_TRY(hipMemsetAsync(s->d_sunx.get(), 0xFF, 8 * np, st));
    return (hipError_t)launch_sun_exit(s->d_sunp.get(), s->d_sunx.get(), sc.ga.get(), X, Y, Z, s->SB, st);
}

// per octant its cube sizes into the upload's A channel and from there into that octant's prim copy
static hipError_t octant_copies(vx_scene *s, const SceneInputs &in, Scratch &sc) {
    for (int oct = 0; oct < 8; oct++) {
        VX_TRY(launch_field_octant(sc.lin.get(), s->X, s->Y, s->Z, in.cap, oct, sc.ga.get(), sc.gb.get(), s->stream.get()));
        VX_TRY(launch_field_box(sc.lin.get(), sc.psum.get(), s->d_prim.get() + oct * s->L.texels, s->X, s->Y, s->Z,
                                s->L.pad, in.cap, oct, s->stream.get()));
    }
    return hipSuccess;
}

// the greedy mesh's quad per face (render.vert:25-28: v_cellPos is the quad origin), allocated after
// the arrays the kernels read every step: placed in front of them it moved their device addresses, and
// the v1 frame measured 3.3 % slower with the same kernel code (profiles/r04_ab_v1_bisect.txt,
// r04_ab_alloc_order.txt).  Optional: a field whose table does not fit still loads; its
// frames then need the unit-cell split and the single glass layer (vx_render refuses others), which are
// the only ones that read no mesh.  VOXMAP_TEST_NO_FACE_TABLE=1 makes the allocation fail (tests).
static hipError_t face_tables(vx_scene *s, const SceneInputs &in, Scratch &sc) {
    const size_t N = (size_t)s->X * s->Y * s->Z;
    const char *no_tab = std::getenv("VOXMAP_TEST_NO_FACE_TABLE");
    if ((no_tab && no_tab[0] == '1') || !alloc_optional(s->d_qface, 6 * N)) return hipSuccess;
    VX_TRY(launch_face_quads(sc.lin.get(), s->d_qface.get(), s->X, s->Y, s->Z, in.chunk, s->stream.get()));
    // the fp32-index walk's companion copy: quad offsets loaded beside
    // every prim word; fields whose walk takes the integer index (or CHUNK > 32) read
    // the face table once after the walk instead.  Optional: not allocated if it does not fit.
    if (!(VX_QSPEC && in.chunk <= 32 && s->f32_scene) || !alloc_optional(s->d_qcopy, 8 * s->L.texels)) return hipSuccess;
    return (hipError_t)launch_qcopy(s->d_qface.get(), s->d_qcopy.get(), s->X, s->Y, s->Z, s->L.pad, s->L.texels,
                                    s->stream.get());
}

// The launch arguments' fields that no frame changes, from zeroed structs
// (padding stays zero): do_render, do_query and do_gbuffer copy them and add the frame's.
static void scene_consts(vx_scene *s) {
    KernelArgs &a = s->ka;
    std::memset(&a, 0, sizeof a);
    a.prim = s->d_prim.get();
    a.sun = s->d_sun.get(); a.sunp = s->d_sunp.get(); a.sunx = s->d_sunx.get();
    a.SB = s->SB; a.SBf = (float)s->SB; a.SXp = s->SXp; a.SXpf = (float)s->SXp;
    a.SXpYp = (unsigned)s->SXp * (unsigned)s->SYp;
    a.sunp_texels = (unsigned)s->SXp * (unsigned)s->SYp * (unsigned)s->SZp;
    a.rg = s->d_rg.get(); a.rg2 = s->d_rg2.get();
    a.noise = s->d_noise.get(); a.noise4 = s->d_noise4.get();
    a.fp2d = s->d_fp2d.get();
    a.qface = s->d_qface.get(); a.qcopy = s->d_qcopy.get();
    a.chunk = s->chunk;
    a.X = s->X; a.Y = s->Y; a.Z = s->Z;
    a.Xf = (float)s->X; a.Yf = (float)s->Y; a.Zf = (float)s->Z;   // float copies: all exact (dimensions < 2^23)
    a.noise_w = s->noise_w; a.noise_h = s->noise_h;
    a.noise_wf = (float)s->noise_w; a.noise_hf = (float)s->noise_h;
    a.noise_rw = 1.0f / (float)s->noise_w; a.noise_rh = 1.0f / (float)s->noise_h;   // powers of two: exact
    while ((1 << a.noise_lw) < s->noise_w) a.noise_lw++;
    a.Xp = s->L.Xp; a.pad = s->L.pad;
    a.Xpf = (float)s->L.Xp; a.Xp4f = (float)(4 * s->L.Xp);
    a.XpYp = (unsigned)s->L.Xp * (unsigned)s->L.Yp;
    a.XY = (unsigned)s->X * (unsigned)s->Y; a.XYZ = a.XY * (unsigned)s->Z;
    a.copy_texels = (unsigned)s->L.texels;
    QueryArgs &q = s->qa;
    std::memset(&q, 0, sizeof q);
    q.prim = a.prim;
    q.X = s->X; q.Y = s->Y; q.Z = s->Z;
    q.pad = a.pad; q.Xp = a.Xp; q.Xpf = a.Xpf; q.XpYp = a.XpYp;
    q.copy_texels = a.copy_texels;
    GbufArgs &g = s->ga;
    std::memset(&g, 0, sizeof g);
    g.prim = a.prim;
    g.Xpf = a.Xpf; g.XpYp = a.XpYp; g.copy_texels = a.copy_texels;
    g.cap = 4 * (s->X + s->Y + s->Z);
}

// the scene's device half; the scratch buffers go after the final stream synchronisation
static int build_scene(vx_scene *s, const vx_scene_desc *d, const SceneInputs &in) {
    Scratch sc;
    hipError_t e = upload(s, in, sc);
    if (e != hipSuccess) return set_error(VX_EDEVICE, std::string("scene upload failed: ") + hipGetErrorString(e));
    if (in.from_grid && (e = grid_field(s, d->map_bytes, sc)) != hipSuccess)
        return set_error(VX_EDEVICE, std::string("device field build failed: ") + hipGetErrorString(e));
    e = step_arrays(s, in, sc);
    if (e == hipSuccess) e = march_copies(s, in, sc);
    if (e == hipSuccess) e = octant_copies(s, in, sc);
    if (e == hipSuccess) e = face_tables(s, in, sc);
    const hipError_t es = hipStreamSynchronize(s->stream.get());
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return set_error(VX_EDEVICE, std::string("field preparation failed: ") + hipGetErrorString(e));
    scene_consts(s);
    return VX_OK;
}

static int read_copy(vx_scene *s, int octant, void *host_out, size_t cap, bool boxes, const char *what) {
    if (!s || !host_out) return set_error(VX_EINVAL, std::string(what) + ": null argument");
    if (octant < 0 || octant > 7) return set_error(VX_EINVAL, std::string(what) + ": octant must be 0..7");
    const size_t n = (size_t)s->X * s->Y * s->Z * 4;
    if (cap < n) return set_error(VX_EINVAL, std::string(what) + ": buffer too small");
    VX_HIP(hipSetDevice(s->device));
    DevBuf<uint32_t> lin;
    VX_HIP(lin.alloc(n / 4));
    hipError_t e = (hipError_t)launch_field_unpack(boxes ? nullptr : s->d_rg.get(), s->d_bcol.get(),
                                                   s->d_prim.get() + (size_t)octant * s->L.texels, lin.get(), s->X, s->Y,
                                                   s->Z, s->L.pad, s->stream.get());
    if (e == hipSuccess) e = hipMemcpyAsync(host_out, lin.get(), n, hipMemcpyDeviceToHost, s->stream.get());
    if (e == hipSuccess) e = hipStreamSynchronize(s->stream.get());
    if (e != hipSuccess) return set_error(VX_EDEVICE, std::string(what) + ": " + hipGetErrorString(e));
    return VX_OK;
}

static int check_render(const vx_scene *s, const vx_frame_params *p, int w, int h, int fmt) {
    if (!s) return set_error(VX_EINVAL, "null scene/params");
    VX_CHECK(check_frame(p, w, h, fmt));
    // a scene without the greedy mesh per face (it did not fit) renders only
    // what reads no mesh: the unit-cell split and the single glass layer
    const unsigned need = VX_FLAG_UNIT_GBUF | VX_FLAG_GLASS_SINGLE;
    if (!s->d_qface && p->quality != 0 && ((p->flags & need) != need || (p->flags & VX_FLAG_GLASS_ORDER)))
        return set_error(VX_EINVAL, "this scene has no face table (it did not fit in device memory): its 3D frames "
                                    "need VX_FLAG_UNIT_GBUF | VX_FLAG_GLASS_SINGLE and not VX_FLAG_GLASS_ORDER");
    return VX_OK;
}

static void fill_stats(vx_stats *st, const unsigned long long *v, float ms, size_t out_bytes) {
    st->pixels = v[ST_PIXELS];
    st->sky_px = v[ST_SKY];
    st->block_px = v[ST_BLOCK];
    st->glass_px = v[ST_GLASS];
    st->primary_fetches = v[ST_PRIM_FETCH];
    st->shadow_rays = v[ST_SHADOW_RAYS];
    st->shadow_fetches = v[ST_SHADOW_FETCH];
    st->ao_samples = v[ST_AO];
    st->noise_px = v[ST_NOISE_PX];
    st->primary_cap_hits = v[ST_CAP_HITS];
    st->reflect_rays = v[ST_REFL_RAYS];
    st->reflect_fetches = v[ST_REFL_FETCH];
    st->rough_px = v[ST_ROUGH];
    st->primary_wave_iters = v[ST_PRIM_WITERS];
    st->march_wave_iters = v[ST_MARCH_WITERS];
    st->march_lane_slots = v[ST_MARCH_SLOTS];
    st->shadow_rays_resolved = v[ST_SHADOW_RESOLVED];
    // 4 B per field texel read (primary, shadow and reflection
    // rays), 32 B per trilinear AO, 80 B per clouded sky pixel (5 bilinear
    // noise taps), 16 B per rough-normal white() tap (4 texels), plus the
    // framebuffer store.
    st->alg_bytes = 4ull * (st->primary_fetches + st->shadow_fetches + st->reflect_fetches) +
                    32ull * st->ao_samples + 80ull * st->noise_px + 16ull * st->rough_px +
                    (unsigned long long)out_bytes * st->pixels;
    st->kernel_ms = ms;
}

// A tiled launch: tiles of tw x th pixels (multiples of the 32 x 8 kernel
// block), tiles_x per tile row; compact output (tile k at k * th * pitch
// pixels, rows pitch pixels apart) or in place in the w-wide frame.
struct TileSpec {
    int tw = 0, th = 0, pitch = 0, tiles_x = 0, inplace = 0;
    const int *ids = nullptr;   // device list
    int n = 0;
};

// The frame's cone copy {oct, kx, ky}: found in the scene's cache, or built on
// stream st into a free or the least recently used slot.  The caller holds
// s->cone_mu from here until its render is enqueued, so every render that
// reads a slot is enqueued before anyone can recycle it.  A recycle waits for
// the device: it needs a third sun window in the scene's two slots, so it
// happens at most once per sun window change (the sun moves about 1 rad per
// hour, map.js:399), and it keeps no handle of a caller's stream (ADVICE r05:
// a caller may destroy a stream it rendered on; an event per render on the
// reader's stream instead costs +3 % at C3, profiles/r04_ab_event_c3.txt).  A
// cache hit waits for the build (wait_ready).  t_build: recorded on st just
// before the build's first packet (vx_prepare_sun's timing), if built.
// doom: the copy carries the doom table of window plan (DESIGN.md §3 "Doom
// table"; part of the cache key).
static int cone_copy(vx_scene *s, int oct, int kx, int ky, bool doom, const int plan[7], hipStream_t st,
                     const int8_t **out, bool *built, vx_scene::Cone **used, hipEvent_t t_build) {
    *built = false;
    vx_scene::Cone *slot = nullptr;
    for (auto &c : s->cones)
        if (c.d && c.oct == oct && c.kx == kx && c.ky == ky && c.doom == doom &&
            (!doom || std::memcmp(c.plan, plan, sizeof c.plan) == 0))
            slot = &c;
    if (!slot) {
        slot = &s->cones[0];
        for (auto &c : s->cones)
            if (!c.d || c.used < slot->used) slot = &c;
        const size_t np = (size_t)s->SXp * s->SYp * s->SZp;
        if (slot->d) {
            VX_HIP(hipDeviceSynchronize());            // every render that read it is enqueued: done
        } else {
            VX_HIP(slot->d.alloc(np));
            if (!slot->ready) VX_HIP(slot->ready.create(hipEventDisableTiming));
        }
        slot->oct = -1;
        if (t_build) VX_HIP(hipEventRecord(t_build, st));
        VX_HIP(hipMemsetAsync(slot->d.get(), 0xFF, np, st));
        int rc = launch_sun_cone(s->d_sunp.get(), slot->d.get(), s->X, s->Y, s->Z, s->SB, oct, kx, ky, st);
        if (rc) return set_error(VX_EDEVICE, std::string("sun cone copy: ") + hipGetErrorString((hipError_t)rc));
        if (doom) {
            rc = launch_sun_doom(s->d_sunp.get(), slot->d.get(), s->X, s->Y, s->Z, s->SB, plan, st);
            if (rc) return set_error(VX_EDEVICE, std::string("sun doom table: ") + hipGetErrorString((hipError_t)rc));
        }
        VX_HIP(hipEventRecord(slot->ready.get(), st));
        slot->ready_seen = false;
        slot->oct = oct; slot->kx = kx; slot->ky = ky;
        slot->doom = doom;
        std::memcpy(slot->plan, plan, sizeof slot->plan);
        *built = true;
    } else {
        VX_CHECK(wait_ready(slot->ready.get(), slot->ready_seen, st));
    }
    slot->used = ++s->cone_tick;
    *out = slot->d.get();
    *used = slot;
    return VX_OK;
}

// The sun exit copy frame constants fc select (vx_exit_info kind 0/1/2):
// a.sunc (cone) built or found, and the info filled.  A frame's cone copy
// carries the doom table unless the frame asks VX_FLAG_NO_DOOM or
// VX_FLAG_SOFT_BRICK (the LDS brick march reads no doom codes).
static int frame_exit(vx_scene *s, const vx_frame_params *p, const FrameConsts &fc, hipStream_t st,
                      const int8_t **sunc, vx_exit_info *info, bool *built, vx_scene::Cone **used,
                      hipEvent_t t_build = nullptr) {
    *sunc = nullptr;
    *used = nullptr;
    bool b = false;
    vx_exit_info e{0, -1, -1, -1, 0.0f};
    const bool tables = s->d_sunx && !(p->flags & VX_FLAG_NO_EXIT);
    if (tables && p->quality != 0 && !(p->flags & (VX_FLAG_NO_SHADOW | VX_FLAG_PRIMARY_ONLY))) {
        int oct, kx, ky;
        if (!(p->flags & VX_FLAG_NO_CONE) && exit_plan(fc, s->SB, &oct, &kx, &ky)) {
            int plan[7] = {0, 0, 0, 0, 0, 0, 0};
            doom_plan(fc, plan);
            const bool doom = plan[6] >= 1 && !(p->flags & (VX_FLAG_NO_DOOM | VX_FLAG_SOFT_BRICK));
            VX_CHECK(cone_copy(s, oct, kx, ky, doom, plan, st, sunc, &b, used, t_build));
            e = vx_exit_info{2, oct, kx, ky, 0.0f};
        } else if (fc.sun_k[0].fast) {
            const float *r = fc.sun_k[0].r;
            e = vx_exit_info{1, (r[0] > 0.0f ? 1 : 0) | (r[1] > 0.0f ? 2 : 0) | (r[2] > 0.0f ? 4 : 0), -1, -1, 0.0f};
        }
    }
    if (built) *built = b;
    if (info) *info = e;
    return VX_OK;
}

// Tile / band-id lists live on the device, uploaded once per distinct list
// and never rewritten while cached: a render on any stream with a list the
// scene holds reads its buffer as it is, with no upload and no wait; a new
// list gets a new buffer, filled with hipMemcpyAsync on the caller's stream
// (renders of it on other streams wait for that copy: wait_ready).  So
// threads may render different lists of one scene on their own streams at
// once, and a list change stalls nothing (rounds 1-5
// rewrote one buffer per kind after a device-wide wait).
// A list is pinned from its lookup until its render is enqueued (ListRef).
// Only when more than kMaxLists distinct lists are cached is the least
// recently used unpinned one freed, after a device wait (its readers may be
// in flight on any stream).
constexpr size_t kMaxLists = 256;

// the list a launch reads, unpinned once the launch is enqueued
struct ListRef {
    vx_scene *s = nullptr;
    vx_scene::ListBuf *b = nullptr;
    void release() {
        if (!b) return;
        std::lock_guard<std::mutex> g(s->lists_mu);
        b->pins--;
        b = nullptr;
    }
    ~ListRef() { release(); }
};

static unsigned long long list_hash(const int *ids, int n) {
    unsigned long long h = 1469598103934665603ull;   // FNV-1a over the ints
    for (int i = 0; i < n; i++) h = (h ^ (unsigned)ids[i]) * 1099511628211ull;
    return h ^ (unsigned long long)n;
}

static int list_acquire(vx_scene *s, hipStream_t st, const int *ids, int n, ListRef &ref) {
    const unsigned long long h = list_hash(ids, n);
    std::lock_guard<std::mutex> g(s->lists_mu);
    vx_scene::ListBuf *b = nullptr;
    for (auto &p : s->lists)
        if (p->hash == h && (int)p->ids.size() == n && std::equal(p->ids.begin(), p->ids.end(), ids)) b = p.get();
    if (b) {
        VX_CHECK(wait_ready(b->ready.get(), b->ready_seen, st));
    } else {
        if (s->lists.size() >= kMaxLists) {
            size_t v = s->lists.size();
            for (size_t i = 0; i < s->lists.size(); i++)
                if (s->lists[i]->pins == 0 && (v == s->lists.size() || s->lists[i]->used < s->lists[v]->used)) v = i;
            if (v != s->lists.size()) {
                VX_HIP(hipDeviceSynchronize());
                VX_HIP(s->lists[v]->d.reset());
                VX_HIP(s->lists[v]->ready.reset());
                s->lists.erase(s->lists.begin() + (long)v);
            }
        }
        auto nb = std::make_unique<vx_scene::ListBuf>();
        nb->ids.assign(ids, ids + n);
        nb->hash = h;
        VX_HIP(nb->d.alloc((size_t)n));
        if (nb->ready.create(hipEventDisableTiming) != hipSuccess)
            return set_error(VX_EDEVICE, "list upload: event creation failed");
        // the entry's own host copy is the source: it lives as long as the buffer
        hipError_t e = hipMemcpyAsync(nb->d.get(), nb->ids.data(), sizeof(int) * (size_t)n, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipEventRecord(nb->ready.get(), st);
        if (e != hipSuccess) {
            (void)hipStreamSynchronize(st);   // before nb goes, with the copy's source and target
            return set_error(VX_EDEVICE, std::string("list upload: ") + hipGetErrorString(e));
        }
        s->lists.push_back(std::move(nb));
        b = s->lists.back().get();
    }
    b->pins++;
    b->used = ++s->list_tick;
    ref.s = s;
    ref.b = b;
    return VX_OK;
}

// One k_render launch: the scene's arguments (scene_consts) and what the frame decides.
static int do_render(vx_scene *s, const vx_frame_params *p, int w, int h, const TileSpec &ts, int fmt, void *out_dev,
                     hipStream_t st, vx_stats *stats, ListRef *lr = nullptr) {
    KernelArgs a;
    std::memcpy(&a, &s->ka, sizeof a);
    if (p->flags & VX_FLAG_NO_EXIT) a.sunx = nullptr;
    a.quad_gbuf = (p->flags & VX_FLAG_UNIT_GBUF) ? 0 : 1;
    a.w = w; a.h = h; a.tile_w = ts.tw; a.tile_h = ts.th;
    a.tile_pitch = ts.pitch; a.tiles_x = ts.tiles_x; a.tile_inplace = ts.inplace;
    a.tile_ids = ts.ids; a.n_tiles = ts.n;
    a.out = out_dev; a.p = *p;
    a.max_shadow_steps = p->max_shadow_steps > 0 ? p->max_shadow_steps : 2 * s->Z;   // render.frag:12
    frame_consts(*p, w, h, s->X, s->Y, s->Z, a.max_shadow_steps, a.fc);
    // the cone copy the frame reads stays pinned from its lookup until this
    // render is enqueued (a second thread must not recycle it in
    // between)
    std::unique_lock<std::mutex> cone_lock(s->cone_mu);
    vx_scene::Cone *cone = nullptr;
    VX_CHECK(frame_exit(s, p, a.fc, st, &a.sunc, nullptr, nullptr, &cone));
    if (!cone) cone_lock.unlock();
    a.kcam = (unsigned)(p->cam_cell[0] + a.pad) + (unsigned)a.Xp * (unsigned)(p->cam_cell[1] + a.pad) +
             a.XpYp * (unsigned)(p->cam_cell[2] + a.pad);   // mod 2^32
    // fp32 x/y index: 4*(x + Xp*y) of a fetched cell lies in [0, 4*Xp*Yp),
    // its partial sums 4x in [0, 4Xp) and y in [0, Yp), all exact fp32
    // integers below 2^24; the 24-bit multiply needs 4*Xp*Yp < 2^23, the
    // 32-bit byte offsets all 8 copies below 4 GiB (f32_scene); |z| < 2^21 (k_render)
    // (the fp32-index walk loads its quad offsets from the qcopy beside each prim word)
    const bool cam_ok = std::abs(p->cam_cell[0]) < (1 << 21) && std::abs(p->cam_cell[1]) < (1 << 21) &&
                        std::abs(p->cam_cell[2]) < (1 << 20);
    a.prim_f32 = s->f32_scene && cam_ok && (s->d_qcopy || !VX_QSPEC) && !(p->flags & VX_FLAG_INT_INDEX) ? 1 : 0;
    a.kx4 = (float)(4 * (p->cam_cell[0] + a.pad));
    a.ky = (float)(p->cam_cell[1] + a.pad);
    a.kz = 4u * a.XpYp * (unsigned)(p->cam_cell[2] + a.pad);
    // the octant terms of that offset, one scalar per sign a lane's compare selects
    // (primary(): 0x4B000000 and 4*XpYp << 22 are the biases of its x/y sum and its z)
    {
        const unsigned XpYp4 = 4u * a.XpYp, kzb = a.kz - 0x4B000000u - (XpYp4 << 22);
        a.kx4b = a.kx4 + 8388608.0f;
        a.kz_neg = kzb + (a.copy_texels << 4);
        a.kz_up = 0u - (a.copy_texels << 4) - XpYp4;
        a.koct0 = a.copy_texels << 2;
        a.koct1 = a.copy_texels << 3;
    }
#ifdef VX_BLOCK_TIMING
    if (!ts.ids) {
        const size_t nb = (size_t)((w + 31) / 32) * (size_t)((h + 7) / 8);
        if (nb > s->blk_cap) {
            VX_HIP(s->d_blk.alloc(2 * nb));
            s->blk_cap = nb;
        }
        s->blk_n = nb;
        a.blk_time = s->d_blk.get();
    }
#endif
    if (stats) {
        a.stats = s->d_stats.get();
        VX_CHECK(stats_begin(s, (size_t)ST_COUNT * 64, st));
    }
    const int rc = launch_render(a, fmt, st);
    if (rc) return set_error(VX_EDEVICE, std::string("render launch failed: ") + hipGetErrorString((hipError_t)rc));
    if (cone) cone_lock.unlock();   // enqueued: a recycle now waits for this render
    if (lr) lr->release();
    if (stats) {
        unsigned long long v[ST_COUNT];
        float ms = 0.0f;
        VX_CHECK(stats_end(s, v, ST_COUNT, st, &ms));
        fill_stats(stats, v, ms, pixel_bytes(fmt));
    }
    return VX_OK;
}

static void fill_query_stats(vx_query_stats *st, uint64_t rays, const unsigned long long *v, float ms) {
    st->rays = rays;
    st->invalid = v[QS_INVALID];
    st->hits = v[QS_HITS];
    st->glass = v[QS_GLASS];
    st->fetches = v[QS_FETCH];
    st->cap_hits = v[QS_CAP_HITS];
    st->kernel_ms = ms;
}

// One k_query launch over device arrays.  It reads only what vx_scene_create
// left behind (the octant copies and their layout), so it takes no scene lock;
// with stats it uses the scene's counters and events, as a vx_render with stats.
static int do_query(vx_scene *s, const void *d_rays, int n, void *d_hits, hipStream_t st, vx_query_stats *stats) {
    QueryArgs a;
    std::memcpy(&a, &s->qa, sizeof a);
    a.rays = d_rays; a.hits = d_hits; a.n = n;
    if (stats) {
        a.stats = s->d_stats.get();
        VX_CHECK(stats_begin(s, QS_COUNT, st));
    }
    const int rc = launch_query(a, st);
    if (rc) return set_error(VX_EDEVICE, std::string("query launch failed: ") + hipGetErrorString((hipError_t)rc));
    if (stats) {
        unsigned long long v[QS_COUNT];
        float ms = 0.0f;
        VX_CHECK(stats_end(s, v, QS_COUNT, st, &ms));
        fill_query_stats(stats, (uint64_t)n, v, ms);
    }
    return VX_OK;
}

// One k_gbuffer launch into device planes.  As do_query: it reads only what
// vx_scene_create left behind, takes no scene lock and keeps no stream handle;
// with stats it uses the scene's counters and events.
static int do_gbuffer(vx_scene *s, const vx_frame_params *p, int w, int h, const vx_gbuffer_planes &d, hipStream_t st,
                      vx_query_stats *stats) {
    GbufArgs a;
    std::memcpy(&a, &s->ga, sizeof a);
    gbuffer_frame(*p, w, h, s->X, s->Y, s->Z, s->L.pad, a);
    a.depth = d.depth; a.opaque_depth = d.opaque_depth; a.surface = d.surface;
    if (stats) {
        a.stats = s->d_stats.get();
        VX_CHECK(stats_begin(s, QS_COUNT, st));
    }
    const int rc = launch_gbuffer(a, st);
    if (rc) return set_error(VX_EDEVICE, std::string("gbuffer launch failed: ") + hipGetErrorString((hipError_t)rc));
    if (stats) {
        unsigned long long v[QS_COUNT];
        float ms = 0.0f;
        VX_CHECK(stats_end(s, v, QS_COUNT, st, &ms));
        fill_query_stats(stats, (uint64_t)w * (uint64_t)h, v, ms);
    }
    return VX_OK;
}

// The march copies a sun query reads, into the march's part of k: built on st by the scene's first
// query (vx_sun_query.hip says why the frames' border does not serve), read by later ones on any stream
// after the build's event.  A scene without padded copies, or one whose wide copies do not fit (memory,
// or the march's 2^23 / 2^32 index limits of march_copies), gets none: k.sunp = nullptr, and every fast
// sun takes the bounds-checked march_fast.
static int sun_query_copies(vx_scene *s, hipStream_t st, KernelArgs &k) {
    std::lock_guard<std::mutex> lock(s->sunq_mu);
    vx_scene::SunQueryCopies &q = s->sunq;
    if (q.state == 0) {
        q.state = -1;
        const int X = s->X, Y = s->Y, Z = s->Z, SB = sun_query_border(Z), ch = s->d_sunx ? 10 : 2;
        const size_t sxy = (size_t)(X + 2 * SB) * (Y + 2 * SB), np = sxy * (size_t)(Z + 2 * SB);
        if (s->d_sunp && sxy < (1u << 23) && sxy * (size_t)(Z + 2 * SB + 3) + 0x4B000000ull < (1ull << 32) &&
            alloc_optional(q.d, (size_t)ch * np)) {
            hipError_t e = q.ready.create(hipEventDisableTiming);
            // d_sunp's two channels and d_sunx's eight are one run of channels each, in the same padded layout
            if (e == hipSuccess) e = (hipError_t)launch_sun_widen(s->d_sunp.get(), q.d.get(), X, Y, Z, s->SB, SB, 2, st);
            if (e == hipSuccess && ch == 10)
                e = (hipError_t)launch_sun_widen(s->d_sunx.get(), q.d.get() + 2 * np, X, Y, Z, s->SB, SB, 8, st);
            if (e == hipSuccess) e = hipEventRecord(q.ready.get(), st);
            if (e != hipSuccess) {
                (void)hipStreamSynchronize(st);
                (void)q.d.reset();
                return set_error(VX_EDEVICE, std::string("sun query copies: ") + hipGetErrorString(e));
            }
            q.SB = SB; q.SXp = X + 2 * SB; q.SYp = Y + 2 * SB; q.SZp = Z + 2 * SB;
            q.exits = ch == 10;
            q.state = 1;
        }
    }
    k.sunc = nullptr;
    if (q.state != 1) {
        k.sunp = nullptr; k.sunx = nullptr;
        return VX_OK;
    }
    VX_CHECK(wait_ready(q.ready.get(), q.ready_seen, st));
    k.SB = q.SB; k.SBf = (float)q.SB; k.SXp = q.SXp; k.SXpf = (float)q.SXp;
    k.SXpYp = (unsigned)q.SXp * (unsigned)q.SYp;
    k.sunp_texels = k.SXpYp * (unsigned)q.SZp;
    k.sunp = q.d.get();
    k.sunx = q.exits ? q.d.get() + 2 * (size_t)k.sunp_texels : nullptr;
    return VX_OK;
}

// One k_sun_query launch over device arrays (d_suns: the call's SunQ table).  As do_query: it reads
// only what vx_scene_create and sun_query_copies left behind and keeps no stream handle; with stats
// it uses the scene's counters and events.
static int do_sun_query(vx_scene *s, const void *d_points, int n, const SunQ *d_suns, int k, int max_steps,
                        uint32_t flags, uint32_t *d_out, hipStream_t st, vx_sun_stats *stats) {
    SunQueryArgs a;
    std::memset(&a, 0, sizeof a);
    std::memcpy(&a.k, &s->ka, sizeof a.k);
    VX_CHECK(sun_query_copies(s, st, a.k));
    if (flags & VX_SUNQ_NO_EXIT) a.k.sunx = nullptr;
    a.k.fc.max_steps = max_steps > 0 ? max_steps : 2 * s->Z;   // render.frag:12
    a.points = d_points; a.out = d_out; a.suns = d_suns;
    a.n = n; a.nsuns = k; a.words = VX_SUN_WORDS(k);
    if (stats) {
        a.stats = s->d_stats.get();
        VX_CHECK(stats_begin(s, SS_COUNT, st));
    }
    const int rc = launch_sun_query(a, st);
    if (rc) return set_error(VX_EDEVICE, std::string("sun query launch failed: ") + hipGetErrorString((hipError_t)rc));
    if (stats) {
        unsigned long long v[SS_COUNT];
        float ms = 0.0f;
        VX_CHECK(stats_end(s, v, SS_COUNT, st, &ms));
        stats->points = (uint64_t)n;
        stats->invalid = v[SS_INVALID];
        stats->rays = v[SS_RAYS];
        stats->culled = v[SS_CULLED];
        stats->lit = v[SS_LIT];
        stats->fetches = v[SS_FETCH];
        stats->kernel_ms = ms;
    }
    return VX_OK;
}

// Chunks [c0, c1) of vx_render_aa's plan into their rows of the w x h device frame d_out:
// chunk c is band c of the (ss*w) x (ss*h) frame at band height ss * chunk_rows_out,
// rendered compact into `scratch` by the band path and resolved right behind it on st,
// while its bytes are still on-die.  One id list 0 .. n_chunks - 1 serves every chunk
// (chunk c reads the one id at offset c) and stays pinned until the last is enqueued: a
// call adds one list to the cache whatever its height.  Every chunk finds the sun copy
// the first one built (frame_exit).  stats: the chunks' counters summed, their kernel
// times plus the resolves'.
static int aa_chunks(vx_scene *s, const vx_frame_params *p, int w, int h, int fmt, const vx_aa_plan &plan, int c0, int c1,
                     void *scratch, void *d_out, hipStream_t st, vx_stats *stats) {
    const int ss = plan.ss, W = ss * w, H = ss * h;
    std::vector<int> ids((size_t)plan.n_chunks);
    for (int c = 0; c < plan.n_chunks; c++) ids[(size_t)c] = c;
    ListRef lr;
    VX_CHECK(list_acquire(s, st, ids.data(), plan.n_chunks, lr));
    TileSpec t;
    t.tw = (W + VX_TILE_ALIGN_X - 1) / VX_TILE_ALIGN_X * VX_TILE_ALIGN_X;
    t.th = ss * plan.chunk_rows_out;
    t.pitch = W;
    t.tiles_x = 1;
    t.n = 1;
    vx_stats sum;
    std::memset(&sum, 0, sizeof sum);
    for (int c = c0; c < c1; c++) {
        const int y0 = c * plan.chunk_rows_out, rows = std::min(plan.chunk_rows_out, h - y0);
        t.ids = lr.b->d.get() + c;
        vx_stats cs;
        VX_CHECK(do_render(s, p, W, H, t, fmt, scratch, st, stats ? &cs : nullptr));
        if (stats) VX_HIP(hipEventRecord(s->ev0.get(), st));
        const int rc = launch_resolve(scratch, static_cast<char *>(d_out) + (size_t)y0 * w * pixel_bytes(fmt), w, rows, ss,
                                      W, fmt, st);
        if (rc) return set_error(VX_EDEVICE, std::string("resolve launch failed: ") + hipGetErrorString((hipError_t)rc));
        if (stats) {
            float ms = 0.0f;
            VX_HIP(hipEventRecord(s->ev1.get(), st));
            VX_HIP(hipEventSynchronize(s->ev1.get()));
            VX_HIP(hipEventElapsedTime(&ms, s->ev0.get(), s->ev1.get()));
            uint64_t *a = &sum.pixels;
            const uint64_t *b = &cs.pixels;
            for (size_t i = 0; i < offsetof(vx_stats, kernel_ms) / sizeof(uint64_t); i++) a[i] += b[i];
            sum.kernel_ms += cs.kernel_ms + (double)ms;
        }
    }
    if (stats) *stats = sum;
    return VX_OK;
}

// One k_ortho launch: rows [row0, row0 + rows) of the w x h orthographic frame of p,
// compact at out_dev.  The frame's part of the arguments as do_render fills it (the
// sun, the colours, the exit copy through frame_exit, pinned until the launch is
// enqueued), and what every ray shares (ortho_frame).
static int do_ortho(vx_scene *s, const vx_frame_params *p, int w, int h, int row0, int rows, int fmt, void *out_dev,
                    hipStream_t st, vx_stats *stats) {
    OrthoArgs oa;
    std::memset(&oa, 0, sizeof oa);
    KernelArgs &a = oa.k;
    std::memcpy(&a, &s->ka, sizeof a);
    if (p->flags & VX_FLAG_NO_EXIT) a.sunx = nullptr;
    a.quad_gbuf = (p->flags & VX_FLAG_UNIT_GBUF) ? 0 : 1;
    a.w = w; a.h = h;
    a.out = out_dev; a.p = *p;
    a.max_shadow_steps = p->max_shadow_steps > 0 ? p->max_shadow_steps : 2 * s->Z;   // render.frag:12
    frame_consts(*p, w, h, s->X, s->Y, s->Z, a.max_shadow_steps, a.fc);
    ortho_frame(*p, oa);
    oa.row0 = row0; oa.rows = rows;
    std::unique_lock<std::mutex> cone_lock(s->cone_mu);
    vx_scene::Cone *cone = nullptr;
    VX_CHECK(frame_exit(s, p, a.fc, st, &a.sunc, nullptr, nullptr, &cone));
    if (!cone) cone_lock.unlock();
    if (stats) {
        a.stats = s->d_stats.get();
        VX_CHECK(stats_begin(s, (size_t)ST_COUNT * 64, st));
    }
    const int rc = launch_ortho(oa, fmt, st);
    if (rc) return set_error(VX_EDEVICE, std::string("ortho launch failed: ") + hipGetErrorString((hipError_t)rc));
    if (cone) cone_lock.unlock();   // enqueued: a recycle now waits for this render
    if (stats) {
        unsigned long long v[ST_COUNT];
        float ms = 0.0f;
        VX_CHECK(stats_end(s, v, ST_COUNT, st, &ms));
        fill_stats(stats, v, ms, pixel_bytes(fmt));
    }
    return VX_OK;
}

// vx_render_ortho's chunks, as aa_chunks: chunk c is rows [ss * y0, ss * (y0 + rows)) of the
// (ss*w) x (ss*h) orthographic frame, rendered compact into `scratch` and resolved right
// behind it into its rows of the w x h device frame d_out.  stats: the chunks' counters
// summed, their kernel times plus the resolves'.
static int ortho_chunks(vx_scene *s, const vx_frame_params *p, int w, int h, int fmt, const vx_aa_plan &plan, void *scratch,
                        void *d_out, hipStream_t st, vx_stats *stats) {
    const int ss = plan.ss, W = ss * w, H = ss * h;
    vx_stats sum;
    std::memset(&sum, 0, sizeof sum);
    for (int c = 0; c < plan.n_chunks; c++) {
        const int y0 = c * plan.chunk_rows_out, rows = std::min(plan.chunk_rows_out, h - y0);
        vx_stats cs;
        VX_CHECK(do_ortho(s, p, W, H, ss * y0, ss * rows, fmt, scratch, st, stats ? &cs : nullptr));
        if (stats) VX_HIP(hipEventRecord(s->ev0.get(), st));
        const int rc = launch_resolve(scratch, static_cast<char *>(d_out) + (size_t)y0 * w * pixel_bytes(fmt), w, rows, ss,
                                      W, fmt, st);
        if (rc) return set_error(VX_EDEVICE, std::string("resolve launch failed: ") + hipGetErrorString((hipError_t)rc));
        if (stats) {
            float ms = 0.0f;
            VX_HIP(hipEventRecord(s->ev1.get(), st));
            VX_HIP(hipEventSynchronize(s->ev1.get()));
            VX_HIP(hipEventElapsedTime(&ms, s->ev0.get(), s->ev1.get()));
            uint64_t *a = &sum.pixels;
            const uint64_t *b = &cs.pixels;
            for (size_t i = 0; i < offsetof(vx_stats, kernel_ms) / sizeof(uint64_t); i++) a[i] += b[i];
            sum.kernel_ms += cs.kernel_ms + (double)ms;
        }
    }
    if (stats) *stats = sum;
    return VX_OK;
}

extern "C" {

int vx_render_ortho(vx_scene *s, const vx_frame_params *p, int w, int h, int ss, int fmt, void *out, int out_on_device,
                    void *stream, size_t scratch_cap, vx_stats *stats) {
    // every check comes before the first GPU call
    if (!p || !out) return set_error(VX_EINVAL, "vx_render_ortho: null params or out");
    vx_aa_plan plan;
    VX_CHECK(vx_aa_plan_for(w, h, ss, fmt, scratch_cap, &plan));
    if (!s) return set_error(VX_EINVAL, "vx_render_ortho: null scene");
    VX_CHECK(check_ortho(p, ss * w, ss * h, fmt));
    const unsigned need = VX_FLAG_UNIT_GBUF | VX_FLAG_GLASS_SINGLE;
    if (!s->d_qface && (p->flags & need) != need)
        return set_error(VX_EINVAL, "this scene has no face table (it did not fit in device memory): its orthographic "
                                    "frames need VX_FLAG_UNIT_GBUF | VX_FLAG_GLASS_SINGLE");
    if (out_on_device && ((uintptr_t)out & (fmt == VX_PIXEL_RGBA32F ? 15u : 3u)))
        return set_error(VX_EINVAL, "vx_render_ortho: a device out must be aligned to 16 bytes (RGBA32F) or 4 (RGBA8)");
    VX_HIP(hipSetDevice(s->device));
    hipStream_t st = stream_of(s, stream);
    const size_t bytes = (size_t)w * h * pixel_bytes(fmt);
    void *scratch = nullptr, *d_out = out_on_device ? out : nullptr;
    int rc = VX_OK;
    hipError_t e = ss > 1 ? hipMallocAsync(&scratch, plan.scratch_bytes, st) : hipSuccess;
    if (e == hipSuccess && !out_on_device) e = hipMallocAsync(&d_out, bytes, st);
    if (e != hipSuccess) rc = set_error(VX_EDEVICE, std::string("vx_render_ortho: staging failed: ") + hipGetErrorString(e));
    if (rc == VX_OK)
        rc = ss > 1 ? ortho_chunks(s, p, w, h, fmt, plan, scratch, d_out, st, stats)
                    : do_ortho(s, p, w, h, 0, h, fmt, d_out, st, stats);
    if (rc == VX_OK && !out_on_device) {
        e = hipMemcpyAsync(out, d_out, bytes, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) rc = set_error(VX_EDEVICE, std::string("vx_render_ortho: readback failed: ") + hipGetErrorString(e));
    }
    if (scratch) (void)hipFreeAsync(scratch, st);
    if (!out_on_device) {
        if (d_out) (void)hipFreeAsync(d_out, st);
        (void)hipStreamSynchronize(st);
    }
    return rc;
}

int vx_render_aa(vx_scene *s, const vx_frame_params *p, int w, int h, int ss, int fmt, void *out, int out_on_device,
                 void *stream, size_t scratch_cap, vx_stats *stats) {
    // the argument checks need no scene and come first; none of them touches the GPU
    if (!p || !out) return set_error(VX_EINVAL, "vx_render_aa: null params or out");
    vx_aa_plan plan;
    VX_CHECK(vx_aa_plan_for(w, h, ss, fmt, scratch_cap, &plan));
    if (!s) return set_error(VX_EINVAL, "vx_render_aa: null scene");
    if (ss == 1) return vx_render(s, p, w, h, fmt, out, out_on_device, stream, stats);
    VX_CHECK(check_render(s, p, ss * w, ss * h, fmt));
    if (out_on_device && ((uintptr_t)out & (fmt == VX_PIXEL_RGBA32F ? 15u : 3u)))
        return set_error(VX_EINVAL, "vx_render_aa: a device out must be aligned to 16 bytes (RGBA32F) or 4 (RGBA8)");
    VX_HIP(hipSetDevice(s->device));
    hipStream_t st = stream_of(s, stream);
    const size_t bytes = (size_t)w * h * pixel_bytes(fmt);
    void *scratch = nullptr, *d_out = out_on_device ? out : nullptr;
    int rc = VX_OK;
    hipError_t e = hipMallocAsync(&scratch, plan.scratch_bytes, st);
    if (e == hipSuccess && !out_on_device) e = hipMallocAsync(&d_out, bytes, st);
    if (e != hipSuccess) rc = set_error(VX_EDEVICE, std::string("vx_render_aa: staging failed: ") + hipGetErrorString(e));
    if (rc == VX_OK) rc = aa_chunks(s, p, w, h, fmt, plan, 0, plan.n_chunks, scratch, d_out, st, stats);
    if (rc == VX_OK && !out_on_device) {
        e = hipMemcpyAsync(out, d_out, bytes, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) rc = set_error(VX_EDEVICE, std::string("vx_render_aa: readback failed: ") + hipGetErrorString(e));
    }
    if (scratch) (void)hipFreeAsync(scratch, st);
    if (!out_on_device) {
        if (d_out) (void)hipFreeAsync(d_out, st);
        (void)hipStreamSynchronize(st);
    }
    return rc;
}

void vx_scene_destroy(vx_scene *s) {
    if (!s) return;
    (void)hipSetDevice(s->device);
    if (s->stream) (void)hipStreamSynchronize(s->stream.get());
    delete s;   // the holders, in reverse order of declaration: the stream last
}

int vx_scene_create(const vx_scene_desc *d, vx_scene **out) {
    if (!d || !out) return set_error(VX_EINVAL, "vx_scene_create: null argument");
    *out = nullptr;
    SceneInputs in;
    VX_CHECK(scene_inputs(d, in));          // validation + container decode (vx_host.cpp)
    VX_HIP(hipSetDevice(d->device));
    vx_scene *s = new vx_scene();
    s->device = d->device;
    s->X = in.X; s->Y = in.Y; s->Z = in.Z;
    s->noise_w = in.NW; s->noise_h = in.NH; s->chunk = in.chunk;
    const FieldLayout &L = s->L = field_layout(in.X, in.Y, in.Z, in.cap);
    // the fp32 x/y index of the primary walk (do_render): its conditions on the field
    s->f32_scene = 4.0 * (double)L.Xp * (double)L.Yp < 8388608.0 && 32.0 * (double)L.texels < 4294967296.0 &&
                   L.Zp < (1 << 20);
    const int rc = build_scene(s, d, in);
    if (rc) vx_scene_destroy(s);
    else *out = s;
    return rc;
}

int vx_scene_vertex2d(const vx_scene *s, void *out, size_t cap, size_t *out_size) {
    if (!s || !out_size) return set_error(VX_EINVAL, "vx_scene_vertex2d: null argument");
    *out_size = vertex2d_bytes(s->quads2d, nullptr, 0);
    if (!out) return VX_OK;
    if (cap < *out_size) return set_error(VX_EINVAL, "vx_scene_vertex2d: output buffer too small");
    vertex2d_bytes(s->quads2d, static_cast<uint8_t *>(out), cap);
    return VX_OK;
}

int vx_scene_dims(const vx_scene *s, int dims[3]) {
    if (!s || !dims) return set_error(VX_EINVAL, "vx_scene_dims: null argument");
    dims[0] = s->X; dims[1] = s->Y; dims[2] = s->Z;
    return VX_OK;
}

int vx_scene_read_field(vx_scene *s, void *host_out, size_t cap) { return vx_scene_read_field_copy(s, 0, host_out, cap); }

int vx_scene_read_field_copy(vx_scene *s, int octant, void *host_out, size_t cap) {
    return read_copy(s, octant, host_out, cap, false, "vx_scene_read_field");
}

int vx_scene_read_boxes(vx_scene *s, int octant, void *host_out, size_t cap) {
    return read_copy(s, octant, host_out, cap, true, "vx_scene_read_boxes");
}

#ifdef VX_BLOCK_TIMING
// diagnostics build only: the last untiled launch's per-block (start, end) on the 100 MHz clock
int vx_debug_block_times(vx_scene *s, unsigned long long *out, size_t cap, size_t *n) {
    if (!s || !n) return set_error(VX_EINVAL, "vx_debug_block_times: null argument");
    *n = s->blk_n;
    if (!out || !s->d_blk) return VX_OK;
    VX_HIP(hipDeviceSynchronize());
    VX_HIP(hipMemcpy(out, s->d_blk.get(), 16 * std::min(cap / 2, s->blk_n), hipMemcpyDeviceToHost));
    return VX_OK;
}
#endif

int vx_scene_read_face_quads(vx_scene *s, void *host_out, size_t cap) {
    if (!s || !host_out) return set_error(VX_EINVAL, "vx_scene_read_face_quads: null argument");
    if (!s->d_qface) return set_error(VX_ENOMEM, "vx_scene_read_face_quads: the scene has no face table (it did not fit)");
    const size_t N = (size_t)s->X * s->Y * s->Z;
    if (cap < 12 * N) return set_error(VX_EINVAL, "vx_scene_read_face_quads: buffer too small");
    VX_HIP(hipSetDevice(s->device));
    DevBuf<uint16_t> tmp;
    VX_HIP(tmp.alloc(6 * N));
    hipError_t e = (hipError_t)launch_face_quads_interleave(s->d_qface.get(), tmp.get(), N, s->stream.get());
    if (e == hipSuccess) e = hipMemcpyAsync(host_out, tmp.get(), 12 * N, hipMemcpyDeviceToHost, s->stream.get());
    if (e == hipSuccess) e = hipStreamSynchronize(s->stream.get());
    if (e != hipSuccess) return set_error(VX_EDEVICE, std::string("vx_scene_read_face_quads: ") + hipGetErrorString(e));
    return VX_OK;
}

int vx_prepare_sun(vx_scene *s, const vx_frame_params *p, void *stream, vx_exit_info *info) {
    if (!s || !p) return set_error(VX_EINVAL, "vx_prepare_sun: null argument");
    VX_CHECK(check_frame(p, 64, 64, VX_PIXEL_RGBA8));
    VX_HIP(hipSetDevice(s->device));
    hipStream_t st = stream_of(s, stream);
    FrameConsts fc;
    const int max_steps = p->max_shadow_steps > 0 ? p->max_shadow_steps : 2 * s->Z;
    frame_consts(*p, 64, 64, s->X, s->Y, s->Z, max_steps, fc);
    const int8_t *sunc = nullptr;
    bool built = false;
    vx_scene::Cone *cone = nullptr;
    {
        // ev0 is recorded inside cone_copy right before the build's first packet:
        // build_ms is the copy's GPU time, not the host's allocation or waits
        std::lock_guard<std::mutex> lock(s->cone_mu);
        VX_CHECK(frame_exit(s, p, fc, st, &sunc, info, &built, &cone, s->ev0.get()));
        if (built) VX_HIP(hipEventRecord(s->ev1.get(), st));
    }
    VX_HIP(hipStreamSynchronize(st));
    if (info && built) {
        float ms = 0.0f;
        VX_HIP(hipEventElapsedTime(&ms, s->ev0.get(), s->ev1.get()));
        info->build_ms = ms;
    }
    return VX_OK;
}

int vx_render(vx_scene *s, const vx_frame_params *p, int w, int h, int fmt, void *out, int out_on_device,
              void *stream, vx_stats *stats) {
    VX_CHECK(check_render(s, p, w, h, fmt));
    if (!out) return set_error(VX_EINVAL, "vx_render: null output");
    VX_HIP(hipSetDevice(s->device));
    const size_t bytes = (size_t)w * h * pixel_bytes(fmt);
    hipStream_t st = stream_of(s, stream);
    if (out_on_device) return do_render(s, p, w, h, TileSpec(), fmt, out, st, stats);
    void *d_out = nullptr;
    VX_HIP(hipMallocAsync(&d_out, bytes, st));
    int rc = do_render(s, p, w, h, TileSpec(), fmt, d_out, st, stats);
    if (rc == VX_OK) {
        hipError_t e = hipMemcpyAsync(out, d_out, bytes, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) rc = set_error(VX_EDEVICE, std::string("readback failed: ") + hipGetErrorString(e));
    }
    (void)hipFreeAsync(d_out, st);
    (void)hipStreamSynchronize(st);
    return rc;
}

int vx_query_rays(vx_scene *s, const vx_ray *rays, int n, vx_ray_hit *hits, int on_device, void *stream,
                  vx_query_stats *stats) {
    if (!s || !rays || !hits) return set_error(VX_EINVAL, "vx_query_rays: null argument");
    if (n < 0 || n > VX_MAX_QUERY_RAYS) return set_error(VX_EINVAL, "vx_query_rays: n out of range (0 .. 2^26)");
    if (on_device && (((uintptr_t)rays & 15u) || ((uintptr_t)hits & 3u)))
        return set_error(VX_EINVAL, "vx_query_rays: device rays must be 16-byte aligned, hits 4-byte");
    if (stats) std::memset(stats, 0, sizeof *stats);
    if (n == 0) return VX_OK;
    VX_HIP(hipSetDevice(s->device));
    hipStream_t st = stream_of(s, stream);
    if (on_device) return do_query(s, rays, n, hits, st, stats);
    const size_t rb = (size_t)n * sizeof(vx_ray), hb = (size_t)n * sizeof(vx_ray_hit);
    void *d_r = nullptr, *d_h = nullptr;
    int rc = VX_OK;
    hipError_t e = hipMallocAsync(&d_r, rb, st);
    if (e == hipSuccess) e = hipMallocAsync(&d_h, hb, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d_r, rays, rb, hipMemcpyHostToDevice, st);
    if (e != hipSuccess) rc = set_error(VX_EDEVICE, std::string("query staging failed: ") + hipGetErrorString(e));
    if (rc == VX_OK) rc = do_query(s, d_r, n, d_h, st, stats);
    if (rc == VX_OK) {
        e = hipMemcpyAsync(hits, d_h, hb, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) rc = set_error(VX_EDEVICE, std::string("query readback failed: ") + hipGetErrorString(e));
    }
    if (d_r) (void)hipFreeAsync(d_r, st);
    if (d_h) (void)hipFreeAsync(d_h, st);
    (void)hipStreamSynchronize(st);
    return rc;
}

int vx_query_sun(vx_scene *s, const vx_sun_point *points, int n, const float (*suns)[3], int k, int max_steps,
                 uint32_t flags, uint32_t *out, int on_device, void *stream, vx_sun_stats *stats) {
    if (!s) return set_error(VX_EINVAL, "vx_query_sun: null scene");
    VX_CHECK(check_sun_query(points, n, suns, k, flags, out, on_device));
    if (stats) std::memset(stats, 0, sizeof *stats);
    if (n == 0) return VX_OK;
    VX_HIP(hipSetDevice(s->device));
    hipStream_t st = stream_of(s, stream);
    // the suns as the kernel reads them (sun_query_entry), uploaded stream-ordered per call.  The table is
    // pageable host memory: hipMemcpyAsync returns once it has taken the source's bytes, so it may go with
    // this call
    std::vector<SunQ> table((size_t)k);
    for (int j = 0; j < k; j++) sun_query_entry(suns[j], table[(size_t)j]);
    const size_t qb = (size_t)k * sizeof(SunQ), pb = (size_t)n * sizeof(vx_sun_point),
                 ob = (size_t)n * VX_SUN_WORDS(k) * sizeof(uint32_t);
    void *d_q = nullptr, *d_p = nullptr, *d_o = nullptr;
    int rc = VX_OK;
    hipError_t e = hipMallocAsync(&d_q, qb, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d_q, table.data(), qb, hipMemcpyHostToDevice, st);
    if (e == hipSuccess && !on_device) {
        e = hipMallocAsync(&d_p, pb, st);
        if (e == hipSuccess) e = hipMallocAsync(&d_o, ob, st);
        if (e == hipSuccess) e = hipMemcpyAsync(d_p, points, pb, hipMemcpyHostToDevice, st);
    }
    if (e != hipSuccess) rc = set_error(VX_EDEVICE, std::string("sun query staging failed: ") + hipGetErrorString(e));
    if (rc == VX_OK)
        rc = do_sun_query(s, on_device ? points : d_p, n, static_cast<const SunQ *>(d_q), k, max_steps, flags,
                          on_device ? out : static_cast<uint32_t *>(d_o), st, stats);
    if (rc == VX_OK && !on_device) {
        e = hipMemcpyAsync(out, d_o, ob, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) rc = set_error(VX_EDEVICE, std::string("sun query readback failed: ") + hipGetErrorString(e));
    }
    if (d_q) (void)hipFreeAsync(d_q, st);
    if (d_p) (void)hipFreeAsync(d_p, st);
    if (d_o) (void)hipFreeAsync(d_o, st);
    if (!on_device || rc != VX_OK) (void)hipStreamSynchronize(st);
    return rc;
}

int vx_render_gbuffer(vx_scene *s, const vx_frame_params *p, int w, int h, const vx_gbuffer_planes *out,
                      int out_on_device, void *stream, vx_query_stats *stats) {
    if (!s || !p || !out) return set_error(VX_EINVAL, "vx_render_gbuffer: null argument");
    if (!out->depth && !out->opaque_depth && !out->surface)
        return set_error(VX_EINVAL, "vx_render_gbuffer: no plane asked for");
    VX_CHECK(check_frame_size(w, h));
    if ((long long)w * h > VX_MAX_QUERY_RAYS)
        return set_error(VX_EINVAL, "vx_render_gbuffer: w * h above VX_MAX_QUERY_RAYS (2^26)");
    if (p->quality == 0)
        return set_error(VX_EINVAL, "vx_render_gbuffer: quality 0 (the 2D frame) draws another mesh; no planes for it");
    VX_CHECK(check_camera(p));
    void *const planes[3] = {out->depth, out->opaque_depth, out->surface};
    if (out_on_device)
        for (void *q : planes)
            if ((uintptr_t)q & 3u) return set_error(VX_EINVAL, "vx_render_gbuffer: device planes must be 4-byte aligned");
    if (stats) std::memset(stats, 0, sizeof *stats);
    VX_HIP(hipSetDevice(s->device));
    hipStream_t st = stream_of(s, stream);
    if (out_on_device) return do_gbuffer(s, p, w, h, *out, st, stats);
    // host planes: one stream-ordered allocation holds the wanted ones back to back
    const size_t plane = (size_t)w * h * 4;
    int wanted = 0;
    for (void *q : planes) wanted += q ? 1 : 0;
    void *d_all = nullptr;
    VX_HIP(hipMallocAsync(&d_all, plane * wanted, st));
    void *d_planes[3] = {nullptr, nullptr, nullptr};
    for (int k = 0, at = 0; k < 3; k++)
        if (planes[k]) d_planes[k] = static_cast<char *>(d_all) + plane * at++;
    const vx_gbuffer_planes dev = {(float *)d_planes[0], (float *)d_planes[1], (uint32_t *)d_planes[2]};
    int rc = do_gbuffer(s, p, w, h, dev, st, stats);
    if (rc == VX_OK) {
        hipError_t e = hipSuccess;
        for (int k = 0; k < 3 && e == hipSuccess; k++)
            if (planes[k]) e = hipMemcpyAsync(planes[k], d_planes[k], plane, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) rc = set_error(VX_EDEVICE, std::string("gbuffer readback failed: ") + hipGetErrorString(e));
    }
    (void)hipFreeAsync(d_all, st);
    (void)hipStreamSynchronize(st);
    return rc;
}

int vx_render_tiles(vx_scene *s, const vx_frame_params *p, int w, int h, int ts, const int *tile_ids, int n_tiles,
                    int fmt, void *out_device, void *stream, vx_stats *stats) {
    VX_CHECK(check_render(s, p, w, h, fmt));
    if (ts <= 0 || ts % VX_TILE_ALIGN_X) return set_error(VX_EINVAL, "tile_size must be a positive multiple of 32");
    if (!tile_ids || n_tiles <= 0 || !out_device) return set_error(VX_EINVAL, "vx_render_tiles: empty tile list");
    const int tx = (w + ts - 1) / ts, ty = (h + ts - 1) / ts;
    VX_CHECK(check_ids(tile_ids, n_tiles, tx * ty, "tile id out of range"));
    if ((unsigned long long)n_tiles * (unsigned long long)ts * (unsigned long long)ts >= (1ull << 32))
        return set_error(VX_EINVAL, "vx_render_tiles: the compact output must hold fewer than 2^32 pixels");
    VX_HIP(hipSetDevice(s->device));
    hipStream_t st = stream_of(s, stream);
    ListRef lr;
    VX_CHECK(list_acquire(s, st, tile_ids, n_tiles, lr));
    TileSpec t;
    t.tw = t.th = t.pitch = ts;
    t.tiles_x = tx;
    t.ids = lr.b->d.get();
    t.n = n_tiles;
    return do_render(s, p, w, h, t, fmt, out_device, st, stats, &lr);
}

int vx_render_bands(vx_scene *s, const vx_frame_params *p, int w, int h, int band_rows, const int *band_ids,
                    int n_bands, int fmt, void *out_device, int inplace, void *stream, vx_stats *stats) {
    VX_CHECK(check_render(s, p, w, h, fmt));
    if (band_rows <= 0 || band_rows % VX_TILE_ALIGN_Y)
        return set_error(VX_EINVAL, "band_rows must be a positive multiple of 8");
    if (!band_ids || n_bands <= 0 || !out_device) return set_error(VX_EINVAL, "vx_render_bands: empty band list");
    VX_CHECK(check_ids(band_ids, n_bands, (h + band_rows - 1) / band_rows, "band id out of range"));
    VX_HIP(hipSetDevice(s->device));
    hipStream_t st = stream_of(s, stream);
    if (!inplace && (unsigned long long)n_bands * (unsigned long long)band_rows * (unsigned long long)w >= (1ull << 32))
        return set_error(VX_EINVAL, "vx_render_bands: the compact output must hold fewer than 2^32 pixels");
    ListRef lr;
    VX_CHECK(list_acquire(s, st, band_ids, n_bands, lr));
    TileSpec t;
    t.tw = (w + VX_TILE_ALIGN_X - 1) / VX_TILE_ALIGN_X * VX_TILE_ALIGN_X;   // one tile spans the row
    t.th = band_rows;
    t.pitch = w;                      // compact bands keep the frame's row pitch
    t.tiles_x = 1;
    t.inplace = inplace ? 1 : 0;
    t.ids = lr.b->d.get();
    t.n = n_bands;
    return do_render(s, p, w, h, t, fmt, out_device, st, stats, &lr);
}

int vx_detile(vx_scene *s, int w, int h, int ts, const int *tile_ids, int n_tiles, int fmt, const void *tiles_device,
              void *frame_device, void *stream) {
    if (!s || !tile_ids || !tiles_device || !frame_device || ts <= 0 || n_tiles <= 0)
        return set_error(VX_EINVAL, "vx_detile: bad arguments");
    if (w <= 0 || h <= 0 || w > 32768 || h > 32768) return set_error(VX_EINVAL, "vx_detile: frame size out of range");
    if (fmt != VX_PIXEL_RGBA32F && fmt != VX_PIXEL_RGBA8) return set_error(VX_EINVAL, "vx_detile: unknown pixel format");
    if (ts % VX_TILE_ALIGN_X) return set_error(VX_EINVAL, "vx_detile: tile_size must be a positive multiple of 32");
    const int tx = (w + ts - 1) / ts, ty = (h + ts - 1) / ts;
    VX_CHECK(check_ids(tile_ids, n_tiles, tx * ty, "vx_detile: tile id out of range"));
    VX_HIP(hipSetDevice(s->device));
    hipStream_t st = stream_of(s, stream);
    ListRef lr;
    VX_CHECK(list_acquire(s, st, tile_ids, n_tiles, lr));
    const int rc = launch_detile(tiles_device, frame_device, w, h, ts, tx, lr.b->d.get(), n_tiles, fmt, st);
    if (rc) return set_error(VX_EDEVICE, std::string("detile failed: ") + hipGetErrorString((hipError_t)rc));
    return VX_OK;
}

int vx_field_build_gpu(const uint8_t *color, int X, int Y, int Z, uint8_t *rgba_out, int device) {
    if (!color || !rgba_out || X <= 0 || Y <= 0 || Z <= 0 || X > 65535 || Y > 65535 || Z > 255)
        return set_error(VX_EINVAL, "vx_field_build_gpu: bad arguments (need 0<X,Y<=65535, 0<Z<=255)");
    const size_t N = (size_t)X * Y * Z;
    if (N > (size_t)INT32_MAX) return set_error(VX_EINVAL, "vx_field_build_gpu: grid too large for int32 volume sums");
    VX_HIP(hipSetDevice(device));
    Stream st;   // declared first: destroyed after the buffers
    DevBuf<uint32_t> d_rgba;
    DevBuf<uint8_t> d_col;
    hipError_t e = st.create();
    if (e == hipSuccess) e = d_col.alloc(N);
    if (e == hipSuccess) e = d_rgba.alloc(N);
    if (e == hipSuccess) e = hipMemcpyAsync(d_col.get(), color, N, hipMemcpyHostToDevice, st.get());
    if (e == hipSuccess) e = (hipError_t)field_build_device(d_col.get(), d_rgba.get(), X, Y, Z, st.get());
    if (e == hipSuccess) e = hipMemcpyAsync(rgba_out, d_rgba.get(), 4 * N, hipMemcpyDeviceToHost, st.get());
    if (e == hipSuccess) e = hipStreamSynchronize(st.get());
    if (e != hipSuccess) return set_error(VX_EDEVICE, std::string("vx_field_build_gpu: ") + hipGetErrorString(e));
    return VX_OK;
}

}  // extern "C"
