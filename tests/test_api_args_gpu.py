"""The argument checks of the device entry points, through the ctypes ABI: each
bad call returns its code and leaves its own text in vx_last_error(), and leaves
nothing behind -- a correct frame renders afterwards, and a scene destroyed and
created again renders the same bytes.  One 8 x 8 x 4 scene, nothing above a
64 x 64 frame."""
import ctypes as C

import numpy as np
import pytest

from gpu_rig import need_gpu  # noqa: F401 (an autouse fixture)

pytestmark = pytest.mark.gpu

X, Y, Z = 8, 8, 4
W = H = 64
N = X * Y * Z


def _grid():
    g = np.random.default_rng(11).integers(0, 22, (Z, Y, X)).astype(np.uint8)   # 0 air, 1..20 colours, 21 glass
    g[np.random.default_rng(12).random((Z, Y, X)) < 0.5] = 0
    return g


def _create(L):
    from voxmap_amd import _abi
    g = _grid()
    d = _abi.SceneDesc()
    d.map_bytes = g.ctypes.data
    d.map_size = g.nbytes
    d.map_format = _abi.FORMAT_GRID
    d.noise_w = d.noise_h = 64          # no noise given: synthesised
    d.X, d.Y, d.Z = X, Y, Z
    h = C.c_void_p()
    assert L.vx_scene_create(C.byref(d), C.byref(h)) == 0, L.vx_last_error()
    return h


class Ctx:
    def __init__(self):
        import torch

        import voxmap_amd as vx
        from voxmap_amd import _abi
        self.L = _abi.lib()
        self.h = _create(self.L)
        self.p = vx.make_frame((4.0, 4.0, 6.0), (1.0, 0.0, 0.5), W, H).params
        self.buf = torch.zeros(W * H * 4, dtype=torch.uint8, device="cuda")       # a 64 x 64 RGBA8 frame
        self.buf2 = torch.zeros(W * H * 4, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        self.out = C.c_void_p(self.buf.data_ptr())
        self.out2 = C.c_void_p(self.buf2.data_ptr())

    def err(self):
        return self.L.vx_last_error().decode()


@pytest.fixture(scope="module")
def ctx():
    c = Ctx()
    yield c
    c.L.vx_scene_destroy(c.h)


def _ids(*v):
    return (C.c_int * max(len(v), 1))(*v)


def _bad(c, rc, text):
    from voxmap_amd import _abi
    assert rc == _abi.VX_EINVAL, (rc, c.err())
    assert text in c.err(), c.err()


@pytest.mark.parametrize("ts", [0, 48])
def test_tiles_tile_size(ctx, ts):
    rc = ctx.L.vx_render_tiles(ctx.h, C.byref(ctx.p), W, H, ts, _ids(0), 1, 1, ctx.out, None, None)
    _bad(ctx, rc, "tile_size must be a positive multiple of 32")


@pytest.mark.parametrize("ids,n", [(None, 1), (_ids(0), 0)])
def test_tiles_empty_list(ctx, ids, n):
    rc = ctx.L.vx_render_tiles(ctx.h, C.byref(ctx.p), W, H, 32, ids, n, 1, ctx.out, None, None)
    _bad(ctx, rc, "vx_render_tiles: empty tile list")


@pytest.mark.parametrize("tid", [-1, 4])          # 64 x 64 in 32 x 32 tiles: ids 0..3
def test_tiles_id_range(ctx, tid):
    rc = ctx.L.vx_render_tiles(ctx.h, C.byref(ctx.p), W, H, 32, _ids(0, tid), 2, 1, ctx.out, None, None)
    _bad(ctx, rc, "tile id out of range")
    assert not ctx.err().startswith("vx_detile")


@pytest.mark.parametrize("rows", [0, 12])
def test_bands_rows(ctx, rows):
    rc = ctx.L.vx_render_bands(ctx.h, C.byref(ctx.p), W, H, rows, _ids(0), 1, 1, ctx.out, 1, None, None)
    _bad(ctx, rc, "band_rows must be a positive multiple of 8")


def test_bands_empty_list(ctx):
    rc = ctx.L.vx_render_bands(ctx.h, C.byref(ctx.p), W, H, 16, _ids(0), 0, 1, ctx.out, 1, None, None)
    _bad(ctx, rc, "vx_render_bands: empty band list")


@pytest.mark.parametrize("bid", [-1, 4])          # 64 rows in bands of 16: ids 0..3
def test_bands_id_range(ctx, bid):
    rc = ctx.L.vx_render_bands(ctx.h, C.byref(ctx.p), W, H, 16, _ids(0, bid), 2, 1, ctx.out, 1, None, None)
    _bad(ctx, rc, "band id out of range")


def test_detile_null(ctx):
    L = ctx.L
    _bad(ctx, L.vx_detile(None, W, H, 32, _ids(0), 1, 1, ctx.out, ctx.out2, None), "vx_detile: bad arguments")
    _bad(ctx, L.vx_detile(ctx.h, W, H, 32, None, 1, 1, ctx.out, ctx.out2, None), "vx_detile: bad arguments")
    _bad(ctx, L.vx_detile(ctx.h, W, H, 32, _ids(0), 1, 1, None, ctx.out2, None), "vx_detile: bad arguments")
    _bad(ctx, L.vx_detile(ctx.h, W, H, 32, _ids(0), 1, 1, ctx.out, None, None), "vx_detile: bad arguments")


def test_detile_frame_size(ctx):
    rc = ctx.L.vx_detile(ctx.h, 0, H, 32, _ids(0), 1, 1, ctx.out, ctx.out2, None)
    _bad(ctx, rc, "vx_detile: frame size out of range")


def test_detile_format(ctx):
    rc = ctx.L.vx_detile(ctx.h, W, H, 32, _ids(0), 1, 7, ctx.out, ctx.out2, None)
    _bad(ctx, rc, "vx_detile: unknown pixel format")


def test_detile_tile_size(ctx):
    rc = ctx.L.vx_detile(ctx.h, W, H, 48, _ids(0), 1, 1, ctx.out, ctx.out2, None)
    _bad(ctx, rc, "vx_detile: tile_size must be a positive multiple of 32")


@pytest.mark.parametrize("tid", [-1, 4])
def test_detile_id_range(ctx, tid):
    rc = ctx.L.vx_detile(ctx.h, W, H, 32, _ids(0, tid), 2, 1, ctx.out, ctx.out2, None)
    _bad(ctx, rc, "vx_detile: tile id out of range")


@pytest.mark.parametrize("fn,what", [("vx_scene_read_field_copy", "vx_scene_read_field"),
                                     ("vx_scene_read_boxes", "vx_scene_read_boxes")])
def test_read_copy(ctx, fn, what):
    host = np.zeros(4 * N, np.uint8)
    f = getattr(ctx.L, fn)
    _bad(ctx, f(ctx.h, 8, host.ctypes.data, host.nbytes), what + ": octant must be 0..7")
    _bad(ctx, f(ctx.h, 0, host.ctypes.data, host.nbytes - 1), what + ": buffer too small")
    assert f(ctx.h, 7, host.ctypes.data, host.nbytes) == 0, ctx.err()


def test_read_face_quads_short(ctx):
    host = np.zeros(12 * N, np.uint8)
    rc = ctx.L.vx_scene_read_face_quads(ctx.h, host.ctypes.data, host.nbytes - 1)
    _bad(ctx, rc, "vx_scene_read_face_quads: buffer too small")
    assert ctx.L.vx_scene_read_face_quads(ctx.h, host.ctypes.data, host.nbytes) == 0, ctx.err()


def test_query_args(ctx):
    import torch
    from voxmap_amd import _abi
    rays = torch.zeros(4 * C.sizeof(_abi.Ray) + 16, dtype=torch.uint8, device="cuda")
    hits = torch.zeros(4 * C.sizeof(_abi.RayHit), dtype=torch.uint8, device="cuda")
    r, h = rays.data_ptr(), hits.data_ptr()
    assert r % 16 == 0
    _bad(ctx, ctx.L.vx_query_rays(ctx.h, C.c_void_p(r), -1, C.c_void_p(h), 1, None, None), "n out of range")
    _bad(ctx, ctx.L.vx_query_rays(ctx.h, C.c_void_p(r + 4), 4, C.c_void_p(h), 1, None, None), "16-byte aligned")


def test_render_null_output(ctx):
    rc = ctx.L.vx_render(ctx.h, C.byref(ctx.p), W, H, 1, None, 1, None, None)
    _bad(ctx, rc, "vx_render: null output")


def _render(c, h):
    import torch
    c.buf.zero_()
    torch.cuda.synchronize()
    assert c.L.vx_render(h, C.byref(c.p), W, H, 1, c.out, 1, None, None) == 0, c.err()
    torch.cuda.synchronize()
    return c.buf.cpu().numpy().reshape(H, W * 4).copy()


def test_frame_after_errors(ctx):
    """After every error case above: a correct frame, and one band of it in
    place, return VX_OK; the band's rows equal the frame's and the others stay."""
    import torch
    full = _render(ctx, ctx.h)
    assert full.any()
    ctx.buf2.zero_()
    torch.cuda.synchronize()
    rc = ctx.L.vx_render_bands(ctx.h, C.byref(ctx.p), W, H, 16, _ids(2), 1, 1, ctx.out2, 1, None, None)
    assert rc == 0, ctx.err()
    torch.cuda.synchronize()
    band = ctx.buf2.cpu().numpy().reshape(H, W * 4)
    assert np.array_equal(band[32:48], full[32:48])
    assert not band[:32].any() and not band[48:].any()


def test_destroy_and_create_again(ctx):
    """A scene destroyed and created again from the same grid renders the same bytes."""
    frames = []
    for _ in range(2):
        h = _create(ctx.L)
        frames.append(_render(ctx, h))
        ctx.L.vx_scene_destroy(h)
    assert np.array_equal(frames[0], frames[1])
    assert np.array_equal(frames[0], _render(ctx, ctx.h))
