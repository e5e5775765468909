"""Ray queries, the host half (no GPU): vx_pixel_ray against the oracle's pixel
direction, vx_place_rays against a numpy float64 restatement of drawOverlay's
projection (map.js:117-137, math.js m4.v4), vx_query_rays' argument checks, the
struct layouts, and the k_query kernel's resources in the built library."""
import ctypes as C
import math
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CAMERAS = [((48.0, 24.0, 18.0), (1.1, 0.0, 0.6)), ((-6.25, 32.5, 9.0), (1.45, 0.0, -math.pi / 2))]


def _u32(a):
    return np.asarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("sbj,rot", CAMERAS)
@pytest.mark.parametrize("w,h", [(7, 5), (96, 64)])
def test_pixel_ray_is_the_oracles_pixel_dir(built, sbj, rot, w, h):
    import oracle
    import voxmap_amd as vx
    fr = vx.make_frame(sbj, rot, w, h)
    L = oracle.lib()
    d = (C.c_float * 3)()
    for py in range(h):
        for px in range(w):
            r = vx.pixel_ray(fr, px, py)
            L.vxo_pixel_dir(C.addressof(fr.params), w, h, px, py, d)
            assert (_u32(r["dir"]) == _u32(list(d))).all(), (px, py)
            assert list(r["cell"]) == list(fr.params.cam_cell)
            assert (_u32(r["fract"]) == _u32(list(fr.params.cam_fract))).all()
            assert r["t_max"] == np.inf and not r["reserved"].any()


def test_pixel_ray_rejects_out_of_range(built):
    import voxmap_amd as vx
    fr = vx.make_frame(*CAMERAS[0], 96, 64)
    for px, py, w, h in [(-1, 0, 96, 64), (0, -1, 96, 64), (96, 0, 96, 64), (0, 64, 96, 64), (0, 0, 0, 64),
                         (0, 0, 96, 0), (0, 0, -3, 64), (0, 0, 40000, 64)]:
        with pytest.raises(vx.VoxmapError) as e:
            vx.pixel_ray(vx.Frame(fr.params, w, h), px, py)
        assert e.value.code == -1


def _projection(w, h, sbj, rot):
    """cam.projection_matrix of map.js:373-391 (float64), column-major, and the camera position."""
    def T(x, y, z):
        m = np.eye(4)
        m[:3, 3] = (x, y, z)
        return m

    def Rx(t):
        c, s = math.cos(t), math.sin(t)
        return np.array([[1, 0, 0, 0], [0, c, -s, 0], [0, s, c, 0], [0, 0, 0, 1.0]])

    def Rz(t):
        c, s = math.cos(t), math.sin(t)
        return np.array([[c, -s, 0, 0], [s, c, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1.0]])

    orbit = T(*sbj) @ Rz(rot[2]) @ Rx(rot[0]) @ T(0, 0, sbj[2])
    pos = orbit[:3, 3].copy()
    f, a = 1.0 / math.tan(math.radians(60) / 2), w / h
    near, far = 1.0, 1000.0                         # math.js:37-42 (with its sqrt(ratio) quirk)
    P = np.array([[f / math.sqrt(a), 0, 0, 0], [0, f * math.sqrt(a), 0, 0],
                  [0, 0, (near + far) / (near - far), 2 * near * far / (near - far)], [0, 0, -1, 0.0]])
    view = Rx(-rot[0]) @ Rz(-rot[2]) @ T(*(-pos))
    return (P @ view).T.reshape(-1).astype(np.float32), pos    # column-major, as u_matrix (float32)


def _overlay_ref(m, cam, place):
    """map.js:117-137 with math.js:106-135 (m4.v4) and :22-29 (vec), float64, as the page runs it."""
    m = [float(v) for v in m]
    v1, v2, v3, v4 = float(place[0]), float(place[1]), float(place[2]), 1.0
    view = [m[r] * v1 + m[4 + r] * v2 + m[8 + r] * v3 + m[12 + r] * v4 for r in range(4)]
    w = view[3]
    with np.errstate(all="ignore"):
        x, y = np.float64(view[0]) / np.float64(w), np.float64(view[1]) / np.float64(w)
    on = not (w < 0) and not (abs(x) > 1.1) and not (abs(y) > 1.1)
    acc = 0.0
    for i in range(3):
        b = float(place[i]) - float(cam[i])
        acc = acc + b * b
    return x, y, w, math.sqrt(acc), on


def test_place_rays_restates_draw_overlay(built):
    import voxmap_amd as vx
    w, h = 1280, 720
    sbj, rot = (48.0, 24.0, 18.0), (1.1, 0.0, 0.6)
    m, cam = _projection(w, h, sbj, rot)
    fr = vx.frame_from_matrix(m, cam)
    fwd = np.array(fr.ray_fwd[:], np.float64)
    right = np.array(fr.ray_right[:], np.float64)
    # in front, behind (w < 0), and beside the camera: |ndc_x| just inside and just outside 1.1
    # (ray_right is the offset of ndc_x = 1 at unit forward distance)
    places = [cam + 30 * fwd, cam - 12 * fwd, cam + 20 * (fwd + 1.0999 * right), cam + 20 * (fwd + 1.1001 * right),
              cam + 20 * (fwd - 1.0999 * right), cam + 20 * (fwd - 1.1001 * right), (50.25, 20.5, 3.0), cam + 0.5 * fwd]
    views, rays = vx.place_rays(m, cam, places)
    assert views.dtype == vx.PLACE_VIEW_DTYPE and rays.dtype == vx.RAY_DTYPE and len(views) == len(rays) == len(places)
    kinds = []
    for k, pl in enumerate(places):
        x, y, ww, dist, on = _overlay_ref(m, cam, pl)
        assert views["ndc_x"][k] == np.float32(x) and views["ndc_y"][k] == np.float32(y)
        assert views["w"][k] == np.float32(ww) and views["distance"][k] == np.float32(dist)
        assert bool(views["on_screen"][k]) == on, k
        kinds.append((ww < 0, on))
        want = np.asarray(pl, np.float64) - np.asarray(cam, np.float64)
        assert (_u32(rays["dir"][k]) == _u32(want.astype(np.float32))).all()
        assert rays["t_max"][k] == 1.0 and not rays["reserved"][k].any()
        assert list(rays["cell"][k]) == list(fr.cam_cell) and (_u32(rays["fract"][k]) == _u32(fr.cam_fract[:])).all()
    # the cases are what they claim to be
    assert kinds[0] == (False, True) and kinds[1] == (True, False)
    assert [k[1] for k in kinds[2:6]] == [True, False, True, False]
    assert abs(abs(views["ndc_x"][2]) - 1.1) < 1e-3 and abs(abs(views["ndc_x"][3]) - 1.1) < 1e-3
    # a fract within 2^-25 of 1 moves to the next cell, as frame_from_matrix does
    cam2 = (10.0 - 2.0 ** -30, 3.5, 7.25)
    _, r2 = vx.place_rays(m, cam2, [(1.0, 2.0, 3.0)])
    f2 = vx.frame_from_matrix(m, cam2)
    assert list(r2["cell"][0]) == list(f2.cam_cell) == [10, 3, 7] and r2["fract"][0][0] == 0.0
    # no places: empty arrays
    v0, r0 = vx.place_rays(m, cam, np.zeros((0, 3)))
    assert len(v0) == 0 and len(r0) == 0


def test_query_rays_argument_errors_do_not_touch_the_gpu(built):
    """Checked before any HIP call: the scene handle below is not a scene, and no GPU is needed."""
    import voxmap_amd as vx
    from voxmap_amd import _abi
    L = vx.lib()
    rays = np.zeros(4, vx.RAY_DTYPE)
    hits = np.zeros(4, vx.HIT_DTYPE)
    fake = C.create_string_buffer(4096)             # never dereferenced: every call fails its argument check
    scene = C.cast(fake, C.c_void_p)
    cases = [(None, rays.ctypes.data, 4, hits.ctypes.data, 0), (scene, None, 4, hits.ctypes.data, 0),
             (scene, rays.ctypes.data, 4, None, 0), (scene, rays.ctypes.data, -1, hits.ctypes.data, 0),
             (scene, rays.ctypes.data, (1 << 26) + 1, hits.ctypes.data, 0),
             (scene, rays.ctypes.data, -1, hits.ctypes.data, 1), (scene, None, 0, None, 1),
             (scene, rays.ctypes.data + 4, 2, hits.ctypes.data, 1)]      # device rays not 16-byte aligned
    for sc, r, n, hh, dev in cases:
        st = _abi.QueryStats()
        rc = L.vx_query_rays(sc, r, n, hh, dev, None, C.byref(st))
        assert rc == _abi.VX_EINVAL, (n, dev, rc)
        assert b"vx_query_rays" in L.vx_last_error()
    assert not hits.view(np.uint8).any()
    # n == 0 is fine and does nothing (no HIP call either: this machine may have no GPU)
    assert L.vx_query_rays(scene, rays.ctypes.data, 0, hits.ctypes.data, 0, None, None) == 0
    assert _abi.MAX_QUERY_RAYS == 1 << 26 and _abi.RAY_INVALID == -1


def test_struct_layouts():
    import voxmap_amd as vx
    from voxmap_amd import _abi
    assert C.sizeof(_abi.Ray) == 48 == vx.RAY_DTYPE.itemsize
    assert C.sizeof(_abi.RayHit) == 88 == vx.HIT_DTYPE.itemsize
    assert C.sizeof(_abi.Surface) == 40 == vx.SURFACE_DTYPE.itemsize
    assert C.sizeof(_abi.PlaceView) == 20 == vx.PLACE_VIEW_DTYPE.itemsize
    assert C.sizeof(_abi.QueryStats) == 56
    for st, dt in [(_abi.Ray, vx.RAY_DTYPE), (_abi.Surface, vx.SURFACE_DTYPE), (_abi.RayHit, vx.HIT_DTYPE),
                   (_abi.PlaceView, vx.PLACE_VIEW_DTYPE)]:
        assert [n for n, _ in st._fields_] == list(dt.names)
        for name, _ in st._fields_:
            assert getattr(st, name).offset == dt.fields[name][1], (st.__name__, name)
    header = open(os.path.join(ROOT, "include", "voxmap.h")).read()
    assert "#define VX_ABI_VERSION 10" in header


def test_hits_visible_rule():
    import voxmap_amd as vx
    h = np.zeros(6, vx.HIT_DTYPE)
    h["n"] = [-1, 0, 1, 1, 2, 2]
    h["s"]["id"][:, 0] = [0, 0, 0, 2, 2, 2]       # records past n are ignored
    h["s"]["id"][:, 1] = [0, 0, 0, 0, 0, 2]
    assert vx.hits_visible(h).tolist() == [True, True, False, True, False, True]


def test_k_query_kernel_resources(built):
    """k_query is in the library, keeps its arguments out of scratch, and its unit holds no render kernel."""
    import subprocess
    import tempfile

    from voxmap_amd import _abi, kernel_meta
    ks = kernel_meta.kernels(_abi.LIB_PATH)
    q = {k: v for k, v in ks.items() if "k_query" in k}
    assert len(q) == 2, sorted(q)                    # with and without counters
    for name, v in q.items():
        assert "k_render" not in name
        assert v["private_segment_fixed_size"] <= kernel_meta.RENDER_SCRATCH_LIMIT, (name, v)
        assert v.get("vgpr_spill_count", 0) == 0, (name, v)
    # the code object that holds k_query holds no k_render kernel
    with tempfile.TemporaryDirectory() as d:
        found = 0
        for co in kernel_meta.code_objects(_abi.LIB_PATH, d):
            notes = subprocess.run([kernel_meta._tool("llvm-readelf"), "--notes", co], check=True,
                                   capture_output=True, text=True).stdout
            if "k_query" in notes:
                found += 1
                assert "k_render" not in notes
        assert found == 1
