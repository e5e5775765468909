"""The frame's depth and surface planes on the GPU (vx_render_gbuffer / k_gbuffer).

The reference per pixel is the scalar oracle: Oracle.primary(params with flags =
VX_FLAG_UNIT_GBUF, Oracle.pixel_dir(...)); the sky record the oracle returns
behind glass (t = inf) is dropped, as tests/test_query_gpu.py's reference does.
The float planes are compared as uint32 words.  Scenes and cameras are that
file's.  The header defines the planes through vx_query_rays over vx_pixel_ray,
so the second reference is that call on the same GPU.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from gpu_rig import Rig, need_gpu, with_flags  # noqa: F401 (need_gpu: an autouse fixture)
from test_query_gpu import CAMS, GLASS, ODD_DIMS, World, _split

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF_BITS = np.float32(np.inf).view(np.uint32)
PLANES = ("depth", "opaque_depth", "surface")
SUBSETS = [tuple(p for k, p in enumerate(PLANES) if m >> k & 1) for m in range(1, 8)]
assert ODD_DIMS == (37, 29, 11)


def pack(n, normal, color, onormal, ocolor):
    return n | normal << 2 | color << 8 | onormal << 18 | ocolor << 24


class Ref:
    """The oracle's planes of one frame, the per-pixel fetches, and the pixel classes."""

    def __init__(self, world, fr):
        w, h = fr.width, fr.height
        p = fr.params.copy()
        p.flags = world.vx.FLAG_UNIT_GBUF
        self.depth = np.full((h, w), np.inf, np.float32)
        self.opaque_depth = np.full((h, w), np.inf, np.float32)
        self.surface = np.zeros((h, w), np.uint32)
        self.fetches = np.zeros((h, w), np.int64)
        self.n = np.zeros((h, w), np.int64)
        self.glass = np.zeros((h, w), bool)
        self.opaque = np.zeros((h, w), bool)
        for py in range(h):
            for px in range(w):
                n, g, f, cap = world.oracle.primary(p, world.oracle.pixel_dir(p, w, h, px, py))
                assert cap == 0
                self.fetches[py, px] = f
                recs = [g[j] for j in range(n) if np.float32(g[j].t) < np.inf]
                if not recs:
                    continue
                first = recs[0]
                op = [r for r in recs if r.id == 0]
                assert len(recs) <= 2 and len(op) <= 1 and (len(recs) == 1 or (first.id == 2 and op))
                self.n[py, px] = len(recs)
                self.glass[py, px] = first.id == 2
                self.opaque[py, px] = bool(op)
                self.depth[py, px] = first.t
                o = (op[0].normal_idx, op[0].color) if op else (0, 0)
                if op:
                    self.opaque_depth[py, px] = op[0].t
                self.surface[py, px] = pack(len(recs), first.normal_idx, first.color, *o)

    def planes(self):
        return {"depth": self.depth, "opaque_depth": self.opaque_depth, "surface": self.surface}

    def classes(self):
        """miss, opaque, glass over sky, glass over opaque."""
        return ((self.n == 0).sum(), (~self.glass & self.opaque).sum(), (self.glass & ~self.opaque).sum(),
                (self.glass & self.opaque).sum())


def same_planes(got, want, what=""):
    assert set(got) == set(want), what
    for name in got:
        a, b = got[name], want[name]
        assert a.shape == b.shape and a.dtype == b.dtype, (what, name)
        bad = np.argwhere(a.view(np.uint32) != b.view(np.uint32))
        assert len(bad) == 0, f"{what}: {name} differs at {len(bad)} pixels, first (y, x) {bad[:5].tolist()}"


def planes_of_hits(vx, hits, w, h):
    """The header's definition: the planes from vx_query_rays' results of the frame's pixel rays."""
    n = hits["n"]
    s = hits["s"]
    valid = np.maximum(n, 0)
    depth = np.where(valid >= 1, s["t"][:, 0], np.float32(np.inf)).astype(np.float32)
    k = np.where((valid >= 1) & (s["id"][:, 0] == 0), 0, np.where((valid >= 2) & (s["id"][:, 1] == 0), 1, -1))
    at = np.arange(len(hits))
    kk = np.maximum(k, 0)
    has = k >= 0
    opaque_depth = np.where(has, s["t"][at, kk], np.float32(np.inf)).astype(np.float32)
    word = np.where(valid >= 1, valid | s["normal_idx"][:, 0] << 2 | s["color"][:, 0] << 8, 0)
    word = word | np.where(has, s["normal_idx"][at, kk] << 18 | s["color"][at, kk] << 24, 0)
    return {"depth": depth.reshape(h, w), "opaque_depth": opaque_depth.reshape(h, w),
            "surface": word.astype(np.uint32).reshape(h, w)}


def numpy_pixel_rays(vx, fr):
    """vx_pixel_ray's rays of a whole frame, vectorised: fp32 in the header's order (np.float32
    division is IEEE)."""
    w, h, p = fr.width, fr.height, fr.params
    one = np.float32(1)
    nx = (2 * np.arange(w) + 1).astype(np.float32) / np.float32(w) - one
    ny = one - (2 * np.arange(h) + 1).astype(np.float32) / np.float32(h)
    rays = np.zeros((h, w), vx.RAY_DTYPE)
    for i in range(3):
        rays["cell"][..., i] = p.cam_cell[i]
        rays["fract"][..., i] = p.cam_fract[i]
        rays["dir"][..., i] = (np.float32(p.ray_fwd[i]) + nx * np.float32(p.ray_right[i]))[None, :] + \
            (ny * np.float32(p.ray_up[i]))[:, None]
    rays["t_max"] = np.inf
    return rays.reshape(-1)


_worlds, _refs = {}, {}


def world(name) -> World:
    if name not in _worlds:
        _worlds[name] = World(name)
    return _worlds[name]


def frame_of(name, cam, w, h):
    return world(name).vx.make_frame(*CAMS[name][cam], w, h)


def ref_of(name, cam, w, h) -> Ref:
    """Computed once per (scene, camera, size), shared by the tests, never written to.  (The cap-3
    world has its own: the same planes as the default cap's, other fetch counts.)"""
    key = (name, cam, w, h)
    if key not in _refs:
        _refs[key] = Ref(world(name), frame_of(name, cam, w, h))
    return _refs[key]


@pytest.fixture(scope="module", autouse=True)
def _close_worlds():
    yield
    for w in _worlds.values():
        w.close()
    _worlds.clear()
    _refs.clear()


# item 1's (scene, camera) list; each at 96x64 and 37x23
PARITY = [("proc5", 1), ("glass_wall", 1), ("odd", 0), ("odd", 1), ("odd_cap3", 0), ("odd_cap3", 1)]
# the cases whose four classes the issue counted (miss, opaque, glass over sky, glass over opaque)
ALL_CLASSES = {("proc5", 1, 96, 64), ("glass_wall", 1, 96, 64), ("odd", 0, 37, 23)}


@pytest.mark.parametrize("w,h", [(96, 64), (37, 23)])
@pytest.mark.parametrize("name,cam", PARITY)
def test_planes_equal_the_oracle_bit_for_bit(name, cam, w, h):
    wd, ref = world(name), ref_of(name, cam, w, h)
    got, st = wd.scene.gbuffer(frame_of(name, cam, w, h), stats=True)
    same_planes(got, ref.planes(), f"{name} cam {cam} {w}x{h}")
    cls = ref.classes()
    print(f"{name} cam {cam} {w}x{h}: miss, opaque, glass over sky, glass over opaque = {[int(c) for c in cls]}")
    assert sum(cls) == w * h
    if (name, cam, w, h) in ALL_CLASSES:
        assert all(c > 0 for c in cls), cls
    assert st.rays == w * h and st.invalid == 0 and st.cap_hits == 0
    assert st.hits == int(ref.n.sum()) and st.glass == int(ref.glass.sum())
    assert st.fetches == int(ref.fetches.sum()), (st.fetches, int(ref.fetches.sum()))


@pytest.mark.parametrize("w,h", [(96, 64), (37, 23)])
@pytest.mark.parametrize("name,cam", PARITY)
def test_planes_equal_query_rays_over_pixel_rays(name, cam, w, h):
    wd = world(name)
    fr = frame_of(name, cam, w, h)
    rays = numpy_pixel_rays(wd.vx, fr)
    for k in (0, w - 1, (h // 2) * w + w // 2, w * h - 1):          # the vectorised rays are vx_pixel_ray's
        assert rays[k].tobytes() == wd.vx.pixel_ray(fr, k % w, k // w).tobytes()
    hits, qst = wd.scene.query_rays(rays, stats=True)
    got, st = wd.scene.gbuffer(fr, stats=True)
    same_planes(got, planes_of_hits(wd.vx, hits, w, h), f"{name} cam {cam} {w}x{h}")
    assert st.as_dict() | {"kernel_ms": 0} == qst.as_dict() | {"kernel_ms": 0}


@pytest.mark.parametrize("w,h", [(1, 1), (1, 64), (64, 1), (33, 9), (31, 7)])
def test_edge_shapes(w, h):
    wd, ref = world("proc5"), ref_of("proc5", 1, w, h)
    got, st = wd.scene.gbuffer(frame_of("proc5", 1, w, h), stats=True)
    same_planes(got, ref.planes(), f"{w}x{h}")
    assert st.rays == w * h and st.fetches == int(ref.fetches.sum()) and st.hits == int(ref.n.sum())


GUARD = 64
PATTERN = 0x5AA5C33C


def device_planes(wd, fr, names, shift=0, stream=None):
    """names' planes through the device path, each inside a buffer with GUARD pattern words before and after
    it (and `shift` more words before: a start that is 4-byte but not 16-byte aligned); checks the guards."""
    import torch
    n = fr.width * fr.height
    bufs = {p: torch.full((GUARD + shift + n + GUARD,), PATTERN, dtype=torch.int32, device="cuda") for p in names}
    torch.cuda.synchronize()
    ptrs = {p: b.data_ptr() + 4 * (GUARD + shift) for p, b in bufs.items()}
    if shift:
        assert all(q % 16 == 4 * (shift % 4) and q % 16 != 0 for q in ptrs.values())
    wd.scene.gbuffer_device(fr, stream=stream, **ptrs)
    torch.cuda.synchronize()
    out = {}
    for p, b in bufs.items():
        raw = b.cpu().numpy().view(np.uint32)
        lo = GUARD + shift
        assert (raw[:lo] == PATTERN).all() and (raw[lo + n:] == PATTERN).all(), f"{p}: a guard word changed"
        body = raw[lo:lo + n].reshape(fr.height, fr.width).copy()
        out[p] = body.view(np.float32) if p != "surface" else body
    return out


@pytest.mark.parametrize("shift", [0, 1])
def test_plane_subsets_and_guards(shift):
    wd = world("proc5")
    fr = frame_of("proc5", 1, 37, 23)
    full = wd.scene.gbuffer(fr)
    same_planes(full, ref_of("proc5", 1, 37, 23).planes())
    assert len(SUBSETS) == 7
    for names in SUBSETS:
        got = device_planes(wd, fr, names, shift=shift)
        same_planes(got, {p: full[p] for p in names}, f"device {names}")
        if shift == 0:
            same_planes(wd.scene.gbuffer(fr, planes=names), {p: full[p] for p in names}, f"host {names}")


def test_host_path_equals_device_path():
    import torch
    wd = world("glass_wall")
    fr = frame_of("glass_wall", 1, 96, 64)
    host = wd.scene.gbuffer(fr)
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    dev = device_planes(wd, fr, PLANES, stream=st.cuda_stream)
    for p in PLANES:
        assert dev[p].tobytes() == host[p].tobytes(), p


# ---- poses ------------------------------------------------------------------------

def posed(wd, pos, fwd=None, right=None, up=None, base=("proc5", 0), w=33, h=17, cell=None):
    """A frame with the camera at pos (split as set_cam splits it) and, when given, an explicit basis."""
    fr = frame_of(*base, w, h)
    p = fr.params.copy()
    c, f = _split(pos)
    for i in range(3):
        p.cam_cell[i], p.cam_fract[i] = int(c[i]) if cell is None else int(cell[i]), float(f[i])
    for name, v in (("ray_fwd", fwd), ("ray_right", right), ("ray_up", up)):
        if v is not None:
            for i in range(3):
                getattr(p, name)[i] = float(np.float32(v[i]))
    return wd.vx.Frame(p, w, h)


def look_at(pos, target):
    f = np.asarray(target, np.float64) - np.asarray(pos, np.float64)
    f /= np.linalg.norm(f)
    r = np.cross(f, (0.0, 0.0, 1.0) if abs(f[2]) < 0.9 else (0.0, 1.0, 0.0))
    r /= np.linalg.norm(r)
    return f, 0.7 * r, 0.45 * np.cross(r, f)


def cell_where(grid, mask_fn):
    """A cell (x, y, z) of the kind mask_fn selects, the one nearest the grid's middle."""
    at = np.argwhere(mask_fn(grid))[:, ::-1]
    assert len(at)
    mid = np.array(grid.shape[::-1]) / 2
    return at[np.argmin(((at - mid) ** 2).sum(1))]


def check_pose(wd, fr, what):
    ref = Ref(wd, fr)
    got, st = wd.scene.gbuffer(fr, stats=True)
    same_planes(got, ref.planes(), what)
    assert st.invalid == 0 and st.cap_hits == 0 and st.fetches == int(ref.fetches.sum()), what
    return ref


@pytest.mark.parametrize("kind", ["air", "solid", "glass"])
def test_camera_inside_the_grid(kind):
    wd = world("proc5")
    pick = {"air": lambda g: g == 0, "solid": lambda g: (g >= 1) & (g < GLASS), "glass": lambda g: g == GLASS}[kind]
    c = cell_where(wd.grid, pick)
    X, Y, Z = wd.dims
    assert (c >= 0).all() and (c < (X, Y, Z)).all() and pick(wd.grid)[c[2], c[1], c[0]]
    ref = check_pose(wd, posed(wd, c + np.array([0.4, 0.55, 0.3])), f"camera in a {kind} cell {c.tolist()}")
    assert (ref.n >= 1).any()


@pytest.mark.parametrize("face", range(6))
def test_camera_outside_each_face_looking_in(face):
    wd = world("proc5")
    dims = np.array(wd.dims, np.float64)
    mid = dims / 2
    pos = mid + np.array([3.3, -2.1, 1.7])
    ax = face // 2
    pos[ax] = -7.25 if face % 2 == 0 else dims[ax] + 7.25
    fwd, right, up = look_at(pos, mid)
    ref = check_pose(wd, posed(wd, pos, fwd, right, up), f"outside face {face}")
    assert (ref.n >= 1).sum() > 50                    # the camera sees the scene (from above, nothing else)


def test_looking_away_every_pixel_misses():
    wd = world("proc5")
    dims = np.array(wd.dims, np.float64)
    pos = np.array([-6.5, dims[1] / 2, 5.5])
    fwd, right, up = look_at(pos, pos - (dims / 2 - pos))
    fr = posed(wd, pos, fwd, right, up)
    ref = check_pose(wd, fr, "looking away")
    got, st = wd.scene.gbuffer(fr, stats=True)
    assert (ref.n == 0).all() and st.hits == 0
    assert (got["depth"].view(np.uint32) == INF_BITS).all() and (got["opaque_depth"].view(np.uint32) == INF_BITS).all()
    assert not got["surface"].any()


def test_straight_down_with_exact_zero_components():
    wd = world("proc5")
    X, Y, Z = wd.dims
    fr = posed(wd, (X / 2 + 0.25, Y / 2 + 0.5, Z + 6.5), (0.0, 0.0, -1.0), (0.8, 0.0, 0.0), (0.0, 0.6, 0.0), w=33, h=17)
    rays = numpy_pixel_rays(wd.vx, fr).reshape(17, 33)
    assert (rays["dir"][8, 16] == (0.0, 0.0, -1.0)).all()            # the centre pixel: two exact zeros
    assert (rays["dir"][:, 16, 0] == 0).all() and (rays["dir"][8, :, 1] == 0).all()
    ref = check_pose(wd, fr, "straight down")
    assert (ref.n >= 1).all()                                        # the ground, at the least


@pytest.mark.parametrize("axis", [0, 1])
def test_camera_cell_at_the_largest_valid_value(axis):
    wd = world("proc5")
    X, Y, Z = wd.dims
    far = (1 << 22) - 1
    pos = np.array([X / 2 + 0.5, Y / 2 + 0.5, 6.5])
    pos[axis] = far + 0.5
    fwd = np.zeros(3)
    fwd[axis] = -1.0
    right = np.zeros(3)
    right[1 - axis] = 6e-6                                           # the grid fills a good part of the frame
    fr = posed(wd, pos, fwd, right, (0.0, 0.0, 1.5e-6))
    assert fr.params.cam_cell[axis] == far
    ref = check_pose(wd, fr, f"cam_cell[{axis}] = 2^22 - 1")
    print(f"cam_cell[{axis}] = 2^22 - 1: classes {[int(c) for c in ref.classes()]}")


def test_degenerate_ray_is_a_miss_and_counted():
    wd = world("proc5")
    vx = wd.vx
    w, h = 33, 9
    fr = posed(wd, (20.3, 12.6, 14.2), (0.0, 0.0, 0.0), (0.9, 0.1, -0.3), (0.1, 0.5, -0.6), w=w, h=h)
    rays = numpy_pixel_rays(vx, fr)
    centre = (h // 2) * w + w // 2
    assert not rays["dir"][centre].any() and (rays["dir"][np.arange(w * h) != centre] != 0).any(1).all()
    hits = wd.scene.query_rays(rays)
    assert hits["n"][centre] == vx.RAY_INVALID and (np.delete(hits["n"], centre) >= 0).all()
    got, st = wd.scene.gbuffer(fr, stats=True)
    assert st.invalid == 1 and st.rays == w * h
    assert got["depth"].view(np.uint32).flat[centre] == INF_BITS
    assert got["opaque_depth"].view(np.uint32).flat[centre] == INF_BITS and got["surface"].flat[centre] == 0
    same_planes(got, planes_of_hits(vx, hits, w, h), "beside the degenerate ray")
    assert (hits["n"] >= 1).any()


@pytest.mark.parametrize("name", ["glass_wall", "proc5"])
def test_surface_colour_is_the_primary_only_frame(name):
    import oracle
    wd = world(name)
    fr = frame_of(name, 1, 96, 64)
    img, _ = wd.scene.render(with_flags(fr, wd.vx.FLAG_PRIMARY_ONLY))
    words = wd.scene.gbuffer(fr, planes=("surface",))["surface"]
    colour = wd.vx.unpack_surface(words)["color"]                    # VX_SURF_COLOR: 0 on a miss = palette 0
    want = np.concatenate([oracle.vxo_palette()[colour], np.ones((64, 96, 1), np.float32)], axis=2)
    assert img.dtype == np.float32 and np.array_equal(img.view(np.uint32), want.view(np.uint32))
    assert len(np.unique(colour)) >= 3


def test_full_size_frame_equals_query_rays():
    import voxmap_amd as vx
    from voxmap_amd import presets
    c = presets.CONFIGS["C2"]
    w, h = 1920, 1080
    assert (c["w"], c["h"], c["scene"], c["camera"]) == (w, h, "s_proc", "K1")
    grid = presets.scene_grid(c["scene"])
    Z, Y, X = grid.shape
    fr = presets.camera_frame(c["camera"], w, h)
    with vx.Scene(map_bytes=grid.tobytes(), map_format=vx.FORMAT_GRID, dims=(X, Y, Z), device=0) as sc:
        hits, qst = sc.query_rays(numpy_pixel_rays(vx, fr), stats=True)
        got, st = sc.gbuffer(fr, stats=True)
    same_planes(got, planes_of_hits(vx, hits, w, h), "1920x1080")
    assert st.as_dict() | {"kernel_ms": 0} == qst.as_dict() | {"kernel_ms": 0}
    assert st.rays == w * h and st.invalid == 0 and st.cap_hits == 0 and st.glass > 0 and st.hits > w * h // 2


def test_bad_arguments_are_einval_then_a_valid_call_succeeds():
    import torch
    from voxmap_amd import _abi
    wd = world("proc5")
    L = wd.vx.lib()
    w, h = 37, 23
    fr = frame_of("proc5", 1, w, h)
    n = w * h
    host = {p: np.full(n, 7, np.uint32) for p in PLANES}
    dev = torch.full((n + 8,), 7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def call(scene=wd.scene.handle, params=fr.params, w=w, h=h, planes="host", on_device=0, edit=None):
        p = params
        if edit is not None:
            p = params.copy()
            edit(p)
        if planes == "host":
            planes = _abi.GbufferPlanes(*(host[k].ctypes.data for k in PLANES))
        return L.vx_render_gbuffer(scene, C.byref(p) if p is not None else None, w, h,
                                   C.byref(planes) if planes is not None else None, on_device, None, None)

    def setv(field, i, v):
        return lambda p: getattr(p, field).__setitem__(i, v)

    cases = {
        "null scene": dict(scene=None), "null params": dict(params=None), "null out": dict(planes=None),
        "all planes null": dict(planes=_abi.GbufferPlanes(None, None, None)),
        "w = 0": dict(w=0), "h = 0": dict(h=0), "w < 0": dict(w=-3), "w = 32769": dict(w=32769), "h = 32769": dict(h=32769),
        "w*h > 2^26": dict(w=8193, h=8192),
        "quality 0": dict(edit=lambda p: setattr(p, "quality", 0)),
        "cam_cell 2^22": dict(edit=setv("cam_cell", 0, 1 << 22)), "cam_cell -2^22": dict(edit=setv("cam_cell", 2, -(1 << 22))),
        "cam_fract 1": dict(edit=setv("cam_fract", 1, 1.0)), "cam_fract < 0": dict(edit=setv("cam_fract", 0, -0.25)),
        "cam_fract NaN": dict(edit=setv("cam_fract", 2, float("nan"))),
        "fwd inf": dict(edit=setv("ray_fwd", 0, float("inf"))), "right NaN": dict(edit=setv("ray_right", 1, float("nan"))),
        "up -inf": dict(edit=setv("ray_up", 2, float("-inf"))),
        "misaligned device depth": dict(planes=_abi.GbufferPlanes(dev.data_ptr() + 2, None, None), on_device=1),
        "misaligned device surface": dict(planes=_abi.GbufferPlanes(None, None, dev.data_ptr() + 1), on_device=1),
    }
    assert (8193 * 8192 > _abi.MAX_QUERY_RAYS) and 8193 <= 32768
    for what, kw in cases.items():
        assert call(**kw) == _abi.VX_EINVAL, what
        assert L.vx_last_error(), what
    torch.cuda.synchronize()
    assert all((a == 7).all() for a in host.values()) and (dev.cpu().numpy() == 7).all()
    # the ignored fields do not make a call invalid: a NaN sun, flags, soft-shadow settings out of range
    def ignored(p):
        p.sun_dir[0] = float("nan")
        p.flags = 0xFFFFFFFF
        p.shadow_samples = 99
        p.sun_radius = 9.0
    assert call(edit=ignored) == 0
    same_planes({k: v.reshape(h, w).view(np.float32) if k != "surface" else v.reshape(h, w) for k, v in host.items()},
                ref_of("proc5", 1, w, h).planes(), "after the rejected calls")


def test_vxrender_gbuffer_files_equal_the_api(tmp_path):
    wd = world("proc5")
    X, Y, Z = wd.dims
    w, h = 96, 64
    sbj, rot = CAMS["proc5"][1]
    path = tmp_path / "map.grid"
    path.write_bytes(wd.grid.tobytes())
    prefix = tmp_path / "planes"
    r = subprocess.run([os.path.join(ROOT, "voxmap_amd", "vxrender"), "--map", str(path), "--format", "grid", "--dims",
                        f"{X},{Y},{Z}", "--size", f"{w},{h}", "--orbit", ",".join(map(str, (*sbj, *rot))),
                        "--out", str(tmp_path / "frame.rgba"), "--gbuffer", str(prefix)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    want = wd.scene.gbuffer(frame_of("proc5", 1, w, h))
    for name, ext in (("depth", "depth.f32"), ("opaque_depth", "opaque.f32"), ("surface", "surface.u32")):
        raw = open(f"{prefix}.{ext}", "rb").read()
        assert raw == want[name].tobytes(), name
    assert os.path.getsize(tmp_path / "frame.rgba") == w * h * 4
