"""Ray queries on the GPU (vx_query_rays / k_query) against the scalar oracle.

The reference, per ray: a copy of a FrameParams with cam_cell / cam_fract set to
the ray's origin and flags = VX_FLAG_UNIT_GBUF, through Oracle.primary(params,
dir) (oracle vxo_primary); t_max applied here as t < t_max.  Compared bit for
bit: n, and per record id, color, normal_idx, cell, fract, t.
"""
import ctypes as C
import math

import numpy as np
import pytest

from gpu_rig import Rig, need_gpu  # noqa: F401 (need_gpu: an autouse fixture)

pytestmark = pytest.mark.gpu

GLASS = 21
INF = np.float32(np.inf)


# ---- scenes: the smallest the project uses for parity -------------------------

def _grid(name):
    from voxmap_amd import scenes
    return {"proc5": lambda: scenes.small_proc(5), "proc7": lambda: scenes.small_proc(7),
            "glass_wall": scenes.glass_wall, "single_block": scenes.single_block,
            # an odd-shaped field with blocks on its far faces, at the default box cap and at cap 3 (the
            # cap is also the copies' border: rays from outside the grid enter through it)
            "odd": lambda: scenes.odd_proc(1, ODD_DIMS), "odd_cap3": lambda: scenes.odd_proc(1, ODD_DIMS)}[name]()


ODD_DIMS = (37, 29, 11)
DIST_CAP = {"odd_cap3": 3}           # vx_scene_desc.dist_cap per world; others: the default (64)


# (camera above the grid, camera outside it looking in) as (sbj, rot) of the orbit camera
CAMS = {
    "proc5": [((48.0, 24.0, 18.0), (1.1, 0.0, 0.6)), ((-6.0, 24.0, 9.0), (1.45, 0.0, -math.pi / 2))],
    "proc7": [((48.0, 24.0, 18.0), (1.1, 0.0, 0.6)), ((-6.0, 24.0, 9.0), (1.45, 0.0, -math.pi / 2))],
    "glass_wall": [((40.0, 20.0, 14.0), (1.25, 0.0, -math.pi / 2)), ((-4.0, 30.0, 7.0), (1.5, 0.0, -math.pi / 2))],
    "single_block": [((20.0, 12.0, 12.0), (0.5, 0.0, 0.3)), ((-5.0, 12.0, 6.0), (1.45, 0.0, -math.pi / 2))],
}
SCENES = list(CAMS)
CAMS["odd"] = CAMS["odd_cap3"] = [((18.5, 14.5, 11.2), (1.0, 0.0, 0.6)), ((-5.0, 14.0, 7.0), (1.45, 0.0, -math.pi / 2))]
ODD_SCENES = ["odd", "odd_cap3"]


class World(Rig):
    """One scene on the device, its oracle, and the reference walk."""

    def __init__(self, name):
        import voxmap_amd as vx
        self.vx = vx
        self.name = name
        self.grid = _grid(name)
        Z, Y, X = self.grid.shape
        self.dims = (X, Y, Z)
        super().__init__(vx.field_build(self.grid), np.zeros((4, 4, 4), np.uint8), self.dims,
                         dist_cap=DIST_CAP.get(name, 0))
        self._params = vx.make_frame((X / 2, Y / 2, 10.0), (1.0, 0.0, 0.0), 64, 64).params
        self._cache = {}

    def make_oracle(self, noise):
        import oracle
        return oracle.Oracle(self.dev_field, noise, cap=DIST_CAP.get(self.name, 64))

    def reference(self, rays, key=None):
        """(HIT_DTYPE array, fetches per ray) of the oracle, t_max applied as t < t_max.
        Invalid rays are the caller's business: every ray here is walked."""
        if key is not None and key in self._cache:
            return self._cache[key]
        vx = self.vx
        out = np.zeros(len(rays), vx.HIT_DTYPE)
        fetches = np.zeros(len(rays), np.int64)
        p = self._params.copy()
        p.flags = vx.FLAG_UNIT_GBUF
        for i, r in enumerate(rays):
            for a in range(3):
                p.cam_cell[a] = int(r["cell"][a])
                p.cam_fract[a] = float(r["fract"][a])
            n, g, f, cap = self.oracle.primary(p, [float(v) for v in r["dir"]])
            assert cap == 0
            fetches[i] = f
            k = 0
            for j in range(n):
                if np.float32(g[j].t) < r["t_max"]:
                    s = out["s"][i, k]
                    s["id"], s["color"], s["normal_idx"] = g[j].id, g[j].color, g[j].normal_idx
                    s["cell"] = list(g[j].cell)
                    s["fract"] = list(g[j].fract)
                    s["t"] = g[j].t
                    k += 1
            out["n"][i] = k
        if key is not None:
            self._cache[key] = (out, fetches)
        return out, fetches

    def pixel_rays(self, cam, w=96, h=64):
        vx = self.vx
        fr = vx.make_frame(*CAMS[self.name][cam], w, h)
        rays = np.zeros(w * h, vx.RAY_DTYPE)
        for py in range(h):
            for px in range(w):
                rays[py * w + px] = vx.pixel_ray(fr, px, py)
        return fr, rays


_worlds = {}


@pytest.fixture
def world(request):
    name = getattr(request, "param", "proc5")
    if name not in _worlds:
        _worlds[name] = World(name)
    return _worlds[name]


@pytest.fixture(scope="module", autouse=True)
def _close_worlds():
    yield
    for w in _worlds.values():
        w.close()
    _worlds.clear()


def _same(hits, ref, what=""):
    """n and every record of s[0..n) equal bit for bit."""
    assert hits.dtype == ref.dtype and hits.shape == ref.shape
    bad = np.flatnonzero(hits["n"] != ref["n"])
    assert bad.size == 0, f"{what}: n differs at {bad[:5].tolist()}: {hits['n'][bad[:5]]} != {ref['n'][bad[:5]]}"
    for k in range(2):
        m = ref["n"] > k
        a, b = hits["s"][m, k], ref["s"][m, k]
        for f in ("id", "color", "normal_idx", "cell"):
            assert np.array_equal(a[f], b[f]), (what, k, f, np.flatnonzero((a[f] != b[f]).reshape(len(a), -1).any(1))[:5])
        for f in ("fract", "t"):
            assert np.array_equal(a[f].view(np.uint32), b[f].view(np.uint32)), (what, k, f)


def _split(pos):
    """origin -> (cell, fract) as set_cam splits a camera position."""
    pos = np.asarray(pos, np.float64)
    fl = np.floor(pos)
    fr = (pos - fl).astype(np.float32)
    up = fr >= 1.0
    return (fl + up).astype(np.int32), np.where(up, np.float32(0), fr)


def random_rays(w: World, n=2000, seed=1234):
    """Seeded rays with origins in air, in solid cells, in glass and outside the grid on every
    side (pointing in and away), directions in all eight octants, fract exactly 0 on some axes.
    Returns (rays, kind per ray): 0 anywhere inside, 1 in a solid cell, 2 in glass, 3 + side outside."""
    vx = w.vx
    rng = np.random.default_rng(seed)
    X, Y, Z = w.dims
    dims = np.array(w.dims, np.float64)
    solid = np.argwhere((w.grid >= 1) & (w.grid <= 20))[:, ::-1]
    glass = np.argwhere(w.grid == GLASS)[:, ::-1]
    air = np.argwhere(w.grid == 0)[:, ::-1]
    rays = np.zeros(n, vx.RAY_DTYPE)
    kind = np.zeros(n, np.int32)
    for i in range(n):
        k = i % 10
        d = np.abs(rng.normal(size=3)) + 1e-3
        d *= np.array([1 if (i >> b) & 1 == 0 else -1 for b in range(3)])     # the eight octants in turn
        d *= 10.0 ** rng.uniform(-2, 2)                                     # not normalised
        if k < 3:
            pos = air[rng.integers(len(air))] + rng.random(3)
            kind[i] = 0
        elif k < 5:
            pos = solid[rng.integers(len(solid))] + rng.random(3)
            kind[i] = 1
        elif k == 5 and len(glass):
            pos = glass[rng.integers(len(glass))] + rng.random(3)
            kind[i] = 2
        else:
            side = int(rng.integers(6))
            pos = rng.random(3) * dims
            ax = side // 2
            off = rng.uniform(0.0, 40.0)
            pos[ax] = -off if side % 2 == 0 else dims[ax] + off
            target = rng.random(3) * dims
            d = (target - pos) * 10.0 ** rng.uniform(-1, 1)
            if rng.random() < 0.3:
                d = -d                                                       # pointing away: a miss
            kind[i] = 3 + side
        cell, fract = _split(pos)
        if i % 4 == 0:
            fract[rng.integers(3)] = 0.0
        if i % 16 == 0:
            fract[:] = 0.0
        rays["cell"][i], rays["fract"][i], rays["dir"][i], rays["t_max"][i] = cell, fract, d.astype(np.float32), INF
    return rays, kind


# ---- the cases ------------------------------------------------------------------

@pytest.mark.parametrize("world", SCENES + ODD_SCENES, indirect=True)
@pytest.mark.parametrize("cam", [0, 1])
def test_pixel_rays_match_the_oracle(world, cam):
    fr, rays = world.pixel_rays(cam)
    assert len(rays) == 6144
    ref, _ = world.reference(rays, key=("px", cam))
    _same(world.scene.query_rays(rays), ref, f"{world.name} cam {cam}")
    # the frame is not empty: the rays see the scene
    assert (ref["n"] >= 1).sum() > 500, (ref["n"] >= 1).sum()
    if world.name in ("proc5", "glass_wall"):
        # glass with a surface behind it, glass with sky behind it or an opaque first surface, and misses
        assert (ref["n"] == 2).any() and (ref["n"] == 1).any() and (ref["n"] == 0).any()
    if world.name == "proc5":
        assert ((ref["n"] == 1) & (ref["s"]["id"][:, 0] == 0)).any()
        if cam == 1:
            assert ((ref["n"] == 1) & (ref["s"]["id"][:, 0] == 2)).any()     # glass with sky behind it


@pytest.mark.parametrize("world", SCENES + ODD_SCENES, indirect=True)
def test_random_rays_match_the_oracle(world):
    rays, kind = random_rays(world)
    assert len(rays) == 2000
    ref, _ = world.reference(rays, key="rnd")
    _same(world.scene.query_rays(rays), ref, world.name)
    # the set holds what it claims: every origin kind, every side, every octant, zero fracts
    want = set(range(3, 9)) | {0, 1} | ({2} if (world.grid == GLASS).any() else set())
    assert set(kind.tolist()) == want
    d = rays["dir"]
    octs = (d[:, 0] < 0) * 1 + (d[:, 1] < 0) * 2 + (d[:, 2] < 0) * 4
    assert set(octs.tolist()) == set(range(8))
    assert (rays["fract"] == 0).all(1).any() and ((rays["fract"] == 0).sum(1) == 1).any()
    outside = kind >= 3
    assert (ref["n"][outside] == 0).any() and (ref["n"][outside] >= 1).any()
    if world.name.startswith("proc"):
        assert (ref["n"][kind == 1] >= 1).any()       # out of a solid cell into a cell of another colour


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1000])
def test_ray_counts_cover_tail_lanes(world, n):
    rays, _ = random_rays(world)
    ref, _ = world.reference(rays, key="rnd")
    # a window that starts off the array's beginning, with canaries behind the result
    lo = 37
    import torch
    dev_r = torch.from_numpy(rays[lo:lo + n].copy().view(np.uint8)).cuda()
    dev_h = torch.full(((n + 3) * world.vx.HIT_DTYPE.itemsize,), 0xA5, dtype=torch.uint8, device="cuda")
    world.scene.query_rays_device(dev_r.data_ptr(), n, dev_h.data_ptr())
    torch.cuda.synchronize()
    raw = dev_h.cpu().numpy()
    hits = raw.view(world.vx.HIT_DTYPE)
    _same(hits[:n], ref[lo:lo + n], f"n = {n}")
    assert (raw[n * world.vx.HIT_DTYPE.itemsize:] == 0xA5).all(), "a tail lane stored past the last ray"
    _same(world.scene.query_rays(rays[lo:lo + n]), ref[lo:lo + n], f"host n = {n}")


@pytest.mark.parametrize("world", ["single_block", "proc5"], indirect=True)
def test_degenerate_directions(world):
    vx = world.vx
    X, Y, Z = world.dims
    base = np.array([0.37, -0.52, -0.61], np.float32)
    inside = (20.3, 12.6, 10.2)
    rows = []                                   # (origin, dir, must miss)
    tiny = np.float32(2.0 ** -45)
    for a in range(3):
        for v in (np.float32(0.0), np.float32(-0.0), tiny, -tiny):
            d = base.copy()
            d[a] = v
            rows.append((inside, d, False))
            rows.append((inside, -d, False))
        for sgn in (1.0, -1.0):                 # two zero components: axis-aligned
            d = np.zeros(3, np.float32)
            d[a] = sgn
            rows.append((inside, d, False))
            d2 = d.copy()
            d2[(a + 1) % 3] = np.float32(-0.0)
            rows.append((inside, d2, False))
        # a zero component on an axis whose slab does not hold the origin: a miss
        for v in (np.float32(0.0), np.float32(-0.0)):
            o = np.array(inside)
            o[a] = -5.5
            d = np.array([0.4, 0.3, -0.2], np.float32)
            d[a] = v
            rows.append((tuple(o), d, True))
            o[a] = world.dims[a] + 3.25
            rows.append((tuple(o), d, True))
    # mixed into waves whose other lanes are ordinary
    ordinary, _ = random_rays(world, n=192, seed=99)
    rays = np.zeros(len(rows) * 4, vx.RAY_DTYPE)
    rays[:] = np.resize(ordinary, len(rays))
    at = np.arange(len(rows)) * 4 + 1
    for i, (o, d, _) in zip(at, rows):
        rays["cell"][i], rays["fract"][i] = _split(o)
        rays["dir"][i], rays["t_max"][i] = d, INF
    ref, _ = world.reference(rays)
    _same(world.scene.query_rays(rays), ref, world.name)
    for i, (_, d, miss) in zip(at, rows):
        if miss:
            assert ref["n"][i] == 0
    if world.name == "single_block":
        # straight down onto the block's top: entered going down the z axis (normal index 4), at its cell
        down = [i for i, (o, d, _) in zip(at, rows) if o == inside and d[2] == -1.0 and d[0] == 0 and d[1] == 0]
        assert len(down) == 2
        for i in down:
            s = ref["s"][i, 0]
            assert ref["n"][i] == 1 and s["normal_idx"] == 4 and s["color"] == 5 and list(s["cell"]) == [20, 12, 2]


def _hitting(world, want=200):
    picked, refs = [], []
    for cam in (0, 1):
        _, rays = world.pixel_rays(cam)
        ref, _ = world.reference(rays, key=("px", cam))
        idx = np.flatnonzero(ref["n"] >= 1)
        idx = idx[:: max(1, len(idx) // (want // 2))][: want // 2]
        picked.append(rays[idx])
        refs.append(ref[idx])
    return np.concatenate(picked), np.concatenate(refs)


@pytest.mark.parametrize("world", ["proc5", "glass_wall"], indirect=True)
def test_t_max_is_strict(world):
    rays, ref = _hitting(world)
    assert len(rays) == 200
    t0 = ref["s"]["t"][:, 0].copy()
    # t_max = the hit's own t: the record is dropped (strict), and so is everything behind it
    at = rays.copy()
    at["t_max"] = t0
    r_at, _ = world.reference(at)
    assert (r_at["n"] == 0).all()
    _same(world.scene.query_rays(at), r_at, "t_max = t")
    # the next float above t keeps it
    up = rays.copy()
    up["t_max"] = np.nextafter(t0, INF)
    r_up, _ = world.reference(up)
    assert (r_up["n"] >= 1).all() and np.array_equal(r_up["s"]["t"][:, 0].view(np.uint32), t0.view(np.uint32))
    _same(world.scene.query_rays(up), r_up, "t_max = next(t)")
    if world.name == "glass_wall":
        two = ref["n"] == 2
        assert two.sum() >= 10
        mid = rays[two].copy()
        tg, tw = ref["s"]["t"][two, 0], ref["s"]["t"][two, 1]
        mid["t_max"] = tg + (tw - tg) * np.float32(0.5)
        assert ((tg < mid["t_max"]) & (mid["t_max"] < tw)).all()
        r_mid, _ = world.reference(mid)
        assert (r_mid["n"] == 1).all() and (r_mid["s"]["id"][:, 0] == 2).all()
        _same(world.scene.query_rays(mid), r_mid, "glass only")


def test_invalid_rays_are_answered_not_walked(world):
    vx = world.vx
    good, _ = random_rays(world, n=64, seed=5)
    bad_edits = [
        lambda r: r["cell"].__setitem__(0, 1 << 22), lambda r: r["cell"].__setitem__(1, -(1 << 22)),
        lambda r: r["cell"].__setitem__(2, np.iinfo(np.int32).min), lambda r: r["cell"].__setitem__(0, np.iinfo(np.int32).max),
        lambda r: r["fract"].__setitem__(0, 1.0), lambda r: r["fract"].__setitem__(1, -0.25),
        lambda r: r["fract"].__setitem__(2, np.nan), lambda r: r["fract"].__setitem__(0, np.inf),
        lambda r: r["dir"].__setitem__(0, np.inf), lambda r: r["dir"].__setitem__(1, -np.inf),
        lambda r: r["dir"].__setitem__(2, np.nan), lambda r: r["dir"].__setitem__(slice(None), 0.0),
        lambda r: r["dir"].__setitem__(slice(None), [0.0, -0.0, 0.0]), lambda r: r.__setitem__("t_max", np.nan),
    ]
    rays = np.zeros(3 * len(bad_edits) + 1, vx.RAY_DTYPE)
    rays[:] = np.resize(good, len(rays))
    bad_at = 3 * np.arange(len(bad_edits)) + 1
    for i, edit in zip(bad_at, bad_edits):
        edit(rays[i])
    ok = np.ones(len(rays), bool)
    ok[bad_at] = False
    ref = np.zeros(len(rays), vx.HIT_DTYPE)
    ref[ok], fetches = world.reference(rays[ok])
    ref["n"][bad_at] = vx.RAY_INVALID
    hits, st = world.scene.query_rays(rays, stats=True)
    assert (hits["n"][bad_at] == -1).all(), hits["n"][bad_at]
    _same(hits, ref, "neighbours of invalid rays")
    assert not hits[bad_at]["s"].view(np.uint8).any()
    assert st.rays == len(rays) and st.invalid == len(bad_edits)
    assert st.fetches == fetches.sum() and st.cap_hits == 0
    # the largest valid cells, far outside the grid: walked (a miss), not rejected
    far = good[:2].copy()
    far["cell"][0] = [(1 << 22) - 1, 3, 3]
    far["cell"][1] = [5, -(1 << 22) + 1, 3]
    far["dir"][0] = [-1.0, 1e-7, -1e-7]
    far["dir"][1] = [1e-7, 1.0, 1e-7]
    r_far, _ = world.reference(far)
    _same(world.scene.query_rays(far), r_far, "far origins")


@pytest.mark.parametrize("world", ["proc5", "glass_wall"] + ODD_SCENES, indirect=True)
def test_statistics_equal_the_oracles_counts(world):
    rays, _ = random_rays(world)
    _, px = world.pixel_rays(0)
    rays = np.concatenate([rays, px[::3]])
    assert (rays["t_max"] == INF).all()
    ref_a, f_a = world.reference(rays[:2000], key="rnd")
    ref_b, f_b = world.reference(px, key=("px", 0))
    ref, fetches = np.concatenate([ref_a, ref_b[::3]]), np.concatenate([f_a, f_b[::3]])
    hits, st = world.scene.query_rays(rays, stats=True)
    _same(hits, ref)
    assert st.rays == len(rays) and st.invalid == 0 and st.cap_hits == 0
    assert st.fetches == int(fetches.sum()), (st.fetches, int(fetches.sum()))
    nrec = int(ref["n"].sum())
    nglass = int(sum(((ref["n"] > k) & (ref["s"]["id"][:, k] == 2)).sum() for k in range(2)))
    assert st.hits == nrec and st.glass == nglass and nglass > 0
    assert st.kernel_ms > 0


def test_host_and_device_paths_give_identical_bytes(world):
    import torch
    rays, _ = random_rays(world)
    host = world.scene.query_rays(rays)
    dev_r = torch.from_numpy(rays.view(np.uint8).copy()).cuda()
    dev_h = torch.empty(len(rays) * host.dtype.itemsize, dtype=torch.uint8, device="cuda")
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    world.scene.query_rays_device(dev_r.data_ptr(), len(rays), dev_h.data_ptr(), stream=st.cuda_stream)
    st.synchronize()
    assert dev_h.cpu().numpy().tobytes() == host.tobytes()
    # unused records and the reserved word are zero: the bytes are a function of the rays alone
    assert not host["reserved"].any() and not host["s"][host["n"] < 2, 1].view(np.uint8).any()


def test_two_streams_beside_a_render(world):
    import torch
    vx = world.vx
    a, _ = random_rays(world, n=2000, seed=1)
    _, b = world.pixel_rays(0)
    fr = vx.make_frame(*CAMS[world.name][0], 256, 144)
    alone_a, alone_b = world.scene.query_rays(a), world.scene.query_rays(b)
    img = torch.empty((144, 256, 4), dtype=torch.uint8, device="cuda")
    world.scene.render_device(fr, img.data_ptr(), pixel_format=vx.PIXEL_RGBA8)
    torch.cuda.synchronize()
    alone_img = img.cpu().numpy().copy()
    da, db = (torch.from_numpy(r.view(np.uint8).copy()).cuda() for r in (a, b))
    size = alone_a.dtype.itemsize
    ha = [torch.zeros(len(a) * size, dtype=torch.uint8, device="cuda") for _ in range(3)]
    hb = [torch.zeros(len(b) * size, dtype=torch.uint8, device="cuda") for _ in range(3)]
    imgs = [torch.zeros_like(img) for _ in range(3)]
    torch.cuda.synchronize()
    s1, s2, s3 = torch.cuda.Stream(), torch.cuda.Stream(), torch.cuda.Stream()
    for k in range(3):
        world.scene.query_rays_device(da.data_ptr(), len(a), ha[k].data_ptr(), stream=s1.cuda_stream)
        world.scene.render_device(fr, imgs[k].data_ptr(), pixel_format=vx.PIXEL_RGBA8, stream=s3.cuda_stream)
        world.scene.query_rays_device(db.data_ptr(), len(b), hb[k].data_ptr(), stream=s2.cuda_stream)
    for s in (s1, s2, s3):
        s.synchronize()
    for k in range(3):
        assert ha[k].cpu().numpy().tobytes() == alone_a.tobytes()
        assert hb[k].cpu().numpy().tobytes() == alone_b.tobytes()
        assert np.array_equal(imgs[k].cpu().numpy(), alone_img)


def test_pick_returns_the_pixels_surface(world):
    vx = world.vx
    fr, rays = world.pixel_rays(0)
    ref, _ = world.reference(rays, key=("px", 0))
    rng = np.random.default_rng(3)
    pixels = [(int(rng.integers(96)), int(rng.integers(64))) for _ in range(20)]
    got = np.zeros(20, vx.HIT_DTYPE)
    for k, (px, py) in enumerate(pixels):
        got[k] = world.scene.pick(fr, px, py)
    want = ref[[py * 96 + px for px, py in pixels]]
    _same(got, want, "pick")
    assert (want["n"] >= 1).any()


def _projection(w, h, sbj, rot):
    """cam.projection_matrix of map.js:373-391 (column-major float32) and the camera position."""
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
    near, far = 1.0, 1000.0
    P = np.array([[f / math.sqrt(a), 0, 0, 0], [0, f * math.sqrt(a), 0, 0],
                  [0, 0, (near + far) / (near - far), 2 * near * far / (near - far)], [0, 0, -1, 0.0]])
    view = Rx(-rot[0]) @ Rz(-rot[2]) @ T(*(-pos))
    return (P @ view).T.reshape(-1).astype(np.float32), pos


def place_set(w: World):
    """Places over the scene: a lattice of points at a few heights, points just behind every
    few glass cells (on both sides of the pane), and some behind and beside the camera."""
    X, Y, Z = w.dims
    pts = [(x + 0.5, y + 0.5, z + 0.5) for z in (1, 3, 6) for y in range(2, Y, 7) for x in range(2, X, 7)]
    for gz, gy, gx in np.argwhere(w.grid == GLASS)[::5]:
        for dx, dy in ((1.5, 0), (-1.5, 0), (0, 1.5), (0, -1.5)):
            pts.append((gx + 0.5 + dx, gy + 0.5 + dy, gz + 0.5))
    pts += [(X / 2, Y / 2, 300.0), (-400.0, Y / 2, 5.0), (X / 2, 900.0, 2.0)]
    return np.array(pts, np.float64)


def test_place_views_hide_what_a_block_hides(world):
    vx = world.vx
    sbj, rot = CAMS[world.name][0]
    m, cam = _projection(1280, 720, sbj, rot)
    places = place_set(world)
    views, visible = world.scene.place_views(m, cam, places)
    v2, rays = vx.place_rays(m, cam, places)
    assert views.tobytes() == v2.tobytes() and (rays["t_max"] == 1).all()
    ref, _ = world.reference(rays)
    opaque = np.zeros(len(rays), bool)
    glass = np.zeros(len(rays), bool)
    for k in range(2):
        opaque |= (ref["n"] > k) & (ref["s"]["id"][:, k] == 0)
        glass |= (ref["n"] > k) & (ref["s"]["id"][:, k] == 2)
    assert np.array_equal(visible, ~opaque)
    on = views["on_screen"] != 0
    # all four kinds occur: in plain view, behind a block, through glass only, off screen
    assert (on & ~opaque & ~glass).any() and (on & opaque).any() and (on & glass & ~opaque).any() and (~on).any()
    assert visible[on & glass & ~opaque].all()
