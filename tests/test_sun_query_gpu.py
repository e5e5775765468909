"""Sun queries on the GPU (vx_query_sun / k_sun_query) against the scalar oracle.

The reference, per point i and sun j, is built here: the face test of
render.frag:228-229 in float32 (a pair it fails is culled: unlit, no march),
else vxo_march(cell, fract, sun, MAX_STEPS) of the oracle over the field the
scene reads back, lit iff step == MAX_STEPS.  Compared bit for bit: every output
word, and the counters (with VX_SUNQ_NO_EXIT, fetches is the oracle's sum).
"""
import ctypes as C
import math

import numpy as np
import pytest

from gpu_rig import Rig, need_gpu, sun_dir  # noqa: F401 (need_gpu: an autouse fixture)

pytestmark = pytest.mark.gpu

K = 41                                # the mask crosses a word boundary
NO_EXIT = 0x1                         # include/voxmap.h VX_SUNQ_NO_EXIT
INVALID = 0xFFFFFFFF

# name -> (dims, dist_cap): the smallest fields that reach each march path
SCENES = {
    "proc5": ((96, 48, 16), 0),       # padded copies, orthant exit copies
    "odd": ((37, 29, 11), 0),         # odd X and Y
    "flat": ((41, 23, 1), 0),         # Z = 1: MAX_STEPS = 2
    "tall": ((24, 20, 127), 8),       # Z > 126: no padded copy, the u8 march_fast path
}
CAM = ((48.0, 24.0, 18.0), (1.1, 0.0, 0.6))          # proc5, the frame of the agreement test
FRAME_SUN = sun_dir(25, 250)


def sun_set():
    """K directions: a sweep of the day, every sign octant, and the edges of the fast-path rule."""
    import voxmap_amd as vx
    s = [vx.sun_from_hour(h) for h in np.linspace(-1.5, 1.5, 24)]                 # hourly-plus; goes through noon
    s[11] = vx.sun_from_hour(0.0)                                                 # (0, 0, 1) itself: the literal path
    s += [(sx * 0.43, sy * 0.61, sz * 0.52) for sz in (1, -1) for sy in (1, -1) for sx in (1, -1)]   # the 8 octants
    s += [(0.6, 2.0 ** -11, 0.7),            # a component below 2^-10: literal
          (0.6, -2.0 ** -10, 0.7),           # exactly 2^-10: fast
          (0.35, 0.2, -0.8),                 # down-going: the G channel
          (2.0, 3.0, 1.5),                   # not normalised, components above 1: literal under the query's rule
          (1.0, 0.5, 0.25),                  # a component of exactly 1: fast
          (float(np.nextafter(np.float32(1), np.float32(2))), 0.5, 0.25),      # one ulp above: literal
          (1.0, 0.0, 0.0),                   # axis-aligned, z = +0
          (-0.3, 0.2, -0.0),                 # z = -0: not "< 0", so no sun is culled by it; a zero dot culls +-z faces
          (0.05, -0.07, 0.02)]               # short: every |r_i| <= 1, fast
    out = np.array(s, np.float32)
    assert out.shape == (K, 3)
    assert (out[11] == (0, 0, 1)).all()
    return out


class World(Rig):
    def __init__(self, name):
        import voxmap_amd as vx
        from voxmap_amd import scenes
        self.vx, self.name = vx, name
        self.dims, self.cap = SCENES[name]
        grid = scenes.small_proc(5) if name == "proc5" else scenes.odd_proc(1, self.dims)
        super().__init__(vx.field_build(grid), np.zeros((4, 4, 4), np.uint8), self.dims, dist_cap=self.cap)
        self.suns = sun_set()
        self._points = None
        self._refs = {}

    def make_oracle(self, noise):
        import oracle
        return oracle.Oracle(self.dev_field, noise, cap=self.cap or 64)       # exit=False: the reference's literal march

    def frame(self, **kw):
        X, Y, Z = self.dims
        cam = CAM if self.name == "proc5" else ((X / 2, Y / 2, 0.1 * max(X, Y) + 0.5 * Z + 2), (1.0, 0.0, 0.6))
        return self.vx.make_frame(*cam, 48, 32, **kw)

    def points(self):
        """The point set of a scene, in this order: first records of a 48 x 32 pixel batch (real faces, fracts
        straight from the device), the field's ground points, 257 seeded random cells (some inside blocks) with no
        face, and the edge fracts."""
        if self._points is not None:
            return self._points
        vx = self.vx
        fr = self.frame()
        rays = np.zeros(48 * 32, vx.RAY_DTYPE)
        for py in range(32):
            for px in range(48):
                rays[py * 48 + px] = vx.pixel_ray(fr, px, py)
        faces = vx.points_of_hits(self.scene.query_rays(rays))
        ground, _ = vx.ground_points(self.dev_field)
        rng = np.random.default_rng(2024)
        rnd = np.zeros(257, vx.SUN_POINT_DTYPE)
        rnd["cell"] = np.stack([rng.integers(0, d, 257) for d in self.dims], 1)
        rnd["fract"] = rng.random((257, 3), dtype=np.float32)
        rnd["normal_idx"] = -1
        one = np.float32(1)
        edge_vals = [np.float32(0), np.nextafter(one, np.float32(0)), np.float32(-2.0 ** -24), np.float32(-1),
                     np.nextafter(np.float32(2), np.float32(0))]
        edges = np.zeros(4 * len(edge_vals), vx.SUN_POINT_DTYPE)
        for k in range(len(edges)):
            edges[k] = rnd[k]                                     # a cell anywhere in the grid, corners included below
            v, a = edge_vals[k // 4], k % 4
            edges["fract"][k] = v if a == 3 else edges["fract"][k]
            if a < 3:
                edges["fract"][k, a] = v
            edges["normal_idx"][k] = 4 if k % 3 == 0 else -1
        X, Y, Z = self.dims
        edges["cell"][0] = (0, 0, 0)
        edges["cell"][7] = edges["cell"][15] = edges["cell"][19] = (X - 1, Y - 1, Z - 1)     # fract -1 and < 2 at the far corner
        edges["cell"][12] = edges["cell"][16] = (0, 0, Z - 1)
        self._points = np.concatenate([faces, ground, rnd, edges])
        self.n_faces, self.n_ground = len(faces), len(ground)
        return self._points

    def reference(self, pts, suns, max_steps, key=None):
        """(words (n, W) uint32, culled pairs, marches, the oracle's summed fetches) for valid points."""
        if key is not None and (key, max_steps) in self._refs:
            return self._refs[key, max_steps]
        import oracle
        L, sc = oracle.lib(), C.byref(self.oracle.sc)
        ms = max_steps if max_steps > 0 else 2 * self.dims[2]
        k = len(suns)
        words = np.zeros((len(pts), 1 + (k + 31) // 32), np.uint32)
        dirs = [(C.c_float * 3)(*[float(v) for v in s]) for s in suns]
        culled = marches = fetches = 0
        m = oracle.OMarch()
        for i, p in enumerate(pts):
            cell = (C.c_int * 3)(*[int(v) for v in p["cell"]])
            fract = (C.c_float * 3)(*[float(v) for v in p["fract"]])
            n = int(p["normal_idx"])
            for j in range(k):
                if n >= 0:
                    along = suns[j][n >> 1] if n % 2 == 0 else -suns[j][n >> 1]          # float32
                    if suns[j][2] < np.float32(0) or not along > np.float32(0):
                        culled += 1
                        continue
                L.vxo_march(sc, cell, fract, dirs[j], ms, C.byref(m))
                marches += 1
                fetches += m.fetches
                if m.step == ms:
                    words[i, 1 + j // 32] |= np.uint32(1 << (j % 32))
                    words[i, 0] += 1
        out = (words, culled, marches, fetches)
        if key is not None:
            self._refs[key, max_steps] = out
        return out


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


def _same_words(got, ref, what):
    assert got.shape == ref.shape and got.dtype == ref.dtype == np.uint32, (what, got.shape, ref.shape)
    bad = np.argwhere(got != ref)
    assert len(bad) == 0, f"{what}: {len(bad)} words differ, first (point, word) {bad[:5].tolist()}: " \
                          f"{[hex(int(got[tuple(b)])) for b in bad[:5]]} != {[hex(int(ref[tuple(b)])) for b in bad[:5]]}"


def _popcount(words):
    return int(sum(bin(int(v)).count("1") for v in words.reshape(-1)))


# ---- the cases ------------------------------------------------------------------

@pytest.mark.parametrize("max_steps", [0, 5])
@pytest.mark.parametrize("world", list(SCENES), indirect=True)
def test_words_and_counters_match_the_oracle(world, max_steps):
    pts = world.points()
    ref, culled, marches, fetches = world.reference(pts, world.suns, max_steps, key="all")
    got, st = world.scene.query_sun(pts, world.suns, max_steps=max_steps, stats=True)
    plain, st_plain = world.scene.query_sun(pts, world.suns, max_steps=max_steps, flags=NO_EXIT, stats=True)
    print(f"{world.name} max_steps {max_steps}: {len(pts)} points, {marches} marches, {culled} culled, fetches "
          f"{st.fetches} default / {st_plain.fetches} NO_EXIT / {fetches} oracle, lit {st.lit}")
    _same_words(plain, ref, f"{world.name} NO_EXIT")
    _same_words(got, ref, f"{world.name} default")
    for s in (st, st_plain):
        assert s.points == len(pts) and s.invalid == 0
        assert s.rays == marches and s.culled == culled and s.rays + s.culled == len(pts) * K
        assert s.lit == _popcount(ref[:, 1:]) == int(ref[:, 0].sum())
        assert s.kernel_ms > 0
    assert st_plain.fetches == fetches, (st_plain.fetches, fetches)
    assert st.fetches <= st_plain.fetches
    # the set holds what it claims: faces with each outcome, every path of the march rule
    # (a one-layer field has no ground point: its blocks are in the top layer)
    assert world.n_faces >= 100 and (world.n_ground >= 100 or world.dims[2] == 1)
    assert len(pts) > world.n_faces + world.n_ground + 257
    assert culled > 0 and marches > culled
    if world.dims[2] > 1:
        assert 0 < st.lit < marches                       # lit and unlit marches both occur
    kind = world.scene.prepare_sun(world.frame(sun=tuple(world.suns[3])))["kind"]
    assert (kind == 0) == (world.name == "tall")          # no padded copy: march_fast over the u8 channels
    if world.name == "proc5" and max_steps == 0:
        assert st.fetches < st_plain.fetches              # the orthant exit copies end open-sky marches at once
    # bits at or past K are zero
    assert not (got[:, 2] >> np.uint32(K - 32)).any()


@pytest.mark.parametrize("n", [1, 63, 257])
def test_point_counts_cover_tail_lanes(world, n):
    import torch
    pts = world.points()
    ref, *_ = world.reference(pts, world.suns, 0, key="all")
    lo = world.n_faces - 20                              # a window over faces and ground points
    W = ref.shape[1]
    dev_p = torch.from_numpy(pts[lo:lo + n].copy().view(np.uint8)).cuda()
    dev_o = torch.full(((n + 3) * W,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    world.scene.query_sun_device(dev_p.data_ptr(), n, world.suns, dev_o.data_ptr())
    torch.cuda.synchronize()
    raw = dev_o.cpu().numpy().view(np.uint32)
    _same_words(raw[:n * W].reshape(n, W), ref[lo:lo + n], f"n = {n}")
    assert (raw[n * W:] == 0x5A5A5A5A).all(), "a tail lane stored past the last point"
    _same_words(world.scene.query_sun(pts[lo:lo + n], world.suns), ref[lo:lo + n], f"host n = {n}")


@pytest.mark.parametrize("world", ["proc5", "tall"], indirect=True)
def test_invalid_points_are_answered_not_marched(world):
    X, Y, Z = world.dims
    pts = world.points()
    good = pts[world.n_faces - 30:world.n_faces + 34]
    below_m1 = np.nextafter(np.float32(-1), np.float32(-np.inf))
    edits = [("cell", 0, -1), ("cell", 0, X), ("cell", 1, -1), ("cell", 1, Y), ("cell", 2, -1), ("cell", 2, Z),
             ("fract", 0, np.nan), ("fract", 1, np.float32(2.0)), ("fract", 2, below_m1), ("fract", 0, np.inf),
             ("normal_idx", None, 6), ("normal_idx", None, -2), ("cell", 0, np.iinfo(np.int32).min)]
    batch = np.zeros(3 * len(edits) + 1, world.vx.SUN_POINT_DTYPE)
    batch[:] = np.resize(good, len(batch))
    bad_at = 3 * np.arange(len(edits)) + 1
    for i, (field, axis, v) in zip(bad_at, edits):
        if axis is None:
            batch[field][i] = v
        else:
            batch[field][i, axis] = v
    ok = np.ones(len(batch), bool)
    ok[bad_at] = False
    ref = np.zeros((len(batch), world.vx.sun_words(K)), np.uint32)
    ref[ok], culled, marches, fetches = world.reference(batch[ok], world.suns, 0)
    ref[bad_at, 0] = INVALID
    for flags in (0, NO_EXIT):
        got, st = world.scene.query_sun(batch, world.suns, flags=flags, stats=True)
        _same_words(got, ref, f"{world.name} flags {flags}")
        assert (got[bad_at, 0] == INVALID).all() and not got[bad_at, 1:].any()
        assert st.points == len(batch) and st.invalid == len(edits)
        assert st.rays == marches and st.culled == culled and st.rays + st.culled == int(ok.sum()) * K
        if flags:
            assert st.fetches == fetches


def test_host_device_and_two_streams_give_the_same_words(world):
    import torch
    pts = world.points()
    host = world.scene.query_sun(pts, world.suns)
    a, b = pts[:1500], pts[700:]
    dev = [torch.from_numpy(p.copy().view(np.uint8)).cuda() for p in (a, b)]
    W = host.shape[1]
    outs = [[torch.zeros(len(p) * W, dtype=torch.int32, device="cuda") for _ in range(3)] for p in (a, b)]
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    for r in range(3):
        world.scene.query_sun_device(dev[0].data_ptr(), len(a), world.suns, outs[0][r].data_ptr(), stream=s1.cuda_stream)
        world.scene.query_sun_device(dev[1].data_ptr(), len(b), world.suns, outs[1][r].data_ptr(), stream=s2.cuda_stream,
                                     flags=NO_EXIT if r == 1 else 0)
    s1.synchronize()
    s2.synchronize()
    for r in range(3):
        _same_words(outs[0][r].cpu().numpy().view(np.uint32).reshape(len(a), W), host[:1500], f"stream 1 round {r}")
        _same_words(outs[1][r].cpu().numpy().view(np.uint32).reshape(len(b), W), host[700:], f"stream 2 round {r}")


def test_agreement_with_the_frame(world):
    """What a frame shades and what a query answers are one thing: for every pixel with a surface, word 0 of
    its first record's sun point is the frame's lit flag (Oracle.terms, slot 0); where the frame does not march
    (the face test fails: 255) it is 0."""
    vx = world.vx
    fr = world.frame(sun=FRAME_SUN, flags=vx.FLAG_UNIT_GBUF)
    lit = world.oracle.terms(fr.params, 48, 32)[0][..., 0].reshape(-1)
    rays = np.zeros(48 * 32, vx.RAY_DTYPE)
    for py in range(32):
        for px in range(48):
            rays[py * 48 + px] = vx.pixel_ray(fr, px, py)
    hits = world.scene.query_rays(rays)
    surface = hits["n"] >= 1
    # the condition on the case, from the oracle alone: marching pixels with both outcomes, culled surfaces
    assert not (lit[~surface] != 255).any()
    marching = surface & (lit != 255)
    assert marching.sum() >= 100 and (lit[marching] == 1).sum() >= 20 and (lit[marching] == 0).sum() >= 20
    assert (surface & (lit == 255)).sum() >= 20
    pts = vx.points_of_hits(hits)
    assert len(pts) == surface.sum()
    ms = fr.params.max_shadow_steps
    for flags in (0, NO_EXIT):
        got = world.scene.query_sun(pts, [FRAME_SUN], max_steps=ms, flags=flags)
        want = np.where(lit[surface] == 255, 0, lit[surface]).astype(np.uint32)
        bad = np.flatnonzero(got[:, 0] != want)
        assert len(bad) == 0, (flags, len(bad), bad[:5].tolist())
        assert np.array_equal(got[:, 1], want)            # k = 1: the mask word is the count


def test_sun_hours_is_the_ground_points_reference(world):
    vx = world.vx
    X, Y, Z = world.dims
    hours = np.linspace(-1.4, 1.4, 13)
    pts, cols = vx.ground_points(world.dev_field)
    suns = np.array([vx.sun_from_hour(h) for h in hours], np.float32)
    ref, *_ = world.reference(pts, suns, 0)
    want = np.zeros(X * Y, np.uint16)
    want[cols] = ref[:, 0]
    got = world.scene.sun_hours(hours)
    assert got.dtype == np.uint16 and got.shape == (Y, X)
    assert np.array_equal(got, want.reshape(Y, X))
    assert (want == 13).any() and ((want > 0) & (want < 13)).any()
