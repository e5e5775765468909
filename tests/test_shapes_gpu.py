"""Odd field shapes, box caps and noise sizes on the GPU against the oracle.

The shapes of tests/test_shapes.py (whose tables, camera and scenes this file
imports; that file holds the oracle to itself at the same inputs): fields whose
X and Y are no multiples of the doom builder's 8 x 8-cell blocks or lie below
one block, fields too flat for a cone plan or the LDS brick, a field too tall
for the padded march copy; box caps other than 64, which are also the border
width of the prim and quad copies; noise textures that are not square.  Per
case the field preparation is read back piece by piece against its restatement,
and 100 x 70 frames (ragged in both directions) are compared with the oracle's
on every fp32 word, every counter and the RGBA8 bytes.  The doom table shows
only in shadow_fetches (a table that is wrong but conservative gives the same
frame), so the counters are the point of the sun-quadrant cases: each sign of
the sun's x and y mirrors the builder's coordinates the other way.
"""
import numpy as np
import pytest

import test_shapes
from gpu_rig import Rig, assert_counters_equal, assert_words_equal, bin_scene, gpu_available, vis_colour
from test_shapes import (BASE, CAPS, DIMS, H, LIMIT, NOISE_SIZES, QUADRANT_SUNS, W, camera, field_of, grid_of, ids,
                         random_noise, scene_floors, sun_dir)

pytestmark = pytest.mark.gpu

FOUR = [BASE, (97, 53, 31)]         # rendered with suns in all four quadrants


class Case(Rig):
    """One scene on the device (dims, cap, noise), the copy it reads back as the
    oracle's field, and the oracle in each march mode over one set of boxes."""

    same = staticmethod(assert_words_equal)

    def __init__(self, dims, tex, cap=0, **kw):
        self.dims, self.cap, self.tex = dims, cap, tex
        self.field = field_of(dims)
        self._oracles = {}
        super().__init__(self.field, tex, dims, dist_cap=cap, **kw)

    def make_oracle(self, noise):
        return None                                     # check() names its own: oracle_in(mode)

    def oracle_in(self, mode=True):
        import oracle
        if mode not in self._oracles:
            first = next(iter(self._oracles.values()), None)
            self._oracles[mode] = oracle.Oracle(self.dev_field, self.tex, cap=self.cap or 64,
                                                oct_e=first.oct_e if first else None, exit=mode)
        return self._oracles[mode]

    def check(self, fr, mode=True, rgba8=True):
        """One frame against the oracle in `mode`: every fp32 word, every counter
        the oracle keeps, no cap hit, and the RGBA8 frame == the oracle's quantised.
        Returns the frame (the oracle's, which is the device's word for word)."""
        return super().check(fr, int_index=False, rgba8=rgba8, oracle=self.oracle_in(mode))


_cases = {}


@pytest.fixture(scope="module", autouse=True)
def _scenes(built):
    if not gpu_available():
        pytest.skip("no GPU visible")
    yield
    for c in _cases.values():
        c.close()
    _cases.clear()
    test_shapes._fields.clear()


def case_of(dims, noise, cap=0, hw=None):
    """The module's scene for (dims, cap, noise size); hw = None: the 1024 x 1024 texture."""
    key = (dims, cap, hw)
    if key not in _cases:
        _cases[key] = Case(dims, noise if hw is None else random_noise(*hw), cap)
    return _cases[key]


def _copies_equal_the_oracle(sc, field, cap):
    import oracle
    for o in range(8):
        dev, box = sc.read_field(o), sc.read_boxes(o)
        assert np.array_equal(dev[..., :3], field[..., :3]), o
        r = oracle.field_octant(field, o, cap)
        assert np.array_equal(dev[..., 3], r), o
        assert np.array_equal(box[..., 0], vis_colour(field[..., 2])), o
        assert np.array_equal(box[..., 1:], oracle.field_box(field, o, cap, r_cube=r)), o


# ---- the field preparation, piece by piece ----------------------------------------

@pytest.mark.parametrize("dims", DIMS, ids=ids)
def test_octant_and_box_copies(dims, noise):
    c = case_of(dims, noise)
    _copies_equal_the_oracle(c.scene, c.field, 64)


@pytest.mark.parametrize("chunk", [0, 5])
@pytest.mark.parametrize("dims", DIMS, ids=ids)
def test_face_quads(dims, chunk, noise):
    """CHUNK = Z and CHUNK = 5, which divides none of the dims."""
    import oracle
    field = field_of(dims)
    want = oracle.face_quads(field, chunk)
    if chunk == 0:
        got = case_of(dims, noise).scene.read_face_quads()
    else:
        with bin_scene(field, noise, dims, mesh_chunk=chunk) as sc:
            got = sc.read_face_quads()
    assert np.array_equal(got, want), int(np.count_nonzero(got != want))
    if dims[2] >= 2:
        assert (want != 0xFFFF).any()


@pytest.mark.parametrize("dims", DIMS, ids=ids)
def test_builders_and_grid_scene(dims, noise):
    """The field built on the device == on the host == the oracle's; the 2D mesh;
    and a scene made from the palette grid reads back what the scene made from
    the field does."""
    import oracle
    import voxmap_amd as vx
    grid = grid_of(dims)
    c = case_of(dims, noise)
    host = vx.field_build(grid)
    assert np.array_equal(vx.field_build_gpu(grid), host)
    assert np.array_equal(host, oracle.field_build(grid))
    assert c.scene.vertex2d() == vx.vertex2d(c.field)
    with vx.Scene(map_bytes=grid.tobytes(), map_format=vx.FORMAT_GRID, noise_bytes=noise.tobytes(),
                  noise_format=vx.FORMAT_BIN, dims=dims, device=0) as sc:
        for o in range(8):
            assert np.array_equal(sc.read_field(o), c.scene.read_field(o)), o
            assert np.array_equal(sc.read_boxes(o), c.scene.read_boxes(o)), o
        assert np.array_equal(sc.read_face_quads(), c.scene.read_face_quads())
        assert sc.vertex2d() == c.scene.vertex2d()
        info_a, info_b = sc.prepare_sun(camera(dims)), c.scene.prepare_sun(camera(dims))
        assert [info_a[k] for k in ("kind", "octant", "kx", "ky")] == [info_b[k] for k in ("kind", "octant", "kx", "ky")]


@pytest.mark.parametrize("dims", DIMS, ids=ids)
def test_prepare_sun_picks_the_oracles_plan(dims, noise):
    """vx_prepare_sun against oracle.exit_plan under the oracle's own rule for
    flat fields (no cone plan below Z = 3, Oracle.hold_exit_table); no copy at
    all on a field too tall for the padded march (Z > 126)."""
    import oracle
    import voxmap_amd as vx
    c = case_of(dims, noise)
    Z = dims[2]
    kinds, cones = set(), 0
    for el, az in QUADRANT_SUNS + [(10, 45), (60, 210)]:
        for n, radius in ((0, 0.0), (4, 0.02)):
            fr = camera(dims, sun=sun_dir(el, az), shadow_samples=n, sun_radius=radius)
            info = c.scene.prepare_sun(fr)
            d = oracle.sun_samples(fr.params.sun_dir[:], radius, n)
            cone, octs, kx, ky = oracle.exit_plan(d, allow_cone=Z >= 3)
            assert len(set(octs)) == 1 and octs[0] >= 0            # every sample in one octant, all fast
            if Z > 126:
                assert info["kind"] == 0, (el, az, n, info)
            elif cone:
                assert (info["kind"], info["octant"], info["kx"], info["ky"]) == (2, octs[0], kx, ky), (el, az, n)
            else:
                assert (info["kind"], info["octant"]) == (1, octs[0]), (el, az, n, info)
            kinds.add(info["kind"])
            cones += oracle.exit_plan(d)[0]
            fr.params.flags |= vx.FLAG_NO_EXIT
            assert c.scene.prepare_sun(fr)["kind"] == 0
    assert kinds == ({0} if Z > 126 else {1} if Z <= 2 else {1, 2})
    assert cones >= 8                                  # suns that take a cone plan where the field allows one


# ---- frames -----------------------------------------------------------------------

POOL, BRICK = 0x80, 0x100
MODES = {
    "v1": dict(flags=0),
    "full": dict(flags=0x30),
    "full_soft4": dict(flags=0x30, shadow_samples=4, sun_radius=0.02),
    "soft16_pool": dict(flags=0x30 | POOL, shadow_samples=16, sun_radius=0.03),
    "soft16_brick": dict(flags=0x30 | BRICK, shadow_samples=16, sun_radius=0.03),
    "general": dict(flags=0x2000 | 0x1000 | 0x30),           # REFLECT_ALL | GLASS_ORDER
    "quality0": dict(quality=0),
    "primary_only": dict(flags=0x8),
}
SUNLESS = ("primary_only",)                                 # no sun march: one sun is enough


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("dims", DIMS, ids=ids)
def test_frames_equal_the_oracle(dims, mode, noise):
    """Suns of opposite signs on x and y (all four quadrants on the two fields
    with partial doom blocks on both axes).  The 16-sample pooled frames also
    equal the per-sample frame; SOFT_POOL with its counters, SOFT_BRICK (which
    falls back to the pooled kernel where the brick does not fit: odd X, Z < 7)
    with the counters of a frame without the doom table, as the oracle counts it."""
    import oracle
    import voxmap_amd as vx
    assert (vx.FLAG_SOFT_POOL, vx.FLAG_SOFT_BRICK, vx.FLAG_REFLECT_ALL | vx.FLAG_GLASS_ORDER,
            vx.FLAG_PRIMARY_ONLY) == (POOL, BRICK, 0x3000, 0x8)
    c = case_of(dims, noise)
    suns = QUADRANT_SUNS[:1] if mode in SUNLESS else QUADRANT_SUNS if dims in FOUR else QUADRANT_SUNS[::2]
    for el, az in suns:
        kw = dict(MODES[mode])
        fr = camera(dims, sun=sun_dir(el, az), **kw)
        img, g = c.check(fr)
        if mode == "full" and (el, az) == QUADRANT_SUNS[0]:
            scene_floors(dims, c.oracle_in().render(fr.params, W, H)[1])
        if mode in ("soft16_pool", "soft16_brick"):
            kw["flags"] = 0x30
            base, gb = c.check(camera(dims, sun=sun_dir(el, az), **kw), rgba8=False)
            assert np.array_equal(img.view(np.uint32), base.view(np.uint32)), (el, az)
            if mode == "soft16_pool":
                assert_counters_equal(g, gb, keys=[k for k, _ in oracle.OStats._fields_])
            else:
                kw["flags"] = 0x30 | vx.FLAG_NO_DOOM
                _, gn = c.check(camera(dims, sun=sun_dir(el, az), **kw), rgba8=False)
                assert g["shadow_fetches"] == gn["shadow_fetches"] >= gb["shadow_fetches"]


@pytest.mark.parametrize("soft", [0, 4], ids=["hard", "soft4"])
@pytest.mark.parametrize("dims", FOUR, ids=ids)
def test_table_flags_change_no_pixel(dims, soft, noise):
    """NO_DOOM, NO_EXIT and NO_CONE: the default frame again, with the counters
    of the oracle in the matching mode; the tables never add a fetch."""
    import voxmap_amd as vx
    c = case_of(dims, noise)
    saved = 0
    for el, az in QUADRANT_SUNS:
        kw = dict(sun=sun_dir(el, az), shadow_samples=soft, sun_radius=0.02 if soft else 0.0)
        img, g = c.check(camera(dims, flags=0x30, **kw))
        fetches = {}
        for flag, mode in ((vx.FLAG_NO_DOOM, True), (vx.FLAG_NO_CONE, "orthant"), (vx.FLAG_NO_EXIT, False)):
            im2, g2 = c.check(camera(dims, flags=0x30 | flag, **kw), mode, rgba8=False)
            assert np.array_equal(im2.view(np.uint32), img.view(np.uint32)), (el, az, flag)
            fetches[flag] = g2["shadow_fetches"]
        assert g["shadow_fetches"] <= fetches[vx.FLAG_NO_DOOM] <= fetches[vx.FLAG_NO_EXIT]
        assert fetches[vx.FLAG_NO_CONE] <= fetches[vx.FLAG_NO_EXIT]
        saved += fetches[vx.FLAG_NO_DOOM] - g["shadow_fetches"]
    assert saved > 0                                    # the doom table is there, and read


@pytest.mark.parametrize("max_steps", [5, 12])
@pytest.mark.parametrize("dims", FOUR, ids=ids)
def test_short_step_budgets(dims, max_steps, noise):
    import voxmap_amd as vx
    c = case_of(dims, noise)
    for el, az in QUADRANT_SUNS:
        for soft in (0, 4):
            kw = dict(sun=sun_dir(el, az), shadow_samples=soft, sun_radius=0.02 if soft else 0.0,
                      max_shadow_steps=max_steps)
            img, _ = c.check(camera(dims, flags=0x30, **kw), rgba8=False)
            im2, _ = c.check(camera(dims, flags=0x30 | vx.FLAG_NO_DOOM, **kw), rgba8=False)
            assert np.array_equal(im2.view(np.uint32), img.view(np.uint32)), (el, az, soft)


@pytest.mark.parametrize("sun", [(0.6, 0.0, 0.8), (0.0, -0.6, 0.8), (0.8, 1e-4, 0.6), (-3e-4, 0.8, 0.6),
                                 (-3e-4, -0.8, 0.6)], ids=["y_zero", "x_zero", "y_tiny", "x_tiny", "x_tiny_y_neg"])
@pytest.mark.parametrize("dims", FOUR, ids=ids)
def test_suns_off_the_fast_path(dims, sun, noise):
    """A zero component (0 * inf = NaN in march(), render.frag:94-105) and one
    below the fast path's 2^-10 bound: the literal march.  Hard shadows, and soft
    ones through the per-sample loop, the pooled pass and the brick flag: with
    radius 0 every sample is the sun itself (all literal), with a radius the
    samples straddle the bound and the octants (fast and literal ones mixed).
    The counting kernels once summed wrong shadow_fetches here (113888 against
    115680 at 97 x 53 x 31, x_tiny, 4 samples; values near 1e11 with y negative)
    under frames that were right."""
    c = case_of(dims, noise)
    assert min(abs(v) for v in sun) < 2.0 ** -10
    c.check(camera(dims, sun=sun, flags=0x30))
    c.check(camera(dims, sun=sun), rgba8=False)
    for extra in (0, POOL, BRICK):
        for n, radius in ((4, 0.0), (4, 0.02), (16, 0.03)):
            c.check(camera(dims, sun=sun, flags=0x30 | extra, shadow_samples=n, sun_radius=radius), rgba8=False)
    c.check(camera(dims, sun=sun, shadow_samples=4, sun_radius=0.02), rgba8=False)


# ---- box caps ---------------------------------------------------------------------

@pytest.mark.parametrize("cap", CAPS)
def test_box_caps(cap, noise):
    """dist_cap is the cap of k_oct_x / k_oct_yz / k_oct_box and the border of
    the eight prim copies and the quad copy: the copies against the oracle's at
    the same cap, and a full-quality frame in two sun quadrants with every
    counter (primary_fetches: the walk takes the oracle's steps, box by box)."""
    c = case_of(BASE, noise, cap=cap)
    _copies_equal_the_oracle(c.scene, c.field, cap)
    for el, az in QUADRANT_SUNS[::2]:
        c.check(camera(BASE, sun=sun_dir(el, az), flags=0x30))
    c.check(camera(BASE, flags=0x2000 | 0x1000 | 0x30), rgba8=False)
    c.check(camera(BASE), rgba8=False)


def test_box_cap_at_the_limit(noise):
    """dist_cap = 255 on a 300-cell row: air runs longer than the 254 an extent
    byte holds.  The one large allocation of the file (about 14 GB of prim and
    quad copies): its own scene, closed at once."""
    import oracle
    dims, cap = LIMIT
    c = Case(dims, noise, cap)
    try:
        _copies_equal_the_oracle(c.scene, c.field, cap)
        assert int(oracle.field_box(c.field, 0, cap)[..., 0].max()) == cap - 1
        c.check(camera(dims))
        scene_floors(dims, c.oracle_in().render(camera(dims, flags=0x30).params, W, H)[1])
    finally:
        c.close()


# ---- noise sizes ------------------------------------------------------------------

@pytest.mark.parametrize("hw", NOISE_SIZES, ids=ids)
def test_noise_sizes(hw, noise):
    """Random textures that are not square (H x W; noise_size = (W, H)) and a
    single texel, full quality with clouds: the fbm plane (clouds) and the three
    white planes (rough surfaces) are read with the masks W - 1 and H - 1."""
    c = case_of(BASE, noise, hw=hw)
    for el, az in QUADRANT_SUNS[::2]:
        _, g = c.check(camera(BASE, sun=sun_dir(el, az), flags=0x30))
        assert g["noise_px"] > 0 and g["rough_px"] > 0 and g["sky_px"] > 0
    c.check(camera(BASE, flags=0x30, shadow_samples=4, sun_radius=0.02), rgba8=False)
    c.check(camera(BASE), rgba8=False)


def test_synthetic_noise_of_a_given_size():
    """No texture given: the scene synthesises noise_seed's at noise_size; the
    oracle is fed vx_noise_synth of the same seed and size."""
    import voxmap_amd as vx
    tex = vx.noise_synth(3, 64, 32)
    assert tex.shape == (32, 64, 4) and len(np.unique(tex)) > 16
    c = Case(BASE, None, noise_seed=3, noise_size=(64, 32))
    try:
        c.tex = tex
        _, g = c.check(camera(BASE, flags=0x30))
        assert g["noise_px"] > 0 and g["rough_px"] > 0
        c.check(camera(BASE, sun=sun_dir(*QUADRANT_SUNS[2])), rgba8=False)
    finally:
        c.close()
