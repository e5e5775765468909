"""Odd field shapes, box caps and noise sizes on the CPU.

Every other frame test renders a field whose X and Y are multiples of 8, with
the default box cap (64) and the square 1024 x 1024 noise texture.  The shapes
here are the smallest that reach the paths those miss (SHAPES below); the
scenes come from scenes.odd_proc, which is valid at any dims and puts blocks on
the far faces of the grid.  This file holds the oracle to itself at those
inputs (its three march modes give one frame), the host builders to the oracle,
and the scenes to floors on what a frame sees, so that tests/test_shapes_gpu.py
(which imports the tables and helpers below) compares the kernels with a sound
reference on frames that are not empty."""
import numpy as np
import pytest

from gpu_rig import sun_dir

SEED = 1
W, H = 100, 70                      # ragged in both directions (not multiples of the 8 x 8 pixel block)

# dims -> what the shape reaches
SHAPES = {
    (37, 29, 11): "odd X and Y; partial doom blocks on both axes; SXp & 3 != 0",
    (61, 7, 13): "Y below one doom block",
    (5, 43, 9): "X below one doom block",
    (33, 12, 40): "Z > Y; chunk = Z = 40 > 32: no quad copy",
    (97, 53, 31): "prime dims; several full doom blocks plus a partial one",
    (50, 30, 2): "Z < 3: orthant tables only, no cone; Z < 7: no brick",
    (41, 23, 1): "Z = 1",
    (24, 20, 127): "Z > 126: no padded march copy; kind 0 from vx_prepare_sun",
}
DIMS = list(SHAPES)
BASE = (37, 29, 11)                 # the field of the cap and noise cases
CAPS = [1, 2, 7, 33, 128]
LIMIT = ((300, 9, 5), 255)          # an air row longer than the 254 a byte holds as an extent
NOISE_SIZES = [(16, 64), (64, 16), (2, 8), (1, 1)]          # (H, W)

# (elevation, azimuth) with r_z > 0 in the four (r_x, r_y) sign quadrants: ++, -+, --, +-
QUADRANT_SUNS = [(33, 30), (40, 120), (25, 250), (20, 300)]


def ids(dims):
    return "x".join(str(v) for v in dims)


def grid_of(dims):
    from voxmap_amd import scenes
    return scenes.odd_proc(SEED, dims)


def camera(dims, **kw):
    """The one camera of every case: above the middle of the field, looking down at 1 rad."""
    import voxmap_amd as vx
    X, Y, Z = dims
    kw.setdefault("sun", sun_dir(*QUADRANT_SUNS[0]))
    return vx.make_frame((X / 2, Y / 2, 0.1 * max(X, Y) + 0.5 * Z + 2), (1.0, 0, 0.6), W, H, **kw)


def random_noise(h, w):
    """A seeded random RGBA8 texture (h, w, 4): a swap of the W and H masks reads other texels."""
    return np.random.default_rng(1000 * h + w).integers(0, 256, (h, w, 4), dtype=np.uint8)


def scene_floors(dims, st):
    """The scene condition, from the oracle's counters of a full-quality frame:
    a case's frame sees blocks or glass on >= 10 % of its pixels and marches
    >= 300 shadow rays.  The limit field (300, 9, 5) is a strip 9 cells wide
    seen from 34 cells above: its bare ground fills 7.3 % of the frame and no
    scene on it reaches 10 % (test_the_limit_strip_cannot_fill_a_tenth_of_the_frame:
    fewer than a tenth of the view rays meet the grid's box at all), so it is
    held to the shadow-ray floor alone."""
    d = st.as_dict()
    assert d["shadow_rays"] >= 300, (dims, d["shadow_rays"])
    if tuple(dims) != LIMIT[0]:
        assert 10 * (d["block_px"] + d["glass_px"]) >= d["pixels"], (dims, d["block_px"], d["glass_px"])
    return d


_fields = {}


def field_of(dims):
    import voxmap_amd as vx
    if dims not in _fields:
        _fields[dims] = vx.field_build(grid_of(dims))
    return _fields[dims]


@pytest.fixture(scope="module", autouse=True)
def _native(built):
    yield
    _fields.clear()


def _modes(field, noise, cap=64):
    """The oracle in its three march modes over one set of boxes."""
    import oracle
    lit = oracle.Oracle(field, noise, cap=cap, exit=False)
    return lit, oracle.Oracle(field, noise, cap=cap, oct_e=lit.oct_e, exit=True), \
        oracle.Oracle(field, noise, cap=cap, oct_e=lit.oct_e, exit="orthant")


def _one_frame_in_three_modes(dims, field, noise, cap=64):
    """Hard and 4-sample soft shadows in two opposite sun quadrants: the three
    modes give the same words, no NaN, no cap hit, and the tables never add a
    shadow fetch.  Returns the hard full-quality counters of the first sun."""
    lit, ex, orth = _modes(field, noise, cap)
    first = None
    for el, az in (QUADRANT_SUNS[0], QUADRANT_SUNS[2]):
        for n, radius in ((0, 0.0), (4, 0.02)):
            fr = camera(dims, sun=sun_dir(el, az), flags=0x30, shadow_samples=n, sun_radius=radius)
            a, sa = lit.render(fr.params, W, H)
            b, sb = ex.render(fr.params, W, H)
            c, sc = orth.render(fr.params, W, H)
            assert not np.isnan(a).any()
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (dims, cap, el, az, n)
            assert np.array_equal(a.view(np.uint32), c.view(np.uint32)), (dims, cap, el, az, n)
            assert sa.primary_cap_hits == 0 and sb.primary_cap_hits == 0
            assert sb.shadow_fetches <= sa.shadow_fetches and sc.shadow_fetches <= sa.shadow_fetches, (dims, cap, el, az, n)
            for k in ("pixels", "block_px", "glass_px", "shadow_rays", "primary_fetches"):
                assert getattr(sa, k) == getattr(sb, k) == getattr(sc, k), k
            first = first or sb
    return first


def test_odd_proc_is_deterministic_and_reaches_the_far_faces():
    from voxmap_amd import scenes
    for dims in DIMS + [LIMIT[0], (3, 3, 3), (1, 1, 1), (2, 1, 6), (1, 9, 2)]:
        X, Y, Z = dims
        g = scenes.odd_proc(SEED, dims)
        assert g.shape == (Z, Y, X) and g.dtype == np.uint8 and int(g.max()) <= scenes.GLASS
        assert np.array_equal(g, scenes.odd_proc(SEED, dims))
        solid = (g >= 1) & (g <= 20)
        assert solid[:, 0, 0].all() and solid[:, Y - 1, X - 1].all()          # the two columns, up to z = Z - 1
        if Z >= 2 and min(X, Y) >= 3:
            assert solid[1:, :, X - 1].sum() > Z - 1 and solid[1:, Y - 1, :].sum() > Z - 1    # more than the column
        if Z >= 5 and min(X, Y) >= 3:
            assert (solid[Z - 1] & ~(g[Z - 2] > 0)).any()                     # the slab, with air beneath
        if Z == 1 and X * Y >= 100:
            assert (g[0] == 0).any() and (g[0] == 13).any() and (g[0] == 2).any()
        if X * Y >= 9:
            assert (g == scenes.GLASS).any()
    assert not np.array_equal(scenes.odd_proc(SEED, BASE), scenes.odd_proc(SEED + 1, BASE))
    # small_proc's ranges go empty on these shapes; it stays as it is (golden files depend on it)
    with pytest.raises(ValueError):
        scenes.small_proc(SEED, dims=(5, 43, 9))


@pytest.mark.parametrize("dims", DIMS + [LIMIT[0], (3, 3, 3)], ids=ids)
def test_oracle_march_modes_agree_and_scene_floors(dims, noise):
    st = _one_frame_in_three_modes(dims, field_of(dims), noise, LIMIT[1] if dims == LIMIT[0] else 64)
    if dims != (3, 3, 3):
        scene_floors(dims, st)


def test_at_least_half_of_the_shapes_show_glass(noise):
    import oracle
    seen = 0
    for dims in DIMS:
        _, st = oracle.Oracle(field_of(dims), noise, exit=True).render(camera(dims, flags=0x30).params, W, H)
        seen += st.glass_px > 0
    assert 2 * seen >= len(DIMS), seen


@pytest.mark.parametrize("cap", CAPS + [32, 255])
def test_oracle_box_caps(cap, noise):
    """Oracle(cap=): one frame in every march mode; the cube of an octant is the
    smallest extent of its box, and neither reaches the cap (a box runs on
    past the grid's faces, so every cap bounds some box)."""
    import oracle
    field = field_of(BASE)
    st = _one_frame_in_three_modes(BASE, field, noise, cap)
    scene_floors(BASE, st)
    for o in (0, 7):
        r = oracle.field_octant(field, o, cap)
        e = oracle.field_box(field, o, cap)
        assert int(e.max()) <= cap - 1 and np.array_equal(e.min(axis=3), r)


@pytest.mark.parametrize("hw", NOISE_SIZES, ids=ids)
def test_oracle_noise_sizes(hw):
    h, w = hw
    tex = random_noise(h, w)
    field = field_of(BASE)
    _one_frame_in_three_modes(BASE, field, tex)
    if h != w:
        # the same bytes read as the transposed size give another frame: W and H are told apart
        import oracle
        fr = camera(BASE, flags=0x30)
        a, _ = oracle.Oracle(field, tex, exit=True).render(fr.params, W, H)
        b, _ = oracle.Oracle(field, tex.reshape(w, h, 4), exit=True).render(fr.params, W, H)
        assert not np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("dims", DIMS + [LIMIT[0]], ids=ids)
def test_host_builders_equal_the_oracle(dims):
    """vx_field_build == vxo_field_build, and vx_vertex2d == the oracle's
    footprint meshed by the restated 2D mesher; footprint_2d carries the same
    quads' corners."""
    import oracle
    import voxmap_amd as vx
    from oracle import mesh_ref
    grid = grid_of(dims)
    field = field_of(dims)
    assert np.array_equal(field, oracle.field_build(grid))
    c = oracle.footprint(field)
    quads = mesh_ref.mesh2d(np.where(c == 0, 22, c).T.copy())
    v2d = vx.vertex2d(field)
    assert v2d == mesh_ref.vertex2d_bytes(quads)
    fp = oracle.footprint_2d(field)
    assert np.array_equal(fp[..., 0], c)
    rec = np.frombuffer(v2d, mesh_ref.REC2D).reshape(-1, 6)
    assert len(rec) == len(quads)
    if dims[2] >= 2:
        assert len(rec) > 0
    for q in rec:
        x, y = int(q[0]["p"][0]), int(q[0]["p"][1])
        w, h = int(q["d"][:, 0].max()), int(q["d"][:, 1].max())
        assert (fp[y:y + h, x:x + w, 1] == (x | (y << 16))).all() and (fp[y:y + h, x:x + w, 0] == q[0]["c"]).all()


@pytest.mark.parametrize("el,az", QUADRANT_SUNS)
def test_frames_read_the_doom_codes_of_the_partial_blocks(el, az, noise):
    """A condition on the scene, like the floors: at (37, 29, 11) the frame of
    each sun quadrant lands shadow rays on doomed cells of the partial 8 x 8-cell
    block row and of the partial block column, in the sun-aligned coordinates
    the doom builder works in (x' = x for a sun with r_x > 0, else X - 1 - x:
    the cells x' >= X - X % 8 are the last 5 on the side the sun shines from).
    With those codes zeroed in a held table the frame keeps every pixel and
    takes more shadow fetches, so a device table that is wrong there, for
    either mirror branch, cannot give the oracle's shadow_fetches."""
    import oracle
    o = oracle.Oracle(field_of(BASE), noise, exit=True)
    fr = camera(BASE, sun=sun_dir(el, az), flags=0x30)
    assert o.hold_exit_table(fr.params) is not None
    table = o._held_doom                                   # (Z, Y, X), read in place by the renders below
    keep = table.copy()
    img, st = o.render(fr.params, W, H)
    for axis in (0, 1):
        n, part = BASE[axis], BASE[axis] % 8
        cells = slice(n - part, n) if fr.params.sun_dir[axis] > 0 else slice(0, part)
        table[...] = keep
        table[(slice(None), slice(None), cells) if axis == 0 else (slice(None), cells)] = 0
        assert int((table > 0).sum()) < int((keep > 0).sum())
        img2, st2 = o.render(fr.params, W, H)
        assert np.array_equal(img.view(np.uint32), img2.view(np.uint32))
        assert st2.shadow_fetches > st.shadow_fetches, (axis, st.shadow_fetches)
    table[...] = keep
    assert o.render(fr.params, W, H)[1].shadow_fetches == st.shadow_fetches


def test_the_limit_strip_cannot_fill_a_tenth_of_the_frame(built):
    """Why scene_floors waives the cover floor at (300, 9, 5): with the camera
    every case shares, fewer than 10 % of the frame's view rays cross the
    grid's box [0, X] x [0, Y] x [0, Z], and only those can show a block or a
    pane.  Every other shape's box is crossed by more."""
    import oracle
    o = oracle.Oracle(field_of((3, 3, 3)), np.zeros((1, 1, 4), np.uint8))

    def crossing(dims):
        p = camera(dims).params
        org = np.array([p.cam_cell[i] + p.cam_fract[i] for i in range(3)], np.float64)
        d = np.array([o.pixel_dir(p, W, H, px, py) for py in range(H) for px in range(W)], np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            t0, t1 = (0.0 - org) / d, (np.array(dims, np.float64) - org) / d
        lo, hi = np.minimum(t0, t1).max(axis=1), np.maximum(t0, t1).min(axis=1)
        return int(np.count_nonzero((hi >= lo) & (hi > 0)))

    assert 10 * crossing(LIMIT[0]) < W * H
    for dims in DIMS:
        assert 10 * crossing(dims) >= W * H, dims
