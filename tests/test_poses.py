"""Degenerate camera poses on the CPU: the pose table and the oracle to itself.

Every other frame test builds its camera with the orbit helper: a handful of
generic poses, none with an axis-aligned basis, a zero cam_fract, or a camera
far from or on the grid.  The poses here are filled into a FrameParams by hand
(frame_from_basis) and reach what those miss in primary<> and walk_reflect:

  exact zero direction components (the IEEE-division / slab branch, taken by a
  wave with a lane whose component is 0: the centre column and row of an odd x
  odd frame under an axis-aligned basis); origins on cell faces and on the
  grid's faces (cam_fract 0, slab_lo == 0, slab_hi == 0); origins inside a
  solid or a glass cell and below the grid; cameras at |cell| 2^20, 2^21 and
  2^22 - 1, either side of the switch between the fp32 and the integer primary
  index; a hit at t = 0 (t0_hit: rayDir = normalize(0) = NaN); other times.

This file holds the conditions that keep tests/test_poses_gpu.py (which
imports the table) from being vacuous: what each pose shows, a census of the
pixel directions (vxo_pixel_dir) for the poses said to have exact zeros, and
the oracle's modes against each other.

Two statements of the table are geometry, not measurements.  A frame's
directions lie in one plane, and a plane meets at most seven of the eight
octants (six through the origin), so no single frame has all eight:
all_octants (fwd = 0, right = x, up = z; d.y == +0 on every pixel, which counts
positive) has the four (x, z) sign patterns with y positive, and its twin
all_octants_yneg (fwd.y = -2^-10) the four with y negative; both keep d.x == 0
on the centre column.  The kernel's wave is an 8 x 8-pixel tile, and at 65 x 32
the sign changes of x and z fall on tile edges (column 32, row 16), so both are
also rendered at 57 x 24, where they fall inside one tile (columns 24-31, rows
8-15), which then holds all four patterns and the zero lanes together.

The far cameras either side of a threshold do not give identical frames: the
ray parameter of a hit differs by one cell, and at t ~ 2^21 the point o + t*d
has a quarter-cell ulp, so hit points round differently.  That equality is
not asserted; each side is held to the floors below on its own."""
import numpy as np
import pytest

SEED, DIMS = 5, (96, 48, 16)
N_BOXES, N_GLASS = 16, 10
ODD, EVEN = (65, 33), (64, 40)      # a centre column and row with nx == 0, ny == 0 exactly; none
OCT, TILE = (65, 32), (57, 24)      # all_octants: never odd x odd (the centre pixel's d would be (0, 0, 0))
SUN = (0.5, 0.3, 0.8)
TIMES = [0.0, 0.001, 500.5, 999.999]

P21, P22, P20 = 1 << 21, 1 << 22, 1 << 20


def _pose(cell, fract, fwd, right, up, **tags):
    return dict(cell=cell, fract=fract, fwd=fwd, right=right, up=up, **tags)


def _far_x(x, s):
    """From x looking at the grid along x; right and up scaled by s so the frame spans it."""
    sg = 1.0 if x < 0 else -1.0
    return _pose((x, 24, 6), (.5, .5, .5), (sg, 0, 0), (0, -sg * 30 / s, 0), (0, 0, 12 / s), far=True)


def _far_y(y, s):
    sg = 1.0 if y < 0 else -1.0
    return _pose((48, y, 6), (.5, .5, .5), (0, sg, 0), (sg * 60 / s, 0, 0), (0, 0, 12 / s), far=True)


def _far_z(z, s):
    return _pose((48, 24, z), (.5, .5, .5), (0, 0, -1), (60 / s, 0, 0), (0, 30 / s, 0), far=True)


# name -> pose.  Tags: zeros (pixels with an exact zero component at ODD), glass (>= 100 glass pixels),
# far (a far camera), no_floor (not held to the 30 % cover floor).
POSES = {
    "down_axis": _pose((48, 24, 40), (.5, .5, 0), (0, 0, -1), (.6, 0, 0), (0, .4, 0), zeros=True, glass=True),
    "down_axis_f0": _pose((48, 24, 40), (0, 0, 0), (0, 0, -1), (.6, 0, 0), (0, .4, 0), zeros=True),
    "fract_negzero": _pose((48, 24, 40), (.5, -0.0, 0), (0, 0, -1), (.6, 0, 0), (0, .4, 0), zeros=True),
    "plus_x_axis": _pose((-30, 24, 6), (0, .5, .5), (1, 0, 0), (0, -.6, 0), (0, 0, .4), zeros=True),
    "minus_y_inside": _pose((48, 47, 5), (.25, .5, .75), (0, -1, 0), (.6, 0, 0), (0, 0, .4), zeros=True),
    "t0_hit": _pose((48, 47, 5), (.25, 0, .75), (0, -1, 0), (.6, 0, 0), (0, 0, .4), zeros=True, no_floor=True),
    "on_face_x0": _pose((0, 24, 6), (0, .5, .5), (1, 0, 0), (0, -.9, 0), (0, 0, .6), zeros=True),
    "on_face_xmax": _pose((96, 24, 6), (0, .5, .5), (-1, 0, 0), (0, .9, 0), (0, 0, .6), zeros=True),
    # sideways on the same two faces: d.x == 0 on the centre column.  At x = 0 slab_lo == 0 (the column is
    # inside the slab and walks the cells x = 0); at x = X slab_hi == 0 (0 < hi is false: the column misses)
    "side_x0": _pose((0, 24, 9), (0, .5, .5), (0, 1, -.5), (1.2, 0, 0), (0, 0, .5), zeros=True),
    "side_xmax": _pose((96, 24, 9), (0, .5, .5), (0, -1, -.5), (1.2, 0, 0), (0, 0, .5), zeros=True, no_floor=True),
    "up_from_below": _pose((48, 24, -20), (.5, .5, .5), (0, 0, 1), (.9, 0, 0), (0, .6, 0), zeros=True, glass=True),
    "sky_up": _pose((48, 24, 40), (.5, .5, .5), (0, 0, 1), (.9, 0, 0), (0, .6, 0), zeros=True, no_floor=True),
    "all_octants": _pose((48, 24, 8), (.5, .5, .5), (0, 0, 0), (1, 0, 0), (0, 0, 1), zeros=True, glass=True,
                         sizes=(OCT, TILE)),
    "all_octants_yneg": _pose((48, 24, 8), (.5, .5, .5), (0, -2.0 ** -10, 0), (1, 0, 0), (0, 0, 1), zeros=True,
                              sizes=(OCT, TILE)),
    "far_x_m21m1": _far_x(-(P21 - 1), P21), "far_x_m21": _far_x(-P21, P21), "far_x_m22m1": _far_x(-(P22 - 1), P22),
    "far_x_p21m1": _far_x(P21 - 1, P21), "far_x_p21": _far_x(P21, P21), "far_x_p22m1": _far_x(P22 - 1, P22),
    "far_y_p21m1": _far_y(P21 - 1, P21), "far_y_p21": _far_y(P21, P21), "far_y_m21": _far_y(-P21, P21),
    "far_y_p22m1": _far_y(P22 - 1, P22), "far_y_m22m1": _far_y(-(P22 - 1), P22),
    "far_z_20m1": _far_z(P20 - 1, P20), "far_z_20": _far_z(P20, P20), "far_z_22m1": _far_z(P22 - 1, P22),
    "far_diag": _pose((P22 - 1, P22 - 1, P21), (.5, .5, .5), (-1, -1 + 20 / P22, -.5 + 4 / P22),
                      (30 / P22, -30 / P22, 0), (0, 0, 10 / P22), far=True, glass=True),
}
POSES["far_x_m21m1"]["glass"] = POSES["far_x_m21"]["glass"] = POSES["far_x_m22m1"]["glass"] = True
GRID_POSES = ("in_solid", "in_glass")                       # their cells are picked from the grid (poses())
NAMES = list(POSES) + list(GRID_POSES)
# (fp32 side, integer side) of the automatic switch: |cell.x|, |cell.y| < 2^21 and |cell.z| < 2^20 -> fp32
THRESHOLDS = [("far_x_m21m1", "far_x_m21"), ("far_x_p21m1", "far_x_p21"), ("far_y_p21m1", "far_y_p21"),
              ("far_z_20m1", "far_z_20")]
MODES_2D = ("down_axis", "far_z_20m1", "far_z_20", "far_z_22m1", "up_from_below")

_state = {}


def grid():
    from voxmap_amd import scenes
    if "grid" not in _state:
        _state["grid"] = scenes.small_proc(SEED, dims=DIMS, n_boxes=N_BOXES, n_glass=N_GLASS)
    return _state["grid"]


def field():
    import oracle
    if "field" not in _state:
        _state["field"] = oracle.field_build(grid())
    return _state["field"]


def buried_cells():
    """(a solid cell whose six neighbours are solid, a glass cell), the first of each in index order."""
    from voxmap_amd import scenes
    g = grid()
    solid = (g >= 1) & (g < scenes.GLASS)
    inner = solid[1:-1, 1:-1, 1:-1].copy()
    for ax in range(3):
        for sh in (0, 2):
            sl = [slice(1, -1)] * 3
            sl[ax] = slice(sh, g.shape[ax] - 2 + sh)
            inner &= solid[tuple(sl)]
    zs, ys, xs = np.nonzero(inner)
    gz, gy, gx = np.nonzero(g == scenes.GLASS)
    assert len(zs) and len(gz)
    return (int(xs[0]) + 1, int(ys[0]) + 1, int(zs[0]) + 1), (int(gx[0]), int(gy[0]), int(gz[0]))


def poses():
    if "poses" not in _state:
        solid, glass = buried_cells()
        basis = dict(fract=(.5, .5, .5), fwd=(.3, .8, -.2), right=(.8, -.3, 0), up=(0, 0, .6))
        _state["poses"] = dict(POSES, in_solid=dict(cell=solid, **basis), in_glass=dict(cell=glass, **basis))
    return _state["poses"]


def sizes_of(name):
    return poses()[name].get("sizes", (ODD, EVEN))


def frame_from_basis(cell, fract, fwd, right, up, w, h, *, sun=SUN, time=123.0, quality=1, flags=0,
                     max_shadow_steps=0, shadow_samples=0, sun_radius=0.0):
    """A Frame filled by hand: the camera's cell and fraction and the ray basis (a pixel's direction is
    fwd + nx * right + ny * up), with no helper's arithmetic in between."""
    import voxmap_amd as vx
    p = vx.FrameParams()
    for i in range(3):
        p.cam_cell[i] = int(cell[i])
        p.cam_fract[i] = float(fract[i])
        p.ray_fwd[i], p.ray_right[i], p.ray_up[i] = float(fwd[i]), float(right[i]), float(up[i])
        p.sun_dir[i] = float(sun[i])
    p.time, p.quality, p.flags = float(time), int(quality), int(flags)
    p.max_shadow_steps, p.shadow_samples, p.sun_radius = int(max_shadow_steps), int(shadow_samples), float(sun_radius)
    return vx.Frame(p, int(w), int(h))


def frame_of(name, wh, **kw):
    q = poses()[name]
    return frame_from_basis(q["cell"], q["fract"], q["fwd"], q["right"], q["up"], wh[0], wh[1], **kw)


def pixel_dirs(o, fr):
    """(h, w, 3) float32 of vxo_pixel_dir."""
    return np.array([[o.pixel_dir(fr.params, fr.width, fr.height, px, py) for px in range(fr.width)]
                     for py in range(fr.height)], np.float32)


def octants(d):
    """The walk's octant per pixel: bit i set iff d_i < 0 (a zero counts as a positive axis)."""
    return (d[..., 0] < 0) * 1 + (d[..., 1] < 0) * 2 + (d[..., 2] < 0) * 4


@pytest.fixture(scope="module")
def orc(built, noise):
    """The oracle in the mode the GPU tests compare with, and its literal-march and unit-split forms."""
    import oracle
    ex = oracle.Oracle(field(), noise, exit=True)
    lit = oracle.Oracle(field(), noise, oct_e=ex.oct_e, exit=False, quad=ex.qoff)
    unit = oracle.Oracle(field(), noise, oct_e=ex.oct_e, exit=True, quad=False)
    yield ex, lit, unit
    _state.clear()


def test_the_field_and_the_buried_cells(orc):
    from voxmap_amd import scenes
    g = grid()
    assert g.shape == DIMS[::-1]
    (sx, sy, sz), (gx, gy, gz) = buried_cells()
    assert 1 <= g[sz, sy, sx] < scenes.GLASS and g[gz, gy, gx] == scenes.GLASS
    for dx, dy, dz in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)):
        assert 1 <= g[sz + dz, sy + dy, sx + dx] < scenes.GLASS
    # t0_hit: the camera cell is air and the cell at -y is a block, so the camera at fract.y = 0 lies on its face
    q = POSES["t0_hit"]
    x, y, z = q["cell"]
    assert g[z, y, x] == 0 and 1 <= g[z, y - 1, x] < scenes.GLASS and q["fract"][1] == 0
    assert set(NAMES) == set(poses())


@pytest.mark.parametrize("name", NAMES)
def test_pose_floors(name, orc):
    """What a pose shows at v1 flags, from the oracle alone: blocks or glass on >= 30 % of the pixels (but for
    the all-sky pose, the sideways pose whose centre column must miss, and t0_hit, held to their own conditions
    below), no cap hit, no NaN; >= 100 glass pixels on the glass poses."""
    ex = orc[0]
    q = poses()[name]
    for wh in sizes_of(name):
        img, st = ex.render(frame_of(name, wh).params, *wh)
        assert not np.isnan(img).any() and st.primary_cap_hits == 0 and st.pixels == wh[0] * wh[1]
        assert st.sky_px + st.block_px + st.glass_px == st.pixels
        if not q.get("no_floor"):
            assert 10 * (st.block_px + st.glass_px) >= 3 * st.pixels, (wh, st.sky_px, st.block_px, st.glass_px)
        if q.get("glass"):
            assert st.glass_px >= 100, (wh, st.glass_px)


def test_threshold_pairs_straddle_the_switch():
    """vx_render walks with the fp32 index iff |cam_cell.x|, |cam_cell.y| < 2^21 and |cam_cell.z| < 2^20: each
    pair has one pose on either side, one cell apart, and every far pose keeps |cell| < 2^22."""
    def fp32(c):
        return abs(c[0]) < P21 and abs(c[1]) < P21 and abs(c[2]) < P20

    for a, b in THRESHOLDS:
        ca, cb = POSES[a]["cell"], POSES[b]["cell"]
        assert fp32(ca) and not fp32(cb) and sum(abs(abs(x) - abs(y)) for x, y in zip(ca, cb)) == 1
    far = [q["cell"] for q in POSES.values() if q.get("far")]
    assert all(max(abs(v) for v in c) < P22 for c in far)
    assert sum(fp32(c) for c in far) == len(THRESHOLDS) and any(max(abs(v) for v in c) == P22 - 1 for c in far)


def test_sky_up_is_all_sky_with_clouds(orc):
    for wh in (ODD, EVEN):
        _, st = orc[0].render(frame_of("sky_up", wh).params, *wh)
        assert st.sky_px == st.pixels and st.noise_px > 0


def test_time_moves_the_clouds(orc):
    frames = [orc[0].render(frame_of("sky_up", ODD, time=t).params, *ODD)[0] for t in TIMES]
    assert sum(not np.array_equal(frames[0].view(np.uint32), f.view(np.uint32)) for f in frames[1:]) >= 1
    assert not any(np.isnan(f).any() for f in frames)


def test_sideways_on_the_grid_faces(orc):
    """d.x == 0 on the centre column.  On x = 0 (slab_lo == 0) the column is inside the slab: it sees what the
    column beside it sees, block for block; on x = X (slab_hi == 0) it misses, and so does everything on the
    side that looks away from the grid."""
    ex = orc[0]
    w, h = ODD
    cx = w // 2
    for name, inside in (("side_x0", True), ("side_xmax", False)):
        fr = frame_of(name, ODD)
        d = pixel_dirs(ex, fr)
        assert (d[:, cx, 0] == 0).all() and (d[:, :cx, 0] < 0).all() and (d[:, cx + 1:, 0] > 0).all()
        img, st = ex.render(frame_of(name, ODD, flags=0x8).params, w, h)        # PRIMARY_ONLY
        sky, _ = ex.render(frame_of("sky_up", ODD, flags=0x8).params, w, h)
        hit = np.array([[ex.primary(fr.params, d[py, px])[0] > 0 for px in range(w)] for py in range(h)])
        if inside:
            assert hit[:, cx].sum() >= h // 3 and not hit[:, :cx].any() and hit[:, cx + 1:].sum() >= w * h // 3
        else:
            assert not hit[:, cx:].any() and hit[:, :cx].sum() >= w * h // 4
        assert st.block_px + st.glass_px == int(hit.sum())


@pytest.mark.parametrize("name", [n for n, q in POSES.items() if q.get("zeros")])
def test_direction_census(name, orc):
    """The poses said to have exact zeros have them: at the odd x odd size (the all_octants pair: at both of
    theirs) some pixel has a component == 0.0 and no pixel has d == (0, 0, 0); at the even size none has a zero.
    An 8 x 8-pixel tile is one wave: a tile with a zero lane and a non-zero lane takes the IEEE branch with
    both kinds of lane in it."""
    ex = orc[0]
    sizes = sizes_of(name)
    for wh in sizes:
        d = pixel_dirs(ex, frame_of(name, wh))
        zero = (d == 0).any(axis=2)
        assert not (d == 0).all(axis=2).any()
        if wh == EVEN:
            assert not zero.any()
            continue
        assert zero.any(), wh
        mixed = 0
        for y0 in range(0, wh[1], 8):
            for x0 in range(0, wh[0], 8):
                z = zero[y0:y0 + 8, x0:x0 + 8]
                mixed += z.any() and not z.all()
        assert mixed >= 1 or zero.all()
        if zero.all():                                     # all_octants: d.y == 0 on every pixel
            assert name == "all_octants" and ((d[..., 0] == 0) & (d[..., 2] != 0)).any()


def test_all_octants_between_them(orc):
    """The pair covers the eight octants, four each (a frame's directions lie in a plane); at 57 x 24 one tile
    holds the frame's four and its zero lanes, at 65 x 32 (sign changes on tile edges) each 32 x 8 block one."""
    ex = orc[0]
    seen = set()
    for name, want in (("all_octants", {0, 1, 4, 5}), ("all_octants_yneg", {2, 3, 6, 7})):
        d = pixel_dirs(ex, frame_of(name, TILE))
        o = octants(d)
        assert set(np.unique(o).tolist()) == want
        best = max((len(set(np.unique(o[y:y + 8, x:x + 8]).tolist())), bool((d[y:y + 8, x:x + 8, 0] == 0).any()))
                   for y in range(0, TILE[1], 8) for x in range(0, TILE[0], 8))
        assert best == (4, True), best
        d = pixel_dirs(ex, frame_of(name, OCT))
        o = octants(d)
        assert set(np.unique(o).tolist()) == want
        assert all(len(np.unique(o[y:y + 8, x:x + 32])) == 1 for y in range(0, 32, 8) for x in range(0, 65, 32))
        seen |= want
    assert seen == set(range(8))


@pytest.mark.parametrize("name", NAMES)
def test_oracle_modes_agree(name, orc):
    """exit=True against the literal march: one frame, full quality hard and soft; the unit split against the
    quad split in what does not depend on the split (what each pixel is, and the walk's fetches)."""
    ex, lit, unit = orc
    wh = sizes_of(name)[0]
    for kw in (dict(flags=0x30), dict(flags=0x30, shadow_samples=4, sun_radius=0.03), dict(flags=0)):
        p = frame_of(name, wh, **kw).params
        a, sa = ex.render(p, *wh)
        b, sb = lit.render(p, *wh)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), kw
        assert sa.shadow_fetches <= sb.shadow_fetches
        for k in ("pixels", "sky_px", "block_px", "glass_px", "primary_fetches", "shadow_rays", "reflect_rays",
                  "reflect_fetches", "primary_cap_hits"):
            assert getattr(sa, k) == getattr(sb, k), (k, kw)
    p = frame_of(name, wh).params
    _, sa = ex.render(p, *wh)
    _, su = unit.render(p, *wh)
    for k in ("pixels", "sky_px", "block_px", "glass_px", "primary_fetches", "primary_cap_hits"):
        assert getattr(sa, k) == getattr(su, k), k
    # the frame's own flag is the same split
    pu = frame_of(name, wh, flags=0x800).params
    a, _ = ex.render(pu, *wh)
    b, _ = unit.render(p, *wh)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_t0_hit_is_nan_under_reflect_all_only(orc):
    """The camera lies on the face it looks at: every view ray hits at t = 0, rayDir = normalize(0) = NaN
    (DESIGN.md §5).  A block's colour does not read rayDir, so the v1 and full-quality frames are finite; with
    REFLECT_ALL every pixel's Fresnel weight is NaN and so is its RGB (alpha stays 1).  A mirror ray whose
    direction is not finite is not walked: it is counted, fetches nothing and is the sky along it (one
    cloud lookup each, nothing else).  The twin pose half a cell back is finite, at one fetch per mirror ray."""
    ex = orc[0]
    w, h = ODD
    for flags in (0, 0x30, 0x8, 0x800):
        img, st = ex.render(frame_of("t0_hit", ODD, flags=flags).params, w, h)
        assert not np.isnan(img).any() and st.block_px == w * h and st.reflect_rays == 0
    img, st = ex.render(frame_of("t0_hit", ODD, flags=0x2030).params, w, h)
    assert np.isnan(img[..., :3]).all() and (img[..., 3] == 1).all()
    base = ex.render(frame_of("t0_hit", ODD, flags=0x30).params, w, h)[1]
    assert st.reflect_rays == w * h and st.reflect_fetches == 0
    assert st.noise_px == base.noise_px + w * h
    for k in ("ao_samples", "shadow_rays", "shadow_fetches", "rough_px", "primary_fetches"):
        assert getattr(st, k) == getattr(base, k), k       # the mirror rays add nothing else
    img, st = ex.render(frame_of("minus_y_inside", ODD, flags=0x2030).params, w, h)
    assert not np.isnan(img).any() and st.reflect_rays == w * h == st.reflect_fetches
