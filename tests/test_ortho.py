"""Orthographic frames on the CPU: the pixel ray and the camera helper against
their definitions, and the oracle-assembled frames that tests/test_ortho_gpu.py
(which imports the views, the builder and the assembler from here) compares the
kernel with.

The definition (include/voxmap.h): pixel (x, y) of an orthographic frame is the
single pixel of the 1 x 1 perspective frame whose camera is that pixel's origin
(vx_pixel_ray_ortho) with ray_right = ray_up = 0.  assemble() builds a frame
that way from the unchanged oracle, one 1 x 1 render per pixel, and sums the
counters.  The census below keeps the GPU comparison from being vacuous: each
view must really show the sky, blocks, glass, stacked panes, lit and shadowed
pixels it is there for.
"""
import ctypes as C
import math

import numpy as np
import pytest

import test_poses
from test_poses import frame_from_basis

SUN = test_poses.SUN
BIG, SMALL = (64, 40), (57, 23)        # whole 8 x 8 tiles; partial tiles on both edges
P21 = 1 << 21
ODD_SEED, ODD_DIMS = 3, (61, 37, 11)
F1 = float(np.nextafter(np.float32(1), np.float32(0)))     # 0x1.fffffep-1


def _view(cell, fract, right, up, fwd, field="main"):
    return dict(cell=cell, fract=fract, right=right, up=up, fwd=fwd, field=field)


DOWN, UP = (0, 0, -1), (0, 0, 1)
ISO = (.4, .8, -.9)
VIEWS = {
    "plan": _view((48, 24, 20), (.5, .5, 0), (48, 0, 0), (0, 24, 0), DOWN),
    "plan_up": _view((48, 24, -4), (.5, .5, .5), (48, 0, 0), (0, 24, 0), UP),
    "iso": _view((20, -10, 40), (.5, .5, .5), (40, -20, 0), (10, 20, 22), ISO),
    "elev_y": _view((48, -6, 8), (.5, .5, 0), (48, 0, 0), (0, 0, 8), (0, 1, 0)),
    "elev_x": _view((100, 24, 8), (.5, .5, .25), (0, 24, 0), (0, 0, 8), (-1, 0, 0)),
    "section": _view((48, 24, 8), (.5, .5, .5), (40, 0, 0), (0, 0, 8), (0, -1, 0)),
    "far_elev_y": _view((48, -P21, 8), (.5, .5, 0), (48, 0, 0), (0, 0, 8), (0, 1, 0)),
    "far_plan": _view((48, 24, P21), (.5, .5, 0), (48, 0, 0), (0, 24, 0), DOWN),
    "edge": _view((0, 0, 20), (0, 0, 0), (60, 0, 0), (0, 30, 0), DOWN),
    "plan_odd": _view((30, 18, 14), (.5, .5, 0), (32, 0, 0), (0, 20, 0), DOWN, field="odd"),
    "iso_odd": _view((10, -8, 30), (.5, .5, .5), (30, -14, 0), (8, 16, 18), ISO, field="odd"),
}
MAIN = ["plan", "plan_up", "iso", "elev_y", "elev_x", "section"]          # at both sizes
EXTRA = ["far_elev_y", "far_plan", "edge", "plan_odd", "iso_odd"]         # at SMALL
CASES = [(n, wh) for n in MAIN for wh in (BIG, SMALL)] + [(n, SMALL) for n in EXTRA]

_state = {}


def odd_field():
    import oracle
    from voxmap_amd import scenes
    if "odd" not in _state:
        _state["odd"] = oracle.field_build(scenes.odd_proc(ODD_SEED, ODD_DIMS))
    return _state["odd"]


def field_of(name):
    return odd_field() if VIEWS[name]["field"] == "odd" else test_poses.field()


def frame_of(name, wh, **kw):
    v = VIEWS[name]
    return frame_from_basis(v["cell"], v["fract"], v["fwd"], v["right"], v["up"], wh[0], wh[1], **kw)


def origins(p, w, h):
    """vx_pixel_ray_ortho's formula restated in numpy float32, for every pixel: (cells (h, w, 3) int32,
    fracts (h, w, 3) float32).  One rounding per operation, in the header's order."""
    f32 = np.float32
    nx = (2 * np.arange(w) + 1).astype(f32) / f32(w) - f32(1)
    ny = f32(1) - (2 * np.arange(h) + 1).astype(f32) / f32(h)
    cells, fracts = np.empty((h, w, 3), np.int32), np.empty((h, w, 3), f32)
    for i in range(3):
        a = (nx[None, :] * f32(p.ray_right[i])) + (ny[:, None] * f32(p.ray_up[i]))
        s = f32(p.cam_fract[i]) + a
        fl = np.floor(s)
        assert a.dtype == s.dtype == fl.dtype == f32
        cells[..., i] = p.cam_cell[i] + fl.astype(np.int32)
        fracts[..., i] = np.minimum(s - fl, f32(F1))
    return cells, fracts


def pixel_params(p, cell, fract):
    """E(x, y): p with the camera at the pixel's origin and ray_right = ray_up = 0."""
    e = p.copy()
    for i in range(3):
        e.cam_cell[i], e.cam_fract[i] = int(cell[i]), float(fract[i])
        e.ray_right[i] = e.ray_up[i] = 0.0
    return e


def assemble(o, fr, census=False):
    """The orthographic frame of fr from 1 x 1 frames of oracle o (its exit table held by the caller):
    (frame (h, w, 4) float32, the summed counters as a dict[, kind, panes, lit]).  census: per pixel,
    kind 0 sky / 1 block / 2 glass, the glass panes in front of its surface, and the first surface's
    sun march (1 lit, 0 shadowed, 255 none)."""
    p, w, h = fr.params, fr.width, fr.height
    cells, fracts = origins(p, w, h)
    img = np.empty((h, w, 4), np.float32)
    total = None
    kind, panes, lit = (np.zeros((h, w), np.uint8) for _ in range(3))
    for y in range(h):
        for x in range(w):
            e = pixel_params(p, cells[y, x], fracts[y, x])
            out, st = o.render(e, 1, 1, threads=1)
            img[y, x] = out[0, 0]
            d = st.as_dict()
            total = d if total is None else {k: total[k] + d[k] for k in d}
            if census:
                kind[y, x] = 0 if st.sky_px else (2 if st.glass_px else 1)
                panes[y, x] = o.glass_layers(e, 1, 1, threads=1)[0, 0]
                lit[y, x] = o.terms(e, 1, 1, threads=1)[0][0, 0, 0]
    return (img, total, kind, panes, lit) if census else (img, total)


@pytest.fixture(scope="module")
def orcs(built, noise):
    """{field: the oracle the GPU tests compare with}, each holding the exit table of SUN."""
    import oracle
    out = {}
    for key, f in (("main", test_poses.field()), ("odd", odd_field())):
        out[key] = oracle.Oracle(f, noise, exit=True)
        out[key].hold_exit_table(frame_of("plan", SMALL).params)
    yield out
    _state.clear()
    test_poses._state.clear()


def lib_ray(fr, px, py, w=None, h=None):
    import voxmap_amd as vx
    from voxmap_amd import _abi
    r = _abi.Ray()
    rc = vx.lib().vx_pixel_ray_ortho(C.byref(fr.params), fr.width if w is None else w, fr.height if h is None else h,
                                     px, py, C.byref(r))
    return rc, r


@pytest.mark.parametrize("name,wh", CASES)
def test_pixel_ray_is_the_formula(name, wh, built):
    """Every pixel of every view, bit for bit, through the C function and through the Python wrapper."""
    import voxmap_amd as vx
    fr = frame_of(name, wh)
    cells, fracts = origins(fr.params, *wh)
    assert (fracts >= 0).all() and (fracts < 1).all()
    for y in range(wh[1]):
        for x in range(wh[0]):
            rc, r = lib_ray(fr, x, y)
            assert rc == 0
            assert tuple(r.cell) == tuple(cells[y, x]), (x, y)
            assert np.array_equal(np.array(r.fract[:], np.float32).view(np.uint32), fracts[y, x].view(np.uint32)), (x, y)
            assert tuple(r.dir) == tuple(fr.params.ray_fwd) and r.t_max == math.inf and tuple(r.reserved) == (0, 0)
    rec = vx.pixel_ray_ortho(fr, wh[0] - 1, 0)
    assert tuple(rec["cell"]) == tuple(cells[0, -1]) and tuple(rec["dir"]) == tuple(fr.params.ray_fwd)


def test_pixel_ray_clamps_a_fraction_that_rounds_to_one(built):
    """cam_fract 0 and right_x = 2^-30: left of the centre s is a tiny negative number, floor(s) = -1 and
    s + 1 rounds to 1.0f; the result is the cell below with the largest fraction under 1."""
    fr = frame_from_basis((7, 5, 3), (0, 0, 0), DOWN, (2.0 ** -30, 0, 0), (0, 1, 0), 8, 8)
    rc, r = lib_ray(fr, 1, 4)                     # nx = 3/8 - 1 < 0; ny = 1 - 9/8 < 0
    assert rc == 0
    assert r.cell[0] == 6 and np.float32(r.fract[0]).view(np.uint32) == np.float32(F1).view(np.uint32) == 0x3F7FFFFF
    assert r.cell[1] == 4 and r.fract[1] == 0.875 and r.cell[2] == 3 and r.fract[2] == 0.0
    rc, r = lib_ray(fr, 6, 4)                     # nx > 0: the camera's own cell
    assert rc == 0 and r.cell[0] == 7 and 0 < r.fract[0] < 2.0 ** -30
    cells, fracts = origins(fr.params, 8, 8)
    assert cells[4, 1, 0] == 6 and fracts[4, 1, 0] == np.float32(F1)


def test_pixel_ray_takes_a_negative_zero_fraction(built):
    v = VIEWS["plan"]
    fr = frame_from_basis(v["cell"], (-0.0, .5, 0), v["fwd"], v["right"], v["up"], *SMALL)
    cells, fracts = origins(fr.params, *SMALL)
    for x, y in ((0, 0), (28, 11), (56, 22)):
        rc, r = lib_ray(fr, x, y)
        assert rc == 0 and tuple(r.cell) == tuple(cells[y, x])
        assert np.array_equal(np.array(r.fract[:], np.float32).view(np.uint32), fracts[y, x].view(np.uint32))
    still = frame_from_basis(v["cell"], (-0.0, -0.0, -0.0), v["fwd"], (0, 0, 0), (0, 0, 0), 3, 3)
    rc, r = lib_ray(still, 1, 1)                  # nx = ny = 0: s = -0 + (0 + 0) = +0, its own cell
    assert rc == 0 and tuple(r.cell) == v["cell"] and tuple(r.fract) == (0.0, 0.0, 0.0)


def test_pixel_ray_rejects_what_is_out_of_range(built):
    from voxmap_amd import _abi
    import voxmap_amd as vx
    fr = frame_of("plan", SMALL)
    w, h = SMALL
    for px, py, ww, hh in ((-1, 0, w, h), (0, -1, w, h), (w, 0, w, h), (0, h, w, h), (0, 0, 0, h), (0, 0, w, 0),
                           (0, 0, 32769, h), (0, 0, w, 32769)):
        rc, _ = lib_ray(fr, px, py, ww, hh)
        assert rc == _abi.VX_EINVAL, (px, py, ww, hh)
        assert "vx_pixel_ray_ortho" in vx.lib().vx_last_error().decode()
    assert vx.lib().vx_pixel_ray_ortho(None, w, h, 0, 0, C.byref(_abi.Ray())) == _abi.VX_EINVAL
    assert vx.lib().vx_pixel_ray_ortho(C.byref(fr.params), w, h, 0, 0, None) == _abi.VX_EINVAL
    assert lib_ray(fr, w - 1, h - 1)[0] == 0 and lib_ray(fr, 0, 0, 32768, 32768)[0] == 0


def _ortho(target, az, el, hw, back, w, h):
    import voxmap_amd as vx
    from voxmap_amd import _abi
    p = _abi.FrameParams()
    rc = vx.lib().vx_frame_from_ortho((C.c_double * 3)(*target), az, el, hw, back, w, h, C.byref(p))
    return rc, p


def _close(v, want, scale=1.0):
    return np.allclose(np.array(v[:], np.float64), np.array(want, np.float64), rtol=0, atol=1e-6 * scale)


def test_frame_from_ortho_axes(built):
    """North-up plan (el = pi/2, az = -pi/2) and the south elevation (el = 0, az = -pi/2) give the stated axes."""
    rc, p = _ortho((48.5, 24.5, 0.0), -math.pi / 2, math.pi / 2, 48.0, 20.0, 64, 32)
    assert rc == 0 and p.quality == 1
    assert _close(p.ray_fwd, (0, 0, -1)) and _close(p.ray_right, (48, 0, 0), 48) and _close(p.ray_up, (0, 24, 0), 48)
    assert tuple(p.cam_cell) == (48, 24, 20) and _close(p.cam_fract, (.5, .5, 0))
    rc, p = _ortho((48.5, 24.5, 8.0), -math.pi / 2, 0.0, 48.0, 30.0, 96, 16)
    assert rc == 0
    assert _close(p.ray_fwd, (0, 1, 0)) and _close(p.ray_right, (48, 0, 0), 48) and _close(p.ray_up, (0, 0, 8), 48)
    assert tuple(p.cam_cell) == (48, -6, 8) and _close(p.cam_fract, (.5, .5, 0))


@pytest.mark.parametrize("az,el", [(0.3, 0.7), (-2.1, 0.2), (2.9, 1.3), (1.0, -0.4)])
@pytest.mark.parametrize("w,h", [(64, 40), (57, 23), (1, 7)])
def test_frame_from_ortho_is_an_orthogonal_basis(az, el, w, h, built):
    target, hw, back = (40.25, -3.5, 7.75), 33.0, 61.5
    rc, p = _ortho(target, az, el, hw, back, w, h)
    assert rc == 0
    f, r, u = (np.array(v[:], np.float64) for v in (p.ray_fwd, p.ray_right, p.ray_up))
    nf, nr, nu = (np.linalg.norm(v) for v in (f, r, u))
    assert abs(nf - 1) <= 1e-6 and abs(nr - hw) <= 1e-6 * hw
    assert abs(nu / nr - h / w) <= 1e-6 * h / w                       # square pixels
    for a, b, s in ((f, r, nr), (f, u, nu), (r, u, nr * nu)):
        assert abs(a @ b) <= 1e-6 * s
    assert np.allclose(np.cross(r, f) / nr, u / nu, atol=1e-6)        # u = r x f: a right-handed image plane
    e = np.array((math.cos(el) * math.cos(az), math.cos(el) * math.sin(az), math.sin(el)))
    assert np.allclose(f, -e, atol=1e-6)
    cam = np.array(p.cam_cell[:], np.float64) + np.array(p.cam_fract[:], np.float64)
    assert np.allclose(cam, np.array(target) + back * e, rtol=0, atol=1e-5)
    assert all(0 <= c < 1 for c in p.cam_fract)


def test_frame_from_ortho_leaves_the_other_fields_and_rejects_bad_input(built):
    import voxmap_amd as vx
    from voxmap_amd import _abi
    p = _abi.FrameParams()
    p.quality, p.flags, p.time, p.shadow_samples = 0, 0x30, 7.5, 3
    p.sun_dir[2] = 0.25
    t = (C.c_double * 3)(1.0, 2.0, 3.0)
    assert vx.lib().vx_frame_from_ortho(t, 0.1, 0.2, 5.0, 9.0, 8, 8, C.byref(p)) == 0
    assert (p.quality, p.flags, p.time, p.shadow_samples, p.sun_dir[2]) == (1, 0x30, 7.5, 3, 0.25)
    nan, inf = float("nan"), float("inf")
    bad = [((1, 2, 3), .1, .2, 0.0, 9, 8, 8), ((1, 2, 3), .1, .2, -1.0, 9, 8, 8), ((1, 2, 3), .1, .2, nan, 9, 8, 8),
           ((nan, 2, 3), .1, .2, 5, 9, 8, 8), ((1, 2, inf), .1, .2, 5, 9, 8, 8), ((1, 2, 3), inf, .2, 5, 9, 8, 8),
           ((1, 2, 3), .1, nan, 5, 9, 8, 8), ((1, 2, 3), .1, .2, 5, inf, 8, 8), ((1, 2, 3), .1, .2, 5, 9, 0, 8),
           ((1, 2, 3), .1, .2, 5, 9, 8, 0), ((1, 2, 3), .1, .2, 5, 9, -4, 8)]
    for a in bad:
        rc, _ = _ortho(*a)
        assert rc == _abi.VX_EINVAL, a
        assert "vx_frame_from_ortho" in vx.lib().vx_last_error().decode()
    assert vx.lib().vx_frame_from_ortho(None, 0.1, 0.2, 5.0, 9.0, 8, 8, C.byref(p)) == _abi.VX_EINVAL
    assert vx.lib().vx_frame_from_ortho(t, 0.1, 0.2, 5.0, 9.0, 8, 8, None) == _abi.VX_EINVAL
    fr = vx.frame_from_ortho((48.5, 24.5, 0), -math.pi / 2, math.pi / 2, 48, 20, 64, 32, sun=SUN, flags=0x30)
    assert (fr.width, fr.height, fr.params.flags, fr.params.quality) == (64, 32, 0x30, 1)
    assert tuple(fr.params.sun_dir) == tuple(np.float32(SUN).tolist())


# ---- the census: what each view shows, from the oracle alone ------------------------------------

def _census(orcs, name, wh):
    key = (name, wh)
    if key not in _state:
        img, st, kind, panes, lit = assemble(orcs[VIEWS[name]["field"]], frame_of(name, wh), census=True)
        n = wh[0] * wh[1]
        assert st["pixels"] == n and st["sky_px"] + st["block_px"] + st["glass_px"] == n
        assert (np.bincount(kind.ravel(), minlength=3) == (st["sky_px"], st["block_px"], st["glass_px"])).all()
        _state[key] = dict(img=img, st=st, n=n, sky=st["sky_px"], block=st["block_px"], glass=st["glass_px"],
                           stacked=int(np.count_nonzero((kind == 2) & (panes >= 2))),
                           lit=int(np.count_nonzero(lit == 1)), unlit=int(np.count_nonzero(lit == 0)))
    return _state[key]


@pytest.mark.parametrize("name,wh", CASES)
def test_census(name, wh, orcs):
    c = _census(orcs, name, wh)
    n = c["n"]
    assert not np.isnan(c["img"]).any() and c["st"]["primary_cap_hits"] == 0
    assert (c["img"][..., 3] == 1).all()
    if name == "plan":
        assert c["sky"] == 0 and c["glass"] >= 30 and 5 * c["unlit"] >= n and 2 * c["lit"] >= n
    if name == "iso":
        assert wh != BIG or c["glass"] >= 100
        assert min(c["sky"], c["lit"], c["unlit"]) * 20 >= n
    if name == "elev_y":
        assert c["stacked"] >= 20
    if name == "section" and wh == SMALL:
        assert c["glass"] >= 400
    if name == "edge":
        assert 10 * c["sky"] >= 3 * n
    if name in ("far_elev_y", "iso_odd"):
        assert c["stacked"] >= 1 and c["glass"] >= 30
    if name in ("far_plan", "plan_odd"):
        assert c["glass"] >= 10 and c["block"] >= n // 2


def test_oracle_modes_agree(orcs, noise):
    """One view in the oracle's other modes: the literal march (exit=False) gives the same frame and the same
    counters but the shadow fetches; the unit split (quad=False) is what VX_FLAG_UNIT_GBUF asks of the default."""
    import oracle
    ex = orcs["main"]
    lit = oracle.Oracle(test_poses.field(), noise, oct_e=ex.oct_e, exit=False, quad=ex.qoff)
    unit = oracle.Oracle(test_poses.field(), noise, oct_e=ex.oct_e, exit=True, quad=False)
    unit.hold_exit_table(frame_of("iso", SMALL).params)
    for flags in (0, 0x30):
        fr = frame_of("iso", SMALL, flags=flags)
        a, sa = assemble(ex, fr)
        b, sb = assemble(lit, fr)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        assert sa["shadow_fetches"] <= sb["shadow_fetches"]
        for k in sa:
            assert k == "shadow_fetches" or sa[k] == sb[k], k
    a, sa = assemble(ex, frame_of("iso", SMALL, flags=0x800))
    b, sb = assemble(unit, frame_of("iso", SMALL))
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and sa == sb
