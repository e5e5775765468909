"""Degenerate and boundary sun directions on the CPU: the sun table and the oracle to itself.

Every other frame test uses one of a dozen generic suns.  The sun march is the part of the build with the
most host-decided thresholds, and each exists twice, written independently: in the oracle (vxo_exit_plan,
vxo_doom_plan, vxo_sun_samples) and in the product (vx_frame.cpp: sun_ray, exit_plan, doom_plan,
frame_consts).  The suns here sit on those thresholds:

  |r_i| >= 2^-10 (the fast path): components on the limit, one ulp under it and at -2^-10; soft shadows
  whose samples fall on both sides, and in several octants (no shared table: the pooled and brick passes
  fall back, each sample reads sunx of its own octant);
  slopes |r_x / r_z| <= 4 (a cone table): exactly 4 gives kx = ceil(4 + 1/64) = 5 and the doom window's
  xhi = ceil(8 (4 + 1/64)) = 33, the widest the kernels are sized for; one ulp over gives the orthant tables;
  ceil(a + 1/64) and floor/ceil(8 (a -+ 1/64)) on integers (slopes 63/64 and k/8 +- 1/64), xlo = -1;
  hmax and the int8 code range (max_shadow_steps 1, 2, 3, 5: no doom table; 1000: crossings up to 120);
  zero components on every axis and sign, -0.0, a sun below the horizon, the zero vector;
  suns with no tangent frame ((0, 0, z), |z| < 0.9: a x sun = 0, every soft sample NaN);
  suns that are not unit length (render.frag uses u_sunDir as given).

This file holds the table, the builders and the conditions that keep tests/test_suns_gpu.py (which imports
them) from being vacuous: each case is what the table says it is (from oracle.sun_samples' float32 output,
the rule restated here), the oracle's modes agree with each other at every case, and every marching case
has lit and unlit fragments (the straddle cases partly lit ones too).

Poses.  The main pose sees 3,742 block and 107 glass pixels and marches 2,740 shadow rays at (0.5, 0.3,
0.8).  Three cases miss a floor there and are rendered from POSE_B instead (the floor stays, the pose
moves): (0.6, 0.8, 0) has 7 unlit fragments from the main pose (295 from POSE_B), the horizon straddle no
fully lit one (its down-going samples reach the ground; POSE_B sees faces near the grid's +x edge: 78),
the slope-4 straddle 8 partly lit ones (256).  The main pose looks along +x and sees no face whose normal is
+x, the only ones a sun of (1, 0, 0) shades without rough normals: that case is rendered from POSE_C, the
main pose mirrored in x, so that it marches at v1 flags too (537 rays, 57 unlit, 480 lit).

The widest doom window.  ((0.7, 0.6, 0.4), 0.2, 16), the first candidate, has (xhi - xlo) + (yhi - ylo) = 39.  A
search over 20,000 random unit suns of the all-positive octant rounded to two decimals, radii 0.1 to 0.5 and
16 samples, keeping the cone plans, found ((0.54, 0.6, 0.59), 0.5, 16): plan (1, 1, 2, 32, 2, 32, 4), cone
(4, 4), width 60 (case "wide"; the first candidate is kept as "wide_39")."""
import numpy as np
import pytest

from test_poses import frame_from_basis

DIMS, SEED, N_BOXES, N_GLASS = (96, 64, 40), 31, 30, 5           # tests/test_doom_gpu.py's field
WH = (96, 64)
POSE = dict(cell=(10, 6, 37), fract=(.5, .5, .5), fwd=(.5, .55, -.5), right=(.8, -.7, 0), up=(.25, .3, .6))
POSE_B = dict(cell=(48, 32, 37), fract=(.5, .5, .5), fwd=(.78, 0, -.62), right=(0, -.45, 0), up=(.19, 0, .23))
POSE_C = dict(cell=(85, 6, 37), fract=(.5, .5, .5), fwd=(-.5, .55, -.5), right=(.8, .7, 0), up=(-.25, .3, .6))
SMALL_DIMS = {"z3": (37, 29, 3), "z2": (37, 29, 2)}              # SB = Z + 2 = 5 = kx at slope 4; SB < 5: no cone
SMALL_WH = (64, 40)
SMALL_POSE = dict(cell=(18, 14, 12), fract=(.5, .5, .5), fwd=(.1, .1, -1), right=(.9, 0, 0), up=(0, .6, 0))
SMALL_SUNS = [(1, 1, .25), (.5, .3, .8)]

LIM = 2.0 ** -10
FULL, NO_DOOM = 0x30, 0x20000
GENERIC, SLOPE4 = (.5, .3, .8), (1, 1, .25)
BUDGETS = (1, 2, 3, 5, 1000)


def nb(x):
    """The float32 next below x toward 0."""
    return float(np.nextafter(np.float32(x), np.float32(0)))


def _case(sun, fast, octs, cone=None, doom=None, radius=0.0, n=0, pose=POSE, **tags):
    """fast: one character per sample, '1' = every |r_i| >= 2^-10; octs: the set of the samples' octants
    (bit i: r_i > 0; -1 for a sample that is not fast); cone: (kx, ky) or None; doom: vxo_doom_plan at the
    default budget 2 Z = 80 for the cone cases."""
    return dict(sun=tuple(float(np.float32(v)) for v in sun), radius=radius, n=n, fast=fast, octs=set(octs), cone=cone,
                doom=doom, pose=pose, **tags)


# Hard shadows.  Tags: marches=False (shadeFactor is 0 on every face: shadow_rays == 0).
HARD = {
    # the axes
    "zenith": _case((0, 0, 1), "0", {-1}),
    "nadir": _case((0, 0, -1), "0", {-1}, marches=False),
    "plus_x": _case((1, 0, 0), "0", {-1}, pose=POSE_C),
    "minus_y": _case((0, -1, 0), "0", {-1}),
    # one zero component
    "x_zero": _case((0, .6, .8), "0", {-1}),
    "y_negzero": _case((.6, -0.0, .8), "0", {-1}),
    "z_zero": _case((.6, .8, 0), "0", {-1}, pose=POSE_B),
    # the fast-path limit
    "y_lim": _case((.6, LIM, .8), "1", {7}, (1, 1), (1, 1, 5, 7, -1, 1, 19)),
    "y_under": _case((.6, nb(LIM), .8), "0", {-1}),
    "y_neglim": _case((.6, -LIM, .8), "1", {5}, (1, 1), (1, -1, 5, 7, -1, 1, 19)),
    "z_lim": _case((.6, .8, LIM), "1", {7}),
    "z_under": _case((.6, .8, nb(LIM)), "0", {-1}),
    "xy_lim": _case((LIM, LIM, 1), "1", {7}, (1, 1), (1, 1, -1, 1, -1, 1, 31)),
    # a slope of exactly 4, and one ulp over
    "s4_x": _case((1, .25, .25), "1", {7}, (5, 2), (1, 1, 31, 33, 7, 9, 6)),
    "s4_xy": _case((1, 1, .25), "1", {7}, (5, 5), (1, 1, 31, 33, 31, 33, 4)),
    "s4_neg": _case((-1, -1, .25), "1", {4}, (5, 5), (-1, -1, 31, 33, 31, 33, 4)),
    "s4_y": _case((-.25, -1, .25), "1", {4}, (2, 5), (-1, -1, 7, 9, 31, 33, 6)),
    "s4_over": _case((1, .25, nb(.25)), "1", {7}),
    # window bounds on integers
    "half": _case((.5, .5, .5), "1", {7}, (2, 2), (1, 1, 7, 9, 7, 9, 11)),
    "k63": _case((63 / 64, -63 / 64, 1), "1", {5}, (1, 1), (1, -1, 7, 8, 7, 8, 12)),
    "k8_in": _case((3 / 8 + 1 / 64, 5 / 8 - 1 / 64, 1), "1", {7}, (1, 1), (1, 1, 3, 4, 4, 5, 17)),
    "k8_out": _case((3 / 8 - 1 / 64, 5 / 8 + 1 / 64, 1), "1", {7}, (1, 1), (1, 1, 2, 3, 5, 6, 18)),
    # not unit length
    "long": _case((2, 1.2, 3.2), "1", {7}, (1, 1), (1, 1, 4, 6, 2, 4, 17)),
    "short": _case(tuple(2.0 ** -6 * v for v in GENERIC), "1", {7}, (1, 1), (1, 1, 4, 6, 2, 4, 17)),
    # below the horizon, and no sun
    "below": _case((.5, .3, -.8), "1", {3}, marches=False),
    "zero": _case((0, 0, 0), "0", {-1}, marches=False),
}

# Soft shadows.  Tags: partly (held to the partly-lit floor), nan (every sample NaN), marches.
SOFT = {
    "x_straddle": _case((2.0 ** -9, .6, .8), "11011111", {-1, 6, 7}, radius=.05, n=8, partly=True),
    "xy_straddle": _case((2.0 ** -9, -2.0 ** -9, 1), "1" * 16, {4, 5, 6, 7}, radius=.05, n=16, partly=True),
    "lim_straddle": _case((1.5 * LIM, .6, .8), "01101011", {-1, 7}, radius=.002, n=8, partly=True),
    "horizon_straddle": _case((.9, .3, .05), "1" * 6, {3, 7}, radius=.3, n=6, partly=True, pose=POSE_B),
    "s4_straddle": _case((1, .25, .25), "1" * 8, {7}, radius=.02, n=8, partly=True, pose=POSE_B),
    "s4_inside": _case((1, .25, .27), "1" * 8, {7}, (4, 1), (1, 1, 28, 31, 6, 8, 6), radius=.01, n=8),
    "soft_zenith": _case((0, 0, 1), "0" + "1" * 15, {-1, 4, 5, 6, 7}, radius=.05, n=16, partly=True),
    "no_tangent": _case((0, 0, .5), "0000", {-1}, radius=.05, n=4, nan=True),
    "soft_zero": _case((0, 0, 0), "0000", {-1}, radius=.05, n=4, nan=True, marches=False),
    "radius_0": _case(GENERIC, "1111", {7}, (1, 1), (1, 1, 4, 6, 2, 4, 17), radius=0.0, n=4),
    "radius_half": _case(GENERIC, "1" * 16, {5, 7}, radius=.5, n=16, partly=True),
    "wide": _case((.54, .6, .59), "1" * 16, {7}, (4, 4), (1, 1, 2, 32, 2, 32, 4), radius=.5, n=16),
    "wide_39": _case((.7, .6, .4), "1" * 16, {7}, (4, 3), (1, 1, 8, 29, 6, 24, 4), radius=.2, n=16),
}
CASES = dict(HARD, **SOFT)
STRADDLES = ("x_straddle", "xy_straddle", "lim_straddle", "horizon_straddle", "s4_straddle")
# (on the limit, one ulp under it): the frames are the same, only the path differs
LIMIT_PAIRS = [("y_lim", "y_under"), ("z_lim", "z_under")]
# consecutive frames need different cone windows (the scene keeps two copies, so slots recycle)
ORDER = ["s4_x", "zenith", "half", "x_straddle", "s4_xy", "nadir", "wide", "y_lim", "s4_y", "plus_x", "k63",
         "xy_straddle", "s4_neg", "minus_y", "wide_39", "y_under", "s4_inside", "x_zero", "xy_lim", "lim_straddle",
         "long", "y_negzero", "s4_over", "horizon_straddle", "k8_in", "z_zero", "y_neglim", "s4_straddle", "k8_out",
         "z_lim", "radius_0", "soft_zenith", "short", "z_under", "radius_half", "no_tangent", "below", "soft_zero",
         "zero"]
assert sorted(ORDER) == sorted(CASES)

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


def small_field(key):
    import oracle
    from voxmap_amd import scenes
    if key not in _state:
        _state[key] = oracle.field_build(scenes.odd_proc(1, SMALL_DIMS[key]))
    return _state[key]


def frame_of(name, **kw):
    c = CASES[name]
    kw.setdefault("flags", FULL)
    return frame_from_basis(**c["pose"], w=WH[0], h=WH[1], sun=c["sun"], shadow_samples=c["n"], sun_radius=c["radius"],
                            **kw)


def budget_frame(sun, budget, **kw):
    kw.setdefault("flags", FULL)
    return frame_from_basis(**POSE, w=WH[0], h=WH[1], sun=sun, max_shadow_steps=budget, **kw)


def small_frame(sun, n=0, radius=0.0, **kw):
    kw.setdefault("flags", FULL)
    return frame_from_basis(**SMALL_POSE, w=SMALL_WH[0], h=SMALL_WH[1], sun=sun, shadow_samples=n, sun_radius=radius,
                            **kw)


def samples(params):
    """oracle.sun_samples of a frame's float32 sun."""
    import oracle
    return oracle.sun_samples(params.sun_dir[:], params.sun_radius, params.shadow_samples)


def classify(d):
    """The rule restated from the float32 samples: (fast per sample, octant per sample or -1, NaN per sample)."""
    a = np.abs(d)
    fast = (a[:, 0] >= np.float32(LIM)) & (a[:, 1] >= np.float32(LIM)) & (a[:, 2] >= np.float32(LIM))
    octs = np.where(fast, (d[:, 0] > 0) * 1 + (d[:, 1] > 0) * 2 + (d[:, 2] > 0) * 4, -1)
    return fast, octs, np.isnan(d).any(axis=1)


def doom_cross(h, xhi, yhi):
    """Boundary crossings from a doomed cell with h into its block (DESIGN.md §3 "Doom table")."""
    return h + (h * xhi) // 8 + 1 + (h * yhi) // 8 + 1


def expected_exit(params, Z=DIMS[2]):
    """What vx_prepare_sun reports for a frame: (kind, octant, kx, ky), from the oracle's plan: the cone
    (Z >= 3), else the orthant copy of sample 0's octant when sample 0 is fast, else nothing."""
    import oracle
    d = samples(params)
    cone, octs, kx, ky = oracle.exit_plan(d, allow_cone=Z >= 3)
    if cone:
        return 2, octs[0], kx, ky
    return (1, octs[0], -1, -1) if octs[0] >= 0 else (0, -1, -1, -1)


def same_words(a, b):
    """NaN at the same positions, every other word equal."""
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and np.array_equal(a.view(np.uint32)[~nan], b.view(np.uint32)[~nan])


def lit_census(o, fr):
    """(fully unlit, fully lit, partly lit) fragments of a frame, from Oracle.terms (both slots)."""
    lit, _ = o.terms(fr.params, fr.width, fr.height)
    v = lit[lit != 255].astype(int)
    m = max(fr.params.shadow_samples, 1)
    return int((v == 0).sum()), int((v == m).sum()), int(((v > 0) & (v < m)).sum())


def make_oracles(f, noise):
    import oracle
    ex = oracle.Oracle(f, noise, exit=True)
    orth = oracle.Oracle(f, noise, oct_e=ex.oct_e, exit="orthant", quad=ex.qoff)
    lit = oracle.Oracle(f, noise, oct_e=ex.oct_e, exit=False, quad=ex.qoff)
    return ex, orth, lit


@pytest.fixture(scope="module")
def orc(built, noise):
    """The oracle with the cone and doom tables, with the orthant tables only, and marching literally."""
    yield make_oracles(field(), noise)
    _state.clear()


def test_the_pose_sees_blocks_and_glass(orc):
    _, st = orc[0].render(frame_from_basis(**POSE, w=WH[0], h=WH[1], sun=GENERIC, flags=FULL).params, *WH)
    assert (st.block_px, st.glass_px, st.shadow_rays) == (3742, 107, 2740)
    assert grid().shape == DIMS[::-1]


@pytest.mark.parametrize("name", list(CASES))
def test_each_case_is_what_the_table_says(name, orc):
    import oracle
    c = CASES[name]
    fr = frame_of(name)
    assert tuple(fr.params.sun_dir[:]) == c["sun"]                 # every component an exact float32
    d = samples(fr.params)
    assert d.dtype == np.float32 and d.shape == (max(c["n"], 1), 3)
    fast, octs, nan = classify(d)
    assert "".join("1" if f else "0" for f in fast) == c["fast"]
    assert set(octs.tolist()) == c["octs"]
    assert nan.all() if c.get("nan") else not nan.any()
    cone, o_octs, kx, ky = oracle.exit_plan(d)
    assert o_octs == octs.tolist()
    assert (cone, (kx, ky)) == ((True, c["cone"]) if c["cone"] else (False, (-1, -1)))
    assert (c["doom"] is None) == (c["cone"] is None)
    if c["cone"]:
        assert oracle.doom_plan(d, 2 * DIMS[2]) == c["doom"]
        assert len(c["octs"]) == 1 and min(c["octs"]) & 4 and all(fast)
        assert (c["doom"][0], c["doom"][1]) == (1 if octs[0] & 1 else -1, 1 if octs[0] & 2 else -1)
    assert expected_exit(fr.params)[0] == (2 if c["cone"] else (1 if fast[0] else 0))


def test_the_named_thresholds():
    """What the table is for, by name."""
    for name, k in (("s4_x", (5, 2)), ("s4_xy", (5, 5)), ("s4_neg", (5, 5)), ("s4_y", (2, 5))):
        c = HARD[name]
        assert c["cone"] == k and max(c["doom"][3], c["doom"][5]) == 33        # kDoomXhi
        assert max(abs(c["sun"][0]), abs(c["sun"][1])) / c["sun"][2] == 4.0
    assert HARD["s4_over"]["cone"] is None and HARD["s4_over"]["sun"][2] == nb(.25) < .25
    assert SOFT["s4_straddle"]["cone"] is None and SOFT["s4_inside"]["cone"] == (4, 1)
    assert HARD["k63"]["cone"] == (1, 1) and 63 / 64 + 1 / 64 == 1.0
    assert HARD["xy_lim"]["doom"][2] == HARD["xy_lim"]["doom"][4] == -1
    for on, under in LIMIT_PAIRS:
        assert HARD[on]["fast"] == "1" and HARD[under]["fast"] == "0"
        diff = [i for i in range(3) if HARD[on]["sun"][i] != HARD[under]["sun"][i]]
        assert len(diff) == 1 and HARD[on]["sun"][diff[0]] == LIM and HARD[under]["sun"][diff[0]] == nb(LIM)
    assert HARD["y_neglim"]["sun"][1] == -LIM and np.signbit(HARD["y_negzero"]["sun"][1])
    for name in STRADDLES[:4]:
        c = SOFT[name]
        assert len(c["octs"] - {-1}) >= 2 or len(set(c["fast"])) == 2
    assert len(SOFT["x_straddle"]["octs"] - {-1}) == 2 and len(set(SOFT["x_straddle"]["fast"])) == 2     # both at once
    # the slope-4 straddle: one octant, all fast, some sample's slope over 4 (no cone) and some under
    import oracle
    d = oracle.sun_samples(SOFT["s4_straddle"]["sun"], SOFT["s4_straddle"]["radius"], SOFT["s4_straddle"]["n"])
    slope = np.abs(d[:, 0].astype(float) / d[:, 2].astype(float))
    assert (slope > 4).any() and (slope < 4).any()
    for name in ("no_tangent", "soft_zero"):
        assert SOFT[name]["nan"] and abs(SOFT[name]["sun"][2]) < .9 and SOFT[name]["sun"][:2] == (0, 0)


@pytest.mark.parametrize("on,under", LIMIT_PAIRS)
def test_limit_pairs_differ_in_the_path_only(on, under, orc):
    """One ulp apart across 2^-10: the same marches with the same lit flag on every fragment and the same
    counters but for the fetches (a table on one side, the literal march on the other).  The frame words
    themselves are not all equal, since the sun enters the shading too (shadeFactor = sqrt(dot(n, sun)) on the
    faces that look along the changed axis, scatter = 1 - sqrt(sun.z)): a one-ulp change of a 2^-10 component,
    under 10^-6 in any colour."""
    ex = orc[0]
    a, sa = ex.render(frame_of(on).params, *WH)
    b, sb = ex.render(frame_of(under).params, *WH)
    assert not np.isnan(a).any() and float(np.abs(a - b).max()) < 1e-6
    for k, v in sa.as_dict().items():
        assert k == "shadow_fetches" or v == getattr(sb, k), k
    assert sa.shadow_rays > 0 and sa.shadow_fetches < sb.shadow_fetches
    la, lb = (ex.terms(frame_of(n).params, *WH)[0] for n in (on, under))
    assert np.array_equal(la, lb) and (la == 0).sum() >= 20 and (la == 1).sum() >= 20


def test_step_budget_plans():
    """max_shadow_steps 1, 2, 3, 5: hmax = 0, no doom table; 1000: the generic sun's plan reaches the last
    code (doom_cross = 120, -128 in the int8 copy); the slope-4 sun's stops under it, one h short of passing."""
    import oracle
    for sun in (GENERIC, SLOPE4):
        d = np.array([sun], np.float32)
        for b in BUDGETS[:4]:
            assert oracle.doom_plan(d, b)[6] == 0
        p = oracle.doom_plan(d, 1000)
        assert oracle.lib().vxo_doom_cross(p[6], p[3], p[5]) == doom_cross(p[6], p[3], p[5]) <= 120
        assert doom_cross(p[6] + 1, p[3], p[5]) > 120
        if sun == GENERIC:
            assert p == (1, 1, 4, 6, 2, 4, 53) and doom_cross(p[6], p[3], p[5]) == 120
        else:
            assert p == (1, 1, 31, 33, 31, 33, 12)


def _modes_agree(oracles, fr):
    """exit=True, the same with VX_FLAG_NO_DOOM, exit="orthant" and exit=False: the same words, what does
    not depend on the tables equal, and shadow_fetches never growing as tables are added."""
    ex, orth, lit = oracles
    w, h = fr.width, fr.height
    nd = fr.params.copy()
    nd.flags |= NO_DOOM
    runs = [ex.render(fr.params, w, h), ex.render(nd, w, h), orth.render(fr.params, w, h), lit.render(fr.params, w, h)]
    for img, st in runs[1:]:
        assert same_words(runs[0][0], img)
        for k in ("pixels", "block_px", "glass_px", "shadow_rays", "primary_fetches", "sky_px", "reflect_rays",
                  "reflect_fetches", "ao_samples", "noise_px"):
            assert getattr(st, k) == getattr(runs[0][1], k), k
    f = [st.shadow_fetches for _, st in runs]
    assert f[0] <= f[1] <= f[2] <= f[3], f
    return runs[0][1], f


@pytest.mark.parametrize("flags", [FULL, 0, 0x2030], ids=["full", "v1", "reflect_all"])
@pytest.mark.parametrize("name", list(CASES))
def test_oracle_modes_agree(name, flags, orc):
    st, _ = _modes_agree(orc, frame_of(name, flags=flags))
    assert (st.shadow_rays > 0) == CASES[name].get("marches", True)


@pytest.mark.parametrize("sun", [GENERIC, SLOPE4], ids=["generic", "slope4"])
@pytest.mark.parametrize("budget", BUDGETS)
def test_oracle_modes_agree_at_step_budgets(budget, sun, orc):
    st, f = _modes_agree(orc, budget_frame(sun, budget))
    assert st.shadow_rays == 2740
    assert f[0] == f[1] if budget <= 5 else f[0] < f[1]            # no doom table at hmax = 0; one that saves at 1000


@pytest.mark.parametrize("name", list(CASES))
def test_lit_floors(name, orc):
    """Every case that marches has >= 20 fragments fully unlit and >= 20 fully lit; the straddle cases, the
    soft zenith and the radius-0.5 case >= 20 partly lit.  The nadir, the sun below the horizon and the zero
    suns march nothing (shadeFactor is 0 on every face): shadow_rays == 0, and their frames are held to the
    oracle all the same."""
    ex = orc[0]
    c = CASES[name]
    fr = frame_of(name)
    unlit, lit, partly = lit_census(ex, fr)
    _, st = ex.render(fr.params, *WH)
    if not c.get("marches", True):
        assert st.shadow_rays == 0 and (unlit, lit, partly) == (0, 0, 0)
        assert st.block_px + st.glass_px > 3000
        return
    assert st.shadow_rays >= 20 * max(c["n"], 1)
    assert unlit >= 20 and lit >= 20, (unlit, lit, partly)
    if c.get("partly"):
        assert partly >= 20, partly
    if c["n"] <= 1:
        assert partly == 0


def test_length_changes_the_shading_only(orc):
    """render.frag uses u_sunDir as given: a sun four times as long, or 2^-6 as long, picks the same tables as
    (0.5, 0.3, 0.8) and gives the same lit flags and fetch counts; the frames differ (the dot products scale)."""
    ex = orc[0]
    unit = frame_from_basis(**POSE, w=WH[0], h=WH[1], sun=GENERIC, flags=FULL)
    a, sa = ex.render(unit.params, *WH)
    for name in ("long", "short"):
        b, sb = ex.render(frame_of(name).params, *WH)
        assert (sb.shadow_rays, sb.shadow_fetches) == (sa.shadow_rays, sa.shadow_fetches)
        assert np.array_equal(ex.terms(frame_of(name).params, *WH)[0], ex.terms(unit.params, *WH)[0])
        assert not same_words(a, b)
        assert HARD[name]["doom"] == SOFT["radius_0"]["doom"]


def test_no_tangent_frame_is_finite_and_marches_in_place(orc):
    """(0, 0, 0.5): every sample direction is NaN.  march_literal's contract (0 * inf = NaN, floor(NaN) := 0)
    keeps such a march in its start cell: every fetch is that cell, the lit flag that of a march that runs
    out of steps there or reads a 0.  The frame has no NaN: the samples enter the lit count only."""
    ex = orc[0]
    fr = frame_of("no_tangent")
    img, st = ex.render(fr.params, *WH)
    assert not np.isnan(img).any() and st.shadow_rays > 0
    assert lit_census(ex, fr)[2] == 0                      # all four samples do the same


@pytest.mark.parametrize("key", list(SMALL_DIMS))
def test_small_fields(key, built, noise):
    """Z = 3: SB = 5 = kx at slope 4, the limit of the cone copy's window; Z = 2: no cone.  X and Y are no
    multiples of the doom build's 8-cell block.  Both have lit and unlit fragments, and the modes agree."""
    import oracle
    oracles = make_oracles(small_field(key), noise)
    Z = SMALL_DIMS[key][2]
    for sun in SMALL_SUNS:
        for n, radius in ((0, 0.0), (4, .02)):
            fr = small_frame(sun, n, radius)
            st, _ = _modes_agree(oracles, fr)
            unlit, lit, _ = lit_census(oracles[0], fr)
            assert st.shadow_rays > 0 and unlit >= 20 and lit >= 20
        want = (2, 7, 5, 5) if Z == 3 else (1, 7, -1, -1)
        assert expected_exit(small_frame(SLOPE4).params, Z) == want
    _state.pop(key, None)


@pytest.mark.parametrize("name", list(SOFT))
def test_host_sun_samples_equal_the_oracles(name, built):
    """vx.sun_samples (vx_sun_samples, the host function frame_consts calls) against oracle.sun_samples, bit
    for bit; NaN on every component where the sun has no tangent frame."""
    import oracle
    import voxmap_amd as vx
    c = SOFT[name]
    a = vx.sun_samples(c["sun"], c["radius"], c["n"])
    b = oracle.sun_samples(c["sun"], c["radius"], c["n"])
    assert a.shape == b.shape == (c["n"], 3) and a.dtype == b.dtype == np.float32
    if c.get("nan"):
        assert np.isnan(a).all() and np.isnan(b).all()
    else:
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
