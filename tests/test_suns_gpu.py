"""Degenerate and boundary sun directions on the GPU against the oracle.

The suns of tests/test_suns.py (whose table, builders and fields this file imports; that file holds the
oracle to itself on them and shows that each case is on the threshold it names and that its frames have lit
and unlit fragments): components on, under and at minus the fast-path limit 2^-10; soft shadows whose samples
fall on both sides of it and in several octants; slopes of exactly 4 (kx = 5, the doom window's xhi = 33, the
last column the kernels are sized for) and one ulp over; window bounds on integers; step budgets with no doom
table and with the last int8 code; zero components on every axis and sign; suns with no tangent frame (every
soft sample NaN); suns that are not unit length, below the horizon, zero.  Every frame is compared with the
oracle on every fp32 word and every counter the oracle keeps (gpu_rig.Rig.check), then rendered again
with VX_FLAG_INT_INDEX.  The cases run in test_suns.ORDER, in which consecutive frames need different cone
windows: the scene keeps two copies, so slots recycle all the time."""
import numpy as np
import pytest

import test_suns
from gpu_rig import Rig, assert_words_equal_nan_positions, gpu_available, with_flags
from test_poses import frame_from_basis
from test_suns import (BUDGETS, CASES, FULL, GENERIC, NO_DOOM, ORDER, POSE, SLOPE4, SMALL_DIMS, SMALL_SUNS, SOFT,
                       budget_frame, expected_exit, frame_of, small_frame)

pytestmark = pytest.mark.gpu

SOFT_POOL, SOFT_BRICK, NO_EXIT, NO_CONE, REFLECT_ALL = 0x80, 0x100, 0x200, 0x400, 0x2000
MODES = {"v1": 0, "full": FULL, "reflect_all": REFLECT_ALL | FULL}


class SunRig(Rig):
    """Rig over any field: the scene, the field it reads back, the oracle with every table over that copy
    (Rig.check compares with it), and the orthant-only and literal oracles over the same boxes."""

    def make_oracle(self, noise):
        full, self.orthant, self.literal = test_suns.make_oracles(self.dev_field, noise)
        return full


@pytest.fixture(scope="module")
def rig(built, noise):
    if not gpu_available():
        pytest.skip("no GPU visible")
    r = SunRig(test_suns.field(), noise, test_suns.DIMS)
    yield r
    r.close()
    test_suns._state.clear()


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", ORDER)
def test_sun_frames_equal_the_oracle(name, mode, rig):
    """Every case at v1, full quality and with mirrors on every surface (whose surfaces march too): all words,
    all counters, again through the integer index.  The soft cases again with the pooled march and with its
    LDS brick staging, which must fall back wherever the samples do not share one fast octant (frame_consts'
    soft_sg = -1), and, sharing one, read the cone copy without doom codes (the brick march has no doom rule;
    the oracle skips the table for that flag too)."""
    fr = frame_of(name, flags=MODES[mode])
    ref, g = rig.check(fr)
    assert (g["shadow_rays"] > 0) == CASES[name].get("marches", True)
    if name in SOFT:
        for extra in (SOFT_POOL, SOFT_POOL | SOFT_BRICK):
            ref2, g2 = rig.check(with_flags(fr, extra))
            assert_words_equal_nan_positions(ref2, ref)
            assert g2["shadow_rays"] == g["shadow_rays"]


@pytest.mark.parametrize("name", ORDER)
def test_table_modes(name, rig):
    """The default frame equals the VX_FLAG_NO_DOOM, VX_FLAG_NO_CONE and VX_FLAG_NO_EXIT frames word for word,
    and each one's shadow_fetches and shadow_rays equal the oracle's in the matching mode: exit=True, the same
    with the flag, exit="orthant", exit=False."""
    fr = frame_of(name)
    base = None
    for flag, o in ((0, rig.oracle), (NO_DOOM, rig.oracle), (NO_CONE, rig.orthant), (NO_EXIT, rig.literal)):
        f = with_flags(fr, flag)
        img, st = rig.scene.render(f, stats=True)
        ref, ost = o.render(f.params, f.width, f.height)
        assert (st.shadow_fetches, st.shadow_rays) == (ost.shadow_fetches, ost.shadow_rays), hex(flag)
        if base is None:
            base = img
            assert_words_equal_nan_positions(img, ref)
        else:
            assert_words_equal_nan_positions(img, base)


@pytest.mark.parametrize("name", ORDER)
def test_prepare_sun_matches_the_plan(name, rig):
    """vx_prepare_sun reports the cone copy with the oracle's (octant, kx, ky) exactly when vxo_exit_plan says
    cone; else the orthant copy of sample 0's octant when sample 0 is on the fast path (frame_exit looks at
    sample 0 alone, also where the samples' octants differ, and also below the horizon, where nothing
    marches); else none.  None under VX_FLAG_NO_EXIT; never a cone under VX_FLAG_NO_CONE."""
    fr = frame_of(name)
    want = expected_exit(fr.params)
    info = rig.scene.prepare_sun(fr)
    assert (info["kind"], info["octant"], info["kx"], info["ky"]) == want
    info = rig.scene.prepare_sun(with_flags(fr, NO_CONE))
    octs = test_suns.classify(test_suns.samples(fr.params))[1]
    assert (info["kind"], info["octant"], info["kx"], info["ky"]) == ((1, octs[0], -1, -1) if octs[0] >= 0
                                                                      else (0, -1, -1, -1))
    assert rig.scene.prepare_sun(with_flags(fr, NO_EXIT))["kind"] == 0
    if name == "below":
        assert want == (1, 3, -1, -1)
    if name in ("nadir", "zero", "soft_zero", "no_tangent"):
        assert want == (0, -1, -1, -1)


@pytest.mark.parametrize("sun", [GENERIC, SLOPE4], ids=["generic", "slope4"])
@pytest.mark.parametrize("budget", BUDGETS)
def test_step_budgets(budget, sun, rig):
    """max_shadow_steps 1, 2, 3, 5 (hmax = 0: a cone copy without a doom table) and 1000 (hmax up to the last
    int8 code, -128): frames and every counter against the oracle, with and without VX_FLAG_NO_DOOM, and the
    two frames against each other."""
    fr = budget_frame(sun, budget)
    ref, g = rig.check(fr)
    ref2, g2 = rig.check(with_flags(fr, NO_DOOM))
    assert_words_equal_nan_positions(ref2, ref)
    assert g["shadow_rays"] == g2["shadow_rays"] == 2740 and g["shadow_fetches"] <= g2["shadow_fetches"]
    if budget <= 5:
        assert g["shadow_fetches"] == g2["shadow_fetches"]          # no table either way
    else:
        assert g["shadow_fetches"] < g2["shadow_fetches"]


@pytest.mark.parametrize("key", list(SMALL_DIMS))
def test_small_fields(key, built, noise):
    """37 x 29 x 3 (SB = 5 = kx at slope 4, the limit of launch_sun_cone's guard) and 37 x 29 x 2 (SB < 5: no
    cone); X and Y are no multiples of the doom build's 8-cell block.  Hard and 4-sample soft shadows under the
    default flags, VX_FLAG_NO_DOOM and VX_FLAG_NO_EXIT (that one against the literal oracle)."""
    if not gpu_available():
        pytest.skip("no GPU visible")
    dims = SMALL_DIMS[key]
    r = SunRig(test_suns.small_field(key), noise, dims)
    try:
        for sun in SMALL_SUNS:
            for n, radius in ((0, 0.0), (4, .02)):
                fr = small_frame(sun, n, radius)
                ref, g = r.check(fr)
                assert g["shadow_rays"] > 0
                ref2, _ = r.check(with_flags(fr, NO_DOOM))
                ref3, _ = r.check(with_flags(fr, NO_EXIT), oracle=r.literal)
                assert_words_equal_nan_positions(ref2, ref)
                assert_words_equal_nan_positions(ref3, ref)
        info = r.scene.prepare_sun(small_frame(SLOPE4))
        got = (info["kind"], info["octant"], info["kx"], info["ky"])
        assert got == ((2, 7, 5, 5) if dims[2] == 3 else (1, 7, -1, -1))
        assert got == expected_exit(small_frame(SLOPE4).params, dims[2])
    finally:
        r.close()
        test_suns._state.pop(key, None)


@pytest.mark.parametrize("name", ["s4_x", "s4_xy", "x_straddle"])
def test_rgba8(name, rig):
    rig.check(frame_of(name), rgba8=True)


def test_sun_argument_checks(rig):
    """vx_render's sun arguments: a NaN or infinite sun_dir component is refused with VX_EINVAL, naming the
    field; shadow_samples = 17 is refused; with 4 samples a sun_radius of -0.0 and 0.5 is accepted and one of
    nextafter(0.5, 1), -2^-30 and NaN refused; with shadow_samples <= 1 any finite radius is accepted."""
    import voxmap_amd as vx
    from voxmap_amd import _abi

    def frame(**kw):
        return frame_from_basis(**POSE, w=32, h=24, flags=FULL, **kw)

    def refused(field, **kw):
        with pytest.raises(vx.VoxmapError) as e:
            rig.scene.render(frame(**kw))
        assert e.value.code == _abi.VX_EINVAL and field in str(e.value), str(e.value)

    for ax in range(3):
        for bad in (float("nan"), float("inf"), -float("inf")):
            refused("sun_dir", sun=tuple(bad if i == ax else GENERIC[i] for i in range(3)))
    refused("shadow_samples", sun=GENERIC, shadow_samples=17, sun_radius=.03)
    over = float(np.nextafter(np.float32(.5), np.float32(1)))
    for bad in (over, -2.0 ** -30, float("nan")):
        refused("sun_radius", sun=GENERIC, shadow_samples=4, sun_radius=bad)
    for good in (-0.0, .5):
        _, g = rig.check(frame(sun=GENERIC, shadow_samples=4, sun_radius=good))
        assert g["shadow_rays"] > 0 and g["shadow_rays"] % 4 == 0
    for n, radius in ((1, 7.5), (0, -3.0), (-2, 1e30), (1, over), (0, .5)):
        _, g = rig.check(frame(sun=GENERIC, shadow_samples=n, sun_radius=radius))
        assert g["shadow_rays"] > 0
