"""The RGBA8 frame is the RGBA32F frame packed: byte = floor(clamp(v, 0, 1) * 255 + 0.5).

pack_rgba8 clamps with the hardware's clamp (vx_math.h clamp01) where the
contract spells min(max(v, 0), 1) as two selects; the forms differ on NaN and
-0 only, and both then give byte 0.  Here every pose of tests/test_poses.py --
the degenerate ones included: t0_hit with mirrors on every surface has NaN in
every colour, clouds lit toward sunCol.r = 1.4 may exceed 1 -- and a glass wall over
bright sky (the 'blend_bright' scene of tests/golden, whose panes blend clamped
values over the canvas byte) is rendered at 96 x 64 in both pixel formats, and
the RGBA8 frame must be the host's packing of the RGBA32F one, byte for byte.
"""
import numpy as np
import pytest

import test_poses
from gpu_rig import bin_scene, gpu_available, quantise_rgba8
from test_poses import NAMES, frame_of

pytestmark = pytest.mark.gpu

WH = (96, 64)
REFLECT_ALL = 0x2000
MODES = {"v1": dict(flags=0), "full": dict(flags=0x30), "reflect_all": dict(flags=REFLECT_ALL | 0x30),
         "no_clouds": dict(flags=0x4)}


def pack(img):
    """floor(clamp(v, 0, 1) * 255 + 0.5) in fp32, one rounding per operation; NaN packs to 0."""
    return quantise_rgba8(np.where(np.isnan(img), np.float32(0), img).astype(np.float32))


def both(scene, fr):
    import voxmap_amd as vx
    f32, _ = scene.render(fr)
    u8, _ = scene.render(fr, pixel_format=vx.PIXEL_RGBA8)
    return f32, u8


@pytest.fixture(scope="module")
def scene(built, noise):
    if not gpu_available():
        pytest.skip("no GPU visible")
    sc = bin_scene(test_poses.field(), noise, test_poses.DIMS)
    yield sc
    sc.close()
    test_poses._state.clear()


@pytest.mark.parametrize("mode", list(MODES))
def test_rgba8_is_the_packed_float_frame(mode, scene):
    seen_nan = 0
    for name in NAMES:
        f32, u8 = both(scene, frame_of(name, WH, **MODES[mode]))
        assert np.array_equal(u8, pack(f32)), name
        seen_nan += int(np.isnan(f32).sum())
    if mode == "reflect_all":
        assert seen_nan >= 3 * WH[0] * WH[1]          # t0_hit: every colour NaN (tests/test_poses.py)


def test_glass_wall_over_bright_sky(built, noise):
    """The blend stage's source: panes over clouds brighter than 1, grazing mirrors (full quality)."""
    if not gpu_available():
        pytest.skip("no GPU visible")
    import voxmap_amd as vx
    from voxmap_amd import scenes
    g = scenes.glass_wall()
    Z, Y, X = g.shape
    field = vx.field_build(g)
    with bin_scene(field, noise, (X, Y, Z)) as sc:
        for flags in (0x30, 0):
            fr = vx.make_frame((24.0, 20.0, 6.0), (2.1, 0.0, -0.5235987755982988), WH[0], WH[1], flags=flags)
            (f32, st), (u8, _) = sc.render(fr, stats=True), sc.render(fr, pixel_format=vx.PIXEL_RGBA8)
            assert st.glass_px >= 100 and st.sky_px >= 100
            assert np.array_equal(u8, pack(f32)), flags
