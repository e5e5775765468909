"""Degenerate camera poses on the GPU against the oracle.

The poses of tests/test_poses.py (whose table, builder and field this file
imports; that file holds the oracle to itself on them and shows that the
frames are not empty and really have the directions claimed): axis-aligned
bases, whose centre column and row have exact zero direction components (a
wave with such a lane takes the IEEE-division / slab branch of primary<> and
of ray_rcp; a mirror ray off an axis-aligned view ray has the same zeros);
origins on cell faces and on the grid's faces, inside a solid and a glass cell,
below the grid; cameras at |cell| = 2^20, 2^21 and 2^22 - 1; a hit at t = 0.
Every frame is compared with oracle.Oracle(dev_field, noise, exit=True) on
every fp32 word and every counter the oracle keeps, then rendered again with
VX_FLAG_INT_INDEX: the same frame and counters from the other index path.
"""
import numpy as np
import pytest

import test_poses
from gpu_rig import Rig, gpu_available
from test_poses import EVEN, MODES_2D, NAMES, ODD, P22, THRESHOLDS, TIMES, frame_from_basis, frame_of, poses, sizes_of

pytestmark = pytest.mark.gpu

UNIT_GBUF, GLASS_ORDER, REFLECT_ALL, PRIMARY_ONLY = 0x800, 0x1000, 0x2000, 0x8
MODES = {
    "v1": dict(flags=0),
    "full": dict(flags=0x30),
    "reflect_all": dict(flags=REFLECT_ALL | 0x30),
    "soft4": dict(flags=0x30, shadow_samples=4, sun_radius=0.03),
    "unit_gbuf": dict(flags=UNIT_GBUF),
    "glass_order": dict(flags=GLASS_ORDER | 0x30),
    "primary_only": dict(flags=PRIMARY_ONLY),
}


@pytest.fixture(scope="module")
def rig(built, noise):
    if not gpu_available():
        pytest.skip("no GPU visible")
    r = Rig(test_poses.field(), noise, test_poses.DIMS)
    yield r
    r.close()
    test_poses._state.clear()


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", [n for n in NAMES if n != "t0_hit"])
def test_pose_frames_equal_the_oracle(name, mode, rig):
    """Every pose in every mode, at each of its sizes, and again through the integer index.

    The index path (vx_render picks the fp32 index iff |cam_cell.x|, |cam_cell.y| < 2^21 and |cam_cell.z| <
    2^20, and the test cannot see which it took): far_x_m21m1, far_x_p21m1, far_y_p21m1 and far_z_20m1, one
    cell inside a bound, take the fp32 index, where the biased index arithmetic is at its limits; far_x_m21,
    far_x_p21, far_y_p21, far_y_m21 and far_z_20, on a bound, and the 2^22 - 1 poses and far_diag take the
    integer index on their own; every other pose takes the fp32 index.  Each is compared with the oracle in the
    path it takes, and the fp32 ones again in the integer path."""
    for wh in sizes_of(name):
        _, g = rig.check(frame_of(name, wh, **MODES[mode]))
        if name == "sky_up":
            assert g["sky_px"] == g["pixels"]


def test_t0_hit(rig):
    """The camera on the face it looks at: every view ray hits at t = 0 and rayDir = normalize(0) is NaN
    (DESIGN.md §5).  Every mode; with REFLECT_ALL every pixel's RGB is NaN in the oracle (test_poses.py), and the
    kernel's must be NaN at the same words with all counters equal.

    Where the NaN goes in the kernel, and why no index is formed from it.  shade_block computes rayDir and
    reads it only for a glass record's alpha and tint (arithmetic) and hands it to the caller for the mirror
    ray; the block's own AO sample, rough-normal lookup and sun march read the record's cell and fraction,
    which are finite (the hit point is the camera).  reflect_color negates one component and starts
    walk_reflect.  Its start cell B + c comes from the glass record and from comparisons (R > 0 and d < 0, false
    for NaN), never from d's value: the first fetch reads an in-grid or border texel of octant copy 0 as for
    any ray.  Beside that texel's sentinel test the walk now tests the direction, and one that is not finite
    returns "sky" there with no fetch counted, so the step loop, whose next cell would be a med3 of
    floor(o + te * d) with a NaN te under an exit axis chosen by comparisons that are all false, never runs on
    it: no med3 with a NaN operand is reached, and no reflected shade_block.  shade_sky then runs on the NaN
    direction.  Its only indices are the noise lookups, formed by wrap_idx: for a NaN (not |fl| < 2^24) it
    takes f2i(fl - q * n) & (n - 1), f2i(NaN) = 0 by an explicit select, and the mask holds any value inside
    the texture; the mountain branch's comparisons are false.  Everything else there is arithmetic.  The
    oracle has the same rule (reflect_color).  Before it, the oracle's walk() stepped such a ray along -z
    through the extents of the +z octant (its two sign tests disagree on NaN: 6 fetches a ray here, ending on
    the ground, which it then shaded with a NaN fraction), and the kernel would have walked +z to the sentinel;
    neither was a defined result.  The Fresnel weight min(|NaN|, 1) is NaN, so the pixel is NaN whatever the
    mirror colour is."""
    for mode, kw in MODES.items():
        for wh in (ODD, EVEN):
            ref, g = rig.check(frame_of("t0_hit", wh, **kw))
            assert g["block_px"] == g["pixels"]
            if mode == "reflect_all":
                assert np.isnan(ref[..., :3]).all() and g["reflect_rays"] == g["pixels"] and g["reflect_fetches"] == 0
            else:
                assert not np.isnan(ref).any()


@pytest.mark.parametrize("fp32_side,int_side", THRESHOLDS)
def test_either_side_of_the_index_switch(fp32_side, int_side, rig):
    """One cell inside the bound (the fp32 index on its own) and on it (the integer index on its own), full
    quality with mirrors on every surface, both sizes; RGBA8 too."""
    for name in (fp32_side, int_side):
        for wh in (ODD, EVEN):
            rig.check(frame_of(name, wh, flags=REFLECT_ALL | 0x30), rgba8=True)


@pytest.mark.parametrize("name", ["down_axis", "far_x_m21", "far_diag"])
def test_rgba8(name, rig):
    for kw in (MODES["v1"], MODES["full"]):
        rig.check(frame_of(name, ODD, **kw), int_index=False, rgba8=True)


@pytest.mark.parametrize("name", MODES_2D)
def test_2d_mode(name, rig):
    """quality = 0: the footprint seen from above (k_render_2d reads cam_cell as the frame kernels do);
    from below the plane everything is the clear colour."""
    for wh in (ODD, EVEN):
        _, g = rig.check(frame_of(name, wh, quality=0), rgba8=True)
        if name == "up_from_below":
            assert g["sky_px"] == g["pixels"]
        else:
            assert 10 * (g["block_px"] + g["glass_px"]) >= 3 * g["pixels"]


@pytest.mark.parametrize("time", TIMES)
@pytest.mark.parametrize("name", ["sky_up", "down_axis"])
def test_time(name, time, rig):
    """Every cloud lookup depends on time (test_poses.py: the oracle's sky_up frames differ between them)."""
    for kw in (MODES["v1"], MODES["reflect_all"]):
        _, g = rig.check(frame_of(name, ODD, time=time, **kw))
        assert g["noise_px"] > 0 or (name, kw) == ("down_axis", MODES["v1"])


def test_check_frame_bounds(rig):
    """vx_render refuses, before any launch and naming the field: cam_cell = +-2^22, cam_fract = 1 and
    -2^-30, a NaN ray_up.  cam_cell = +-(2^22 - 1) and cam_fract = -0.0 are accepted."""
    import voxmap_amd as vx
    from voxmap_amd import _abi
    q = {k: poses()["down_axis"][k] for k in ("cell", "fract", "fwd", "right", "up")}

    def refused(field, **kw):
        with pytest.raises(vx.VoxmapError) as e:
            rig.scene.render(frame_from_basis(**dict(q, **kw), w=8, h=8))
        assert e.value.code == _abi.VX_EINVAL and field in str(e.value), str(e.value)

    for ax in range(3):
        for v in (P22, -P22):
            refused("cam_cell", cell=tuple(v if i == ax else q["cell"][i] for i in range(3)))
        for v in (1.0, -2.0 ** -30):
            refused("cam_fract", fract=tuple(v if i == ax else .5 for i in range(3)))
        refused("ray_up", up=tuple(float("nan") if i == ax else q["up"][i] for i in range(3)))
        for v in (P22 - 1, -(P22 - 1)):
            cell = tuple(v if i == ax else q["cell"][i] for i in range(3))
            rig.check(frame_from_basis(**dict(q, cell=cell), w=8, h=8))
        rig.check(frame_from_basis(**dict(q, fract=tuple(-0.0 if i == ax else .5 for i in range(3))), w=8, h=8))
