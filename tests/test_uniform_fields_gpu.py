"""The values the host computes for the frame kernels in place of wave-uniform vector work: per scene the
float copies of the dimensions ((float)X, Y, Z, noise_w, noise_h, SXp, Xp, 4 Xp), per frame "the sun goes
down" (sun.z < 0.0f), per sun sample its axis-sign pattern (the fast march's switch).

A wrong or stale one of them gives a wrong frame, so every case is a frame held to the oracle: gpu_rig's
Rig.check with rgba8=True (the counting fp32 kernel, the integer index, the RGBA8 kernel) and, beside it, the
fp32 kernel that does not count, word for word equal to the one that does.  The scene is small and odd, so
that no dimension is a power of two or equal to another: 24 x 20 x 12 with a 64 x 32 noise texture, frames of
64 x 48.  The cases: the eight sun octants at v1 and full-quality flags, hard and 4-sample soft shadows (the
EXT 0, 1 and 2 kernels); suns with z = -0.0, +0.0 and z < 0; a zero component (the literal march, which must
not look at the sign pattern); suns within 2^-10 of perpendicular to each axis normal (the ROUGH sun factor's
smallest arguments); bands (the TILED kernels) against the whole frame's rows; two suns alternating on one
scene; two scenes of different dimensions alive at once.

test_the_oracle_renders_every_case_finite runs without a GPU: no case's frame has a NaN (an RGBA8 frame
could not hold one), and the pose sees blocks, glass and sky and marches lit and unlit shadow rays."""
import numpy as np
import pytest

from gpu_rig import Rig, assert_bytes_equal, assert_words_equal, gpu_available
from test_poses import frame_from_basis

DIMS, NOISE_WH = (24, 20, 12), (64, 32)
DIMS_B, NOISE_WH_B = (17, 23, 9), (32, 128)
WH = (64, 48)
POSE = dict(cell=(-5, -4, 15), fract=(.25, .5, .75), fwd=(.62, .52, -.5), right=(.5, -.6, 0), up=(.2, .17, .45))
FULL = 0x30                                        # VX_FLAG_REFLECT | VX_FLAG_ROUGH
E = 2.0 ** -11
OCTANTS = [tuple(s * v for s, v in zip(sg, (.5, .3, .8))) for sg in
           [(sx, sy, sz) for sz in (1, -1) for sy in (1, -1) for sx in (1, -1)]]
HORIZON = {"negzero": (.6, .8, -0.0), "poszero": (.6, .8, 0.0), "down": (.5, .3, -.8)}
ZERO_COMPONENT = (0.0, .6, .8)
# within 2^-10 of perpendicular to the normals of each axis: that component +-2^-11 (z = -2^-11 is "down")
PERPENDICULAR = [tuple(s * E if i == ax else v for i, v in enumerate(base))
                 for ax, base in ((0, (0, .6, .8)), (1, (.6, 0, .8)), (2, (.6, .8, 0))) for s in (1, -1)]
MODES = [(0, 0, 0.0), (FULL, 0, 0.0), (0, 4, .03), (FULL, 4, .03)]   # (flags, shadow samples, sun radius)


def frame(sun, flags=FULL, n=0, radius=0.0, pose=POSE):
    return frame_from_basis(**pose, w=WH[0], h=WH[1], sun=sun, flags=flags, shadow_samples=n, sun_radius=radius)


def all_cases():
    """(id, frame) of every frame the GPU tests hold to the oracle on the main scene."""
    out = []
    for i, sun in enumerate(OCTANTS):
        out += [(f"oct{i}_{fl:x}_{n}", frame(sun, fl, n, r)) for fl, n, r in MODES]
    for name, sun in HORIZON.items():
        out += [(f"{name}_{fl:x}", frame(sun, fl)) for fl in (0, FULL)]
    out += [(f"zero_{n}", frame(ZERO_COMPONENT, FULL, n, r)) for n, r in ((0, 0.0), (4, .03))]
    out += [(f"perp{i}", frame(sun)) for i, sun in enumerate(PERPENDICULAR)]
    return out


def make_field(dims, seed):
    import oracle
    from voxmap_amd import scenes
    return oracle.field_build(scenes.odd_proc(seed, dims))


def make_noise(wh, seed):
    import voxmap_amd as vx
    return vx.noise_synth(seed, wh[0], wh[1])


def test_the_oracle_renders_every_case_finite(built):
    import oracle
    o = oracle.Oracle(make_field(DIMS, 7), make_noise(NOISE_WH, 3), exit=True)
    assert len({*DIMS, *NOISE_WH}) == 5 and all(d & (d - 1) for d in DIMS)
    for name, fr in all_cases():
        img, st = o.render(fr.params, *WH)
        assert not np.isnan(img).any(), name
        assert st.block_px > 500 and st.glass_px > 10 and st.sky_px > 300, (name, st.as_dict())
    # a sun above the horizon marches, and finds lit and unlit fragments
    for sun in OCTANTS[:4] + [ZERO_COMPONENT] + PERPENDICULAR[:4]:
        fr = frame(sun)
        lit, _ = o.terms(fr.params, *WH)
        v = lit[lit != 255]
        assert (v == 0).sum() >= 20 and (v == 1).sum() >= 20, sun
    for name, sun in HORIZON.items():
        _, st = o.render(frame(sun).params, *WH)
        # ROUGH: z = +-0 is not "down" (its jittered normals still face the sun), z < 0 is
        assert (st.shadow_rays > 0) == (name != "down"), name
    # the perpendicular suns reach the ROUGH root with small arguments on the faces of their axis
    assert all(abs(s[ax]) == E for ax in range(3) for s in PERPENDICULAR[2 * ax:2 * ax + 2])


class BothKernelsRig(Rig):
    same = staticmethod(assert_words_equal)        # no case has a NaN (the CPU test above)

    def check_all(self, fr):
        """Rig.check with the RGBA8 frame, and the fp32 kernel without counters equal to the one with them."""
        ref, g = self.check(fr, rgba8=True)
        counted, _ = self.scene.render(fr, stats=True)
        plain, _ = self.scene.render(fr)
        assert_words_equal(plain, counted)
        assert_words_equal(plain, ref)
        return ref, g


@pytest.fixture(scope="module")
def rig(built):
    if not gpu_available():
        pytest.skip("no GPU visible")
    r = BothKernelsRig(make_field(DIMS, 7), make_noise(NOISE_WH, 3), DIMS)
    yield r
    r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("octant", range(8))
def test_sun_octants(octant, rig):
    """Each sign pattern at v1 and ROUGH | REFLECT, hard and 4-sample soft: the EXT 0, 1 and 2 kernels."""
    for flags, n, radius in MODES:
        _, g = rig.check_all(frame(OCTANTS[octant], flags, n, radius))
        assert (g["shadow_rays"] > 0) == (OCTANTS[octant][2] > 0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(HORIZON))
def test_sun_on_and_under_the_horizon(name, rig):
    """z = -0.0 and +0.0 are not "down" (-0.0 < 0.0f is false): with ROUGH their fragments still march."""
    for flags in (0, FULL):
        _, g = rig.check_all(frame(HORIZON[name], flags))
        if flags == FULL:
            assert (g["shadow_rays"] > 0) == (name != "down")


@pytest.mark.gpu
def test_zero_component_takes_the_literal_march(rig):
    for n, radius in ((0, 0.0), (4, .03)):
        _, g = rig.check_all(frame(ZERO_COMPONENT, FULL, n, radius))
        assert g["shadow_rays"] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(len(PERPENDICULAR)))
def test_suns_nearly_perpendicular_to_an_axis(k, rig):
    rig.check_all(frame(PERPENDICULAR[k]))


@pytest.mark.gpu
@pytest.mark.parametrize("flags,n,radius", MODES)
def test_bands_equal_the_frames_rows(flags, n, radius, rig):
    """Bands of 8 rows (the TILED kernels), in place: RGBA8 and fp32, against the whole frame's rows."""
    import torch

    import voxmap_amd as vx
    fr = frame(OCTANTS[1], flags, n, radius)
    w, h = WH
    ids = [0, 2, 5]
    for fmt, dt, npdt in ((vx.PIXEL_RGBA8, torch.uint8, np.uint8), (vx.PIXEL_RGBA32F, torch.float32, np.float32)):
        full, _ = rig.scene.render(fr, pixel_format=fmt)
        out = torch.zeros(h * w * 4, dtype=dt, device="cuda:0")
        torch.cuda.synchronize()        # the fill (torch's stream) before the scene's stream writes
        rig.scene.render_bands(fr, 8, ids, out.data_ptr(), inplace=True, pixel_format=fmt)
        torch.cuda.synchronize()
        img = out.cpu().numpy().reshape(h, w, 4)
        rows = np.concatenate([np.arange(8 * b, 8 * b + 8) for b in ids])
        assert img.dtype == npdt
        (assert_bytes_equal if fmt == vx.PIXEL_RGBA8 else assert_words_equal)(img[rows], full[rows])


@pytest.mark.gpu
def test_alternating_suns_on_one_scene(rig):
    """Two frames whose suns differ in octant, in "down" and in the march they take, alternately: each render
    equals the oracle's frame of its own sun (a per-frame value kept from the frame before would not)."""
    import voxmap_amd as vx
    frames = [frame(OCTANTS[0]), frame(OCTANTS[6]), frame(ZERO_COMPONENT, FULL, 4, .03), frame(OCTANTS[3], 0)]
    refs = [rig.check_all(fr)[0] for fr in frames]
    for _ in range(2):
        for fr, ref in zip(frames, refs):
            assert_words_equal(rig.scene.render(fr)[0], ref)
            assert_bytes_equal(rig.scene.render(fr, pixel_format=vx.PIXEL_RGBA8)[0],
                               (np.clip(ref, 0, 1) * np.float32(255) + np.float32(.5)).astype(np.uint8))


@pytest.mark.gpu
def test_two_scenes_of_different_dimensions(rig):
    """A second scene (17 x 23 x 9, noise 32 x 128) alive beside the first: frames of both, interleaved, each
    against its own oracle (a per-scene value shared between scenes would give one of them a wrong frame)."""
    pose_b = dict(cell=(-4, -5, 12), fract=(.5, .25, .5), fwd=(.5, .6, -.5), right=(.6, -.5, 0), up=(.17, .2, .45))
    other = BothKernelsRig(make_field(DIMS_B, 11), make_noise(NOISE_WH_B, 5), DIMS_B)
    try:
        for sun, flags, n, radius in ((OCTANTS[0], FULL, 0, 0.0), (OCTANTS[2], FULL, 4, .03), (OCTANTS[1], 0, 0, 0.0)):
            _, ga = rig.check_all(frame(sun, flags, n, radius))
            _, gb = other.check_all(frame(sun, flags, n, radius, pose=pose_b))
            assert ga["block_px"] > 500 and gb["block_px"] > 300 and gb["shadow_rays"] > 0
    finally:
        other.close()
