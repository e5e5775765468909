"""The per-frame ray-length bit (FrameConsts::rays_ranged) changes no frame.

vx_render* decide once per frame, from the ray basis alone, whether every view
ray's length lies in [2^-40, 2^41); the sky branch of k_render then normalises
the view ray without the IEEE square root's and division's range handling
(normalize3_ranged) and clamps with the hardware clamp, else it runs the literal
forms.  The host's test is conservative: it wants |fwd| + |right| + |up| in
[2^-28, 2^40) and the plane fwd + span(right, up) at least 2^-10 of that sum
away from the origin.  Here a sky-heavy pose is rendered at 64 x 48

  as it is (the bit set: an orthogonal basis of ordinary size),
  with the basis scaled by 2^-50 and by 2^50 (exact scalings: the bit clear,
    every length outside the ranged form's domain), and
  with a sheared basis that comes out of vx_frame_from_matrix, `up` almost
    parallel to `fwd`, so that the plane passes the origin at 8e-4 of the
    basis' size (the bit clear, the lengths themselves ordinary)

and every frame must equal the oracle's in every fp32 word and counter
(gpu_rig.Rig.check, which also renders through the integer index).  The
same frames through vx_render_tiles and vx_render_bands must equal the whole
frame.  A second pose with blocks and sky takes the same four bases.
"""
import numpy as np
import pytest

import test_poses
from gpu_rig import Rig, gpu_available
from test_poses import frame_from_basis, poses

pytestmark = pytest.mark.gpu

WH = (64, 48)
FULL = 0x30
BASES = ["unit", "tiny", "huge", "sheared"]


@pytest.fixture(scope="module")
def rig(built, noise):
    if not gpu_available():
        pytest.skip("no GPU visible")
    r = Rig(test_poses.field(), noise, test_poses.DIMS)
    yield r
    r.close()
    test_poses._state.clear()


def sheared(q):
    """The pose's basis with `up` replaced by 1.2 fwd + 0.001 of the old up, through a u_matrix: unprojecting
    NDC (x, y, 1, 1) by the inverse gives cam + fwd + x right + y up (w = 1), which is what
    vx_frame_from_matrix reads its basis from."""
    import voxmap_amd as vx
    fwd, right, up = (np.array(q[k], np.float64) for k in ("fwd", "right", "up"))
    fwd = fwd / np.linalg.norm(fwd)
    up2 = 1.2 * fwd + 0.001 * up
    cam = np.array(q["cell"], np.float64) + np.array(q["fract"], np.float64)
    third = np.cross(right, fwd)                       # any vector that makes the inverse well conditioned
    inv = np.zeros((4, 4))
    inv[:3, 0], inv[:3, 1], inv[:3, 2] = right, up2, third
    inv[:3, 3], inv[3, 3] = cam + fwd - third, 1.0
    m = np.linalg.inv(inv)
    p = vx.frame_from_matrix(m.T.reshape(-1).tolist(), cam.tolist())     # column-major
    got = [np.array([v[i] for i in range(3)]) for v in (p.ray_fwd, p.ray_right, p.ray_up)]
    assert np.allclose(got[0], fwd, atol=1e-5) and np.allclose(got[1], right, atol=1e-5)
    assert np.allclose(got[2], up2, atol=1e-5)
    return dict(q, fwd=tuple(got[0]), right=tuple(got[1]), up=tuple(got[2]))


def based(name, basis):
    q = poses()[name]
    q = {k: q[k] for k in ("cell", "fract", "fwd", "right", "up")}
    if basis == "sheared":
        return sheared(q)
    s = {"unit": 1.0, "tiny": 2.0 ** -50, "huge": 2.0 ** 50}[basis]
    return dict(q, **{k: tuple(s * v for v in q[k]) for k in ("fwd", "right", "up")})


def expected_bit(q):
    """The host's rule (vx_frame.cpp rays_ranged), restated."""
    f, r, u = (np.array(q[k], np.float32).astype(np.float64) for k in ("fwd", "right", "up"))
    n = np.cross(r, u)
    S = sum(np.linalg.norm(v) for v in (f, r, u))
    return bool(np.linalg.norm(n) > 0 and 2.0 ** -28 <= S < 2.0 ** 40 and abs(f @ n) / np.linalg.norm(n) >= S * 2.0 ** -10)


@pytest.mark.parametrize("basis", BASES)
@pytest.mark.parametrize("name", ["sky_up", "plus_x_axis"])
def test_frames_equal_the_oracle_whatever_the_bit(name, basis, rig):
    q = based(name, basis)
    assert expected_bit(q) == (basis == "unit")
    for flags in (0, FULL):
        _, g = rig.check(frame_from_basis(**q, w=WH[0], h=WH[1], flags=flags))
        assert g["sky_px"] > 0
        if name == "sky_up" and basis != "sheared":
            assert g["sky_px"] == g["pixels"] and g["noise_px"] > 0


@pytest.mark.parametrize("basis", BASES)
def test_tiles_and_bands_equal_the_frame(basis, rig):
    import torch
    import voxmap_amd as vx
    w, h = WH
    fr = frame_from_basis(**based("sky_up", basis), w=w, h=h, flags=FULL)
    whole, _ = rig.scene.render(fr)
    out = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    rig.scene.render_bands(fr, 16, [0, 1, 2], out.data_ptr(), inplace=True, pixel_format=vx.PIXEL_RGBA32F)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint32), whole.view(np.uint32))
    ts = 32                                            # 2 x 2 tiles, the lower two 16 rows high
    tiles = torch.zeros((4, ts, ts, 4), dtype=torch.float32, device="cuda")
    rig.scene.render_tiles(fr, ts, [0, 1, 2, 3], tiles.data_ptr(), pixel_format=vx.PIXEL_RGBA32F)
    torch.cuda.synchronize()
    t = tiles.cpu().numpy()
    for k in range(4):
        y0, x0 = (k // 2) * ts, (k % 2) * ts
        part = whole[y0:y0 + ts, x0:x0 + ts]
        assert np.array_equal(t[k, :part.shape[0], :part.shape[1]].view(np.uint32), part.view(np.uint32)), k
