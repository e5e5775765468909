"""The primary walk's per-lane octant constants and its hit record, axis by axis, against the oracle.

primary() places a ray's octant terms (s, hp, the index constants) from its three sign compares and the
record's values (quad offsets, the face plane, the zero fraction, the normal index) from the exit axis of the
last step.  The field and the cameras here are built so that every one of those placements takes every value
it can: faces of all six normals in view, greedy quads whose faces carry non-zero offsets along both in-face
axes at once and an offset at the mesh chunk's edge, a glass pane in front of a slab and a second in front of
that (the glass record and the stacked pass), one camera along each octant diagonal, two whose frame centre
lies along an axis (the sign changes cut through the 8 x 8-pixel waves, so a wave mixes octants), and one
above the grid, where the slab entry starts the walk.  Every frame goes through Rig.check with the integer
index and the RGBA8 frame: words and counters equal to oracle.Oracle(dev_field, noise, exit=True)."""
import math

import numpy as np
import pytest

from gpu_rig import Rig, gpu_available
from test_poses import frame_from_basis

pytestmark = pytest.mark.gpu

DIMS = (24, 20, 12)
CHUNK = 8
GLASS = 21
SIZES = ((64, 40), (61, 37))            # whole waves; partial edge waves and a centre column and row of exact zeros
FLAGS = (0, 0x30, 0x800, 0x8)           # v1, full quality, VX_FLAG_UNIT_GBUF, VX_FLAG_PRIMARY_ONLY


def grid():
    """(Z, Y, X) colours: the ground slab, a wall slab, a pillar that floats (its underside is a face), and two
    glass panes one behind the other in front of the wall."""
    X, Y, Z = DIMS
    g = np.zeros((Z, Y, X), np.uint8)
    g[0:2, :, :] = 3                    # ground: +z faces 24 x 20, cut by the chunks of 8
    g[2:10, 2:18, 17:20] = 5            # wall: -x / +x faces 16 x 8, -y / +y 3 x 8, top 3 x 16
    g[5:10, 5:10, 3:8] = 9              # pillar, air beneath: all six normals, 5 x 5 faces
    g[2:8, 6:14, 14] = GLASS            # pane in front of the wall
    g[2:8, 6:14, 11] = GLASS            # and a second in front of that
    return g


def _unit(v):
    n = math.sqrt(sum(c * c for c in v))
    return tuple(c / n for c in v)


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _camera(pos, fwd, spread=(.8, .5)):
    f = _unit(fwd)
    helper = (0.0, 0.0, 1.0) if abs(f[2]) < .9 else (1.0, 0.0, 0.0)
    r = _unit(_cross(f, helper))
    u = _unit(_cross(r, f))
    cell = tuple(math.floor(p) for p in pos)
    return dict(cell=cell, fract=tuple(p - c for p, c in zip(pos, cell)), fwd=f,
                right=tuple(spread[0] * c for c in r), up=tuple(spread[1] * c for c in u))


INSIDE = (9.4, 10.4, 3.6)               # in the air between the pillar and the nearer pane
CAMERAS = {f"oct{o}": _camera(INSIDE, tuple(-1.0 if o >> i & 1 else 1.0 for i in range(3))) for o in range(8)}
# a frame centre along an axis: d.y and d.z (d.x and d.y) change sign inside the frame's middle waves
CAMERAS["plus_x"] = dict(cell=(1, 10, 4), fract=(.5, .25, .75), fwd=(1.0, 0.0, 0.0), right=(0.0, -.8, 0.0),
                         up=(0.0, 0.0, .5))
CAMERAS["minus_z"] = dict(cell=(9, 11, 11), fract=(.25, .5, .5), fwd=(0.0, 0.0, -1.0), right=(.8, 0.0, 0.0),
                          up=(0.0, .5, 0.0))
CAMERAS["above"] = _camera((-4.5, -3.25, 19.5), (1.0, .8, -.9), spread=(.6, .4))


class ChunkRig(Rig):
    def make_oracle(self, noise):
        import oracle
        return oracle.Oracle(self.dev_field, noise, exit=True, chunk=CHUNK)


@pytest.fixture(scope="module")
def rig(built, noise):
    if not gpu_available():
        pytest.skip("no GPU visible")
    import oracle
    r = ChunkRig(oracle.field_build(grid()), noise, DIMS, mesh_chunk=CHUNK)
    yield r
    r.close()


def test_the_field_has_what_the_cameras_need(rig):
    """Faces of every normal whose offsets are non-zero along both in-face axes (on quads at least 3 cells a
    side) and reach the chunk's edge; the +x camera sees one pane and two panes in front of a surface, and
    the inside cameras' frame centres cover the eight octants."""
    q = rig.oracle.qoff
    face = q != 0xFFFF
    du, dv = q & 0xff, q >> 8
    for n in range(6):
        assert (face[..., n] & (du[..., n] >= 2) & (dv[..., n] >= 2)).any(), n
    assert (face & (du == CHUNK - 1)).any() and (face & (dv == CHUNK - 1)).any()
    fr = frame_from_basis(**CAMERAS["plus_x"], w=64, h=40)
    layers = rig.oracle.glass_layers(fr.params, 64, 40)
    assert (layers >= 2).any() and (layers == 1).any()
    for o in range(8):
        fwd = CAMERAS[f"oct{o}"]["fwd"]
        assert sum((1 << i) for i in range(3) if fwd[i] < 0) == o


@pytest.mark.parametrize("name", list(CAMERAS))
def test_frames_equal_the_oracle(name, rig):
    for w, h in SIZES:
        for flags in FLAGS:
            _, g = rig.check(frame_from_basis(**CAMERAS[name], w=w, h=h, flags=flags), int_index=True, rgba8=True)
            assert g["block_px"] + g["glass_px"] > 0
            if name == "plus_x":                                # through both panes
                assert g["glass_px"] > 0
