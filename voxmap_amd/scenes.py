"""Synthetic scenes in the reference's map.bin format.

The real field (res/map.blob) is AES-encrypted with a key that is not in the
reference repository (src/web/ui.js:47,169-179), so benchmarks and parity
tests run on synthetic palette-index grids with the same layout, turned into
map.bin texels by ``vx_field_build`` (the sdf.cpp:405-470 restatement).

Grids are (Z, Y, X) uint8 palette indices, x fastest in memory like map.bin
(render.js:62).  Index 0 = air, 1..20 = opaque palette colours, 21 = glass
(render.vert:21, sdf.cpp:195,337).
"""
from __future__ import annotations

import gzip
import os

import numpy as np

GLASS = 21
_DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data")


def s_proc(seed: int = 1, dims=(1024, 256, 32), n_boxes: int = 400, n_glass: int = 30) -> np.ndarray:
    """S-proc: ground, ~400 boxes (w 4-40, h 2-28, palette 1-20), ~5% overhang
    slabs, 30 glass panes.  Deterministic in ``seed``."""
    X, Y, Z = dims
    rng = np.random.default_rng(seed)
    g = np.zeros((Z, Y, X), np.uint8)
    g[0] = 2                                   # grass ground at z = 0
    # a few roads / courtyards on the ground plane
    for _ in range(max(1, X // 64)):
        if rng.random() < 0.5:
            y0 = int(rng.integers(0, Y - 8)); g[0, y0:y0 + int(rng.integers(3, 8)), :] = 13
        else:
            x0 = int(rng.integers(0, X - 8)); g[0, :, x0:x0 + int(rng.integers(3, 8))] = 13
    zmax = Z - 1
    for _ in range(n_boxes):
        w = int(rng.integers(4, 41)); d = int(rng.integers(4, 41))
        hgt = int(rng.integers(2, min(29, zmax) + 1))
        x0 = int(rng.integers(0, max(1, X - w))); y0 = int(rng.integers(0, max(1, Y - d)))
        col = int(rng.integers(1, 21))
        if rng.random() < 0.05:                # overhang slab: floating roof with air beneath
            z0 = int(rng.integers(3, max(4, zmax - 3)))
            t = int(rng.integers(1, 4))
            g[z0:min(Z, z0 + t), y0:y0 + d, x0:x0 + w] = col
            # one supporting pillar so it reads as a building
            g[1:z0, y0:y0 + 2, x0:x0 + 2] = col
        else:
            g[1:1 + hgt, y0:y0 + d, x0:x0 + w] = col
    for _ in range(n_glass):                   # glass panes, 1 voxel thick
        L = int(rng.integers(6, 30)); hgt = int(rng.integers(3, min(20, zmax)))
        x0 = int(rng.integers(0, X - L)); y0 = int(rng.integers(0, Y - L))
        if rng.random() < 0.5:
            g[1:1 + hgt, y0, x0:x0 + L] = GLASS
        else:
            g[1:1 + hgt, y0:y0 + L, x0] = GLASS
    return g


# colour -> storey height for the campus extrusion (deterministic, arbitrary:
# the plaintext vertex2d.bin.gz carries top colours but no heights, sdf.cpp:156)
_CAMPUS_HEIGHT = np.array([0, 1, 1, 6, 9, 12, 8, 7, 5, 1, 1, 10, 14, 4, 3, 11, 13, 6, 9, 16, 2, 8], np.int32)


NOISE_PATH = os.path.join(_DATA, "noise.bin.gz")


def real_noise() -> np.ndarray:
    """(1024, 1024, 4) RGBA8: the reference's plaintext res/noise.bin.gz
    (noise.cpp:34-41 layout; render.js:138-149 uploads it as u_noise),
    shipped as data in voxmap_amd/data/."""
    with gzip.open(NOISE_PATH, "rb") as f:
        return np.frombuffer(f.read(), np.uint8).reshape(1024, 1024, 4)


def campus_footprint() -> np.ndarray:
    """(Y, X) top-colour map rasterised from the reference's plaintext
    res/vertex2d.bin.gz by tools/make_campus_footprint.py."""
    path = os.path.join(_DATA, "campus_footprint.npy.gz")
    with gzip.open(path, "rb") as f:
        return np.load(f, allow_pickle=False)


def s_campus(dims=(1024, 256, 32)) -> np.ndarray:
    """S-campus: the real campus footprint extruded by a fixed colour->height table."""
    X, Y, Z = dims
    fp = campus_footprint()
    assert fp.shape == (Y, X), fp.shape
    g = np.zeros((Z, Y, X), np.uint8)
    g[0] = np.where(fp > 0, fp, 2).astype(np.uint8)
    hgt = _CAMPUS_HEIGHT[np.minimum(fp, 21)]
    hgt = np.minimum(hgt, Z - 1)
    for z in range(1, Z):
        m = hgt >= z
        g[z][m] = fp[m]
    return g


def upsample3(g: np.ndarray, k: int = 3) -> np.ndarray:
    """S-up3: nearest k-fold upsample (C5's 3072x768x96 field)."""
    return np.repeat(np.repeat(np.repeat(g, k, axis=0), k, axis=1), k, axis=2)


def s_glass(seed: int = 1, dims=(1024, 256, 32), n_houses: int = 60, n_facades: int = 40) -> np.ndarray:
    """S-glass: S-proc plus glass that stacks along a view ray (the
    single-layer deviation): hollow glass pavilions (a one-voxel glass shell
    around air: a ray crosses the front pane, then the inside of the back pane,
    both front-facing glass faces) and glass screens standing off two facades of
    a building.  Deterministic in ``seed``."""
    X, Y, Z = dims
    g = s_proc(seed, dims)
    rng = np.random.default_rng(seed + 1000)
    for _ in range(n_houses):                  # hollow glass pavilions on the ground
        w = int(rng.integers(6, 24)); d = int(rng.integers(6, 24)); hgt = int(rng.integers(4, min(16, Z - 2)))
        x0 = int(rng.integers(0, X - w)); y0 = int(rng.integers(0, Y - d))
        g[1:1 + hgt, y0:y0 + d, x0:x0 + w] = GLASS
        g[1:hgt, y0 + 1:y0 + d - 1, x0 + 1:x0 + w - 1] = 0          # open inside, glass roof kept
    for _ in range(n_facades):                 # a building with glass screens off two facades
        w = int(rng.integers(8, 30)); d = int(rng.integers(8, 30)); hgt = int(rng.integers(6, min(24, Z - 1)))
        x0 = int(rng.integers(4, X - w - 4)); y0 = int(rng.integers(4, Y - d - 4))
        col = int(rng.integers(1, 21))
        g[1:1 + hgt, y0:y0 + d, x0:x0 + w] = col
        off = int(rng.integers(2, 4))
        g[1:1 + hgt, y0 - off, x0:x0 + w] = GLASS                  # screen in front of the -y facade
        g[1:1 + hgt, y0:y0 + d, x0 + w - 1 + off] = GLASS          # and of the +x facade
    return g


def ref_boxes(seed: int = 7, dims=(1024, 256, 32), n_boxes: int = 40) -> np.ndarray:
    """Pinned map `boxes`: 40 seeded random boxes in empty space, no ground (so marches leave through
    z = 0 too), at the generator's fixed size; every colour 1..20 and glass occurs."""
    X, Y, Z = dims
    rng = np.random.default_rng(seed)
    g = np.zeros((Z, Y, X), np.uint8)
    for k in range(n_boxes):
        w, d, h = int(rng.integers(3, 40)), int(rng.integers(3, 40)), int(rng.integers(1, 20))
        x0, y0, z0 = int(rng.integers(0, X - w)), int(rng.integers(0, Y - d)), int(rng.integers(0, Z - h))
        g[z0:z0 + h, y0:y0 + d, x0:x0 + w] = 1 + k % 21
    return g


def ref_edges(dims=(1024, 256, 32)):
    """Pinned map `edges`: what a random map does not reach in the generator (sdf.cpp).  Returns (grid,
    overwrites); overwrites lists (x, y, z, colour) lines a map.txt carries before the grid's own line for
    that cell (the last write wins, the palette keeps the overwritten colour), each under a taller block of
    its column or at z = 0, where the 2D rule (sdf.cpp:201) does not see it.

    - the 8 corners of the grid hold blocks; the low one is a 3-cube around an air shaft at cell (0, 0, .),
      which is the one cell where the field's gradient rule is off (x + y + z > 0, sdf.cpp:440);
    - full columns on the faces x = 0, x = X - 1, y = 0, y = Y - 1;
    - a slab in the top layer with air under it, a block in layer 0 only (a column whose top block is at
      z = 0), single voxels in the bottom, a middle and the top layer;
    - faces lying on chunk planes (x = 64, y = 32) from either side in one colour, and boxes across them;
    - a floorless hollow box: inside, the downward radius is cut by max = z (sdf.cpp:437);
    - glass panes, two of them parallel."""
    X, Y, Z = dims
    g = np.zeros((Z, Y, X), np.uint8)
    for k, (cx, cy, cz) in enumerate((a, b, c) for c in (0, 1) for b in (0, 1) for a in (0, 1)):
        xs = slice(X - 2, X) if cx else slice(0, 2)
        ys = slice(Y - 2, Y) if cy else slice(0, 2)
        zs = slice(Z - 2, Z) if cz else slice(0, 2)
        g[zs, ys, xs] = 1 + k
    g[0:3, 0:3, 0:3] = 1
    g[0:3, 0, 0] = 0                               # the air shaft in the low corner
    g[:, 100, 0] = 9
    g[:, 150, X - 1] = 10
    g[:, 0, 300] = 11
    g[:, Y - 1, 700] = 12
    g[Z - 1, 40:80, 200:260] = 13                  # a slab in the top layer, air under it
    g[0, 120:124, 500:504] = 14                    # a block in layer 0 only
    g[0, 10, 900] = 15                             # single voxels
    g[5, 200, 600] = 16
    g[Z - 1, 128, 512] = 17
    g[1:6, 40:50, 58:64] = 5                       # +x face on the chunk plane x = 64
    g[1:6, 52:60, 64:70] = 5                       # -x face on it, the same colour
    g[1:5, 26:32, 100:110] = 6                     # +y face on the chunk plane y = 32
    g[1:5, 32:38, 112:120] = 6                     # -y face on it
    g[1:4, 60:68, 90:100] = 7                      # across y = 64
    g[2:9, 140:150, 120:136] = 18                  # across x = 128
    g[0:12, 180:220, 300:340] = 19                 # a hollow box without a floor
    g[0:11, 181:219, 301:339] = 0
    g[1:10, 90, 400:420] = GLASS                   # two parallel panes
    g[1:10, 94, 400:420] = GLASS
    g[2:8, 100:115, 450] = GLASS
    g[0:20, 230:234, 800:804] = 20                 # a tall block: the overwritten cells lie under its top
    overwrites = [(800, 230, 3, 4), (801, 231, 7, GLASS), (500, 120, 0, 2), (0, 100, 0, 16)]
    return g, overwrites


def single_block(dims=(64, 32, 16), at=(20, 12, 1), color=5) -> np.ndarray:
    X, Y, Z = dims
    g = np.zeros((Z, Y, X), np.uint8)
    g[0] = 2
    x, y, z = at
    g[z, y, x] = color
    return g


def glass_wall(dims=(64, 64, 16)) -> np.ndarray:
    """A glass wall (x = 36) over a ground plane with a white block behind it:
    looking up through the wall toward the sun (hour 1.0), the panes blend over
    cloudy sky next to the sun disc whose red exceeds 1 (render.frag:193,202:
    clouds mix toward sunCol.r = 1.4) and, with REFLECT, mirror it at grazing
    angles -- the case where the GL blend stage's clamps and 8-bit destination
    (render.js:84-86, map.js:7) decide the pixel (tests/golden 'blend_bright')."""
    X, Y, Z = dims
    g = np.zeros((Z, Y, X), np.uint8)
    g[0] = 2
    g[1:Z - 1, 4:Y - 4, 36] = GLASS
    g[1:6, 10:20, 50:56] = 20
    return g


def small_proc(seed: int, dims=(96, 48, 16), n_boxes=12, n_glass=3) -> np.ndarray:
    """A small S-proc-like scene that the scalar oracle renders in seconds."""
    return s_proc(seed, dims, n_boxes=n_boxes, n_glass=n_glass)


def odd_proc(seed: int, dims, n_boxes: int = 10, n_glass: int = 6) -> np.ndarray:
    """A scene for any X, Y, Z >= 1 (s_proc's ranges go empty below 9 x 9 x 5),
    with blocks on the far faces of the grid, where a kernel's partial blocks
    and mirrored coordinates end: ground at z = 0 (with holes and a second
    colour when Z = 1, where nothing else can stand); boxes sized relative to
    the dims, in turn flush with x = X - 1, with y = Y - 1, up to z = Z - 1 and
    anywhere; a block column at (0, 0) and one at (X - 1, Y - 1) up to z = Z - 1;
    when Z >= 5 overhang slabs over the four corners, the far one in the top
    layer, with air beneath;
    one-voxel glass panes, standing where Z >= 2, lying in the ground layer
    where Z = 1.  Deterministic in ``seed``."""
    X, Y, Z = (int(v) for v in dims)
    assert X >= 1 and Y >= 1 and Z >= 1, dims
    rng = np.random.default_rng(seed)
    g = np.zeros((Z, Y, X), np.uint8)
    g[0] = 2

    def span(n, lo, hi):
        """(start, length) of a run of lo..hi cells (clipped to n) inside [0, n)."""
        length = int(rng.integers(min(lo, n), min(hi, n) + 1))
        return int(rng.integers(0, n - length + 1)), length

    if Z == 1:
        # the top of a one-layer field is the grid's face, which shows nothing:
        # what a frame sees are the walls of the holes
        for k in range(max(6, X * Y // 8)):
            x0, w = span(X, 1, max(1, X // 12))
            y0, d = span(Y, 1, max(1, Y // 12))
            g[0, y0:y0 + d, x0:x0 + w] = 13 if k % 3 == 0 else 0
    else:
        for k in range(n_boxes):
            x0, w = span(X, 1, max(2, X // 4))
            y0, d = span(Y, 1, max(2, Y // 4))
            hgt = int(rng.integers(1, Z))              # 1 .. Z - 1 layers above the ground
            col = int(rng.integers(1, 21))
            if k % 4 == 0:
                x0 = X - w
            elif k % 4 == 1:
                y0 = Y - d
            elif k % 4 == 2:
                hgt = Z - 1
            g[1:1 + hgt, y0:y0 + d, x0:x0 + w] = col
    if Z >= 5:
        # overhang slabs over the four corners, air beneath: a sun of either sign on x and on
        # y finds cells whose rays all end in a slab (what a doom table marks) next to the grid
        # face its coordinates are mirrored from; the far one in the top layer, each wide
        # enough for a sun slope of about 1
        w, d = max(4, X // 3), max(4, Y // 3)
        for far_x, far_y, z in ((1, 1, Z - 1), (0, 1, Z - 2), (1, 0, Z - 3), (0, 0, Z - 2)):
            xs = slice(max(0, X - w), X) if far_x else slice(0, w)
            ys = slice(max(0, Y - d), Y) if far_y else slice(0, d)
            g[z, ys, xs] = int(rng.integers(1, 21))
    for k in range(n_glass):
        x0, lx = span(X, 1, max(2, X // 3))
        y0, ly = span(Y, 1, max(2, Y // 3))
        hgt = int(rng.integers(1, Z)) if Z >= 2 else 0
        z0, z1 = (1, 1 + hgt) if Z >= 2 else (0, 1)
        if k % 2 == 0:
            g[z0:z1, y0, x0:x0 + lx] = GLASS
        else:
            g[z0:z1, y0:y0 + ly, x0] = GLASS
    g[:, 0, 0] = 7
    g[:, Y - 1, X - 1] = 9
    return g
