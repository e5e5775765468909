"""The reference's own programs as a yardstick — TEST INFRASTRUCTURE ONLY.

Where a reference tree is present, oracle/Makefile's `ref` targets compile two
things into oracle/_ref/ (never committed):

* ``sdf_ref``: the map generator (src/gen/sdf.cpp) as it stands, against the
  serial parallel_for of oracle/ref/tbb.  It reads maps/map.txt and writes
  out/{map,vertex,vertex2d}.bin at its fixed 1024 x 256 x 32, CHUNK 32.
* ``libvxref_frag.so``: the fragment shader (src/shaders/render.frag, and
  render.vert for palette() and normal()) compiled as C++ through
  oracle/ref/glsl_shim.h, whose built-ins are written from DESIGN.md §5.

This module binds both: ``Frag`` runs march() and main() over batches,
``sdf_outputs`` runs the generator on a pinned map.  What they return is
recorded under tests/golden/ (tests/golden/make_ref_golden.py), so the tests
hold the oracle and the kernels to it with or without the tree.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
REF_DIR = os.path.join(_HERE, "_ref")
FRAG_LIB = os.path.join(REF_DIR, "libvxref_frag.so")
SDF_BIN = os.path.join(REF_DIR, "sdf_ref")
REF_TREE = os.environ.get("REF", "/root/reference")        # oracle/Makefile's REF
DIMS = (1024, 256, 32)                   # voxmap.h:6-8, render.h:14-16
CHUNK = 32                               # voxmap.h:9
GLASS = 21
GLASS_RGB = 8505300                      # sdf.cpp:17; :195 adds 0x1000000, so it sorts last
PINNED_MAPS = ("boxes", "edges")
SKY_BYTES = 5 * 6 * 16                   # the five skybox quads (sdf.cpp:247-279)

REC = np.dtype([("p", "<i2", 3), ("d", "<i2", 3), ("c", "u1"), ("n", "u1"), ("id", "u1"), ("pad", "u1")])


def available() -> bool:
    return os.path.exists(FRAG_LIB) and os.path.exists(SDF_BIN)


# ---- the compiled shader ----------------------------------------------------------------

_frag = None


def frag_lib():
    global _frag
    if _frag is None:
        L = C.CDLL(FRAG_LIB)
        ip, fp = C.POINTER(C.c_int), C.POINTER(C.c_float)
        L.vxref_constants.argtypes = [ip, fp]
        L.vxref_bind.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int]
        L.vxref_bind.restype = C.c_int
        L.vxref_uniforms.argtypes = [C.c_int, ip, fp, C.c_float, fp]
        L.vxref_march.argtypes = [C.c_int] + [C.c_void_p] * 8
        L.vxref_main.argtypes = [C.c_int] + [C.c_void_p] * 6
        L.vxref_palette.argtypes = [C.c_int, fp]
        L.vxref_normal.argtypes = [C.c_int, fp]
        for f in (L.vxref_constants, L.vxref_uniforms, L.vxref_march, L.vxref_main, L.vxref_palette, L.vxref_normal):
            f.restype = None
        _frag = L
    return _frag


def _i3(a):
    return np.ascontiguousarray(np.asarray(a, np.int32).reshape(-1, 3))


def _f3(a):
    return np.ascontiguousarray(np.asarray(a, np.float32).reshape(-1, 3))


class Frag:
    """The compiled shader over one field (Z, Y, X, 4) and one noise texture (H, W, 4).  The library keeps
    one binding and one set of uniforms: the latest Frag bound, the latest uniforms() set."""

    def __init__(self, field_zyx4, noise_hw4):
        self.field = np.ascontiguousarray(field_zyx4, np.uint8)
        self.noise = np.ascontiguousarray(noise_hw4, np.uint8)
        self.bind()

    def bind(self):
        Z, Y, X, _ = self.field.shape
        H, W, _ = self.noise.shape
        rc = frag_lib().vxref_bind(self.field.ctypes.data, X, Y, Z, self.noise.ctypes.data, W, H)
        if rc:
            raise ValueError(f"vxref_bind: {rc} (field {X} x {Y} x {Z}, noise {W} x {H})")

    def uniforms(self, quality, cam_cell, cam_fract, time, sun):
        frag_lib().vxref_uniforms(int(quality), (C.c_int * 3)(*[int(v) for v in cam_cell]),
                                  (C.c_float * 3)(*[float(v) for v in cam_fract]), float(time),
                                  (C.c_float * 3)(*[float(v) for v in sun]))

    def march(self, cell, fract, direction):
        """march() per row: a dict of cell (n, 3) int32, fract, normal (n, 3) float32, min_dist (n,), step (n,)."""
        c, f, d = _i3(cell), _f3(fract), _f3(direction)
        n = len(c)
        assert len(f) == n and len(d) == n
        out = {"cell": np.zeros((n, 3), np.int32), "fract": np.zeros((n, 3), np.float32),
               "normal": np.zeros((n, 3), np.float32), "min_dist": np.zeros(n, np.float32),
               "step": np.zeros(n, np.int32)}
        self.bind()
        frag_lib().vxref_march(n, c.ctypes.data, f.ctypes.data, d.ctypes.data, out["cell"].ctypes.data,
                               out["fract"].ctypes.data, out["normal"].ctypes.data, out["min_dist"].ctypes.data,
                               out["step"].ctypes.data)
        return out

    def main(self, cell, fract, color, normal_idx, frag_id):
        """main() per fragment under the uniforms set last: o_color (n, 4) float32."""
        c, f = _i3(cell), _f3(fract)
        col, nrm, fid = (np.ascontiguousarray(np.asarray(a, np.int32).reshape(-1)) for a in (color, normal_idx, frag_id))
        n = len(c)
        assert len(f) == n and len(col) == n and len(nrm) == n and len(fid) == n
        out = np.zeros((n, 4), np.float32)
        self.bind()
        frag_lib().vxref_main(n, c.ctypes.data, f.ctypes.data, col.ctypes.data, nrm.ctypes.data, fid.ctypes.data,
                              out.ctypes.data)
        return out


def constants():
    """The prelude's constants: {X, Y, Z, c_glass, MAX_STEPS} ints, {Xf, Yf, Zf} floats, Sf (3,) float32."""
    i, f = (C.c_int * 5)(), (C.c_float * 6)()
    frag_lib().vxref_constants(i, f)
    out = dict(zip(("X", "Y", "Z", "c_glass", "MAX_STEPS"), list(i)))
    out.update(zip(("Xf", "Yf", "Zf"), list(f)[:3]))
    out["Sf"] = np.array(list(f)[3:], np.float32)
    return out


def palette(p: int):
    out = (C.c_float * 3)()
    frag_lib().vxref_palette(int(p), out)
    return np.array(list(out), np.float32)


def normal(n: int):
    out = (C.c_float * 3)()
    frag_lib().vxref_normal(int(n), out)
    return np.array(list(out), np.float32)


# ---- the generator ------------------------------------------------------------------------

def colours():
    """21 colour values, index k - 1 for palette index k: 20 opaque ones in ascending order (the bytes of
    render.vert's palette, so the generator's sorted set numbers them 1..20) and glass, which sorts last."""
    from . import vxo_palette
    rgb = np.rint(vxo_palette()[1:21].astype(np.float64) * 255).astype(np.int64)
    out = [int(r) << 16 | int(g) << 8 | int(b) for r, g, b in rgb]
    assert out == sorted(set(out)) and GLASS_RGB not in out and len(out) == 20
    return out + [GLASS_RGB]


def write_map_txt(path, grid_zyx, overwrites=()):
    """A map.txt the generator reads back as ``grid_zyx`` (0 = air, 1..21): 3 header lines, then
    `x-512 y-5 z hex` per block (sdf.cpp:185-194).  Lines before the grid's own:

    - every colour once on the grid's first block, that block's own colour first, so that the palette holds
      all 21 (the indices are ranks in the set of colours met, sdf.cpp:196,216) and the 2D colour of that
      column, which only a first write above its top sets (sdf.cpp:201), is the block's;
    - ``overwrites``: (x, y, z, colour index) lines for cells the grid writes again with another colour."""
    g = np.asarray(grid_zyx)
    Z, Y, X = g.shape
    assert (X, Y, Z) == DIMS and g.max() <= GLASS
    col = colours()
    zs, ys, xs = np.nonzero(g)
    assert len(zs), "an empty map registers no colour"
    lines = ["# voxmap pinned map", "# x y z colour", "#"]
    z0, y0, x0 = int(zs[0]), int(ys[0]), int(xs[0])
    own = int(g[z0, y0, x0])
    for k in [own] + [k for k in range(1, 22) if k != own]:
        lines.append(f"{x0 - 512} {y0 - 5} {z0} {col[k - 1]:x}")
    for (x, y, z, k) in overwrites:
        assert g[z, y, x] not in (0, k), "an overwritten cell is a block of another colour"
        assert z == 0 or g[z + 1:, y, x].any(), "an overwritten cell lies under its column's top, or at z = 0"
        lines.append(f"{x - 512} {y - 5} {z} {col[k - 1]:x}")
    hexes = np.array([f"{c:x}" for c in col])
    for x, y, z, h in zip(xs - 512, ys - 5, zs, hexes[g[zs, ys, xs] - 1]):
        lines.append(f"{x} {y} {z} {h}")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def map_grid(name: str):
    """(grid, overwrites) of a pinned map."""
    from voxmap_amd import scenes
    if name == "boxes":
        return scenes.ref_boxes(), []
    if name == "edges":
        return scenes.ref_edges()
    raise KeyError(name)


def sdf_outputs(name: str):
    """(map.bin, vertex.bin, vertex2d.bin) paths of the generator's run on pinned map ``name``, run in
    oracle/_ref/maps/<name>/ when they are missing."""
    d = os.path.join(REF_DIR, "maps", name)
    outs = [os.path.join(d, "out", f) for f in ("map.bin", "vertex.bin", "vertex2d.bin")]
    if not (all(os.path.exists(p) for p in outs) and os.path.exists(os.path.join(d, "done"))):
        os.makedirs(os.path.join(d, "maps"), exist_ok=True)
        os.makedirs(os.path.join(d, "out"), exist_ok=True)
        grid, over = map_grid(name)
        write_map_txt(os.path.join(d, "maps", "map.txt"), grid, over)
        subprocess.run([SDF_BIN], cwd=d, check=True, stdout=subprocess.DEVNULL)
        open(os.path.join(d, "done"), "w").close()
    return tuple(outs)


def build_maps():
    """oracle.build()'s step after make: the generator's outputs for the pinned maps, where it was built."""
    if available():
        for name in PINNED_MAPS:
            sdf_outputs(name)


# ---- vertex.bin, read back ------------------------------------------------------------------

def skybox_bytes() -> bytes:
    """The first 480 bytes of every vertex.bin: the five skybox quads of sdf.cpp:247-279 (colour 0, normal
    1, id 1; origin, first and second edge), six vert() records each in the odd-normal winding (:112-114)."""
    X, Y, _ = DIMS
    quads = [((0, 0, Y), (X, 0, 0), (0, Y, 0)), ((0, 0, 0), (X, 0, 0), (0, 0, Y)), ((X, 0, 0), (0, Y, 0), (0, 0, Y)),
             ((X, Y, 0), (-X, 0, 0), (0, 0, Y)), ((0, Y, 0), (0, -Y, 0), (0, 0, Y))]
    rec = np.zeros(30, REC)
    for q, (p, a, b) in enumerate(quads):
        a, b = np.array(a), np.array(b)
        rec["p"][6 * q:6 * q + 6] = p
        rec["d"][6 * q:6 * q + 6] = [0 * a, b, a, b, a + b, a]
    rec["n"], rec["id"] = 1, 1
    return rec.tobytes()


def quads_of_vertex_bin(raw: bytes) -> np.ndarray:
    """The quads after the skybox as (n, 9) int32 rows x, y, z, w, h, colour, normal index, id, and the
    quad's number in the file; w along u = (d + 1) % 3 and h along v = (d + 2) % 3 of its axis d.  Checks
    the record layout of every quad (vert(), tri(), quad() of sdf.cpp:94-141)."""
    rec = np.frombuffer(raw[SKY_BYTES:], REC).reshape(-1, 6)
    p, d = rec["p"].astype(np.int32), rec["d"].astype(np.int32)
    n = rec["n"][:, 0].astype(np.int32)
    ax = n // 2
    u, v = (ax + 1) % 3, (ax + 2) % 3
    ext = d.max(axis=1)
    rows = np.arange(len(rec))
    w, h = ext[rows, u], ext[rows, v]
    for name in ("p", "c", "n", "id", "pad"):
        if not (rec[name] == rec[name][:, :1]).all():
            raise AssertionError(f"vertex.bin: a quad's six records differ in {name}")
    if (ext[rows, ax] != 0).any() or (w < 1).any() or (h < 1).any() or (rec["pad"] != 0).any():
        raise AssertionError("vertex.bin: a quad is not a w x h rectangle in its plane")
    du, dv = np.zeros((len(rec), 3), np.int32), np.zeros((len(rec), 3), np.int32)
    du[rows, u], dv[rows, v] = w, h
    zero = np.zeros_like(du)
    even = np.stack([zero, du, dv, dv, du, du + dv], 1)
    odd = np.stack([zero, dv, du, dv, du + dv, du], 1)
    if not (d == np.where((n % 2 == 1)[:, None, None], odd, even)).all():
        raise AssertionError("vertex.bin: a quad's corner order is not quad()'s")
    return np.stack([p[:, 0, 0], p[:, 0, 1], p[:, 0, 2], w, h, rec["c"][:, 0], n, rec["id"][:, 0], rows], 1).astype(np.int32)


def expand_quads(quads: np.ndarray, dims=DIMS) -> np.ndarray:
    """(Z, Y, X, 6) uint16 in oracle.face_quads' form from quads_of_vertex_bin's rows: every quad covers
    w x h faces and stores du | dv << 8 at each face's cell and normal index; 0xFFFF where no quad covers.
    A face two quads cover must get one value from both (the chunk-plane repeats)."""
    X, Y, Z = dims
    out = np.full((Z, Y, X, 6), 0xFFFF, np.uint16)
    for x, y, z, w, h, _c, n, _id, _k in quads.tolist():
        d = n // 2
        u, v = (d + 1) % 3, (d + 2) % 3
        lo = [x, y, z]
        lo[d] -= 0 if n % 2 else 1              # even: the cell below the plane, facing +d; odd: the cell on it
        ext = [1, 1, 1]
        ext[u], ext[v] = w, h
        shape = [1, 1, 1]
        shape[u] = w
        val_u = np.arange(w, dtype=np.uint16).reshape(shape)
        shape = [1, 1, 1]
        shape[v] = h
        val = (val_u + (np.arange(h, dtype=np.uint16).reshape(shape) << 8)).transpose(2, 1, 0)      # (z, y, x)
        if min(lo) < 0 or lo[0] + ext[0] > X or lo[1] + ext[1] > Y or lo[2] + ext[2] > Z:
            raise AssertionError(f"quad {(x, y, z, w, h, n)} lies outside the grid")
        view = out[lo[2]:lo[2] + ext[2], lo[1]:lo[1] + ext[1], lo[0]:lo[0] + ext[0], n]
        if ((view != 0xFFFF) & (view != val)).any():
            raise AssertionError(f"quad {(x, y, z, w, h, n)} covers a face another quad covers differently")
        view[...] = val
    return out


def quad_keys(quads: np.ndarray, dims=DIMS, chunk=CHUNK) -> np.ndarray:
    """vxo_face_order's key of each quad's origin face (uint64), the oracle's glass draw order."""
    from . import lib
    X, Y, Z = dims
    keys = np.zeros(len(quads), np.uint64)
    L = lib()
    for i, (x, y, z, _w, _h, _c, n, _id, _k) in enumerate(quads.tolist()):
        cell = [x, y, z]
        cell[n // 2] -= 0 if n % 2 else 1
        keys[i] = L.vxo_face_order((C.c_int * 3)(*cell), n, 0, X, Y, Z, chunk)
    return keys


# ---- the oracle's march and shade over a bare scene ---------------------------------------------

class BareScene:
    """An oracle scene of a field and a noise texture only: what vxo_march and vxo_shade read.  No traversal
    boxes, quad table or 2D footprint, so it costs nothing to set up; vxo_primary must not be called on it."""

    def __init__(self, field_zyx4, noise_hw4):
        from . import OScene
        self.field = np.ascontiguousarray(field_zyx4, np.uint8)
        self.noise = np.ascontiguousarray(noise_hw4, np.uint8)
        Z, Y, X, _ = self.field.shape
        H, W, _ = self.noise.shape
        self.sc = OScene(X, Y, Z, self.field.ctypes.data, self.noise.ctypes.data, W, H)

    def march(self, cell, fract, direction, max_steps):
        """vxo_march per row, in Frag.march's form."""
        from . import OMarch, lib
        c, f, d = _i3(cell), _f3(fract), _f3(direction)
        n = len(c)
        out = {"cell": np.zeros((n, 3), np.int32), "fract": np.zeros((n, 3), np.float32),
               "normal": np.zeros((n, 3), np.float32), "min_dist": np.zeros(n, np.float32),
               "step": np.zeros(n, np.int32)}
        L, m = lib(), OMarch()
        ip, fp = C.POINTER(C.c_int), C.POINTER(C.c_float)
        for i in range(n):
            L.vxo_march(C.byref(self.sc), c[i].ctypes.data_as(ip), f[i].ctypes.data_as(fp), d[i].ctypes.data_as(fp),
                        int(max_steps), C.byref(m))
            out["cell"][i], out["fract"][i], out["normal"][i] = m.cell[:], m.fract[:], m.normal[:]
            out["min_dist"][i], out["step"][i] = m.min_dist, m.step
        return out

    def shade(self, params, cell, fract, color, normal_idx, frag_id, prim_dir=None):
        """vxo_shade per fragment under the frame ``params``; sky fragments (id 1) take their direction from
        prim_dir's row (default: their fract, which is where a recorded sky fragment keeps it)."""
        from . import OGbuf, lib
        c, f = _i3(cell), _f3(fract)
        pd = f if prim_dir is None else _f3(prim_dir)
        n = len(c)
        out = np.zeros((n, 4), np.float32)
        L, g = lib(), OGbuf()
        fp = C.POINTER(C.c_float)
        for i in range(n):
            g.id, g.color, g.normal_idx = int(frag_id[i]), int(color[i]), int(normal_idx[i])
            g.cell[:] = c[i].tolist()
            g.fract[:] = f[i].tolist()
            L.vxo_shade(C.byref(self.sc), C.addressof(params), C.byref(g), pd[i].ctypes.data_as(fp),
                        out[i].ctypes.data_as(fp), None)
        return out


# ---- the recorded cases: three hand-filled cameras over S-proc ------------------------------

SUN_A = (0.35, 0.25, 0.9)
UNIT_GBUF = 0x800                        # include/voxmap.h VX_FLAG_UNIT_GBUF
FRAME_W, FRAME_H = 96, 64
# name -> (camera cell, elevation, azimuth); cam_fract = (0, 0, 0), so a sky fragment's v_fractPos = the
# pixel's direction makes render.frag:154 normalise exactly that direction
CAMERAS = {"down": ((381, 128, 40), -0.9, 0.3), "level": ((381, 128, 12), -0.15, 0.3), "edge": ((-20, 128, 20), -0.3, 0.0)}
# for main() fragments only: from outside y = 0 along +y just above the horizon, where the sky's mountain
# branch (render.frag:199) lies: its height falls off with (x / y)^2 and needs y > 0
SKY_CAMERAS = {"north": ((381, -20, 20), 0.12, 1.5707963267948966)}


def hand_frame(name, w=FRAME_W, h=FRAME_H, quality=1, time=12.5, sun=SUN_A, flags=UNIT_GBUF):
    """A vx.Frame filled by hand: fwd = (cos el cos az, cos el sin az, sin el), right = tan 30 * w / h *
    (-sin az, cos az, 0), up = tan 30 * (right^ x fwd), in float64 and rounded once to float32."""
    import math

    import voxmap_amd as vx
    cell, el, az = CAMERAS[name] if name in CAMERAS else SKY_CAMERAS[name]
    fwd = np.array([math.cos(el) * math.cos(az), math.cos(el) * math.sin(az), math.sin(el)])
    rhat = np.array([-math.sin(az), math.cos(az), 0.0])
    t = math.tan(math.radians(30.0))
    right, up = t * w / h * rhat, t * np.cross(rhat, fwd)
    p = vx.FrameParams()
    p.quality, p.frame, p.time, p.flags = int(quality), 0, float(time), int(flags)
    for i in range(3):
        p.cam_cell[i], p.cam_fract[i], p.sun_dir[i] = int(cell[i]), 0.0, float(sun[i])
        p.ray_fwd[i], p.ray_right[i], p.ray_up[i] = float(fwd[i]), float(right[i]), float(up[i])
    return vx.Frame(p, int(w), int(h))


def face_test(normal_idx, sun):
    """render.frag:228-232 for an axis normal: does the fragment march?  float32; the dot of an axis normal
    with the sun is +- one sun component exactly."""
    n = np.asarray(normal_idx)
    s = np.asarray(sun, np.float32).reshape(-1, 3)
    along = np.where(n % 2 == 0, 1, -1).astype(np.float32) * s[np.arange(len(n)) if len(s) > 1 else 0, n // 2]
    return ~(s[..., 2] < np.float32(0)) & (along > np.float32(0))
