"""The field and mesh restatements against the reference's own map generator, compiled (oracle/refpin.py).

src/gen/sdf.cpp, built as it stands against a serial parallel_for, ran on two pinned maps (scenes.ref_boxes: 40
random boxes; scenes.ref_edges: the grid's borders, the x + y + z > 0 rule, the max = o ? z : Z cut, chunk planes,
doubly written cells, a column whose top is at z = 0, glass).  tests/golden/ holds what it wrote: the SHA-256 of
map.bin, and vertex.bin and vertex2d.bin themselves.  Held to them, by bytes:

* map.bin == oracle.field_build == vx.field_build (by hash; live, where oracle/_ref is built, by bytes too);
* vertex2d.bin == vx.vertex2d;
* vertex.bin: the five skybox quads, then quads whose per-face expansion == oracle.face_quads(field, 32), with no
  face where no quad covers, and whose order in the file ascends in vxo_face_order's key (the glass draw order).

mesh_ref.greedy_mesh is not run here: it takes over a minute at this size, and test_quad_gbuf.py holds it to
oracle.face_quads at small ones.
"""
import gzip
import hashlib
import json
import os

import numpy as np
import pytest

from gpu_rig import assert_blob_equal, assert_ints_equal

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
MAPS = ("boxes", "edges")


def sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()


@pytest.fixture(scope="module")
def recorded():
    """name -> {"sdf": the hashes, "vertex": bytes, "vertex2d": bytes}; the mesh files checked against their hashes."""
    meta = json.load(open(os.path.join(GOLD, "ref_sdf.json")))
    out = {}
    for name in MAPS:
        files = {k: gzip.decompress(open(os.path.join(GOLD, f"ref_{name}_{k}.bin.gz"), "rb").read())
                 for k in ("vertex", "vertex2d")}
        for k, b in files.items():
            assert len(b) == meta[name][k + ".bin"]["bytes"] and sha(b) == meta[name][k + ".bin"]["sha256"], (name, k)
        out[name] = dict(files, sdf=meta[name])
    return out


@pytest.fixture(scope="module")
def world(built):
    """name -> (grid, host field, parsed quads), made once per module."""
    import voxmap_amd as vx
    from oracle import refpin
    made = {}

    def get(name, recorded):
        if name not in made:
            grid = refpin.map_grid(name)[0]
            made[name] = (grid, vx.field_build(grid), refpin.quads_of_vertex_bin(recorded[name]["vertex"]))
        return made[name]
    return get


@pytest.mark.parametrize("name", MAPS)
def test_field_is_the_generators_map_bin(recorded, world, name):
    import oracle
    grid, field, _ = world(name, recorded)
    want = recorded[name]["sdf"]["map.bin"]
    assert field.nbytes == want["bytes"] == 4 * 1024 * 256 * 32
    assert sha(field.tobytes()) == want["sha256"]
    assert_ints_equal(oracle.field_build(grid), field, "oracle field bytes")


@pytest.mark.parametrize("name", MAPS)
def test_vertex2d_is_the_generators(recorded, world, name):
    import voxmap_amd as vx
    _, field, _ = world(name, recorded)
    assert_blob_equal(vx.vertex2d(field), recorded[name]["vertex2d"], "vertex2d.bin")


@pytest.mark.parametrize("name", MAPS)
def test_vertex_bin_expands_to_the_oracles_face_quads(recorded, world, name):
    import oracle
    from oracle import refpin
    _, field, quads = world(name, recorded)
    raw = recorded[name]["vertex"]
    assert_blob_equal(raw[:refpin.SKY_BYTES], refpin.skybox_bytes(), "the skybox quads")
    assert (len(raw) - refpin.SKY_BYTES) % 96 == 0 and len(quads) == (len(raw) - refpin.SKY_BYTES) // 96
    got = refpin.expand_quads(quads)
    ref = oracle.face_quads(field, refpin.CHUNK)
    assert_ints_equal(got == 0xFFFF, ref == 0xFFFF, "faces no quad covers")
    assert_ints_equal(got, ref, "face quads")
    # colour and id of every quad: the colour of the cell its faces belong to; id 2 for glass alone
    x, y, z, _w, _h, c, n, fid, _k = quads.T
    cell = np.stack([x, y, z], 1)
    cell[np.arange(len(quads)), n // 2] -= np.where(n % 2 == 1, 0, 1)
    assert_ints_equal(field[cell[:, 2], cell[:, 1], cell[:, 0], 2].astype(np.int32), c, "quad colours")
    assert_ints_equal(fid, np.where(c == refpin.GLASS, 2, 0).astype(np.int32), "quad ids")


@pytest.mark.parametrize("name", MAPS)
def test_file_order_is_the_oracles_draw_order(recorded, world, name):
    """Colour-major (sdf.cpp:284); within a colour ascending in vxo_face_order's key.  A quad on an interior chunk
    plane is written twice, by the chunk below (its last slice) and by the chunk above (its slice -1): the key is
    the first writer's, so the repeat is dropped before comparing."""
    from oracle import refpin
    _, _, quads = world(name, recorded)
    keys = refpin.quad_keys(quads)
    colour = quads[:, 5]
    assert (np.diff(colour) >= 0).all()
    ident = [tuple(q) for q in quads[:, :8].tolist()]
    first, repeats = {}, []
    for i, q in enumerate(ident):
        if q in first:
            repeats.append(i)
        else:
            first[q] = i
    rep = np.zeros(len(quads), bool)
    rep[repeats] = True
    n, plane = quads[:, 6], quads[np.arange(len(quads)), quads[:, 6] // 2]
    on_plane = (n // 2 < 2) & (plane % refpin.CHUNK == 0)
    # every quad on an interior chunk plane of x or y occurs twice, nothing else does
    assert_ints_equal(np.array([ident.count(q) for q in ident]) == 2, on_plane, "quads written twice")
    assert rep.sum() * 2 == on_plane.sum()
    for c in np.unique(colour):
        k = keys[(colour == c) & ~rep]
        assert (k[1:] > k[:-1]).all(), f"colour {c}: the file order is not the key order"
    if name == "edges":
        assert on_plane.sum() >= 8 and (colour[on_plane] == 5).any() and (colour[on_plane] == 6).any()
        assert (colour == refpin.GLASS).sum() >= 6


def test_edges_map_reaches_what_it_claims(recorded, world):
    """Read off the field the generator's rules produce, at the cells the map was built for."""
    from oracle import refpin
    grid, field, _ = world("edges", recorded)
    X, Y, Z = refpin.DIMS
    R, G, B = field[..., 0], field[..., 1], field[..., 2]
    assert grid[0, 0, 0] == 0 and B[0, 0, 0] == 22                        # the air shaft: cell (0, 0, 0) is air
    assert G[0, 0, 0] == 1 and R[0, 0, 0] == 1                            # its radii start from min = 1, no gradient rule
    for cz in (0, Z - 1):
        for cy in (0, Y - 1):
            for cx in (0, X - 1):
                assert (cx, cy, cz) == (0, 0, 0) or grid[cz, cy, cx] != 0
    assert grid[:, 100, 0].all() and grid[:, 150, X - 1].all() and grid[:, 0, 300].all() and grid[:, Y - 1, 700].all()
    assert grid[Z - 1, 60, 230] != 0 and not grid[:Z - 1, 60, 230].any()   # the slab, air under it
    assert grid[0, 121, 501] != 0 and not grid[1:, 121, 501].any()         # a column whose top is at z = 0
    # the floorless hollow: at z = 5 in its middle the walls are 18 cells away, the downward radius is cut at z
    assert G[5, 200, 320] == 5 and G[9, 200, 320] == 9 and R[0, 200, 320] > 5
    # the overwritten cells hold the last colour written
    _, over = refpin.map_grid("edges")
    for x, y, z, k in over:
        assert B[z, y, x] == grid[z, y, x] != k
    assert set(np.unique(refpin.map_grid("boxes")[0])) == set(range(22))


# ---- live: the program's files are the recorded ones ------------------------------------------------------

@pytest.mark.parametrize("name", MAPS)
def test_generator_writes_the_recorded_files(recorded, world, name):
    from oracle import refpin
    if not refpin.available():
        pytest.skip("no reference tree: oracle/_ref is not built")
    _, field, _ = world(name, recorded)
    mp, vp, v2p = refpin.sdf_outputs(name)
    assert_blob_equal(open(vp, "rb").read(), recorded[name]["vertex"], "vertex.bin")
    assert_blob_equal(open(v2p, "rb").read(), recorded[name]["vertex2d"], "vertex2d.bin")
    raw = open(mp, "rb").read()
    assert sha(raw) == recorded[name]["sdf"]["map.bin"]["sha256"]
    assert_blob_equal(field.tobytes(), raw, "map.bin")


# ---- the comparison fires ---------------------------------------------------------------------------------

def test_a_flipped_bit_is_seen(recorded, world):
    import oracle
    from oracle import refpin
    _, field, quads = world("edges", recorded)
    ref = oracle.face_quads(field, refpin.CHUNK)
    raw = bytearray(recorded["edges"]["vertex"])
    glass = int(np.flatnonzero(quads[:, 5] == refpin.GLASS)[0])
    # the x of a glass quad's six records, one cell on: layout intact, the faces move
    for v in range(6):
        raw[refpin.SKY_BYTES + 96 * glass + 16 * v] ^= 1
    moved = refpin.expand_quads(refpin.quads_of_vertex_bin(bytes(raw)))
    with pytest.raises(AssertionError, match="face quads differ"):
        assert_ints_equal(moved, ref, "face quads")
    # one record's corner offset alone: the layout check itself
    raw = bytearray(recorded["edges"]["vertex"])
    raw[refpin.SKY_BYTES + 96 * glass + 16 * 1 + 6] ^= 1
    with pytest.raises(AssertionError, match="vertex.bin"):
        refpin.quads_of_vertex_bin(bytes(raw))
    # a field bit: the hash
    f = field.copy()
    f[3, 7, 9, 1] ^= 1
    assert sha(f.tobytes()) != recorded["edges"]["sdf"]["map.bin"]["sha256"]
    with pytest.raises(AssertionError, match="1 field bytes differ"):
        assert_ints_equal(f, field, "field bytes")
    # two quads swapped in the file: the order check's comparison
    keys = refpin.quad_keys(quads)
    k = keys[quads[:, 5] == refpin.GLASS]
    assert (k[1:] > k[:-1]).all() and not (k[::-1][1:] > k[::-1][:-1]).all()
