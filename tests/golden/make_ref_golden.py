"""Regenerate the fixtures recorded from the reference's own programs (oracle/refpin.py):

  ref_sdf.json                  per pinned map (scenes.ref_boxes, scenes.ref_edges): SHA-256 and size of the
                                generator's map.bin, vertex.bin and vertex2d.bin
  ref_<map>_vertex.bin.gz,      the two mesh files themselves (map.bin is 32 MiB; its hash pins it)
  ref_<map>_vertex2d.bin.gz
  ref_frag.npz                  inputs and outputs of the compiled fragment shader: march() over points x the 41
                                suns of tests/test_sun_query_gpu.py::sun_set on two fields, and main() over
                                fragments (uniform sets x records of the oracle's primary visibility)
  ref_frames.npz                three 96 x 64 frames assembled from main() over the oracle's UNIT_GBUF records

Only data the programs read or wrote is stored: no text of theirs.  Needs the reference tree, i.e. oracle/_ref
built by `make -C oracle`; refuses to run without it.  Run from the repo root:
  python tests/golden/make_ref_golden.py
"""
import gzip
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

import oracle  # noqa: E402
import voxmap_amd as vx  # noqa: E402
from oracle import refpin  # noqa: E402
from voxmap_amd import presets, scenes  # noqa: E402

MAX_STEPS = 64
SUN_LOW = (0.35, 0.25, -0.9)             # below the horizon: no fragment marches
SUN_ZERO = (0.6, 0.0, 0.8)               # a zero component: march()'s 0 * inf
FRAG_FIELDS = ("s_proc", "s_glass")
MARCH_FIELDS = ("s_proc", "edges")

_fields = {}


def field(name):
    if name not in _fields:
        grid = refpin.map_grid(name)[0] if name in refpin.PINNED_MAPS else presets.scene_grid(name)
        _fields[name] = vx.field_build(grid)
    return _fields[name]


def suns41():
    from test_sun_query_gpu import sun_set
    return sun_set()


# ---- march cases --------------------------------------------------------------------------------

def edge_fracts(cells):
    """The edge fracts of tests/test_sun_query_gpu.py over the given cells: 0, 1 - ulp, -2^-24, -1 and 2 - ulp
    on each axis in turn and on all three."""
    one = np.float32(1)
    vals = [np.float32(0), np.nextafter(one, np.float32(0)), np.float32(-2.0 ** -24), np.float32(-1),
            np.nextafter(np.float32(2), np.float32(0))]
    rng = np.random.default_rng(77)
    out_c, out_f = [], []
    for k in range(4 * len(vals)):
        f = rng.random(3, dtype=np.float32)
        v, a = vals[k // 4], k % 4
        if a == 3:
            f[:] = v
        else:
            f[a] = v
        out_c.append(cells[k % len(cells)])
        out_f.append(f)
    return np.array(out_c, np.int32), np.array(out_f, np.float32)


def march_points(name, orc):
    """(cell, fract) of a field's march points: first records of pixel rays (unit split), ground points,
    seeded random cells, the edge fracts; on `edges` the cells the random map does not reach."""
    X, Y, Z = refpin.DIMS
    rng = np.random.default_rng(2025)
    cells, fracts = [], []
    if name == "s_proc":
        for cam in refpin.CAMERAS:
            fr = refpin.hand_frame(cam)
            got = 0
            for py in range(2, 64, 7):
                for px in range(3, 96, 11):
                    n, g, _, _ = orc.primary(fr.params, orc.pixel_dir(fr.params, 96, 64, px, py))
                    if n >= 1 and got < 10:
                        cells.append(list(g[0].cell)); fracts.append(list(g[0].fract)); got += 1
        gp, _ = vx.ground_points(field(name))
        pick = gp[rng.choice(len(gp), 14, replace=False)]
        cells += pick["cell"].tolist(); fracts += pick["fract"].tolist()
    else:
        special = [(0, 0, 0), (0, 0, 1), (0, 0, 2), (0, 0, 5), (0, 0, Z - 1), (1, 3, 1), (3, 1, 0), (X - 1, Y - 1, 5),
                   (X - 3, Y - 3, Z - 3), (X - 1, 0, 10), (0, Y - 1, 10), (320, 200, 5), (320, 200, 0), (310, 190, 10),
                   (230, 60, Z - 2), (230, 60, 3), (410, 92, 4), (410, 91, 4), (410, 95, 4), (512, 128, Z - 2),
                   (61, 45, 6), (64, 50, 3), (105, 32, 2), (802, 232, 20), (502, 122, 1), (1, 100, 7)]
        cells += [list(c) for c in special]
        fracts += rng.random((len(special), 3), dtype=np.float32).tolist()
    rnd = np.stack([rng.integers(0, d, 14) for d in (X, Y, Z)], 1)
    cells += rnd.tolist(); fracts += rng.random((14, 3), dtype=np.float32).tolist()
    corner = [(0, 0, 0), (X - 1, Y - 1, Z - 1), (0, 0, Z - 1), (X - 1, 0, 0)] + rnd[:4].tolist()
    ec, ef = edge_fracts(corner)
    return np.concatenate([np.array(cells, np.int32), ec]), np.concatenate([np.array(fracts, np.float32), ef])


# ---- main() fragments -----------------------------------------------------------------------------

def records_of(orc, fr, pixels, sky):
    """The oracle's primary records of the given pixels as fragment rows; sky pixels (no record, or the record
    behind a pane) become the skybox fragment v_cellPos = u_cellPos, v_fractPos = the pixel's direction where
    ``sky`` (cam_fract must be 0 then), else are left out."""
    w, h = fr.width, fr.height
    rows = []
    for (px, py) in pixels:
        d = orc.pixel_dir(fr.params, w, h, px, py)
        n, g, _, cap = orc.primary(fr.params, d)
        assert not cap
        recs = [g[k] for k in range(n)] or [None]
        for r in recs:
            if r is None or r.id == 1:
                if sky:
                    rows.append((list(fr.params.cam_cell), list(d), 0, 1, 1))
            else:
                rows.append((list(r.cell), list(r.fract), r.color, r.normal_idx, r.id))
    return rows


def run_set(fragq, orc, fr, pixels, sky, field_name):
    rows = records_of(orc, fr, pixels, sky)
    p = fr.params
    uni = dict(field=FRAG_FIELDS.index(field_name), quality=p.quality, cell=list(p.cam_cell), fract=list(p.cam_fract),
               time=p.time, sun=list(p.sun_dir))
    cell = np.array([r[0] for r in rows], np.int32)
    fract = np.array([r[1] for r in rows], np.float32)
    col, nrm, fid = (np.array([r[k] for r in rows], np.int32) for k in (2, 3, 4))
    fragq.uniforms(p.quality, uni["cell"], uni["fract"], p.time, uni["sun"])
    out = fragq.main(cell, fract, col, nrm, fid)
    # the reference's own sun march per block fragment that passes the face test (-1: none), and the sky
    # branch: only the cloud branch of render.frag:199-203 reads u_time
    step = np.full(len(rows), -1, np.int32)
    marching = (fid != 1) & refpin.face_test(nrm, uni["sun"])
    if marching.any():
        step[marching] = fragq.march(cell[marching], fract[marching], np.tile(np.float32(uni["sun"]), (int(marching.sum()), 1)))["step"]
    mountain = np.zeros(len(rows), bool)
    s = fid == 1
    if s.any():
        fragq.uniforms(p.quality, uni["cell"], uni["fract"], p.time + 321.0, uni["sun"])
        other = fragq.main(cell[s], fract[s], col[s], nrm[s], fid[s])
        mountain[s] = (other.view(np.uint32) == out[s].view(np.uint32)).all(axis=1)
    return uni, dict(cell=cell, fract=fract, color=col, normal=nrm, id=fid, out=out, step=step, mountain=mountain)


def grid_pixels(w, h, sx, sy, ox=0, oy=0):
    return [(px, py) for py in range(oy, h, sy) for px in range(ox, w, sx)]


def main():
    if not refpin.available():
        sys.exit("oracle/_ref is not built: the fixtures are recorded from the reference's own programs")
    oracle.build()
    noise = scenes.real_noise()
    os.chdir(HERE)

    # ---- the generator's outputs
    sdf = {}
    for name in refpin.PINNED_MAPS:
        paths = refpin.sdf_outputs(name)
        raw = [open(p, "rb").read() for p in paths]
        sdf[name] = {k: {"sha256": hashlib.sha256(b).hexdigest(), "bytes": len(b)}
                     for k, b in zip(("map.bin", "vertex.bin", "vertex2d.bin"), raw)}
        for k, b in zip(("vertex", "vertex2d"), raw[1:]):
            with open(f"ref_{name}_{k}.bin.gz", "wb") as f:
                f.write(gzip.compress(b, 9, mtime=0))
    with open("ref_sdf.json", "w") as f:
        json.dump(sdf, f, indent=1, sort_keys=True)
        f.write("\n")

    # ---- the shader
    orcs = {n: oracle.Oracle(field(n), noise, chunk=refpin.CHUNK) for n in FRAG_FIELDS}
    frags = {n: refpin.Frag(field(n), noise) for n in set(FRAG_FIELDS + MARCH_FIELDS)}
    suns = suns41()
    store = {"suns": suns}
    for name in MARCH_FIELDS:
        cell, fract = march_points(name, orcs.get(name))
        P, K = len(cell), len(suns)
        res = frags[name].march(np.repeat(cell, K, 0), np.repeat(fract, K, 0), np.tile(suns, (P, 1)))
        store[f"march_{name}_cell"], store[f"march_{name}_fract"] = cell, fract
        for k, v in res.items():
            store[f"march_{name}_o_{k}"] = v.reshape((P, K) + v.shape[1:])
        print(f"march {name}: {P} points x {K} suns")

    sets, parts = [], []

    def add(field_name, fr, pixels, sky):
        uni, part = run_set(frags[field_name], orcs[field_name], fr, pixels, sky, field_name)
        part["set"] = np.full(len(part["id"]), len(sets), np.int32)
        sets.append(uni)
        parts.append(part)

    Q = 0                                 # the quad split: no UNIT_GBUF flag
    for cam in refpin.CAMERAS:
        add("s_proc", refpin.hand_frame(cam), grid_pixels(96, 64, 3, 2), True)
        add("s_proc", refpin.hand_frame(cam, time=0.0, flags=Q), grid_pixels(96, 64, 5, 4, 1, 1), True)
    add("s_proc", refpin.hand_frame("edge", quality=0, time=999.0), grid_pixels(96, 64, 4, 3, 2, 1), True)
    add("s_proc", refpin.hand_frame("level", sun=SUN_LOW), grid_pixels(96, 64, 4, 3, 1, 2), True)
    add("s_proc", refpin.hand_frame("down", sun=SUN_ZERO), grid_pixels(96, 64, 4, 3, 3, 0), True)
    add("s_glass", refpin.hand_frame("down", time=999.0), grid_pixels(96, 64, 4, 3), True)
    add("s_proc", refpin.hand_frame("north"), grid_pixels(96, 64, 3, 2), True)
    add("s_proc", refpin.hand_frame("north", time=999.0, sun=SUN_ZERO), grid_pixels(96, 64, 5, 3, 2, 1), True)
    for cam in ("K0", "K1", "K2"):
        for flags in (refpin.UNIT_GBUF, Q):
            add("s_glass", presets.camera_frame(cam, 64, 40, time=12.5, sun=refpin.SUN_A, flags=flags),
                grid_pixels(64, 40, 2, 1, 1 if flags else 0), False)
        add("s_proc", presets.camera_frame(cam, 48, 30, flags=refpin.UNIT_GBUF), grid_pixels(48, 30, 2, 2), False)
    for k in ("quality", "field"):
        store[f"set_{k}"] = np.array([u[k] for u in sets], np.int32)
    store["set_cell"] = np.array([u["cell"] for u in sets], np.int32)
    for k in ("fract", "sun"):
        store[f"set_{k}"] = np.array([u[k] for u in sets], np.float32)
    store["set_time"] = np.array([u["time"] for u in sets], np.float32)
    for k in parts[0]:
        store[f"frag_{k}"] = np.concatenate([p[k] for p in parts])
    np.savez_compressed("ref_frag.npz", **store)
    fid, step = store["frag_id"], store["frag_step"]
    print(f"main: {len(fid)} fragments in {len(sets)} sets: sky {int((fid == 1).sum())} (mountain "
          f"{int(store['frag_mountain'].sum())}), glass {int((fid == 2).sum())}, lit {int(((fid == 0) & (step == MAX_STEPS)).sum())}, "
          f"unlit {int(((fid == 0) & (step >= 0) & (step < MAX_STEPS)).sum())}, no march {int(((fid == 0) & (step < 0)).sum())}")

    # ---- the three frames
    frames = {}
    for cam in refpin.CAMERAS:
        fr = refpin.hand_frame(cam)
        orc, fq = orcs["s_proc"], frags["s_proc"]
        w, h = fr.width, fr.height
        n_rec = np.zeros((h, w), np.uint8)
        cell, fract = np.zeros((h, w, 3), np.int32), np.zeros((h, w, 3), np.float32)
        col, nrm, fid = (np.zeros((h, w), np.int32) for _ in range(3))
        for py in range(h):
            for px in range(w):
                d = orc.pixel_dir(fr.params, w, h, px, py)
                n, g, _, cap = orc.primary(fr.params, d)
                assert not cap
                n_rec[py, px] = n
                if n == 0:
                    cell[py, px], fract[py, px], col[py, px], nrm[py, px], fid[py, px] = list(fr.params.cam_cell), list(d), 0, 1, 1
                else:
                    r = g[0]
                    cell[py, px], fract[py, px] = list(r.cell), list(r.fract)
                    col[py, px], nrm[py, px], fid[py, px] = r.color, r.normal_idx, r.id
        p = fr.params
        fq.uniforms(p.quality, list(p.cam_cell), list(p.cam_fract), p.time, list(p.sun_dir))
        out = fq.main(cell.reshape(-1, 3), fract.reshape(-1, 3), col.reshape(-1), nrm.reshape(-1), fid.reshape(-1))
        step = np.full(w * h, -1, np.int32)
        m = (fid.reshape(-1) == 0) & refpin.face_test(nrm.reshape(-1), list(p.sun_dir))
        step[m] = fq.march(cell.reshape(-1, 3)[m], fract.reshape(-1, 3)[m], np.tile(np.float32(list(p.sun_dir)), (int(m.sum()), 1)))["step"]
        frames.update({f"{cam}_out": out.reshape(h, w, 4), f"{cam}_n": n_rec, f"{cam}_cell": cell, f"{cam}_fract": fract,
                       f"{cam}_color": col.astype(np.uint8), f"{cam}_normal": nrm.astype(np.uint8),
                       f"{cam}_id": fid.astype(np.uint8), f"{cam}_step": step.reshape(h, w).astype(np.int8)})
        blk = (n_rec == 1).reshape(-1)
        print(f"frame {cam}: sky {int((n_rec == 0).sum())}, lit {int((blk & (step == MAX_STEPS)).sum())}, unlit "
              f"{int((blk & (step >= 0) & (step < MAX_STEPS)).sum())}, no march {int((blk & (step < 0)).sum())}, glass "
              f"{int((n_rec == 2).sum())}")
    np.savez_compressed("ref_frames.npz", **frames)
    for f in sorted(os.listdir(".")):
        if f.startswith("ref_"):
            print(f"{os.path.getsize(f):9d} {f}")


if __name__ == "__main__":
    main()
