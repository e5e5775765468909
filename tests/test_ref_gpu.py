"""The HIP kernels against what the reference's own programs wrote (tests/golden/ref_*, recorded by
tests/golden/make_ref_golden.py from the compiled map generator and fragment shader).

Reads tests/golden/ only, never a reference tree.  One scene per field, 1024 x 256 x 32 (the generator's size):

* field build: vx_field_build_gpu hashes to the generator's map.bin for both pinned maps;
* mesh: a FORMAT_GRID scene's face-quad table == the per-face expansion of the generator's vertex.bin, and its 2D
  mesh == the generator's vertex2d.bin;
* sun query: vx_query_sun's lit words == `step == MAX_STEPS` of the compiled march() over the recorded points and
  the 41 suns, with the exit tables and without (VX_SUNQ_NO_EXIT);
* frames: vx_render of three hand-filled 96 x 64 frames == the frames assembled from the compiled main(), word for
  word, and the device's own vx_query_rays records == the recorded varyings.

Kept out of the frame comparison by construction, not by tolerance: pixels whose ray crosses glass (their colour
goes through the blend stage, which is no shader text), listed by the recorded mask, at most 1 % of a frame; the
skybox at infinity (the cameras have cam_fract = 0, for which the recorded sky fragment normalises exactly the
pixel's direction); sampler LOD (LOD 0 on both sides).
"""
import gzip
import hashlib
import json
import os

import numpy as np
import pytest

from gpu_rig import (INT_INDEX, assert_blob_equal, assert_ints_equal, assert_no_cap_hits, assert_words_equal, bin_scene,
                     need_gpu, with_flags)  # noqa: F401 (need_gpu: an autouse fixture)

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
MAPS = ("boxes", "edges")
MAX_STEPS = 64
NO_EXIT = 0x1                         # include/voxmap.h VX_SUNQ_NO_EXIT


def load(name):
    with np.load(os.path.join(GOLD, name)) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def sdf():
    meta = json.load(open(os.path.join(GOLD, "ref_sdf.json")))
    for name in MAPS:
        for k in ("vertex", "vertex2d"):
            meta[name][k] = gzip.decompress(open(os.path.join(GOLD, f"ref_{name}_{k}.bin.gz"), "rb").read())
            assert hashlib.sha256(meta[name][k]).hexdigest() == meta[name][k + ".bin"]["sha256"]
    return meta


@pytest.fixture(scope="module")
def frag():
    return load("ref_frag.npz")


@pytest.fixture(scope="module")
def frames():
    return load("ref_frames.npz")


_scenes = {}


@pytest.fixture(scope="module")
def scene_of(noise):
    """name -> the module's one scene of that field: the pinned maps as FORMAT_GRID (field and mesh built on the
    device), S-proc as the host-built map.bin."""
    import voxmap_amd as vx
    from oracle import refpin
    from voxmap_amd import presets

    def get(name):
        if name not in _scenes:
            if name in MAPS:
                grid = refpin.map_grid(name)[0]
                _scenes[name] = vx.Scene(map_bytes=grid.tobytes(), map_format=vx.FORMAT_GRID, noise_bytes=noise.tobytes(),
                                         noise_format=vx.FORMAT_BIN, dims=refpin.DIMS, device=0, mesh_chunk=refpin.CHUNK)
            else:
                _scenes[name] = bin_scene(vx.field_build(presets.scene_grid(name)), noise, refpin.DIMS,
                                          mesh_chunk=refpin.CHUNK)
        return _scenes[name]
    yield get
    for s in _scenes.values():
        s.close()
    _scenes.clear()


@pytest.mark.parametrize("name", MAPS)
def test_device_field_build_hashes_to_the_generators_map_bin(sdf, name):
    import voxmap_amd as vx
    from oracle import refpin
    field = vx.field_build_gpu(refpin.map_grid(name)[0])
    assert field.nbytes == sdf[name]["map.bin"]["bytes"]
    assert hashlib.sha256(field.tobytes()).hexdigest() == sdf[name]["map.bin"]["sha256"]


@pytest.mark.parametrize("name", MAPS)
def test_scene_mesh_is_the_generators(sdf, scene_of, name):
    from oracle import refpin
    sc = scene_of(name)
    field = sc.read_field()
    field[..., 3] = 0                  # the copy's A byte is the octant's air-cube size (include/voxmap.h); map.bin's is 0
    assert hashlib.sha256(field.tobytes()).hexdigest() == sdf[name]["map.bin"]["sha256"]
    want = refpin.expand_quads(refpin.quads_of_vertex_bin(sdf[name]["vertex"]))
    got = sc.read_face_quads()
    assert_ints_equal(got == 0xFFFF, want == 0xFFFF, "faces no quad covers")
    assert_ints_equal(got, want, "face quads")
    assert_blob_equal(sc.vertex2d(), sdf[name]["vertex2d"], "vertex2d.bin")


@pytest.mark.parametrize("name", ["s_proc", "edges"])
def test_sun_query_is_the_compiled_march(frag, scene_of, name):
    import voxmap_amd as vx
    cell, fract, suns = frag[f"march_{name}_cell"], frag[f"march_{name}_fract"], frag["suns"]
    lit = frag[f"march_{name}_o_step"] == MAX_STEPS                       # (P, K)
    P, K = lit.shape
    assert K == 41 and P >= 50 and 0.1 < lit.mean() < 0.9
    want = np.zeros((P, vx.sun_words(K)), np.uint32)
    want[:, 0] = lit.sum(axis=1)
    for j in range(K):
        want[:, 1 + j // 32] |= lit[:, j].astype(np.uint32) << np.uint32(j % 32)
    pts = np.zeros(P, vx.SUN_POINT_DTYPE)
    pts["cell"], pts["fract"], pts["normal_idx"] = cell, fract, -1            # no face: every pair marches
    sc = scene_of(name)
    for flags in (0, NO_EXIT):
        got, st = sc.query_sun(pts, suns, max_steps=0, flags=flags, stats=True)
        assert st.invalid == 0 and st.culled == 0 and st.rays == P * K
        assert_ints_equal(got, want, f"{name} lit words, flags {flags}")


@pytest.mark.parametrize("cam", ["down", "level", "edge"])
def test_frames_are_the_compiled_shaders(frames, scene_of, cam):
    import voxmap_amd as vx
    from oracle import refpin
    sc = scene_of("s_proc")
    fr = refpin.hand_frame(cam)
    w, h = fr.width, fr.height
    ref, n_rec = frames[f"{cam}_out"], frames[f"{cam}_n"]
    glass = n_rec == 2
    assert glass.sum() <= 61                                   # at most 1 % of the frame left out
    assert not np.isnan(ref[~glass]).any()
    img, st = sc.render(fr, stats=True)
    assert_no_cap_hits(st)
    assert st.sky_px == (n_rec == 0).sum() and st.glass_px == glass.sum()
    assert_words_equal(img[~glass], ref[~glass])
    img2, _ = sc.render(with_flags(fr, INT_INDEX))
    assert_words_equal(img2[~glass], ref[~glass])
    # the device's own records of these pixels are the recorded varyings
    rays = np.zeros(w * h, vx.RAY_DTYPE)
    for py in range(h):
        for px in range(w):
            rays[py * w + px] = vx.pixel_ray(fr, px, py)
    hits = sc.query_rays(rays)
    assert_ints_equal(hits["n"].reshape(h, w).astype(np.uint8), n_rec, "records per pixel")
    hit = (n_rec >= 1).reshape(-1)
    s0 = hits["s"][hit, 0]
    assert_ints_equal(s0["cell"], frames[f"{cam}_cell"].reshape(-1, 3)[hit], "v_cellPos")
    assert_words_equal(s0["fract"], frames[f"{cam}_fract"].reshape(-1, 3)[hit])
    for k in ("color", "normal_idx", "id"):
        assert_ints_equal(s0[k].astype(np.uint8), frames[f"{cam}_{k[:6]}"].reshape(-1)[hit], k)


def test_frames_hold_every_pixel_class(frames):
    """Conditions on the recorded frames, from the reference's outputs alone (census 1,549 / 6,759 / 1,398)."""
    sky = lit = unlit = 0
    for cam in ("down", "level", "edge"):
        n_rec, step = frames[f"{cam}_n"], frames[f"{cam}_step"]
        sky += int((n_rec == 0).sum())
        lit += int(((n_rec == 1) & (step == MAX_STEPS)).sum())
        unlit += int(((n_rec == 1) & (step >= 0) & (step < MAX_STEPS)).sum())
    assert sky >= 1000 and lit >= 2000 and unlit >= 1000, (sky, lit, unlit)
