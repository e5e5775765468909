"""The oracle against the reference's own fragment shader, compiled (oracle/refpin.py).

The shader text (render.frag; render.vert for palette() and normal()) compiles unedited as C++ through
oracle/ref/glsl_shim.h, whose built-ins are written from DESIGN.md §5.  Its inputs and outputs over the cases of
tests/golden/make_ref_golden.py are recorded in tests/golden/ref_frag.npz; here

* the oracle's vxo_march and vxo_shade are held to the recorded outputs word for word, always;
* where oracle/_ref is built (a reference tree is present), the compiled shader is run again and must give the
  recorded outputs, so the fixture and the live program agree.

No tolerance: cells and steps as integers, floats as words, NaN exactly where the reference has NaN (the payload of
a NaN is the compiler's and the machine's, not the shader's).  Kept out of the comparison by construction:

* sampler LOD: DESIGN.md §5 defines LOD 0 on both sides (the page samples the field with mipmaps);
* the skybox at infinity: a sky fragment is recorded as v_cellPos = u_cellPos, v_fractPos = the pixel's direction
  under u_fractPos = 0, for which render.frag:154 normalises exactly that direction, as the oracle does;
* primary visibility, the blend stage and the extensions are no shader text: the records come from the oracle's
  own vxo_primary, and only single fragments are compared.
"""
import os
import re

import numpy as np
import pytest

from gpu_rig import assert_blob_equal, assert_ints_equal, assert_words_equal, assert_words_equal_nan_positions

HERE = os.path.dirname(os.path.abspath(__file__))
MAX_STEPS = 64                                       # render.frag:12 at Z = 32
FRAG_FIELDS = ("s_proc", "s_glass")
MARCH_FIELDS = ("s_proc", "edges")


@pytest.fixture(scope="module")
def rec():
    with np.load(os.path.join(HERE, "golden", "ref_frag.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def fields(built):
    """name -> map.bin field, built once per module by the product's host code."""
    import voxmap_amd as vx
    from oracle import refpin
    from voxmap_amd import presets
    made = {}

    def get(name):
        if name not in made:
            grid = refpin.map_grid(name)[0] if name in refpin.PINNED_MAPS else presets.scene_grid(name)
            made[name] = vx.field_build(grid)
        return made[name]
    return get


def live():
    from oracle import refpin
    if not refpin.available():
        pytest.skip("no reference tree: oracle/_ref is not built")
    return refpin


def set_params(rec, k):
    """The frame of uniform set k: nothing but the uniforms render.frag reads."""
    import voxmap_amd as vx
    p = vx.FrameParams()
    p.quality, p.time = int(rec["set_quality"][k]), float(rec["set_time"][k])
    for i in range(3):
        p.cam_cell[i], p.cam_fract[i] = int(rec["set_cell"][k, i]), float(rec["set_fract"][k, i])
        p.sun_dir[i] = float(rec["set_sun"][k, i])
    return p


def same_march(got, rec, name):
    P, K = rec[f"march_{name}_o_step"].shape
    assert_ints_equal(got["cell"].reshape(P, K, 3), rec[f"march_{name}_o_cell"], f"{name} march cells")
    assert_ints_equal(got["step"].reshape(P, K), rec[f"march_{name}_o_step"], f"{name} march steps")
    assert_words_equal_nan_positions(got["fract"].reshape(P, K, 3), rec[f"march_{name}_o_fract"])
    assert_words_equal_nan_positions(got["normal"].reshape(P, K, 3), rec[f"march_{name}_o_normal"])
    assert_words_equal(got["min_dist"].reshape(P, K), rec[f"march_{name}_o_min_dist"])


def march_inputs(rec, name):
    cell, fract, suns = rec[f"march_{name}_cell"], rec[f"march_{name}_fract"], rec["suns"]
    P, K = len(cell), len(suns)
    return np.repeat(cell, K, 0), np.repeat(fract, K, 0), np.tile(suns, (P, 1))


# ---- the oracle against the recorded outputs ------------------------------------------------------

def test_recorded_suns_are_the_sun_querys_set(rec, built):
    from test_sun_query_gpu import sun_set
    assert_words_equal(rec["suns"], sun_set())


@pytest.mark.parametrize("name", MARCH_FIELDS)
def test_oracle_march_equals_the_compiled_march(rec, fields, noise, name):
    from oracle import refpin
    sc = refpin.BareScene(fields(name), noise)
    same_march(sc.march(*march_inputs(rec, name), MAX_STEPS), rec, name)


@pytest.mark.parametrize("name", FRAG_FIELDS)
def test_oracle_shade_equals_the_compiled_main(rec, fields, noise, name):
    from oracle import refpin
    sc = refpin.BareScene(fields(name), noise)
    seen = 0
    for k in np.flatnonzero(rec["set_field"] == FRAG_FIELDS.index(name)):
        m = rec["frag_set"] == k
        got = sc.shade(set_params(rec, k), rec["frag_cell"][m], rec["frag_fract"][m], rec["frag_color"][m],
                       rec["frag_normal"][m], rec["frag_id"][m])
        assert_words_equal_nan_positions(got, rec["frag_out"][m])
        seen += int(m.sum())
    assert seen >= 2000


def test_oracle_lit_flag_equals_the_compiled_march_of_each_fragment(rec, fields, noise):
    """The sun march main() runs (render.frag:233) per recorded fragment: the oracle's step count is the
    reference's, and so is which fragments march at all (frag_step = -1: the face test of :228-232 fails)."""
    from oracle import refpin
    for name in FRAG_FIELDS:
        sc = refpin.BareScene(fields(name), noise)
        m = (rec["set_field"][rec["frag_set"]] == FRAG_FIELDS.index(name)) & (rec["frag_id"] != 1)
        sun = rec["set_sun"][rec["frag_set"]]
        marching = np.zeros(len(m), bool)
        for k in np.unique(rec["frag_set"][m]):
            s = m & (rec["frag_set"] == k)
            marching[s] = refpin.face_test(rec["frag_normal"][s], rec["set_sun"][k])
        assert_ints_equal((rec["frag_step"] >= 0) & m, marching & m, f"{name}: which fragments march")
        got = sc.march(rec["frag_cell"][marching & m], rec["frag_fract"][marching & m], sun[marching & m], MAX_STEPS)
        assert_ints_equal(got["step"], rec["frag_step"][marching & m], f"{name} sun march steps")


# ---- the recorded cases hold what they claim: from the reference's outputs alone ----------------------

def test_census_of_the_recorded_cases(rec):
    fid, step = rec["frag_id"], rec["frag_step"]
    n = {"fragments": len(fid), "sky": (fid == 1).sum(), "glass": (fid == 2).sum(),
         "lit": ((fid == 0) & (step == MAX_STEPS)).sum(), "unlit": ((fid == 0) & (step >= 0) & (step < MAX_STEPS)).sum(),
         "no march": ((fid == 0) & (step < 0)).sum(), "mountain": rec["frag_mountain"].sum(),
         "cloud": ((fid == 1) & ~rec["frag_mountain"]).sum()}
    print({k: int(v) for k, v in n.items()})
    assert n["fragments"] >= 5000
    for k in ("sky", "glass", "lit", "unlit", "no march"):
        assert n[k] >= 500, (k, int(n[k]))
    assert n["mountain"] >= 100 and n["cloud"] >= 100               # both branches of render.frag:199
    assert not (rec["frag_mountain"] & (fid != 1)).any()
    # both field kinds, both qualities, the three times, a sun below the horizon, a sun with a zero component
    assert set(rec["set_field"]) == {0, 1} and set(rec["set_quality"]) == {0, 1}
    assert {0.0, 12.5, 999.0} <= set(rec["set_time"].tolist())
    assert (rec["set_sun"][:, 2] < 0).any() and (rec["set_sun"] == 0).any()
    # both G-buffer splits: a quad-relative record has an in-face v_fractPos of 2 or more
    assert (rec["frag_fract"][fid != 1].max(axis=1) >= 2).sum() >= 500
    assert (np.abs(rec["frag_fract"][fid != 1]).max(axis=1) <= 1).sum() >= 500
    # march(): how each one ended
    cases = 0
    ends = {"budget": 0, "block": 0, "-x": 0, "+x": 0, "-y": 0, "+y": 0, "-z": 0, "+z": 0}
    dims = np.array([1024, 256, 32])
    for name in MARCH_FIELDS:
        cell, st = rec[f"march_{name}_o_cell"].reshape(-1, 3), rec[f"march_{name}_o_step"].reshape(-1)
        cases += len(st)
        out_lo, out_hi = cell < 0, cell >= dims
        inside = ~(out_lo | out_hi).any(axis=1)
        ends["budget"] += int(((st == MAX_STEPS) & inside).sum())
        ends["block"] += int((st < MAX_STEPS).sum())
        assert not ((st < MAX_STEPS) & ~inside).any()              # a march that left the grid reports MAX_STEPS
        for a, ax in enumerate("xyz"):
            ends["-" + ax] += int(out_lo[:, a].sum())
            ends["+" + ax] += int(out_hi[:, a].sum())
    print(cases, ends)
    assert cases >= 3000
    assert all(v >= 1 for v in ends.values()), ends
    assert any(np.isnan(rec[f"march_{n}_o_fract"]).any() for n in MARCH_FIELDS)      # the 0 * inf of a zero component


# ---- the live program against its recording ---------------------------------------------------------

@pytest.mark.parametrize("name", MARCH_FIELDS)
def test_compiled_march_gives_the_recorded_outputs(rec, fields, noise, name):
    refpin = live()
    same_march(refpin.Frag(fields(name), noise).march(*march_inputs(rec, name)), rec, name)


@pytest.mark.parametrize("name", FRAG_FIELDS)
def test_compiled_main_gives_the_recorded_outputs(rec, fields, noise, name):
    refpin = live()
    fq = refpin.Frag(fields(name), noise)
    for k in np.flatnonzero(rec["set_field"] == FRAG_FIELDS.index(name)):
        m = rec["frag_set"] == k
        args = [rec[f"frag_{v}"][m] for v in ("cell", "fract", "color", "normal", "id")]
        fq.uniforms(rec["set_quality"][k], rec["set_cell"][k], rec["set_fract"][k], rec["set_time"][k], rec["set_sun"][k])
        out = fq.main(*args)
        assert_words_equal_nan_positions(out, rec["frag_out"][m])
        # the mountain flag: only the cloud branch reads u_time
        sky = args[4] == 1
        if sky.any():
            fq.uniforms(rec["set_quality"][k], rec["set_cell"][k], rec["set_fract"][k], float(rec["set_time"][k]) + 321.0,
                        rec["set_sun"][k])
            other = fq.main(*[a[sky] for a in args])
            same = (other.view(np.uint32) == out[sky].view(np.uint32)).all(axis=1)
            assert_ints_equal(same, rec["frag_mountain"][m][sky], "sky fragments that do not read u_time")


def test_prelude_is_the_shaders_own_header(built):
    """oracle/ref/frag_host.cpp's prelude stands in for render.h: the same uniforms, the same constants; and the
    compiled palette() and normal() are the oracle's tables."""
    import oracle
    refpin = live()
    text = open(os.path.join(refpin.REF_TREE, "src", "shaders", "render.h")).read()
    ints = {k: int(v) for k, v in re.findall(r"const int (\w+) = (\d+);", text)}
    assert set(ints) == {"X", "Y", "Z", "c_glass"}
    c = refpin.constants()
    assert {k: c[k] for k in ints} == ints
    assert (c["Xf"], c["Yf"], c["Zf"]) == (float(ints["X"]), float(ints["Y"]), float(ints["Z"]))
    assert re.search(r"const vec3 Sf = 1\.0 / vec3\(Xf, Yf, Zf\);", text)
    assert_words_equal(c["Sf"], np.float32(1) / np.array([c["Xf"], c["Yf"], c["Zf"]], np.float32))
    frag = open(os.path.join(refpin.REF_TREE, "src", "shaders", "render.frag")).read()
    assert re.search(r"const int MAX_STEPS = 2\*Z;", frag) and c["MAX_STEPS"] == 2 * ints["Z"] == MAX_STEPS
    uniforms = set(re.findall(r"^uniform (\w+) (\w+);", text, re.M))
    host = open(os.path.join(os.path.dirname(refpin.__file__), "ref", "frag_host.cpp")).read()
    ours = set(re.findall(r"^ +(\w+) (u_\w+); +\\$", host, re.M))
    assert len(uniforms) == 7 and ours == uniforms
    pal = oracle.vxo_palette()
    for p in range(22):
        assert_words_equal(refpin.palette(p), pal[p])
    for p in (-1, 22, 255):
        assert refpin.palette(p).tolist() == [1.0, 1.0, 1.0]                # render.vert:21's trailing vec3(1)
    want = {0: (1, 0, 0), 1: (-1, 0, 0), 2: (0, 1, 0), 3: (0, -1, 0), 4: (0, 0, 1), 5: (0, 0, -1), 6: (0, 0, 0), -1: (0, 0, 0)}
    for n, v in want.items():
        assert refpin.normal(n).tolist() == list(map(float, v))


# ---- the comparators fire ---------------------------------------------------------------------------

def test_the_comparators_fire_on_a_flipped_bit(rec):
    step = rec["march_s_proc_o_step"]
    bad = step.copy()
    bad[3, 7] ^= 1
    assert_ints_equal(step, step.copy())
    with pytest.raises(AssertionError, match="1 steps differ"):
        assert_ints_equal(bad, step, "steps")
    with pytest.raises(AssertionError, match="not two integer arrays"):
        assert_ints_equal(step.astype(np.int64), step)
    with pytest.raises(AssertionError, match="not two integer arrays"):
        assert_ints_equal(step.astype(np.float32), step.astype(np.float32))
    out = rec["frag_out"]
    flipped = out.copy()
    flipped.view(np.uint32)[11, 2] ^= 1
    assert_words_equal_nan_positions(out, out.copy())
    with pytest.raises(AssertionError, match="1 words differ"):
        assert_words_equal_nan_positions(flipped, out)
    fr = rec["march_s_proc_o_fract"]
    k = tuple(np.argwhere(np.isnan(fr))[0])
    lost = fr.copy()
    lost[k] = 0.0
    with pytest.raises(AssertionError, match="NaN positions"):
        assert_words_equal_nan_positions(lost, fr)
    blob = rec["frag_out"].tobytes()
    assert_blob_equal(blob, bytes(blob))
    with pytest.raises(AssertionError, match="1 blob bytes differ"):
        assert_blob_equal(blob[:100] + bytes([blob[100] ^ 0x10]) + blob[101:], blob)
    with pytest.raises(AssertionError, match="bytes against"):
        assert_blob_equal(blob[:-1], blob)
