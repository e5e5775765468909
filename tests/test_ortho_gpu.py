"""Orthographic frames on the GPU against the oracle-assembled frames.

The views, the frame builder and the assembler come from tests/test_ortho.py,
which holds the definition to the oracle alone and shows what each view has
(sky, blocks, glass, stacked panes, lit and shadowed pixels).  Here every frame
of vx_render_ortho equals, word for word, the frame assembled from the oracle's
1 x 1 perspective frames at the pixels' own origins, with the summed counters
and no cap hit; then the flags, the definition on the device itself, the device
output path, supersampling, and the argument checks.
"""
import ctypes as C

import numpy as np
import pytest

import test_ortho as T
import test_poses
from gpu_rig import (Rig, assert_bytes_equal, assert_counters_equal, assert_no_cap_hits, assert_words_equal,
                     assert_words_equal_nan_positions, gpu_available, quantise_rgba8)
from test_aa import resolve_f32, resolve_u8
from test_ortho import BIG, CASES, SMALL, VIEWS, assemble, frame_of, origins, pixel_params

pytestmark = pytest.mark.gpu

F32, U8 = 0, 1
NO_SHADOW, NO_AO, NO_CLOUDS, PRIMARY_ONLY, REFLECT, ROUGH = 0x1, 0x2, 0x4, 0x8, 0x10, 0x20
NO_EXIT, NO_CONE, UNIT_GBUF, GLASS_SINGLE, NO_DOOM = 0x200, 0x400, 0x800, 0x8000, 0x20000
REJECTED = {"VX_FLAG_INT_INDEX": 0x40, "VX_FLAG_SOFT_POOL": 0x80, "VX_FLAG_SOFT_BRICK": 0x100,
            "VX_FLAG_GLASS_ORDER": 0x1000, "VX_FLAG_REFLECT_ALL": 0x2000, "VX_FLAG_ROWS_BOTTOM_UP": 0x4000}
EINVAL = -1


@pytest.fixture(scope="module")
def rigs(built, noise):
    """{field: a Rig}; each rig's oracle holds the exit table of the views' sun."""
    if not gpu_available():
        pytest.skip("no GPU visible")
    out = {"main": Rig(test_poses.field(), noise, test_poses.DIMS), "odd": Rig(T.odd_field(), noise, T.ODD_DIMS)}
    for r in out.values():
        r.oracle.hold_exit_table(frame_of("plan", SMALL).params)
    yield out
    for r in out.values():
        r.close()
    T._state.clear()
    test_poses._state.clear()


def formula_bytes(g, bpp):
    return (4 * (g["primary_fetches"] + g["shadow_fetches"] + g["reflect_fetches"]) + 32 * g["ao_samples"] +
            80 * g["noise_px"] + 16 * g["rough_px"] + bpp * g["pixels"])


def check(rig, fr, oracle=None, rgba8=True):
    """One orthographic frame against the assembled one: the words, every counter the oracle keeps, no cap
    hit, the header's alg_bytes, and the RGBA8 frame against the quantised reference.  Returns both."""
    import voxmap_amd as vx
    img, st = rig.scene.render_ortho(fr, stats=True)
    ref, ost = assemble(oracle or rig.oracle, fr)
    assert img.shape == ref.shape == (fr.height, fr.width, 4)
    assert_words_equal_nan_positions(img, ref)
    g = st.as_dict()
    assert_counters_equal(g, ost)
    assert_no_cap_hits(g)
    assert g["pixels"] == fr.width * fr.height and g["shadow_rays_resolved"] == 0
    assert g["alg_bytes"] == formula_bytes(g, 16) and g["kernel_ms"] > 0
    if rgba8:
        assert not np.isnan(ref).any()
        img8, st8 = rig.scene.render_ortho(fr, pixel_format=vx.PIXEL_RGBA8, stats=True)
        assert_bytes_equal(img8, quantise_rgba8(ref))
        assert_counters_equal(st8, ost)
        assert st8.alg_bytes == formula_bytes(st8.as_dict(), 4)
    return ref, g


@pytest.mark.parametrize("name,wh", CASES, ids=lambda v: str(v).replace(" ", ""))
def test_view_frames_equal_the_assembled_oracle_frames(name, wh, rigs):
    _, g = check(rigs[VIEWS[name]["field"]], frame_of(name, wh))
    if name == "plan":
        assert g["sky_px"] == 0
    if name in ("plan_up", "elev_y", "far_elev_y"):
        assert g["shadow_rays"] == 0            # every face seen is turned from the sun: no march
    else:
        assert g["shadow_rays"] > 0 and g["shadow_fetches"] > 0


def _oracle_for(rig, noise, flags):
    """The oracle whose counters a frame with these flags must give: NO_EXIT the literal march, NO_CONE the
    orthant tables, NO_DOOM the cone table without the doom table; else the rig's own."""
    import oracle
    ex = rig.oracle
    if flags & NO_EXIT:
        return oracle.Oracle(rig.dev_field, noise, oct_e=ex.oct_e, exit=False, quad=ex.qoff)
    if flags & (NO_CONE | NO_DOOM):
        o = oracle.Oracle(rig.dev_field, noise, oct_e=ex.oct_e, exit="orthant" if flags & NO_CONE else True, quad=ex.qoff)
        o.hold_exit_table(frame_of("plan", SMALL, flags=flags).params)
        return o
    return ex


FLAG_SETS = {"reflect_rough": REFLECT | ROUGH, "unit_gbuf": UNIT_GBUF, "glass_single": GLASS_SINGLE,
             "bare": NO_SHADOW | NO_AO | NO_CLOUDS, "primary_only": PRIMARY_ONLY, "no_exit": NO_EXIT,
             "no_cone": NO_CONE, "no_doom": NO_DOOM}


@pytest.mark.parametrize("mode", list(FLAG_SETS))
@pytest.mark.parametrize("name", ["iso", "elev_y"])
def test_flags(name, mode, rigs, noise):
    rig, flags = rigs["main"], FLAG_SETS[mode]
    ref, g = check(rig, frame_of(name, SMALL, flags=flags), oracle=_oracle_for(rig, noise, flags))
    if mode == "reflect_rough":
        assert g["reflect_rays"] > 0 and g["rough_px"] > 0
    if mode == "bare":
        assert g["shadow_rays"] == g["ao_samples"] == g["noise_px"] == 0
    if mode in ("no_exit", "no_cone", "no_doom") and name == "iso":
        # the same frame as with every table, by other fetches
        base, gb = rig.scene.render_ortho(frame_of(name, SMALL), stats=True)
        assert_words_equal(base, ref)
        assert gb.shadow_rays == g["shadow_rays"] and gb.shadow_fetches <= g["shadow_fetches"]


# 16 pixels (x, y) of iso at SMALL and what the oracle's census shows there (tests/test_ortho.py)
FIXED = {"sky": [(0, 0), (56, 22), (20, 2), (56, 0)],
         "block": [(45, 0), (30, 10), (3, 8), (15, 21), (55, 12)],
         "glass": [(28, 4), (43, 4), (38, 5), (50, 8), (11, 11), (30, 14)],
         "stacked": [(33, 7)]}


def test_the_definition_on_the_device(rigs):
    """Each of the 16 pixels equals the single pixel of vx_render's 1 x 1 frame at that pixel's origin."""
    import voxmap_amd as vx
    rig = rigs["main"]
    assert sum(len(v) for v in FIXED.values()) == 16
    for flags in (0, REFLECT | ROUGH):
        fr = frame_of("iso", SMALL, flags=flags)
        cells, fracts = origins(fr.params, *SMALL)
        img, _ = rig.scene.render_ortho(fr)
        img8, _ = rig.scene.render_ortho(fr, pixel_format=vx.PIXEL_RGBA8)
        for kind, pixels in FIXED.items():
            for x, y in pixels:
                one = vx.Frame(pixel_params(fr.params, cells[y, x], fracts[y, x]), 1, 1)
                px, st = rig.scene.render(one, stats=True)
                assert (st.sky_px, st.block_px, st.glass_px) == {"sky": (1, 0, 0), "block": (0, 1, 0)}.get(kind, (0, 0, 1))
                if kind in ("glass", "stacked"):
                    panes = rig.oracle.glass_layers(one.params, 1, 1, threads=1)[0, 0]
                    assert (panes >= 2) == (kind == "stacked"), (x, y, panes)
                assert_words_equal(img[y:y + 1, x:x + 1], px)
                px8, _ = rig.scene.render(one, pixel_format=vx.PIXEL_RGBA8)
                assert_bytes_equal(img8[y:y + 1, x:x + 1], px8)


def test_picking_needs_nothing_new(rigs):
    """vx_pixel_ray_ortho's rays go to vx_query_rays as they stand: what each of the 16 pixels shows."""
    import voxmap_amd as vx
    fr = frame_of("iso", SMALL)
    pixels = [(k, xy) for k, v in FIXED.items() for xy in v]
    hits = rigs["main"].scene.query_rays(np.array([vx.pixel_ray_ortho(fr, x, y) for _, (x, y) in pixels]))
    for (kind, xy), hit in zip(pixels, hits):
        if kind == "sky":
            assert hit["n"] == 0, xy
        else:
            assert hit["n"] >= 1 and hit["s"][0]["id"] == (0 if kind == "block" else 2), (kind, xy)
            assert hit["s"][0]["t"] > 0 and np.isfinite(hit["s"][0]["t"])


@pytest.mark.parametrize("fmt", [F32, U8], ids=["f32", "u8"])
def test_device_output_between_canary_rows(fmt, rigs):
    """Into the middle of a torch buffer with canary rows before and after the frame, at 57 x 23, whose edge
    tiles are partial: the frame is the host path's and the canaries keep their pattern."""
    import torch
    rig = rigs["main"]
    w, h = SMALL
    fr = frame_of("iso", SMALL)
    host, hst = rig.scene.render_ortho(fr, pixel_format=fmt, stats=True)
    row = w * (16 if fmt == F32 else 4)
    guard, n = 9 * row - (9 * row) % 16, h * row           # nine canary rows each side, 16-byte aligned
    buf = torch.full((guard + n + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    for stats in (False, True):
        st = rig.scene.render_ortho_device(fr, buf.data_ptr() + guard, pixel_format=fmt, stream=stream.cuda_stream,
                                           stats=stats)
        stream.synchronize()
        got = buf.cpu().numpy()
        assert (got[:guard] == 0xA5).all() and (got[guard + n:] == 0xA5).all()
        assert got[guard:guard + n].tobytes() == host.tobytes()
        if stats:
            assert_counters_equal(st, hst)
        else:
            assert st is None
        buf[guard:guard + n] = 0xA5
    torch.cuda.synchronize()


@pytest.mark.parametrize("fmt", [F32, U8], ids=["f32", "u8"])
@pytest.mark.parametrize("s", [2, 4])
def test_supersampling_is_the_resolve_of_the_big_orthographic_frame(s, fmt, rigs):
    import voxmap_amd as vx
    rig = rigs["main"]
    w, h = 24, 16
    bpp = 16 if fmt == F32 else 4
    for name in ("iso", "elev_y"):
        fr = frame_of(name, (w, h))
        big, bst = rig.scene.render_ortho(frame_of(name, (s * w, s * h)), pixel_format=fmt, stats=True)
        want = (resolve_f32 if fmt == F32 else resolve_u8)(big, s)
        least = 8 * s * w * bpp
        assert vx.aa_plan(w, h, s, fmt, least)["n_chunks"] == s * h // 8 >= 4 and vx.aa_plan(w, h, s, fmt)["n_chunks"] == 1
        for cap in (0, least):
            img, st = rig.scene.render_ortho(fr, s, pixel_format=fmt, stats=True, scratch_cap=cap)
            (assert_words_equal if fmt == F32 else assert_bytes_equal)(img, want)
            assert_counters_equal(st, bst, keys=[k for k in bst.as_dict() if not k.endswith("_iters") and
                                                 k not in ("march_lane_slots", "kernel_ms")])
            assert st.pixels == s * s * w * h and st.alg_bytes == bst.alg_bytes and st.kernel_ms > 0
            plain, _ = rig.scene.render_ortho(fr, s, pixel_format=fmt, scratch_cap=cap)
            assert plain.tobytes() == img.tobytes()
    one, _ = rig.scene.render_ortho(fr, 1, pixel_format=fmt, scratch_cap=1)       # ss = 1: no scratch, the cap unread
    assert one.tobytes() == rig.scene.render_ortho(fr, pixel_format=fmt)[0].tobytes()


def test_argument_errors(rigs):
    """Every VX_EINVAL case of the header; a rejected flag names itself; and nothing ran: the valid call that
    follows gives the frame and the counters of one launch."""
    import torch
    import voxmap_amd as vx
    rig = rigs["main"]
    sc, L = rig.scene, vx.lib()
    v = VIEWS["plan"]
    w, h = SMALL
    good = frame_of("plan", SMALL)
    want, wst = sc.render_ortho(good, stats=True)
    out = np.zeros((h, w, 4), np.float32)

    def refused(fr, word, **kw):
        with pytest.raises(vx.VoxmapError) as e:
            sc.render_ortho(fr, **kw)
        assert e.value.code == EINVAL and word in str(e.value), (word, str(e.value))
        assert word in L.vx_last_error().decode()

    def basis(**kw):
        q = dict(cell=v["cell"], fract=v["fract"], fwd=v["fwd"], right=v["right"], up=v["up"])
        q.update({k: kw.pop(k) for k in list(kw) if k in q})
        return T.frame_from_basis(q["cell"], q["fract"], q["fwd"], q["right"], q["up"], w, h, **kw)

    # NULL scene, params, out
    p = C.byref(good.params)
    assert L.vx_render_ortho(None, p, w, h, 1, F32, out.ctypes.data, 0, None, 0, None) == EINVAL
    assert L.vx_render_ortho(sc.handle, None, w, h, 1, F32, out.ctypes.data, 0, None, 0, None) == EINVAL
    assert L.vx_render_ortho(sc.handle, p, w, h, 1, F32, None, 0, None, 0, None) == EINVAL
    # sizes, ss, scratch_cap, pixel format, alignment
    for fw, fh in ((0, h), (w, 0), (32769, 1), (1, 32769)):
        refused(vx.Frame(good.params, fw, fh), "frame size")
    refused(vx.Frame(good.params, 16385, 1), "ss * w", supersample=2)
    refused(vx.Frame(good.params, 1, 8193), "ss * h", supersample=4)
    refused(good, "ss", supersample=3)
    refused(good, "ss", supersample=0)
    refused(good, "scratch_cap", supersample=2, scratch_cap=8 * 2 * w * 16 - 1)
    refused(good, "pixel format", pixel_format=7)
    buf = torch.full((w * h * 16 + 32,), 0xA5, dtype=torch.uint8, device="cuda")
    with pytest.raises(vx.VoxmapError) as e:
        sc.render_ortho_device(good, buf.data_ptr() + 4)
    assert e.value.code == EINVAL and "aligned" in str(e.value)
    # the frame itself
    refused(basis(quality=0), "quality")
    for ax in range(3):
        for f in (1.0, -2.0 ** -30, float("nan")):
            refused(basis(fract=tuple(f if i == ax else .5 for i in range(3))), "cam_fract")
        refused(basis(right=tuple(float("nan") if i == ax else 1.0 for i in range(3))), "ray_right")
        refused(basis(up=tuple(float("inf") if i == ax else 1.0 for i in range(3))), "ray_up")
        refused(basis(fwd=tuple(float("-inf") if i == ax else 1.0 for i in range(3))), "ray_fwd")
        # |cam_cell| + ceil(|right| + |up|) + 2 >= 2^22: refused on the bound, taken one cell inside it
        reach = int(np.ceil(abs(v["right"][ax]) + abs(v["up"][ax])))
        for sign in (1, -1):
            edge = sign * ((1 << 22) - reach - 2)
            refused(basis(cell=tuple(edge if i == ax else v["cell"][i] for i in range(3))), "2^22")
            inside = basis(cell=tuple(edge - sign if i == ax else v["cell"][i] for i in range(3)))
            _, st = sc.render_ortho(inside, stats=True)
            assert st.pixels == w * h and st.primary_cap_hits == 0
    refused(basis(fwd=(0.0, -0.0, 0.0)), "ray_fwd")
    refused(basis(shadow_samples=2, sun_radius=0.03), "shadow_samples")
    sc.render_ortho(basis(shadow_samples=1))                       # 0 and 1 are the hard shadow
    for name, bit in REJECTED.items():
        refused(basis(flags=bit), name)
        refused(basis(flags=bit | REFLECT | ROUGH), name)
    refused(basis(flags=0x10000), "0x10000")
    refused(basis(flags=1 << 31), "0x80000000")
    # nothing of the above ran or wrote: the buffer keeps its pattern, the next call is one launch's
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == 0xA5).all() and not out.any()
    img, st = sc.render_ortho(good, stats=True)
    assert_words_equal(img, want)
    assert_counters_equal(st, wst, keys=[k for k in wst.as_dict() if k != "kernel_ms"])
