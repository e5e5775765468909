"""Sun queries, the host half (no GPU): vx_query_sun's argument checks, the struct
layouts and VX_SUN_WORDS, vx_ground_points against a numpy restatement, and the
k_sun_query kernel's resources in the built library."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_query_sun_argument_errors_do_not_touch_the_gpu(built):
    """Checked before any HIP call: the scene handle below is not a scene, and no GPU is needed."""
    import voxmap_amd as vx
    from voxmap_amd import _abi
    L = vx.lib()
    pts = np.zeros(4, vx.SUN_POINT_DTYPE)
    out = np.full((4, 2), 0xA5A5A5A5, np.uint32)
    suns = np.array([[0.3, 0.4, 0.5], [0.0, 0.0, 1.0]], np.float32)
    fake = C.create_string_buffer(4096)             # never dereferenced: every call fails its argument check
    scene = C.cast(fake, C.c_void_p)
    P, S, O = pts.ctypes.data, suns.ctypes.data, out.ctypes.data

    def bad_sun(v, at=1):
        s = suns.copy()
        s[at] = v
        return s

    nan, inf, zero, mzero = (bad_sun(v) for v in ([0.1, np.nan, 0.2], [np.inf, 0.1, 0.2], [0.0, 0.0, 0.0],
                                                  [0.0, -0.0, 0.0]))
    many = np.tile(suns, (600, 1))                  # 1200 > VX_MAX_SUNS
    #        scene  points n   suns  k  flags out on_device
    cases = [(None, P, 4, S, 2, 0, O, 0), (scene, None, 4, S, 2, 0, O, 0), (scene, P, 4, None, 2, 0, O, 0),
             (scene, P, 4, S, 2, 0, None, 0), (scene, P, -1, S, 2, 0, O, 0), (scene, P, (1 << 26) + 1, S, 2, 0, O, 0),
             (scene, P, 4, S, 0, 0, O, 0), (scene, P, 4, S, -3, 0, O, 0),
             (scene, P, 4, many.ctypes.data, _abi.MAX_SUNS + 1, 0, O, 0),
             (scene, P, 4, nan.ctypes.data, 2, 0, O, 0), (scene, P, 4, inf.ctypes.data, 2, 0, O, 0),
             (scene, P, 4, zero.ctypes.data, 2, 0, O, 0), (scene, P, 4, mzero.ctypes.data, 2, 0, O, 0),
             (scene, P, 4, S, 2, 0x2, O, 0), (scene, P, 4, S, 2, 0x80000000, O, 0),
             (scene, P + 4, 2, S, 2, 0, O, 1), (scene, P, 2, S, 2, 0, O + 2, 1),   # misaligned device arrays
             (scene, None, 0, None, 2, 0, None, 1), (None, P, 0, S, 2, 0, O, 0)]
    for i, (sc, p, n, s, k, flags, o, dev) in enumerate(cases):
        st = _abi.SunStats()
        rc = L.vx_query_sun(sc, p, n, s, k, 0, flags, o, dev, None, C.byref(st))
        assert rc == _abi.VX_EINVAL, (i, rc)
        assert b"vx_query_sun" in L.vx_last_error()
    assert (out == 0xA5A5A5A5).all()
    # n == 0 is fine and does nothing (no HIP call either: this machine may have no GPU)
    st = _abi.SunStats(points=7)
    assert L.vx_query_sun(scene, P, 0, S, 2, 0, 0, O, 0, None, C.byref(st)) == 0
    assert st.points == 0 and (out == 0xA5A5A5A5).all()
    assert L.vx_query_sun(scene, P, 0, many.ctypes.data, _abi.MAX_SUNS, 5, _abi.SUNQ_NO_EXIT, O, 1, None, None) == 0


def test_struct_layouts_and_sun_words():
    import voxmap_amd as vx
    from voxmap_amd import _abi
    assert C.sizeof(_abi.SunPoint) == 32 == vx.SUN_POINT_DTYPE.itemsize
    assert C.sizeof(_abi.SunStats) == 56
    assert [n for n, _ in _abi.SunPoint._fields_] == list(vx.SUN_POINT_DTYPE.names)
    for name, _ in _abi.SunPoint._fields_:
        assert getattr(_abi.SunPoint, name).offset == vx.SUN_POINT_DTYPE.fields[name][1], name
    assert [vx.sun_words(k) for k in (1, 32, 33, 1024)] == [2, 2, 3, 33]
    header = open(os.path.join(ROOT, "include", "voxmap.h")).read()
    assert "#define VX_ABI_VERSION 10" in header
    # the header's own macro and constants, evaluated
    m = re.search(r"#define VX_SUN_WORDS\(k\) (.+)", header)
    assert m
    for k in (1, 32, 33, 1024):
        assert eval(m.group(1).replace("(k)", f"({k})").replace("/", "//")) == vx.sun_words(k)
    assert re.search(r"#define VX_MAX_SUNS (\d+)", header).group(1) == str(_abi.MAX_SUNS) == "1024"
    assert int(re.search(r"#define VX_SUN_INVALID (0x[0-9A-Fa-f]+)u", header).group(1), 16) == _abi.SUN_INVALID
    assert int(re.search(r"#define VX_SUNQ_NO_EXIT (0x[0-9A-Fa-f]+)u", header).group(1), 16) == _abi.SUNQ_NO_EXIT


def _ground_ref(field):
    """numpy restatement: per column the topmost cell with R == G == 0; skipped if none or in the top layer."""
    Z, Y, X, _ = field.shape
    block = (field[..., 0] == 0) & (field[..., 1] == 0)
    has = block.any(0)
    ztop = Z - 1 - np.argmax(block[::-1], axis=0)            # (Y, X)
    keep = has & (ztop < Z - 1)
    ys, xs = np.nonzero(keep)                                # row-major: y, then x -- x fastest
    return xs, ys, ztop[ys, xs] + 1


def _fields():
    import voxmap_amd as vx
    from voxmap_amd import scenes
    rng = np.random.default_rng(11)
    odd = rng.integers(0, 3, size=(9, 43, 5, 4)).astype(np.uint8)     # (Z, Y, X, 4) of a (5, 43, 9) field: raw texels
    odd[..., 0] *= rng.integers(0, 2, size=odd.shape[:3]).astype(np.uint8)
    odd[..., 1] *= odd[..., 0] > 0                                    # G == 0 wherever R == 0, plus R == 0, G != 0 cells
    odd[2, :, :, 1] = np.where(odd[2, :, :, 0] == 0, 3, odd[2, :, :, 1])   # R == 0 but G != 0: not a block
    tiny = np.full((3, 3, 3, 4), 5, np.uint8)
    tiny[:, 1, 1, :2] = 0                                             # a full-height column: skipped
    tiny[0, 0, 2, :2] = 0                                             # ground only
    tiny[1, 2, 0, :2] = 0                                             # a block at z = 1, air below and above
    # column (0, 0) stays empty
    return {"proc5": vx.field_build(scenes.small_proc(5)), "single_block": vx.field_build(scenes.single_block()),
            "odd": odd, "tiny": tiny}


@pytest.mark.parametrize("name", ["proc5", "single_block", "odd", "tiny"])
def test_ground_points_match_numpy(built, name):
    import voxmap_amd as vx
    from voxmap_amd import _abi
    field = _fields()[name]
    Z, Y, X, _ = field.shape
    xs, ys, zs = _ground_ref(field)
    pts, cols = vx.ground_points(field)
    assert len(pts) == len(xs) == len(cols) and len(pts) > 0
    assert np.array_equal(pts["cell"], np.stack([xs, ys, zs], 1))
    assert np.array_equal(cols, xs + X * ys) and (np.diff(cols) > 0).all()
    assert (pts["fract"] == np.float32([0.5, 0.5, 0.0])).all()
    assert (pts["normal_idx"] == 4).all() and not pts["reserved"].any()
    if name == "tiny":
        assert [tuple(c) for c in pts["cell"]] == [(2, 0, 1), (0, 2, 2)]
    if name == "odd":
        assert len(pts) < X * Y                               # some columns are skipped
    # the size query alone, a buffer one short, and no columns array
    L = vx.lib()
    n = C.c_size_t(99)
    assert L.vx_ground_points(field.ctypes.data, X, Y, Z, None, None, 0, C.byref(n)) == 0 and n.value == len(pts)
    short = np.zeros(len(pts), vx.SUN_POINT_DTYPE)
    assert L.vx_ground_points(field.ctypes.data, X, Y, Z, short.ctypes.data, None, len(pts) - 1,
                              C.byref(n)) == _abi.VX_EINVAL
    assert L.vx_ground_points(field.ctypes.data, X, Y, Z, short.ctypes.data, None, len(pts), C.byref(n)) == 0
    assert short.tobytes() == pts.tobytes()
    for bad in [(None, X, Y, Z), (field.ctypes.data, 0, Y, Z), (field.ctypes.data, X, -1, Z), (field.ctypes.data, X, Y, 0)]:
        assert L.vx_ground_points(*bad, None, None, 0, C.byref(n)) == _abi.VX_EINVAL
    assert L.vx_ground_points(field.ctypes.data, X, Y, Z, None, None, 0, None) == _abi.VX_EINVAL


def test_points_of_hits_keeps_the_first_record():
    import voxmap_amd as vx
    h = np.zeros(5, vx.HIT_DTYPE)
    h["n"] = [-1, 0, 1, 2, 1]
    for i in range(5):
        h["s"]["cell"][i, 0] = [i, i + 1, i + 2]
        h["s"]["fract"][i, 0] = [0.25 * i, 0.0, 0.5]
        h["s"]["normal_idx"][i, 0] = i
        h["s"]["normal_idx"][i, 1] = 5
    p = vx.points_of_hits(h)
    assert p.dtype == vx.SUN_POINT_DTYPE and len(p) == 3
    assert p["normal_idx"].tolist() == [2, 3, 4] and p["cell"].tolist() == [[2, 3, 4], [3, 4, 5], [4, 5, 6]]
    assert p["fract"][:, 0].tolist() == [0.5, 0.75, 1.0] and not p["reserved"].any()


def test_k_sun_query_kernel_resources(built):
    """k_sun_query is in the library under a name kernel_meta.check does not budget, keeps the KernelArgs
    copy it carries out of scratch, and spills nothing."""
    from voxmap_amd import _abi, kernel_meta
    ks = kernel_meta.kernels(_abi.LIB_PATH)
    q = {k: v for k, v in ks.items() if "k_sun_query" in k}
    assert len(q) == 2, sorted(q)                    # with and without counters
    for name, v in q.items():
        assert "k_render" not in name
        assert v["private_segment_fixed_size"] == 0, (name, v)
        assert v.get("vgpr_spill_count", 0) == 0, (name, v)
