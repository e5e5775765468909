"""Supersampled antialiasing on the CPU: the plan, the argument checks, the resolves.

vx_render_aa (include/voxmap.h) renders the (ss*w) x (ss*h) frame in chunks of
whole output rows and resolves each on the device.  What needs no GPU is here:
vx_aa_plan_for, the pure host function that returns the split vx_render_aa
uses; the VX_EINVAL list, which is checked before any GPU call (so it is
reachable with a NULL scene, and a NULL scene with valid arguments reports its
own error); the additive ABI; and the numpy restatement of the two resolves
(resolve_u8, resolve_f32), which tests/test_aa_gpu.py imports as its reference
and which is held here to a per-pixel Python loop written from the header's
text.
"""
import ctypes as C
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, U8 = 0, 1                      # VX_PIXEL_RGBA32F, VX_PIXEL_RGBA8
BPP = {F32: 16, U8: 4}
EINVAL = -1


# ---- the resolves, restated (the GPU test's reference) -----------------------------

def resolve_u8(hi: np.ndarray, s: int) -> np.ndarray:
    """(s*h, s*w, 4) uint8 -> (h, w, 4): per channel (sum of the s*s bytes + s*s/2) / (s*s), integers."""
    h, w = hi.shape[0] // s, hi.shape[1] // s
    total = hi.reshape(h, s, w, s, 4).astype(np.uint32).sum(axis=(1, 3))
    return ((total + s * s // 2) // (s * s)).astype(np.uint8)


def _resolve2_f32(hi: np.ndarray) -> np.ndarray:
    """((H(0,0) + H(1,0)) + (H(0,1) + H(1,1))) * 0.25f, indices (dx, dy), fp32 adds in this order."""
    return ((hi[0::2, 0::2] + hi[0::2, 1::2]) + (hi[1::2, 0::2] + hi[1::2, 1::2])) * np.float32(0.25)


def resolve_f32(hi: np.ndarray, s: int) -> np.ndarray:
    """(s*h, s*w, 4) float32 -> (h, w, 4): the 2 x 2 resolve, for s = 4 applied twice."""
    assert hi.dtype == np.float32 and s in (2, 4)
    out = _resolve2_f32(hi)
    return out if s == 2 else _resolve2_f32(out)


def _slow_u8(hi, s):
    h, w = hi.shape[0] // s, hi.shape[1] // s
    out = np.zeros((h, w, 4), np.uint8)
    for y in range(h):
        for x in range(w):
            for c in range(4):
                total = sum(int(hi[s * y + dy, s * x + dx, c]) for dy in range(s) for dx in range(s))
                out[y, x, c] = (total + s * s // 2) // (s * s)
    return out


def _slow_block2(px):
    """px(dx, dy) -> one np.float32, the header's expression."""
    return np.float32(np.float32(np.float32(px(0, 0) + px(1, 0)) + np.float32(px(0, 1) + px(1, 1))) * np.float32(0.25))


def _slow_f32(hi, s):
    h, w = hi.shape[0] // s, hi.shape[1] // s
    out = np.zeros((h, w, 4), np.float32)
    for y in range(h):
        for x in range(w):
            for c in range(4):
                if s == 2:
                    out[y, x, c] = _slow_block2(lambda dx, dy: hi[2 * y + dy, 2 * x + dx, c])
                else:       # 2 x 2 blocks first, then 2 x 2 of those results
                    q = {(i, j): _slow_block2(lambda dx, dy: hi[4 * y + 2 * j + dy, 4 * x + 2 * i + dx, c])
                         for i in range(2) for j in range(2)}
                    out[y, x, c] = _slow_block2(lambda dx, dy: q[dx, dy])
    return out


@pytest.mark.parametrize("s", [2, 4])
def test_resolve_restatement_u8(s):
    rng = np.random.default_rng(10 + s)
    hi = rng.integers(0, 256, (5 * s, 11 * s, 4), dtype=np.uint8)
    hi[:s, :s] = 255                              # a block of all 255: 255 * n + n/2 stays in its half
    hi[:s, s:2 * s] = 0
    hi[s:2 * s, :s, 0] = [[255] * s, *[[254] * s] * (s - 1)]      # a sum just past a rounding step
    got = resolve_u8(hi, s)
    assert got.shape == (5, 11, 4) and got.dtype == np.uint8
    assert np.array_equal(got, _slow_u8(hi, s))
    assert (got[0, 0] == 255).all() and (got[0, 1] == 0).all()


@pytest.mark.parametrize("s", [2, 4])
def test_resolve_restatement_f32(s):
    rng = np.random.default_rng(20 + s)
    # magnitudes spread over many binades, both signs: the order of the adds shows
    hi = (rng.standard_normal((5 * s, 11 * s, 4)) * np.exp2(rng.integers(-6, 7, (5 * s, 11 * s, 4)))).astype(np.float32)
    got = resolve_f32(hi, s)
    want = _slow_f32(hi, s)
    assert got.shape == (5, 11, 4) and got.dtype == np.float32
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # the order matters on these inputs: another association gives other bits somewhere
    other = ((hi[0::2, 0::2] + hi[1::2, 0::2]) + (hi[0::2, 1::2] + hi[1::2, 1::2])) * np.float32(0.25)
    if s == 2:
        assert not np.array_equal(other.view(np.uint32), got.view(np.uint32))


# ---- the plan -----------------------------------------------------------------------

def _min_cap(w, s, fmt):
    return 8 * s * w * BPP[fmt]


# (w, h, ss, fmt, cap); cap None = the minimum of that row, 0 = the default
PLANS = [
    (1, 1, 2, U8, 0), (1, 1, 4, F32, 0), (1, 1, 2, U8, None), (1, 1, 4, F32, None),
    (37, 19, 2, U8, None), (37, 19, 4, U8, None), (37, 19, 2, F32, None), (37, 19, 4, F32, None),
    (37, 19, 2, U8, 0), (37, 19, 4, F32, 0), (37, 19, 2, U8, 1 << 30), (37, 19, 4, F32, 1 << 40),
    (64, 40, 2, U8, None), (64, 40, 4, F32, 3 * 8 * 4 * 64 * 16 + 5),         # three chunks' worth and a bit
    (1, 333, 2, U8, None), (1, 333, 4, U8, 300), (333, 1, 2, F32, None), (5, 7, 4, U8, 2 * 8 * 4 * 5 * 4),
    (3840, 2160, 2, U8, 0), (3840, 2160, 2, U8, 8 << 20), (3840, 2160, 4, F32, 0), (3840, 2160, 2, F32, 128 << 20),
    (16384, 16384, 2, F32, 0), (8192, 8192, 4, F32, None), (8192, 8192, 4, U8, 0),
    (37, 19, 1, U8, 0), (37, 19, 1, F32, 1),
]


@pytest.mark.parametrize("w,h,s,fmt,cap", PLANS)
def test_plan_tiles_the_rows(built, w, h, s, fmt, cap):
    import voxmap_amd as vx
    cap = _min_cap(w, s, fmt) if cap is None else cap
    plan = vx.aa_plan(w, h, s, fmt, cap)
    assert plan["ss"] == s
    rows, n = plan["chunk_rows_out"], plan["n_chunks"]
    assert rows >= 1 and n >= 1
    # chunk c covers [c * rows, min(h, (c + 1) * rows)): [0, h) exactly once, in order
    covered = []
    for c in range(n):
        y0, y1 = c * rows, min(h, (c + 1) * rows)
        assert y0 < y1, "an empty chunk"
        covered += [(y0, y1)]
        if c < n - 1:
            assert y1 - y0 == rows and (s * rows) % 8 == 0
    assert covered[0][0] == 0 and covered[-1][1] == h
    assert all(a[1] == b[0] for a, b in zip(covered, covered[1:]))
    if s == 1:
        assert (rows, n, plan["scratch_bytes"]) == (h, 1, 0)
        return
    assert (s * rows) % 8 == 0
    eff = cap if cap else vx.AA_DEFAULT_SCRATCH
    assert plan["scratch_bytes"] == s * rows * s * w * BPP[fmt] <= eff
    # as many rows as the cap holds: one more block of 8 hi-res rows would not fit, or the frame is covered
    assert plan["scratch_bytes"] + 8 * s * w * BPP[fmt] > eff or n == 1
    if cap == _min_cap(w, s, fmt):
        assert s * rows == 8 and n == -(-s * h // 8)


def test_default_scratch_is_the_headers(built):
    import re
    import voxmap_amd as vx
    text = open(os.path.join(ROOT, "include", "voxmap.h")).read()
    m = re.search(r"#define VX_AA_DEFAULT_SCRATCH \(\(size_t\)(\d+) << (\d+)\)", text)
    assert m and int(m.group(1)) << int(m.group(2)) == vx.AA_DEFAULT_SCRATCH
    assert re.search(r"#define VX_AA_MAX 4\b", text) and vx.AA_MAX == 4


# ---- errors: VX_EINVAL before any GPU call ------------------------------------------

def _params():
    import voxmap_amd as vx
    return vx.make_frame((48.0, 24.0, 18.0), (1.1, 0.0, 0.6), 64, 40).params


def _call(scene, p, w, h, s, fmt, out, cap=0):
    import voxmap_amd as vx
    L = vx.lib()
    rc = L.vx_render_aa(scene, C.byref(p) if p is not None else None, w, h, s, fmt,
                        out.ctypes.data if out is not None else None, 0, None, cap, None)
    return rc, L.vx_last_error().decode()


def test_argument_errors_need_no_scene(built):
    p, out = _params(), np.zeros((40, 64, 4), np.float32)
    for s in (0, 3, 5, 8, -2):
        rc, msg = _call(None, p, 64, 40, s, U8, out)
        assert rc == EINVAL and "ss" in msg, (s, msg)
    for w, h, s in ((16385, 40, 2), (64, 16385, 2), (8193, 40, 4), (64, 8193, 4), (0, 40, 2), (64, -1, 2)):
        rc, msg = _call(None, p, w, h, s, U8, out)
        assert rc == EINVAL and "32768" in msg, (w, h, s, msg)
    for s, fmt in ((2, U8), (4, U8), (2, F32), (4, F32)):
        rc, msg = _call(None, p, 64, 40, s, fmt, out, cap=_min_cap(64, s, fmt) - 1)
        assert rc == EINVAL and "scratch_cap" in msg, (s, fmt, msg)
    rc, msg = _call(None, p, 64, 40, 2, 7, out)
    assert rc == EINVAL and "pixel format" in msg
    rc, msg = _call(None, None, 64, 40, 2, U8, out)
    assert rc == EINVAL and "null" in msg
    rc, msg = _call(None, p, 64, 40, 2, U8, None)
    assert rc == EINVAL and "null" in msg
    # a NULL scene with every other argument valid reports its own error, at each factor
    for s in (1, 2, 4):
        rc, msg = _call(None, p, 64, 40, s, U8, out, cap=_min_cap(64, s, U8))
        assert rc == EINVAL and "null scene" in msg, (s, msg)


def test_plan_errors(built):
    import voxmap_amd as vx
    for args, word in (((64, 40, 3, U8, 0), "ss"), ((16385, 40, 2, U8, 0), "32768"), ((64, 40, 2, 9, 0), "pixel format"),
                       ((64, 40, 4, F32, _min_cap(64, 4, F32) - 1), "scratch_cap"), ((0, 40, 2, U8, 0), "32768")):
        with pytest.raises(vx.VoxmapError) as e:
            vx.aa_plan(*args)
        assert e.value.code == EINVAL and word in str(e.value), (args, str(e.value))
    assert vx.lib().vx_aa_plan_for(64, 40, 2, U8, 0, None) == EINVAL
    assert vx.aa_plan(16384, 16384, 2, U8)["n_chunks"] >= 1          # the largest frame is in range


# ---- the ABI stays 10, and grows ----------------------------------------------------

def test_abi_is_additive(built):
    import voxmap_amd as vx
    from voxmap_amd import _abi
    text = open(os.path.join(ROOT, "include", "voxmap.h")).read()
    assert "#define VX_ABI_VERSION 10\n" in text
    assert vx.lib().vx_abi_version() == 10 == _abi.ABI_VERSION
    for name in ("vx_render_aa", "vx_aa_plan_for"):
        assert name in text and hasattr(vx.lib(), name) and name in {s[0] for s in _abi.SIGNATURES}
    assert "map.js:7" in text
    assert C.sizeof(_abi.AaPlan) == 24 and _abi.AaPlan.scratch_bytes.offset == 16
    for name in ("aa_plan", "AA_MAX", "AA_DEFAULT_SCRATCH"):
        assert name in vx.__all__ and hasattr(vx, name)
    for name in ("render_aa", "render_aa_device"):
        assert callable(getattr(vx.Scene, name))
    import inspect
    assert inspect.signature(vx.Scene.draw_scene).parameters["supersample"].default == 1
