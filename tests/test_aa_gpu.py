"""vx_render_aa on the GPU against the oracle's hi-res frame, resolved in numpy.

The sub-pixel rays of a w x h frame at factor s are the pixel rays of the
(s*w) x (s*h) frame of the same FrameParams, so the oracle pins every sample:
the reference of a case is Oracle.render(params, s*w, s*h) (fp32), put through
the numpy restatement of the header's resolve that tests/test_aa.py holds to a
per-pixel loop -- bit for bit in RGBA32F, and in RGBA8 every byte of the oracle
frame quantised (gpu_rig.quantise_rgba8) and then integer-resolved.

Two scenes, one camera each (an eye and a view direction; the basis is built in
look_frame) whose hi-res frames hold sky, block and glass pixels, asserted on
the oracle's counters.  Every hi-res word at these poses is finite (asserted
before any comparison of bits), so the fp32 resolve meets no NaN payload.
Output shapes: 37 x 19 (odd width: the hi-res rows of s = 2 RGBA8 are 8 bytes
off every other row; ragged against the 32 x 8 block and an 8-row chunk),
64 x 40 (everything aligned) and 1 x 1.  The 4 or 16 samples of a 1 x 1 output
cannot hold all three pixel classes, so the census is asserted at the two
larger shapes.
"""
import ctypes as C
import threading

import numpy as np
import pytest

from gpu_rig import (Rig, assert_bytes_equal, assert_counters_equal, assert_no_cap_hits, assert_words_equal,
                     gpu_available, quantise_rgba8)
from test_aa import BPP, F32, U8, resolve_f32, resolve_u8
from test_poses import frame_from_basis

pytestmark = pytest.mark.gpu

EINVAL = -1
SHAPES = [(37, 19), (64, 40), (1, 1)]
FACTORS = [2, 4]
# scene -> (eye, view direction)
CAMERAS = {
    "proc3": ((10.3, 5.2, 12.4), (1.0, 0.5, -0.45)),
    "glass_wall": ((5.3, 20.2, 9.4), (1.0, 0.3, -0.2)),
}
TAN = 0.7                            # half-width of the view at distance 1


def look_frame(name, w, h, **kw):
    """The scene's camera at w x h: fwd the unit view direction, right horizontal, up
    perpendicular to both, the view TAN wide and TAN * h / w high whatever the size."""
    eye, d = CAMERAS[name]
    fwd = np.array(d, np.float64) / np.linalg.norm(d)
    right = np.cross(fwd, (0.0, 0.0, 1.0))
    right /= np.linalg.norm(right)
    up = np.cross(right, fwd)
    cell = [int(np.floor(v)) for v in eye]
    fract = [float(np.float32(v - c)) for v, c in zip(eye, cell)]
    return frame_from_basis(cell, fract, fwd, right * TAN, up * (TAN * h / w), w, h, **kw)


class World(Rig):
    """One scene on the device, the oracle over its read-back field, and the
    oracle's hi-res frames, each rendered once and left unchanged."""

    def __init__(self, name, noise):
        import voxmap_amd as vx
        from voxmap_amd import scenes
        self.name = name
        grid = scenes.small_proc(3) if name == "proc3" else scenes.glass_wall()
        Z, Y, X = grid.shape
        assert (X, Y, Z) == ((96, 48, 16) if name == "proc3" else (64, 64, 16))
        super().__init__(vx.field_build(grid), noise, (X, Y, Z))
        self._hi = {}

    def hi(self, fr, s):
        """(fp32 frame, OStats dict) of the oracle at s * (w, h); finite, read-only."""
        key = (bytes(fr.params), fr.width, fr.height, s)
        if key not in self._hi:
            ref, ost = self.oracle.render(fr.params, s * fr.width, s * fr.height)
            assert np.isfinite(ref).all()
            ref.setflags(write=False)
            self._hi[key] = (ref, ost.as_dict())
        return self._hi[key]

    def reference(self, fr, s, fmt):
        ref, ost = self.hi(fr, s)
        return (resolve_f32(ref, s) if fmt == F32 else resolve_u8(quantise_rgba8(ref), s)), ost

    def plain_stats(self, fr, s, fmt):
        """The counters of a plain Scene.render of the hi-res frame."""
        import voxmap_amd as vx
        _, st = self.scene.render(vx.Frame(fr.params, s * fr.width, s * fr.height), pixel_format=fmt, stats=True)
        return st.as_dict()


_worlds = {}


@pytest.fixture(scope="module", autouse=True)
def _scenes(built):
    if not gpu_available():
        pytest.skip("no GPU visible")
    yield
    for w in _worlds.values():
        w.close()
    _worlds.clear()


def world(name, noise):
    if name not in _worlds:
        _worlds[name] = World(name, noise)
    return _worlds[name]


def _check(wd, fr, s, fmt, **kw):
    """render_aa with stats against the resolved oracle frame, the oracle's counters and
    the plain hi-res render's; returns the image."""
    want, ost = wd.reference(fr, s, fmt)
    img, st = wd.scene.render_aa(fr, s, pixel_format=fmt, stats=True, **kw)
    assert img.shape == (fr.height, fr.width, 4)
    (assert_words_equal if fmt == F32 else assert_bytes_equal)(img, want)
    g = st.as_dict()
    assert_counters_equal(g, ost)
    assert_counters_equal(g, wd.plain_stats(fr, s, fmt))
    assert_no_cap_hits(g)
    assert g["pixels"] == s * s * fr.width * fr.height
    assert g["kernel_ms"] > 0
    return img


@pytest.mark.parametrize("fmt", [F32, U8], ids=["f32", "u8"])
@pytest.mark.parametrize("s", FACTORS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda v: f"{v[0]}x{v[1]}")
@pytest.mark.parametrize("name", list(CAMERAS))
def test_equals_the_resolved_oracle_frame(name, shape, s, fmt, noise):
    wd = world(name, noise)
    fr = look_frame(name, *shape)
    if shape != (1, 1):
        _, ost = wd.hi(fr, s)
        assert ost["sky_px"] > 0 and ost["block_px"] > 0 and ost["glass_px"] > 0, ost
    img = _check(wd, fr, s, fmt)
    if fmt == U8:
        assert (img[..., 3] == 255).all()


@pytest.mark.parametrize("fmt", [F32, U8], ids=["f32", "u8"])
@pytest.mark.parametrize("s", FACTORS)
def test_chunking_changes_no_byte(s, fmt, noise):
    """The least scratch (one chunk per 8 hi-res rows, the last one ragged) and one chunk."""
    import voxmap_amd as vx
    wd = world("proc3", noise)
    w, h = 37, 19
    fr = look_frame("proc3", w, h)
    least = 8 * s * w * BPP[fmt]
    many, one = vx.aa_plan(w, h, s, fmt, least), vx.aa_plan(w, h, s, fmt, 1 << 30)
    assert many["n_chunks"] == -(-s * h // 8) >= 5 and (s * h) % 8 != 0 and one["n_chunks"] == 1
    a = _check(wd, fr, s, fmt, scratch_cap=least)
    b = _check(wd, fr, s, fmt, scratch_cap=1 << 30)
    assert a.tobytes() == b.tobytes()
    c, _ = wd.scene.render_aa(fr, s, pixel_format=fmt, scratch_cap=3 * least)       # and without stats
    assert c.tobytes() == a.tobytes()


@pytest.mark.parametrize("mode", ["full_quality", "soft4", "quality0"])
def test_flags_pass_through(mode, noise):
    import voxmap_amd as vx
    kw = {"full_quality": dict(flags=vx.FLAG_FULL_QUALITY), "soft4": dict(shadow_samples=4, sun_radius=0.03),
          "quality0": dict(quality=0)}[mode]
    for name in CAMERAS:
        wd = world(name, noise)
        fr = look_frame(name, 37, 19, **kw)
        for fmt in (F32, U8):
            _check(wd, fr, 2, fmt)
    # the mode shows: another frame than the default one
    base, _ = wd.hi(look_frame(name, 37, 19), 2)
    assert not np.array_equal(wd.hi(fr, 2)[0], base)


@pytest.mark.parametrize("fmt", [F32, U8], ids=["f32", "u8"])
def test_factor_one_is_vx_render(fmt, noise):
    wd = world("proc3", noise)
    fr = look_frame("proc3", 37, 19)
    a, sa = wd.scene.render_aa(fr, 1, pixel_format=fmt, stats=True, scratch_cap=1)     # the cap is not looked at
    b, sb = wd.scene.render(fr, pixel_format=fmt, stats=True)
    assert a.tobytes() == b.tobytes()
    assert_counters_equal(sa, sb)                   # two Stats: the same counters on both sides


@pytest.mark.parametrize("shape,s,fmt,guard", [((37, 19), 2, U8, 64), ((37, 19), 4, F32, 64), ((64, 40), 2, U8, 64),
                                               ((64, 40), 2, U8, 68), ((64, 40), 4, U8, 68), ((64, 40), 2, F32, 64)],
                         ids=lambda v: str(v).replace(" ", ""))
def test_device_output_on_a_callers_stream(shape, s, fmt, guard, noise):
    """Into the middle of a tensor, `guard` bytes from either end (68: an RGBA8 out that is
    4- but not 8-byte aligned): the guards keep their pattern, the frame is the host path's."""
    import torch
    wd = world("glass_wall", noise)
    w, h = shape
    fr = look_frame("glass_wall", w, h)
    host, _ = wd.scene.render_aa(fr, s, pixel_format=fmt)
    n = w * h * BPP[fmt]
    buf = torch.full((guard + n + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    for cap in (0, 8 * s * w * BPP[fmt]):
        assert wd.scene.render_aa_device(fr, s, buf.data_ptr() + guard, pixel_format=fmt, stream=stream.cuda_stream,
                                         scratch_cap=cap) is None
        stream.synchronize()
        got = buf.cpu().numpy()
        assert (got[:guard] == 0xA5).all() and (got[guard + n:] == 0xA5).all()
        assert got[guard:guard + n].tobytes() == host.tobytes()
        buf[guard:guard + n] = 0xA5
    if fmt == F32:       # an RGBA32F out off its 16-byte alignment is refused, nothing written
        import voxmap_amd as vx
        with pytest.raises(vx.VoxmapError) as e:
            wd.scene.render_aa_device(fr, s, buf.data_ptr() + guard + 4, pixel_format=fmt, stream=stream.cuda_stream)
        assert e.value.code == EINVAL and "aligned" in str(e.value)
        stream.synchronize()
        assert (buf.cpu().numpy() == 0xA5).all()


def test_two_threads_two_factors(noise):
    """One scene, two threads on their own streams, factors 2 and 4 at once, the least
    scratch (many chunks each): each result is its single-threaded frame."""
    import torch
    wd = world("proc3", noise)
    w, h = 37, 19
    fr = look_frame("proc3", w, h)
    want = {s: wd.scene.render_aa(fr, s, pixel_format=U8)[0] for s in FACTORS}
    results, errors = {}, []

    def work(s):
        try:
            stream = torch.cuda.Stream()
            out = torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda")
            stream.wait_stream(torch.cuda.current_stream())
            frames = []
            for _ in range(4):
                wd.scene.render_aa_device(fr, s, out.data_ptr(), pixel_format=U8, stream=stream.cuda_stream,
                                          scratch_cap=8 * s * w * 4)
                stream.synchronize()
                frames.append(out.cpu().numpy().copy())
            results[s] = frames
        except Exception as e:  # pragma: no cover - reported below
            errors.append((s, repr(e)))

    torch.cuda.synchronize()
    threads = [threading.Thread(target=work, args=(s,)) for s in FACTORS]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for s in FACTORS:
        for f in results[s]:
            assert f.tobytes() == want[s].tobytes(), s


def test_argument_errors_with_a_live_scene(noise):
    import voxmap_amd as vx
    wd = world("proc3", noise)
    fr = look_frame("proc3", 37, 19)
    cases = [(fr, dict(supersample=3), "ss"),
             (vx.Frame(fr.params, 16385, 1), dict(supersample=2), "ss * w"),
             (vx.Frame(fr.params, 1, 8193), dict(supersample=4), "ss * h"),
             (fr, dict(supersample=2, scratch_cap=8 * 2 * 37 * 16 - 1), "scratch_cap")]
    for f, kw, word in cases:
        with pytest.raises(vx.VoxmapError) as e:
            wd.scene.render_aa(f, **kw)
        assert e.value.code == EINVAL and word in str(e.value), (kw, str(e.value))
        assert word in vx.lib().vx_last_error().decode()
    # the scene renders as before
    _check(wd, fr, 2, F32)


def test_draw_scene_routes_through_it(noise):
    """Scene.draw_scene(supersample=2) is render_aa of the same frame; 1 is the plain canvas."""
    import voxmap_amd as vx
    wd = world("proc3", noise)
    cam, sun = (48.3, 24.2, 12.5), vx.sun_from_hour(1.0)
    # a camera looking straight down: clip = P * T(-cam) * (x, y, z, 1), w_clip = -z_eye
    proj = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, -1.002, -0.2], [0, 0, -1, 0]], np.float64)
    move = np.eye(4)
    move[:3, 3] = [-v for v in cam]
    m = (proj @ move).T.reshape(-1).astype(np.float32)           # column-major, as u_matrix
    args = (m, cam, sun, 0, 5.0)
    q = vx.frame_from_matrix(m, cam)
    for i in range(3):
        q.sun_dir[i] = sun[i]
    q.quality, q.time = 1, 5.0
    f2 = vx.Frame(q, 37, 19)
    assert wd.scene.draw_scene(*args, width=37, height=19).tobytes() == \
        wd.scene.render(f2, pixel_format=U8)[0].tobytes()
    assert wd.scene.draw_scene(*args, width=37, height=19, supersample=2).tobytes() == \
        wd.scene.render_aa(f2, 2, pixel_format=U8)[0].tobytes()
