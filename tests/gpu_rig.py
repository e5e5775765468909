"""The contract of the GPU tests, stated once: every frame the HIP library
renders equals the scalar oracle's frame word for word, with the same work
counters and no cap hit.

A helper module, not a test module (pytest collects test_*.py only): the GPU
probe and the fixture that skips without one, the scene constructor, the
comparators, and Rig, a scene on the device with the oracle over the field it
reads back.  pytest does not rewrite the `assert` statements of a file it does
not collect, so every check here raises an AssertionError with its own text;
tests/test_gpu_rig.py shows on the CPU that each one fires.
"""
import math

import numpy as np
import pytest

INT_INDEX = 0x40                    # include/voxmap.h VX_FLAG_INT_INDEX


def gpu_available():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:  # pragma: no cover
        return False


@pytest.fixture(scope="module", autouse=True)
def need_gpu(built):
    """Imported by name into a test module: builds, then skips the module without a GPU."""
    if not gpu_available():
        pytest.skip("no GPU visible")


def bin_scene(field, noise, dims, **kw):
    """vx.Scene over a field (Z, Y, X, 4) and a noise texture (H, W, 4), both as FORMAT_BIN bytes, on device
    0; kw: dist_cap, mesh_chunk, noise_seed, noise_size.  noise = None: the scene synthesises its own."""
    import voxmap_amd as vx
    if noise is None:
        return vx.Scene(map_bytes=field.tobytes(), map_format=vx.FORMAT_BIN, dims=tuple(dims), device=0, **kw)
    kw.setdefault("noise_size", (noise.shape[1], noise.shape[0]))
    return vx.Scene(map_bytes=field.tobytes(), map_format=vx.FORMAT_BIN, noise_bytes=noise.tobytes(),
                    noise_format=vx.FORMAT_BIN, dims=tuple(dims), device=0, **kw)


def sun_dir(el_deg, az_deg):
    el, az = math.radians(el_deg), math.radians(az_deg)
    return (math.cos(el) * math.cos(az), math.cos(el) * math.sin(az), math.sin(el))


def vis_colour(b):
    """The traversal's colour: meshed palette indices 1..21 (sdf.cpp:284), else 0 (include/voxmap.h)."""
    return np.where((b >= 1) & (b <= 21), b, 0).astype(np.uint8)


def quantise_rgba8(ref):
    """The RGBA8 frame of an fp32 frame: floor(clamp(v, 0, 1) * 255 + 0.5) in fp32, one rounding per operation."""
    q = np.clip(ref, 0, 1) * np.float32(255) + np.float32(0.5)
    if q.dtype != np.float32:
        raise AssertionError(f"quantised in {q.dtype}, not in float32")
    return q.astype(np.uint8)


def with_flags(frame, flags):
    import voxmap_amd as vx
    p = frame.params.copy()
    p.flags |= flags
    return vx.Frame(p, frame.width, frame.height)


# ---- comparators --------------------------------------------------------------------

def _raise_if(bad, what, note=""):
    """bad: a boolean array, True where two arrays differ."""
    if bad.any():
        raise AssertionError(f"{int(np.count_nonzero(bad))} {what} differ{note}; first at {np.argwhere(bad)[:5].tolist()}")


def _words(img, ref):
    if img.shape != ref.shape or img.dtype != np.float32 or ref.dtype != np.float32:
        raise AssertionError(f"{img.dtype} {img.shape} against {ref.dtype} {ref.shape}: not two fp32 frames of one shape")
    return img.view(np.uint32), ref.view(np.uint32)


def assert_words_equal(img, ref, rows=None):
    """Every 32-bit word equal, a NaN's sign and payload included; rows: an index into both first."""
    if rows is not None:
        img, ref = img[rows], ref[rows]
    a, b = _words(img, ref)
    if (a != b).any():
        with np.errstate(all="ignore"):
            rel = np.nanmax(np.abs(img - ref) / np.maximum(np.abs(ref), 1e-6))
        _raise_if(a != b, "words", f" (max rel {rel:.3g})")


def assert_words_equal_nan_positions(img, ref):
    """NaN exactly where ref has NaN (sign and payload are not compared: x86's 0/0 and the GPU's differ),
    every other word equal."""
    a, b = _words(img, ref)
    nan = np.isnan(ref)
    _raise_if(np.isnan(img) != nan, "NaN positions")
    _raise_if((a != b) & ~nan, "words")


def assert_bytes_equal(img, ref):
    """Two RGBA8 frames, every byte."""
    if img.shape != ref.shape or img.dtype != np.uint8 or ref.dtype != np.uint8:
        raise AssertionError(f"{img.dtype} {img.shape} against {ref.dtype} {ref.shape}: not two RGBA8 frames of one shape")
    _raise_if(img != ref, "bytes")


def assert_ints_equal(got, ref, what="values"):
    """Two integer arrays of one shape and dtype (cells, steps, mask words, quad tables), every element."""
    got, ref = np.asarray(got), np.asarray(ref)
    if got.shape != ref.shape or got.dtype != ref.dtype or got.dtype.kind not in "iub":
        raise AssertionError(f"{what}: {got.dtype} {got.shape} against {ref.dtype} {ref.shape}: not two integer arrays of one kind")
    _raise_if(got != ref, what)


def assert_blob_equal(got, ref, what="blob"):
    """Two byte strings (a file against its recorded copy): the length, then every byte."""
    got, ref = bytes(got), bytes(ref)
    if len(got) != len(ref):
        raise AssertionError(f"{what}: {len(got)} bytes against {len(ref)}")
    if got != ref:
        a, b = np.frombuffer(got, np.uint8), np.frombuffer(ref, np.uint8)
        _raise_if(a != b, f"{what} bytes")


def _dict(st):
    return st if isinstance(st, dict) else st.as_dict()


def assert_counters_equal(st, ost, keys=None, ignore=("kernel_ms",)):
    """Every counter the reference ost keeps (or those of keys), but for the ignored ones, equal in st;
    Stats objects or dicts."""
    g, o = _dict(st), _dict(ost)
    for k in o if keys is None else keys:
        if k in ignore:
            continue
        if k not in g or k not in o:
            raise AssertionError(f"counter {k} is missing from the {'result' if k not in g else 'reference'}")
        if g[k] != o[k]:
            raise AssertionError(f"counter {k}: {g[k]} != {o[k]}")


def assert_no_cap_hits(st):
    hits = _dict(st)["primary_cap_hits"]
    if hits != 0:
        raise AssertionError(f"{hits} primary walks ended at the step cap")


# ---- the rig ------------------------------------------------------------------------

class Rig:
    """A field on the device, the copy the scene reads back, and the oracle over that copy."""

    same = staticmethod(assert_words_equal_nan_positions)      # a subclass may hold frames to assert_words_equal

    def __init__(self, field, noise, dims, **scene_kw):
        self.scene = bin_scene(field, noise, dims, **scene_kw)
        self.dev_field = self.scene.read_field()
        self.oracle = self.make_oracle(noise)

    def make_oracle(self, noise):
        """The oracle check() compares with when it is given none: every exit table, the default cap."""
        import oracle
        return oracle.Oracle(self.dev_field, noise, exit=True)

    def close(self):
        self.scene.close()

    def check(self, fr, int_index=True, rgba8=False, oracle=None):
        """One frame against the oracle: the words (self.same), every counter the oracle keeps, no cap hit;
        then with VX_FLAG_INT_INDEX the same words and counters, and the RGBA8 frame == the oracle's quantised.
        Returns the oracle's frame and the kernel's counters."""
        import voxmap_amd as vx
        w, h = fr.width, fr.height
        img, st = self.scene.render(fr, stats=True)
        ref, ost = (oracle or self.oracle).render(fr.params, w, h)
        self.same(img, ref)
        assert_counters_equal(st, ost)
        assert_no_cap_hits(st)
        if int_index:
            if fr.params.flags & INT_INDEX:
                raise AssertionError("the frame asks for the integer index itself")
            img2, st2 = self.scene.render(with_flags(fr, INT_INDEX), stats=True)
            self.same(img2, img)
            assert_counters_equal(st2, st)
        if rgba8:
            if np.isnan(ref).any():
                raise AssertionError("a NaN in the oracle's frame has no RGBA8 value")
            img8, _ = self.scene.render(fr, pixel_format=vx.PIXEL_RGBA8)
            assert_bytes_equal(img8, quantise_rgba8(ref))
        return ref, st.as_dict()
