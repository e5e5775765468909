"""tests/gpu_rig.py on the CPU: each shared assertion passes on equal input and fires, with its own text, on
the smallest difference of its kind.  pytest does not rewrite that module's asserts, so this is where its
failure messages are seen to exist."""
import math

import numpy as np
import pytest

import gpu_rig
from gpu_rig import (assert_bytes_equal, assert_counters_equal, assert_no_cap_hits, assert_words_equal,
                     assert_words_equal_nan_positions, quantise_rgba8, sun_dir, vis_colour)

QNAN, QNAN_NEG, QNAN_PAYLOAD = 0x7FC00000, 0xFFC00000, 0x7FC00001      # the GPU's 0/0, x86's, another payload


def frame(nan_at=(), nan_bits=QNAN):
    """A 3 x 4 x 4 fp32 frame of distinct finite words, +0 and -0 among them, with NaNs at flat positions."""
    words = np.arange(48, dtype=np.float32).reshape(3, 4, 4) / np.float32(7)
    words[0, 0, 1] = -0.0
    bits = words.view(np.uint32)
    for i in nan_at:
        bits.reshape(-1)[i] = nan_bits
    return words


def flipped(img, i=29):
    out = img.copy()
    out.view(np.uint32).reshape(-1)[i] ^= 1             # one ulp of one word
    return out


WORD_COMPARATORS = [assert_words_equal, assert_words_equal_nan_positions]


@pytest.mark.parametrize("same", WORD_COMPARATORS)
def test_word_comparators_pass_on_equal_frames(same):
    same(frame(), frame())
    same(frame(nan_at=(5, 40)), frame(nan_at=(5, 40)))


@pytest.mark.parametrize("same", WORD_COMPARATORS)
def test_word_comparators_fire_on_one_flipped_word(same):
    with pytest.raises(AssertionError, match=r"1 words differ.*first at \[\[1, 3, 1\]\]"):
        same(flipped(frame()), frame())
    plus = frame()
    plus[0, 0, 1] = 0.0                                 # +0.0 against -0.0: equal as numbers, not as words
    assert np.array_equal(plus, frame())
    with pytest.raises(AssertionError, match=r"1 words differ.*first at \[\[0, 0, 1\]\]"):
        same(plus, frame())
    with pytest.raises(AssertionError, match="not two fp32 frames of one shape"):
        same(frame()[:2], frame())
    with pytest.raises(AssertionError, match="not two fp32 frames of one shape"):
        same(frame().astype(np.float64), frame())


def test_all_words_sees_a_nan_payload_and_rows():
    with pytest.raises(AssertionError, match="1 words differ"):
        assert_words_equal(frame(nan_at=(5,), nan_bits=QNAN_PAYLOAD), frame(nan_at=(5,)))
    with pytest.raises(AssertionError, match="1 words differ"):
        assert_words_equal(frame(nan_at=(5,), nan_bits=QNAN_NEG), frame(nan_at=(5,)))
    bad = flipped(frame())                              # flat word 29 lies in row 1
    assert_words_equal(bad, frame(), rows=[0, 2])
    assert_words_equal(bad, frame(), rows=slice(0, 1))
    with pytest.raises(AssertionError, match=r"first at \[\[0, 3, 1\]\]"):
        assert_words_equal(bad, frame(), rows=[1, 2])


def test_nan_positions_ignores_the_payload_not_the_place():
    ref = frame(nan_at=(5, 40))
    assert_words_equal_nan_positions(frame(nan_at=(5, 40), nan_bits=QNAN_NEG), ref)
    assert_words_equal_nan_positions(frame(nan_at=(5, 40), nan_bits=QNAN_PAYLOAD), ref)
    with pytest.raises(AssertionError, match="2 NaN positions differ"):
        assert_words_equal_nan_positions(frame(nan_at=(5, 41)), ref)            # moved: one missing, one extra
    with pytest.raises(AssertionError, match="1 NaN positions differ"):
        assert_words_equal_nan_positions(frame(nan_at=(5,)), ref)
    with pytest.raises(AssertionError, match="1 NaN positions differ"):
        assert_words_equal_nan_positions(frame(nan_at=(5, 40, 41)), ref)
    with pytest.raises(AssertionError, match="1 words differ"):
        assert_words_equal_nan_positions(flipped(frame(nan_at=(5, 40))), ref)


def test_bytes():
    a = (np.arange(48) * 5).astype(np.uint8).reshape(3, 4, 4)
    assert_bytes_equal(a, a.copy())
    b = a.copy()
    b[2, 1, 3] ^= 1
    with pytest.raises(AssertionError, match=r"1 bytes differ; first at \[\[2, 1, 3\]\]"):
        assert_bytes_equal(b, a)
    with pytest.raises(AssertionError, match="not two RGBA8 frames"):
        assert_bytes_equal(a.astype(np.int32), a)
    with pytest.raises(AssertionError, match="not two RGBA8 frames"):
        assert_bytes_equal(a[:2], a)


class FakeStats:
    def __init__(self, **kw):
        self.kw = kw

    def as_dict(self):
        return dict(self.kw)


def test_counters():
    ref = dict(pixels=12, sky_px=5, shadow_rays=7)
    got = dict(ref, march_wave_iters=3, kernel_ms=0.25)              # the kernel keeps more than the oracle
    assert_counters_equal(got, ref)
    assert_counters_equal(FakeStats(**got), FakeStats(**ref))
    with pytest.raises(AssertionError, match="counter sky_px: 6 != 5"):
        assert_counters_equal(dict(got, sky_px=6), ref)
    with pytest.raises(AssertionError, match="counter sky_px: 6 != 5"):
        assert_counters_equal(FakeStats(**dict(got, sky_px=6)), ref)
    lacking = {k: v for k, v in got.items() if k != "shadow_rays"}
    with pytest.raises(AssertionError, match="shadow_rays is missing from the result"):
        assert_counters_equal(lacking, ref)
    # keys: those and no others
    assert_counters_equal(dict(got, sky_px=6), ref, keys=("pixels", "shadow_rays"))
    with pytest.raises(AssertionError, match="counter sky_px"):
        assert_counters_equal(dict(got, sky_px=6), ref, keys=("sky_px",))
    with pytest.raises(AssertionError, match="march_wave_iters is missing from the reference"):
        assert_counters_equal(got, ref, keys=("march_wave_iters",))
    # ignore: kernel_ms unless told otherwise
    assert_counters_equal(got, dict(got, kernel_ms=0.5))
    with pytest.raises(AssertionError, match="counter kernel_ms"):
        assert_counters_equal(got, dict(got, kernel_ms=0.5), ignore=())
    assert_counters_equal(dict(got, sky_px=6), ref, ignore=("sky_px",))


def test_no_cap_hits():
    assert_no_cap_hits(dict(primary_cap_hits=0))
    assert_no_cap_hits(FakeStats(primary_cap_hits=0))
    with pytest.raises(AssertionError, match="1 primary walks"):
        assert_no_cap_hits(dict(primary_cap_hits=1))
    with pytest.raises(AssertionError, match="1 primary walks"):
        assert_no_cap_hits(FakeStats(primary_cap_hits=1))


def test_quantise_rgba8():
    half = np.float32(0.5) / np.float32(255)
    # eps = 2^-24: v * 255 + 0.5 is then 1.5e-5 short of 1, far more than the sum's rounding (2^-25) can make up;
    # one ulp of `half` under it is not (that sum is a tie and rounds to 1.0)
    v = np.array([0, half - np.float32(2.0 ** -24), half, 1, 2, -1], np.float32)
    assert quantise_rgba8(v).tolist() == [0, 0, 1, 255, 255, 0]
    assert quantise_rgba8(v).dtype == np.uint8
    with pytest.raises(AssertionError, match="float64"):
        quantise_rgba8(v.astype(np.float64))


def test_sun_dir_and_vis_colour():
    x, y, z = sun_dir(90, 0)
    assert abs(x) < 1e-15 and y == 0 and z == 1
    assert sun_dir(0, 0) == (1, 0, 0)
    x, y, z = sun_dir(30, 90)
    assert abs(x) < 1e-15 and math.isclose(y, math.sqrt(3) / 2) and math.isclose(z, 0.5)
    assert vis_colour(np.array([0, 1, 21, 22, 255], np.uint8)).tolist() == [0, 1, 21, 0, 0]


def test_the_rig_checks_every_part_of_the_contract(monkeypatch):
    """Rig.check over a stand-in scene and oracle: it passes when they agree and fires on a word, a counter, a
    cap hit, the integer-index frame and the RGBA8 frame."""
    monkeypatch.setattr(gpu_rig, "with_flags", lambda fr, flags: FakeFrame(fr.params.flags | flags))

    class Params:
        def __init__(self, flags):
            self.flags = flags

    class FakeFrame:
        width, height = 4, 3

        def __init__(self, flags=0):
            self.params = Params(flags)

    class FakeOracle:
        def render(self, params, w, h):
            return frame(), FakeStats(pixels=12, primary_cap_hits=0)

    class FakeScene:
        def __init__(self, **faults):
            self.faults = faults

        def render(self, fr, stats=False, pixel_format=0):
            if pixel_format:
                img = quantise_rgba8(frame())
                return (img ^ 1 if "rgba8" in self.faults else img), None
            int_index = bool(fr.params.flags & gpu_rig.INT_INDEX)
            img = flipped(frame()) if "word" in self.faults or (int_index and "int_word" in self.faults) else frame()
            st = dict(pixels=12, primary_cap_hits=0, march_wave_iters=9, kernel_ms=0.1 + int_index)
            st.update(self.faults.get("stats", {}))
            if int_index:
                st.update(self.faults.get("int_stats", {}))
            return img, FakeStats(**st)

    def rig(**faults):
        r = gpu_rig.Rig.__new__(gpu_rig.Rig)
        r.scene, r.oracle = FakeScene(**faults), FakeOracle()
        return r

    ref, g = rig().check(FakeFrame(), rgba8=True)
    assert np.array_equal(ref, frame()) and g["march_wave_iters"] == 9
    for faults, text in ((dict(word=1), "1 words differ"), (dict(stats=dict(pixels=13)), "counter pixels: 13 != 12"),
                         (dict(stats=dict(primary_cap_hits=2)), "counter primary_cap_hits"),
                         (dict(int_word=1), "1 words differ"),
                         (dict(int_stats=dict(march_wave_iters=8)), "counter march_wave_iters: 8 != 9"),
                         (dict(rgba8=1), "48 bytes differ")):
        with pytest.raises(AssertionError, match=text):
            rig(**faults).check(FakeFrame(), rgba8=True)
    rig(int_word=1).check(FakeFrame(), int_index=False)
    rig(rgba8=1).check(FakeFrame())
    with pytest.raises(AssertionError, match="integer index itself"):
        rig().check(FakeFrame(gpu_rig.INT_INDEX))
    # a cap hit the oracle has too still fails
    r = rig(stats=dict(primary_cap_hits=2))
    r.oracle.render = lambda params, w, h: (frame(), FakeStats(pixels=12, primary_cap_hits=2))
    with pytest.raises(AssertionError, match="2 primary walks"):
        r.check(FakeFrame())
