"""CPU: the 16-bit fixed point of the inside test's near stage (csrc/ray_winding.hip: near_encode), through
tuch_near_encode_host -- the kernels' own __host__ __device__ conversion run on the host.

Levels are k / 8192 m, k in [-32768, 32767].  Rounding DOWN gives the largest level <= value, rounding UP the smallest
level >= value, both pinned here to a float64 floor / ceil.  Where no such level exists (below the range rounding down,
above it rounding up) and for NaN the result is the end of the range on that side: -32768 rounding down, +32767 rounding
up.  A number rounded down only ever stands on the left of a `left > right` rejection and a number rounded up only on
the right, so those two codes can never reject.  On the OTHER side of the range the conversion clamps to the last level,
which is still a level on the correct side of the value (and keeps the conversion monotone)."""
import ctypes

import numpy as np

SCALE = 8192.0
LO, HI = -32768, 32767


def _encoder():
    from tuch_amd import _C
    fn = _C.lib().tuch_near_encode_host
    out = ctypes.c_int(0)
    ref = ctypes.byref(out)

    def enc(value, up):
        assert fn(ctypes.c_float(value), int(up), ref) == 0
        return out.value
    return enc


def _expected(values, up):
    """float64: ceil / floor of value * SCALE, clamped to the levels (value * SCALE is exact in float64)."""
    t = values.astype(np.float64) * SCALE
    return np.clip(np.ceil(t) if up else np.floor(t), LO, HI).astype(np.int64)


def test_every_level_and_its_neighbours_round_to_the_correct_side():
    enc = _encoder()
    levels = (np.arange(LO, HI + 1, dtype=np.float64) / SCALE).astype(np.float32)
    assert np.array_equal(levels.astype(np.float64) * SCALE, np.arange(LO, HI + 1))      # every level is a float
    below = np.nextafter(levels, np.float32(-np.inf))
    above = np.nextafter(levels, np.float32(np.inf))
    for values in (levels, below, above):
        for up in (False, True):
            want = _expected(values, up)
            got = np.fromiter((enc(float(v), up) for v in values), dtype=np.int64, count=len(values))
            bad = np.nonzero(got != want)[0]
            assert bad.size == 0, (up, float(values[bad[0]]), int(got[bad[0]]), int(want[bad[0]]))
    # the level itself is a fixed point of both directions
    assert enc(float(levels[12345]), False) == enc(float(levels[12345]), True) == LO + 12345


def test_beyond_the_range_saturates_to_the_code_that_never_rejects():
    enc = _encoder()
    top, bottom = np.float32(4.0), np.float32(-4.0)             # 32768 / SCALE (one past the last level), LO / SCALE
    inf = np.float32(np.inf)
    for v in (top, np.nextafter(top, inf), np.nextafter(top, -inf), np.float32(3.0e38), inf):
        assert enc(float(v), True) == HI, v                     # no level >= v: the code no lower bound exceeds
        assert enc(float(v), False) == HI, v                    # the largest level <= v is the last one
    assert enc(float(np.nextafter(np.float32(HI / SCALE), -inf)), True) == HI
    for v in (np.nextafter(bottom, -inf), np.float32(-3.0e38), -inf):
        assert enc(float(v), False) == LO, v                    # no level <= v: the code that exceeds no upper bound
        assert enc(float(v), True) == LO, v                     # the smallest level >= v is the first one
    assert enc(float(bottom), False) == LO and enc(float(bottom), True) == LO
    assert enc(float(np.nextafter(bottom, inf)), False) == LO and enc(float(np.nextafter(bottom, inf)), True) == LO + 1
    nan = float('nan')
    assert enc(nan, True) == HI and enc(nan, False) == LO


def test_zero_and_denormals():
    enc = _encoder()
    assert enc(-0.0, False) == 0 and enc(-0.0, True) == 0 and enc(0.0, False) == 0 and enc(0.0, True) == 0
    tiny = [np.float32(1e-45), np.float32(1e-39), np.nextafter(np.float32(1.17549435e-38), np.float32(0))]
    for v in tiny:
        assert v > 0 and v < np.finfo(np.float32).tiny
        assert enc(float(v), False) == 0 and enc(float(v), True) == 1, v
        assert enc(float(-v), True) == 0 and enc(float(-v), False) == -1, v
    values = np.array(tiny + [-t for t in tiny] + [np.float32(0.0), np.float32(-0.0)], np.float32)
    for up in (False, True):
        assert [enc(float(v), up) for v in values] == list(_expected(values, up))
