"""The resampler's kernels (csrc/resample.hip) at every geometry the tile planner distinguishes: all 132 ordered pairs of the twelve
standard rates (include/wwhip.h: "every pair ... passes") and 500000 -> 16000, against the float64 statement of tests/resample64.py.

tests/test_gpu_resample.py runs seven rates to 16 kHz, which are two of the planner's classes - both with full tiles everywhere.
Here every pair runs, so every class does (tests/resample64.py: plan_class, CLASS_REPS; tests/native/launch_plan_check.cpp holds the
library's planner to the same table on the CPU):
  the up == 1 form with 63, 100, 136 and 209 lanes per tile instead of 256; the phase form with 128, 64 and no items per long tile
  (no items: long ranges take resample_phase_kernel<1> too); up = 2560 (11025 -> 192000: the largest table, 174,080 taps) and
  down = 2560 (192000 -> 11025: the longest staged spans); output rates other than 16 kHz.

The error bound is the derived one of tests/test_gpu_resample.py, not a measured one: |y - y64| <= (tpp + 2) * 2^-24 * A[m],
A[m] = sum |h| |x|; where A[m] = 0 the output is exactly 0.  Everything that says "same bits" is assert_array_equal.

Shapes per pair: clips of 1, 2, 3, down - 1, down, down + 1 samples (short ranges: resample_phase_kernel<1> or one partial tile of
the up == 1 form), one long clip of max(4500, 16 up + 4100) outputs (more than two tiles of every form - the largest tile is 2,048
outputs -, and 16 up is the planner's threshold for the 8-outputs-per-item form, which the clip takes across at least two tiles
wherever the pair has that form), a full-scale square of 1,000 samples, 1,000 zeros, and the square followed by the zeros."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resample64 as R64  # noqa: E402

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
PAIRS = R64.PAIRS + ((500000, 16000),)
REPS = R64.CLASS_REPS


def _id(pair):
    return f"{pair[0]}-{pair[1]}"


def _pcm(rng, n, rate):
    t = np.arange(n) / float(rate)
    chirp = 8000.0 * np.sin(2 * np.pi * (200.0 * t + 0.5 * 3800.0 / 1.5 * np.mod(t, 1.5) * np.mod(t, 1.5)))
    return np.clip(np.rint(rng.normal(0, 2000, n) + chirp), -32768, 32767).astype(np.int16)


def _square(n):
    return np.where((np.arange(n) // 37) % 2 == 0, 32767, -32768).astype(np.int16)


def _long_len(up, down):
    cnt = max(4500, 16 * up + 4100)
    return -(-cnt * down // up)


def _ref(x, up, down, half, h):
    """(y64, A) of a clip: the float64 output and the bound's sum |h| |x|."""
    x64 = x.astype(np.float64) / 32768.0 if x.dtype == np.int16 else x.astype(np.float64)
    if len(x) <= 4096:
        return R64.direct(x64, up, down, half, h), R64.direct(np.abs(x64), up, down, half, np.abs(h))
    return R64.poly(x64, up, down, h), R64.poly(np.abs(x64), up, down, np.abs(h))


@pytest.mark.parametrize("pair", PAIRS, ids=_id)
def test_pair_against_float64_alone_and_as_int16(pair):
    """a. the geometry the library reports is the float64 statement's; b. every output within the derived bound (and exactly 0 where
    the bound is 0) for int16 and float32 clips, ONE ragged call per sample format; c. a clip alone has the bits it has in the batch;
    d. the int16 output is clip(rint(y * 32768)) of the float output, for the long clip and the squares."""
    from wwhip.resample import Resampler
    rate_in, rate_out = pair
    up, down, half, h = R64.design(rate_in, rate_out)
    tpp = R64.tpp(up, half)
    rng = np.random.default_rng(rate_in + 7 * rate_out)
    lengths = [1, 2, 3, down - 1, down, down + 1, _long_len(up, down)]
    sq = _square(1000)
    clips = {"i16": [_pcm(rng, n, rate_in) for n in lengths] + [sq, np.zeros(1000, np.int16), np.concatenate((sq, np.zeros(1000, np.int16)))],
             "f32": [(_pcm(rng, n, rate_in).astype(np.float32) / np.float32(32768.0)) * np.float32(0.999) for n in lengths] + [np.zeros(1000, np.float32)]}
    LONG, SQUARE, SILENT, SQUARE_ZEROS = 6, 7, {"i16": 8, "f32": 7}, 9
    rs = Resampler(rate_in, rate_out)
    try:
        assert (rs.up, rs.down, rs.half, rs.taps_per_output) == (up, down, half, tpp)                                           # a.
        assert rs.table_bytes == 4 * tpp * up
        got = {k: rs(clips[k], np.float32) for k in clips}
        worst = 0.0
        for k in clips:                                                                                                        # b.
            for x, y in zip(clips[k], got[k]):
                y64, A = _ref(x, up, down, half, h)
                assert y.dtype == np.float32 and y.shape == y64.shape == (rs.out_len(len(x)),) == (R64.out_len(len(x), up, down),)
                bound = (tpp + 2) * U * A
                err = np.abs(y.astype(np.float64) - y64)
                used = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
                worst = max(worst, used)
                assert (err <= bound).all(), (pair, k, len(x), used)
            assert not got[k][SILENT[k]].any() and got[k][SILENT[k]].shape == (rs.out_len(1000),)
        assert len(got["i16"][LONG]) >= max(4500, 16 * up + 4100)
        print(f"{rate_in} -> {rate_out} {R64.plan_class(up, down, half)}: worst used fraction of (tpp + 2) 2^-24 A = {worst:.3f}, "
              f"largest |y| of the square {float(np.abs(got['i16'][SQUARE]).max()):.3f}")
        for k in clips:                                                                                                        # c.
            for x, y in zip(clips[k], got[k]):
                np.testing.assert_array_equal(rs(x), y)
        for i in (LONG, SQUARE, SQUARE_ZEROS):                                                                                 # d.
            want = np.clip(np.rint(got["i16"][i] * np.float32(32768.0)), -32768, 32767).astype(np.int16)
            np.testing.assert_array_equal(rs(clips["i16"][i], np.int16), want)
        # the band-limited full-scale square overshoots (Gibbs: about 9 % of the jump of 2), so the int16 clamp is exercised
        assert np.abs(got["i16"][SQUARE]).max() > 1.0
    finally:
        rs.close()


@pytest.mark.parametrize("pair", REPS, ids=_id)
def test_pieces_and_packets_are_the_one_shot(pair):
    """e. The long clip in four pieces with exactly ceil(half / up) samples of history - cut at 0, 1, an odd count near a third and
    three outputs past a tile boundary - is the one-shot bit for bit, in one call and piece by piece; so are StreamResampler's
    packets of 1 .. 3,000 samples (never more than a sixth of the clip, so that a short clip is cut too)."""
    from wwhip.resample import Resampler, StreamResampler, determined
    rate_in, rate_out = pair
    up, down, half, _ = R64.design(rate_in, rate_out)
    x = _pcm(np.random.default_rng(rate_in + 11 * rate_out), _long_len(up, down), rate_in)
    rs = Resampler(rate_in, rate_out)
    st = StreamResampler(rate_in, rate_out)
    try:
        one = rs(x)
        tile = R64.tile_outputs(up, down, half, len(one))
        hist = -(-half // up)
        cuts = [0, 1, (len(one) // 3) | 1, max(1, (2 * len(one) // 3) // tile) * tile + 3, len(one)]
        assert cuts == sorted(set(cuts)) and len(one) > 2 * tile, (cuts, tile)
        segs, i0, o0, cnt = [], [], [], []
        for a, b in zip(cuts[:-1], cuts[1:]):
            k0 = max(0, a * down // up - hist)                      # exactly ceil(half / up) samples of history
            k1 = min(len(x), ((b - 1) * down + half) // up + 1)     # up to the last sample the piece's last output reads
            segs.append(x[k0:k1]); i0.append(k0); o0.append(a); cnt.append(b - a)
        np.testing.assert_array_equal(np.concatenate(rs.ranges(segs, i0, o0, cnt)), one)
        for s, a, b, n in zip(segs, i0, o0, cnt):                   # and each piece in a call of its own
            np.testing.assert_array_equal(rs.range(s, a, b, n), one[b:b + n])
        rng = np.random.default_rng(3)
        got, pos, pushes = [], 0, 0
        while pos < len(x):
            k = int(rng.integers(1, min(3000, max(1, len(x) // 6)) + 1))
            got.append(st.push(x[pos:pos + k]))
            pos = min(pos + k, len(x))
            pushes += 1
            assert st.n_out == determined(pos, up, down, half)
        got.append(st.flush())
        assert pushes >= 6
        np.testing.assert_array_equal(np.concatenate(got), one)
    finally:
        st.close()
        rs.close()


def test_refusals_at_the_table_limit():
    """f. 44101 <-> 16000 (about 3 M taps either way) are WW_EINVAL with *out == NULL; 500000 -> 16000 is accepted."""
    from wwhip import _lib
    lib, ctx = _lib.load(), _lib.default_context()
    for ri, ro in ((44101, 16000), (16000, 44101)):
        h = C.c_void_p(1)                                           # (not NULL going in: the call clears it)
        assert lib.ww_resampler_create(ctx.handle, ri, ro, None, C.byref(h)) == _lib.WW_EINVAL and not h.value
        text = (lib.ww_last_error(ctx.handle) or b"").decode()
        assert "WW_RESAMPLE_MAX_TAPS" in text and "1048576" in text, text
    h = C.c_void_p()
    assert lib.ww_resampler_create(ctx.handle, 500000, 16000, None, C.byref(h)) == _lib.WW_OK and h.value
    info = _lib.ResampleInfo()
    assert lib.ww_resampler_info(h, C.byref(info)) == _lib.WW_OK
    assert (info.up, info.down, info.half, info.taps_per_output, info.table_bytes) == (4, 125, 4233, 2117, 4 * 2117 * 4)
    assert lib.ww_resampler_destroy(h) == _lib.WW_OK
