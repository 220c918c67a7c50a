"""Stream banks at the rates whose geometry takes the rate kernels (csrc/resample.hip: stream_rate_tick_kernel,
stream_rate_splice_kernel) where tests/test_gpu_stream_rate.py and tests/test_gpu_stream_rates.py (48000, 44100, 22050, 8000) do not go.

No new contract (tests/stream_rate_pairs.py states it): a bank at rate R gives the bits of the 16 kHz bank given z = D zeros + the
one-shot's int16 output - and tests/test_gpu_resample_pairs.py holds the one-shot at these rates against float64.  What is new is
the path through the kernels:

  rate      F     pieces  H     tick: pieces past the first 320 | history loops' second trip (H > 320) | splice second trip (H > 256)
  192000    3840  480     827   yes                              yes (three trips)                      yes (four)
  176400    3528  441     760   yes                              yes (three)                            yes (three)
  96000     1920  240     414   -                                yes                                    yes
  88200     1764  221     380   -                                yes                                    yes
  500000   10000  1250    2152  four trips                       seven trips                            (not fed)
  32000, 24000, 16050: short histories (138, 104, 70) at up = 1, up = 2 and up = 320; a frame at 16050 is 321 samples = 642 bytes,
  so the streams' frames start 0, 2, 4, 6, 8 bytes off a 16-byte boundary.

Shapes as in tests/test_gpu_stream_rate.py: S = 5 streams, 40 ticks, stream 0 a full-scale square, one all-zero stream; the bank of
eight classes has S = 8, the bank at the staging cap S = 2 and 12 ticks (a frame is 10,000 samples)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stream_rate_pairs as P  # noqa: E402

pytestmark = pytest.mark.gpu

S, TICKS = P.S, P.TICKS
FORMS = {"crnn": ("CRNN", {}), "causal": ("Wavenet", dict(causal=True))}  # (the rate kernel is the same under every tick form)
SET_MEMBERS = ["CRNN_nosilence", "CRNN_nosilence_enhanced"]
EIGHT = [192000, 16000, 176400, 8000, 96000, 88200, 24000, 16050]  # WW_STREAM_MAX_RATES classes, one stream each


@pytest.fixture(scope="module")
def engines(assets):
    from wwhip.engine import Engine
    out = {m: Engine(os.path.join(assets, m)) for m in ["CRNN", "Wavenet"] + SET_MEMBERS}
    yield out
    for e in out.values():
        e.close()


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("rate", [192000, 176400, 96000, 88200, 32000, 24000, 16050])
def test_rate_bank_equals_the_16k_bank_given_z(engines, rate, form):
    from wwhip.engine import StreamBank
    model, kw = FORMS[form]
    eng = engines[model]
    rs = P.resampler(rate, eng.ctx)
    bank_r, bank_16 = StreamBank(eng, S, sample_rate=rate, **kw), StreamBank(eng, S, **kw)
    try:
        assert bank_r.sample_rate == rate and bank_r.frame_samples == rate // 50 and bank_16.frame_samples == 320
        seen = P.run_pair(bank_r, bank_16, rs, P.signals(rate))
        assert seen >= S * (2 * TICKS - 4)  # every stream delivered its windows: 77 rows in 40 ticks
    finally:
        bank_r.close()
        bank_16.close()


@pytest.mark.parametrize("rate", [192000, 176400])
def test_flags_freeze_and_reset(engines, rate):
    """The schedule of tests/test_gpu_stream_rate.py: stream 1 has is_speech off for ticks 10-19, stream 2 is frozen for ticks 12-17,
    stream 3 is reset after tick 20.  A young stream (held < H) with H > 320: the history's read and write-back take more than one
    trip while part of the row still reads as zero - after the start and again after the reset (H = 827 / 760 is less than a frame,
    so it is the first tick of each signal)."""
    from wwhip.engine import StreamBank
    eng = engines["CRNN"]
    rs = P.resampler(rate, eng.ctx)
    speech, active = np.ones((TICKS, S), np.uint8), np.zeros((TICKS, S), np.uint8)
    speech[10:20, 1] = 0
    active[12:18, 2] = 1
    bank_r, bank_16 = StreamBank(eng, S, sample_rate=rate, resampler=rs), StreamBank(eng, S)
    try:
        P.run_pair(bank_r, bank_16, rs, P.signals(rate), speech, active, reset_after={20: [3]})
    finally:
        bank_r.close()
        bank_16.close()


@pytest.mark.parametrize("rate", [176400, 192000])
def test_feed_at_the_banks_rate(engines, rate):
    """The five phases of tests/test_gpu_stream_rate.py's test of the same name (ticks of one stream, one sample to each, random
    packets of 1 .. 3000 samples, two ticks at a sample count that is no multiple of the frame, the last 7 samples) on a causal
    Wavenet bank: the splice kernel's keep loops at H = 760 / 827, reading the history the tick's kernel wrote and the reverse."""
    from test_gpu_stream_rate import test_feed_at_the_banks_rate as feed_phases
    if rate == 176400:
        up, down = 40, 441
        stop = rate - 2 * (rate // 50) - 7
        assert (stop * up) % down != 0  # the ticks' outputs do not start on an input sample
    feed_phases(engines, rate)


def _signal(s, rate, ticks=TICKS):
    """Stream s's int16 signal at ``rate``: stream 0 the full-scale square, stream 5 zeros, the rest a tone plus seeded noise."""
    n = ticks * (rate // 50)
    if s == 0:
        return np.where((np.arange(n) // 23) % 2 == 0, 32767, -32767).astype(np.int16)
    if s == 5:
        return np.zeros(n, np.int16)
    rng = np.random.default_rng(1000 * s + rate)
    tone = 0.25 * 32768 * np.sin(2 * np.pi * (300.0 + 170.0 * s) * np.arange(n) / rate)
    return np.clip(np.rint(tone + rng.normal(0, 0.08 * 32768, n)), -32768, 32767).astype(np.int16)


@pytest.mark.parametrize("kind", ["engine", "model_set"])
def test_eight_classes_in_one_bank(engines, kind):
    """``sample_rate=EIGHT``: the most classes a bank takes, the frames one ragged block at ``bank.frame_offs``.  Stream s equals
    stream s of the uniform bank at its own rate (the 16000 stream: of the plain bank) bit for bit - one oracle bank of 8 streams per
    rate, stream s's frames in slot s and zeros in the others.  After tick 15 ``set_rate`` swaps the 192000 and the 8000 stream;
    each goes on as a fresh stream at its new rate (the oracles reset the slot).  ``model_set``: the same on a ModelSet bank with
    the streams dealt [0, 1, 0, 1, 1, 0, 1, 0]."""
    from wwhip.engine import ModelSet, StreamBank
    n = len(EIGHT)
    ms = ModelSet([engines[m] for m in SET_MEMBERS]) if kind == "model_set" else None
    eng, kw = (ms, dict(models=[0, 1, 0, 1, 1, 0, 1, 0])) if ms is not None else (engines["CRNN"], {})
    mixed = StreamBank(eng, n, sample_rate=EIGHT, **kw)
    oracles = {R: (StreamBank(eng, n, **kw) if R == 16000 else StreamBank(eng, n, sample_rate=R, **kw)) for R in EIGHT}
    cur, seen, ones = list(EIGHT), np.zeros(n, int), np.ones(n, np.uint8)
    sig = {}
    try:
        assert len(set(EIGHT)) == 8 and mixed._mixed
        assert np.array_equal(mixed.frame_offs, np.concatenate(([0], np.cumsum([r // 50 for r in EIGHT]))))
        for t in range(TICKS):
            frames = []
            for s in range(n):
                if (s, cur[s]) not in sig:
                    sig[(s, cur[s])] = _signal(s, cur[s])
                F = cur[s] // 50
                frames.append(sig[(s, cur[s])][t * F:(t + 1) * F])
            block = np.concatenate(frames)
            assert len(block) == mixed.frame_offs[n]
            got = mixed.step(block, ones)
            for R, bank in oracles.items():
                mine = [s for s in range(n) if cur[s] == R]
                fr = np.zeros((n, R // 50), np.int16)
                for s in mine:
                    fr[s] = frames[s]
                want = bank.step(fr, ones)
                for s in mine:
                    assert got[1][s] == want[1][s], ("tick", t, "stream", s, got[1], want[1])
                    assert np.array_equal(P.bits(got[0][s]), P.bits(want[0][s])), ("tick", t, "stream", s, got[0][s], want[0][s])
                    seen[s] += int(got[1][s])
            if t == 15:
                mixed.set_rate([3], 192000)
                mixed.set_rate([0], 8000)
                cur[3], cur[0] = 192000, 8000
                for bank in oracles.values():
                    bank.reset([0, 3])
                assert np.array_equal(mixed.sample_rates, cur)
                assert np.array_equal(mixed.frame_offs, np.concatenate(([0], np.cumsum([r // 50 for r in cur]))))
        for s in range(n):
            assert np.array_equal(P.bits(mixed.window(s)), P.bits(oracles[cur[s]].window(s))), ("window of stream", s)
        assert (seen >= 2 * TICKS - 12).all(), seen  # (the two moved streams start over once: a new signal's first windows again)
    finally:
        for b in [mixed] + list(oracles.values()):
            b.close()
        if ms is not None:
            ms.close()


def test_bank_at_the_staging_cap(engines):
    """500000 Hz: up 4, down 125, half 4233, 2117 taps per output, F = 10000, D = 34, H = 2152 - 12,156 of the tick's
    WW_RATE_STAGE_MAX = 12,288 staged floats, a frame of 1,250 16-byte pieces (four trips of the piece loop), seven trips of the
    history loops.  12 ticks of 2 streams (the square, and a tone plus noise) against the 16 kHz bank given z.  510000 Hz would
    stage 12,399: refused, and ww_last_error names the count - in Python and through ww_stream_attach_resampler."""
    from wwhip import _lib
    from wwhip.engine import StreamBank
    from wwhip.resample import Resampler
    eng = engines["CRNN"]
    rate, ticks = 500000, 12
    rs = P.resampler(rate, eng.ctx)
    assert (rs.up, rs.down, rs.half, rs.taps_per_output) == (4, 125, 4233, 2117)
    x = np.stack([_signal(0, rate, ticks), _signal(1, rate, ticks)])
    bank_r, bank_16 = StreamBank(eng, 2, sample_rate=rate, resampler=rs), StreamBank(eng, 2)
    try:
        assert bank_r.frame_samples == 10000
        seen = P.run_pair(bank_r, bank_16, rs, x, ticks=ticks)
        assert seen >= 2 * (2 * ticks - 4)
    finally:
        bank_r.close()
        bank_16.close()
    with pytest.raises(ValueError, match="12399 staged samples"):
        StreamBank(eng, 2, sample_rate=510000)
    lib = _lib.load()
    r51 = Resampler(510000, 16000, eng.ctx)
    plain = StreamBank(eng, 2)
    try:
        assert lib.ww_stream_attach_resampler(plain._h, r51._h) == _lib.WW_EINVAL
        text = lib.ww_last_error(eng.ctx.handle).decode()
        assert "12399" in text and "12288" in text and "510000" in text, text
        n = C.c_int32(-1)
        assert lib.ww_stream_frame_samples(plain._h, C.byref(n)) == _lib.WW_OK and n.value == 320  # the bank is as it was
    finally:
        plain.close()
        r51.close()
