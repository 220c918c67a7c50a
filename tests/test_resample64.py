"""The resampler's float64 statement (wwhip.resample.design) against the tests' own (tests/resample64.py) and scipy, the filter's
quality in float64, StreamResampler's range arithmetic with the float64 reference in place of the kernel, and the defaults of the
entry points that refuse other rates.  No GPU."""
import os
import sys
import wave

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resample64 as R64  # noqa: E402

from wwhip import resample as RS  # noqa: E402

RATES = R64.RATES


@pytest.fixture(scope="module")
def designs():
    return {r: R64.design(r) for r in RATES}


@pytest.fixture(scope="module")
def rep_designs(designs):
    """The seven rates to 16 kHz as before, and the representatives of every class of the tile planner."""
    out = {(r, 16000): designs[r] for r in RATES}
    out.update({p: R64.design(*p) for p in R64.CLASS_REPS})
    return out


def test_design_agrees_with_the_reference_statement(designs):
    assert len(R64.PAIRS) == 132 and len(set(R64.PAIRS)) == 132
    for ri, ro in R64.PAIRS:
        up, down, half, h = RS.design(ri, ro)
        u2, d2, h2, want = designs[ri] if ro == 16000 and ri in designs else R64.design(ri, ro)
        assert (up, down, half) == (u2, d2, h2) and h.dtype == np.float64 and h.shape == want.shape == (2 * half + 1,)
        assert np.abs(h - want).max() <= 1e-15 * np.abs(want).max(), (ri, ro)
        assert RS.taps_per_output(up, half) == R64.tpp(up, half)
    table = {48000: (1, 3, 102, 205), 44100: (160, 441, 14934, 187), 8000: (2, 1, 68, 69)}
    for r, want in table.items():
        up, down, half, _ = RS.design(r, 16000)
        assert (up, down, half, RS.taps_per_output(up, half)) == want
    assert RS.design(16000, 16000)[:3] == (1, 1, 0)
    with pytest.raises(ValueError):
        RS.design(0, 16000)


def test_class_representatives_are_of_the_classes_they_stand_for(rep_designs):
    """(form, ne8, ne1, lanes1) of every pair of CLASS_REPS by the tests' own statement of the planner's arithmetic
    (tests/native/launch_plan_check.cpp holds the library's against the same table, for all 132 pairs)."""
    want = {(192000, 8000): ("decim", 0, 256, 63), (176400, 11025): ("decim", 64, 256, 100), (192000, 16000): ("decim", 64, 256, 136),
            (192000, 24000): ("decim", 128, 256, 209), (96000, 16000): ("decim", 128, 256, 256),
            (192000, 11025): ("phase", 0, 256, 0), (32000, 11025): ("phase", 0, 256, 0), (176400, 8000): ("phase", 0, 256, 0),
            (176400, 16000): ("phase", 64, 256, 0), (88200, 16000): ("phase", 128, 256, 0), (48000, 11025): ("phase", 128, 256, 0),
            (11025, 192000): ("phase", 256, 256, 0), (8000, 192000): ("phase", 256, 256, 0), (16000, 48000): ("phase", 256, 256, 0),
            (16000, 44100): ("phase", 256, 256, 0), (500000, 16000): ("phase", 0, 256, 0)}
    assert set(want) == set(R64.CLASS_REPS)
    for p in R64.CLASS_REPS:
        up, down, half, _ = rep_designs[p]
        assert R64.plan_class(up, down, half) == want[p], p
    assert rep_designs[(11025, 192000)][0] == 2560 and R64.tpp(2560, rep_designs[(11025, 192000)][2]) * 2560 == 174080
    assert rep_designs[(192000, 11025)][1] == 2560 and R64.tpp(147, rep_designs[(192000, 11025)][2]) * 147 == 173460
    assert (rep_designs[(32000, 11025)][0], rep_designs[(8000, 192000)][:2]) == (441, (24, 1))
    assert R64.tpp(4, rep_designs[(500000, 16000)][2]) == 2117


def test_direct_sum_is_scipy_resample_poly(rep_designs):
    rng = np.random.default_rng(5)
    for r, (up, down, half, h) in rep_designs.items():
        x = rng.uniform(-1, 1, 3001)
        a, b = R64.direct(x, up, down, half, h), R64.poly(x, up, down, h)
        assert a.shape == b.shape == (R64.out_len(len(x), up, down),)
        err = float(np.abs(a - b).max())
        print(f"{r}: max|direct - scipy| = {err:.2e}")
        assert err <= 1e-13, (r, err)


def test_every_phase_has_unit_dc_gain(rep_designs):
    for r, (up, down, half, h) in rep_designs.items():
        gains = np.array([h[(half + p) % up::up].sum() for p in range(up)])
        err = float(np.abs(gains - 1.0).max())
        print(f"{r}: max|DC gain - 1| = {err:.2e}")
        assert err <= 1e-7, (r, err)


def test_tones_come_out_as_the_same_tones_at_16k(designs):
    for r in RATES:
        up, down, half, h = designs[r]
        n = r // 4
        y = R64.poly(R64.tones(r, n, min(r, 16000) / 2), up, down, h)
        want = R64.tones(16000, len(y), min(r, 16000) / 2)
        edge = -(-half // down) + 1
        err = float(np.abs(y - want)[edge:len(y) - edge].max())
        print(f"{r}: tone error away from {edge} edge outputs = {err:.2e}")
        assert len(y) > 4 * edge and err <= 1e-7, (r, err)


def test_stop_band_tone_is_gone(designs):
    """The stop band starts where the Kaiser window's main lobe, centred on the cutoff rolloff * 8 kHz, has its first zero:
    sqrt(beta^2 + pi^2) / pi * L / (2 half) above the cutoff; it ends at the input's Nyquist frequency."""
    for r in RATES:
        if r <= 16000:
            continue
        up, down, half, h = designs[r]
        L = r * up
        f_stop = R64.ROLLOFF * 8000.0 + np.sqrt(R64.BETA ** 2 + np.pi ** 2) / np.pi * L / (2 * half)
        f = f_stop + 0.25 * (r / 2 - f_stop)
        x = 0.5 * np.sin(2 * np.pi * f * np.arange(r // 4) / r)
        y = R64.poly(x, up, down, h)
        edge = -(-half // down) + 1
        rel = float(np.abs(y[edge:len(y) - edge]).max() / 0.5)
        print(f"{r}: {f:.0f} Hz comes out at {rel:.2e} of its amplitude")
        assert rel <= 1e-6, (r, rel)


def test_stream_ranges_with_the_float64_reference_in_place_of_the_kernel(designs):
    rng = np.random.default_rng(11)
    for r in RATES:
        up, down, half, h = designs[r]
        x = rng.uniform(-1, 1, 40000).astype(np.float32)
        one = R64.poly(x, up, down, h)
        st = RS.StreamResampler(r, 16000, backend=lambda seg, i0, o0, n: R64.direct(seg, up, down, half, h, i0, o0, n), dtype=np.float64)
        got, pos, keep = [], 0, 0
        while pos < len(x):
            k = int(rng.integers(0, 5001))
            y = st.push(x[pos:pos + k])
            pos = min(pos + k, len(x))
            # exactly the outputs whose last input, floor((m down + half) / up), has arrived
            det = max(0, (pos * up - half - 1) // down + 1)
            assert st.n_out == det and len(y) == det - sum(len(g) for g in got)
            assert det == 0 or (det - 1) * down + half < pos * up <= det * down + half
            got.append(y)
            keep = max(keep, len(st._hist))
        got.append(st.flush())
        y = np.concatenate(got)
        assert y.shape == one.shape and np.abs(y - one).max() <= 1e-13, r
        assert keep <= 2 * -(-half // up) + -(-down // up) + 1, (r, keep)   # what the next output can still reach
        st.reset()
        assert st.n_in == 0 and st.n_out == 0 and len(st.flush()) == 0


def _wav(path, pcm, rate, channels=1):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(channels)
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(np.ascontiguousarray(pcm, np.int16).tobytes())


def test_other_rates_are_refused_unless_asked_for(tmp_path):
    from wwhip.evaluate import read_wav, read_wav_pcm, wav_length
    from wwhip.io import WavInput
    rng = np.random.default_rng(2)
    for rate, n in ((48000, 4801), (44100, 4411), (8000, 801)):
        p = str(tmp_path / f"r{rate}.wav")
        _wav(p, rng.integers(-3000, 3000, n), rate)
        for f in (read_wav, read_wav_pcm, wav_length):
            with pytest.raises(ValueError):
                f(p)
        with pytest.raises(ValueError):
            WavInput(p)
        up, down, _, _ = R64.design(rate)
        assert wav_length(p, 16000, resample=True) == R64.out_len(n, up, down) == -(-n * up // down)
        assert wav_length(p, rate) == n and len(read_wav(p, rate)) == n
