"""The float64 log-mel front end of oracle/ref64.py pinned on the CPU: the signal set covers where a front end goes wrong, the
float64 front end is the reference's framing restated, the fp32 C oracle meets it at the precise tolerance, and that tolerance
sees defects the absolute rules of the other front-end tests let through."""
import os

import numpy as np
import pytest

from oracle import ref64 as R
from oracle.cpu import CpuOracle
from oracle.numpy_ref import RefFilter
from wwhip import weights as W

SIGNAL_SEED = 3       # tests/test_gpu_frontend64.py uses the same
TAU_REL = 5e-7        # precise front end: |X| and the mel sum in fp32 (C oracle measured 1.2e-7)
TAU_FFT32 = 2e-7      # an fp32 Hann product and transform, relative to the frame's 2-norm (NumPy complex64 measured 4.6e-8)
TOL_MEL = 1e-4        # the absolute rule of tests/test_gpu_parity.py (golden clips)
TOL_SWEEP = 2e-5      # the absolute rule of test_logmel_parameter_sweep_vs_oracle (noise)
CASES = [(32767.0, True, 0.0, 160), (32768.0, False, 0.0, 160), (32767.0, True, 0.97, 160), (30000.0, True, 0.0, 160),
         (32768.0, False, 0.5, 80), (32767.0, False, 0.0, 200), (32767.0, True, 0.0, 512), (1000.0, True, 0.3, 37)]


@pytest.fixture(scope="module")
def crnn(assets):
    d = os.path.join(assets, "CRNN")
    return R.Ref64(d), CpuOracle(W.pack_blob(W.load_model_dir(d)))


@pytest.fixture(scope="module")
def signals():
    return R.frontend_signals(SIGNAL_SEED)


def _set(ref, signals, case):
    return R.LogMel64.concat([ref.logmel(p, *case) for p in signals.values()])


def _variant(ref, pcm, case, fft32=False):
    """A front end with the Hann product in fp32 (and, with ``fft32``, the transform as well), from the same float32 samples."""
    div, clip, pre, hop = case
    fr = R.frames_of(R.preemphasise(R.quantise(pcm, div, clip), pre), hop)
    hx = fr.astype(np.float32) * R.HANN64.astype(np.float32)
    X = np.fft.rfft(hx, axis=1) if fft32 else np.fft.rfft(hx.astype(np.float64), axis=1)
    return R.mel64(ref.frontend.filt, np.abs(X).astype(np.float64), R.frame_norms(R.stft64(fr))).y


def test_signal_set_covers_the_edges(crnn, signals):
    """At the hop-160 grid with divisor 32767: hundreds of bands just above the floor, rows whose bands span more than 1e5,
    bins 0, 128 and 256 each the loudest of some row, and clipping."""
    ref = crnn[0]
    r = _set(ref, signals, CASES[0])
    fl = r.floor
    near = (r.e > fl) & (r.e < 4 * fl)
    assert near.sum() >= 300, near.sum()
    span = r.e.max(axis=1) / np.maximum(r.e.min(axis=1), fl)
    assert (span >= 1e5).sum() >= 20, (span >= 1e5).sum()
    loud = np.argmax(r.mag, axis=1)
    for k in (0, 128, 256):
        assert (loud == k).sum() >= 3, k
    pcm = np.concatenate(list(signals.values()))
    assert (pcm == -32768).sum() >= 100
    assert (R.quantise(pcm, 32767.0, False) < -1.0).any() and not (R.quantise(pcm, 32768.0, False) < -1.0).any()
    assert np.array_equal(R.frontend_signals(SIGNAL_SEED)["pink_formants"], signals["pink_formants"])


@pytest.mark.parametrize("case", CASES[:3] + CASES[4:5] + CASES[7:])
def test_logmel64_is_the_reference_filter_in_float64(crnn, signals, case):
    """RefFilter (the reference's per-sample ring, pre-emphasis carried across 320-sample chunks, the hop) feeding float64
    |X| to the filter graph evaluated in float64 gives Ref64.logmel's rows to 1e-12."""
    ref = crnn[0]
    div, clip, pre, hop = case

    class Filter64(RefFilter):
        def stft_mag(self):
            return np.abs(np.fft.rfft(self.sample_window.read_all() * self._fft_window, n=512))

    for name in ("tone_dither", "impulse1", "square", "pink_formants", "dc"):
        pcm = signals[name]
        f = Filter64(lambda m: ref.m.filter(m)[0], pre_emphasis=pre)
        f.hop_length = hop
        f._prev_sample = np.float32(0.0)
        x = R.quantise(pcm, div, clip)
        rows = []
        for i in range(0, len(x), 320):
            rows += f.filter_frame(x[i:i + 320].copy())
        want = ref.logmel(pcm, *case).y
        assert len(rows) == len(want), name
        assert np.abs(np.array(rows) - want).max() < 1e-12, name


@pytest.mark.parametrize("case", CASES)
def test_c_oracle_meets_the_precise_bound(crnn, signals, case):
    """The fp32 C oracle (fp64 transform, fp32 |X|, fp32 mel sum, logf) on every case of the GPU parameter sweep, with one ulp
    of the log (glibc's logf; the GPU's needs two): worst
    tau_rel 1.2e-7 (divisor 32768, pre-emphasis 0.5, hop 80).  Before its pre-emphasis was kept from contracting into an FMA it
    needed 7.5e-4 at pre-emphasis 0.97 (3.8e-4 in log-mel, the pre-emphasised DC clip)."""
    ref, ora = crnn
    r = _set(ref, signals, case)
    got = np.concatenate([ora.logmel(p, *case) for p in signals.values()])
    print(f"\nFE64 C oracle {case}: needs tau_rel {R.needed_taus(got, r, ulps=1)[0]:.2e}", end="")
    R.check_logmel(got, r, TAU_REL, 0.0, ulps=1)


def test_c_oracle_float_input(crnn, signals):
    """logmel_f32 on samples beyond +-1 (not clipped on that path) with pre-emphasis."""
    ref, ora = crnn
    for name in ("square", "tone_dither", "chirp", "impulse256"):
        x = signals[name].astype(np.float32) / np.float32(12000.0)
        R.check_logmel(ora.logmel_f32(x, 0.97, 160), ref.logmel_f32(x, 0.97, 160), TAU_REL, 0.0)


def test_fp32_hann_product_fails_the_precise_check_but_passes_the_absolute_rules(crnn, signals, golden):
    """The Hann product in fp32 instead of fp64: within 1e-4 of float64 on the golden clips and within 2e-5 on noise, yet more
    than 100x the precise bound on the signal set (the loud tone plus +-1 LSB dither)."""
    ref = crnn[0]
    z = np.load(os.path.join(golden, "frontend.npz"))
    for n in ("noise_chirp", "quiet", "silence", "fullscale", "ragged"):
        pcm = z[n + ".pcm"]
        assert np.abs(_variant(ref, pcm, CASES[0]) - ref.logmel(pcm).y).max() < TOL_MEL, n
    noise = np.clip(np.random.default_rng(57).normal(0, 4000, 24000), -32768, 32767).astype(np.int16)
    assert np.abs(_variant(ref, noise, CASES[0]) - ref.logmel(noise).y).max() < TOL_SWEEP
    r = _set(ref, signals, CASES[0])
    bad = np.concatenate([_variant(ref, p, CASES[0]) for p in signals.values()])
    assert R.logmel_ratios(bad, r, TAU_REL, 0.0).max() > 100.0
    with pytest.raises(AssertionError):
        R.check_logmel(bad, r, TAU_REL, 0.0)


@pytest.mark.parametrize("case", [CASES[0], CASES[2], CASES[4]])
def test_fp32_transform_fails_the_precise_check_but_passes_the_fast_mode_check(crnn, signals, case):
    """An fp32 Hann product and transform (NumPy's complex64 rfft) is what the fast mode does: it meets tau_fft = TAU_FFT32
    (measured 4.6e-8), so that tau is sized for legitimate fp32 error, and it fails the precise check."""
    ref = crnn[0]
    r = _set(ref, signals, case)
    fast = np.concatenate([_variant(ref, p, case, fft32=True) for p in signals.values()])
    print(f"\nFE64 fp32 transform {case}: needs tau_fft {R.needed_taus(fast, r, TAU_REL, 0.0)[1]:.2e}", end="")
    R.check_logmel(fast, r, TAU_REL, TAU_FFT32)
    assert R.logmel_ratios(fast, r, TAU_REL, 0.0).max() > 10.0


def test_checks_on_hand_made_rows():
    fl, sc = 1e-5, 0.5
    e = np.array([[1.0, 2e-5, 1e-7]])
    y = (np.log(np.maximum(e, fl)) + 11.5) * sc
    ref = R.LogMel64(y, e, e.copy(), np.full_like(e, 100.0), fl, sc, np.zeros((1, 257)), np.ones(1))
    assert R.check_logmel(y, ref, 1e-7, 0.0) == 0.0
    got = y.copy()
    got[0, 1] += sc * 3e-6 * 2e-5 / 2e-5           # 3e-6 relative in the energy of a band at twice the floor
    assert R.needed_taus(got, ref, ulps=0)[0] == pytest.approx(3e-6, rel=1e-6)
    assert R.needed_taus(got, ref, ulps=0)[1] == pytest.approx(3e-6 * 2e-5 / 100.0, rel=1e-6)
    with pytest.raises(AssertionError):
        R.check_logmel(got, ref, 1e-6, 0.0, ulps=0)
    got = y.copy()
    got[0, 2] += 2.0 * sc * np.spacing(np.float32(abs(np.log(fl))))   # below the floor: two ulps of ln(floor)
    R.check_logmel(got, ref, 0.0, 0.0, ulps=2)
    with pytest.raises(AssertionError):
        R.check_logmel(got, ref, 0.0, 0.0, ulps=1)
    X = np.fft.rfft(np.hanning(512) * np.cos(2 * np.pi * 5 * np.arange(512) / 512))[None]
    m = np.abs(X) + 1e-9
    assert R.check_stft(m, X, 0.0, 2e-9 / R.frame_norms(X)[0]) == pytest.approx(0.5, rel=1e-3)
    with pytest.raises(AssertionError):
        R.check_stft(m, X, 0.0, 0.9e-9 / R.frame_norms(X)[0])
