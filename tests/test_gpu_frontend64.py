"""The HIP log-mel front ends against the float64 front end of oracle/ref64.py, element by element.

Every case checks log-mel rows with ``check_logmel`` - the error bounded relative to max(e64, floor) by an fp32 term for |X| and
the mel sum (``tau_rel``) and one for the transform that scales with the frame's 2-norm (``tau_fft``), plus an ulp of the log -
on the signal set of ``frontend_signals`` (silence, LSB dither at the floor, DC, Nyquist, fs/4, bin-centred tones, a loud tone
over +-1 LSB dither, impulses at the frame's edges, a clipped square wave, a chirp, noise, 1/f noise with formants), and keeps
the absolute rule of the other front-end tests where one applies.  Each case prints what it needed (``pytest -s``); every tau
below is about 4x the worst measured on an MI355X, quoted in the test's docstring."""
import os

import numpy as np
import pytest

from oracle import ref64 as R

pytestmark = pytest.mark.gpu

SIGNAL_SEED = 3      # tests/test_frontend64.py pins the signal set's coverage
TAU_REL = 9e-7       # precise front end: |X| and the mel sum in fp32 (measured 2.2e-7, stream windows; batch 2.0e-7)
TAU_FFT = 1e-6       # precise=False: fp32 transform, relative to the frame's 2-norm (measured 2.7e-7, stream windows; batch 1.3e-7)
TAU_STFT_REL = 5e-7  # Engine.stft_mag, precise: |X| rounded to fp32 (measured 1.2e-7)
TAU_STFT_FFT = 1.2e-5  # Engine.stft_mag, precise=False (measured 2.9e-6: a -40 dB tone at bin 129)
TOL_SWEEP = 2e-5     # the absolute rule of test_logmel_parameter_sweep_vs_oracle (precise), kept
TOL_POST = 1e-4      # the absolute posterior rule of tests/test_gpu_parity.py, kept
STREAM_TICKS = 200
CASES = [(32767.0, True, 0.0, 160), (32768.0, False, 0.0, 160), (32768.0, True, 0.0, 100), (32767.0, False, 0.0, 80),
         (30000.0, True, 0.0, 160), (1000.0, False, 0.0, 160), (32767.0, True, 0.97, 160), (32768.0, False, 0.5, 80),
         (30000.0, False, 0.97, 512), (1000.0, True, 0.5, 7)]


@pytest.fixture(scope="module")
def engines(assets):
    from wwhip.engine import Engine
    out = {m: Engine(os.path.join(assets, m)) for m in ("CRNN", "Wavenet")}
    yield out
    for e in out.values():
        e.close()


@pytest.fixture(scope="module")
def refs(assets):
    return {m: R.Ref64(os.path.join(assets, m)) for m in ("CRNN", "Wavenet")}


@pytest.fixture(scope="module")
def signals():
    return R.frontend_signals(SIGNAL_SEED)


def _logmel(case, got, ref, tau_rel, tau_fft, tol=None):
    """check_logmel with what the case needed printed; ``tol``: the absolute rule as well."""
    got = np.asarray(got, np.float64).reshape(ref.y.shape)
    need = R.needed_taus(got, ref, tau_rel if tau_fft else 0.0, 0.0)
    print(f"\nFE64 {case}: needs tau_rel {need[0]:.2e} (tau_fft 0), tau_fft {need[1]:.2e} (tau_rel {tau_rel if tau_fft else 0:g}); "
          f"max|dy| {np.abs(got - ref.y).max() if got.size else 0.0:.2e}", end="")
    ratio = R.check_logmel(got, ref, tau_rel, tau_fft)
    if tol is not None and got.size:
        assert np.abs(got - ref.y).max() < tol, case
    return ratio


# ---------------------------------------------------------------- a. Engine.logmel, precise (logmel_rows_kernel)
@pytest.mark.parametrize("case", CASES)
def test_logmel_precise_signal_set(engines, refs, signals, case):
    """The whole signal set as one ragged batch: divisors 32767 / 32768 (fast_div) and 30000 / 1000 (__fdiv_rn), clip on and
    off, pre-emphasis 0 (straight-line staging) and 0.97 / 0.5 (generic), hops 160, 100, 80, 512 and 7.  Measured: tau_rel
    2.0e-7 (pre-emphasis 0.97), max|dy| 1.05e-6.  Before the pre-emphasis was kept from contracting into one FMA (one rounding
    where the reference rounds the product and the difference) the 0.97 cases were 440-780x over this bound (3.2e-4 and 5.6e-4
    in log-mel)."""
    from wwhip.engine import frontend_params
    e, r = engines["CRNN"], refs["CRNN"]
    pcm = list(signals.values())
    got = e.logmel(pcm, frontend_params(*case, True))
    want = [r.logmel(p, *case) for p in pcm]
    for g, w, n in zip(got, want, signals):
        assert g.shape == w.y.shape, (n, g.shape, w.y.shape)
    _logmel(f"logmel precise {case}", np.concatenate(got), R.LogMel64.concat(want), TAU_REL, 0.0, TOL_SWEEP)


# ---------------------------------------------------------------- b. float input
@pytest.mark.parametrize("pre,hop", [(0.0, 160), (0.97, 160), (0.5, 100)])
def test_logmel_float_input(engines, refs, signals, pre, hop):
    """ww_logmel_f32 on the signal set scaled by 1/12000: samples up to +-2.7, not clipped on that path.  Measured: tau_rel
    1.6e-7."""
    from wwhip.engine import frontend_params
    e, r = engines["CRNN"], refs["CRNN"]
    x = [p.astype(np.float32) / np.float32(12000.0) for p in signals.values()]
    assert max(float(np.abs(v).max()) for v in x) > 2.0
    got = e.logmel(x, frontend_params(32767.0, True, pre, hop, True))
    want = R.LogMel64.concat([r.logmel_f32(v, pre, hop) for v in x])
    _logmel(f"logmel float input pre={pre} hop={hop}", np.concatenate(got), want, TAU_REL, 0.0, TOL_SWEEP)


# ---------------------------------------------------------------- c. precise=False
@pytest.mark.parametrize("case", [CASES[0], CASES[1], CASES[6], CASES[7]])
def test_logmel_fast_mode_signal_set(engines, refs, signals, case):
    """logmel_kernel<float> (fp32 Hann product and butterflies) on the signal set, with tau_fft.  The fast mode's absolute 2e-4
    rule is not applied here: an fp32 transform exceeds it legitimately on a loud tone over +-1 LSB dither.  Measured: tau_fft
    1.2e-7 (at tau_rel 5e-7), max|dy| 1.15e-3."""
    from wwhip.engine import frontend_params
    e, r = engines["CRNN"], refs["CRNN"]
    pcm = list(signals.values())
    got = np.concatenate(e.logmel(pcm, frontend_params(*case, False)))
    _logmel(f"logmel precise=False {case}", got, R.LogMel64.concat([r.logmel(p, *case) for p in pcm]), TAU_REL, TAU_FFT)


@pytest.mark.parametrize("name", ["CRNN", "Wavenet"])
def test_fast_mode_end_to_end_on_tone_and_dither(engines, refs, name):
    """The fast mode's stated guarantee (posteriors within 1e-4) where its log-mel error is largest: a 29,000-amplitude tone
    over +-1 LSB dither, 1.5 s, every fourth hop-1 window of the stream (zeros in front) against Ref64 on windows of
    Ref64.logmel rows.  Measured: max|dy| 1.3e-3, max|dp| 7.6e-7 (CRNN), 1.4e-8 (Wavenet): the guarantee holds."""
    from wwhip.engine import frontend_params
    e, r = engines[name], refs[name]
    rng = np.random.default_rng(91)
    t = np.arange(24000) / 16000.0
    pcm = np.clip(np.rint(29000.0 * np.sin(2 * np.pi * 1000.0 * t) + rng.integers(-1, 2, len(t))), -32768, 32767).astype(np.int16)
    mel = e.logmel([pcm], frontend_params(precise=False))[0]
    ref = r.logmel(pcm)
    _logmel(f"{name} tone + dither precise=False", mel, ref, TAU_REL, TAU_FFT)
    got = e.forward(R.stream_windows(mel, e.window)[::4])[:, e.posterior_index]
    want = r.forward(R.stream_windows(ref.y.astype(np.float32), e.window)[::4])[0][:, e.posterior_index]
    err = float(np.abs(got - want).max())
    print(f"\nFE64 {name} tone + dither precise=False end to end: max|dp| {err:.2e}", end="")
    assert err < TOL_POST


# ---------------------------------------------------------------- e. Engine.stft_mag
def _edge_frames(signals):
    fr = [R.frames_of(R.quantise(signals[n]), 160)[:4] for n in ("silence", "dc", "nyquist", "fs4", "tone1_full", "tone2_m40",
                                                                  "tone127_full", "tone129_m40", "tone255_full", "tone_dither",
                                                                  "square", "impulse0", "impulse1", "impulse255", "impulse256",
                                                                  "impulse510", "impulse511")]
    wide = R.frames_of(signals["square"].astype(np.float32) / np.float32(12000.0), 160)[:3]   # beyond +-1
    return np.concatenate(fr + [wide]).astype(np.float32)


def test_stft_mag_edge_frames(engines, signals):
    """Engine.stft_mag on frames of DC, Nyquist, fs/4, tones at bins 1, 2, 127, 129, 255, tone + dither, impulses at positions
    0, 1, 255, 256, 510, 511 and values beyond +-1, both modes; the absolute rules of test_stft_magnitude_vs_numpy kept.
    Measured: tau_rel 1.2e-7 (precise), tau_fft 2.9e-6 (precise=False)."""
    e = engines["CRNN"]
    frames = _edge_frames(signals)
    X = R.stft64(frames)
    want = np.abs(X)
    for precise, tr, tf in ((True, TAU_STFT_REL, 0.0), (False, 0.0, TAU_STFT_FFT)):
        got = e.stft_mag(frames, precise=precise).astype(np.float64)
        m = np.abs(got - want)
        norm = R.frame_norms(X)[:, None]
        with np.errstate(divide="ignore", invalid="ignore"):
            need_rel = float(np.where(m > 0, m / want, 0.0).max())
            need_fft = float((m / np.where(norm > 0, norm, 1.0)).max())
        print(f"\nFE64 stft_mag precise={precise}: needs tau_rel {need_rel:.2e} (alone), tau_fft {need_fft:.2e} (alone)", end="")
        R.check_stft(got, X, tr, tf)
        if precise:
            np.testing.assert_allclose(got, want.astype(np.float32), rtol=2e-6, atol=1e-9)
        else:
            assert np.abs(got - want).max() < 2e-4 * max(1.0, float(want.max()))


# ---------------------------------------------------------------- f. streaming mel rows
def _stream_plan(signals, S, ticks, seed):
    """PCM [ticks, S, 320] cut from the signal set (every stream its own order, so tick boundaries fall inside signals), VAD runs,
    active stretches and a whole-bank reset tick."""
    rng = np.random.default_rng(seed)
    names = list(signals)
    pcm = np.zeros((ticks, S, 320), np.int16)
    speech = np.zeros((ticks, S), bool)
    active = np.zeros((ticks, S), bool)
    for s in range(S):
        x = np.concatenate([signals[names[i]] for i in rng.permutation(len(names))])
        x = np.concatenate([x, x])[int(rng.integers(0, 5000)):][:ticks * 320]
        pcm[:, s] = x.reshape(ticks, 320)
        t, v = 0, True
        while t < ticks:
            n = int(rng.integers(10, 60)) if v else int(rng.integers(1, 6))
            speech[t:t + n, s] = v
            t, v = t + n, not v
        a = int(rng.integers(10, ticks - 20))
        active[a:a + int(rng.integers(2, 8)), s] = True
    return pcm, speech, active, ticks // 2 + 7


def _reference(fe, T, plan, pre, div, clip):
    """The reference's gating (oracle/numpy_ref.RefGatedStream) with the float64 front end as its mel_row, normalising with
    ``div`` / ``clip``.  Returns every stream's rows in the order they were made (LogMel64) and, per tick and stream, the
    window after the tick as (end, k): its last k rows are rows[end - k:end], the T - k in front are zero."""
    from oracle import numpy_ref
    pcm, speech, active, bank_reset = plan
    ticks, S = speech.shape
    rows = [[] for _ in range(S)]
    since = np.zeros(S, np.int64)          # rows since the stream's last reset

    def mel_row(s):
        def f(frame):
            r = fe.frame(frame)
            rows[s].append(r)
            since[s] += 1
            return r.y[0]
        return f

    keep = numpy_ref.normalise_pcm
    numpy_ref.normalise_pcm = lambda f: R.quantise(f, div, clip)   # (RefGatedStream's own: 32767, clipped)
    try:
        gs = [numpy_ref.RefGatedStream(mel_row(s), T, 40, pre_emphasis=pre) for s in range(S)]
        wins = []
        for t in range(ticks):
            if t == bank_reset:
                for g in gs:
                    g.reset()
                since[:] = 0
            for s in range(S):
                gs[s].tick(pcm[t, s], bool(speech[t, s]), bool(active[t, s]))
                if t and speech[t - 1, s] and not speech[t, s]:
                    since[s] = 0               # (the tick reset the stream on the VAD fall)
            wins.append([(len(rows[s]), int(min(T, since[s]))) for s in range(S)])
    finally:
        numpy_ref.normalise_pcm = keep
    return [R.LogMel64.concat(r) for r in rows], wins


@pytest.mark.parametrize("name", ["CRNN", "Wavenet"])
def test_stream_windows_vs_float64(engines, refs, signals, name):
    """StreamBank.window after every tick of 8 streams x 200 ticks, against the reference's gating (RefGatedStream) on the
    float64 front end: per-stream VAD runs (single-stream resets on every fall), active stretches, a whole-bank reset,
    pre-emphasis 0.97.  Forms: the default one-launch tick, two_launch (stream_frontend_kernel) and full_recompute, each precise
    and not, and two banks with divisor 32768 and clip off.  The zero rows in front of a stream's rows are exactly 0.
    Measured: tau_rel 2.2e-7 (precise), tau_fft 2.7e-7 (precise=False, the radix-4 fp32 transform of fft_device.h)."""
    from wwhip.engine import StreamBank, frontend_params
    e, r = engines[name], refs[name]
    S, T, PRE = 8, e.window, 0.97
    plan = _stream_plan(signals, S, STREAM_TICKS, 17)
    pcm, speech, active, bank_reset = plan
    forms = [dict(), dict(two_launch=True), dict(full_recompute=True)]
    banks = [(f, p, 32767.0, True) for f in forms for p in (True, False)] + [(dict(), True, 32768.0, False),
                                                                            (dict(two_launch=True), False, 32768.0, False)]
    want = {}
    for form, precise, div, clip in banks:
        if (div, clip) not in want:
            want[(div, clip)] = _reference(r.frontend, T, plan, PRE, div, clip)
        rows, wins = want[(div, clip)]
        bank = StreamBank(e, S, frontend_params(div, clip, PRE, 160, precise), **form)
        got, idx = [[] for _ in range(S)], [[] for _ in range(S)]
        try:
            for t in range(STREAM_TICKS):
                if t == bank_reset:
                    bank.reset()
                bank.step(pcm[t], speech[t].astype(np.uint8), active[t].astype(np.uint8))
                fell = np.nonzero(speech[t - 1] & ~speech[t])[0] if t else np.zeros(0, np.int64)
                if len(fell):
                    bank.reset(fell)                              # tflite.py:143-146
                for s in range(S):
                    w = bank.window(s)
                    end, k = wins[t][s]
                    assert not w[:T - k].any(), (form, precise, t, s, k)
                    got[s].append(w[T - k:])
                    idx[s].append(np.arange(end - k, end))
        finally:
            bank.close()
        g = np.concatenate([np.concatenate(x) for x in got])
        ref = R.LogMel64.concat([rows[s][np.concatenate(idx[s])] for s in range(S)])
        assert len(g) > 50 * STREAM_TICKS
        case = f"{name} stream window {form or 'one launch'} precise={precise} divisor {div:g} clip={clip}"
        _logmel(case, g, ref, TAU_REL, 0.0 if precise else TAU_FFT, TOL_SWEEP if precise else None)
