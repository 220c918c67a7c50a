"""oracle/ref64.py pinned on the CPU: the decision windows cover each model's logit range, the fp32 C oracle meets
the float64 reference in logit space, and the logit-space check sees an error that the absolute |dp| < 1e-4 rule
does not."""
import os

import numpy as np
import pytest

from oracle import ref64 as R
from oracle.cpu import CpuOracle
from wwhip import weights as W

MODELS = ["CRNN", "CRNN_softmax", "Wavenet", "Wavenet_alt", "CRNN_nosilence", "CRNN_nosilence_enhanced", "CRNN_old"]
SEED = 7          # decision windows
STREAM_SEED = 5   # streaming input (tests/test_gpu_ref64.py uses the same)
STREAM_TICKS = 100


@pytest.fixture(scope="module")
def models(assets):
    out = {}
    for m in MODELS:
        ora = CpuOracle(W.pack_blob(W.load_model_dir(os.path.join(assets, m))))
        ref = R.Ref64(os.path.join(assets, m))
        wins = R.decision_windows(ora, ora.window, SEED)
        out[m] = (ora, ref, wins, ref.forward(wins))
    return out


@pytest.mark.parametrize("name", MODELS)
def test_decision_windows_cover_the_logit_range(models, name):
    ora, ref, wins, (out64, _) = models[name]
    lg = np.sort(R.logit(out64[:-2, -1]))   # (the all-zero and the partial window sit anywhere)
    assert lg[0] <= -8.5 and lg[-1] >= 2.5, (lg[0], lg[-1])
    assert np.diff(lg).max() <= 1.5, np.diff(lg).max()
    assert not wins[-2].any() and wins[-1, -1].sum() == 0 and wins[-1, 0].any()
    np.testing.assert_array_equal(R.decision_windows(ora, ora.window, SEED), wins)


@pytest.mark.parametrize("name", MODELS)
def test_fp32_oracle_meets_the_float64_reference(models, name):
    """measured: tau 1.3e-5 (CRNN_nosilence, logit -17), encoder 3.3e-6 (CRNN_old)."""
    ora, ref, wins, (out64, enc64) = models[name]
    out, enc = ora.forward(wins, want_enc=True)
    R.check_posteriors(out, out64, tau=2e-5)
    R.check_enc(enc, enc64, 1e-5)


@pytest.mark.parametrize("name", MODELS)
def test_a_small_logit_error_fails_the_check_but_passes_the_absolute_rule(models, name):
    """A kernel off by 1e-3 in logit fails check_posteriors(tau=1e-4) on every decision window, while the old
    |dp| < 1e-4 rule accepts it on every window where p or 1 - p is below 0.1 - most of them."""
    ora, ref, wins, (out64, _) = models[name]
    col = ora.n_out - 1
    bad = R.shift_logit(ora.forward(wins), col, 1e-3)
    assert (R.posterior_ratios(bad, out64, tau=1e-4) > 1.0).all()
    with pytest.raises(AssertionError):
        R.check_posteriors(bad, out64, tau=1e-4)
    sat = np.minimum(out64[:, col], 1.0 - out64[:, col]) < 0.1
    assert sat.sum() >= len(wins) // 2, sat.sum()
    assert (np.abs(bad - out64).max(axis=1)[sat] < 1e-4).all()


@pytest.mark.parametrize("name", ["CRNN", "Wavenet"])
def test_streaming_input_crosses_the_decision_range(models, name):
    """The PCM stream of tests/test_gpu_ref64.py: its streamed posteriors (C oracle front end, float64 model) span at
    least 6 logit units; delayed by whole ticks it gives all-zero mel rows followed by the same rows, so that streams
    offset in time share their windows."""
    ora, ref = models[name][:2]
    pcm = R.decision_stream(ora, STREAM_TICKS * 320, STREAM_SEED)
    np.testing.assert_array_equal(R.decision_stream(ora, STREAM_TICKS * 320, STREAM_SEED), pcm)
    mel = ora.logmel(pcm)
    wins = R.stream_windows(mel, ora.window)
    assert len(wins) == len(mel)
    np.testing.assert_array_equal(wins[-1], mel[-ora.window:])
    out64, _ = ref.forward(wins)
    lg = R.logit(out64[:, -1])
    assert lg.max() - lg.min() >= 6.0, (lg.min(), lg.max())
    for d in (1, 3):
        late = ora.logmel(np.concatenate([np.zeros(d * 320, np.int16), pcm])[:len(pcm)])
        assert not late[:2 * d].any()
        np.testing.assert_array_equal(late[2 * d:], mel[:len(late) - 2 * d])


def test_checks_on_hand_made_rows():
    want = np.array([[0.5], [1e-6], [1.0 - 2.0 ** -20]])
    assert R.check_posteriors(want, want, 1e-5) == 0.0
    got = want.copy()
    got[1] *= 1.0 + 5e-6                                   # relative error 5e-6 of the tail probability
    assert R.check_posteriors(got, want, 1e-5, ulps=0) == pytest.approx(0.5, rel=1e-6)
    with pytest.raises(AssertionError):
        R.check_posteriors(got, want, 4e-6)
    got = want.copy()
    got[2] += 3 * 2.0 ** -24                               # three fp32 ulps below 1: the ulps term
    R.check_posteriors(got, want, 1e-9)
    with pytest.raises(AssertionError):
        R.check_posteriors(got, want, 1e-9, ulps=2)
    assert R.needed_tau(got, want, ulps=0) == pytest.approx(3 * 2.0 ** -24 / 2.0 ** -20)
    enc = np.array([[0.5, -3.0], [0.1, 0.2]])
    e2 = enc + np.array([[2.9e-5, 0.0], [0.0, 9e-6]])
    assert R.check_enc(e2, enc, 1e-5) == pytest.approx(0.9667, rel=1e-3)   # row 0: 2.9e-5 / (1e-5 * 3)
    with pytest.raises(AssertionError):
        R.check_enc(e2, enc, 8e-6)
