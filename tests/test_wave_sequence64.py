"""The float64 whole-sequence evaluation of the Wavenet (tests/wave_sequence64.py), pinned against what already exists.

The sequence form (``Engine.sequence_forward``, ``StreamBank(causal=True)``) reads the reference's Wavenet as its trainer builds
it with ``timesteps=None``: one causal, fully convolutional pass over a sequence of any length.  Its yardstick is a float64 NumPy
evaluation written from ``WavenetParams``; these tests tie that yardstick to ``oracle.ref64.Ref64`` - the op-by-op reading of
the flatbuffers, which shares nothing with the product's weight extraction - and document the chunking scheme of the kernel.
No GPU and no native library: this is the yardstick, not the proof of the feature (tests/test_gpu_wave_sequence.py is).
"""
import os

import numpy as np
import pytest

from oracle import ref64 as R
from wave_sequence64 import HIST, WaveSeq64, softmax

MODELS = ["Wavenet", "Wavenet_alt"]
TOL = 1e-12


def mel_sequence(rng, rows, n_mel=40):
    """Seeded stand-in for log-mel rows: slowly varying band energies plus noise, floor-clipped like the front end's."""
    base = np.cumsum(rng.normal(0, 0.15, (rows, n_mel)), axis=0)
    base -= base.mean(axis=0)
    return np.maximum(base + rng.normal(0, 0.5, (rows, n_mel)), -2.0).astype(np.float32)


@pytest.fixture(scope="module", params=MODELS)
def pair(request, assets):
    from wwhip import weights as W
    d = os.path.join(assets, request.param)
    return WaveSeq64(W.load_model_dir(d).wavenet), R.Ref64(d)


def test_receptive_field_is_181_rows(pair):
    seq, _ = pair
    assert seq.rf == 181 and seq.T == 182 and max(2 * b["d"] for b in seq.blocks) <= HIST


def test_a_window_is_the_window_form(pair):
    """On T-row windows the whole-sequence reading IS the window form: encoder rows and posteriors agree with Ref64.forward to
    <= 1e-12 (measured 1.3e-15 / 2.2e-16)."""
    seq, ref = pair
    rng = np.random.default_rng(11)
    wins = np.stack([mel_sequence(rng, seq.T) for _ in range(4)] + [np.zeros((seq.T, 40), np.float32)])
    out64, enc64 = ref.forward(wins)
    for w, o, e in zip(wins, out64, enc64):
        got = seq.sequence(w)
        de, dp = np.abs(got["enc"] - e).max(), np.abs(got["post"] - o).max()
        print(f"\nwindow: enc {de:.2e} post {dp:.2e}", end="")
        assert de <= TOL and dp <= TOL
        # P = T over T rows pools the whole window: the last frame posterior is the window's posterior
        assert np.abs(got["post_frames"][-1] - o).max() <= TOL


def test_a_late_row_is_the_last_row_of_the_window_that_ends_there(pair):
    """Row t >= T - 1 of a long sequence against position T - 1 of the window ending at t (that position's cone, RF = 181 rows,
    never reaches the window's pad): <= 1e-12 (measured 0)."""
    seq, ref = pair
    x = mel_sequence(np.random.default_rng(12), 600)
    e, _, _ = seq.rows(x)
    for t in (seq.T - 1, seq.T, 300, 455, 599):
        _, enc64 = ref.forward(x[t - seq.T + 1:t + 1][None])
        d = np.abs(e[t] - enc64[0][seq.T - 1]).max()
        print(f"\nrow {t}: {d:.2e}", end="")
        assert d <= TOL
    # and an early row is NOT the window form's (the window pads its own left edge): the two readings differ by construction
    _, enc64 = ref.forward(np.concatenate([x[50:60], np.zeros((seq.T - 10, 40), np.float32)])[None])
    assert np.abs(e[59] - enc64[0][9]).max() > 1e-3


@pytest.mark.parametrize("pool", [None, 0, 1, 7])
def test_frame_posteriors_against_a_literal_loop(pair, pool):
    seq, _ = pair
    x = mel_sequence(np.random.default_rng(13), 400)
    got = seq.sequence(x, pool)
    z = got["logits"]
    P = seq.T if pool is None else pool
    for t in range(len(z)):
        lo = 0 if P == 0 else max(0, t - P + 1)
        m = np.array([max(z[s][c] for s in range(lo, t + 1)) for c in range(seq.n_out)])
        assert np.array_equal(got["post_frames"][t], softmax(m)), t
    if pool == 0:
        assert np.array_equal(got["post"], got["post_frames"][-1])


def test_chunks_with_carried_history_are_the_one_piece_evaluation(pair):
    """The kernel's scheme before anyone runs it: rows in chunks, each block's last 16 rows of BatchNorm output carried in place
    of the causal zero rows.  Equal to the one-piece evaluation to <= 1e-12 wherever the chunk borders fall (not exactly: BLAS
    may sum differently for different row counts)."""
    seq, _ = pair
    x = mel_sequence(np.random.default_rng(14), 700)
    e, z, _ = seq.rows(x)
    for cuts in ([192, 384, 576], [16, 32, 48], [1, 2, 3, 5, 8, 200], [181, 182, 183], [350]):
        ec, zc = seq.chunked(x, cuts)
        d = max(np.abs(ec - e).max(), np.abs(zc - z).max())
        print(f"\ncuts {cuts[:4]}..: {d:.2e}", end="")
        assert d <= TOL
    # one row at a time, as a stream advances it
    ec, zc = seq.chunked(x[:300], list(range(1, 300)))
    assert max(np.abs(ec - e[:300]).max(), np.abs(zc - z[:300]).max()) <= TOL


def test_a_segment_needs_rf_minus_one_rows_of_warm_up(pair):
    """A segment cut out of the middle of a sequence and started RF - 1 rows early from an all-zero history reproduces the rows
    it keeps: how the kernel cuts a long sequence into segments that run in parallel."""
    seq, _ = pair
    x = mel_sequence(np.random.default_rng(15), 900)
    e, z, _ = seq.rows(x)
    s0 = 517
    ew, zw, _ = seq.rows(x[s0 - (seq.rf - 1):])
    assert max(np.abs(ew[seq.rf - 1:] - e[s0:]).max(), np.abs(zw[seq.rf - 1:] - z[s0:]).max()) <= TOL
