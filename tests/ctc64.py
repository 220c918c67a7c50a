"""The CTC-trained CRNN (``Arik_CRNN_CTC``, reference ``wwdetect/CRNN/model.py:82-145``) in float64, and the synthetic models the
CTC tests run.  Host only: NumPy, ``geometry64`` (the conv and the GRU of ``Crnn64``) and ``wwhip.weights`` / ``wwhip.ctc``.

The model is ``Crnn64`` up to layer 1; layer 2 returns its whole sequence - row t is ``[h_fwd(t) | h_bwd(t)]``, the backward state at
t being the one after rows 18..t, as Keras' ``Bidirectional(return_sequences=True)`` concatenates them - and the detector is one
dense layer with a softmax on every row.
"""
from __future__ import annotations

import numpy as np

import geometry64 as G
from wave_sequence64 import softmax

TAU = 4e-5       # tests/test_gpu_ref64.py's constants for the same recurrences
TAU_E = 1.2e-5
N_WINDOWS = 70
WINDOW_SEED = 1900
STEPS = 19
LS = (2, 4, 8)

# Per L: (seed, w2_sigma, bias of the blank).  Chosen on the float64 reference alone (tests/test_ctc_host.py asserts the conditions):
# at most 10 % of the 70 windows undecidable, one window that decodes to two or more labels, one that decodes to none.  A head of
# sigma 0.5 on 64 states in (-1, 1) puts the classes' logits a few units apart and lets the argmax change along the 19 rows; the
# blank's bias decides how often it wins.  Decoded lengths 0, 1, 2, 3.. of the 70 windows in float64: L = 2: 7, 42, 16, 5 (one
# window undecidable); L = 4: 9, 46, 13, 2; L = 8: 12, 22, 13, 12, 6, 2, 3.
MODELS = {2: (311, 0.5, 1.0), 4: (311, 0.5, 1.0), 8: (311, 0.5, 2.0)}


class Ctc64(G.Crnn64):
    def sequence(self, windows: np.ndarray):
        """``[B, T, n_mel]`` -> ``(steps [B, 19, L], enc [B, 19, 64])`` in float64."""
        w = np.asarray(windows)
        feat = self.features(w.reshape((-1,) + w.shape[-2:]))
        l1 = np.concatenate([self._gru(feat, self.g1[0], False), self._gru(feat, self.g1[1], True)], axis=2)
        enc = np.concatenate([self._gru(l1, self.g2[0], False), self._gru(l1, self.g2[1], True)], axis=2)
        return softmax(enc @ self.w2.T + self.b2), enc


def synthetic_ctc(seed: int, L: int, w2_sigma: float = 0.5, blank_bias: float = 0.0):
    """``geometry64.synthetic_crnn`` at the standard geometry with its head swapped for a CTC head of ``L`` classes (the same draw
    of ``head_w2`` / ``head_b2``; ``blank_bias`` is added to the last class's bias)."""
    from wwhip import weights as W
    b = G.synthetic_crnn(seed=seed, **G._STD, n_out=L, head=G.SMX, w2_sigma=w2_sigma)
    bias = b.crnn.head_b2.copy()
    bias[L - 1] += np.float32(blank_bias)
    b.crnn = W.crnn_ctc_params(b.crnn, b.crnn.head_w2, bias)
    return b


def model(L: int):
    seed, sigma, blank = MODELS[L]
    return synthetic_ctc(seed, L, sigma, blank)


def windows(n: int = N_WINDOWS) -> np.ndarray:
    return G.windows(WINDOW_SEED, n, 151, 40)


def decode64(steps64: np.ndarray, max_labels=None):
    from wwhip import ctc
    return ctc.greedy_decode(steps64, max_labels)


def decidable(steps64: np.ndarray, tau: float = TAU) -> np.ndarray:
    """Per window: at each of its rows the float64 top-two posteriors differ by more than ``2 tau min(p, 1 - p)`` of the larger
    one plus 8 float32 ulps - a float32 result within ``check_posteriors``' bound of both cannot order them the other way."""
    s = np.sort(np.asarray(steps64, np.float64), axis=2)
    p1, p2 = s[:, :, -1], s[:, :, -2]
    margin = 2.0 * tau * np.minimum(p1, 1.0 - p1) + 8.0 * np.spacing(p1.astype(np.float32)).astype(np.float64)
    return np.all(p1 - p2 > margin, axis=1)


def _rows(classes, L: int, hi: float = 0.9):
    """One posterior row per entry of ``classes``: ``hi`` on that class, the rest shared among the others."""
    out = np.full((len(classes), L), (1.0 - hi) / (L - 1), np.float32)
    out[np.arange(len(classes)), classes] = hi
    return out


def hand_cases():
    """``[(name, steps [T, L], max_labels, want_labels, want_length)]``: the decode's rules one at a time (L = 4: the blank is 3)."""
    B = 3
    tie = _rows([0, 0, 0], 4)
    tie[0] = [0.1, 0.4, 0.4, 0.1]      # 1 and 2 tie: the lower index
    tie[1] = [0.25, 0.25, 0.25, 0.25]  # all four tie: class 0, not the blank
    tie[2] = [0.1, 0.1, 0.4, 0.4]      # 2 and the blank tie: 2
    distinct = _rows([k % 19 for k in range(19)], 20)   # 19 emissions, all different (L = 20: the blank never wins)
    return [
        ("all blank", _rows([B] * 19, 4), 2, [-1, -1], 0),
        ("a a blank a", _rows([1, 1, B, 1], 4), 3, [1, 1, -1], 2),
        ("repeats collapsed", _rows([0, 0, 0, 2, 2, 1, 1, 1, 1], 4), 4, [0, 2, 1, -1], 3),
        ("ties pick the lower index", tie, 3, [1, 0, 2], 3),
        ("19 emissions, two kept", distinct, 2, [0, 1], 19),
        ("one step", _rows([2], 4), 1, [2], 1),
        ("one blank step", _rows([B], 4), 1, [-1], 0),
        ("hey snips", _rows([B, 1, 1, B, B, 2, 2, B], 4), 2, [1, 2], 2),
    ]


_cache: dict = {}


def reference(L: int):
    """``(bundle, windows, steps64, enc64)`` of the L-class model, computed once per process."""
    if L not in _cache:
        b = model(L)
        w = windows()
        s, e = Ctc64(b.crnn).sequence(w)
        s.setflags(write=False)
        e.setflags(write=False)
        _cache[L] = (b, w, s, e)
    return _cache[L]
