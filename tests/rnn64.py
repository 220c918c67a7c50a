"""CRNNs of either recurrent cell, any width and any head width: synthetic bundles and their float64 reading.

Host only: NumPy and ``wwhip.weights``.  ``synthetic_rnn`` builds a ``ModelBundle`` of seeded normal weights in
``geometry64.synthetic_crnn``'s scales for ``cell`` in {GRU, LSTM}, ``H`` units and a head of ``F``; ``Rnn64`` reads ``CrnnParams`` in
float64 (``weights.GruDir``'s layout: G gate blocks of H rows, z, r, h for a reset-after GRU and Keras' i, f, c, o for an LSTM, whose
one bias is ``b_x``).  ``tests/test_rnn64.py`` ties it to ``geometry64.Crnn64`` on GRU / 32 rows and to ``torch.nn.GRU`` /
``torch.nn.LSTM``; ``ROWS`` names the models ``tests/test_gpu_rnn_cells.py`` runs on the device.
"""
from __future__ import annotations

import dataclasses
from typing import Dict

import numpy as np

import geometry64 as G64
from wave_sequence64 import softmax

GRU, LSTM = 0, 1   # weights.CELL_GRU, weights.CELL_LSTM
GATES = {GRU: 3, LSTM: 4}


def _sigmoid(v):
    return 1.0 / (1.0 + np.exp(-v))


def synthetic_rnn(seed: int, cell: int, H: int, F: int, T: int, n_mel: int, C: int, KF: int, KT: int, SF: int, ST: int, same: bool,
                  n_out: int, head: int, w2_sigma: float = 0.5):
    """A CRNN bundle of seeded normal weights.  Scales (``geometry64.synthetic_crnn``'s): conv 1 / (3 sqrt(KF KT)), biases 0.1, w_x
    1 / sqrt(in), w_h 1 / sqrt(H), head w1 1 / sqrt(2H) (1 / 8 at H = 32) and w2 ``w2_sigma``."""
    from wwhip import weights as W
    rng = np.random.default_rng(seed)
    n = G64._n
    if same:
        out_f, pad_f = W._same_pad(n_mel, KF, SF)
        out_t, pad_t = W._same_pad(T, KT, ST)
    else:
        out_f, pad_f = (n_mel - KF) // SF + 1, (0, 0)
        out_t, pad_t = (T - KT) // ST + 1, (0, 0)
    g = GATES[cell]

    def direction(n_in):
        w_x, b_x, w_h, b_h = n(rng, 1 / np.sqrt(n_in), g * H, n_in), n(rng, 0.1, g * H), n(rng, 1 / np.sqrt(H), g * H, H), n(rng, 0.1, g * H)
        return W.GruDir(w_x, b_x, w_h, b_h if cell == GRU else None)   # (drawn either way: the other weights do not move with the cell)

    conv_w, conv_b = n(rng, 1 / (3 * np.sqrt(KF * KT)), C, KF, KT), n(rng, 0.1, C)
    g1 = (direction(out_f * C), direction(out_f * C))
    g2 = (direction(2 * H), direction(2 * H))
    p = W.CrnnParams(n_mel, T, conv_w, conv_b, SF, ST, pad_f, pad_t, out_f, out_t, g1, g2, n(rng, 1 / np.sqrt(2 * H), F, 2 * H), n(rng, 0.1, F),
                     n(rng, w2_sigma, n_out, F), n(rng, 0.1, n_out), head, cell)
    return W.ModelBundle(W.KIND_CRNN, G64.cut_filter(n_mel), crnn=p)


class Rnn64:
    """``CrnnParams`` in float64 for either cell: zero-padded conv + ReLU, features f * C + c, a bidirectional layer returning
    sequences (forward | backward), one returning its last states (forward's after the last row | backward's after row 0),
    Dense F ReLU, Dense n_out, sigmoid or softmax.

    GRU (Keras reset_after, gates z, r, h): ``c = tanh(x_c + r (W_h h + b_h)_c)``, ``h = z h + (1 - z) c``.
    LSTM (Keras, gates i, f, c, o; one bias, in x): ``c = f c + i tanh(.)``, ``h = o tanh(c)``."""

    def __init__(self, params) -> None:
        self.p = params
        self.cell, self.H = int(params.cell), int(params.units)
        f = lambda a: None if a is None else np.asarray(a, np.float64)
        self.conv_w, self.conv_b = f(params.conv_w), f(params.conv_b)
        self.l1 = [tuple(f(a) for a in (g.w_x, g.b_x, g.w_h, g.b_h)) for g in params.gru1]
        self.l2 = [tuple(f(a) for a in (g.w_x, g.b_x, g.w_h, g.b_h)) for g in params.gru2]
        self.w1, self.b1, self.w2, self.b2 = f(params.head_w1), f(params.head_b1), f(params.head_w2), f(params.head_b2)

    def features(self, windows: np.ndarray) -> np.ndarray:
        """``[B, T, n_mel]`` -> ``[B, OT, OF * C]`` (every patch as one row of an im2col product)."""
        p = self.p
        x = np.asarray(windows, np.float64).transpose(0, 2, 1)
        C, KF, KT = self.conv_w.shape
        need_f, need_t = (p.out_f - 1) * p.stride_f + KF, (p.out_t - 1) * p.stride_t + KT
        xp = np.zeros((x.shape[0], max(need_f, p.pad_f[0] + x.shape[1]), max(need_t, p.pad_t[0] + x.shape[2])))
        xp[:, p.pad_f[0]:p.pad_f[0] + x.shape[1], p.pad_t[0]:p.pad_t[0] + x.shape[2]] = x
        patches = np.lib.stride_tricks.sliding_window_view(xp, (KF, KT), axis=(1, 2))[:, ::p.stride_f, ::p.stride_t][:, :p.out_f, :p.out_t]
        y = np.maximum(np.einsum("bftij,cij->btfc", patches, self.conv_w) + self.conv_b, 0.0)
        return y.reshape(x.shape[0], p.out_t, p.out_f * C)

    def layer(self, seq: np.ndarray, g, reverse: bool) -> np.ndarray:
        """``seq [B, n, in]`` -> the states ``[B, n, H]`` at their rows' positions."""
        w_x, b_x, w_h, b_h = g
        H = self.H
        B, n, _ = seq.shape
        h, c = np.zeros((B, H)), np.zeros((B, H))
        out = np.empty((B, n, H))
        for t in (range(n - 1, -1, -1) if reverse else range(n)):
            xp, hp = seq[:, t] @ w_x.T + b_x, h @ w_h.T + (0.0 if b_h is None else b_h)
            if self.cell == GRU:
                z = _sigmoid(xp[:, :H] + hp[:, :H])
                r = _sigmoid(xp[:, H:2 * H] + hp[:, H:2 * H])
                h = z * h + (1.0 - z) * np.tanh(xp[:, 2 * H:] + r * hp[:, 2 * H:])
            else:
                s = xp + hp
                i, fg, o = _sigmoid(s[:, :H]), _sigmoid(s[:, H:2 * H]), _sigmoid(s[:, 3 * H:])
                c = fg * c + i * np.tanh(s[:, 2 * H:3 * H])
                h = o * np.tanh(c)
            out[:, t] = h
        return out

    def sequences(self, feat: np.ndarray) -> np.ndarray:
        return np.concatenate([self.layer(feat, self.l1[0], False), self.layer(feat, self.l1[1], True)], axis=2)

    def encode(self, windows: np.ndarray) -> np.ndarray:
        l1 = self.sequences(self.features(windows))
        return np.concatenate([self.layer(l1, self.l2[0], False)[:, -1], self.layer(l1, self.l2[1], True)[:, 0]], axis=1)

    def logits(self, enc: np.ndarray) -> np.ndarray:
        return np.maximum(np.asarray(enc, np.float64) @ self.w1.T + self.b1, 0.0) @ self.w2.T + self.b2

    def detect(self, enc: np.ndarray) -> np.ndarray:
        z = self.logits(enc)
        return softmax(z) if self.p.head_kind == 1 else _sigmoid(z)

    def forward(self, windows: np.ndarray):
        """``[B, T, n_mel]`` -> ``(post [B, n_out], enc [B, 2H])`` in float64."""
        w = np.asarray(windows)
        enc = self.encode(w.reshape((-1,) + w.shape[-2:]))
        return self.detect(enc), enc


@dataclasses.dataclass(frozen=True)
class Row:
    name: str
    args: dict
    edge: str

    def bundle(self):
        return synthetic_rnn(**self.args)

    @property
    def T(self) -> int:
        return int(self.args["T"])

    @property
    def n_mel(self) -> int:
        return int(self.args["n_mel"])


SIG, SMX = 0, 1
_STD = dict(T=151, n_mel=40, C=32, KF=5, KT=20, SF=2, ST=8, same=True)
_ONE_STEP = dict(T=6, n_mel=40, C=1, KF=40, KT=6, SF=1, ST=1, same=False)      # geometry64's c-one-step
_FEAT63 = dict(T=33, n_mel=40, C=7, KF=8, KT=4, SF=4, ST=1, same=False)         # geometry64's c-feat63
_TWO_STEPS = dict(T=7, n_mel=40, C=4, KF=40, KT=6, SF=1, ST=1, same=False)      # OT = 2: both ping-pong buffers, no middle step


def _r(name, edge, **a):
    return Row(name, a, edge)


ROWS: Dict[str, Row] = {r.name: r for r in [
    _r("gru16", "4 lanes per unit; SEQP pad of 32; GEMM N = 96", seed=301, cell=GRU, H=16, F=64, **_STD, n_out=1, head=SIG),
    _r("gru48", "idle lanes, two-wave directions; SEQP pad of 32 on 96; F = 40, 8-way softmax", seed=302, cell=GRU, H=48, F=40, **_STD, n_out=8,
       head=SMX),
    _r("gru64", "two-wave directions; the widest GRU; GEMM N = 384", seed=303, cell=GRU, H=64, F=64, **_STD, n_out=2, head=SMX),
    _r("lstm16", "4 lanes per unit, four gates; GEMM N = 128", seed=304, cell=LSTM, H=16, F=64, **_STD, n_out=2, head=SMX),
    _r("lstm32", "the shipped width with the other cell (the stream row)", seed=305, cell=LSTM, H=32, F=64, **_STD, n_out=2, head=SMX),
    _r("lstm48", "idle lanes with four gates; SEQP pad of 32 on 96", seed=306, cell=LSTM, H=48, F=64, **_STD, n_out=1, head=SIG),
    _r("lstm64", "128 weights per lane; GEMM N = 512", seed=307, cell=LSTM, H=64, F=64, **_STD, n_out=2, head=SMX),
    _r("lstm48-one-step", "1 step, 1 live feature, no prefetch", seed=308, cell=LSTM, H=48, F=64, **_ONE_STEP, n_out=1, head=SIG),
    _r("gru64-f1-feat63", "30 steps, FEATP padding, a head of one unit", seed=309, cell=GRU, H=64, F=1, **_FEAT63, n_out=2, head=SMX),
    _r("lstm64-two-steps", "2 steps: both ping-pong buffers, no middle", seed=310, cell=LSTM, H=64, F=64, **_TWO_STEPS, n_out=2, head=SMX),
]}

WINDOW_SEED = 950
N_WINDOWS = 70


def row_windows(name: str, n: int = N_WINDOWS) -> np.ndarray:
    r = ROWS[name]
    return G64.windows(WINDOW_SEED + list(ROWS).index(name), n, r.T, r.n_mel)
