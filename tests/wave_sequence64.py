"""The Wavenet's whole-sequence reading in float64 NumPy, written from ``wwhip.weights.WavenetParams``.

For a mel sequence ``x[0..L)`` of any length: encoder rows ``e[t]`` (the skip sum), head logits ``z[t]`` (before the max over
time), the sequence posterior ``softmax(max_t z[t])`` and the frame posteriors ``pf[t] = softmax(max of z over the last P rows
up to t)`` of the reference's Keras model evaluated on the whole sequence (wwdetect/wavenet/wavenet_model.py:11-128 with
``timesteps=None``): causal taps read zeros in front of row 0 and nothing else is padded.

``tests/test_wave_sequence64.py`` pins this file against ``oracle.ref64.Ref64`` (the op-by-op reading of the flatbuffers) on
``T``-row windows, where the two readings coincide; ``tests/test_gpu_wave_sequence.py`` then holds the HIP kernels to it.
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import numpy as np

HIST = 16  # rows of a block's BatchNorm output the next chunk can reach back to (2 * dilation <= 16)


def _sigmoid(v: np.ndarray) -> np.ndarray:
    return 1.0 / (1.0 + np.exp(-v))


def softmax(v: np.ndarray) -> np.ndarray:
    e = np.exp(v - v.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


class WaveSeq64:
    def __init__(self, params) -> None:
        f = lambda a: None if a is None else np.asarray(a, np.float64)
        self.p = params
        self.T = int(params.n_frames)
        self.n_mel = int(params.n_mel)
        self.w_in, self.b_in = f(params.w_in), f(params.b_in)
        self.blocks = [dict(d=int(b.dilation), s=f(b.bn_scale), t=f(b.bn_shift), w_sig=f(b.w_sig), b_sig=f(b.b_sig),
                            w_tanh=f(b.w_tanh), b_tanh=f(b.b_tanh), w_res=f(b.w_res), b_res=f(b.b_res), w_skip=f(b.w_skip),
                            b_skip=f(b.b_skip)) for b in params.blocks]
        self.order = list(params.skip_order)
        self.w1, self.b1, self.w2, self.b2 = f(params.det_w1), f(params.det_b1), f(params.det_w2), f(params.det_b2)
        self.C = self.w_in.shape[1]
        self.n_out = self.w2.shape[1]
        self.rf = 1 + 2 * sum(b["d"] for b in self.blocks)  # receptive field: row t sees rows t - rf + 1 .. t

    def zero_history(self) -> List[np.ndarray]:
        return [np.zeros((HIST, self.C)) for _ in self.blocks]

    def rows(self, x: np.ndarray, hist: Optional[List[np.ndarray]] = None) -> Tuple[np.ndarray, np.ndarray, List[np.ndarray]]:
        """``x [n, n_mel]``: the next ``n`` rows of a sequence whose blocks' last ``HIST`` rows of BatchNorm output are ``hist``
        (``None``: the sequence starts here, zeros).  Returns ``(e [n, S], z [n, n_out], history after these rows)``."""
        x = np.asarray(x, np.float64)
        n = len(x)
        hist = self.zero_history() if hist is None else hist
        h = np.maximum(x @ self.w_in + self.b_in, 0.0)
        skips, new_hist = [], []
        for b, hb in zip(self.blocks, hist):
            d = b["d"]
            u = np.concatenate([hb, h * b["s"] + b["t"]])          # rows -HIST .. n - 1
            sig = np.zeros((n, self.C)) + b["b_sig"]
            tan = np.zeros((n, self.C)) + b["b_tanh"]
            for k in range(3):                                     # tap k reads u[t - (2 - k) d]
                tap = u[HIST - (2 - k) * d: HIST - (2 - k) * d + n]
                sig = sig + tap @ b["w_sig"][k]
                tan = tan + tap @ b["w_tanh"][k]
            g = np.tanh(tan) * _sigmoid(sig)
            if b["w_res"] is not None:
                h = np.maximum(g @ b["w_res"] + b["b_res"], 0.0) + h
            skips.append(np.maximum(g @ b["w_skip"] + b["b_skip"], 0.0))
            new_hist.append(u[-HIST:])
        e = np.zeros_like(skips[0])
        for i in self.order:
            e = e + skips[i]
        hd = np.maximum(np.maximum(e, 0.0) @ self.w1 + self.b1, 0.0)
        return e, hd @ self.w2 + self.b2, new_hist

    def chunked(self, x: np.ndarray, cuts) -> Tuple[np.ndarray, np.ndarray]:
        """``rows`` over the pieces ``x[0:c0], x[c0:c1], ...`` with the history carried from piece to piece."""
        hist, es, zs = None, [], []
        for a, b in zip([0] + list(cuts), list(cuts) + [len(x)]):
            if b > a:
                e, z, hist = self.rows(x[a:b], hist)
                es.append(e)
                zs.append(z)
        return np.concatenate(es), np.concatenate(zs)

    def pooled(self, z: np.ndarray, pool: Optional[int] = None) -> np.ndarray:
        """``m[t][c] = max of z[s][c] over max(0, t - P + 1) <= s <= t``; ``pool=None``: P = T, ``0``: from row 0."""
        P = self.T if pool is None else int(pool)
        if P == 0 or P >= len(z):
            return np.maximum.accumulate(z, axis=0)
        m = z.copy()
        for k in range(1, P):
            m[k:] = np.maximum(m[k:], z[:-k])
        return m

    def sequence(self, x: np.ndarray, pool: Optional[int] = None) -> dict:
        e, z, _ = self.rows(x)
        return {"enc": e, "logits": z, "post": softmax(z.max(axis=0)), "post_frames": softmax(self.pooled(z, pool))}
