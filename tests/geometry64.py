"""Model geometries the loader accepts but no shipped model has: synthetic bundles, their float64 readings, and the table of them.

Host only: NumPy and ``wwhip.weights`` (no torch, no native library at module level).  ``synthetic_crnn`` / ``synthetic_wavenet``
build a ``ModelBundle`` of seeded normal weights at any geometry ``ww_model_load`` (csrc/model_pack.h) takes; ``Crnn64`` is the
CRNN in float64 written from ``CrnnParams`` (the Wavenet's is ``wave_sequence64.WaveSeq64``: on exactly T rows its sequence
reading is the window form); ``engine_for`` puts a bundle on the device; ``GEOMETRIES`` names the rows every test walks.
``tests/test_geometry64.py`` ties ``Crnn64`` to ``oracle.ref64.Ref64`` on the shipped models and every row to the C oracle, which
parses the blob by section name in C and shares nothing with this file.
"""
from __future__ import annotations

import dataclasses
import os
from typing import Dict, Optional, Sequence

import numpy as np

from wave_sequence64 import WaveSeq64, softmax

_ASSETS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "wakeword-detection_amd", "assets", "tf_lite_models")
H = 32   # GRU units (the loader takes no other)
WC = 16  # Wavenet channels
WS = 32  # Wavenet skip channels

_filter_cache: dict = {}


def cut_filter(n_mel: int):
    """The shipped ``Wavenet`` directory's filter cut to its first ``n_mel`` bands."""
    from wwhip import weights as W
    if "full" not in _filter_cache:
        _filter_cache["full"] = W.load_model_dir(os.path.join(_ASSETS, "Wavenet")).filt
    f = _filter_cache["full"]
    return dataclasses.replace(f, weight=np.ascontiguousarray(f.weight[:n_mel]), bias=np.ascontiguousarray(f.bias[:n_mel]))


def _n(rng, sigma, *shape):
    return (sigma * rng.normal(size=shape)).astype(np.float32)


def synthetic_crnn(seed: int, T: int, n_mel: int, C: int, KF: int, KT: int, SF: int, ST: int, same: bool, n_out: int, head: int,
                   w2_sigma: float = 0.5):
    """A CRNN bundle of seeded normal weights, H = 32.  Scales: conv 1 / (3 sqrt(KF KT)), biases 0.1, GRU w_x 1 / sqrt(in) and
    w_h 1 / sqrt(32), head w1 1 / 8 and w2 ``w2_sigma``."""
    from wwhip import weights as W
    rng = np.random.default_rng(seed)
    if same:
        out_f, pad_f = W._same_pad(n_mel, KF, SF)
        out_t, pad_t = W._same_pad(T, KT, ST)
    else:
        out_f, pad_f = (n_mel - KF) // SF + 1, (0, 0)
        out_t, pad_t = (T - KT) // ST + 1, (0, 0)

    def gru(n_in):
        return W.GruDir(_n(rng, 1 / np.sqrt(n_in), 3 * H, n_in), _n(rng, 0.1, 3 * H), _n(rng, 1 / np.sqrt(H), 3 * H, H), _n(rng, 0.1, 3 * H))

    conv_w, conv_b = _n(rng, 1 / (3 * np.sqrt(KF * KT)), C, KF, KT), _n(rng, 0.1, C)
    g1 = (gru(out_f * C), gru(out_f * C))
    g2 = (gru(2 * H), gru(2 * H))
    p = W.CrnnParams(n_mel, T, conv_w, conv_b, SF, ST, pad_f, pad_t, out_f, out_t, g1, g2,
                     _n(rng, 1 / 8, 2 * H, 2 * H), _n(rng, 0.1, 2 * H), _n(rng, w2_sigma, n_out, 2 * H), _n(rng, 0.1, n_out), head)
    return W.ModelBundle(W.KIND_CRNN, cut_filter(n_mel), crnn=p)


def synthetic_wavenet(seed: int, T: int, n_mel: int, dilations: Sequence[int], has_res: Sequence[bool], n_out: int,
                      w2_sigma: float = 0.5, skip_bias_mean: float = 0.0):
    """A Wavenet bundle of seeded normal weights, C = 16, S = 32, skips summed in block order.  Scales: w_in 0.15 (bias 0.2),
    BatchNorm scale 1 + 0.2 N and shift 0.2, gates 0.25 (biases 0.3), res and skip 0.3 (biases 0.1), det_w1 0.2 / sqrt(NB),
    det_w2 ``w2_sigma``.  ``skip_bias_mean`` lifts the skip biases: with ONE block the encoder output is the ReLU of one zero-mean
    row, half zeros by construction."""
    from wwhip import weights as W
    rng = np.random.default_rng(seed)
    nb = len(dilations)
    assert len(has_res) == nb
    w_in, b_in = _n(rng, 0.15, n_mel, WC), _n(rng, 0.2, WC)
    blocks = []
    for d, res in zip(dilations, has_res):
        bn_s, bn_t = (1.0 + 0.2 * rng.normal(size=WC)).astype(np.float32), _n(rng, 0.2, WC)
        w_sig, b_sig, w_tanh, b_tanh = _n(rng, 0.25, 3, WC, WC), _n(rng, 0.3, WC), _n(rng, 0.25, 3, WC, WC), _n(rng, 0.3, WC)
        w_res, b_res = _n(rng, 0.3, WC, WC), _n(rng, 0.1, WC)   # (drawn either way: the other weights do not move with has_res)
        w_skip, b_skip = _n(rng, 0.3, WC, WS), _n(rng, 0.1, WS) + np.float32(skip_bias_mean)
        blocks.append(W.WaveBlock(int(d), bn_s, bn_t, w_sig, b_sig, w_tanh, b_tanh, w_res if res else None, b_res if res else None,
                                  w_skip, b_skip))
    p = W.WavenetParams(T, n_mel, w_in, b_in, blocks, list(range(nb)), _n(rng, 0.2 / np.sqrt(nb), WS, WS), _n(rng, 0.1, WS),
                        _n(rng, w2_sigma, WS, n_out), _n(rng, 0.1, n_out))
    return W.ModelBundle(W.KIND_WAVENET, cut_filter(n_mel), wavenet=p)


def windows(seed: int, n: int, T: int, n_mel: int) -> np.ndarray:
    """``[n, T, n_mel]`` float32 stand-ins for log-mel windows: a random walk over time (sigma 0.15) plus noise (sigma 0.7) around
    2.5, clipped to [0, 6.5]."""
    rng = np.random.default_rng(seed)
    walk = np.cumsum(rng.normal(0, 0.15, (n, T, n_mel)), axis=1)
    return np.clip(2.5 + walk + rng.normal(0, 0.7, (n, T, n_mel)), 0.0, 6.5).astype(np.float32)


def _sigmoid(v):
    return 1.0 / (1.0 + np.exp(-v))


class Crnn64:
    """``CrnnParams`` in float64: zero-padded conv + ReLU, features f * C + c, BiGRU (sequences: forward | backward), BiGRU (last
    states: forward's after the last row | backward's after row 0), Dense 64 ReLU, Dense n_out, sigmoid or softmax.  GRU gates are
    Keras ``reset_after`` in the order z, r, h: ``c = tanh(x_c + r (W_h h + b_h)_c)``, ``h = z h + (1 - z) c``."""

    def __init__(self, params) -> None:
        self.p = params
        f = lambda a: np.asarray(a, np.float64)
        self.conv_w, self.conv_b = f(params.conv_w), f(params.conv_b)
        self.g1 = [tuple(f(a) for a in (g.w_x, g.b_x, g.w_h, g.b_h)) for g in params.gru1]
        self.g2 = [tuple(f(a) for a in (g.w_x, g.b_x, g.w_h, g.b_h)) for g in params.gru2]
        self.w1, self.b1, self.w2, self.b2 = f(params.head_w1), f(params.head_b1), f(params.head_w2), f(params.head_b2)

    def features(self, windows: np.ndarray) -> np.ndarray:
        """``[B, T, n_mel]`` -> ``[B, OT, OF * C]``."""
        p = self.p
        x = np.asarray(windows, np.float64).transpose(0, 2, 1)   # [B, mel, frames]
        C, KF, KT = self.conv_w.shape
        need_f, need_t = (p.out_f - 1) * p.stride_f + KF, (p.out_t - 1) * p.stride_t + KT
        xp = np.zeros((x.shape[0], max(need_f, p.pad_f[0] + x.shape[1]), max(need_t, p.pad_t[0] + x.shape[2])))
        xp[:, p.pad_f[0]:p.pad_f[0] + x.shape[1], p.pad_t[0]:p.pad_t[0] + x.shape[2]] = x
        out = np.empty((x.shape[0], p.out_t, p.out_f, C))
        for of in range(p.out_f):
            for ot in range(p.out_t):
                patch = xp[:, of * p.stride_f:of * p.stride_f + KF, ot * p.stride_t:ot * p.stride_t + KT]
                out[:, ot, of] = np.maximum(np.einsum("bft,cft->bc", patch, self.conv_w) + self.conv_b, 0.0)
        return out.reshape(x.shape[0], p.out_t, p.out_f * C)

    @staticmethod
    def _gru(seq: np.ndarray, g, reverse: bool) -> np.ndarray:
        """``seq [B, n, in]`` -> the states ``[B, n, H]`` at their rows' positions."""
        w_x, b_x, w_h, b_h = g
        B, n, _ = seq.shape
        h = np.zeros((B, H))
        out = np.empty((B, n, H))
        for t in (range(n - 1, -1, -1) if reverse else range(n)):
            xp, hp = seq[:, t] @ w_x.T + b_x, h @ w_h.T + b_h
            z = _sigmoid(xp[:, :H] + hp[:, :H])
            r = _sigmoid(xp[:, H:2 * H] + hp[:, H:2 * H])
            c = np.tanh(xp[:, 2 * H:] + r * hp[:, 2 * H:])
            h = z * h + (1.0 - z) * c
            out[:, t] = h
        return out

    def encode(self, windows: np.ndarray) -> np.ndarray:
        feat = self.features(windows)
        l1 = np.concatenate([self._gru(feat, self.g1[0], False), self._gru(feat, self.g1[1], True)], axis=2)
        return np.concatenate([self._gru(l1, self.g2[0], False)[:, -1], self._gru(l1, self.g2[1], True)[:, 0]], axis=1)

    def logits(self, enc: np.ndarray) -> np.ndarray:
        return np.maximum(np.asarray(enc, np.float64) @ self.w1.T + self.b1, 0.0) @ self.w2.T + self.b2

    def detect(self, enc: np.ndarray) -> np.ndarray:
        z = self.logits(enc)
        return softmax(z) if self.p.head_kind == 1 else _sigmoid(z)

    def forward(self, windows: np.ndarray):
        """``[B, T, n_mel]`` -> ``(post [B, n_out], enc [B, 64])`` in float64."""
        w = np.asarray(windows)
        enc = self.encode(w.reshape((-1,) + w.shape[-2:]))
        return self.detect(enc), enc


class Wave64:
    """The Wavenet's window form on ``WaveSeq64``: a T-row window is a T-row sequence."""

    def __init__(self, params) -> None:
        self.seq = WaveSeq64(params)

    def forward(self, windows: np.ndarray):
        """``[B, T, n_mel]`` -> ``(post [B, n_out], enc [B, T, S])`` in float64."""
        got = [self.seq.sequence(w) for w in np.asarray(windows).reshape((-1, self.seq.T, self.seq.n_mel))]
        return np.array([g["post"] for g in got]), np.array([g["enc"] for g in got])

    def logits(self, windows: np.ndarray) -> np.ndarray:
        return np.array([self.seq.sequence(w)["logits"] for w in np.asarray(windows).reshape((-1, self.seq.T, self.seq.n_mel))])

    def detect(self, enc: np.ndarray) -> np.ndarray:
        """``[n, T, S]`` encoder rows -> ``[n, n_out]``: the head on every row, the max over time, softmax."""
        s = self.seq
        e = np.asarray(enc, np.float64)
        z = np.maximum(np.maximum(e, 0.0) @ s.w1 + s.b1, 0.0) @ s.w2 + s.b2
        return softmax(z.max(axis=1))


def reference(bundle):
    """The float64 reading of a bundle: an object with ``forward(windows) -> (post, enc)`` and ``detect(enc)``."""
    return Crnn64(bundle.crnn) if bundle.crnn is not None else Wave64(bundle.wavenet)


def blob_of(bundle, seed: int = 77) -> bytes:
    """``pack_blob(bundle)``, except that a Wavenet block WITHOUT a residual conv carries seeded non-zero ``w_res`` / ``b_res``
    behind its ``has_res`` = 0 (``pack_blob`` writes zeros there): a kernel that applied the conv regardless would add zeros and go
    unnoticed.  The flag decides, not the weights - the float64 reading and the C oracle skip the conv."""
    from wwhip import weights as W
    if bundle.wavenet is None or all(b.w_res is not None for b in bundle.wavenet.blocks):
        return W.pack_blob(bundle)
    rng = np.random.default_rng(seed)
    w = bundle.wavenet
    blocks = [b if b.w_res is not None else dataclasses.replace(b, w_res=_n(rng, 0.3, WC, WC), b_res=_n(rng, 0.1, WC) + np.float32(0.2))
              for b in w.blocks]
    blob = bytearray(W.pack_blob(dataclasses.replace(bundle, wavenet=dataclasses.replace(w, blocks=blocks))))
    flags = np.array([b.w_res is not None for b in w.blocks], np.int32).tobytes()
    n = int(np.frombuffer(blob, np.uint32, 1, 12)[0])
    for i in range(n):
        e = 16 + 32 * i
        if bytes(blob[e:e + 24]).rstrip(b"\0") == b"wave.has_res":
            off, cnt = (int(x) for x in np.frombuffer(blob, np.uint32, 2, e + 24))
            assert cnt * 4 == len(flags)
            blob[off:off + len(flags)] = flags
            return bytes(blob)
    raise AssertionError("no wave.has_res section")


def engine_for(bundle, **kw):
    """An ``Engine`` on ``bundle`` instead of a model directory, loaded from ``blob_of(bundle)``: ``weights.load_model_dir`` and
    ``weights.pack_blob`` are patched around the constructor alone (a module-scoped fixture can call this).  ``kw`` goes to
    ``Engine``."""
    import pytest
    from wwhip import weights as W
    from wwhip.engine import Engine
    blob = blob_of(bundle)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(W, "load_model_dir", lambda path: bundle)
        mp.setattr(W, "pack_blob", lambda b: blob)
        return Engine("synthetic", **kw)


@dataclasses.dataclass(frozen=True)
class Geometry:
    name: str
    kind: str            # "crnn" | "wavenet"
    args: dict           # synthetic_crnn's / synthetic_wavenet's keyword arguments
    edge: str            # what the row is there for
    standard: bool = False   # a CRNN of the shipped conv geometry (the kernels built for it)

    def bundle(self):
        return (synthetic_crnn if self.kind == "crnn" else synthetic_wavenet)(**self.args)

    @property
    def T(self) -> int:
        return int(self.args["T"])

    @property
    def n_mel(self) -> int:
        return int(self.args["n_mel"])

    @property
    def n_out(self) -> int:
        return int(self.args["n_out"])


SIG, SMX = 0, 1   # weights.HEAD_SIGMOID, weights.HEAD_SOFTMAX
_STD = dict(T=151, n_mel=40, C=32, KF=5, KT=20, SF=2, ST=8, same=True)
_SHIPPED_D = [1, 2, 4, 8] * 6


def _c(name, edge, standard=False, **a):
    return Geometry(name, "crnn", a, edge, standard)


def _w(name, edge, **a):
    return Geometry(name, "wavenet", a, edge)


GEOMETRIES: Dict[str, Geometry] = {g.name: g for g in [
    _c("c-std-n8", "widest head in every standard kernel", True, seed=101, **_STD, n_out=8, head=SMX),
    _c("c-std-n3-sigmoid", "sigmoid at width above 1", True, seed=102, **_STD, n_out=3, head=SIG),
    _c("c-t150", "the generic predicate's near miss (pads 7, 7)", seed=103, **dict(_STD, T=150), n_out=2, head=SMX),
    _c("c-one-step", "one live feature column of 64; a recurrence of one step", seed=104, T=6, n_mel=40, C=1, KF=40, KT=6, SF=1, ST=1,
       same=False, n_out=1, head=SIG),
    _c("c-feat63", "OF C = 63, one short of FEATP", seed=105, T=33, n_mel=40, C=7, KF=8, KT=4, SF=4, ST=1, same=False, n_out=2, head=SMX),
    _c("c-feat65", "OF C = 65: FEATP = 128", seed=106, T=40, n_mel=40, C=13, KF=8, KT=5, SF=8, ST=3, same=False, n_out=1, head=SIG),
    _c("c-c64", "the largest C; OF C = 576, an exact multiple", seed=107, T=64, n_mel=40, C=64, KF=8, KT=3, SF=4, ST=2, same=False, n_out=8,
       head=SMX),
    _c("c-lds-limit", "T n_mel = 16384: the loader's own bound; a 32-band filter", seed=108, T=512, n_mel=32, C=3, KF=5, KT=20, SF=2, ST=8,
       same=True, n_out=3, head=SMX),
    _w("w-t1", "the smallest accepted model", seed=201, T=1, n_mel=40, dilations=[1], has_res=[False], n_out=2, skip_bias_mean=0.3),
    _w("w-t16", "exactly one tile", seed=202, T=16, n_mel=40, dilations=[2, 8], has_res=[True, False], n_out=2),
    _w("w-t17-m13", "a second tile of one row; input padding; descending dilations; no residual in the middle", seed=203, T=17, n_mel=13,
       dilations=[8, 1, 4], has_res=[True, False, True], n_out=3),
    _w("w-t100-odd", "odd NB; softmax of one value", seed=204, T=100, n_mel=39, dilations=([1, 2, 4, 8] * 6)[:23], has_res=[False] * 23,
       n_out=1),
    _w("w-t183", "one row beyond the one-launch tick's T", seed=205, T=183, n_mel=40, dilations=_SHIPPED_D, has_res=[True] * 23 + [False],
       n_out=2),
    _w("w-max", "every bound met at once", seed=206, T=192, n_mel=40, dilations=[8] * 32, has_res=[True] * 32, n_out=16,
       w2_sigma=0.1),   # (32 blocks' skip sum reaches 20: at 0.5 a 16-way softmax puts column 1 below 1e-3)
]}

CRNN_ROWS = [n for n, g in GEOMETRIES.items() if g.kind == "crnn"]
STANDARD_ROWS = [n for n, g in GEOMETRIES.items() if g.standard]
GENERIC_ROWS = [n for n, g in GEOMETRIES.items() if g.kind == "crnn" and not g.standard]
WAVE_ROWS = [n for n, g in GEOMETRIES.items() if g.kind == "wavenet"]

WINDOW_SEED = 900   # + the row's position in GEOMETRIES: the windows the GPU tests run and test_geometry64.py vets
N_WINDOWS = 70


def row_windows(name: str, n: int = N_WINDOWS) -> np.ndarray:
    g = GEOMETRIES[name]
    return windows(WINDOW_SEED + list(GEOMETRIES).index(name), n, g.T, g.n_mel)


def oracle_takes(g: Geometry) -> bool:
    """The fp32 C oracle's own limits (oracle/ww_oracle.c): KF KT <= 256, OT <= 256, a Wavenet head of at most 8."""
    if g.kind == "wavenet":
        return g.n_out <= 8
    b = g.bundle().crnn
    return g.args["KF"] * g.args["KT"] <= 256 and b.out_t <= 256


def expected_geometry(bundle) -> dict:
    """What ``model_pack_check`` prints for the bundle (its ``geom crnn`` / ``geom wave`` words)."""
    if bundle.crnn is not None:
        c = bundle.crnn
        return dict(n_mel=c.n_mel, T=c.n_frames, C=c.conv_w.shape[0], KF=c.conv_w.shape[1], KT=c.conv_w.shape[2], SF=c.stride_f, ST=c.stride_t,
                    PF=c.pad_f[0], PT=c.pad_t[0], OF=c.out_f, OT=c.out_t, H=c.units, NOUT=c.n_out, HEAD=c.head_kind)
    w = bundle.wavenet
    return dict(T=w.n_frames, n_mel=w.n_mel, C=w.channels, S=w.skip_channels, NB=len(w.blocks), NOUT=int(w.det_w2.shape[1]),
                dil=[b.dilation for b in w.blocks], has_res=[int(b.w_res is not None) for b in w.blocks])
