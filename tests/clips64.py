"""Clip sets, geometries and the float64 reading of the clip path (``ww_clips_forward_dev``: PCM -> log-mel -> one zero-padded
window per clip -> encode + detect).  Not a test file; ``tests/test_clips64.py`` pins it on the CPU and
``tests/test_gpu_clips64.py`` holds the HIP path to it.

A clip set is cut from ``oracle.ref64.decision_stream`` (the PCM stream whose streamed posteriors cross a model's decision
range) at a fixed stride, so that the clips' posteriors cover several logit units instead of the one or two that Gaussian
noise reaches.  The reference is the composition ``test_stream_bank_vs_float64`` uses for "front end + model in float64":
``Ref64.logmel`` rows rounded to fp32, the first ``min(nf, T)`` of them in an all-zero ``[T, 40]`` window, ``Ref64.forward``.
"""
from __future__ import annotations

from typing import Dict, List, Tuple

import numpy as np

from oracle import ref64 as R

WIN = 512          # samples per frame
STREAM_N = 96000   # samples of the stream the clips are cut from
STREAM_SEED = 5    # tests/test_ref64.py and tests/test_gpu_ref64.py use the same stream seed
STRIDE = 4000      # samples between clip starts (8,000 is too coarse: the Wavenet's 32,001-sample set then spans 5.2 logits)

DEFAULT = (32767.0, True, 0.0, 160)   # divisor, clip, pre-emphasis, hop

# (id, (fixed, per_T): samples = fixed + per_T * T with T the model's window, divisor, clip, pre-emphasis, hop, precise, what the
# row reaches in csrc/frontend.hip (logmel_rows_kernel's row -> clip lookup and staging) and csrc/api.hip (the window hand-over)).
# Rows c, d, i-993 and j have a multiple of four frames per clip, so no wave of theirs holds rows of two clips; the "row belongs
# to the next clip" step and the frame-by-frame staging of a wave that straddles two clips run at b, e - h, i-24001, k - n.
GEOMETRY_TABLE = [
    ("a", (400, 0)) + DEFAULT + (True, "nf = 0: no front-end launch, the model on the all-zero window"),
    ("b", (832, 0)) + DEFAULT + (True, "nf = 3: the plain divide below four frames"),
    ("c", (993, 0)) + DEFAULT + (True, "nf = 4, odd length: magic multiply, every clip starts at another 16-byte phase"),
    ("d", (3553, 0)) + DEFAULT + (True, "nf = 20, odd length"),
    ("e", (24001, 0)) + DEFAULT + (True, "the benchmark's length + 1: nf = 147"),
    ("f", (WIN - 160, 160)) + DEFAULT + (True, "nf = T exactly"),
    ("g", (WIN, 160)) + DEFAULT + (True, "nf = T + 1: the window is the clip's first T frames"),
    ("h", (32001, 0)) + DEFAULT + (True, "nf = 197 > T for both model kinds"),
    ("i-24001", (24001, 0), 32768.0, False, 0.97, 160, True, "pre-emphasis: generic staging, 64-bit plain-divide lookup"),
    ("i-993", (993, 0), 32768.0, False, 0.97, 160, True, "the same at nf = 4"),
    ("j", (993, 0), 12345.0, True, 0.0, 160, True, "a divisor that is neither 32767 nor 32768: not fast_div"),
    ("k-12001", (12001, 0), 32767.0, True, 0.0, 80, True, "hop 80: nf = 144"),
    ("k-16513", (16513, 0), 32767.0, True, 0.0, 80, True, "hop 80: nf = 201 > T"),
    ("l", (24001, 0), 32767.0, True, 0.0, 200, True, "hop 200 > 168: nf = 118, not simple_w"),
    ("m", (24001, 0), 32767.0, True, 0.0, 512, True, "hop 512: nf = 46, frames do not overlap"),
    ("n", (700, 0), 32767.0, True, 0.0, 1, True, "hop 1: nf = 189 > T, a wave's four rows one sample apart"),
    ("o-993", (993, 0)) + DEFAULT + (False, "precise = 0: logmel_kernel, tiles_per_utt = 1"),
    ("o-24001", (24001, 0)) + DEFAULT + (False, "precise = 0: tiles_per_utt = 10"),
    ("o-32001", (32001, 0)) + DEFAULT + (False, "precise = 0: tiles_per_utt = 13"),
]
GEOMETRY_IDS = [row[0] for row in GEOMETRY_TABLE]
PRECISE_IDS = [row[0] for row in GEOMETRY_TABLE if row[6]]          # a - n
FAST_FRONTEND_IDS = [row[0] for row in GEOMETRY_TABLE if not row[6]]  # o


def geometry(gid: str, T: int) -> Tuple[int, float, bool, float, int, bool]:
    """``(samples, divisor, clip, pre_emphasis, hop, precise)`` of table row ``gid`` for a model whose window is ``T`` frames."""
    for row in GEOMETRY_TABLE:
        if row[0] == gid:
            fixed, per_t = row[1]
            return (fixed + per_t * T,) + tuple(row[2:7])
    raise KeyError(gid)


def num_frames(samples: int, hop: int) -> int:
    return (samples - WIN) // hop + 1 if samples >= WIN else 0


_STREAMS: Dict[tuple, np.ndarray] = {}


def clip_stream(cpu_oracle, n: int = STREAM_N, seed: int = STREAM_SEED) -> np.ndarray:
    """``decision_stream(cpu_oracle, n, seed)``, built once per model (keyed by the model's packed weights)."""
    key = (hash(cpu_oracle._blob.tobytes()), n, seed)
    if key not in _STREAMS:
        _STREAMS[key] = R.decision_stream(cpu_oracle, n, seed)
    return _STREAMS[key]


def clip_set(cpu_oracle, samples: int, stride: int = STRIDE, n: int = STREAM_N, seed: int = STREAM_SEED) -> np.ndarray:
    """The int16 clips ``src[o : o + samples]`` for ``o = 0, stride, ...`` that lie inside the ``n``-sample decision stream:
    ``[n_clips, samples]``, 16 (32,001 samples) to 24 (400 samples) clips at the defaults."""
    src = clip_stream(cpu_oracle, n, seed)
    return np.stack([src[o:o + samples] for o in range(0, n - samples + 1, stride)])


def pad_windows(mels, T: int, n_mel: int = 40) -> np.ndarray:
    """One all-zero ``[T, n_mel]`` fp32 window per clip with the clip's first ``min(nf, T)`` log-mel rows in front."""
    wins = np.zeros((len(mels), T, n_mel), np.float32)
    for i, m in enumerate(mels):
        k = min(len(m), T)
        wins[i, :k] = np.asarray(m, np.float32)[:k]
    return wins


def ref_clip_posteriors(ref64, clips, T: int, divisor: float = 32767.0, clip: bool = True, preemph: float = 0.0,
                        hop: int = 160) -> np.ndarray:
    """Float64 detect rows ``[n_clips, n_out]`` of the clip path: ``Ref64.logmel`` rows as fp32 -> window -> ``Ref64.forward``."""
    mels = [ref64.logmel(c, divisor, clip, preemph, hop).y.astype(np.float32) for c in clips]
    return ref64.forward(pad_windows(mels, T))[0]


def oracle_clip_posteriors(cpu_oracle, clips, divisor: float = 32767.0, clip: bool = True, preemph: float = 0.0,
                           hop: int = 160) -> np.ndarray:
    """The fp32 C oracle composed the same way: ``CpuOracle.logmel`` -> window -> ``CpuOracle.forward``."""
    mels = [cpu_oracle.logmel(c, divisor, clip, preemph, hop) for c in clips]
    return cpu_oracle.forward(pad_windows(mels, cpu_oracle.window, cpu_oracle.n_mel))


class ClipRefs:
    """Clip sets and their float64 posteriors, each ``(model, samples, front end)`` evaluated once (``precise`` does not enter:
    it selects a kernel, not a specification)."""

    def __init__(self, oracles: dict, refs: dict) -> None:
        self.oracles, self.refs = oracles, refs   # name -> CpuOracle, name -> Ref64
        self._memo: Dict[tuple, np.ndarray] = {}

    def clips(self, name: str, gid: str) -> np.ndarray:
        return clip_set(self.oracles[name], geometry(gid, self.oracles[name].window)[0])

    def want64(self, name: str, gid: str) -> np.ndarray:
        ora = self.oracles[name]
        samples, divisor, clip, pre, hop, _ = geometry(gid, ora.window)
        key = (name, samples, divisor, clip, pre, hop)
        if key not in self._memo:
            self._memo[key] = ref_clip_posteriors(self.refs[name], clip_set(ora, samples), ora.window, divisor, clip, pre, hop)
            self._memo[key].setflags(write=False)
        return self._memo[key]


def spans(out64: np.ndarray) -> List[float]:
    """``[lowest, highest]`` logit of the last column of float64 detect rows."""
    lg = R.logit(np.asarray(out64)[:, -1])
    return [float(lg.min()), float(lg.max())]
