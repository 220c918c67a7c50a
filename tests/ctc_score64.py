"""What the forward-algorithm score tests share (host only): path enumeration, the targets of the end-to-end cases, the sliding
sequence with its float64 scores, and the derived bounds.

Bounds.  Every term of the recurrence is non-negative, so rounding errors only accumulate as relative ones: a state's value passes
through at most three float32 roundings per step (two additions, one product) on its longest chain, and the joins at the end add
two, so on the SAME float32 posteriors ``|s32 - s64| <= (3T + 2) 2^-24 s64``, plus ``(2U + 1) T 2^-126`` where a value under
FLT_MIN was flushed (one per state and step at most).  Against the float64 MODEL the posteriors themselves differ: the project
holds each to ``tau min(p, 1 - p) + 4 ulp32(p)`` (``ref64.check_posteriors``), a relative ``tau + 2^-21`` at most, and a path's
probability is a product of T of them."""
from __future__ import annotations

import itertools

import numpy as np

import ctc64

TARGETS = {2: [(0,)], 4: [(1, 2), (0,), (1, 1)], 8: [(1, 2), (3, 4, 5)]}
MODES = ("exact", "prefix")
# the (L, mode) pairs whose sliding scores are compared against thresholds.  Not (2, "prefix"): with one label, "starts with it" is
# 1 - P(every step blank), which is 1 to the last float64 digit on every one of these windows - no threshold separates them.
SLIDE_CASES = [(2, "exact"), (4, "exact"), (8, "exact"), (4, "prefix"), (8, "prefix")]
T = ctc64.STEPS


def enumerate_paths(y, c):
    """``(P(decode == c), P(decode starts with c))`` of one ``[T, L]`` table by enumeration of all ``L^T`` paths, in float64."""
    y = np.asarray(y, np.float64)
    steps, L = y.shape
    exact = prefix = 0.0
    c = list(c)
    for path in itertools.product(range(L), repeat=steps):
        out, prev = [], -1
        for k in path:
            if k != L - 1 and k != prev:
                out.append(k)
            prev = k
        p = float(np.prod([y[t, path[t]] for t in range(steps)]))
        if out == c:
            exact += p
        if out[:len(c)] == c:
            prefix += p
    return exact, prefix


def arithmetic_bound(score64, steps: int, U: int):
    """The bound on ``|float32 score - float64 score|`` over the same float32 posteriors."""
    return (3 * steps + 2) * 2.0 ** -24 * np.asarray(score64, np.float64) + (2 * U + 1) * steps * 2.0 ** -126


def model_bound(score64, U: int, tau: float = ctc64.TAU):
    """The bound on ``|the library's score - the float64 model's score|``: the posteriors' own tolerance through T factors (1 % of
    slack for the second-order terms of ``(1 + d)^T``), then the arithmetic."""
    s = np.asarray(score64, np.float64)
    return s * (1.01 * T * (tau + 2.0 ** -21)) + arithmetic_bound(s, T, U)


def slide_mel(L: int) -> np.ndarray:
    """300 rows of the L-class model's test windows: 75 windows at hop 2 (tests/test_gpu_ctc.py slides over the same rows)."""
    w = ctc64.reference(L)[1]
    return np.concatenate([w[7], w[8]])[:300]


def slide_windows(L: int) -> np.ndarray:
    mel = slide_mel(L)
    return np.stack([mel[i:i + 151] for i in range(0, 300 - 151 + 1, 2)])


_cache: dict = {}


def slide_scores64(L: int, mode: str) -> np.ndarray:
    """``[K, 75]``: the float64 model's scores of the sliding windows for ``TARGETS[L]``."""
    from wwhip import ctc
    if L not in _cache:
        _cache[L] = ctc64.Ctc64(ctc64.reference(L)[0].crnn).sequence(slide_windows(L))[0]
    return ctc.score(_cache[L], TARGETS[L], mode)


def thresholds(scores64: np.ndarray) -> np.ndarray:
    """Per plane the 25 %, 50 % and 75 % quantiles of its float64 scores: ``[K, 3]``."""
    return np.quantile(np.asarray(scores64, np.float64), [0.25, 0.5, 0.75], axis=1).T


def decidable(scores64: np.ndarray, thr: np.ndarray, L: int) -> np.ndarray:
    """``[K, 3, n]``: the float64 score lies farther from the threshold than ``model_bound``, so a score within the bound of it falls
    on the same side."""
    s = np.asarray(scores64, np.float64)
    bound = np.stack([model_bound(s[k], len(c)) for k, c in enumerate(TARGETS[L])])
    return np.abs(s[:, None, :] - thr[:, :, None]) > bound[:, None, :]
