"""CTC-trained CRNNs: the label set, the greedy decode in numpy (the statement the device decode is tested against), and the
wake-word rule of the reference's ``eval_CTC`` (``wwdetect/CRNN/evaluate.py:100-150``).

``Arik_CRNN_CTC`` (``wwdetect/CRNN/model.py:82-145``) gives 19 rows of ``L`` posteriors per window: ``L - 1`` labels and the blank,
which is the LAST class (``dataloader.py:54-62``: ``[OTHER]`` = 0, ``[HEY]`` = 1, ``[SNIPS]`` = 2).  ``K.ctc_decode(greedy=True)``
takes the argmax of every row, merges repeats, drops blanks; ``eval_CTC`` keeps the first two labels and calls a clip a wake word
iff they read ``[HEY][SNIPS]``.

Keras takes ``log(y + 1e-7)`` before its argmax.  That map is monotone: it cannot reverse the order of two posteriors, only turn
a strict order into a tie where both round to one logarithm.  The decode here - and the library's, ``csrc/ctc_decode.h`` - reads
the posteriors themselves.

``score`` is the forward algorithm over the same posteriors: the probability that a window's label sequence collapses to a target -
what ``K.ctc_batch_cost`` (``wwdetect/CRNN/train.py:184-200``) is minus the logarithm of -, the number a threshold can be put on.
``csrc/ctc_score.h`` states it; the function here is that statement in float64.
"""
from __future__ import annotations

from typing import NamedTuple, Optional, Sequence, Tuple

import numpy as np

LABELS = ("[OTHER]", "[HEY]", "[SNIPS]")
WAKEWORD = (1, 2)  # [HEY][SNIPS]


class CtcResult(NamedTuple):
    """What ``Engine.ctc_forward`` / ``ctc_slide_forward`` return: ``labels [n, max_labels]`` int32 padded with -1, ``lengths [n]``
    int32 (the whole decoded length, which may exceed ``max_labels``), and where asked for ``steps [n, 19, L]`` / ``enc [n, 19, 64]``."""
    labels: np.ndarray
    lengths: np.ndarray
    steps: Optional[np.ndarray] = None
    enc: Optional[np.ndarray] = None


def greedy_decode(steps, max_labels: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray]:
    """``steps [n, T, L]`` (or ``[T, L]``) posteriors -> ``(labels [n, max_labels] int32 padded with -1, lengths [n] int32)``.

    Per step the argmax over the classes, the lowest index on a tie; a class is emitted when it is not the blank (``L - 1``) and
    differs from the previous step's argmax - the blank counts as a previous value, so ``a, blank, a`` reads ``a a``.
    ``max_labels`` defaults to ``T`` (nothing cut); ``lengths`` is the whole decoded length either way."""
    s = np.asarray(steps)
    if s.ndim == 2:
        s = s[None]
    if s.ndim != 3 or s.shape[1] < 1 or s.shape[2] < 2:
        raise ValueError(f"steps must be [n, T >= 1, L >= 2], got {s.shape}")
    n, T, L = s.shape
    m = T if max_labels is None else int(max_labels)
    if m < 1:
        raise ValueError("max_labels must be positive")
    best = s.argmax(axis=2)  # (numpy's argmax returns the first maximum)
    prev = np.concatenate([np.full((n, 1), -1, best.dtype), best[:, :-1]], axis=1)
    emit = (best != L - 1) & (best != prev)
    labels = np.full((n, m), -1, np.int32)
    lengths = emit.sum(axis=1).astype(np.int32)
    for i in range(n):
        seq = best[i, emit[i]][:m]
        labels[i, :len(seq)] = seq
    return labels, lengths


SCORE_MODES = {"exact": 0, "prefix": 1}  # include/wwhip.h: WW_CTC_SCORE_EXACT, WW_CTC_SCORE_PREFIX
SCORE_MAX_TARGET, SCORE_MAX_TARGETS, SCORE_MAX_STEPS = 9, 8, 64


def score_mode(mode) -> int:
    """``"exact"`` / ``"prefix"`` (or their numbers 0 / 1) -> the number the library takes."""
    if mode in SCORE_MODES:
        return SCORE_MODES[mode]
    if isinstance(mode, (int, np.integer)) and int(mode) in SCORE_MODES.values():
        return int(mode)
    raise ValueError(f"unknown mode {mode!r}: 'exact' (P(decode == target)) or 'prefix' (P(decode starts with target))")


def pack_targets(targets, L: int) -> Tuple[np.ndarray, np.ndarray]:
    """A list of label tuples (or one tuple) -> ``(table [K, 9] int32, lengths [K] int32)`` as the library takes them, with its
    rules checked: 1..8 targets of 1..9 labels in ``[0, L - 2]``."""
    tg = list(targets)
    if tg and isinstance(tg[0], (int, np.integer)):
        tg = [tuple(tg)]
    if not 1 <= len(tg) <= SCORE_MAX_TARGETS:
        raise ValueError(f"K = {len(tg)} targets outside 1..{SCORE_MAX_TARGETS}")
    table, lens = np.zeros((len(tg), SCORE_MAX_TARGET), np.int32), np.zeros(len(tg), np.int32)
    for k, c in enumerate(tg):
        c = [int(x) for x in c]
        if not 1 <= len(c) <= SCORE_MAX_TARGET:
            raise ValueError(f"target {k} has U = {len(c)} labels, outside 1..{SCORE_MAX_TARGET}")
        if min(c) < 0 or max(c) > L - 2:
            raise ValueError(f"target {k} = {tuple(c)} has a label outside [0, L - 2] = [0, {L - 2}] (the blank is class L - 1)")
        table[k, :len(c)], lens[k] = c, len(c)
    return table, lens


def score(steps, targets, mode="exact", dtype=np.float64) -> np.ndarray:
    """``steps [n, T, L]`` (or ``[T, L]``) posteriors, ``targets`` a list of label tuples -> ``[K, n]``: per target and window the
    probability that the window's decode IS the target (``mode="exact"``, the CTC loss's quantity) or STARTS WITH it
    (``"prefix"``, the quantity of :func:`is_wakeword`).  The blank is class ``L - 1``; repeats in a target are allowed.

    States ``s = 0 .. 2U``: even ``s`` the blank, odd ``s`` label ``c[(s - 1) / 2]``; ``skip(s)``: ``s`` odd, ``>= 3`` and its label
    differs from the one before.  ``a_0(0) = y_0[blank]``, ``a_0(1) = y_0[c_0]``;
    ``a_t(s) = ((a(s) + a(s - 1)) + (skip(s) ? a(s - 2) : 0)) * y_t[cls(s)]``.  Exact: ``a(2U) + a(2U - 1)`` at the last step.
    Prefix: ``P_0 = (U == 1 ? y_0[c_0] : 0)``, ``P_t = P_{t-1} + (a_{t-1}(2U - 2) + (skip(2U - 1) ? a_{t-1}(2U - 3) : 0)) * y_t[c_{U-1}]``.

    The linear domain, no rescaling, in ``dtype``: float64 is the statement the library is tested against; with ``np.float32`` every
    operation is one float32 operation in ``csrc/ctc_score.h``'s order, and the result carries that header's bits."""
    y = np.asarray(steps, dtype)
    if y.ndim == 2:
        y = y[None]
    if y.ndim != 3 or y.shape[1] < 1 or y.shape[2] < 2:
        raise ValueError(f"steps must be [n, T >= 1, L >= 2], got {y.shape}")
    n, T, L = y.shape
    table, lens = pack_targets(targets, L)
    prefix = score_mode(mode) == SCORE_MODES["prefix"]
    out = np.zeros((len(lens), n), dtype)
    zero = np.zeros(n, dtype)
    for k, U in enumerate(lens):
        c = table[k, :U]
        S = 2 * U + 1
        cls = [L - 1 if s % 2 == 0 else c[(s - 1) // 2] for s in range(S)]
        skip = [s % 2 == 1 and s >= 3 and c[(s - 1) // 2] != c[(s - 3) // 2] for s in range(S)]
        a = [zero] * S
        a[0], a[1] = y[:, 0, L - 1], y[:, 0, c[0]]
        P = y[:, 0, c[0]] if U == 1 else zero
        for t in range(1, T):
            if prefix:
                P = P + (a[S - 3] + (a[S - 4] if skip[S - 2] else zero)) * y[:, t, c[U - 1]]
            a = [((a[s] + (a[s - 1] if s >= 1 else zero)) + (a[s - 2] if skip[s] else zero)) * y[:, t, cls[s]] for s in range(S)]
        out[k] = P if prefix else a[S - 1] + a[S - 2]
    return out


def score_rows(steps, targets, mode="exact") -> np.ndarray:
    """``csrc/ctc_score.h``'s float32 function over host arrays (``ww_ctc_score_rows``; no GPU): ``[K, n]`` float32 - the bits the
    device kernel is held to."""
    from . import _lib
    y = np.ascontiguousarray(steps, np.float32)
    if y.ndim == 2:
        y = y[None]
    if y.ndim != 3:
        raise ValueError(f"steps must be [n, T, L], got {y.shape}")
    n, T, L = y.shape
    table, lens = pack_targets(targets, L)
    out = np.empty((len(lens), n), np.float32)
    _lib.raise_for(_lib.load().ww_ctc_score_rows(_lib.ptr(y), n, T, L, _lib.ptr(table), _lib.ptr(lens), len(lens), score_mode(mode),
                                                 _lib.ptr(out)), None)
    return out


def is_wakeword(labels, lengths, target: Sequence[int] = WAKEWORD) -> np.ndarray:
    """True where the decoded string starts with ``target``: ``lengths >= len(target)`` and the first ``len(target)`` labels equal
    it - ``eval_CTC``'s comparison of ``decoded[:, :2]`` with ``[HEY][SNIPS]``."""
    lab = np.atleast_2d(np.asarray(labels))
    ln = np.atleast_1d(np.asarray(lengths))
    k = len(target)
    if k < 1:
        raise ValueError("target is empty")
    if lab.shape[1] < k:
        return np.zeros(lab.shape[0], bool)
    return (ln >= k) & np.all(lab[:, :k] == np.asarray(target, lab.dtype)[None], axis=1)


def label_string(labels, length: int, names: Sequence[str] = LABELS) -> str:
    """One row of ``labels`` as text, e.g. ``"[HEY][SNIPS]"`` (a class beyond ``names`` prints as its number; a string longer
    than the row ends in ``...``)."""
    row = [int(c) for c in np.asarray(labels).ravel() if c >= 0]
    text = "".join(names[c] if c < len(names) else f"[{c}]" for c in row)
    return text + ("..." if int(length) > len(row) else "")
