"""CTC-trained CRNNs: the label set, the greedy decode in numpy (the statement the device decode is tested against), and the
wake-word rule of the reference's ``eval_CTC`` (``wwdetect/CRNN/evaluate.py:100-150``).

``Arik_CRNN_CTC`` (``wwdetect/CRNN/model.py:82-145``) gives 19 rows of ``L`` posteriors per window: ``L - 1`` labels and the blank,
which is the LAST class (``dataloader.py:54-62``: ``[OTHER]`` = 0, ``[HEY]`` = 1, ``[SNIPS]`` = 2).  ``K.ctc_decode(greedy=True)``
takes the argmax of every row, merges repeats, drops blanks; ``eval_CTC`` keeps the first two labels and calls a clip a wake word
iff they read ``[HEY][SNIPS]``.

Keras takes ``log(y + 1e-7)`` before its argmax.  That map is monotone: it cannot reverse the order of two posteriors, only turn
a strict order into a tie where both round to one logarithm.  The decode here - and the library's, ``csrc/ctc_decode.h`` - reads
the posteriors themselves.
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
