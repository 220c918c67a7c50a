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

``align`` is the max-product twin: the most probable path through the target's lattice and the steps at which it enters and leaves
each label - where in the window the wake word lies, to one conv step (``csrc/ctc_align.h``; ``step_rows`` / ``span_rows`` /
``span_seconds`` turn steps into mel rows and time).

``beam_search`` is the prefix beam search: the most probable label STRINGS of a window and their probabilities, where the greedy
decode collapses the most probable path - ``K.ctc_decode(greedy=False, beam_width, top_paths)``'s question.  ``csrc/ctc_beam.h``
states it (the textbook search in the linear domain on the posteriors themselves; not TensorFlow's log-domain bits); the function
here is that statement in float64, ``beam_rows`` the library's float32 function on the host.

``occupancy`` is the forward-backward pass: given that a window reads a target, the share of each step that each label holds over
ALL such paths, the completion step's distribution in prefix mode, and the per-class share whose difference from the posteriors is
the gradient of the CTC loss with respect to a step's logits (``csrc/ctc_occupancy.h``; ``occupancy_rows`` is the library's float32
function on the host, :class:`CtcOccupancy` carries ``blank``, ``loss``, ``grad`` and ``expected_step``).
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


class CtcAlignment(NamedTuple):
    """``value [K, n]``: the probability of the best path of target ``k`` over window ``i`` (0: there is none);
    ``span [K, n, U_max, 2]`` int32: the first and the last step at which that path is on label ``u`` (-1: no such label, or no
    path); in prefix mode the last label's pair is ``{t*, t*}``, the step that completes the target.  ``paths`` (``wwhip.ctc.align``
    only): ``paths[k][i]`` the path itself, a class per step - ``T`` steps in exact mode, ``t* + 1`` in prefix mode - or ``None``."""
    value: np.ndarray
    span: np.ndarray
    paths: Optional[list] = None


def align(steps, targets, mode="exact") -> CtcAlignment:
    """``csrc/ctc_align.h`` in float64: ``steps [n, T, L]`` (or ``[T, L]``), ``targets`` a list of label tuples.

    The lattice is :func:`score`'s with max in the place of the sum: ``v_0(0) = y_0[blank]``, ``v_0(1) = y_0[c_0]``; for ``t >= 1``
    the candidates ``v(s)`` (shift 0), ``v(s - 1)`` (shift 1), ``v(s - 2)`` (shift 2, where ``skip(s)``), the best being the first
    of the largest, and ``v_t(s) = best * y_t[cls(s)]``.  Exact: the path ends at ``T - 1`` in state ``2U - 1``, or ``2U`` if that is
    strictly larger.  Prefix: ``q_t = max(v_{t-1}(2U - 2), skip(2U - 1) ? v_{t-1}(2U - 3)) * y_t[c_{U-1}]``,
    ``q_0 = (U == 1 ? y_0[c_0] : 0)``; the path enters state ``2U - 1`` at the earliest step ``t*`` of the largest ``q_t`` and ends
    there."""
    y = np.asarray(steps, np.float64)
    if y.ndim == 2:
        y = y[None]
    if y.ndim != 3 or y.shape[1] < 1 or y.shape[2] < 2:
        raise ValueError(f"steps must be [n, T >= 1, L >= 2], got {y.shape}")
    n, T, L = y.shape
    table, lens = pack_targets(targets, L)
    prefix = score_mode(mode) == SCORE_MODES["prefix"]
    K, umax = len(lens), int(lens.max())
    value, span = np.zeros((K, n), np.float64), np.full((K, n, umax, 2), -1, np.int32)
    paths = [[None] * n for _ in range(K)]
    for k, U in enumerate(lens):
        c = table[k, :U]
        S = 2 * U + 1
        cls = [L - 1 if s % 2 == 0 else int(c[(s - 1) // 2]) for s in range(S)]
        skip = [s % 2 == 1 and s >= 3 and c[(s - 1) // 2] != c[(s - 3) // 2] for s in range(S)]
        for i in range(n):
            v = [0.0] * S
            v[0], v[1] = y[i, 0, L - 1], y[i, 0, c[0]]
            bp = np.zeros((T, S), np.int64)
            Q, t_star, q_shift = (y[i, 0, c[0]] if U == 1 else 0.0), 0, 0
            for t in range(1, T):
                if prefix:
                    m, sh = v[S - 3], 1
                    if skip[S - 2] and v[S - 4] > m:
                        m, sh = v[S - 4], 2
                    q = m * y[i, t, c[U - 1]]
                    if q > Q:
                        Q, t_star, q_shift = q, t, sh
                nv = [0.0] * S
                for s in range(S):
                    best, sh = v[s], 0
                    if s >= 1 and v[s - 1] > best:
                        best, sh = v[s - 1], 1
                    if skip[s] and v[s - 2] > best:
                        best, sh = v[s - 2], 2
                    bp[t, s] = sh
                    nv[s] = best * y[i, t, cls[s]]
                v = nv
            if prefix:
                value[k, i] = Q
                if Q == 0.0:
                    continue
                states = [S - 2]
                s, t = S - 2 - q_shift, t_star - 1
            else:
                s = S - 1 if v[S - 1] > v[S - 2] else S - 2
                value[k, i] = v[s]
                if v[s] == 0.0:
                    continue
                states, t = [], T - 1
            while t >= 0:
                states.append(s)
                if t >= 1:
                    s -= int(bp[t, s])
                t -= 1
            states.reverse()
            paths[k][i] = np.array([cls[s] for s in states], np.int32)
            for t, s in enumerate(states):
                if s % 2:
                    u = (s - 1) // 2
                    if span[k, i, u, 0] < 0:
                        span[k, i, u, 0] = t
                    span[k, i, u, 1] = t
    return CtcAlignment(value, span, paths)


def align_rows(steps, targets, mode="exact") -> CtcAlignment:
    """``csrc/ctc_align.h``'s float32 function over host arrays (``ww_ctc_align_rows``; no GPU): ``value [K, n]`` float32 and
    ``span [K, n, U_max, 2]`` int32 - the bits the device kernel is held to."""
    from . import _lib
    y = np.ascontiguousarray(steps, np.float32)
    if y.ndim == 2:
        y = y[None]
    if y.ndim != 3:
        raise ValueError(f"steps must be [n, T, L], got {y.shape}")
    n, T, L = y.shape
    table, lens = pack_targets(targets, L)
    value, span = np.empty((len(lens), n), np.float32), np.empty((len(lens), n, SCORE_MAX_TARGET, 2), np.int8)
    _lib.raise_for(_lib.load().ww_ctc_align_rows(_lib.ptr(y), n, T, L, _lib.ptr(table), _lib.ptr(lens), len(lens), score_mode(mode),
                                                 _lib.ptr(value), _lib.ptr(span)), None)
    return CtcAlignment(value, span[:, :, :int(lens.max())].astype(np.int32))


class CtcOccupancy(NamedTuple):
    """``value [K, n]``: the score ``Z`` of target ``k`` over window ``i`` (:func:`score`'s, for the same mode);
    ``occ [K, n, T, 9]``: given that the window reads the target, the probability that its path is on label ``u`` at step ``t``, over
    all such paths (rows ``u >= U`` are 0); in prefix mode ``occ[..., U - 1]`` is the probability that step ``t`` COMPLETES the
    target, which sums to 1 over ``t``.  ``cls [K, n, T, L]`` (exact mode, where asked for; else ``None``): the same posterior per
    class, the blank included; every row sums to 1.  Where ``value == 0`` there is no such path and every entry is 0."""
    value: np.ndarray
    occ: np.ndarray
    cls: Optional[np.ndarray] = None

    @property
    def blank(self) -> np.ndarray:
        """``[K, n, T]``: ``1 - occ.sum(-1)``, in exact mode the blank's share of each step (it may be a rounding below 0)."""
        return 1 - self.occ.sum(axis=-1)

    @property
    def loss(self) -> np.ndarray:
        """``[K, n]``: ``-log(value)``, what ``K.ctc_batch_cost`` is on the posteriors themselves (``inf`` where ``value == 0``)."""
        with np.errstate(divide="ignore"):
            return -np.log(self.value)

    def grad(self, steps) -> np.ndarray:
        """``[K, n, T, L]``: ``steps - cls``, the gradient of :attr:`loss` with respect to the LOGITS of each step (the softmax's
        inputs) of ``steps [n, T, L]``.  It is zeros where ``value == 0``: the loss is infinite there and has no gradient, and a
        caller that sums these over clips must not take the posteriors themselves for an error signal.  Exact mode with ``cls``."""
        if self.cls is None:
            raise ValueError("grad needs cls: exact mode, want_classes=True")
        y = np.asarray(steps, self.cls.dtype)
        if y.ndim == 2:
            y = y[None]
        if y.shape != self.cls.shape[1:]:
            raise ValueError(f"steps must be {self.cls.shape[1:]}, got {y.shape}")
        return np.where((self.value == 0)[:, :, None, None], 0, y[None] - self.cls).astype(self.cls.dtype)

    @property
    def expected_step(self) -> np.ndarray:
        """``[K, n, 9]``: per label ``sum_t t occ / sum_t occ``, the mean step of the label under the posterior over paths (in prefix
        mode the last label's is the mean completion step); NaN where the label is absent or ``value == 0``."""
        t = np.arange(self.occ.shape[2], dtype=np.float64)[None, None, :, None]
        with np.errstate(invalid="ignore", divide="ignore"):
            return (t * self.occ).sum(axis=2) / self.occ.sum(axis=2, dtype=np.float64)


def occupancy(steps, targets, mode="exact", dtype=np.float64) -> CtcOccupancy:
    """``csrc/ctc_occupancy.h`` in ``dtype``: ``steps [n, T, L]`` (or ``[T, L]``) posteriors, ``targets`` a list of label tuples ->
    :class:`CtcOccupancy` (``cls`` in exact mode, ``None`` in prefix mode).

    :func:`score`'s lattice and forward variable ``a_t(s)``.  Exact: ``b_{T-1}(2U) = b_{T-1}(2U - 1) = 1``,
    ``m_{t+1}(s) = b_{t+1}(s) y_{t+1}[cls(s)]``, ``b_t(s) = (m(s) + m(s + 1)) + (skip(s + 2) ? m(s + 2) : 0)`` - no ``y_t`` in ``b_t``,
    so nothing is divided by a posterior -, ``Z = a_{T-1}(2U) + a_{T-1}(2U - 1)``, ``g_t(s) = a_t(s) b_t(s) / Z``;
    ``occ[t, u] = g_t(2u + 1)`` and ``cls[t, k]`` the sum of ``g_t(s)`` over the states of class ``k`` in ascending ``s``.  Prefix: the
    live states are ``0 .. 2U - 2``, ``b_{T-1} = 0``, the backward value of the completed state ``2U - 1`` is 1 at every step, ``Z`` is
    the prefix score and ``occ[t, U - 1] = e_t / Z`` with ``e_t`` the score's completion term.  ``Z == 0``: everything is 0.

    float64 is the statement the library is tested against; with ``np.float32`` every operation is one float32 operation in the
    header's order and the result carries ``ww_ctc_occupancy_rows``' bits."""
    y = np.asarray(steps, dtype)
    if y.ndim == 2:
        y = y[None]
    if y.ndim != 3 or y.shape[1] < 1 or y.shape[2] < 2:
        raise ValueError(f"steps must be [n, T >= 1, L >= 2], got {y.shape}")
    n, T, L = y.shape
    table, lens = pack_targets(targets, L)
    prefix = score_mode(mode) == SCORE_MODES["prefix"]
    K = len(lens)
    value, occ = np.zeros((K, n), y.dtype), np.zeros((K, n, T, SCORE_MAX_TARGET), y.dtype)
    cls_out = None if prefix else np.zeros((K, n, T, L), y.dtype)
    zero, one = np.zeros(n, y.dtype), np.ones(n, y.dtype)
    for k, U in enumerate(lens):
        c = table[k, :U]
        S = 2 * U + 1
        cls = [L - 1 if s % 2 == 0 else int(c[(s - 1) // 2]) for s in range(S)]
        skip = [s % 2 == 1 and s >= 3 and c[(s - 1) // 2] != c[(s - 3) // 2] for s in range(S)] + [False, False]
        a = [[zero] * S for _ in range(T)]
        a[0][0], a[0][1] = y[:, 0, L - 1], y[:, 0, c[0]]
        e = [y[:, 0, c[0]] if U == 1 else zero]  # the completion terms, e_t
        P = e[0]
        for t in range(1, T):
            p = a[t - 1]
            e.append((p[S - 3] + (p[S - 4] if skip[S - 2] else zero)) * y[:, t, c[U - 1]])
            P = P + e[t]
            a[t] = [((p[s] + (p[s - 1] if s >= 1 else zero)) + (p[s - 2] if skip[s] else zero)) * y[:, t, cls[s]] for s in range(S)]
        Z = P if prefix else a[T - 1][S - 1] + a[T - 1][S - 2]
        if prefix:  # a_t(2U - 1) is not live: e_t sits there, under a backward value pinned to 1
            for t in range(T):
                a[t][S - 2] = e[t]
        value[k] = Z
        some = Z != 0
        Zs = np.where(some, Z, 1)
        b = [zero] * (S - 2) + [one, zero if prefix else one]
        for t in range(T - 1, -1, -1):
            g = [np.where(some, (a[t][s] * b[s]) / Zs, 0) for s in range(S)]
            for u in range(U):
                occ[k, :, t, u] = g[2 * u + 1]
            if cls_out is not None:
                seen = set()
                for s in range(S):  # ascending s, from the first state of the class
                    cls_out[k, :, t, cls[s]] = cls_out[k, :, t, cls[s]] + g[s] if cls[s] in seen else g[s]
                    seen.add(cls[s])
            if t == 0:
                break
            m = [b[s] * y[:, t, cls[s]] for s in range(S)] + [zero, zero]
            b = [(m[s] + m[s + 1]) + (m[s + 2] if skip[s + 2] else zero) for s in range(S)]
            if prefix:
                b[S - 2], b[S - 1] = one, zero
    return CtcOccupancy(value, occ, cls_out)


def occupancy_rows(steps, targets, mode="exact", want_classes: Optional[bool] = None) -> CtcOccupancy:
    """``csrc/ctc_occupancy.h``'s float32 function over host arrays (``ww_ctc_occupancy_rows``; no GPU) - the bits the device kernel
    is held to.  ``want_classes``: ``cls`` too (the default in exact mode; the library refuses it in prefix mode)."""
    from . import _lib
    y = np.ascontiguousarray(steps, np.float32)
    if y.ndim == 2:
        y = y[None]
    if y.ndim != 3:
        raise ValueError(f"steps must be [n, T, L], got {y.shape}")
    n, T, L = y.shape
    table, lens = pack_targets(targets, L)
    md = score_mode(mode)
    if want_classes is None:
        want_classes = md == SCORE_MODES["exact"]
    K = len(lens)
    value, occ = np.empty((K, n), np.float32), np.empty((K, n, max(T, 0), SCORE_MAX_TARGET), np.float32)
    cls = np.empty((K, n, max(T, 0), max(L, 0)), np.float32) if want_classes else None
    _lib.raise_for(_lib.load().ww_ctc_occupancy_rows(_lib.ptr(y), n, T, L, _lib.ptr(table), _lib.ptr(lens), K, md, _lib.ptr(value), _lib.ptr(occ),
                                                     _lib.ptr(cls)), None)
    return CtcOccupancy(value, occ, cls)


BEAM_MAX_T, BEAM_MAX_L, BEAM_MAX_WIDTH, BEAM_MAX_PATHS = 19, 8, 64, 8  # include/wwhip.h: WW_CTC_BEAM_*
_KEY_LEN_SHIFT = 3 * BEAM_MAX_T  # a prefix key: the length above bit 57, the labels below at 3 bits each, the first label highest


class CtcBeam(NamedTuple):
    """``labels [n, P, max_labels]`` int32 padded with -1, ``lengths [n, P]`` int32 (the whole length; -1: the path is absent),
    ``probs [n, P]``: the P most probable label strings of each window, descending.  ``log_probs`` is what Keras returns."""
    labels: np.ndarray
    lengths: np.ndarray
    probs: np.ndarray

    @property
    def log_probs(self) -> np.ndarray:
        with np.errstate(divide="ignore"):
            return np.log(self.probs)


def beam_rel_bound(T: int) -> float:
    """``csrc/ctc_beam.h``'s derived bound: the relative error of a reported probability against the float64 statement on the same
    float32 posteriors with the same pruning decisions, ``(3 T + 2) 2^-24``."""
    return (3 * int(T) + 2) * 2.0 ** -24


def _beam_args(T, L, beam_width, top_paths, max_labels):
    W, P = int(beam_width), int(top_paths)
    M = T if max_labels is None else int(max_labels)
    if not 1 <= T <= BEAM_MAX_T:
        raise ValueError(f"T = {T} outside 1..{BEAM_MAX_T}")
    if not 2 <= L <= BEAM_MAX_L:
        raise ValueError(f"L = {L} outside 2..{BEAM_MAX_L}")
    if not 1 <= W <= BEAM_MAX_WIDTH:
        raise ValueError(f"beam_width = {W} outside 1..{BEAM_MAX_WIDTH}")
    if not 1 <= P <= min(W, BEAM_MAX_PATHS):
        raise ValueError(f"top_paths = {P} outside 1..min(beam_width, {BEAM_MAX_PATHS})")
    if not 1 <= M <= T:
        raise ValueError(f"max_labels = {M} outside 1..T = 1..{T}")
    return W, P, M


def key_labels(key: int) -> Tuple[int, ...]:
    """A prefix key -> its labels."""
    key = int(key)
    n = key >> _KEY_LEN_SHIFT
    return tuple((key >> (_KEY_LEN_SHIFT - 3 * (i + 1))) & 7 for i in range(n))


def beam_search(steps, beam_width: int, top_paths: int = 1, max_labels: Optional[int] = None, dtype=np.float64, trace: Optional[list] = None) -> CtcBeam:
    """``csrc/ctc_beam.h`` in ``dtype``: CTC prefix beam search over ``steps [n, T, L]`` (or ``[T, L]``) posteriors, the blank being
    class ``L - 1`` - the ``top_paths`` most probable label strings of each window and their probabilities.

    The beam: at most ``beam_width`` entries ``(key, pb, pnb)``, from the empty prefix with ``(1, 0)``.  A step, for every entry
    ``A`` with ``tot = pb + pnb``: stay ``pb' = tot * y[blank]``, ``pnb' = pnb * y[last(A)]`` (0 for the empty prefix); extend, for
    every label ``c``, ``ext = (c == last(A) ? pb : tot) * y[c]`` - added to ``pnb'`` of ``A + c`` where that is a beam entry (its stay
    term first, then one addition), else a new candidate ``(0, ext)``.  The next beam: the first ``beam_width`` candidates by
    total ``pb' + pnb'`` descending (NaN ranks as -1), then key ascending (shorter first, then lexicographic).

    float64 is the statement the library is tested against; with ``np.float32`` every operation is one float32 operation in the
    header's order and the result carries ``ww_ctc_beam_rows``' bits.  ``trace`` (a list) receives per window a list of per-step
    ``(ranks, keys)`` of ALL the step's candidates in the order - what a test needs to judge how close a pruning decision was."""
    y = np.asarray(steps, dtype)
    if y.ndim == 2:
        y = y[None]
    if y.ndim != 3:
        raise ValueError(f"steps must be [n, T, L], got {y.shape}")
    n, T, L = y.shape
    W, P, M = _beam_args(T, L, beam_width, top_paths, max_labels)
    dt = y.dtype.type
    u = np.uint64
    labels, lengths, probs = np.full((n, P, M), -1, np.int32), np.full((n, P), -1, np.int32), np.zeros((n, P), y.dtype)
    cs = np.arange(L - 1)
    for i in range(n):
        key, pb, pnb = np.zeros(1, u), np.ones(1, y.dtype), np.zeros(1, y.dtype)
        steps_trace = []
        with np.errstate(all="ignore"):
            for t in range(T):
                row = y[i, t]
                ln = (key >> u(_KEY_LEN_SHIFT)).astype(np.int64)
                last = np.where(ln > 0, (key >> (_KEY_LEN_SHIFT - 3 * np.maximum(ln, 1)).astype(u)).astype(np.int64) & 7, -1)
                tot = pb + pnb
                st_pb = tot * row[L - 1]
                st_pnb = np.where(last >= 0, pnb * row[np.maximum(last, 0)], dt(0))
                ext = np.where(cs[None, :] == last[:, None], pb[:, None], tot[:, None]) * row[None, :L - 1]  # [nb, L - 1]
                child = key[:, None] + (u(1) << u(_KEY_LEN_SHIFT)) + (cs[None, :].astype(u) << (_KEY_LEN_SHIFT - 3 * (ln[:, None] + 1)).astype(u))
                # a child that is itself a beam entry takes the extension: its stay term first, then one addition
                order = np.argsort(key)
                pos = np.minimum(np.searchsorted(key[order], child), len(key) - 1)
                found = key[order][pos] == child
                st_pnb = st_pnb.copy()
                tgt = order[pos[found]]
                st_pnb[tgt] = st_pnb[tgt] + ext[found]
                new = ~found
                c_key = np.concatenate([key, child[new]])
                c_pb = np.concatenate([st_pb, np.zeros(int(new.sum()), y.dtype)])
                c_pnb = np.concatenate([st_pnb, ext[new]])
                total = c_pb + c_pnb
                rank = np.where(np.isnan(total), dt(-1), total)
                sel = np.lexsort((c_key, -rank))
                if trace is not None:
                    steps_trace.append((rank[sel].copy(), c_key[sel].copy()))
                sel = sel[:W]
                key, pb, pnb = c_key[sel], c_pb[sel], c_pnb[sel]
            total = pb + pnb
        if trace is not None:
            trace.append(steps_trace)
        for p in range(min(P, len(key))):
            if total[p] == 0:
                continue
            lab = key_labels(key[p])
            lengths[i, p], probs[i, p] = len(lab), total[p]
            labels[i, p, :min(M, len(lab))] = lab[:M]
    return CtcBeam(labels, lengths, probs)


def beam_rows(steps, beam_width: int, top_paths: int = 1, max_labels: Optional[int] = None) -> CtcBeam:
    """``csrc/ctc_beam.h``'s float32 function over host arrays (``ww_ctc_beam_rows``; no GPU) - the bits the device kernel is held to."""
    from . import _lib
    y = np.ascontiguousarray(steps, np.float32)
    if y.ndim == 2:
        y = y[None]
    if y.ndim != 3:
        raise ValueError(f"steps must be [n, T, L], got {y.shape}")
    n, T, L = y.shape
    W, P = int(beam_width), int(top_paths)
    M = T if max_labels is None else int(max_labels)
    labels, lengths, probs = np.empty((n, max(P, 0), max(M, 0)), np.int32), np.empty((n, max(P, 0)), np.int32), np.empty((n, max(P, 0)), np.float32)
    _lib.raise_for(_lib.load().ww_ctc_beam_rows(_lib.ptr(y), n, T, L, W, P, M, _lib.ptr(labels), _lib.ptr(lengths), _lib.ptr(probs)), None)
    return CtcBeam(labels, lengths, probs)


# the conv front of the standard geometry (a 151-row window -> 19 steps): kernel 20 rows, stride 8, 6 rows of padding in front
CONV_KT, CONV_ST, CONV_PT, WINDOW_ROWS = 20, 8, 6, 151
ROW_SECONDS = 0.01  # a mel row every 10 ms


def step_rows(t) -> Tuple[np.ndarray, np.ndarray]:
    """The mel rows of a window that conv step ``t`` reads at the standard geometry: ``(first, last)`` =
    ``[8 t - 6, 8 t + 13]`` clipped to ``[0, 150]`` (scalars or arrays)."""
    t = np.asarray(t)
    first, last = CONV_ST * t - CONV_PT, CONV_ST * t - CONV_PT + CONV_KT - 1
    return np.clip(first, 0, WINDOW_ROWS - 1), np.clip(last, 0, WINDOW_ROWS - 1)


def span_rows(span, window_row0=0) -> np.ndarray:
    """``span [..., 2]`` (first step, last step; -1: none) of windows that start at row ``window_row0`` (a number, or an array that
    broadcasts against ``span[..., 0]``) -> ``[..., 2]`` int64: the first row the first step reads and the last row the last step
    reads, counted on the sequence's rows; -1 where the span is -1."""
    sp = np.asarray(span).astype(np.int64)
    if sp.ndim < 1 or sp.shape[-1] != 2:
        raise ValueError(f"span must be [..., 2], got {sp.shape}")
    row0 = np.asarray(window_row0, np.int64)
    out = np.stack([step_rows(sp[..., 0])[0] + row0, step_rows(sp[..., 1])[1] + row0], axis=-1)
    out[(sp < 0).any(axis=-1)] = -1
    return out


def span_seconds(span, window_row0=0) -> np.ndarray:
    """:func:`span_rows` in seconds, ``[..., 2]`` float64: the time at which the first row starts and the time at which the last
    row ends (a row every 10 ms); NaN where the span is -1."""
    rows = span_rows(span, window_row0)
    out = np.stack([rows[..., 0] * ROW_SECONDS, (rows[..., 1] + 1) * ROW_SECONDS], axis=-1)
    out[(rows < 0).any(axis=-1)] = np.nan
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
