"""What the Viterbi-alignment tests share (host only): the enumeration of every path, the path a span stands for, the float32
posteriors of the end-to-end cases and the derived bounds.

Enumeration.  Exact mode: the paths of T steps whose collapse (repeats merged, blanks dropped) IS the target.  Prefix mode: what
follows a completed target is free, so the object is the path UP TO the step that completes the target - every path of 1..T steps
whose collapse is the target and whose last step emits the target's last label.  A full path starts with the target iff it extends
exactly one of those, and (rows that sum to 1) the probability of such a partial path is the probability of all the full paths
that extend it.  The best is the most probable, the shortest among equals.

Bounds.  ``csrc/ctc_align.h`` rounds once per step, in the multiplication: the value is a product of T posteriors with T - 1
float32 roundings, so on the SAME float32 posteriors ``|v32 - v64| <= (T - 1) 2^-24 v64``, plus an absolute term where a product
under FLT_MIN is flushed.  A comparison of two float32 candidates can prefer the one whose float64 value is smaller only by the
two candidates' own rounding, so the float32 path's float64 probability is at least ``v64 (1 - 2 (T - 1) 2^-24)``."""
from __future__ import annotations

import itertools

import numpy as np

import ctc64

MODES = ("exact", "prefix")
TARGETS = {2: [(0,), (0, 0), (0, 0, 0)], 4: [(1,), (1, 2), (1, 2, 0)], 8: [(3,), (1, 2), (1, 1, 5)]}
T = ctc64.STEPS


def collapse(path, L: int):
    out, prev = [], -1
    for k in path:
        if k != L - 1 and k != prev:
            out.append(int(k))
        prev = k
    return out


def enumerate_best(y, c, mode: str):
    """``(best probability, best path or None, second-best probability)`` over the admissible paths of ``y [T, L]``, in float64
    (0.0 where there is no such path)."""
    y = np.asarray(y, np.float64)
    steps, L = y.shape
    c = list(c)
    found = []
    lengths = (steps,) if mode == "exact" else range(1, steps + 1)
    for n in lengths:
        for path in itertools.product(range(L), repeat=n):
            if collapse(path, L) != c:
                continue
            if mode == "prefix" and collapse(path[:-1], L) == c:
                continue   # (the target was complete before the last step)
            p = 1.0
            for t, k in enumerate(path):
                p *= y[t, k]
            found.append((p, path))
    if not found:
        return 0.0, None, 0.0
    found.sort(key=lambda e: (-e[0], len(e[1])))
    return found[0][0], np.array(found[0][1], np.int32), (found[1][0] if len(found) > 1 else 0.0)


def path_of_span(span, c, steps: int, L: int, mode: str):
    """The path a span ``[U, 2]`` stands for: label ``u`` on steps ``first_u .. last_u``, the blank everywhere else - up to step
    ``T - 1`` in exact mode, up to ``t*`` (the last label's step) in prefix mode.  Asserts that the spans are ordered."""
    span = np.asarray(span)
    end = steps if mode == "exact" else int(span[len(c) - 1, 1]) + 1
    path = np.full(end, L - 1, np.int32)
    prev = -1
    for u, label in enumerate(c):
        a, b = int(span[u, 0]), int(span[u, 1])
        assert prev < a <= b < end, (span.tolist(), u)
        path[a:b + 1] = label
        prev = b
    return path


def path_probability(y, path) -> float:
    y = np.asarray(y, np.float64)
    return float(np.prod([y[t, k] for t, k in enumerate(path)]))


def value_bound(value64, steps: int):
    """The bound on ``|float32 value - float64 value|`` over the same float32 posteriors."""
    return (steps - 1) * 2.0 ** -24 * np.asarray(value64, np.float64) + 1e-37


def path_floor(value64, steps: int):
    """The least float64 probability a float32-optimal path can have."""
    return np.asarray(value64, np.float64) * (1.0 - 2 * (steps - 1) * 2.0 ** -24)


def posteriors32(L: int) -> np.ndarray:
    """``[70, 19, L]`` float32: the float64 reference model's posteriors of the 70 test windows, rounded to float32."""
    return np.ascontiguousarray(ctc64.reference(L)[2], np.float32)
