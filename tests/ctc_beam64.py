"""Helpers of the beam-search tests: enumeration of all paths, seeded tables, the grid of sixteenths, and which windows float64
decides.  The statement itself is ``wwhip.ctc.beam_search`` (``csrc/ctc_beam.h`` in float64)."""
import itertools

import numpy as np

import ctc64

T = ctc64.STEPS


def enumerate_strings(y) -> dict:
    """``{label string: P(decode == string)}`` of one ``[T, L]`` table by enumeration of all ``L^T`` paths, in float64."""
    y = np.asarray(y, np.float64)
    steps, L = y.shape
    out: dict = {}
    for path in itertools.product(range(L), repeat=steps):
        p = 1.0
        for t, c in enumerate(path):
            p *= y[t, c]
        s, prev = [], -1
        for c in path:
            if c != L - 1 and c != prev:
                s.append(c)
            prev = c
        out[tuple(s)] = out.get(tuple(s), 0.0) + p
    return out


def strings_of(beam, i: int = 0) -> list:
    """Window ``i`` of a ``CtcBeam`` -> ``[(label string or None, prob)]`` per reported place (``None``: absent).  The strings are
    whole only where ``max_labels`` did not cut them."""
    out = []
    for p in range(beam.lengths.shape[1]):
        n = int(beam.lengths[i, p])
        out.append((None if n < 0 else tuple(int(c) for c in beam.labels[i, p, :n]), beam.probs[i, p]))
    return out


def random_tables(seed: int = 20262, n: int = 1000):
    """``[(steps [T, L] float32, W, P, max_labels)]``: tests/test_ctc_score_native.py's recipe restricted to T <= 19 and L <= 8 - the
    first tables walk the (T, W) corners; a third lie on a grid of sixteenths (exact zeros and ties), a third carry a blank that wins
    often; every eleventh holds a NaN, every thirteenth an Inf."""
    rng = np.random.default_rng(seed)
    corners = [(T_, W) for T_ in (1, 2, 3, 18, 19) for W in (1, 2, 7, 64)]
    widths = (1, 2, 3, 4, 7, 8, 16, 31, 64)
    out = []
    for i in range(n):
        T_, W = corners[i] if i < len(corners) else (int(rng.integers(1, 20)), int(widths[rng.integers(0, len(widths))]))
        L = int(rng.integers(2, 9))
        s = rng.dirichlet(np.full(L, 0.4), T_).astype(np.float32)
        if i % 3 == 0:
            s = np.round(s * 16) / np.float32(16)
        elif i % 3 == 1:
            s[:, L - 1] += np.float32(0.5)
        if i % 11 == 10:
            s[rng.integers(0, T_), rng.integers(0, L)] = np.nan
        if i % 13 == 12:
            s[rng.integers(0, T_), rng.integers(0, L)] = np.inf
        P = int(rng.integers(1, min(W, 8) + 1))
        out.append((np.ascontiguousarray(s, np.float32), W, P, int(rng.integers(1, T_ + 1))))
    return out


def sixteenths(rng, n: int, steps: int, L: int) -> np.ndarray:
    """``[n, steps, L]`` float32 posteriors on a grid of sixteenths: exact zeros, equal totals (every product is exact in float32)."""
    y = rng.dirichlet(np.full(L, 0.6), (n, steps))
    return (np.round(y * 16) / 16).astype(np.float32)


def tables(rng, n: int, steps: int, L: int) -> np.ndarray:
    """Posteriors with a peak per row, every third sequence on the grid of sixteenths."""
    y = rng.dirichlet(np.full(L, 0.3), (n, steps)).astype(np.float32)
    y[::3] = np.round(y[::3] * 16) / np.float32(16)
    return y


def same_bits(a, b, msg="") -> None:
    """Two ``CtcBeam``: equal labels, lengths and probability BITS."""
    np.testing.assert_array_equal(a.labels, b.labels, err_msg=f"labels {msg}")
    np.testing.assert_array_equal(a.lengths, b.lengths, err_msg=f"lengths {msg}")
    np.testing.assert_array_equal(np.ascontiguousarray(a.probs, np.float32).view(np.uint32), np.ascontiguousarray(b.probs, np.float32).view(np.uint32),
                                  err_msg=f"probs {msg}")


def decidable(trace, W: int, P: int, bound: float) -> np.ndarray:
    """Per window of a ``beam_search(..., trace=)`` run in float64: at every step the totals of the W-th and the (W + 1)-th
    candidate, and the final totals of places 0 .. P, lie farther apart than ``2 bound`` relative to the larger - so float32
    arithmetic within ``bound`` of float64 prunes and orders the same way.  A step with at most W candidates decides nothing."""
    out = np.ones(len(trace), bool)

    def apart(a, b):
        if a == 0.0:  # both exactly 0 (a posterior of 0 on every path): the key orders them, in any arithmetic
            return True
        return (a - b) > 2.0 * bound * a
    for i, steps in enumerate(trace):
        for rank, _ in steps:
            if len(rank) > W and not apart(float(rank[W - 1]), float(rank[W])):
                out[i] = False
        last = steps[-1][0]
        for p in range(min(P, len(last) - 1)):
            if not apart(float(last[p]), float(last[p + 1])):
                out[i] = False
    return out
