"""The evaluator tail in float64, the way the reference runs it (utils/evaluate_models.py:185-218, :80-99; wwdetect/wfst.py:17-71).
NumPy only; the yardstick of tests/test_gpu_sweep64.py and the statement tests/test_sweep64.py pins.

``smooth`` is tests/events64.py's: the reference's literal ``np.convolve(..., 'same')``.  ``np.convolve`` sums its products in another
order than the library's ascending chain ``acc += x[j] * (1.0 / win)``, so the two differ in the last bits: ``smooth_bound`` says by
how much at most, and a count is compared with this file only where no smoothed value is nearer to a threshold than twice that
(``margin``).  Inputs whose values are multiples of 2^-10 with a power-of-two window have no rounding at all and need neither.

The second half of the file makes the inputs that the CPU test (which pins their margins on the reference alone) and the GPU test
(which runs them through the library) share."""
import itertools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import events64 as E  # noqa: E402

smooth = E.smooth
LN2 = 0.6931471805599453                        # float64(-log(1 / 2)): the start arc of the lattice
DEFAULT_THR = np.arange(0.5, 0.99999, 0.005)    # utils/evaluate_models.py:185
_CELLS = 1 << 25                                # rows x thresholds held at once by counts / accepts


def counts(sm, thr):
    """The reference's ``prev_wake`` loop (:206-216) for every threshold: how many rows are above (``sm[i] > t``, so a NaN is not)
    while the row before is not above or does not exist."""
    sm = np.asarray(sm, np.float64).ravel()
    thr = np.asarray(thr, np.float64).ravel()
    out = np.zeros(thr.size, np.int64)
    if sm.size == 0:
        return out
    step = max(1, _CELLS // sm.size)
    for k in range(0, thr.size, step):
        above = sm[None, :] > thr[k:k + step, None]
        out[k:k + step] = above[:, 0] + (above[:, 1:] & ~above[:, :-1]).sum(axis=1)
    return out


def accepts(pos, thr):
    """``(pos > np.float32(t)).sum()`` per threshold for float32 ``pos``: the comparison NumPy 1.19.5 - which the reference pins - makes
    between a float32 array and a float64 scalar, written out so that it does not depend on the NumPy that runs this file."""
    pos = np.asarray(pos)
    assert pos.dtype == np.float32, pos.dtype
    pos = pos.ravel()
    t32 = np.asarray(thr, np.float64).ravel().astype(np.float32)
    out = np.zeros(t32.size, np.int64)
    step = max(1, _CELLS // max(pos.size, 1))
    for k in range(0, t32.size, step):
        out[k:k + step] = (pos[None, :] > t32[k:k + step, None]).sum(axis=1)
    return out


def pick(rows, n_out, pidx, offs=None):
    """Element ``pidx`` of the rows ``[n][n_out]`` (:80,86), or with a table of ``n_seg + 1`` offsets - clamped to ``[0, n]`` - ``np.max``
    of each run (:98-99): a NaN in a run makes the run NaN.  The reference never takes the maximum of nothing; here it is -inf."""
    col = np.asarray(rows, np.float32).reshape(-1, n_out)[:, pidx]
    if offs is None:
        return col.copy()
    offs = np.clip(np.asarray(offs, np.int64), 0, col.size)
    out = np.full(offs.size - 1, -np.inf, np.float32)
    for s in range(offs.size - 1):
        if offs[s + 1] > offs[s]:
            out[s] = np.max(col[offs[s]:offs[s + 1]])
    return out


def smooth_bound(neg, win):
    """Per row ``2 * (win + 2) * 2^-53 * sum |neg[j]| / win`` over the row's window: how far the library's smoothed value may be from
    ``smooth``'s.  Each of the two sums has ``win`` products ``x[j] * v`` and ``win - 1`` additions, with ``v`` = 1 / win rounded once,
    so either is within ``(win + 2) * 2^-53 * sum |x[j]| / win`` of the exact value, whatever its order.
    ``win <= 0``: 0, nothing is rounded.  (The window's ``sum |x| / win`` is taken with ``smooth`` itself: the same rows, and its own
    rounding is 1e-15 of a bound.)"""
    a = np.abs(np.nan_to_num(np.asarray(neg, np.float64), nan=0.0))
    if win <= 0:
        return np.zeros(a.size)
    return 2.0 * (win + 2) * 2.0 ** -53 * smooth(a, win)


def margin(sm, thr):
    """The smallest ``|sm[i] - t|`` over all rows and thresholds - ``events64.margin`` for many thresholds at once (NaN rows, which are
    above nothing whatever the threshold, left out)."""
    s = np.sort(np.asarray(sm, np.float64).ravel())
    s = s[~np.isnan(s)]
    thr = np.asarray(thr, np.float64).ravel()
    if s.size == 0 or thr.size == 0:
        return np.inf
    at = np.searchsorted(s, thr)
    below = np.abs(thr - s[np.clip(at - 1, 0, s.size - 1)])
    above = np.abs(s[np.clip(at, 0, s.size - 1)] - thr)
    return float(np.minimum(below, above).min())


def margin_holds(neg, win, thr):
    """``(margin, needed)``: the smallest distance of a float64 smoothed value from a threshold, and twice the largest
    ``smooth_bound`` of the input - counts are compared with this file where the first exceeds the second."""
    return margin(smooth(neg, win), thr), 2.0 * float(smooth_bound(neg, win).max(initial=0.0))


def viterbi_cost(costs, path, stay_bonus):
    """The float32 cost of state paths through the 2 x T lattice, accumulated in time order as the lattice does: the start arc
    ``float32(ln 2 + c[0][p])`` (a float64 sum), then ``d + (c - bonus)`` where the state stays and ``d + c`` where it changes.
    ``costs [..., T, 2]`` and ``path [..., T]`` broadcast against each other."""
    c = np.asarray(costs, np.float32)
    p = np.asarray(path, np.int64)
    lead = np.broadcast_shapes(c.shape[:-2], p.shape[:-1])
    c = np.broadcast_to(c, lead + c.shape[-2:])
    p = np.broadcast_to(p, lead + p.shape[-1:])
    at = np.take_along_axis(c, p[..., None], axis=-1)[..., 0]      # [..., T]: the cost of the state the path is in
    b = np.float32(stay_bonus)
    with np.errstate(invalid="ignore", over="ignore"):
        d = (LN2 + at[..., 0].astype(np.float64)).astype(np.float32)
        for t in range(1, p.shape[-1]):
            stay = p[..., t] == p[..., t - 1]
            d = np.where(stay, d + (at[..., t] - b), d + at[..., t]).astype(np.float32)
    return d


def viterbi_best(costs, stay_bonus):
    """The smallest ``viterbi_cost`` over all ``2^T`` paths, per superframe (``costs [n, T, 2]``).  float32 addition is monotone, so
    the lattice's recursion ends at this value whatever way it breaks ties."""
    c = np.asarray(costs, np.float32)
    T = c.shape[-2]
    paths = np.array(list(itertools.product((0, 1), repeat=T)), np.int64)   # [2^T, T]
    return viterbi_cost(c[:, None], paths[None], stay_bonus).min(axis=1)


# ---------------------------------------------------------------- inputs shared by tests/test_sweep64.py and tests/test_gpu_sweep64.py
WINDOWS = (0, 1, 2, 3, 29, 30, 31, 32)
TRIP_SWEEP = 2048 * 256      # rows one trip of sweep_kernel's grid takes (ww_k_far_frr's cap)
TRIP_SMOOTH = 4096 * 256     # and of smooth_kernel's
BIG_THR = {30: np.array([0.40, 0.44, 0.46, 0.48, 0.51, 0.55, 0.80, 0.95]),     # 8 thresholds: through the noise's smoothed values, and two
           1: np.array([0.30, 0.45, 0.51, 0.55, 0.70, 0.85, 0.95, 0.96])}      # that (window 30) only the placed 0.97 runs are above
THR_COUNTS = (1, 255, 256, 257, 1024)


def noise(seed, n):
    """Posteriors as the evaluator tests draw them: ``clip(normal(0.45, 0.2))`` in float32."""
    return np.clip(np.random.default_rng(seed).normal(0.45, 0.2, n), 0, 1).astype(np.float32)


def lengths(win):
    """The stream lengths of the smoothing cases of one window: ``win``, ``win + 1`` (at least 1), 255, 256, 257, 5000."""
    return sorted({max(win, 1), max(win, 1) + 1, 255, 256, 257, 5000})


def smoothing_cases(win):
    """``[(name, neg)]``: one seeded stream per length of ``lengths(win)``.  (Window 2 at 5,000 rows has its own seed: the first one
    put a clipped 1.0 next to a clipped 0, whose mean is the threshold 0.5 itself - no margin.)"""
    seeds = {(2, 5000): 5000}
    return [(f"win {win} n {n}", noise(seeds.get((win, n), 1000 + 37 * win + k), n)) for k, n in enumerate(lengths(win))]


def constant_cases(win):
    """``[(name, neg, count)]``: every value 1.0 and every value 0, at ``max(win, 1)`` and at 257 rows, with the number of rises at every
    default threshold - one (the smoothed values climb to the plateau near 1 and fall again: one run) and none.  At the edge rows of
    the all-ones streams a smoothed value IS a threshold (15 / 30 = 0.5), so no margin exists and the count is stated instead."""
    out = []
    for n in sorted({max(win, 1), 257}):
        out.append((f"win {win} n {n} ones", np.ones(n, np.float32), 1))
        out.append((f"win {win} n {n} zeros", np.zeros(n, np.float32), 0))
    return out


def dyadic_case(win):
    """5,000 multiples of 2^-10 in [0, 1] - every product and partial sum of a power-of-two window is exact - and thresholds taken from
    the float64 smoothed values themselves: 40 distinct ones with their float64 neighbours below and above."""
    rng = np.random.default_rng(2000 + win)
    neg = (rng.integers(0, 1025, 5000) / 1024.0).astype(np.float32)
    vals = np.unique(smooth(neg, win))
    vals = rng.choice(vals, min(40, vals.size), replace=False)
    thr = np.concatenate([vals, np.nextafter(vals, -np.inf), np.nextafter(vals, np.inf)])
    return neg, thr


def big_cases():
    """``[(name, neg, win, thr)]`` past one trip of the grids: 2048 * 256 + 1 and 4096 * 256 + 777 rows of noise.  ``run``: 80 rows of
    0.97 straddle each of the rows 524,288 and 1,048,576 that exist (the row before a trip's first row is above too: no rise there).
    ``rise``, window 1 only: row b - 1 is 0.2 and row b 0.9 (a rise exactly on a trip's first row)."""
    out = []
    for n, seed in ((TRIP_SWEEP + 1, 3001), (TRIP_SMOOTH + 777, 3002)):
        bounds = [b for b in (TRIP_SWEEP, TRIP_SMOOTH) if b < n]
        for win, kind in ((30, "run"), (1, "run"), (1, "rise")):
            neg = noise(seed + win + (kind == "rise"), n)
            for b in bounds:
                if kind == "run":
                    neg[b - 40:min(b + 40, n)] = 0.97
                else:
                    neg[b - 1], neg[b] = 0.2, 0.9
            out.append((f"n {n} win {win} {kind}", neg, win, BIG_THR[win]))
    return out


def threshold_list(n_thr):
    """``n_thr`` ascending thresholds across the smoothed values of ``threshold_stream()``."""
    return 0.30 + 0.40 * (np.arange(n_thr) + 0.5) / n_thr


def threshold_stream():
    """20,000 rows of noise (window 30) and 300 positives for the threshold-count cases."""
    return noise(4001, 20_000), np.random.default_rng(4002).uniform(0.2, 1.0, 300).astype(np.float32)


def float32_rule_thresholds():
    """From the default thresholds plus 0.1 and 0.3: ``(up, down)``, those whose float32 value is above them and below them."""
    cand = np.concatenate([DEFAULT_THR, [0.1, 0.3]])
    f = cand.astype(np.float32).astype(np.float64)
    return cand[f > cand], cand[f < cand]


def float32_rule_positives(t):
    """``float32(t)`` and its two float32 neighbours: ``[below, at, above]``.  Under the float32 rule exactly one of them - the last - is
    above ``t``, on whichever side of ``t`` its float32 value lies; a float64 comparison also accepts ``float32(t)`` where that is > t."""
    f = np.float32(t)
    return np.array([np.nextafter(f, np.float32(-np.inf)), f, np.nextafter(f, np.float32(np.inf))], np.float32)
