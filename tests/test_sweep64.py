"""tests/sweep64.py - the float64 statement of the evaluator tail - pinned without a GPU: against tests/events64.py's walk, the two
oracles and the golden fixture; the float32 rule for positives; the exactness that lets the dyadic GPU cases ask for equal bits;
and, on the reference alone, the margin of every input that tests/test_gpu_sweep64.py compares with float64 counts."""
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import events64 as E  # noqa: E402
import sweep64 as S  # noqa: E402

from oracle import cpu  # noqa: E402
from oracle import numpy_ref as NR  # noqa: E402


def _chain(neg, win):
    """The library's rule (include/wwhip.h): the ascending chain ``acc += (double)x[j] * (1.0 / win)`` over the row's clipped window."""
    x = np.asarray(neg, np.float64)
    v = 1.0 / win
    shift = (win - 1) // 2
    out = np.zeros(x.size)
    for i in range(x.size):
        acc = 0.0
        for j in range(max(i + shift - (win - 1), 0), min(i + shift, x.size - 1) + 1):
            acc += x[j] * v
        out[i] = acc
    return out


def test_counts_are_the_walk_and_the_oracle():
    neg = S.noise(11, 3000)
    sm = S.smooth(neg, 30)
    got = S.counts(sm, S.DEFAULT_THR)
    assert got.max() > 10 and got.min() == 0
    np.testing.assert_array_equal(got, [len(E.walk(sm, t)) for t in S.DEFAULT_THR])
    pos = np.random.default_rng(12).uniform(0.3, 1, 200).astype(np.float32)
    frr, far, cnt, sm_ref = NR.far_frr(pos, neg, 200, 1.5)
    np.testing.assert_array_equal(sm_ref, sm)
    np.testing.assert_array_equal(got, cnt)
    np.testing.assert_array_equal((200 - S.accepts(pos, S.DEFAULT_THR)) / 200, frr)
    np.testing.assert_array_equal(got, cpu.far_frr(pos, sm, S.DEFAULT_THR, 200, 1.5)[2])
    # NaN rows are above nothing; a run may begin on the row after one
    sm = np.array([np.nan, 0.9, 0.9, np.nan, 0.9, 0.1, np.nan])
    np.testing.assert_array_equal(S.counts(sm, [0.5, 0.95, -1.0]), [2, 0, 2])
    np.testing.assert_array_equal(S.counts(sm, [0.5]), [len(E.walk(sm, 0.5))])
    np.testing.assert_array_equal(S.counts(np.zeros(0), [0.5]), [0])


@pytest.mark.parametrize("case", ["short", "long", "exact30"])
def test_statement_reproduces_the_golden_evaluator(golden, case):
    z = np.load(os.path.join(golden, "evaluator.npz"))
    sm = S.smooth(z[case + ".neg"], 30)
    np.testing.assert_allclose(sm, z[case + ".smoothed"], rtol=0, atol=1e-15)   # (np.convolve's order of summation is its build's)
    np.testing.assert_array_equal(S.counts(sm, S.DEFAULT_THR), z[case + ".cnt"])
    np.testing.assert_array_equal(S.counts(z[case + ".smoothed"], S.DEFAULT_THR), z[case + ".cnt"])
    pos = z[case + ".pos"]
    assert pos.dtype == np.float32
    np.testing.assert_array_equal((200 - S.accepts(pos, S.DEFAULT_THR)) / 200, z[case + ".frr"])


def test_margin_is_events64_margin():
    sm = S.smooth(S.noise(13, 700), 30)
    thr = S.DEFAULT_THR[:40]
    assert S.margin(sm, thr) == min(E.margin([[sm]], t) for t in thr)
    assert S.margin(np.array([0.25, np.nan, 0.75]), [0.5, 0.7]) == pytest.approx(0.05)
    assert S.margin(np.zeros(0), [0.5]) == np.inf


@pytest.mark.parametrize("win", [1, 2, 4, 32])
def test_dyadic_streams_have_no_rounding(win):
    """Multiples of 2^-10 and a power-of-two window: np.convolve and the library's ascending chain agree bit for bit, which is what lets
    the dyadic GPU cases ask for equal bits and equal counts at thresholds that ARE smoothed values."""
    neg, thr = S.dyadic_case(win)
    sm = S.smooth(neg, win)
    np.testing.assert_array_equal(sm[:600], _chain(neg, win)[:600])
    np.testing.assert_array_equal(sm[-600:], _chain(neg, win)[-600:])
    assert np.all(sm * (1024 * win) == np.round(sm * (1024 * win)))   # every value a multiple of 2^-10 / win: the sums were exact
    assert thr.size >= 90 and np.isin(thr, sm).sum() >= 30
    c = S.counts(sm, thr).reshape(3, -1)
    assert np.any(c[0] != c[1])   # a threshold equal to a smoothed value counts other rises than the one just below: '>' against '>='


def test_smooth_bound_covers_the_two_summation_orders():
    """The bound is derived, not measured; this only checks that the derivation is not contradicted (and not vacuous by orders of
    magnitude) where both sums can be written down here."""
    worst = 0.0
    for win in (2, 3, 29, 30, 31, 32):
        neg = S.noise(500 + win, 400)
        d = np.abs(_chain(neg, win) - S.smooth(neg, win))
        b = S.smooth_bound(neg, win)
        assert np.all(d <= b), win
        worst = max(worst, float((d / np.maximum(b, 1e-300)).max()))
    assert S.smooth_bound(np.ones(64, np.float32), 30).max() == pytest.approx(2 * 32 * 2.0 ** -53, rel=1e-12)   # about 7e-15
    assert np.all(S.smooth_bound(S.noise(1, 9), 0) == 0)
    assert worst > 1e-3   # the two orders do differ: a comparison with no allowance would fail


def test_float32_rule_for_positives():
    """The reference's NumPy compares a float32 array with a float64 threshold in float32.  For a threshold t and the positives
    float32(t) and its two float32 neighbours, exactly ONE positive - the upper neighbour - is above t, on whichever side of t
    float32(t) lies.  A float64 comparison accepts two of them where float32(t) > t."""
    up, down = S.float32_rule_thresholds()
    assert up.size > 10 and down.size > 10 and 0.1 in up.tolist() + down.tolist()
    for t in np.concatenate([up, down]):
        pos = S.float32_rule_positives(t)
        assert pos[0] < pos[1] < pos[2] and pos[1] == np.float32(t)
        in64 = int((pos.astype(np.float64) > t).sum())
        assert in64 == (2 if t in up else 1)          # what the rule is NOT
        np.testing.assert_array_equal(S.accepts(pos, [t]), [1])
        thr = np.array([t])
        frr, _, _, _ = NR.far_frr(pos, np.zeros(1, np.float32), 3, 1.0, thr, windowsize=1)
        assert frr[0] == (3 - 1) / 3, t
        frr, _, _ = cpu.far_frr(pos, np.zeros(0), thr, 3, 1.0)
        assert frr[0] == (3 - 1) / 3, t
    # all of them in one call
    ts = np.concatenate([up, down])
    pos = np.concatenate([S.float32_rule_positives(t) for t in ts])
    want = S.accepts(pos, ts)
    np.testing.assert_array_equal((pos.size - want) / pos.size, NR.far_frr(pos, np.zeros(1, np.float32), pos.size, 1.0, ts, windowsize=1)[0])
    np.testing.assert_array_equal((pos.size - want) / pos.size, cpu.far_frr(pos, np.zeros(0), ts, pos.size, 1.0)[0])
    assert np.any(want != [(pos.astype(np.float64) > t).sum() for t in ts])


def test_pick_statement():
    rows = np.array([[0.1, 0.9], [0.5, np.nan], [-0.0, -np.inf], [0.7, 0.2]], np.float32)
    np.testing.assert_array_equal(S.pick(rows, 2, 0), np.array([0.1, 0.5, -0.0, 0.7], np.float32))
    np.testing.assert_array_equal(S.pick(rows, 2, 0, [0, 2, 2, 4]), np.array([0.5, -np.inf, 0.7], np.float32))
    got = S.pick(rows, 2, 1, [-3, 1, 2, 9])       # clamped to [0, 4]
    assert got[0] == np.float32(0.9) and np.isnan(got[1]) and got[2] == np.float32(0.2)


def test_viterbi_statement_against_the_restated_lattice():
    """``viterbi_cost`` of the path oracle/numpy_ref.wfst_smooth returns equals ``viterbi_best`` (stay bonus 1: the reference's), and the
    brute force agrees with a plain loop over the paths."""
    rng = np.random.default_rng(21)
    pp = rng.uniform(0.01, 0.99, (40, 6, 1)).astype(np.float32)
    pp = np.concatenate([1 - pp, pp], axis=2)
    costs = -np.log(pp)
    best = S.viterbi_best(costs, 1.0)
    paths = np.array([NR.wfst_smooth(x) for x in pp])
    np.testing.assert_array_equal(S.viterbi_cost(costs, paths, 1.0), best)
    for i in (0, 17):
        slow = []
        for path in itertools.product((0, 1), repeat=6):
            d = np.float32(S.LN2 + np.float64(costs[i, 0, path[0]]))
            for t in range(1, 6):
                c = costs[i, t, path[t]]
                d = np.float32(d + np.float32(c - np.float32(1.0))) if path[t] == path[t - 1] else np.float32(d + c)
            slow.append(d)
        assert best[i] == min(slow)
    # ties keep state 0
    half = np.full((1, 5, 2), -np.log(np.float32(0.5)), np.float32)
    assert S.viterbi_cost(half, np.zeros((1, 5), int), 2.5) == S.viterbi_best(half, 2.5)


# ---------------------------------------------------------------- the margins of the GPU test's inputs, on the reference alone
def _assert_margin(name, neg, win, thr):
    have, need = S.margin_holds(neg, win, thr)
    assert have > need, (name, have, need)


@pytest.mark.parametrize("win", S.WINDOWS)
def test_margin_of_the_smoothing_cases(win):
    for name, neg in S.smoothing_cases(win):
        _assert_margin(name, neg, win, S.DEFAULT_THR)
    # the constant streams have no margin (docstring of constant_cases): their count is stated, and the statement gives it
    for name, neg, count in S.constant_cases(win):
        np.testing.assert_array_equal(S.counts(S.smooth(neg, win), S.DEFAULT_THR), np.full(S.DEFAULT_THR.size, count), err_msg=name)


def test_margin_of_the_cases_past_one_trip():
    cases = S.big_cases()
    assert len(cases) == 6
    for name, neg, win, thr in cases:
        assert thr.size == 8
        _assert_margin(name, neg, win, thr)
        c = S.counts(S.smooth(neg, win), thr)
        assert c[0] > 1000, (name, c)
        if win == 30:   # the last threshold: only the runs placed across the trips' first rows are above it
            assert c[-1] == (neg.size > S.TRIP_SMOOTH) + 1, (name, c)


@pytest.mark.parametrize("n_thr", S.THR_COUNTS)
def test_margin_of_the_threshold_count_cases(n_thr):
    neg, _ = S.threshold_stream()
    thr = S.threshold_list(n_thr)
    _assert_margin(f"{n_thr} thresholds", neg, 30, thr)
    c = S.counts(S.smooth(neg, 30), thr)
    assert c.max() > 100 and (n_thr < 255 or np.unique(c).size > 20)
