"""The Viterbi alignment on the host: ``wwhip.ctc.align`` (the float64 statement of csrc/ctc_align.h) against the enumeration of every
path, hand cases and the tie rules through it and through the library's host function (``ww_ctc_align_rows``), that function against
the float64 statement on the same float32 posteriors, its refusals, and the step -> row arithmetic."""

import numpy as np
import pytest

import ctc64
import ctc_align64 as A64
from wwhip import ctc

B = 3  # the blank of the L = 4 hand cases

# (T, target), L = 3; the seed of case i is 500 + i (chosen on the float64 enumeration alone: the margin below holds for each)
ENUM_CASES = [(6, (0, 1)), (6, (0, 0)), (6, (1, 0)), (5, (1,)), (5, (1, 1)), (4, (0, 1)), (3, (0, 0)), (3, (1, 0)), (2, (0, 0)), (2, (0, 1)),
              (1, (0,)), (1, (0, 1)), (6, (1,))]


@pytest.mark.parametrize("i", range(len(ENUM_CASES)))
@pytest.mark.parametrize("mode", A64.MODES)
def test_float64_statement_equals_path_enumeration(i, mode):
    T, c = ENUM_CASES[i]
    y = np.random.default_rng(500 + i).dirichlet(np.ones(3), T)
    best, path, second = A64.enumerate_best(y, c, mode)
    got = ctc.align(y, [c], mode)
    print(f"\nT={T} c={c} {mode}: best {best:.17g} second {second:.17g} got {got.value[0, 0]:.17g} path {got.paths[0][0]}", end="")
    if path is None:
        assert T < len(c) + sum(a == b for a, b in zip(c, c[1:]))
        assert got.value[0, 0] == 0.0 and got.paths[0][0] is None and (got.span == -1).all()
        return
    assert best - second > 1e-6 * best   # the margin, on the enumeration alone
    assert abs(got.value[0, 0] - best) <= 1e-12 * best
    np.testing.assert_array_equal(got.paths[0][0], path)
    np.testing.assert_array_equal(A64.path_of_span(got.span[0, 0], c, T, 3, mode), path)


def _both(y, targets, mode):
    """The float64 statement and the library's host function on the same rows: they must agree on the spans here."""
    a, r = ctc.align(y, targets, mode), ctc.align_rows(y, targets, mode)
    np.testing.assert_array_equal(a.span, r.span)
    np.testing.assert_allclose(r.value, a.value, rtol=64 * 2.0 ** -24, atol=0)
    assert r.value.dtype == np.float32 and r.span.dtype == np.int32
    return r


def test_hey_snips_rows():
    y = ctc64._rows([B, 1, 1, B, B, 2, 2, B], 4)
    e, p = _both(y, [(1, 2)], "exact"), _both(y, [(1, 2)], "prefix")
    assert e.span[0, 0].tolist() == [[1, 2], [5, 6]]
    assert p.span[0, 0].tolist() == [[1, 2], [5, 5]]
    hi = np.float64(y[0, B])
    np.testing.assert_allclose(e.value[0, 0], hi ** 8, rtol=1e-6)
    np.testing.assert_allclose(p.value[0, 0], hi ** 6, rtol=1e-6)
    np.testing.assert_array_equal(ctc.align(y, [(1, 2)], "exact").paths[0][0], [B, 1, 1, B, B, 2, 2, B])
    np.testing.assert_array_equal(ctc.align(y, [(1, 2)], "prefix").paths[0][0], [B, 1, 1, B, B, 2])


def test_equal_labels_take_the_blank_where_it_is_cheapest():
    """Target (1, 1) on rows that all favour label 1: the path must spend one step on the blank, and takes step 2, where the blank
    has 0.4."""
    y = ctc64._rows([1, 1, 1, 1], 4)
    y[2] = [0.05, 0.5, 0.05, 0.4]
    e, p = _both(y, [(1, 1)], "exact"), _both(y, [(1, 1)], "prefix")
    assert e.span[0, 0].tolist() == [[0, 1], [3, 3]] and p.span[0, 0].tolist() == [[0, 1], [3, 3]]
    np.testing.assert_allclose(e.value[0, 0], 0.9 * 0.9 * 0.4 * 0.9, rtol=1e-6)
    # three steps hold 1, blank, 1 and nothing else; two steps hold nothing
    assert _both(y[:3], [(1, 1)], "exact").span[0, 0].tolist() == [[0, 0], [2, 2]]
    for mode in A64.MODES:
        r = _both(y[:2], [(1, 1)], mode)
        assert r.value[0, 0] == 0.0 and (r.span == -1).all()


def test_too_few_steps_and_one_step():
    y = np.array([[0.7, 0.2, 0.1]], np.float32)
    for mode in A64.MODES:
        r = _both(y, [(0, 1), (0,), (1,)], mode)
        assert r.value[:, 0].tolist() == [0.0, np.float32(0.7), np.float32(0.2)]
        assert r.span[:, 0].tolist() == [[[-1, -1], [-1, -1]], [[0, 0], [-1, -1]], [[0, 0], [-1, -1]]]
        r = _both(np.array([[0.75, 0.25]], np.float32), [(0,)], mode)   # L = 2, U = 1, T = 1
        assert r.value[0, 0] == 0.75 and r.span[0, 0].tolist() == [[0, 0]]


def test_tie_rules_on_rows_of_equal_posteriors():
    """0.25 everywhere is exact in float32, so every candidate that is reachable ties and the rules decide.  Exact: state 2U - 1
    beats 2U (the path ends on the last label, not on a blank behind it) and stay beats shift (going back from the end the path
    stays on a label as long as the label was reachable): 1, 2, 2, 2, 2.  Prefix: q_t falls by 0.25 a step, t* = 1.  On rows of ones
    every q_t ties: the earliest t* wins."""
    y = np.full((5, 4), 0.25, np.float32)
    e, p = _both(y, [(1, 2), (1,), (1, 1)], "exact"), _both(y, [(1, 2), (1,), (1, 1)], "prefix")
    assert (e.value == 0.25 ** 5).all()
    assert e.span[:, 0].tolist() == [[[0, 0], [1, 4]], [[0, 4], [-1, -1]], [[0, 0], [2, 4]]]
    assert p.value[:, 0].tolist() == [0.25 ** 2, 0.25, 0.25 ** 3]
    assert p.span[:, 0].tolist() == [[[0, 0], [1, 1]], [[0, 0], [-1, -1]], [[0, 0], [2, 2]]]
    ones = np.ones((6, 4), np.float32)
    e, p = _both(ones, [(1, 2), (2, 2)], "exact"), _both(ones, [(1, 2), (2, 2)], "prefix")
    assert (e.value == 1).all() and (p.value == 1).all()
    assert e.span[:, 0].tolist() == [[[0, 0], [1, 5]], [[0, 0], [2, 5]]]
    assert p.span[:, 0].tolist() == [[[0, 0], [1, 1]], [[0, 0], [2, 2]]]


def test_an_exact_zero_on_the_only_path():
    y = ctc64._rows([1, 2], 4)
    assert _both(y, [(1, 2)], "exact").span[0, 0].tolist() == [[0, 0], [1, 1]]
    y[1, 2] = 0.0
    for mode in A64.MODES:
        r = _both(y, [(1, 2), (1,)], mode)
        assert r.value[0, 0] == 0.0 and (r.span[0] == -1).all()
        assert r.value[1, 0] > 0 and r.span[1, 0, 0, 0] == 0   # the other target of the call is not touched by it
    # a zero that only closes one of two ways: 1, 2, 2 is gone, 1, 1, 2 stays
    y = ctc64._rows([1, 2, 2], 4)
    y[1] = [0.05, 0.5, 0.0, 0.45]
    assert _both(y, [(1, 2)], "exact").span[0, 0].tolist() == [[0, 1], [2, 2]]


@pytest.mark.parametrize("L", ctc64.LS)
@pytest.mark.parametrize("mode", A64.MODES)
def test_host_function_against_the_float64_statement(L, mode):
    """``ww_ctc_align_rows`` on the reference model's 70 windows of float32 posteriors: the value within T - 1 roundings of the
    float64 value, and the float32 path - rebuilt from its spans - an optimal path up to rounding (not necessarily the same path)."""
    y = A64.posteriors32(L)
    assert y.shape == (ctc64.N_WINDOWS, A64.T, L)
    tg = A64.TARGETS[L]
    a, r = ctc.align(y, tg, mode), ctc.align_rows(y, tg, mode)
    worst_v = worst_p = 0.0
    for k, c in enumerate(tg):
        for i in range(y.shape[0]):
            v64, v32 = a.value[k, i], float(r.value[k, i])
            err, bound = abs(v32 - v64), A64.value_bound(v64, A64.T)
            worst_v = max(worst_v, err / bound)
            assert err <= bound, (k, i, v32, v64)
            if v32 == 0.0:
                assert (r.span[k, i] == -1).all()
                continue
            path = A64.path_of_span(r.span[k, i, :len(c)], c, A64.T, L, mode)
            assert A64.collapse(path, L) == list(c) and (r.span[k, i, len(c):] == -1).all()
            p64 = A64.path_probability(y[i], path)
            worst_p = max(worst_p, (v64 - p64) / v64)
            assert p64 >= A64.path_floor(v64, A64.T), (k, i, p64, v64)
    print(f"\nL={L} {mode}: worst |v32 - v64| / bound {worst_v:.3g}; worst (v64 - p64(path32)) / v64 {worst_p:.3g}; "
          f"values {a.value.min():.3g} .. {a.value.max():.3g}", end="")
    assert (a.value > 0).all()


def test_host_function_refuses_before_it_writes():
    from wwhip import _lib
    lib = _lib.load()
    y = np.full((2, 3, 4), 0.25, np.float32)
    tab, lens = ctc.pack_targets([(1, 2)], 4)

    def call(T=3, L=4, tab=tab, lens=lens, K=1, mode=0, no_value=False, no_span=False, n=2):
        value, span = np.full((8, 2), -7.0, np.float32), np.full((8, 2, 9, 2), 77, np.int8)
        rc = lib.ww_ctc_align_rows(_lib.ptr(y), n, T, L, _lib.ptr(tab), _lib.ptr(lens), K, mode, None if no_value else _lib.ptr(value),
                                   None if no_span else _lib.ptr(span))
        if rc or n == 0:
            assert (value == -7.0).all() and (span == 77).all()
        return rc, (lib.ww_last_error(None) or b"").decode(), value, span

    rc, _, value, span = call()
    assert rc == 0 and (value[0] == 0.25 ** 3).all() and (value[1:] == -7.0).all()
    assert (span[0, :, 2:] == -1).all() and (span[0, :, :2] >= 0).all() and (span[1:] == 77).all()
    for kw, word in ((dict(T=0), "T = 0"), (dict(T=65), "T = 65"), (dict(L=1), "L = 1"), (dict(L=65), "L = 65"), (dict(K=0), "K = 0"), (dict(K=9), "K = 9"),
                     (dict(mode=2), "mode"), (dict(mode=-1), "mode"), (dict(lens=np.array([0], np.int32)), "U = 0"),
                     (dict(lens=np.array([10], np.int32)), "U = 10"), (dict(tab=np.full((1, 9), 3, np.int32)), "label"),
                     (dict(tab=np.full((1, 9), -1, np.int32)), "label"), (dict(tab=None), "NULL"), (dict(lens=None), "NULL"),
                     (dict(no_value=True), "NULL"), (dict(no_span=True), "NULL"), (dict(n=-1), "negative")):
        rc, text = call(**kw)[:2]
        assert rc == _lib.WW_EINVAL and word in text, (kw, rc, text)
    assert call(n=0)[0] == 0


def test_refusals_of_the_python_statement():
    y = np.full((3, 4), 0.25)
    for bad in ([(3,)], [(-1,)], [()], [(0,) * 10], [(0,)] * 9, []):
        with pytest.raises(ValueError):
            ctc.align(y, bad)
        with pytest.raises(ValueError):
            ctc.align_rows(y, bad)
    with pytest.raises(ValueError):
        ctc.align(y, [(0,)], "loss")
    with pytest.raises(ValueError):
        ctc.align(np.zeros((3, 1)), [(0,)])


def test_step_rows_and_span_seconds():
    """KT = 20, ST = 8, PT = 6: conv step t reads rows 8 t - 6 .. 8 t + 13 of the 151-row window."""
    first, last = ctc.step_rows(np.arange(19))
    assert first.tolist() == [0] + [8 * t - 6 for t in range(1, 19)] and last.tolist() == [8 * t + 13 for t in range(18)] + [150]
    assert [int(v) for v in ctc.step_rows(1)] == [2, 21] and [int(v) for v in ctc.step_rows(18)] == [138, 150]
    span = np.array([[[1, 2], [5, 6], [-1, -1]], [[0, 0], [18, 18], [-1, -1]]])
    assert ctc.span_rows(span).tolist() == [[[2, 29], [34, 61], [-1, -1]], [[0, 13], [138, 150], [-1, -1]]]
    assert ctc.span_rows(span, np.array([[100], [-150]])).tolist() == [[[102, 129], [134, 161], [-1, -1]], [[-150, -137], [-12, 0], [-1, -1]]]
    sec = ctc.span_seconds(span, 100)
    np.testing.assert_allclose(sec[0, :2], [[1.02, 1.30], [1.34, 1.62]], rtol=1e-12)
    assert np.isnan(sec[:, 2]).all()
