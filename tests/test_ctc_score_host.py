"""The forward-algorithm score on the host: ``wwhip.ctc.score`` (the float64 statement of csrc/ctc_score.h) against enumeration of
every path, its orderings and exact zeros, hand cases, the library's host function (``ww_ctc_score_rows``) against the float32
form of the same statement, the score trigger rule against numpy, and the conditions the GPU tests rely on."""

import numpy as np
import pytest

import ctc64
import ctc_score64 as S64
from wwhip import ctc

ENUM_CASES = [(6, 3, (0, 1)), (6, 3, (1, 1)), (5, 4, (2,)), (7, 3, (0, 1, 0)), (6, 4, (1, 1, 2)), (7, 4, (0, 1)), (3, 3, (0, 0)), (2, 3, (0, 0)),
              (1, 2, (0,)), (1, 3, (0, 1)), (4, 4, (1, 1, 2))]


@pytest.mark.parametrize("T,L,c", ENUM_CASES)
def test_float64_statement_equals_path_enumeration(T, L, c):
    rng = np.random.default_rng(100 * T + L)
    y = rng.dirichlet(np.ones(L), T)
    exact, prefix = S64.enumerate_paths(y, c)
    got_e, got_p = ctc.score(y, [c], "exact")[0, 0], ctc.score(y, [c], "prefix")[0, 0]
    atol = L ** T * 2.0 ** -52   # the enumeration's own sum: L^T terms below 1, each addition rounded once
    print(f"\nT={T} L={L} c={c}: exact {got_e:.17g} (enumerated {exact:.17g}), prefix {got_p:.17g} ({prefix:.17g})", end="")
    assert abs(got_e - exact) <= atol and abs(got_p - prefix) <= atol
    if T < len(c) + sum(a == b for a, b in zip(c, c[1:])):
        assert got_e == 0.0 and got_p == 0.0 and exact == 0.0 and prefix == 0.0


def test_a_repeat_needs_a_blank_between():
    """``(0, 0)`` at T = 2 is exactly 0 (two steps cannot hold 0, blank, 0), at T = 3 it is the one path 0, blank, 0."""
    y = np.random.default_rng(3).dirichlet(np.ones(3), 3)
    for mode in S64.MODES:
        assert ctc.score(y[:2], [(0, 0)], mode)[0, 0] == 0.0
        np.testing.assert_allclose(ctc.score(y, [(0, 0)], mode)[0, 0], y[0, 0] * y[1, 2] * y[2, 0], rtol=1e-15)


@pytest.mark.parametrize("c,need", [((1, 1, 2), 4), ((0, 1, 0), 3), ((2,), 1), ((1, 1, 1), 5), ((0, 1, 2, 0, 1, 2, 0, 1, 2), 9), ((3, 3, 3, 3, 3, 3, 3, 3, 3), 17)])
def test_too_few_steps_give_exactly_zero(c, need):
    y = np.random.default_rng(len(c)).dirichlet(np.ones(5), need)
    for mode in S64.MODES:
        for dtype in (np.float64, np.float32):
            if need > 1:
                assert ctc.score(y[:need - 1], [c], mode, dtype)[0, 0] == 0.0
            assert ctc.score(y, [c], mode, dtype)[0, 0] > 0.0


def test_exact_is_below_prefix_is_below_one():
    rng = np.random.default_rng(8)
    for T, L in ((19, 4), (19, 8), (64, 3), (5, 2), (1, 6)):
        y = rng.dirichlet(np.full(L, 0.5), (40, T))
        tg = [tuple(rng.integers(0, L - 1, U)) for U in (1, 2, 3, 5, 9)]
        e, p = ctc.score(y, tg, "exact"), ctc.score(y, tg, "prefix")
        assert e.shape == p.shape == (5, 40) and (e >= 0).all()
        assert (e <= p * (1 + 1e-12)).all() and (p <= 1 + 1e-12).all()
        if T == 1:
            np.testing.assert_array_equal(e[0], p[0])   # one step, one label: the same single path
            assert (e[1:] == 0).all()


def test_hand_cases():
    """The "hey snips" rows of ``ctc64.hand_cases()`` - blank, 1, 1, blank, blank, 2, 2, blank at 0.9 - and the same rows at 1.0."""
    name, steps, _, labels, _ = [c for c in ctc64.hand_cases() if c[0] == "hey snips"][0]
    assert labels == [1, 2]
    y = steps.astype(np.float64)
    y /= y.sum(axis=1, keepdims=True)   # (float32 rows sum to 1 within an ulp; "starts with" leaves the rest of a path free, so it is
    hi, lo = y[0, 3], y[0, 0]           # the enumerated probability only on rows that sum to 1)
    for mode in S64.MODES:
        got = ctc.score(y, [(1, 2), (2, 1), (1,), (0,)], mode)[:, 0]
        want = [S64.enumerate_paths(y, c)[S64.MODES.index(mode)] for c in ((1, 2), (2, 1), (1,), (0,))]
        np.testing.assert_allclose(got, want, rtol=0, atol=4 ** 8 * 2.0 ** -52)
        # the greedy path alone is one of the target's alignments; moving one of its boundaries by a step is another
        assert got[0] > hi ** 8 + hi ** 7 * lo
        if mode == "exact":
            assert got[0] > 100 * got[1] and got[0] > 100 * got[2]   # "2 1" and "1" alone need two steps off the rows' peaks
        else:
            assert got[2] > got[0] > got[1]   # starts with "1" > starts with "1 2"; "2 1" needs a 2 on the first, blank, row
    one_hot = ctc64._rows([3, 1, 1, 3, 3, 2, 2, 3], 4, hi=1.0)
    for dtype in (np.float64, np.float32):
        np.testing.assert_array_equal(ctc.score(one_hot, [(1, 2), (2, 1), (1,), (2,)], "exact", dtype)[:, 0], [1, 0, 0, 0])
        np.testing.assert_array_equal(ctc.score(one_hot, [(1, 2), (2, 1), (1,), (2,)], "prefix", dtype)[:, 0], [1, 0, 1, 0])


def test_refusals_of_the_python_statement():
    y = np.full((3, 4), 0.25)
    for bad in ([(3,)], [(-1,)], [()], [(0,) * 10], [(0,)] * 9, []):
        with pytest.raises(ValueError):
            ctc.score(y, bad)
    with pytest.raises(ValueError):
        ctc.score(y, [(0,)], "loss")
    with pytest.raises(ValueError):
        ctc.score(np.zeros((3, 1)), [(0,)])


def test_host_function_carries_the_float32_statements_bits():
    """``ww_ctc_score_rows`` (csrc/ctc_score.h over host arrays) against the float32 form of ``ctc.score``: the same bits."""
    rng = np.random.default_rng(11)
    for T, L in ((19, 4), (64, 12), (1, 2), (2, 3), (33, 64)):
        y = rng.dirichlet(np.full(L, 0.3), (9, T)).astype(np.float32)
        tg = [tuple(rng.integers(0, L - 1, U)) for U in (1, 2, 4, 9)] + [(0, 0)]
        for mode in S64.MODES:
            np.testing.assert_array_equal(ctc.score_rows(y, tg, mode), ctc.score(y, tg, mode, np.float32))


def test_host_function_refuses_before_it_writes():
    from wwhip import _lib
    lib = _lib.load()
    y = np.full((2, 3, 4), 0.25, np.float32)
    tab, lens = ctc.pack_targets([(1, 2)], 4)

    def call(T=3, L=4, tab=tab, lens=lens, K=1, mode=0):
        out = np.full((8, 2), -7.0, np.float32)
        rc = lib.ww_ctc_score_rows(_lib.ptr(y), 2, T, L, _lib.ptr(tab), _lib.ptr(lens), K, mode, _lib.ptr(out))
        assert (out == -7.0).all() or rc == 0
        return rc, (lib.ww_last_error(None) or b"").decode()

    assert call()[0] == 0
    for kw, word in ((dict(T=0), "T = 0"), (dict(T=65), "T = 65"), (dict(L=1), "L = 1"), (dict(L=65), "L = 65"), (dict(K=0), "K = 0"), (dict(K=9), "K = 9"),
                     (dict(mode=2), "mode"), (dict(lens=np.array([0], np.int32)), "U = 0"), (dict(lens=np.array([10], np.int32)), "U = 10"),
                     (dict(tab=np.full((1, 9), 3, np.int32)), "label"), (dict(tab=np.full((1, 9), -1, np.int32)), "label")):
        rc, text = call(**kw)
        assert rc == _lib.WW_EINVAL and word in text, (kw, rc, text)
    out = np.full(4, -7.0, np.float32)
    assert lib.ww_ctc_score_rows(_lib.ptr(y), 0, 3, 4, _lib.ptr(tab), _lib.ptr(lens), 1, 0, _lib.ptr(out)) == 0 and (out == -7.0).all()


@pytest.mark.parametrize("L,mode", S64.SLIDE_CASES)
def test_sliding_thresholds_decide_nine_windows_in_ten(L, mode):
    """What tests/test_gpu_ctc_score.py's threshold comparison relies on, on the float64 reference alone."""
    s = S64.slide_scores64(L, mode)
    assert s.shape == (len(S64.TARGETS[L]), 75) and (s > 0).all() and (s <= 1).all()
    d = S64.decidable(s, S64.thresholds(s), L)
    print(f"\nL={L} {mode}: scores {s.min():.3g} .. {s.max():.3g}; undecidable per plane and threshold {(~d).sum(axis=2).tolist()}", end="")
    assert ((~d).sum(axis=2) <= 0.1 * s.shape[1]).all()
    assert s.min() > 1e-30   # far from FLT_MIN: no underflow on these models


def _trigger_numpy(speech, active, scores, n_post, thr, was):
    fired, slots, fall = [], [], []
    for s in range(len(speech)):
        if was[s] and not speech[s]:
            fall.append(s)
        was[s] = speech[s] != 0
        win = -1
        for k in range(n_post[s]):
            over = [j for j in range(len(thr)) if float(scores[s, k, j]) > thr[j]]
            if over:
                win = max(over, key=lambda j: (scores[s, k, j], -j))
                break
        if win >= 0 and not active[s]:
            active[s] = 1
            fired.append(s)
            slots.append(win)
    return fired, slots, fall


def test_score_trigger_rule_against_numpy():
    from wwhip import _lib
    lib = _lib.load()
    rng = np.random.default_rng(17)
    S, K = 37, 3
    thr = np.array([0.5, 0.25, 0.75])
    was, active = np.zeros(S, np.uint8), np.zeros(S, np.uint8)
    was_n, active_n = was.copy(), active.copy()
    seen = set()
    for tick in range(60):
        speech = (rng.random(S) < 0.8).astype(np.uint8)
        n_post = rng.integers(0, 3, S).astype(np.int32)
        scores = (np.round(rng.random((S, 2, K)) * 8) / 8).astype(np.float32)   # a grid of eighths: ties and values ON a threshold
        if tick % 7 == 0:
            active[:] = active_n[:] = 0
        fired, slot, fall, cnt = np.full(S, -1, np.int32), np.full(S, -1, np.int32), np.full(S, -1, np.int32), np.zeros(2, np.int32)
        rc = lib.ww_ctc_score_trigger_bank_step(S, K, _lib.ptr(speech), _lib.ptr(active), _lib.ptr(scores), _lib.ptr(n_post), _lib.ptr(thr), _lib.ptr(was),
                                                _lib.ptr(fired), _lib.ptr(slot), _lib.ptr(cnt[0:1]), _lib.ptr(fall), _lib.ptr(cnt[1:2]))
        assert rc == 0
        f, sl, fl = _trigger_numpy(speech, active_n, scores, n_post, thr, was_n)
        assert fired[:cnt[0]].tolist() == f and slot[:cnt[0]].tolist() == sl and fall[:cnt[1]].tolist() == fl
        np.testing.assert_array_equal(active, active_n)
        np.testing.assert_array_equal(was, was_n)
        seen.update(sl)
    assert seen == {0, 1, 2}
    cnt = np.zeros(2, np.int32)
    assert lib.ww_ctc_score_trigger_bank_step(S, 9, _lib.ptr(speech), _lib.ptr(active), _lib.ptr(scores), _lib.ptr(n_post), _lib.ptr(thr), _lib.ptr(was),
                                              _lib.ptr(fired), _lib.ptr(slot), _lib.ptr(cnt[0:1]), _lib.ptr(fall), _lib.ptr(cnt[1:2])) == _lib.WW_EINVAL
