"""The evaluator tail on the device - ``smooth_kernel``, ``sweep_kernel``, ``pick_kernel`` and ``viterbi2_kernel`` (csrc/posterior.hip)
behind ``ww_far_frr``, ``ww_far_frr_dev``, ``ww_posterior_pick_dev`` and ``ww_superframe_smooth`` - against tests/sweep64.py, the
float64 statement of what the reference computes.

Smoothed values are held to ``sweep64.smooth_bound`` (np.convolve and the library's ascending chain sum in different orders); counts
are ``array_equal`` to the rule applied to the values the call returned and, where tests/test_sweep64.py pins the margin on the
reference alone, to the rule applied to the float64 values; the dyadic cases have no rounding and no tolerance anywhere."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sweep64 as S  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng(assets):
    from wwhip.engine import Engine
    e = Engine(os.path.join(assets, "CRNN"))
    yield e
    e.close()


def _sweep(eng, pos, neg, thr, win, num=1.0, hours=1.0):
    """``ww_far_frr`` over host arrays: ``(accepted, fa_count, smoothed)`` - ``accepted`` is the integer behind the FRR it returns for
    ``num`` wake words, ``frr = (num - accepted) / num``."""
    pos = np.asarray(pos, np.float32)
    frr, fa, cnt, sm = eng.far_frr(pos, neg, thr, num, hours, window=win, want_smoothed=True)
    np.testing.assert_array_equal(fa, cnt / hours)
    return _accepted(frr, num), cnt, sm


def _accepted(frr, num):
    acc = num - frr * num
    assert np.abs(acc - np.rint(acc)).max() < 1e-6, acc   # (two roundings of at most num * 2^-52)
    return np.rint(acc).astype(np.int64)


def _check_smoothed(name, sm, neg, win):
    want = S.smooth(neg, win)
    assert sm.shape == want.shape, name
    bound = S.smooth_bound(neg, win)
    err = np.abs(sm - want)
    assert np.all(err <= bound), (name, int(np.argmax(err - bound)), float(err.max()), float(bound.max()))
    return want


NO_POS = np.zeros(0, np.float32)


# ---------------------------------------------------------------- 1 + 3. smoothing and counts, every window
@pytest.mark.parametrize("win", S.WINDOWS)
def test_smoothing_and_counts_against_float64(eng, win):
    """Windows 0, 1, 2, 3, 29, 30, 31, 32 (odd and even centring) at ``n`` = ``win``, ``win + 1``, 255, 256, 257 and 5000 rows of seeded
    noise: every smoothed value within ``smooth_bound`` of np.convolve's, the counts at the default thresholds equal to the rule on the
    returned values and (margin pinned in tests/test_sweep64.py) on the float64 values.  Streams of all ones and all zeros: the same
    bound, and the one rise / no rise that the statement gives."""
    thr = S.DEFAULT_THR
    for name, neg in S.smoothing_cases(win):
        _, cnt, sm = _sweep(eng, NO_POS, neg, thr, win)
        sm64 = _check_smoothed(name, sm, neg, win)
        np.testing.assert_array_equal(cnt, S.counts(sm, thr), err_msg=name)
        np.testing.assert_array_equal(cnt, S.counts(sm64, thr), err_msg=name)
    for name, neg, count in S.constant_cases(win):
        _, cnt, sm = _sweep(eng, NO_POS, neg, thr, win)
        _check_smoothed(name, sm, neg, win)
        np.testing.assert_array_equal(cnt, S.counts(sm, thr), err_msg=name)
        np.testing.assert_array_equal(cnt, np.full(thr.size, count), err_msg=name)


@pytest.mark.parametrize("win", [0, -1])
def test_no_window_widens_the_input_bit_for_bit(eng, win):
    for n in (1, 257, 5000):
        neg = S.noise(1500 + n, n)
        _, cnt, sm = _sweep(eng, NO_POS, neg, S.DEFAULT_THR, win)
        assert sm.tobytes() == neg.astype(np.float64).tobytes()
        np.testing.assert_array_equal(cnt, S.counts(neg.astype(np.float64), S.DEFAULT_THR))


def test_stream_shorter_than_its_window_is_refused(eng):
    with pytest.raises(ValueError):
        eng.far_frr(NO_POS, S.noise(1, 29), np.array([0.5]), 1.0, 1.0, window=30)


# ---------------------------------------------------------------- 2. dyadic: no tolerance anywhere
@pytest.mark.parametrize("win", [1, 2, 4, 32])
def test_dyadic_streams_equal_float64_bit_for_bit(eng, win):
    """Multiples of 2^-10 and a power-of-two window: nothing is rounded (tests/test_sweep64.py), so the smoothed values are float64's
    bits and the counts are equal at thresholds that ARE smoothed values, and at their float64 neighbours: '>' against '>='."""
    neg, thr = S.dyadic_case(win)
    _, cnt, sm = _sweep(eng, NO_POS, neg, thr, win)
    sm64 = S.smooth(neg, win)
    assert sm.tobytes() == sm64.tobytes()
    np.testing.assert_array_equal(cnt, S.counts(sm64, thr))


# ---------------------------------------------------------------- 4. past one trip of the grid-stride loops
def _dev_sweep(eng, d_pos, n_pos, d_neg, n_neg, thr, win, d_sm, num=1.0, hours=1.0):
    from wwhip import _lib
    thr = np.ascontiguousarray(thr, np.float64)
    frr, fa, cnt = np.full(thr.size, -7.0), np.full(thr.size, -7.0), np.full(thr.size, -7, np.int64)
    vp = lambda t: C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None
    rc = _lib.load().ww_far_frr_dev(eng.ctx.handle, vp(d_pos), int(n_pos), vp(d_neg), int(n_neg), int(win), _lib.ptr(thr), thr.size,
                                    float(num), float(hours), _lib.ptr(frr), _lib.ptr(fa), _lib.ptr(cnt), vp(d_sm))
    _lib.raise_for(rc, eng.ctx.handle)
    return frr, fa, cnt


def test_negatives_past_one_trip_of_the_grid(eng):
    """2048 * 256 + 1 and 4096 * 256 + 777 rows: ``sweep_kernel`` (2,048 workgroups) takes a second and a third trip, ``smooth_kernel``
    (4,096) a second one.  A run of 0.97 lies across each trip's first row (its ``prev`` is the last row of the trip before), and
    with window 1 a rise sits exactly on it.  Smoothed values within the bound, counts equal to the rule on the returned and on the
    float64 values; ``ww_far_frr_dev`` over device pointers, with and without a ``d_smoothed`` buffer, gives ``ww_far_frr``'s bits."""
    import torch
    for name, neg, win, thr in S.big_cases():
        frr, fa, cnt, sm = eng.far_frr(NO_POS, neg, thr, 1.0, 2.4, window=win, want_smoothed=True)
        sm64 = _check_smoothed(name, sm, neg, win)
        np.testing.assert_array_equal(cnt, S.counts(sm, thr), err_msg=name)
        np.testing.assert_array_equal(cnt, S.counts(sm64, thr), err_msg=name)
        np.testing.assert_array_equal(fa, cnt / 2.4, err_msg=name)
        d_neg = torch.from_numpy(neg).cuda()
        d_sm = torch.full((neg.size,), -3.0, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        with_sm = _dev_sweep(eng, None, 0, d_neg, neg.size, thr, win, d_sm, 1.0, 2.4)
        without = _dev_sweep(eng, None, 0, d_neg, neg.size, thr, win, None, 1.0, 2.4)
        for got in (with_sm, without):
            for g, w in zip(got, (frr, fa, cnt)):
                np.testing.assert_array_equal(g, w, err_msg=name)
        assert d_sm.cpu().numpy().tobytes() == sm.tobytes(), name
        del d_neg, d_sm


def test_positives_past_one_trip_of_the_grid(eng):
    """2048 * 256 + 5 positives against 1,000 negatives: the positives' loop of ``sweep_kernel`` takes a second trip."""
    import torch
    n_pos = S.TRIP_SWEEP + 5
    pos = np.random.default_rng(3101).uniform(0.2, 1.0, n_pos).astype(np.float32)
    pos[-5:] = [0.2, 0.999, 0.6, 0.2, 0.999]     # the second trip's rows: known answers at the ends of the threshold list
    neg = S.noise(3102, 1000)
    thr = S.BIG_THR[30]
    acc, cnt, sm = _sweep(eng, pos, neg, thr, 30, num=float(n_pos))
    want = S.accepts(pos, thr)
    assert want[0] > want[-1] > 0
    np.testing.assert_array_equal(acc, want)
    np.testing.assert_array_equal(cnt, S.counts(sm, thr))
    d_pos, d_neg = torch.from_numpy(pos).cuda(), torch.from_numpy(neg).cuda()
    torch.cuda.synchronize()
    frr_d, _, cnt_d = _dev_sweep(eng, d_pos, n_pos, d_neg, neg.size, thr, 30, None, float(n_pos), 1.0)
    np.testing.assert_array_equal(_accepted(frr_d, float(n_pos)), want)
    np.testing.assert_array_equal(cnt_d, cnt)


# ---------------------------------------------------------------- 5. thresholds
@pytest.mark.parametrize("n_thr", S.THR_COUNTS)
def test_threshold_counts_around_one_pass_of_the_fill(eng, n_thr):
    """1, 255, 256, 257 and 1,024 thresholds (the LDS fill takes 256 per pass; 1,024 is the limit) on 20,000 rows: every count."""
    neg, pos = S.threshold_stream()
    thr = S.threshold_list(n_thr)
    acc, cnt, sm = _sweep(eng, pos, neg, thr, 30, num=float(pos.size))
    sm64 = _check_smoothed(f"{n_thr} thresholds", sm, neg, 30)
    np.testing.assert_array_equal(cnt, S.counts(sm, thr))
    np.testing.assert_array_equal(cnt, S.counts(sm64, thr))
    np.testing.assert_array_equal(acc, S.accepts(pos, thr))


def test_one_threshold_too_many_is_refused_and_writes_nothing(eng):
    from wwhip import _lib
    neg, pos = S.threshold_stream()
    thr = S.threshold_list(1025)
    frr, fa, cnt, sm = np.full(1025, -7.0), np.full(1025, -7.0), np.full(1025, -7, np.int64), np.full(neg.size, -7.0)
    rc = _lib.load().ww_far_frr(eng.ctx.handle, _lib.ptr(pos), pos.size, _lib.ptr(neg), neg.size, 30, _lib.ptr(thr), 1025, 300.0, 1.0,
                                _lib.ptr(frr), _lib.ptr(fa), _lib.ptr(cnt), _lib.ptr(sm))
    assert rc == _lib.WW_EINVAL
    assert np.all(frr == -7.0) and np.all(fa == -7.0) and np.all(cnt == -7) and np.all(sm == -7.0)
    with pytest.raises(ValueError, match="1024"):
        eng.far_frr(pos, neg, thr, 300.0, 1.0)
    # and the context still works
    acc, cnt, _ = _sweep(eng, pos, neg, thr[:1024], 30, num=float(pos.size))
    np.testing.assert_array_equal(acc, S.accepts(pos, thr[:1024]))


def test_thresholds_in_any_order_with_repeats_and_out_of_range(eng):
    """A shuffled list with repeats gives, entry by entry, the counts of the sorted list; threshold -1 counts one rise on a stream
    that is not empty (and accepts every positive), threshold 2 none."""
    neg, pos = S.threshold_stream()
    base = S.threshold_list(40)
    acc0, cnt0, _ = _sweep(eng, pos, neg, base, 30, num=float(pos.size))
    idx = np.random.default_rng(4003).integers(0, 40, 100)
    assert np.unique(idx).size < idx.size and np.any(np.diff(idx) < 0)
    acc, cnt, sm = _sweep(eng, pos, neg, base[idx], 30, num=float(pos.size))
    np.testing.assert_array_equal(cnt, cnt0[idx])
    np.testing.assert_array_equal(acc, acc0[idx])
    np.testing.assert_array_equal(cnt, S.counts(sm, base[idx]))
    acc, cnt, _ = _sweep(eng, pos, neg, np.array([2.0, -1.0, 0.5, -1.0]), 30, num=float(pos.size))
    np.testing.assert_array_equal(cnt[[0, 1, 3]], [0, 1, 1])
    np.testing.assert_array_equal(acc[[0, 1, 3]], [0, pos.size, pos.size])
    _, cnt, _ = _sweep(eng, NO_POS, np.zeros(1, np.float32), np.array([-1.0, 2.0]), 1)
    np.testing.assert_array_equal(cnt, [1, 0])


# ---------------------------------------------------------------- 6. the float32 rule for positives
def test_positives_compare_in_float32(eng):
    """The positives and thresholds of tests/test_sweep64.py::test_float32_rule_for_positives: of ``float32(t)`` and its two float32
    neighbours exactly one is above ``t`` - also where ``float32(t) > t``, where a float64 comparison would accept two."""
    up, down = S.float32_rule_thresholds()
    for t in np.concatenate([up, down]):
        acc, _, _ = _sweep(eng, S.float32_rule_positives(t), np.zeros(1, np.float32), np.array([t]), 1, num=3.0)
        assert acc[0] == 1, (t, acc)
    ts = np.concatenate([up, down])
    pos = np.concatenate([S.float32_rule_positives(t) for t in ts])
    acc, _, _ = _sweep(eng, pos, np.zeros(1, np.float32), ts, 1, num=float(pos.size))
    np.testing.assert_array_equal(acc, S.accepts(pos, ts))


# ---------------------------------------------------------------- 7. NaN
@pytest.mark.parametrize("at", [0, 2500, 4999])
def test_a_nan_row_is_above_nothing(eng, at):
    """One NaN among 5,000 negatives (window 30): the smoothed rows whose window holds it are NaN - float64's rows -, the others are
    within the bound, and the counts are the rule on the returned values: a NaN is not above, a run may begin on the row after."""
    neg = S.noise(5100 + at, 5000)
    neg[max(at - 40, 0):at + 40] = np.maximum(neg[max(at - 40, 0):at + 40], np.float32(0.8))   # the NaN rows cut a run in two
    neg[at] = np.nan
    thr = np.array([0.3, 0.45, 0.5, 0.6, 0.75])
    _, cnt, sm = _sweep(eng, NO_POS, neg, thr, 30)
    sm64 = S.smooth(neg, 30)
    rows = np.arange(5000)
    np.testing.assert_array_equal(np.isnan(sm64), (rows >= at - 14) & (rows <= at + 15))
    np.testing.assert_array_equal(np.isnan(sm), np.isnan(sm64))
    ok = ~np.isnan(sm64)
    assert np.all(np.abs(sm - sm64)[ok] <= S.smooth_bound(neg, 30)[ok])
    np.testing.assert_array_equal(cnt, S.counts(sm, thr))
    if at == 2500:   # (the input does what it is for: the NaN rows lie inside a run, which the statement counts as two)
        clean = np.where(np.isnan(neg), np.float32(0.8), neg)
        assert S.counts(sm64, thr)[-1] == S.counts(S.smooth(clean, 30), thr)[-1] + 1


def test_a_nan_positive_is_not_accepted(eng):
    pos = np.array([np.nan, 0.9, 0.2, np.nan], np.float32)
    acc, _, _ = _sweep(eng, pos, np.zeros(1, np.float32), np.array([-1.0, 0.5, 2.0]), 1, num=4.0)
    np.testing.assert_array_equal(acc, [2, 1, 0])


# ---------------------------------------------------------------- 8. pick
def _pick(eng, rows, n_out, pidx, offs=None):
    """``ww_posterior_pick_dev`` on ``rows [n][n_out]``; the output buffer is filled with 7 first and has one spare element."""
    import torch
    from wwhip import _lib
    rows = np.ascontiguousarray(rows, np.float32).reshape(-1, n_out)
    n = rows.shape[0]
    d_rows = torch.from_numpy(rows).cuda()
    n_res = n if offs is None else len(offs) - 1
    d_out = torch.full((n_res + 1,), 7.0, dtype=torch.float32, device="cuda")
    d_offs = None if offs is None else torch.from_numpy(np.ascontiguousarray(offs, np.int64)).cuda()
    torch.cuda.synchronize()
    rc = _lib.load().ww_posterior_pick_dev(eng.ctx.handle, C.c_void_p(d_rows.data_ptr()), n, n_out, pidx,
                                           None if d_offs is None else C.c_void_p(d_offs.data_ptr()), 0 if offs is None else n_res,
                                           C.c_void_p(d_out.data_ptr()))
    _lib.raise_for(rc, eng.ctx.handle)
    eng.ctx.synchronize()
    out = d_out.cpu().numpy()
    assert out[-1] == 7.0          # nothing written behind the last result
    return out[:-1]


def _same_with_nan(got, want, what):
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape, what
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=str(what))
    np.testing.assert_array_equal(got[~np.isnan(want)], want[~np.isnan(want)], err_msg=str(what))


def _pick_rows(seed, n, n_out):
    """Rows in [-1, 1] with -0.0 and -inf among them."""
    rng = np.random.default_rng(seed)
    rows = rng.uniform(-1, 1, (n, n_out)).astype(np.float32)
    flat = rows.reshape(-1)
    k = max(1, flat.size // 50)
    flat[rng.choice(flat.size, k, replace=False)] = -np.inf
    flat[rng.choice(flat.size, k, replace=False)] = -0.0
    return rows


@pytest.mark.parametrize("n_out", [1, 2, 3])
def test_pick_every_column_and_run_length(eng, n_out):
    """Every ``pidx`` of 1, 2 and 3 columns.  Without offsets at 1, 255, 256 and 257 rows; with offsets, runs of 1, 63, 64, 65, 128, 129
    and 1,000 windows in one table (the 64-lane loop and the shuffle reduction), and tables of 1, 3, 4 and 5 runs (four waves per
    workgroup).  ``array_equal`` to ``sweep64.pick``."""
    for pidx in range(n_out):
        for n in (1, 255, 256, 257):
            rows = _pick_rows(6000 + n, n, n_out)
            _same_with_nan(_pick(eng, rows, n_out, pidx), S.pick(rows, n_out, pidx), (n_out, pidx, n))
        lens = np.array([1, 63, 64, 65, 128, 129, 1000])
        offs = np.concatenate(([0], np.cumsum(lens)))
        rows = _pick_rows(6100 + pidx, offs[-1] + 11, n_out)       # (11 rows behind the last run belong to none)
        rows[offs[-2] + 999, pidx] = 0.9999                         # each long run's maximum in its last round of 64
        rows[offs[5] + 128, pidx] = 0.9998
        rows[offs[3] + 64, pidx] = 0.9997
        _same_with_nan(_pick(eng, rows, n_out, pidx, offs), S.pick(rows, n_out, pidx, offs), (n_out, pidx, "lengths"))
        for n_seg in (1, 3, 4, 5):
            lens = np.random.default_rng(6200 + n_seg).integers(1, 90, n_seg)
            offs = np.concatenate(([0], np.cumsum(lens)))
            rows = _pick_rows(6300 + n_seg, offs[-1], n_out)
            _same_with_nan(_pick(eng, rows, n_out, pidx, offs), S.pick(rows, n_out, pidx, offs), (n_out, pidx, n_seg))


def test_pick_clamps_offsets_and_an_empty_run_is_minus_inf(eng):
    rows = _pick_rows(6400, 300, 2)
    offs = np.array([-5, 70, 70, 200, 309], np.int64)       # below 0, an empty run, past n
    got = _pick(eng, rows, 2, 1, offs)
    _same_with_nan(got, S.pick(rows, 2, 1, offs), "clamped")
    assert got[1] == -np.inf
    col = rows[:, 1]
    np.testing.assert_array_equal(got[[0, 2, 3]], [col[:70].max(), col[70:200].max(), col[200:].max()])


@pytest.mark.parametrize("at", [0, 63, 64, 199])
def test_pick_a_run_holding_a_nan_is_nan(eng, at):
    """The reference's ``np.max`` (utils/evaluate_models.py:98-99) returns NaN for a clip with a NaN posterior, and the clip is then a
    reject at every threshold; so does the library (a plain ``fmaxf`` would return the greatest of the other windows)."""
    rows = _pick_rows(6500 + at, 500, 2)
    offs = np.array([0, 100, 300, 500], np.int64)
    rows[100 + at, 1] = np.nan
    for pidx in (0, 1):
        got = _pick(eng, rows, 2, pidx, offs)
        _same_with_nan(got, S.pick(rows, 2, pidx, offs), (at, pidx))
    assert np.isnan(got[1]) and not np.isnan(got[0]) and not np.isnan(got[2])
    _same_with_nan(_pick(eng, rows, 2, 1), S.pick(rows, 2, 1), (at, "rows"))
    # the clip is a reject: a NaN positive is above nothing
    acc, _, _ = _sweep(eng, got, np.zeros(1, np.float32), np.array([-1.0]), 1, num=3.0)
    assert acc[0] == 2


# ---------------------------------------------------------------- 9. Viterbi
def _viterbi(costs, stay_bonus):
    """``ww_superframe_smooth`` on ready-made costs ``[n][T][2]``: ``(path, wake)``."""
    from wwhip import _lib
    c = np.ascontiguousarray(costs, np.float32)
    n, T, _ = c.shape
    ctx = _lib.default_context()
    path, wake = np.full((n, T), 9, np.uint8), np.full(n, 9, np.uint8)
    _lib.raise_for(_lib.load().ww_superframe_smooth(ctx.handle, _lib.ptr(c), n, T, C.c_float(stay_bonus), 1, _lib.ptr(path), _lib.ptr(wake)),
                   ctx.handle)
    return path, wake


def _check_paths(what, costs, path, wake, bonus):
    assert path.max() <= 1, what
    np.testing.assert_array_equal(wake.astype(bool), path.any(axis=1), err_msg=str(what))
    got, best = S.viterbi_cost(costs, path, bonus), S.viterbi_best(costs, bonus)
    assert got.dtype == best.dtype == np.float32
    np.testing.assert_array_equal(got, best, err_msg=str(what))


@pytest.mark.parametrize("T", [1, 2, 7, 8])
def test_viterbi_returns_a_shortest_path(T):
    """Superframes of 1, 2, 7 and 8 steps, 1, 256 and 257 of them, stay bonus 0, 0.5, 1 and 2.5.  Posteriors through
    ``wwhip.wfst.smooth_batch`` (costs ``-np.log(p)`` made on the host) and ready-made costs with +inf entries through
    ``ww_superframe_smooth``: the returned path's float32 cost is the smallest over all 2^T paths, and ``wake`` says whether it
    visits state 1.  All-0.5 posteriors: every path ties, and ties keep state 0."""
    from wwhip import wfst
    for n in (1, 256, 257):
        rng = np.random.default_rng(7000 + 10 * T + n)
        p = rng.uniform(0.002, 0.998, (n, T, 1)).astype(np.float32)
        if n > 1:
            p[::5] = rng.uniform(0.4, 0.6, (len(p[::5]), T, 1))      # near-ties: the bonus decides
        pp = np.concatenate([np.float32(1) - p, p], axis=2)
        ready = rng.uniform(-1.0, 6.0, (n, T, 2)).astype(np.float32)
        ready[rng.uniform(size=ready.shape) < 0.1] = np.inf
        if n > 2:
            ready[1] = np.inf                                        # no finite path at all
            ready[2, :, 1] = np.inf                                  # state 1 closed
        for bonus in (0.0, 0.5, 1.0, 2.5):
            path, wake = wfst.smooth_batch(pp, stay_bonus=bonus)
            _check_paths(("posteriors", T, n, bonus), -np.log(pp), path, wake, bonus)
            path, wake = _viterbi(ready, bonus)
            _check_paths(("costs", T, n, bonus), ready, path, wake, bonus)
            if n > 2 and T > 1:
                assert not path[2].any()
            half = np.full((n, T, 2), 0.5, np.float32)
            for device_log in (False, True):
                path, wake = wfst.smooth_batch(half, stay_bonus=bonus, device_log=device_log)
                assert not path.any() and not wake.any(), (T, n, bonus, device_log)
