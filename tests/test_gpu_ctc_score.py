"""The forward-algorithm score on the MI355X: ctc_score_kernel's bits against the host function of the same header
(``ww_ctc_score_rows``), its accuracy against the float64 statement (``wwhip.ctc.score``) within the derived bound, the rows it
writes, the model forms end to end, the sliding form into the FAR/FRR sweep and the event finder, and the refusals.

Shapes: the kernel alone at every segment width (U = 1 .. 9 -> P = 4, 8, 16, 32) and at segment, wave and workgroup edges of n; the
model forms on the standard geometry, L = 2, 4, 8 classes, n = 1, 3, 70 windows (``ctc64.windows``).  Bounds: tests/ctc_score64.py."""
import os

import numpy as np
import pytest

import ctc64
import ctc_score64 as S64

pytestmark = pytest.mark.gpu

SENT = -7.0
NS = (1, 7, 9, 63, 65, 257)
US = (1, 2, 3, 4, 8, 9)


@pytest.fixture(scope="module")
def models():
    from wwhip.engine import Engine
    cache = {}

    def get(L):
        if L not in cache:
            b, wins, _, _ = ctc64.reference(L)
            e = Engine(f"synthetic-ctc-{L}", bundle=b)
            cache[L] = (e, wins, e.ctc_forward(wins, max_labels=19, want=("labels", "steps")))
        return cache[L]
    yield get
    for e, _, _ in cache.values():
        e.close()


def _score_dev(e, steps, targets, mode, pad=0):
    """``ctc_score_dev`` on host posteriors ``[n, T, L]``; the output buffer starts as a sentinel and has ``pad`` floats behind it."""
    import torch
    n, T, L = steps.shape
    d_steps = torch.from_numpy(np.ascontiguousarray(steps, np.float32)).cuda() if n else torch.zeros(1, device="cuda")
    d_out = torch.full((len(targets) * n + pad,), SENT, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    e.ctc_score_dev(d_steps.data_ptr(), n, T, L, targets, mode, d_out.data_ptr())
    e.ctx.synchronize()
    out = d_out.cpu().numpy()
    return (out[:len(targets) * n].reshape(len(targets), n), out[len(targets) * n:]) if pad else out.reshape(len(targets), n)


def _tables(rng, n, T, L):
    """Posteriors with a peak per row (a Dirichlet of small concentration), a third of the sequences on a grid of sixteenths."""
    y = rng.dirichlet(np.full(L, 0.3), (n, T)).astype(np.float32)
    y[::3] = np.round(y[::3] * 16) / np.float32(16)
    return y


def _target_sets(rng, L):
    """K = 1, 3, 8; every U of ``US`` alone (one segment width per call) and mixed in one call; the repeats ``(1, 1)``, ``(1, 2, 1)``."""
    draw = lambda U: tuple(int(c) for c in rng.integers(0, L - 1, U))
    sets = [[draw(U)] for U in US] + [[draw(U) for _ in range(3)] for U in US] + [[draw(U) for _ in range(8)] for U in (1, 4, 9)]
    sets += [[draw(U) for U in (1, 9, 2, 4, 3, 8, 1, 5)], [draw(2), draw(9), draw(1)]]
    if L >= 4:
        sets += [[(1, 1)], [(1, 2, 1)], [(1, 1), (1, 2, 1), (1, 2)]]
    else:
        sets += [[(0, 0)], [(0, 0, 0)]]
    return sets


# ---- 1: the kernel's bits ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 2, 19, 64])
@pytest.mark.parametrize("L", [2, 4, 8, 64])
def test_kernel_bits_equal_the_host_function(models, T, L):
    from wwhip import ctc
    e = models(2)[0]
    rng = np.random.default_rng(1000 * T + L)
    sets = _target_sets(rng, L)
    nonzero = 0
    for n in NS:
        y = _tables(rng, n, T, L)
        for tg in sets:
            for mode in S64.MODES:
                got, want = _score_dev(e, y, tg, mode), ctc.score_rows(y, tg, mode)
                np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32), err_msg=f"n={n} T={T} L={L} {tg} {mode}")
                nonzero += int((want > 0).sum())
    assert nonzero > 0


# ---- 2: accuracy against float64 -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,L", [(19, 4), (19, 8), (64, 3), (64, 64), (2, 2)])
def test_kernel_against_the_float64_statement(models, T, L):
    from wwhip import ctc
    e = models(2)[0]
    rng = np.random.default_rng(7 * T + L)
    y = _tables(rng, 65, T, L)
    worst = 0.0
    for tg in ([tuple(int(c) for c in rng.integers(0, L - 1, U))] for U in US):
        for mode in S64.MODES:
            got, want = _score_dev(e, y, tg, mode).astype(np.float64), ctc.score(y, tg, mode)
            bound = S64.arithmetic_bound(want, T, len(tg[0]))
            worst = max(worst, float((np.abs(got - want) / bound).max()))
            assert (np.abs(got - want) <= bound).all(), (tg, mode, float((np.abs(got - want) / bound).max()))
    print(f"\nT={T} L={L}: worst error {worst:.3f} of the bound (3T + 2) 2^-24 s + (2U + 1) T 2^-126", end="")


@pytest.mark.parametrize("L", ctc64.LS)
def test_model_scores_against_the_float64_statement(models, L):
    """On the models' own posteriors: within the arithmetic bound of float64 on the same float32 posteriors, and within the model
    bound of the float64 MODEL's scores."""
    from wwhip import ctc
    e, wins, full = models(L)
    s64 = ctc64.reference(L)[2]
    for mode in S64.MODES:
        got = e.ctc_score(wins, S64.TARGETS[L], mode).astype(np.float64)
        same, model = ctc.score(full.steps, S64.TARGETS[L], mode), ctc.score(s64, S64.TARGETS[L], mode)
        for k, c in enumerate(S64.TARGETS[L]):
            r1 = np.abs(got[k] - same[k]) / S64.arithmetic_bound(same[k], 19, len(c))
            r2 = np.abs(got[k] - model[k]) / S64.model_bound(model[k], len(c))
            print(f"\nL={L} {mode} {c}: scores {got[k].min():.3g} .. {got[k].max():.3g}; {r1.max():.3f} of the arithmetic bound "
                  f"({(np.abs(got[k] - same[k]) / same[k]).max() / 2.0 ** -24:.2f} x 2^-24), {r2.max():.3f} of the model bound", end="")
            assert (r1 <= 1).all() and (r2 <= 1).all()


# ---- 3: extents ------------------------------------------------------------------------------------------------------------------------
def test_rows_written_and_nothing_else(models):
    from wwhip import ctc
    e = models(2)[0]
    rng = np.random.default_rng(5)
    tg = [(1, 2), (0,), (2, 2, 1)]
    for n in (1, 9, 65, 257):
        y = _tables(rng, n, 19, 4)
        for mode in S64.MODES:
            got, tail = _score_dev(e, y, tg, mode, pad=300)
            assert (tail == SENT).all()
            np.testing.assert_array_equal(got, ctc.score_rows(y, tg, mode))
    got, tail = _score_dev(e, np.zeros((0, 19, 4), np.float32), tg, "exact", pad=64)
    assert got.size == 0 and (tail == SENT).all()


def test_nan_posteriors_reach_their_own_scores_alone(models):
    e = models(2)[0]
    rng = np.random.default_rng(6)
    for tg in ([(1, 2), (0,), (2, 2, 1)], [(0, 1, 2, 0, 1, 2, 0, 1, 2)], [(1,)]):
        y = _tables(rng, 70, 19, 4)
        clean = {m: _score_dev(e, y, tg, m) for m in S64.MODES}
        y[33] = np.nan
        for mode in S64.MODES:
            got = _score_dev(e, y, tg, mode)
            assert np.isnan(got[:, 33]).all()
            keep = np.arange(70) != 33
            np.testing.assert_array_equal(got[:, keep], clean[mode][:, keep])


# ---- 4: the model forms ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", ctc64.LS)
@pytest.mark.parametrize("n", [1, 3, 70])
def test_engine_score_is_the_kernel_on_the_engines_own_steps(models, L, n):
    e, wins, full = models(L)
    fwd = e.ctc_forward(wins[:n], max_labels=3, want=("labels", "steps"))
    np.testing.assert_array_equal(fwd.steps, full.steps[:n])
    for mode in S64.MODES:
        want = _score_dev(e, fwd.steps, S64.TARGETS[L], mode)
        got = e.ctc_score(wins[:n], S64.TARGETS[L], mode)
        assert got.shape == (len(S64.TARGETS[L]), n) and got.dtype == np.float32
        np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
        both, dec = e.ctc_score(wins[:n], S64.TARGETS[L], mode, max_labels=3)
        np.testing.assert_array_equal(both, got)
        np.testing.assert_array_equal(dec.labels, fwd.labels)
        np.testing.assert_array_equal(dec.lengths, fwd.lengths)


@pytest.mark.parametrize("L", ctc64.LS)
def test_windows_dev_form_and_partial_clips(models, L):
    """Descriptors on the same rows give ``ctc_score``'s bits into sentinel-filled planes; the decode beside it is ``ctc_forward``'s."""
    import torch
    e, wins, full = models(L)
    n, T, F = wins.shape
    K = len(S64.TARGETS[L])
    d_mel = torch.from_numpy(wins.reshape(-1, F)).cuda()
    d_row, d_valid = torch.from_numpy(np.arange(n, dtype=np.int64) * T).cuda(), torch.full((n,), T, dtype=torch.int32, device="cuda")
    d_score = torch.full((K * n + 100,), SENT, dtype=torch.float32, device="cuda")
    d_lab, d_len = torch.full((n, 2), -9, dtype=torch.int32, device="cuda"), torch.full((n,), -9, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    e.ctc_score_windows_dev(d_mel.data_ptr(), n * T, d_row.data_ptr(), d_valid.data_ptr(), n, S64.TARGETS[L], "prefix", d_score.data_ptr(), 2,
                            d_lab.data_ptr(), d_len.data_ptr())
    e.ctx.synchronize()
    out = d_score.cpu().numpy()
    assert (out[K * n:] == SENT).all()
    np.testing.assert_array_equal(out[:K * n].reshape(K, n), e.ctc_score(wins, S64.TARGETS[L], "prefix"))
    np.testing.assert_array_equal(d_lab.cpu().numpy(), full.labels[:, :2])
    np.testing.assert_array_equal(d_len.cpu().numpy(), full.lengths)


# ---- 5: sliding --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,mode", S64.SLIDE_CASES)
def test_slide_score_planes_feed_the_sweep_and_the_event_finder(models, L, mode):
    import torch
    e = models(L)[0]
    tg = S64.TARGETS[L]
    K = len(tg)
    mel, cut = S64.slide_mel(L), S64.slide_windows(L)
    n = len(cut)
    got, dec = e.ctc_slide_score(mel, 2, tg, mode, max_labels=2)
    np.testing.assert_array_equal(got.view(np.uint32), e.ctc_score(cut, tg, mode).view(np.uint32))
    fwd = e.ctc_slide_forward(mel, 2, 2)
    np.testing.assert_array_equal(dec.labels, fwd.labels)
    np.testing.assert_array_equal(dec.lengths, fwd.lengths)
    assert e.ctc_slide_score(mel[:150], 2, tg, mode).shape == (K, 0)
    # against the float64 model, where float64 decides
    s64 = S64.slide_scores64(L, mode)
    thr = S64.thresholds(s64)
    assert (np.abs(got - s64) <= np.stack([S64.model_bound(s64[k], len(c)) for k, c in enumerate(tg)])).all()
    d = S64.decidable(s64, thr, L)
    over, over64 = got.astype(np.float64)[:, None, :] > thr[:, :, None], s64[:, None, :] > thr[:, :, None]
    np.testing.assert_array_equal(over[d], over64[d])
    # the same planes on the device, straight into the event finder and the sweep
    d_mel = torch.from_numpy(mel).cuda()
    d_row, d_valid = torch.from_numpy(np.arange(n, dtype=np.int64) * 2).cuda(), torch.full((n,), 151, dtype=torch.int32, device="cuda")
    d_score = torch.full((K, n), SENT, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    e.ctc_score_windows_dev(d_mel.data_ptr(), len(mel), d_row.data_ptr(), d_valid.data_ptr(), n, tg, mode, d_score.data_ptr())
    e.ctx.synchronize()
    np.testing.assert_array_equal(d_score.cpu().numpy(), got)
    t_ev = thr[:, 1]
    ev_dev = e.posterior_events_dev(d_score.data_ptr(), n, t_ev, window=4, planes=K)
    ev_host = e.posterior_events(got, t_ev, window=4)
    np.testing.assert_array_equal(ev_dev, ev_host)
    assert len(ev_host) > 0
    sweep = np.sort(thr[0])
    dev = e.far_frr_dev(d_score[0].data_ptr(), n, d_score[K - 1].data_ptr(), n, sweep, float(n), 1.0, window=4)
    host = e.far_frr(got[0], got[K - 1], sweep, float(n), 1.0, window=4)
    for a, b in zip(dev, host):
        np.testing.assert_array_equal(a, b)


# ---- 5b: the evaluator --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", S64.MODES)
def test_evaluate_ctc_with_thresholds_adds_scores_and_the_sweep(models, mode):
    from wwhip.evaluate import evaluate_ctc
    e, wins, _ = models(4)
    rng = np.random.default_rng(11)
    lens = rng.integers(60, 201, 40)
    long = np.concatenate([wins[i] for i in range(40, 44)])
    clips = [long[o:o + n].copy() for o, n in zip(rng.integers(0, len(long) - 200, 40), lens)]
    hot = rng.integers(0, 2, 40)
    base = evaluate_ctc(e, clips, hot)
    assert "scores" not in base and "frr" not in base
    padded = np.zeros((40, 151, 40), np.float32)
    for i, c in enumerate(clips):
        padded[i, :min(len(c), 151)] = c[:151]
    want = e.ctc_score(padded, [(1, 2)], mode)[0]
    thr = np.quantile(want.astype(np.float64), [0.2, 0.5, 0.8])
    got = evaluate_ctc(e, clips, hot, thresholds=thr, mode=mode)
    for key, v in base.items():   # what it returns without thresholds, unchanged
        np.testing.assert_array_equal(np.asarray(got[key]), np.asarray(v), err_msg=key)
    np.testing.assert_array_equal(got["scores"].view(np.uint32), want.view(np.uint32))
    truth = hot.astype(bool)
    hours = float(lens[~truth].sum()) * 0.01 / 3600.0
    frr, fa, cnt = e.far_frr(want[truth], want[~truth], thr, float(truth.sum()), hours, window=1)
    np.testing.assert_array_equal(got["frr"], frr)
    np.testing.assert_array_equal(got["fa_per_hour"], fa)
    np.testing.assert_array_equal(got["fa_count"], cnt)
    # no smoothing: the counts are the plain comparisons
    neg = want[~truth].astype(np.float64)
    rising = [(int(((neg > t) & ~np.concatenate(([False], neg[:-1] > t))).sum())) for t in thr]
    assert got["fa_count"].tolist() == rising
    np.testing.assert_allclose(got["frr"], [1.0 - (want[truth] > np.float32(t)).sum() / truth.sum() for t in thr], rtol=1e-12)


# ---- 6: refusals -------------------------------------------------------------------------------------------------------------------------
def _raw_dev(e, d_steps, n, T, L, tab, lens, K, mode, d_out):
    from wwhip import _lib
    rc = e._lib.ww_ctc_score_dev(e.ctx.handle, d_steps, n, T, L, _lib.ptr(tab), _lib.ptr(lens), K, mode, d_out)
    return rc, (e._lib.ww_last_error(e.ctx.handle) or b"").decode()


def test_refusals_come_before_anything_is_written(models, assets):
    import torch
    from wwhip import _lib, ctc
    from wwhip.engine import Engine
    e, wins, _ = models(4)
    d_steps = torch.full((4, 19, 4), 0.25, dtype=torch.float32, device="cuda")
    d_out = torch.full((64,), SENT, dtype=torch.float32, device="cuda")
    tab, lens = ctc.pack_targets([(1, 2)], 4)
    one = lambda v: np.array([v], np.int32)
    cases = [(dict(T=0), "T = 0"), (dict(T=65), "T = 65"), (dict(L=1), "L = 1"), (dict(L=65), "L = 65"), (dict(K=0), "K = 0"), (dict(K=9), "K = 9"),
             (dict(mode=2), "mode"), (dict(lens=one(0)), "U = 0"), (dict(lens=one(10)), "U = 10"), (dict(tab=np.full((1, 9), 3, np.int32)), "label"),
             (dict(tab=np.full((1, 9), -1, np.int32)), "label")]
    for kw, word in cases:
        a = dict(T=19, L=4, tab=tab, lens=lens, K=1, mode=0)
        a.update(kw)
        rc, text = _raw_dev(e, d_steps.data_ptr(), 4, a["T"], a["L"], a["tab"], a["lens"], a["K"], a["mode"], d_out.data_ptr())
        assert rc == _lib.WW_EINVAL and word in text and "ww_ctc_score_dev" in text, (kw, rc, text)
    e.ctx.synchronize()
    assert (d_out.cpu().numpy() == SENT).all()
    # the model forms: the same rules (L is the model's), and the model itself
    score = np.full((8, 3), SENT, np.float32)
    for kw, word in cases[4:]:
        a = dict(tab=tab, lens=lens, K=1, mode=0)
        a.update(kw)
        rc = e._lib.ww_ctc_score(e.ctx.handle, e.handle, _lib.ptr(wins[:3]), 3, _lib.ptr(a["tab"]), _lib.ptr(a["lens"]), a["K"], a["mode"], _lib.ptr(score),
                                 0, None, None)
        assert rc == _lib.WW_EINVAL and word in (e._lib.ww_last_error(e.ctx.handle) or b"").decode(), kw
    lab = np.full((3, 2), -9, np.int32)
    assert e._lib.ww_ctc_score(e.ctx.handle, e.handle, _lib.ptr(wins[:3]), 3, _lib.ptr(tab), _lib.ptr(lens), 1, 0, _lib.ptr(score), 2, _lib.ptr(lab),
                               None) == _lib.WW_EINVAL
    assert (score == SENT).all() and (lab == -9).all()
    with pytest.raises(ValueError, match="label"):
        e.ctc_score(wins[:3], [(3,)])
    with pytest.raises(ValueError):
        e.ctc_slide_score(S64.slide_mel(4), 2, [(1, 2)], "loss")
    # split-bf16 mode and a model that is no CTC model
    e.set_precision("bf16x3")
    try:
        with pytest.raises(ValueError):
            e.ctc_score(wins[:3], [(1, 2)])
        with pytest.raises(ValueError):
            e.ctc_slide_score(S64.slide_mel(4), 2, [(1, 2)])
    finally:
        e.set_precision("fp32")
    np.testing.assert_array_equal(e.ctc_score(wins[:3], [(1, 2)]), e.ctc_score(wins[:70], [(1, 2)])[:, :3])
    plain = Engine(os.path.join(assets, "CRNN_softmax"))
    try:
        with pytest.raises(ValueError, match="not a CTC"):
            plain.ctc_score(np.zeros((1, plain.window, plain.n_mel), np.float32), [(0,)])
        # the kernel alone takes any posteriors, whatever the engine's model
        np.testing.assert_array_equal(_score_dev(plain, np.full((3, 5, 4), 0.25, np.float32), [(1, 2)], "exact"),
                                      ctc.score_rows(np.full((3, 5, 4), 0.25, np.float32), [(1, 2)], "exact"))
    finally:
        plain.close()
