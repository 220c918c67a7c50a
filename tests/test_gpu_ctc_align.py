"""The Viterbi alignment on the MI355X: ctc_align_kernel's values (as bits) and spans against the host function of the same header
(``ww_ctc_align_rows``), the bytes it writes, the model forms end to end, and the refusals.

Shapes: the smallest that reach every branch of the kernel.  n = 67 sequences (no multiple of the 64, 32, 16 or 8 pairs of a
workgroup, so the last workgroup has dead segments; with K = 3 targets a sequence's segments also straddle waves); the U sets
{1}, {1, 2, 3}, {4, 5, 7}, {8, 9, 2} select the four segment widths P = 4, 8, 16, 32; T = 1, 2 (no loop / one step), 8, 9 (the
prefetch group of 8 steps ends / a second group of one step), 16, 17 (the first back-pointer word is full / the second begins), 19
(the models' T), 33 (the third word) and 64 (the limit); L = 2 (labels are all equal: every target needs its blanks), 4 and 64.
The model forms run on the standard geometry: 70 windows stay inside one chunk of ``ctc_score_chunks`` (a chunk is 16,384
windows), so the chunk loop's second pass is not reached here."""
import ctypes
import os

import numpy as np
import pytest

import ctc64
import ctc_align64 as A64

pytestmark = pytest.mark.gpu

SENT, SENT_B = -7.0, 0x55
N = 67
TS = (1, 2, 8, 9, 16, 17, 19, 33, 64)
U_SETS = ((1, 1, 1), (1, 2, 3), (4, 5, 7), (8, 9, 2))


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


def _align_dev(e, steps, targets, mode, pad=0):
    """``ctc_align_dev`` on host posteriors ``[n, T, L]`` -> ``(value [K, n], span [K, n, 9, 2] int8, value tail, span tail)``; the
    outputs start as sentinels and have ``pad`` elements behind them."""
    import torch
    n, T, L = steps.shape
    K = len(targets)
    d_steps = torch.from_numpy(np.ascontiguousarray(steps, np.float32)).cuda() if n else torch.zeros(1, device="cuda")
    d_value = torch.full((K * n + pad,), SENT, dtype=torch.float32, device="cuda")
    d_span = torch.full((K * n * 18 + pad,), SENT_B, dtype=torch.int8, device="cuda")
    torch.cuda.synchronize()
    e.ctc_align_dev(d_steps.data_ptr(), n, T, L, targets, mode, d_value.data_ptr(), d_span.data_ptr())
    e.ctx.synchronize()
    v, s = d_value.cpu().numpy(), d_span.cpu().numpy()
    return v[:K * n].reshape(K, n), s[:K * n * 18].reshape(K, n, 9, 2), v[K * n:], s[K * n * 18:]


def _rows_host(steps, targets, mode):
    """``ww_ctc_align_rows`` with all 9 span rows: ``(value [K, n] float32, span [K, n, 9, 2] int8)``."""
    from wwhip import _lib, ctc
    y = np.ascontiguousarray(steps, np.float32)
    n, T, L = y.shape
    tab, lens = ctc.pack_targets(targets, L)
    value, span = np.full((len(lens), n), SENT, np.float32), np.full((len(lens), n, 9, 2), SENT_B, np.int8)
    assert _lib.load().ww_ctc_align_rows(_lib.ptr(y), n, T, L, _lib.ptr(tab), _lib.ptr(lens), len(lens), ctc.score_mode(mode), _lib.ptr(value),
                                         _lib.ptr(span)) == 0
    return value, span


def _targets(rng, L, us, equal_neighbours):
    out = []
    for U in us:
        c = rng.integers(0, L - 1, U)
        if L > 2:
            for u in range(1, U):   # no equal neighbours ...
                while c[u] == c[u - 1]:
                    c[u] = rng.integers(0, L - 1)
            if equal_neighbours and U >= 2:   # ... or one pair, and from U = 4 a second
                c[1] = c[0]
                if U >= 4:
                    c[U - 1] = c[U - 2]
        out.append(tuple(int(v) for v in c))
    return out


def _tables(rng, n, T, L, targets):
    """Sequence i follows a path that reads target i % K (0.7 on the path's class, so that a product of 64 posteriors does not
    underflow; the rest shared by a seeded draw), dwelling a random number of steps per state - cut off where T is too short.  A
    third of the sequences lie on a grid of sixteenths (exact zeros and exact ties); every seventh has one label of its target
    zeroed on every row (no path at all for that target)."""
    y = 0.3 * rng.dirichlet(np.full(L, 0.3), (n, T))
    for i in range(n):
        c = targets[i % len(targets)]
        states = [L - 1 if s % 2 == 0 else c[s // 2] for s in range(2 * len(c) + 1)]
        cuts = np.sort(rng.integers(0, T + 1, len(states) - 1))
        y[i, np.arange(T), [states[int(np.searchsorted(cuts, t, side="right"))] for t in range(T)]] += 0.7
    y = y.astype(np.float32)
    y[::3] = np.round(y[::3] * 16) / np.float32(16)
    for i in range(5, n, 7):
        y[i, :, targets[i % len(targets)][0]] = 0.0
    return y


# ---- 1: the kernel's bits ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("L", [2, 4, 64])
def test_kernel_values_and_spans_equal_the_host_function(models, T, L):
    e = models(2)[0]
    rng = np.random.default_rng(1000 * T + L)
    paths = none = 0
    for us in U_SETS:
        for eq in (False, True):
            tg = _targets(rng, L, us, eq)
            y = _tables(rng, N, T, L, tg)
            for mode in A64.MODES:
                gv, gs, _, _ = _align_dev(e, y, tg, mode)
                wv, ws = _rows_host(y, tg, mode)
                np.testing.assert_array_equal(gv.view(np.uint32), wv.view(np.uint32), err_msg=f"T={T} L={L} {tg} {mode}")
                np.testing.assert_array_equal(gs, ws, err_msg=f"T={T} L={L} {tg} {mode}")
                paths += int((wv != 0).sum())
                none += int((wv == 0).sum())
    print(f"\nT={T} L={L}: {paths} pairs with a path, {none} without", end="")
    assert paths > 0 and none > 0   # (U = 1 at T = 1 has a path; a zeroed label or a T too short has none)


# ---- 2: extents, and a second call ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("us", U_SETS)
def test_bytes_written_and_nothing_else(models, us):
    """Exactly K n values and K n 18 span bytes: the sentinels behind them survive, every byte in front of them is the host's (whose
    spans hold steps 0 .. 63 or -1, never the sentinel), and a second identical call gives identical bits."""
    e = models(2)[0]
    rng = np.random.default_rng(sum(us))
    tg = _targets(rng, 4, us, True)
    for n in (1, N):
        y = _tables(rng, n, 19, 4, tg)
        for mode in A64.MODES:
            gv, gs, tv, ts = _align_dev(e, y, tg, mode, pad=300)
            assert (tv == SENT).all() and (ts == SENT_B).all()
            wv, ws = _rows_host(y, tg, mode)
            np.testing.assert_array_equal(gv.view(np.uint32), wv.view(np.uint32))
            np.testing.assert_array_equal(gs, ws)
            assert (gs != SENT_B).all()
            again = _align_dev(e, y, tg, mode, pad=300)
            np.testing.assert_array_equal(again[0].view(np.uint32), gv.view(np.uint32))
            np.testing.assert_array_equal(again[1], gs)
    gv, gs, tv, ts = _align_dev(e, np.zeros((0, 19, 4), np.float32), tg, "exact", pad=64)
    assert gv.size == 0 and gs.size == 0 and (tv == SENT).all() and (ts == SENT_B).all()


# ---- 3: the model forms ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", ctc64.LS)
@pytest.mark.parametrize("n", [1, 3, 70])
def test_engine_align_is_the_kernel_on_the_engines_own_steps(models, L, n):
    e, wins, full = models(L)
    tg = A64.TARGETS[L]
    umax = max(len(c) for c in tg)
    fwd = e.ctc_forward(wins[:n], max_labels=3, want=("labels", "steps"))
    np.testing.assert_array_equal(fwd.steps, full.steps[:n])
    for mode in A64.MODES:
        wv, ws, _, _ = _align_dev(e, fwd.steps, tg, mode)
        got = e.ctc_align(wins[:n], tg, mode)
        assert got.value.shape == (len(tg), n) and got.value.dtype == np.float32
        assert got.span.shape == (len(tg), n, umax, 2) and got.span.dtype == np.int32
        np.testing.assert_array_equal(got.value.view(np.uint32), wv.view(np.uint32))
        np.testing.assert_array_equal(got.span, ws[:, :, :umax])
        assert (ws[:, :, umax:] == -1).all() and (got.value > 0).all()
        both, dec = e.ctc_align(wins[:n], tg, mode, max_labels=3)
        np.testing.assert_array_equal(both.value, got.value)
        np.testing.assert_array_equal(both.span, got.span)
        np.testing.assert_array_equal(dec.labels, fwd.labels)
        np.testing.assert_array_equal(dec.lengths, fwd.lengths)
        # and the path it names is an optimal one of the float64 statement on the same posteriors, up to rounding
        from wwhip import ctc
        a64 = ctc.align(fwd.steps, tg, mode)
        assert (np.abs(got.value - a64.value) <= A64.value_bound(a64.value, 19)).all()
        for k, c in enumerate(tg):
            for i in range(n):
                path = A64.path_of_span(got.span[k, i, :len(c)], c, 19, L, mode)
                assert A64.path_probability(fwd.steps[i], path) >= A64.path_floor(a64.value[k, i], 19)


@pytest.mark.parametrize("L", ctc64.LS)
def test_slide_align_equals_the_explicit_windows(models, L):
    """170 rows at hop 2: 10 windows."""
    e, wins, _ = models(L)
    tg = A64.TARGETS[L]
    mel = np.concatenate([wins[7], wins[8]])[:170]
    cut = np.stack([mel[i:i + 151] for i in range(0, 170 - 151 + 1, 2)])
    assert len(cut) == 10
    for mode in A64.MODES:
        got, dec = e.ctc_slide_align(mel, 2, tg, mode, max_labels=2)
        want = e.ctc_align(cut, tg, mode)
        np.testing.assert_array_equal(got.value.view(np.uint32), want.value.view(np.uint32))
        np.testing.assert_array_equal(got.span, want.span)
        fwd = e.ctc_slide_forward(mel, 2, 2)
        np.testing.assert_array_equal(dec.labels, fwd.labels)
        np.testing.assert_array_equal(dec.lengths, fwd.lengths)
        al = e.ctc_slide_align(mel[:150], 2, tg, mode)
        assert al.value.shape == (len(tg), 0) and al.span.shape[:2] == (len(tg), 0)


@pytest.mark.parametrize("L", ctc64.LS)
def test_windows_dev_form_writes_its_planes_and_nothing_else(models, L):
    import torch
    e, wins, full = models(L)
    n, T, F = wins.shape
    tg = A64.TARGETS[L]
    K = len(tg)
    d_mel = torch.from_numpy(wins.reshape(-1, F)).cuda()
    d_row, d_valid = torch.from_numpy(np.arange(n, dtype=np.int64) * T).cuda(), torch.full((n,), T, dtype=torch.int32, device="cuda")
    d_value = torch.full((K * n + 100,), SENT, dtype=torch.float32, device="cuda")
    d_span = torch.full((K * n * 18 + 100,), SENT_B, dtype=torch.int8, device="cuda")
    d_lab, d_len = torch.full((n, 2), -9, dtype=torch.int32, device="cuda"), torch.full((n,), -9, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    e.ctc_align_windows_dev(d_mel.data_ptr(), n * T, d_row.data_ptr(), d_valid.data_ptr(), n, tg, "prefix", d_value.data_ptr(), d_span.data_ptr(), 2,
                            d_lab.data_ptr(), d_len.data_ptr())
    e.ctx.synchronize()
    v, s = d_value.cpu().numpy(), d_span.cpu().numpy()
    assert (v[K * n:] == SENT).all() and (s[K * n * 18:] == SENT_B).all()
    want = e.ctc_align(wins, tg, "prefix")
    umax = want.span.shape[2]
    np.testing.assert_array_equal(v[:K * n].reshape(K, n).view(np.uint32), want.value.view(np.uint32))
    s = s[:K * n * 18].reshape(K, n, 9, 2)
    np.testing.assert_array_equal(s[:, :, :umax], want.span)
    assert (s[:, :, umax:] == -1).all()
    np.testing.assert_array_equal(d_lab.cpu().numpy(), full.labels[:, :2])
    np.testing.assert_array_equal(d_len.cpu().numpy(), full.lengths)


def test_evaluate_ctc_with_align_adds_spans(models):
    from wwhip import ctc
    from wwhip.evaluate import evaluate_ctc
    e, wins, _ = models(4)
    rng = np.random.default_rng(11)
    lens = rng.integers(60, 201, 12)
    long = np.concatenate([wins[i] for i in range(40, 44)])
    clips = [long[o:o + n].copy() for o, n in zip(rng.integers(0, len(long) - 200, 12), lens)]
    hot = rng.integers(0, 2, 12)
    base = evaluate_ctc(e, clips, hot)
    assert "spans" not in base
    padded = np.zeros((12, 151, 40), np.float32)
    for i, c in enumerate(clips):
        padded[i, :min(len(c), 151)] = c[:151]
    want = e.ctc_align(padded, [(1, 2)], "exact")
    got = evaluate_ctc(e, clips, hot, align=True)
    for key, v in base.items():   # what it returns without align, unchanged
        np.testing.assert_array_equal(np.asarray(got[key]), np.asarray(v), err_msg=key)
    np.testing.assert_array_equal(got["align_value"].view(np.uint32), want.value[0].view(np.uint32))
    np.testing.assert_array_equal(got["spans"], want.span[0])
    np.testing.assert_array_equal(got["span_seconds"], ctc.span_seconds(want.span[0]))


# ---- 4: refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_come_before_anything_is_written(models, assets):
    import torch
    from wwhip import _lib, ctc
    from wwhip.engine import Engine
    e, wins, _ = models(4)
    lib, ctx = e._lib, e.ctx.handle
    d_steps = torch.full((4, 19, 4), 0.25, dtype=torch.float32, device="cuda")
    d_value = torch.full((64,), SENT, dtype=torch.float32, device="cuda")
    d_span = torch.full((64 * 18,), SENT_B, dtype=torch.int8, device="cuda")
    tab, lens = ctc.pack_targets([(1, 2)], 4)
    one = lambda v: np.array([v], np.int32)
    cases = [(dict(T=0), "T = 0"), (dict(T=65), "T = 65"), (dict(L=1), "L = 1"), (dict(L=65), "L = 65"), (dict(K=0), "K = 0"), (dict(K=9), "K = 9"),
             (dict(mode=2), "mode"), (dict(lens=one(0)), "U = 0"), (dict(lens=one(10)), "U = 10"), (dict(tab=np.full((1, 9), 3, np.int32)), "label"),
             (dict(tab=np.full((1, 9), -1, np.int32)), "label"), (dict(value=None), "NULL"), (dict(span=None), "NULL")]
    text = lambda: (lib.ww_last_error(ctx) or b"").decode()
    for kw, word in cases:
        a = dict(T=19, L=4, tab=tab, lens=lens, K=1, mode=0, value=d_value.data_ptr(), span=d_span.data_ptr())
        a.update(kw)
        rc = lib.ww_ctc_align_dev(ctx, d_steps.data_ptr(), 4, a["T"], a["L"], _lib.ptr(a["tab"]), _lib.ptr(a["lens"]), a["K"], a["mode"], a["value"], a["span"])
        assert rc == _lib.WW_EINVAL and word in text() and "ww_ctc_align_dev" in text(), (kw, rc, text())
    e.ctx.synchronize()
    assert (d_value.cpu().numpy() == SENT).all() and (d_span.cpu().numpy() == SENT_B).all()
    # the model forms: the same rules (L is the model's: label 3 is its blank), NULL outputs, and the model itself
    value, span = np.full((8, 3), SENT, np.float32), np.full((8, 3, 9, 2), SENT_B, np.int8)
    for kw, word in cases[4:]:
        a = dict(tab=tab, lens=lens, K=1, mode=0, value=_lib.ptr(value), span=_lib.ptr(span))
        a.update(kw)
        rc = lib.ww_ctc_align(ctx, e.handle, _lib.ptr(wins[:3]), 3, _lib.ptr(a["tab"]), _lib.ptr(a["lens"]), a["K"], a["mode"], a["value"], a["span"], 0, None, None)
        assert rc == _lib.WW_EINVAL and word in text(), (kw, text())
        got = ctypes.c_int64(0)
        rc = lib.ww_ctc_slide_align(ctx, e.handle, _lib.ptr(wins[0]), 151, 2, _lib.ptr(a["tab"]), _lib.ptr(a["lens"]), a["K"], a["mode"], a["value"], a["span"], 0,
                                    None, None, ctypes.byref(got))
        assert rc == _lib.WW_EINVAL, kw
    lab = np.full((3, 2), -9, np.int32)
    assert lib.ww_ctc_align(ctx, e.handle, _lib.ptr(wins[:3]), 3, _lib.ptr(tab), _lib.ptr(lens), 1, 0, _lib.ptr(value), _lib.ptr(span), 2, _lib.ptr(lab),
                            None) == _lib.WW_EINVAL
    assert (value == SENT).all() and (span == SENT_B).all() and (lab == -9).all()
    with pytest.raises(ValueError, match="label"):
        e.ctc_align(wins[:3], [(3,)])
    with pytest.raises(ValueError, match="K = 0"):
        e.ctc_align(wins[:3], [])
    with pytest.raises(ValueError, match="K = 9"):
        e.ctc_align(wins[:3], [(1,)] * 9)
    with pytest.raises(ValueError):
        e.ctc_slide_align(wins[0], 2, [(1, 2)], 2)
    # split-bf16 mode and a model that is no CTC model
    e.set_precision("bf16x3")
    try:
        with pytest.raises(ValueError):
            e.ctc_align(wins[:3], [(1, 2)])
    finally:
        e.set_precision("fp32")
    plain = Engine(os.path.join(assets, "CRNN_softmax"))
    try:
        with pytest.raises(ValueError, match="not a CTC"):
            plain.ctc_align(np.zeros((1, plain.window, plain.n_mel), np.float32), [(0,)])
        with pytest.raises(ValueError, match="not a CTC"):
            plain.ctc_slide_align(np.zeros((200, plain.n_mel), np.float32), 2, [(0,)])
        # the kernel alone takes any posteriors, whatever the engine's model
        y = np.full((3, 5, 4), 0.25, np.float32)
        gv, gs, _, _ = _align_dev(plain, y, [(1, 2)], "exact")
        wv, ws = _rows_host(y, [(1, 2)], "exact")
        np.testing.assert_array_equal(gv, wv)
        np.testing.assert_array_equal(gs, ws)
    finally:
        plain.close()

