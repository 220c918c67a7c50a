"""The forward-backward occupancy on the MI355X: ctc_occupancy_kernel's value, occ and cls (as bits) against the host function of the
same header (``ww_ctc_occupancy_rows``), the words it writes, the model forms end to end against the float64 model, one window
through every form, and the refusals.

Shapes: the 1,500 seeded tables of the native check grouped by (T, L), and calls built so that every kernel shape runs: U = 1, 3, 7, 9
select the segment widths P = 4, 8, 16, 32; K = 1, and K = 8 with mixed lengths in one call; with K = 1 the number of pairs is one
less than, equal to and one more than the 256 / P pairs of a workgroup (the dead-tail segment, and a segment's top lane beside its
neighbour's state 0); T = 1 (no loop), 2 (one step), 19 (the models') and 64 (the limit, 64 KB of LDS); L = 2 and 64; with and without
cls.  The model forms run on the standard geometry: 70 and 75 windows stay inside one chunk."""
import ctypes
import os

import numpy as np
import pytest

import ctc64
import ctc_occupancy64 as O64
import ctc_score64 as S64

pytestmark = pytest.mark.gpu

CANARY = np.uint32(0x55555555)
PAD = 512   # guard words on both sides of every output


@pytest.fixture(scope="module")
def models():
    from wwhip.engine import Engine
    cache = {}

    def get(L):
        if L not in cache:
            b, wins, _, _ = ctc64.reference(L)
            cache[L] = (Engine(f"synthetic-ctc-{L}", bundle=b), wins)
        return cache[L]
    yield get
    for e, _ in cache.values():
        e.close()


def _guarded(words):
    import torch
    return torch.full((PAD + words + PAD,), int(CANARY), dtype=torch.int32, device="cuda")


def _split(buf, words):
    """-> (the words, True if both guards are intact)."""
    a = buf.cpu().numpy().view(np.uint32)
    return a[PAD:PAD + words], bool((a[:PAD] == CANARY).all() and (a[PAD + words:] == CANARY).all())


def _occ_dev(e, steps, targets, mode, want_cls):
    """``ctc_occupancy_dev`` on host posteriors ``[n, T, L]`` -> ``(value [K, n], occ [K, n, T, 9], cls [K, n, T, L] | None)`` as
    uint32; the outputs start as canaries between guard words, which must be intact, and every word must have been written."""
    import torch
    n, T, L = steps.shape
    K = len(targets)
    d_steps = torch.from_numpy(np.ascontiguousarray(steps, np.float32)).cuda()
    nv, no, nc = K * n, K * n * T * 9, K * n * T * L
    d_value, d_occ, d_cls = _guarded(nv), _guarded(no), _guarded(nc)
    torch.cuda.synchronize()
    e.ctc_occupancy_dev(d_steps.data_ptr(), n, T, L, targets, mode, d_value.data_ptr() + 4 * PAD, d_occ.data_ptr() + 4 * PAD,
                        d_cls.data_ptr() + 4 * PAD if want_cls else 0)
    e.ctx.synchronize()
    (v, gv), (o, go), (c, gc) = _split(d_value, nv), _split(d_occ, no), _split(d_cls, nc)
    assert gv and go and gc, "a guard word was written"
    assert (v != CANARY).all() and (o != CANARY).all(), "an output word was not written"
    if want_cls:
        assert (c != CANARY).all(), "a cls word was not written"
    else:
        assert (c == CANARY).all(), "cls was written though none was passed"
    return v.reshape(K, n), o.reshape(K, n, T, 9), c.reshape(K, n, T, L) if want_cls else None


def _assert_host_bits(e, steps, targets, mode, want_cls, msg):
    from wwhip import ctc
    v, o, c = _occ_dev(e, steps, targets, mode, want_cls)
    w = ctc.occupancy_rows(steps, targets, mode, want_classes=want_cls)
    np.testing.assert_array_equal(v, w.value.view(np.uint32), err_msg=msg)
    np.testing.assert_array_equal(o, w.occ.view(np.uint32), err_msg=msg)
    if want_cls:
        np.testing.assert_array_equal(c, w.cls.view(np.uint32), err_msg=msg)
    for k, tg in enumerate(targets):
        assert not o[k, :, :, len(tg):].any(), msg + ": a row past U is not +0"
    return v


# ---- (a) the kernel's bits --------------------------------------------------------------------------------------------------------------
def test_seeded_tables_carry_the_host_functions_bits(models):
    """The native check's 1,500 tables, grouped by (T, L); a group's targets go eight to a call, over all of its tables."""
    e = models(2)[0]
    groups = {}
    for y, c in O64.random_tables():
        groups.setdefault(y.shape, []).append((y, c))
    calls = some = none = 0
    for (T, L), tabs in sorted(groups.items()):
        steps = np.stack([y for y, _ in tabs])
        targets = sorted({c for _, c in tabs})
        for j in range(0, len(targets), 8):
            tg = targets[j:j + 8]
            for mode, want_cls in (("exact", True), ("prefix", False)):
                v = _assert_host_bits(e, steps, tg, mode, want_cls, f"T={T} L={L} {tg} {mode}")
                calls, some, none = calls + 1, some + int((v != 0).sum()), none + int((v == 0).sum())
    print(f"\n{len(groups)} (T, L) groups, {calls} calls: {some} pairs with a path, {none} without", end="")
    assert some > 1000 and none > 100


def _targets(rng, L, us):
    out = []
    for j, U in enumerate(us):
        c = rng.integers(0, L - 1, U)
        if L > 2:
            for u in range(1, U):
                while c[u] == c[u - 1]:
                    c[u] = rng.integers(0, L - 1)
            if j % 2 and U >= 2:   # every other target with equal neighbours
                c[1] = c[0]
        out.append(tuple(int(v) for v in c))
    return out


def _tables(rng, n, T, L, targets):
    """Sequence i follows a path that reads target i % K (0.7 on the path's class, so that a product of 64 posteriors does not
    underflow), dwelling a random number of steps per state; a third of the sequences lie on a grid of sixteenths (exact zeros);
    every seventh has one label of its target zeroed on every row (no path at all)."""
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


@pytest.mark.parametrize("U", [1, 3, 7, 9])
def test_every_kernel_shape(models, U):
    e = models(2)[0]
    P = {1: 4, 3: 8, 7: 16, 9: 32}[U]
    per = 256 // P
    mixed = [U, 1, max(U - 1, 1), U, 2 if U > 2 else 1, U, 1, max(U - 2, 1)]   # K = 8: the longest selects P
    rng = np.random.default_rng(U)
    some = none = 0
    for T in (1, 2, 19, 64):
        for L in (2, 64):
            for us, ns in (((U,), (per - 1, per, per + 1)), (mixed, (per // 8, per // 8 + 1))):
                tg = _targets(rng, L, us)
                for n in ns:
                    y = _tables(rng, n, T, L, tg)
                    for mode, want_cls in (("exact", True), ("exact", False), ("prefix", False)):
                        v = _assert_host_bits(e, y, tg, mode, want_cls, f"U={U} T={T} L={L} K={len(tg)} n={n} {mode} cls={want_cls}")
                        some, none = some + int((v != 0).sum()), none + int((v == 0).sum())
    print(f"\nU={U} (P={P}): {some} pairs with a path, {none} without", end="")
    assert some > 0 and none > 0


def test_a_second_call_and_an_empty_call(models):
    import torch
    e = models(2)[0]
    rng = np.random.default_rng(77)
    tg = _targets(rng, 4, (2, 3, 1))
    y = _tables(rng, 67, 19, 4, tg)   # 201 pairs: workgroups of 32, the last with dead segments
    a, b = _occ_dev(e, y, tg, "exact", True), _occ_dev(e, y, tg, "exact", True)
    for x, z in zip(a, b):
        np.testing.assert_array_equal(x, z)
    d = _guarded(64)
    e.ctc_occupancy_dev(0, 0, 19, 4, tg, "exact", d.data_ptr() + 4 * PAD, d.data_ptr() + 4 * PAD, 0)   # n = 0: nothing read or written
    e.ctx.synchronize()
    assert (d.cpu().numpy().view(np.uint32) == CANARY).all()


# ---- (b) end to end against the float64 model -------------------------------------------------------------------------------------------
Z_FLOOR = 2.0e-17   # every window of the float64 reference, every target and mode: the absolute term stays under 1e-18


@pytest.mark.parametrize("L", ctc64.LS)
def test_engine_occupancy_is_within_the_model_bound_of_the_float64_model(models, L):
    from wwhip import ctc
    e, wins = models(L)
    steps64 = ctc64.reference(L)[2]
    tg = S64.TARGETS[L]
    worst = 0.0
    for mode in O64.MODES:
        want = ctc.occupancy(steps64, tg, mode)
        assert want.value.shape == (len(tg), len(wins)) and (want.value >= Z_FLOOR).all(), want.value.min()   # no window left out
        got = e.ctc_occupancy(wins, tg, mode, want_classes=mode == "exact")
        assert got.value.dtype == np.float32 and got.occ.shape == (len(tg), len(wins), 19, 9) and got.occ.dtype == np.float32
        np.testing.assert_array_equal(got.value.view(np.uint32), e.ctc_score(wins, tg, mode).view(np.uint32))
        for k, c in enumerate(tg):
            bound = O64.model_bound(want.occ[k], want.value[k], len(c))
            err = np.abs(got.occ[k].astype(np.float64) - want.occ[k])
            worst = max(worst, (err / np.maximum(bound, 1e-300)).max())
            assert (err <= bound).all(), (mode, c, (err / np.maximum(bound, 1e-300)).max())
            if mode == "exact":
                assert got.cls.shape == (len(tg), len(wins), 19, L)
                bound = O64.model_bound(want.cls[k], want.value[k], len(c), classes=True)
                err = np.abs(got.cls[k].astype(np.float64) - want.cls[k])
                worst = max(worst, (err / np.maximum(bound, 1e-300)).max())
                assert (err <= bound).all(), (mode, c, "cls", (err / np.maximum(bound, 1e-300)).max())
            else:
                assert got.cls is None
    print(f"\nL={L}: worst needed fraction of the model bound {worst:.3f}", end="")


# ---- (c) one window, whatever the path -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", ctc64.LS)
def test_one_window_gives_the_same_bits_through_every_form(models, L):
    import torch
    e, _ = models(L)
    tg = S64.TARGETS[L]
    K = len(tg)
    mel, cut = S64.slide_mel(L), S64.slide_windows(L)
    n = len(cut)
    assert n == 75
    d_mel = torch.from_numpy(np.ascontiguousarray(mel)).cuda()
    d_row, d_valid = torch.from_numpy(np.arange(n, dtype=np.int64) * 2).cuda(), torch.full((n,), 151, dtype=torch.int32, device="cuda")
    fwd = e.ctc_forward(cut, max_labels=2)
    for mode in O64.MODES:
        want_cls = mode == "exact"
        want = e.ctc_occupancy(cut, tg, mode, want_classes=want_cls)
        got, dec = e.ctc_slide_occupancy(mel, 2, tg, mode, want_classes=want_cls, max_labels=2)
        nv, no, nc = K * n, K * n * 19 * 9, K * n * 19 * L
        d_value, d_occ, d_cls = _guarded(nv), _guarded(no), _guarded(nc)
        d_lab, d_len = torch.full((n, 2), -9, dtype=torch.int32, device="cuda"), torch.full((n,), -9, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        e.ctc_occupancy_windows_dev(d_mel.data_ptr(), len(mel), d_row.data_ptr(), d_valid.data_ptr(), n, tg, mode, d_value.data_ptr() + 4 * PAD,
                                    d_occ.data_ptr() + 4 * PAD, d_cls.data_ptr() + 4 * PAD if want_cls else 0, 2, d_lab.data_ptr(), d_len.data_ptr())
        e.ctx.synchronize()
        (v, gv), (o, go), (c, gc) = _split(d_value, nv), _split(d_occ, no), _split(d_cls, nc)
        assert gv and go and gc
        for name, a, b, d in (("value", want.value, got.value, v), ("occ", want.occ, got.occ, o), ("cls", want.cls, got.cls, c)):
            if a is None:
                assert b is None and (d == CANARY).all()
                continue
            np.testing.assert_array_equal(b.view(np.uint32), a.view(np.uint32), err_msg=f"{name} {mode}: slide")
            np.testing.assert_array_equal(d.reshape(a.shape), a.view(np.uint32), err_msg=f"{name} {mode}: windows_dev")
        np.testing.assert_array_equal(dec.labels, fwd.labels)
        np.testing.assert_array_equal(dec.lengths, fwd.lengths)
        np.testing.assert_array_equal(d_lab.cpu().numpy(), fwd.labels)
        np.testing.assert_array_equal(d_len.cpu().numpy(), fwd.lengths)
    none = e.ctc_slide_occupancy(mel[:150], 2, tg, "exact")
    assert none.value.shape == (K, 0) and none.occ.shape == (K, 0, 19, 9)


# ---- (d) refusals ------------------------------------------------------------------------------------------------------------------------------
def test_refusals_come_before_anything_is_written(models, assets):
    import torch
    from wwhip import _lib, ctc
    from wwhip.engine import Engine
    e, wins = models(4)
    lib, ctx = e._lib, e.ctx.handle
    d_steps = torch.full((4, 19, 4), 0.25, dtype=torch.float32, device="cuda")
    d_value, d_occ, d_cls = _guarded(64), _guarded(4 * 19 * 9), _guarded(4 * 19 * 4)
    tab, lens = ctc.pack_targets([(1, 2)], 4)
    one = lambda v: np.array([v], np.int32)
    cases = [(dict(T=0), "T = 0"), (dict(T=65), "T = 65"), (dict(L=1), "L = 1"), (dict(L=65), "L = 65"), (dict(K=0), "K = 0"), (dict(K=9), "K = 9"),
             (dict(mode=2), "mode"), (dict(lens=one(0)), "U = 0"), (dict(lens=one(10)), "U = 10"), (dict(tab=np.full((1, 9), 3, np.int32)), "label"),
             (dict(tab=np.full((1, 9), -1, np.int32)), "label"), (dict(tab=None), "NULL"), (dict(lens=None), "NULL"), (dict(value=None), "NULL"),
             (dict(occ=None), "NULL"), (dict(mode=1), "cls")]
    text = lambda: (lib.ww_last_error(ctx) or b"").decode()
    for kw, word in cases:
        a = dict(T=19, L=4, tab=tab, lens=lens, K=1, mode=0, value=d_value.data_ptr() + 4 * PAD, occ=d_occ.data_ptr() + 4 * PAD, cls=d_cls.data_ptr() + 4 * PAD)
        a.update(kw)
        p = lambda k: None if a[k] is None else _lib.ptr(a[k])
        rc = lib.ww_ctc_occupancy_dev(ctx, d_steps.data_ptr(), 4, a["T"], a["L"], p("tab"), p("lens"), a["K"], a["mode"], a["value"], a["occ"], a["cls"])
        assert rc == _lib.WW_EINVAL and word in text() and "ww_ctc_occupancy_dev" in text(), (kw, rc, text())
    rc = lib.ww_ctc_occupancy_dev(ctx, None, 4, 19, 4, _lib.ptr(tab), _lib.ptr(lens), 1, 0, d_value.data_ptr() + 4 * PAD, d_occ.data_ptr() + 4 * PAD, None)
    assert rc == _lib.WW_EINVAL and "NULL" in text()
    e.ctx.synchronize()
    for d in (d_value, d_occ, d_cls):
        assert (d.cpu().numpy().view(np.uint32) == CANARY).all()
    # the model forms: the same rules (L is the model's: label 3 is its blank), NULL outputs, the decode's pair, and the model itself
    value, occ, cls = np.full((8, 3), -7, np.float32), np.full((8, 3, 19, 9), -7, np.float32), np.full((8, 3, 19, 4), -7, np.float32)
    got = ctypes.c_int64(0)
    for kw, word in cases[4:]:
        a = dict(tab=tab, lens=lens, K=1, mode=0, value=value, occ=occ, cls=cls)
        a.update(kw)
        p = lambda k: None if a[k] is None else _lib.ptr(a[k])
        rc = lib.ww_ctc_occupancy(ctx, e.handle, _lib.ptr(wins[:3]), 3, p("tab"), p("lens"), a["K"], a["mode"], p("value"), p("occ"), p("cls"), 0, None, None)
        assert rc == _lib.WW_EINVAL and word in text() and "ww_ctc_occupancy" in text(), (kw, text())
        rc = lib.ww_ctc_slide_occupancy(ctx, e.handle, _lib.ptr(wins[0]), 151, 2, p("tab"), p("lens"), a["K"], a["mode"], p("value"), p("occ"), p("cls"), 0,
                                        None, None, ctypes.byref(got))
        assert rc == _lib.WW_EINVAL and word in text() and "ww_ctc_slide_occupancy" in text(), (kw, text())
        rc = lib.ww_ctc_occupancy_windows_dev(ctx, e.handle, d_steps.data_ptr(), 151, d_steps.data_ptr(), d_steps.data_ptr(), 1, p("tab"), p("lens"), a["K"],
                                              a["mode"], None if a["value"] is None else d_value.data_ptr() + 4 * PAD,
                                              None if a["occ"] is None else d_occ.data_ptr() + 4 * PAD, d_cls.data_ptr() + 4 * PAD, 0, None, None)
        assert rc == _lib.WW_EINVAL and word in text() and "ww_ctc_occupancy_windows_dev" in text(), (kw, text())
    lab = np.full((3, 2), -9, np.int32)
    assert lib.ww_ctc_occupancy(ctx, e.handle, _lib.ptr(wins[:3]), 3, _lib.ptr(tab), _lib.ptr(lens), 1, 0, _lib.ptr(value), _lib.ptr(occ), None, 2,
                                _lib.ptr(lab), None) == _lib.WW_EINVAL and "go together" in text()
    assert lib.ww_ctc_occupancy(ctx, e.handle, _lib.ptr(wins[:3]), 3, _lib.ptr(tab), _lib.ptr(lens), 1, 0, _lib.ptr(value), _lib.ptr(occ), None, 20,
                                _lib.ptr(lab), _lib.ptr(lab)) == _lib.WW_EINVAL and "max_labels" in text()
    e.ctx.synchronize()
    assert (value == -7).all() and (occ == -7).all() and (cls == -7).all() and (lab == -9).all()
    for d in (d_value, d_occ, d_cls):
        assert (d.cpu().numpy().view(np.uint32) == CANARY).all()
    with pytest.raises(ValueError, match="label"):
        e.ctc_occupancy(wins[:3], [(3,)])
    with pytest.raises(ValueError, match="K = 0"):
        e.ctc_occupancy(wins[:3], [])
    with pytest.raises(ValueError, match="cls"):
        e.ctc_occupancy(wins[:3], [(1, 2)], "prefix", want_classes=True)
    with pytest.raises(ValueError):
        e.ctc_slide_occupancy(wins[0], 2, [(1, 2)], 2)
    # split-bf16 mode and a model that is no CTC model: the family's message
    e.set_precision("bf16x3")
    try:
        with pytest.raises(ValueError):
            e.ctc_occupancy(wins[:3], [(1, 2)])
    finally:
        e.set_precision("fp32")
    plain = Engine(os.path.join(assets, "CRNN_softmax"))
    try:
        with pytest.raises(ValueError, match="not a CTC"):
            plain.ctc_occupancy(np.zeros((1, plain.window, plain.n_mel), np.float32), [(0,)])
        with pytest.raises(ValueError, match="not a CTC"):
            plain.ctc_slide_occupancy(np.zeros((200, plain.n_mel), np.float32), 2, [(0,)])
        # the kernel alone takes any posteriors, whatever the engine's model
        _assert_host_bits(plain, np.full((3, 5, 4), 0.25, np.float32), [(1, 2)], "exact", True, "plain engine")
    finally:
        plain.close()
