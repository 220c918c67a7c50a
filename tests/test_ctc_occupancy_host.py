"""The forward-backward occupancy on the host: ``wwhip.ctc.occupancy`` (the float64 statement of csrc/ctc_occupancy.h) against the
enumeration of every path and against ``torch.nn.functional.ctc_loss`` in double, its sum rules, the library's host function
(``ww_ctc_occupancy_rows``) against the statement on the same float32 posteriors within the derived bound, the score's bits, the
``Z == 0`` cases, the refusals, and ``CtcOccupancy``'s properties on a hand case."""

import numpy as np
import pytest

import ctc64
import ctc_occupancy64 as O64
import ctc_score64 as S64
from wwhip import _lib, ctc


def test_float64_statement_equals_path_enumeration():
    tables = O64.small_tables()
    assert len(tables) >= 300
    worst, some, none = 0.0, 0, 0
    for y, c in tables:
        want = O64.enumerate_occupancy(y, c)
        for mode in O64.MODES:
            got = ctc.occupancy(y, [c], mode)
            Z, occ, cls = want[mode]
            d = [abs(got.value[0, 0] - Z), np.abs(got.occ[0, 0] - occ).max()]
            if mode == "exact":
                d.append(np.abs(got.cls[0, 0] - cls).max())
            else:
                assert got.cls is None
            worst = max(worst, *d)
            some, none = some + (Z > 0), none + (Z == 0)
            if Z == 0:
                assert got.value[0, 0] == 0 and not got.occ.any() and (got.cls is None or not got.cls.any())
    print(f"\n{len(tables)} tables: worst |statement - enumeration| = {worst:.3g}; {some} with a path, {none} without", end="")
    assert worst <= 1e-12 and some > 300 and none > 20


@pytest.mark.parametrize("L", [4, 8])
@pytest.mark.parametrize("repeat", [False, True])
def test_cls_is_what_torch_ctc_loss_differentiates_to(L, repeat):
    """``torch.nn.functional.ctc_loss`` in float64 on the CPU, ``log_probs = log(y)``, T = 19: ``exp(-loss)`` is ``value``, and
    ``y - log_probs.grad`` is ``cls`` (torch hands back the gradient with respect to the logits under the log-softmax, ``y - cls``)."""
    import torch
    rng = np.random.default_rng(40 + L + repeat)
    T, n = 19, 6
    y = rng.dirichlet(np.full(L, 0.8), (n, T))
    c = (1, 1, 0) if repeat else (1, 2, 0) if L > 4 else (1, 2)
    got = ctc.occupancy(y, [c], "exact")
    lp = torch.tensor(np.log(y).transpose(1, 0, 2), dtype=torch.float64, requires_grad=True)   # [T, n, L]
    tg = torch.tensor([c] * n, dtype=torch.long)
    rel = ab = 0.0
    for i in range(n):   # (one clip at a time: reduction="sum" over one clip is its own loss)
        lp.grad = None
        loss = torch.nn.functional.ctc_loss(lp[:, i:i + 1], tg[i:i + 1], torch.tensor([T]), torch.tensor([len(c)]), blank=L - 1, reduction="sum")
        loss.backward()
        rel = max(rel, abs(np.exp(-loss.item()) - got.value[0, i]) / got.value[0, i])
        ab = max(ab, np.abs((y[i] - lp.grad[:, i].numpy()) - got.cls[0, i]).max())
    print(f"\nL={L} c={c}: exp(-loss) vs value {rel:.3g} relative; y - grad vs cls {ab:.3g}", end="")
    assert rel <= 1e-12 and ab <= 1e-12


def test_sum_rules():
    rng = np.random.default_rng(3)
    for L, c in ((4, (1, 2)), (4, (1, 1)), (8, (3, 4, 5)), (2, (0,)), (12, (0, 1, 2, 3, 4, 5, 6, 7, 8))):
        y = rng.dirichlet(np.full(L, 0.5), (9, 19))
        ex, pr = ctc.occupancy(y, [c], "exact"), ctc.occupancy(y, [c], "prefix")
        assert (ex.value > 0).all() and (pr.value >= ex.value).all()
        np.testing.assert_allclose(ex.cls.sum(-1), 1.0, atol=1e-12)
        np.testing.assert_allclose(pr.occ[0, :, :, len(c) - 1].sum(-1), 1.0, atol=1e-12)
        assert (ex.blank >= -1e-12).all() and (ex.occ >= 0).all() and (pr.occ >= 0).all()
        np.testing.assert_allclose(ex.blank, ex.cls[..., L - 1], atol=1e-12)   # the blank's share, two ways
        assert not ex.occ[..., len(c):].any() and not pr.occ[..., len(c):].any()


@pytest.mark.parametrize("L", ctc64.LS)
@pytest.mark.parametrize("mode", O64.MODES)
def test_host_function_is_within_the_arithmetic_bound_of_the_statement(L, mode):
    steps = ctc64.reference(L)[2].astype(np.float32)   # the float64 model's posteriors, cast
    worst = 0.0
    for c in S64.TARGETS[L]:
        g64, g32 = ctc.occupancy(steps, [c], mode), ctc.occupancy_rows(steps, [c], mode)
        assert g32.occ.dtype == np.float32 and g32.occ.shape == (1, len(steps), 19, 9)
        np.testing.assert_array_equal(g32.value.view(np.uint32), ctc.score_rows(steps, [c], mode).view(np.uint32))   # the score's bits
        bound = O64.arithmetic_bound(g64.occ, g64.value, 19, len(c))
        err = np.abs(g32.occ.astype(np.float64) - g64.occ)
        worst = max(worst, (err / np.maximum(bound, 1e-300)).max())
        assert (err <= bound).all()
        if mode == "exact":
            bound = O64.arithmetic_bound(g64.cls, g64.value, 19, len(c), classes=True)
            err = np.abs(g32.cls.astype(np.float64) - g64.cls)
            worst = max(worst, (err / np.maximum(bound, 1e-300)).max())
            assert (err <= bound).all()
        else:
            assert g32.cls is None
    print(f"\nL={L} {mode}: worst needed fraction of the arithmetic bound {worst:.3f}", end="")


def test_float32_statement_carries_the_host_functions_bits():
    """``ctc.occupancy(dtype=float32)`` does the header's operations in the header's order."""
    for y, c in O64.random_tables(n=200):
        for mode in O64.MODES:
            a, b = ctc.occupancy(y, [c], mode, dtype=np.float32), ctc.occupancy_rows(y, [c], mode)
            np.testing.assert_array_equal(a.value.view(np.uint32), b.value.view(np.uint32))
            np.testing.assert_array_equal(a.occ.view(np.uint32), b.occ.view(np.uint32))
            if mode == "exact":
                np.testing.assert_array_equal(a.cls.view(np.uint32), b.cls.view(np.uint32))


def test_no_path_gives_zeros_everywhere():
    rng = np.random.default_rng(9)
    y = rng.dirichlet(np.ones(4), (3, 2)).astype(np.float32)
    short = ctc.occupancy_rows(y, [(0, 1, 2)], "exact")   # T = 2 < U = 3
    y5 = rng.dirichlet(np.ones(4), (3, 5)).astype(np.float32)
    y5[:, :, 1] = 0.0   # a zeroed column: no path reads label 1
    for r in (short, ctc.occupancy_rows(y, [(0, 1, 2)], "prefix"), ctc.occupancy_rows(y5, [(0, 1)], "exact"), ctc.occupancy_rows(y5, [(0, 1)], "prefix"),
              ctc.occupancy(y5, [(0, 1)], "exact"), ctc.occupancy(y, [(1, 1)], "prefix")):
        assert not r.value.any() and not r.occ.any() and (r.cls is None or not r.cls.any())
        assert not np.signbit(r.occ).any() and (r.cls is None or not np.signbit(r.cls).any())
    assert np.isinf(short.loss).all() and not short.grad(y).any() and np.isnan(short.expected_step).all()


def test_every_byte_is_written():
    y = np.random.default_rng(2).dirichlet(np.ones(5), (4, 7)).astype(np.float32)
    tab, lens = ctc.pack_targets([(0, 1), (2,)], 5)
    for mode, want_cls in ((0, True), (0, False), (1, False)):
        value, occ, cls = np.full((2, 4), np.nan, np.float32), np.full((2, 4, 7, 9), np.nan, np.float32), np.full((2, 4, 7, 5), np.nan, np.float32)
        assert _lib.load().ww_ctc_occupancy_rows(_lib.ptr(y), 4, 7, 5, _lib.ptr(tab), _lib.ptr(lens), 2, mode, _lib.ptr(value), _lib.ptr(occ),
                                                 _lib.ptr(cls) if want_cls else None) == 0
        assert not np.isnan(value).any() and not np.isnan(occ).any() and np.isnan(cls).any() != want_cls
        assert not occ[0, :, :, 2:].any() and not occ[1, :, :, 1:].any()


def test_refusals():
    lib = _lib.load()
    y = np.full((2, 3, 4), 0.25, np.float32)
    tab, lens = ctc.pack_targets([(1, 2)], 4)
    one = lambda v: np.array([v], np.int32)
    value, occ, cls = np.full((1, 2), -7, np.float32), np.full((1, 2, 3, 9), -7, np.float32), np.full((1, 2, 3, 4), -7, np.float32)
    cases = [(dict(T=0), "T = 0"), (dict(T=65), "T = 65"), (dict(L=1), "L = 1"), (dict(L=65), "L = 65"), (dict(K=0), "K = 0"), (dict(K=9), "K = 9"),
             (dict(mode=2), "mode"), (dict(lens=one(0)), "U = 0"), (dict(lens=one(10)), "U = 10"), (dict(tab=np.full((1, 9), 3, np.int32)), "label"),
             (dict(tab=np.full((1, 9), -1, np.int32)), "label"), (dict(tab=None), "NULL"), (dict(lens=None), "NULL"), (dict(value=None), "NULL"),
             (dict(occ=None), "NULL"), (dict(mode=1), "cls"), (dict(n=-1), "negative"), (dict(steps=None), "NULL")]
    for kw, word in cases:
        a = dict(steps=y, n=2, T=3, L=4, tab=tab, lens=lens, K=1, mode=0, value=value, occ=occ, cls=cls)
        a.update(kw)
        p = lambda k: None if a[k] is None else _lib.ptr(a[k])
        rc = lib.ww_ctc_occupancy_rows(p("steps"), a["n"], a["T"], a["L"], p("tab"), p("lens"), a["K"], a["mode"], p("value"), p("occ"), p("cls"))
        text = (lib.ww_last_error(None) or b"").decode()
        assert rc == _lib.WW_EINVAL and word in text and "ww_ctc_occupancy_rows" in text, (kw, rc, text)
    assert (value == -7).all() and (occ == -7).all() and (cls == -7).all()
    assert lib.ww_ctc_occupancy_rows(None, 0, 3, 4, _lib.ptr(tab), _lib.ptr(lens), 1, 0, _lib.ptr(value), _lib.ptr(occ), None) == 0   # n = 0
    with pytest.raises(ValueError, match="cls"):
        ctc.occupancy_rows(y, [(1, 2)], "prefix", want_classes=True)
    with pytest.raises(ValueError, match="label"):
        ctc.occupancy(y, [(3,)])
    with pytest.raises(ValueError, match="mode"):
        ctc.occupancy(y, [(1,)], "best")


def test_properties_on_hey_snips_rows():
    B = 3
    y = ctc64._rows([B, 1, 1, B, B, 2, 2, B], 4)
    for r in (ctc.occupancy(y, [(1, 2)], "exact"), ctc.occupancy_rows(y, [(1, 2)], "exact")):
        assert r.value.shape == (1, 1) and r.occ.shape == (1, 1, 8, 9) and r.cls.shape == (1, 1, 8, 4)
        es = r.expected_step
        assert es.shape == (1, 1, 9) and 1 <= es[0, 0, 0] <= 2 and 5 <= es[0, 0, 1] <= 6 and np.isnan(es[0, 0, 2:]).all()
        np.testing.assert_allclose(r.loss, -np.log(r.value.astype(np.float64)), rtol=1e-6)
        np.testing.assert_allclose(r.blank, 1 - r.occ.sum(-1), atol=0)
        np.testing.assert_allclose(r.blank[0, 0], r.cls[0, 0, :, B], atol=1e-5)
        g = r.grad(y)
        assert g.shape == (1, 1, 8, 4)
        np.testing.assert_allclose(g[0, 0], y - r.cls[0, 0], atol=1e-7)
        np.testing.assert_allclose(g.sum(-1), 0, atol=1e-5)   # a gradient with respect to logits sums to 0 over the classes
        # the path [B 1 1 B B 2 2 B] dominates: its steps hold their labels almost surely
        assert r.occ[0, 0, 1, 0] > 0.8 and r.occ[0, 0, 2, 0] > 0.8 and r.occ[0, 0, 5, 1] > 0.8 and r.occ[0, 0, 6, 1] > 0.8 and r.blank[0, 0, 0] > 0.8
    p = ctc.occupancy(y, [(1, 2)], "prefix")
    assert p.cls is None and abs(p.occ[0, 0, :, 1].sum() - 1) < 1e-12 and p.occ[0, 0, 5, 1] > 0.8 and p.occ[0, 0, :, 1].argmax() == 5
    with pytest.raises(ValueError, match="cls"):
        p.grad(y)
