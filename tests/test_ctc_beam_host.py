"""The prefix beam search without a GPU: the float64 statement (``wwhip.ctc.beam_search``) against enumeration of all paths and
against ``ctc.score``, hand cases, the order's properties, the library's host function (``ww_ctc_beam_rows``) against the float32
form of the statement bit for bit, the header / binding / exports, and the refusals."""
import os
import re

import numpy as np
import pytest

import ctc64
import ctc_beam64 as B64

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CSRC = os.path.join(_ROOT, "wakeword-detection_amd", "csrc")

FAMILY = {"ww_ctc_beam_dev": 11, "ww_ctc_beam_rows": 10, "ww_ctc_beam": 10, "ww_ctc_beam_windows_dev": 13, "ww_ctc_slide_beam": 12,
          "ww_stream_step_ctc_beam": 14}


# ---- the statement ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,L", [(1, 2), (6, 2), (3, 4), (5, 3)])
def test_an_exhaustive_beam_is_the_enumeration_of_all_paths(T, L):
    """Every prefix count here is at most 64, so a beam of 64 prunes nothing: the strings and their probabilities are exact."""
    from wwhip import ctc
    rng = np.random.default_rng(10 * T + L)
    for trial in range(3):
        y = rng.dirichlet(np.full(L, 0.5), T)
        if trial == 2:
            y = np.round(y * 16) / 16   # exact zeros: strings that no path reaches
        want = {s: p for s, p in B64.enumerate_strings(y).items() if p > 0}
        assert len(want) <= 64
        got = {}
        steps_trace = []
        beam = ctc.beam_search(y, 64, 8, trace=steps_trace)
        ranks, keys = steps_trace[0][-1]
        for r, k in zip(ranks, keys):
            if r > 0:
                got[ctc.key_labels(k)] = float(r)
        assert set(got) == set(want)
        for s, p in want.items():
            assert abs(got[s] - p) <= 1e-13, (s, got[s], p)
        # the reported paths: the most probable strings, each the exact score of its string
        top = sorted(want.items(), key=lambda kv: -kv[1])
        for place, (s, p) in enumerate(B64.strings_of(beam)):
            if place >= len(top):
                assert s is None and p == 0
                continue
            assert abs(p - top[place][1]) <= 1e-13
            assert abs(p - want[s]) <= 1e-13
            if len(s) >= 1:
                assert abs(p - ctc.score(y, [s], "exact")[0, 0]) <= 1e-13
            else:
                assert abs(p - np.prod(y[:, L - 1])) <= 1e-13


def test_hand_cases():
    from wwhip import ctc
    cases = {name: steps for name, steps, _, _, _ in ctc64.hand_cases()}
    top = ctc.beam_search(cases["hey snips"], 8, 2)
    assert B64.strings_of(top)[0][0] == (1, 2) and top.lengths[0, 0] == 2 and top.labels.shape == (1, 2, 8)
    blank = ctc.beam_search(cases["all blank"], 8, 1)
    assert blank.lengths[0, 0] == 0 and blank.probs[0, 0] > 0 and (blank.labels == -1).all()
    # rows that admit fewer than P strings of probability above 0: the places past them are absent
    only = np.zeros((4, 4))
    only[:, 3] = 1.0
    only[1] = [0, 0.5, 0, 0.5]
    few = ctc.beam_search(only, 8, 4)
    assert [s for s, _ in B64.strings_of(few)] == [(), (1,), None, None] or [s for s, _ in B64.strings_of(few)] == [(1,), (), None, None]
    assert few.lengths[0].tolist()[2:] == [-1, -1] and (few.probs[0, 2:] == 0).all() and (few.labels[0, 2:] == -1).all()
    assert np.isneginf(few.log_probs[0, 2:]).all() and np.isfinite(few.log_probs[0, :2]).all()
    one = ctc.beam_search(cases["one step"], 1, 1, 1)
    assert B64.strings_of(one)[0][0] == (2,)
    # max_labels cuts the labels, not the length
    cut = ctc.beam_search(cases["repeats collapsed"], 8, 1, 2)
    assert cut.lengths[0, 0] == 3 and cut.labels[0, 0].tolist() == [0, 2]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_properties_descending_distinct_and_ties_by_key(dtype):
    from wwhip import ctc
    rng = np.random.default_rng(3)
    for L in (2, 3, 5, 8):
        y = B64.tables(rng, 12, 19, L)
        for W, P in ((1, 1), (4, 4), (64, 8)):
            b = ctc.beam_search(y, W, P, dtype=dtype)
            assert (np.diff(b.probs, axis=1) <= 0).all()
            for i in range(len(y)):
                strings = [s for s, _ in B64.strings_of(b, i) if s is not None]
                assert len(set(strings)) == len(strings)
    # a grid of sixteenths with flat rows: equal totals, which the key orders - shorter first, then lexicographic
    flat = np.full((2, 3), 1.0 / 4, dtype)
    flat[:, 2] = 0.5
    b = ctc.beam_search(flat, 64, 8, dtype=dtype)
    got = B64.strings_of(b)
    want = B64.enumerate_strings(flat)
    order = sorted(want.items(), key=lambda kv: (-kv[1], len(kv[0]), kv[0]))
    assert [s for s, _ in got][:len(order)] == [s for s, _ in order][:8]
    assert len({p for _, p in order}) < len(order)   # there ARE ties
    # NaN ranks below every number, +Inf above
    odd = np.array([[0.5, np.nan, 0.25], [0.5, 0.25, 0.25]], dtype)
    b = ctc.beam_search(odd, 8, 8, dtype=dtype)
    nan_at = np.isnan(b.probs[0])
    assert nan_at.any() and np.flatnonzero(b.probs[0] > 0).max() < np.flatnonzero(nan_at).min()
    odd[0, 1] = np.inf
    b = ctc.beam_search(odd, 8, 8, dtype=dtype)
    assert np.isposinf(b.probs[0, 0]) and B64.strings_of(b)[0][0][0] == 1


# ---- the library -------------------------------------------------------------------------------------------------------------------------
def test_the_librarys_host_function_carries_the_float32_statements_bits():
    from wwhip import ctc
    present = absent = 0
    for i, (steps, W, P, M) in enumerate(B64.random_tables(n=400)):
        got, want = ctc.beam_rows(steps, W, P, M), ctc.beam_search(steps, W, P, M, np.float32)
        B64.same_bits(got, want, f"table {i}: {steps.shape} W={W} P={P} M={M}")
        present += int((want.lengths >= 0).sum())
        absent += int((want.lengths < 0).sum())
    assert present > 400 and absent > 20
    # a batch is its rows
    y = B64.tables(np.random.default_rng(4), 9, 19, 4)
    whole = ctc.beam_rows(y, 8, 3, 5)
    for i in range(9):
        B64.same_bits(type(whole)(whole.labels[i:i + 1], whole.lengths[i:i + 1], whole.probs[i:i + 1]), ctc.beam_rows(y[i], 8, 3, 5))


def test_the_derived_bound_holds_where_float64_decides():
    """``csrc/ctc_beam.h``'s (3T + 2) 2^-24 on the host function, on tables whose pruning float64 decides."""
    from wwhip import ctc
    rng = np.random.default_rng(8)
    checked = 0
    for L, W in ((3, 4), (4, 8), (8, 64)):
        y = rng.dirichlet(np.full(L, 0.8), (40, 19)).astype(np.float32)
        trace = []
        want = ctc.beam_search(y, W, 4, trace=trace)
        ok = B64.decidable(trace, W, 4, ctc.beam_rel_bound(19))
        got = ctc.beam_rows(y, W, 4)
        np.testing.assert_array_equal(got.labels[ok], want.labels[ok])
        err = np.abs(got.probs[ok].astype(np.float64) - want.probs[ok])
        assert (err <= ctc.beam_rel_bound(19) * want.probs[ok] + 5 * 19 * 20 * 2.0 ** -126).all()
        checked += int(ok.sum())
    assert checked > 60


def test_header_binding_and_exports():
    from wwhip import _lib
    header = open(os.path.join(_ROOT, "include", "wwhip.h")).read()
    for name, n_args in FAMILY.items():
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert m, f"{name} is not declared in include/wwhip.h"
        assert name in _lib.SYMBOLS, f"{name} is not bound in wwhip/_lib.py"
        assert len(_lib.SYMBOLS[name][1]) == m.group(1).count(",") + 1 == n_args, name
    lib = _lib.load()
    for name in FAMILY:
        assert hasattr(lib, name), name
    for name, value in (("WW_CTC_BEAM_MAX_T", 19), ("WW_CTC_BEAM_MAX_WIDTH", 64), ("WW_CTC_BEAM_MAX_PATHS", 8)):
        assert re.search(rf"#define {name} {value}\b", header), name
    from wwhip import ctc
    assert (ctc.BEAM_MAX_T, ctc.BEAM_MAX_WIDTH, ctc.BEAM_MAX_PATHS) == (19, 64, 8)
    beam_h = open(os.path.join(_CSRC, "ctc_beam.h")).read()
    code = re.sub(r"//[^\n]*", "", beam_h)
    assert "hip/" not in code and "__global__" not in code
    assert "static_assert" in code and "ww_cs_add" in code and "ww_cs_mul" in code
    build = open(os.path.join(_ROOT, "wakeword-detection_amd", "wwhip", "_build.py")).read()
    assert '"ctc_beam.hip"' in build and '"ctc_beam.h"' in build


def test_refusals_name_the_rule_and_write_nothing():
    from wwhip import _lib, ctc
    lib = _lib.load()
    y = np.full((2, 19, 4), 0.25, np.float32)
    lab, ln, pr = np.full((2, 8, 19), -77, np.int32), np.full((2, 8), -77, np.int32), np.full((2, 8), -7.0, np.float32)
    cases = [(dict(T=0), "T = 0"), (dict(T=20), "T = 20"), (dict(L=1), "L = 1"), (dict(L=9), "L = 9"), (dict(W=0), "beam_width = 0"),
             (dict(W=65), "beam_width = 65"), (dict(P=0), "top_paths = 0"), (dict(P=9), "top_paths = 9"), (dict(W=3, P=4), "top_paths = 4"),
             (dict(M=0), "max_labels = 0"), (dict(M=20), "max_labels = 20"), (dict(n=-1), "negative"), (dict(lab=None), "NULL"), (dict(ln=None), "NULL"),
             (dict(pr=None), "NULL"), (dict(y=None), "NULL")]
    for kw, word in cases:
        a = dict(y=_lib.ptr(y), n=2, T=19, L=4, W=8, P=2, M=19, lab=_lib.ptr(lab), ln=_lib.ptr(ln), pr=_lib.ptr(pr))
        a.update(kw)
        rc = lib.ww_ctc_beam_rows(a["y"], a["n"], a["T"], a["L"], a["W"], a["P"], a["M"], a["lab"], a["ln"], a["pr"])
        text = (lib.ww_last_error(None) or b"").decode()
        assert rc == _lib.WW_EINVAL and word in text and "ww_ctc_beam_rows" in text, (kw, rc, text)
    assert (lab == -77).all() and (ln == -77).all() and (pr == -7.0).all()
    assert lib.ww_ctc_beam_rows(_lib.ptr(y), 0, 19, 4, 8, 2, 19, _lib.ptr(lab), _lib.ptr(ln), _lib.ptr(pr)) == _lib.WW_OK
    assert (lab == -77).all()
    for kw in (dict(beam_width=0), dict(beam_width=65), dict(beam_width=8, top_paths=9), dict(beam_width=2, top_paths=3), dict(beam_width=8, max_labels=20)):
        with pytest.raises(ValueError):
            ctc.beam_search(y, **kw)
        with pytest.raises(ValueError):
            ctc.beam_rows(y, **kw)
    with pytest.raises(ValueError, match="T = 20"):
        ctc.beam_search(np.full((20, 4), 0.25), 8)
    with pytest.raises(ValueError, match="L = 9"):
        ctc.beam_search(np.full((3, 9), 0.1), 8)
