"""The Viterbi alignment in CTC stream banks on the MI355X (``ww_stream_step_ctc_align``): 40 ticks of tests/stream_ctc64.py's signal,
S = 3 - stream 1 toggles, stream 2 is frozen for a while, stream 1 is reset -, L = 4, the targets (1, 2) and (1,), both modes, in
every form of the bank.  A tick's alignment is held to ``ww_ctc_align_rows`` (the host function of csrc/ctc_align.h) on the
posteriors the same tick returns; those posteriors are held to float64 by tests/test_gpu_stream_ctc.py."""
import os

import numpy as np
import pytest
from numpy.testing import assert_array_equal

import ctc64
import ctc_align64 as A64
import stream_ctc64 as SC

pytestmark = pytest.mark.gpu

TICKS, S, L, M = 40, 3, 4, 9
TARGETS = [(1, 2), (1,)]
K = len(TARGETS)
SENT, SENT_B = -7.0, 0x55
RESET_TICK = 30
FORMS = {"one launch": {}, "two launches": dict(two_launch=True), "sync wait": dict(sync_wait=True), "full recompute": dict(full_recompute=True)}


def _flags():
    """``[TICKS, S]`` uint8, bit 0 speech, bit 1 active: stream 1 silent on ticks 12..17 and on every third tick from 33, stream 2
    frozen on ticks 20..27."""
    f = np.ones((TICKS, S), np.uint8)
    t = np.arange(TICKS)
    f[:, 1] = ~(((t >= 12) & (t < 18)) | ((t >= 33) & (t % 3 == 0))) & 1
    f[20:28, 2] |= 2
    return f


@pytest.fixture(scope="module")
def engine():
    from wwhip.engine import Engine
    e = Engine("synthetic-ctc-4", bundle=ctc64.model(L))
    yield e
    e.close()


def _rows_host(steps, mode):
    """``ww_ctc_align_rows`` on ``[n, 19, L]`` -> ``(value [n, K], span [n, K, 9, 2] int8)``: a tick's layout."""
    from wwhip import _lib, ctc
    y = np.ascontiguousarray(steps, np.float32)
    tab, lens = ctc.pack_targets(TARGETS, L)
    value, span = np.empty((K, len(y)), np.float32), np.empty((K, len(y), 9, 2), np.int8)
    assert _lib.load().ww_ctc_align_rows(_lib.ptr(y), len(y), 19, L, _lib.ptr(tab), _lib.ptr(lens), K, ctc.score_mode(mode), _lib.ptr(value),
                                         _lib.ptr(span)) == 0
    return np.ascontiguousarray(value.T), np.ascontiguousarray(span.transpose(1, 0, 2, 3))


def _raw_tick(bank, frames, flags, call="align"):
    """One tick through the library with sentinel-filled outputs -> ``(n, labels, lengths, steps, scores, align_value, align_span)``."""
    from wwhip import _lib
    p = _lib.ptr
    labels, lengths = np.full((S, 2, M), -55, np.int32), np.full((S, 2), -55, np.int32)
    steps, scores, n = np.full((S, 2, 19, L), SENT, np.float32), np.full((S, 2, K), SENT, np.float32), np.full(S, -55, np.int32)
    value, span = np.full((S, 2, K), SENT, np.float32), np.full((S, 2, K, 9, 2), SENT_B, np.int8)
    frames, flags = np.ascontiguousarray(frames), np.ascontiguousarray(flags)
    if call == "align":
        rc = bank._lib.ww_stream_step_ctc_align(bank._h, p(frames), p(flags), M, p(labels), p(lengths), p(steps), p(scores), p(value), p(span), p(n))
    else:
        rc = bank._lib.ww_stream_step_ctc_score(bank._h, p(frames), p(flags), M, p(labels), p(lengths), p(steps), p(scores), p(n))
    _lib.raise_for(rc, bank.engine.ctx.handle)
    return n, labels, lengths, steps, scores, value, span


@pytest.mark.parametrize("mode", A64.MODES)
def test_alignment_is_the_host_function_on_the_ticks_own_steps_in_every_form(engine, mode):
    from wwhip.engine import CtcStreamBank
    e = engine
    x, flags = SC.pcm(), _flags()
    aligned = {k: CtcStreamBank(e, S, max_labels=M, want_steps=True, targets=TARGETS, mode=mode, align=True, **kw) for k, kw in FORMS.items()}
    scored = {k: CtcStreamBank(e, S, max_labels=M, want_steps=True, targets=TARGETS, mode=mode, **kw) for k, kw in FORMS.items()}   # the parent's tick
    seen, windows, paths = set(), 0, 0
    try:
        for t in range(TICKS):
            if t == RESET_TICK:
                for b in list(aligned.values()) + list(scored.values()):
                    b.reset([1])
            got = {}
            for name in FORMS:
                n, labels, lengths, steps, scores, value, span = _raw_tick(aligned[name], x[t], flags[t])
                got[name] = (value, span)
                pn, plabels, plengths, psteps, pscores, _, _ = _raw_tick(scored[name], x[t], flags[t], call="score")
                # the tick itself, scores included, is what it is without the alignment
                assert_array_equal(n, pn, err_msg=f"{name} tick {t}")
                assert_array_equal(labels, plabels, err_msg=f"{name} tick {t}")
                assert_array_equal(lengths, plengths, err_msg=f"{name} tick {t}")
                assert_array_equal(steps.view(np.uint32), psteps.view(np.uint32), err_msg=f"{name} tick {t}")
                assert_array_equal(scores.view(np.uint32), pscores.view(np.uint32), err_msg=f"{name} tick {t}")
                for s in range(S):
                    k = int(n[s])
                    seen.add(k)
                    assert (value[s, k:] == SENT).all() and (span[s, k:] == SENT_B).all() and (scores[s, k:] == SENT).all()
                    if not k:
                        continue
                    windows += k
                    wv, ws = _rows_host(steps[s, :k], mode)
                    assert_array_equal(value[s, :k].view(np.uint32), wv.view(np.uint32), err_msg=f"{name} tick {t} stream {s}")
                    assert_array_equal(span[s, :k], ws, err_msg=f"{name} tick {t} stream {s}")
                    paths += int((wv != 0).sum())
                    if name == "full recompute":
                        off = e.ctc_align(aligned[name].window(s)[None], TARGETS, mode)
                        assert_array_equal(value[s, k - 1].view(np.uint32), off.value[:, 0].view(np.uint32))
                        assert_array_equal(span[s, k - 1, :, :2], off.span[:, 0])
                        assert (span[s, k - 1, :, 2:] == -1).all()
            # the incremental forms agree with one another bit for bit
            for name in ("two launches", "sync wait"):
                assert_array_equal(got["one launch"][0].view(np.uint32), got[name][0].view(np.uint32), err_msg=f"{name} tick {t}")
                assert_array_equal(got["one launch"][1], got[name][1], err_msg=f"{name} tick {t}")
    finally:
        for b in list(aligned.values()) + list(scored.values()):
            b.close()
    assert seen == {0, 1, 2} and windows > 4 * 130 and paths > windows


def test_python_tick_carries_the_alignment(engine):
    from wwhip.engine import CtcStreamBank
    e = engine
    x, flags = SC.pcm(), _flags()
    bank = CtcStreamBank(e, S, max_labels=2, want_steps=True, targets=TARGETS, mode="prefix", align=True)
    try:
        for t in range(12):
            tick = bank.step(x[t], flags[t] & 1, flags[t] >> 1)
            assert tick.align_values.shape == (S, 2, K) and tick.align_values.dtype == np.float32
            assert tick.spans.shape == (S, 2, K, 2, 2) and tick.spans.dtype == np.int32
            for s in range(S):
                k = int(tick.n[s])
                assert (tick.align_values[s, k:] == 0).all() and (tick.spans[s, k:] == -1).all()
                if k:
                    wv, ws = _rows_host(tick.steps[s, :k], "prefix")
                    assert_array_equal(tick.align_values[s, :k], wv)
                    assert_array_equal(tick.spans[s, :k], ws[:, :, :2])
        with pytest.raises(ValueError, match="targets"):
            CtcStreamBank(e, S, align=True)
    finally:
        bank.close()


def test_the_wake_word_stage_records_where_the_word_lay(engine):
    """``CtcWakewordBank(align=True)``: on a fire, ``wake_span_rows`` is the fired target's span on the window that fired, in rows of
    the stream - here by hand: conv step t reads rows 8 t - 6 .. 8 t + 13 of the window (clipped to 0 .. 150), and the window whose
    newest row is the stream's row r starts at row r - 150."""
    from wwhip.context import ContextBank
    from wwhip.engine import CtcStreamBank
    from wwhip.wakeword import CtcWakewordBank
    e = engine
    x, flags = SC.pcm(), _flags()
    sp = flags & 1
    probe = CtcStreamBank(e, S, max_labels=2, targets=TARGETS, mode="prefix")
    try:
        seen = [probe.step(x[t], sp[t]) for t in range(TICKS)]
    finally:
        probe.close()
    all_scores = np.concatenate([tk.scores[s, :tk.n[s]] for tk in seen for s in range(S) if tk.n[s]])
    thr = np.quantile(all_scores.astype(np.float64), 0.5, axis=0)
    ctxs = ContextBank(S)
    with pytest.raises(ValueError, match="thresholds"):
        CtcWakewordBank(S, engine=e, align=True)
    plain = CtcStreamBank(e, S, max_labels=2, targets=TARGETS, mode="prefix")
    try:
        with pytest.raises(ValueError, match="align"):
            CtcWakewordBank(S, bank=plain, thresholds=thr, align=True)
    finally:
        plain.close()
    bank = CtcStreamBank(e, S, max_labels=2, targets=TARGETS, mode="prefix", align=True)
    stage = CtcWakewordBank(S, bank=bank, thresholds=thr, align=True)
    delivered, was, fired = [0] * S, [0] * S, []
    try:
        assert all(stage.wake_span_rows(s) == (-1, -1) for s in range(S))
        for t in range(TICKS):
            if t in (15, 31):
                ctxs.is_active[:] = 0
            ctxs.is_speech[:] = sp[t]
            tick = stage(ctxs, x[t])
            for s, j in zip(stage.fired_ids.tolist(), stage.fired_slots.tolist()):
                k = [any(float(tick.scores[s, k, i]) > thr[i] for i in range(K)) for k in range(int(tick.n[s]))].index(True)
                newest = delivered[s] + k                      # the stream's row count at the window that fired
                first_step, last_step = int(tick.spans[s, k, j, 0, 0]), int(tick.spans[s, k, j, len(TARGETS[j]) - 1, 1])
                assert tick.align_values[s, k, j] > 0 and 0 <= first_step <= last_step <= 18
                want = (newest - 150 + max(0, 8 * first_step - 6), newest - 150 + min(150, 8 * last_step + 13))
                assert stage.wake_span_rows(s) == want, (t, s, j, stage.wake_span_rows(s), want)
                fired.append((t, s, j) + want)
            for s in range(S):
                delivered[s] += int(tick.n[s])
                if was[s] and not sp[t, s]:
                    delivered[s] = 0                           # (the stage reset the stream)
                was[s] = int(sp[t, s])
    finally:
        stage.close()
    print(f"\nfired (tick, stream, slot, first row, last row): {fired}", end="")
    assert len({f[1] for f in fired}) >= 2 and len(fired) > 2


def test_refusals_move_nothing(engine, assets):
    from wwhip import _lib
    from wwhip.engine import CtcStreamBank, Engine, StreamBank
    e = engine
    lib, p = _lib.load(), _lib.ptr
    x = SC.pcm()
    labels_only, no_targets = CtcStreamBank(e, S, max_labels=M), CtcStreamBank(e, S, max_labels=M, want_steps=True)
    ready = CtcStreamBank(e, S, max_labels=M, targets=TARGETS)
    twin = CtcStreamBank(e, S, max_labels=M, targets=TARGETS)
    shipped = Engine(os.path.join(assets, "CRNN"))
    plain = StreamBank(shipped, S)
    err = lambda eng: lib.ww_last_error(eng.ctx.handle).decode()
    try:
        ones = np.ones(S, np.uint8)
        labels, lengths = np.full((S, 2, M), -55, np.int32), np.full((S, 2), -55, np.int32)
        scores, n = np.full((S, 2, K), SENT, np.float32), np.full(S, -55, np.int32)
        value, span = np.full((S, 2, K), SENT, np.float32), np.full((S, 2, K, 9, 2), SENT_B, np.int8)

        def call(bank, sc=scores, v=value, sn=span, t=0):
            frames = np.ascontiguousarray(x[t])
            return lib.ww_stream_step_ctc_align(bank._h, p(frames), p(ones), M, p(labels), p(lengths), None, None if sc is None else p(sc),
                                                None if v is None else p(v), None if sn is None else p(sn), p(n))

        for bank, eng, word in ((labels_only, e, "WW_STREAM_CTC_STEPS"), (no_targets, e, "no targets"), (plain, shipped, "ww_stream_create_ctc")):
            assert call(bank) == _lib.WW_EINVAL and "ww_stream_step_ctc_align" in err(eng) and word in err(eng), err(eng)
        for kw in (dict(sc=None), dict(v=None), dict(sn=None)):
            assert call(ready, **kw) == _lib.WW_EINVAL and "NULL" in err(e)
        assert (labels == -55).all() and (lengths == -55).all() and (scores == SENT).all() and (n == -55).all()
        assert (value == SENT).all() and (span == SENT_B).all()
        # nothing moved: the bank ticks with its twin's bits, and the other calls of a bank that has aligned are what they were
        for t in range(8):
            if t % 2:
                assert call(ready, t=t) == 0
                got_n, got_scores = n.copy(), scores.copy()
                want = twin.step(x[t], ones)
                assert_array_equal(got_n, want.n)
                for s in range(S):
                    assert_array_equal(got_scores[s, :want.n[s]], want.scores[s, :want.n[s]])
            else:
                got, want = ready.step(x[t], ones), twin.step(x[t], ones)
                assert_array_equal(got.n, want.n)
                assert_array_equal(got.labels, want.labels)
                assert_array_equal(got.scores, want.scores)
                assert got.spans is None
    finally:
        for b in (labels_only, no_targets, ready, twin, plain):
            b.close()
        shipped.close()
