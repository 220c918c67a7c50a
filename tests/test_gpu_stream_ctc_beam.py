"""The prefix beam search in CTC stream banks on the MI355X (``ww_stream_step_ctc_beam``): 40 ticks of tests/stream_ctc64.py's signal,
S = 3 - stream 1 toggles, stream 2 is frozen for a while, stream 1 is reset -, L = 4, in every form of the bank.  A tick's paths are
held to ``ww_ctc_beam_rows`` (the host function of csrc/ctc_beam.h) on the posteriors the same tick returns; those posteriors are
held to float64 by tests/test_gpu_stream_ctc.py."""
import os

import numpy as np
import pytest
from numpy.testing import assert_array_equal

import ctc64
import ctc_beam64 as B64
import stream_ctc64 as SC

pytestmark = pytest.mark.gpu

TICKS, S, L, M = 40, 3, 4, 9
W, P, BM = 8, 3, 5
SENT_I, SENT = -55, -7.0
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


def _raw_tick(bank, frames, flags, beam=True):
    """One tick through the library with sentinel-filled outputs."""
    from wwhip import _lib
    p = _lib.ptr
    labels, lengths = np.full((S, 2, M), SENT_I, np.int32), np.full((S, 2), SENT_I, np.int32)
    steps, n = np.full((S, 2, 19, L), SENT, np.float32), np.full(S, SENT_I, np.int32)
    bl, bn, bp = np.full((S, 2, P, BM), SENT_I, np.int32), np.full((S, 2, P), SENT_I, np.int32), np.full((S, 2, P), SENT, np.float32)
    frames, flags = np.ascontiguousarray(frames), np.ascontiguousarray(flags)
    if beam:
        rc = bank._lib.ww_stream_step_ctc_beam(bank._h, p(frames), p(flags), M, p(labels), p(lengths), p(steps), W, P, BM, p(bl), p(bn), p(bp), p(n))
    else:
        rc = bank._lib.ww_stream_step_ctc(bank._h, p(frames), p(flags), M, p(labels), p(lengths), p(steps), p(n))
    _lib.raise_for(rc, bank.engine.ctx.handle)
    return n, labels, lengths, steps, bl, bn, bp


def test_beam_is_the_host_function_on_the_ticks_own_steps_in_every_form(engine):
    from wwhip import ctc
    from wwhip.engine import CtcStreamBank
    e = engine
    x, flags = SC.pcm(), _flags()
    beamed = {k: CtcStreamBank(e, S, max_labels=M, want_steps=True, beam_width=W, top_paths=P, beam_max_labels=BM, **kw) for k, kw in FORMS.items()}
    plain = {k: CtcStreamBank(e, S, max_labels=M, want_steps=True, **kw) for k, kw in FORMS.items()}   # the parent's tick
    seen, windows = set(), 0
    try:
        for t in range(TICKS):
            if t == RESET_TICK:
                for b in list(beamed.values()) + list(plain.values()):
                    b.reset([1])
            got = {}
            for name in FORMS:
                n, labels, lengths, steps, bl, bn, bp = _raw_tick(beamed[name], x[t], flags[t])
                got[name] = (bl, bn, bp)
                pn, plabels, plengths, psteps, _, _, _ = _raw_tick(plain[name], x[t], flags[t], beam=False)
                # the tick itself is what it is without the beam
                assert_array_equal(n, pn, err_msg=f"{name} tick {t}")
                assert_array_equal(labels, plabels, err_msg=f"{name} tick {t}")
                assert_array_equal(lengths, plengths, err_msg=f"{name} tick {t}")
                assert_array_equal(steps.view(np.uint32), psteps.view(np.uint32), err_msg=f"{name} tick {t}")
                for s in range(S):
                    k = int(n[s])
                    seen.add(k)
                    assert (bl[s, k:] == SENT_I).all() and (bn[s, k:] == SENT_I).all() and (bp[s, k:] == SENT).all()
                    if not k:
                        continue
                    windows += k
                    want = ctc.beam_rows(steps[s, :k], W, P, BM)
                    B64.same_bits(ctc.CtcBeam(bl[s, :k], bn[s, :k], bp[s, :k]), want, f"{name} tick {t} stream {s}")
                    if name == "full recompute":
                        off = e.ctc_beam(beamed[name].window(s)[None], W, P, BM)
                        B64.same_bits(ctc.CtcBeam(bl[s, k - 1:k], bn[s, k - 1:k], bp[s, k - 1:k]), off, f"offline, tick {t} stream {s}")
            for name in ("two launches", "sync wait"):   # the incremental forms agree with one another bit for bit
                for a, b in zip(got["one launch"], got[name]):
                    assert_array_equal(a.view(np.uint32), b.view(np.uint32), err_msg=f"{name} tick {t}")
    finally:
        for b in list(beamed.values()) + list(plain.values()):
            b.close()
    assert seen == {0, 1, 2} and windows > 4 * 130


def test_python_tick_carries_the_beam(engine):
    from wwhip import ctc
    from wwhip.engine import CtcStreamBank
    e = engine
    x, flags = SC.pcm(), _flags()
    bank = CtcStreamBank(e, S, max_labels=2, beam_width=64, top_paths=8)   # (no want_steps: the bank keeps the posteriors for itself)
    twin = CtcStreamBank(e, S, max_labels=2, want_steps=True)
    try:
        for t in range(12):
            tick, ref = bank.step(x[t], flags[t] & 1, flags[t] >> 1), twin.step(x[t], flags[t] & 1, flags[t] >> 1)
            assert tick.steps is None and tick.scores is None and tick.spans is None
            assert tick.beam_labels.shape == (S, 2, 8, 19) and tick.beam_lengths.shape == (S, 2, 8) and tick.beam_probs.dtype == np.float32
            assert_array_equal(tick.n, ref.n)
            assert_array_equal(tick.labels, ref.labels)
            for s in range(S):
                k = int(tick.n[s])
                assert (tick.beam_labels[s, k:] == -1).all() and (tick.beam_lengths[s, k:] == -1).all() and (tick.beam_probs[s, k:] == 0).all()
                if k:
                    B64.same_bits(ctc.CtcBeam(tick.beam_labels[s, :k], tick.beam_lengths[s, :k], tick.beam_probs[s, :k]),
                                  ctc.beam_rows(ref.steps[s, :k], 64, 8))
        assert twin.step(x[12], flags[12] & 1).beam_labels is None
    finally:
        bank.close()
        twin.close()


def test_refusals_move_nothing(engine, assets):
    from wwhip import _lib
    from wwhip.engine import CtcStreamBank, Engine, StreamBank
    e = engine
    lib, p = _lib.load(), _lib.ptr
    x = SC.pcm()
    with pytest.raises(ValueError, match="targets"):
        CtcStreamBank(e, S, targets=[(1, 2)], beam_width=8)
    for kw in (dict(beam_width=0), dict(beam_width=65), dict(beam_width=8, top_paths=9), dict(beam_width=2, top_paths=3), dict(beam_width=8, beam_max_labels=20)):
        with pytest.raises(ValueError):
            CtcStreamBank(e, S, **kw)
    labels_only = CtcStreamBank(e, S, max_labels=M)
    ready, twin = CtcStreamBank(e, S, max_labels=M, want_steps=True), CtcStreamBank(e, S, max_labels=M, want_steps=True)
    shipped = Engine(os.path.join(assets, "CRNN"))
    plain = StreamBank(shipped, S)
    err = lambda eng: lib.ww_last_error(eng.ctx.handle).decode()
    try:
        ones = np.ones(S, np.uint8)
        labels, lengths, n = np.full((S, 2, M), SENT_I, np.int32), np.full((S, 2), SENT_I, np.int32), np.full(S, SENT_I, np.int32)
        bl, bn, bp = np.full((S, 2, 8, 19), SENT_I, np.int32), np.full((S, 2, 8), SENT_I, np.int32), np.full((S, 2, 8), SENT, np.float32)

        def call(bank, w=W, pp=P, m=BM, a=bl, b=bn, c=bp, t=0):
            frames = np.ascontiguousarray(x[t])
            return lib.ww_stream_step_ctc_beam(bank._h, p(frames), p(ones), M, p(labels), p(lengths), None, w, pp, m, None if a is None else p(a),
                                               None if b is None else p(b), None if c is None else p(c), p(n))

        for bank, eng, word in ((labels_only, e, "WW_STREAM_CTC_STEPS"), (plain, shipped, "ww_stream_create_ctc")):
            assert call(bank) == _lib.WW_EINVAL and "ww_stream_step_ctc_beam" in err(eng) and word in err(eng), err(eng)
        for kw, word in ((dict(w=0), "beam_width"), (dict(w=65), "beam_width"), (dict(pp=9), "top_paths"), (dict(w=2, pp=3), "top_paths"), (dict(m=0), "max_labels"),
                         (dict(m=20), "max_labels"), (dict(a=None), "NULL"), (dict(b=None), "NULL"), (dict(c=None), "NULL")):
            assert call(ready, **kw) == _lib.WW_EINVAL and word in err(e), (kw, err(e))
        assert (labels == SENT_I).all() and (lengths == SENT_I).all() and (n == SENT_I).all()
        assert (bl == SENT_I).all() and (bn == SENT_I).all() and (bp == SENT).all()
        # nothing moved: the bank ticks with its twin's bits, with the beam on one tick and without it on the next
        for t in range(8):
            want = twin.step(x[t], ones)
            if t % 2:
                assert call(ready, t=t) == 0
                assert_array_equal(n, want.n)
            else:
                got = ready.step(x[t], ones)
                assert_array_equal(got.n, want.n)
                assert_array_equal(got.labels, want.labels)
                assert_array_equal(got.steps, want.steps)
                assert got.beam_labels is None
    finally:
        for b in (labels_only, ready, twin, plain):
            b.close()
        shipped.close()
