"""CTC stream banks on the MI355X (``ww_stream_create_ctc``, ``ww_stream_step_ctc``, ``ww_stream_step_ctc_trigger``): the script of
tests/stream_ctc64.py - 170 ticks, S = 3, a toggling and a frozen stream, a reset, the 144-slot cache wrapped twice - through the
incremental kernel's CTC form in every launch form and through the full-recompute form, against float64 (``Ctc64`` over the bank's own
windows), against the numpy decode - exactly -, against one another - bit for bit - and against the offline path.

Bounds: ``ctc64.TAU``, the project's constant for these recurrences (tests/test_gpu_ref64.py), not a new one; the needed values are
printed (``pytest -s``).  tests/test_stream_ctc_host.py asserts on the float64 reference alone what these tests rely on."""
import ctypes as C
import os

import numpy as np
import pytest
from numpy.testing import assert_array_equal

import ctc64
import stream_ctc64 as SC
from oracle import ref64 as R

pytestmark = pytest.mark.gpu

TAU = ctc64.TAU
M = 9   # WW_STREAM_CTC_MAX_LABELS


def _engine(L):
    from wwhip.engine import Engine
    return Engine(f"synthetic-ctc-{L}", bundle=ctc64.model(L))


def _play(banks, on_tick=None):
    """The script through every bank of ``banks`` in lock step -> {name: [CtcTick per tick]}."""
    x, sp, act = SC.pcm(), SC.speech(), SC.active()
    out = {k: [] for k in banks}
    for t in range(SC.TICKS):
        if t == SC.RESET_TICK:
            for b in banks.values():
                b.reset(list(SC.RESET_IDS))
        for k, b in banks.items():
            out[k].append(b.step(x[t], sp[t], act[t]))
        if on_tick is not None:
            on_tick(t, {k: v[-1] for k, v in out.items()})
    return out


class Run:
    """One model's run: a ``want_steps`` bank in the default form, a ``want_steps`` full-recompute bank and two label-only banks
    (``max_labels`` 1 and 2) over the whole script; at the sampled ticks the newest window of each stream that delivered one, with its
    float64 posteriors and the offline path's outputs, each computed once."""

    def __init__(self, L):
        from wwhip.engine import CtcStreamBank
        self.L = L
        self.engine = e = _engine(L)
        banks = {"steps": CtcStreamBank(e, SC.S, max_labels=M, want_steps=True),
                 "full": CtcStreamBank(e, SC.S, max_labels=M, want_steps=True, full_recompute=True),
                 "m1": CtcStreamBank(e, SC.S, max_labels=1), "m2": CtcStreamBank(e, SC.S)}
        self.keys, wins = [], []

        def sample(t, ticks):
            if not SC.sampled(t):
                return
            for s in range(SC.S):
                n = int(ticks["steps"].n[s])
                if n:
                    w = banks["steps"].window(s)
                    assert_array_equal(w, banks["full"].window(s))
                    self.keys.append((t, s, n - 1))
                    wins.append(w)
        try:
            self.ticks = _play(banks, sample)
        finally:
            for b in banks.values():
                b.close()
        self.windows = np.stack(wins)
        self.steps64, _ = ctc64.Ctc64(ctc64.model(L).crnn).sequence(self.windows)
        self.offline = e.ctc_forward(self.windows, max_labels=M, want=("labels", "steps"))

    def sampled(self, name):
        """``(steps [n, 19, L], labels [n, 9], lengths [n])`` of bank ``name`` at the sampled windows."""
        tk = self.ticks[name]
        return (np.stack([tk[t].steps[s, k] for t, s, k in self.keys]), np.stack([tk[t].labels[s, k] for t, s, k in self.keys]),
                np.array([tk[t].lengths[s, k] for t, s, k in self.keys]))

    def close(self):
        self.engine.close()


@pytest.fixture(scope="module")
def runs():
    cache = {}

    def get(L):
        if L not in cache:
            cache[L] = Run(L)
        return cache[L]
    yield get
    for r in cache.values():
        r.close()


# ---- 1: against float64 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", ctc64.LS)
def test_posteriors_against_float64(runs, L):
    r = runs(L)
    n64, _ = SC.play()
    for t in range(SC.TICKS):   # the framing: every bank delivers the windows the reference's rule gives
        for name in r.ticks:
            assert_array_equal(r.ticks[name][t].n, n64[t], err_msg=f"{name} tick {t}")
    assert r.keys == SC.sample_keys() and len(r.keys) > 80
    for name in ("steps", "full"):
        got = r.sampled(name)[0]
        assert got.shape == r.steps64.shape and np.isfinite(got).all() and got.min() >= 0.0 and got.max() <= 1.0
        print(f"\nCTC stream bank L={L} {name}: posteriors need tau {R.needed_tau(got.reshape(-1, L), r.steps64.reshape(-1, L)):.2e} "
              f"(tau {TAU:g}), max|dp| {np.abs(got - r.steps64).max():.2e}", end="")
        R.check_posteriors(got.reshape(-1, L), r.steps64.reshape(-1, L), TAU)
        np.testing.assert_allclose(got.sum(axis=2), 1.0, atol=4e-7)


# ---- 2: the decode, exactly ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", ctc64.LS)
def test_decode_is_the_numpy_statement_of_the_ticks_own_steps(runs, L):
    from wwhip import ctc
    r = runs(L)
    cut = {1: False, 2: False, M: False}
    for t in range(SC.TICKS):
        ref = r.ticks["steps"][t]
        for name, m in (("steps", M), ("full", M), ("m2", 2), ("m1", 1)):
            tk = r.ticks[name][t]
            own = tk.steps if tk.steps is not None else ref.steps   # (the label-only banks carry the bits of the steps bank: test 4)
            for s in range(SC.S):
                n = int(tk.n[s])
                assert tk.labels.shape == (SC.S, 2, m)
                if n:
                    labels, lengths = ctc.greedy_decode(own[s, :n], m)
                    assert_array_equal(tk.labels[s, :n], labels, err_msg=f"{name} tick {t} stream {s}")
                    assert_array_equal(tk.lengths[s, :n], lengths, err_msg=f"{name} tick {t} stream {s}")
                    cut[m] |= bool((lengths > m).any())
                assert (tk.labels[s, n:] == -1).all() and (tk.lengths[s, n:] == 0).all()
    assert cut[1] and cut[2]   # strings longer than max_labels were seen, and reported their whole length


# ---- 3: against the reference's decode ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", ctc64.LS)
def test_labels_equal_the_float64_decode_where_it_is_decidable(runs, L):
    r = runs(L)
    dec = ctc64.decidable(r.steps64)
    labels64, lengths64 = ctc64.decode64(r.steps64, M)
    assert (~dec).sum() <= 0.10 * len(dec), (L, int((~dec).sum()))
    for name in ("steps", "full"):
        _, labels, lengths = r.sampled(name)
        assert_array_equal(labels[dec], labels64[dec], err_msg=name)
        assert_array_equal(lengths[dec], lengths64[dec], err_msg=name)
    assert (lengths64[dec] == 0).any() and (lengths64[dec] >= 2).any()


# ---- 4: the forms, bit for bit -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precise", [True, False])
def test_forms_are_bit_identical(precise):
    from wwhip.engine import CtcStreamBank, frontend_params
    e = _engine(4)
    kw = {"one launch polled": {}, "two launches waited": dict(two_launch=True, sync_wait=True), "one launch waited": dict(sync_wait=True),
          "two launches polled": dict(two_launch=True), "steps, one launch": dict(want_steps=True),
          "steps, two launches": dict(want_steps=True, two_launch=True)}
    banks = {k: CtcStreamBank(e, SC.S, frontend_params(precise=precise), max_labels=M, **v) for k, v in kw.items()}
    try:
        ticks = _play(banks)
    finally:
        for b in banks.values():
            b.close()
        e.close()
    ref = ticks["steps, one launch"]
    seen = set()
    for name, tk in ticks.items():
        for t in range(SC.TICKS):
            assert_array_equal(tk[t].n, ref[t].n, err_msg=f"{name} tick {t}")
            assert_array_equal(tk[t].labels, ref[t].labels, err_msg=f"{name} tick {t}")
            assert_array_equal(tk[t].lengths, ref[t].lengths, err_msg=f"{name} tick {t}")
            if tk[t].steps is not None:
                assert_array_equal(tk[t].steps.view(np.uint32), ref[t].steps.view(np.uint32), err_msg=f"{name} tick {t}")
            seen.update(int(v) for v in tk[t].n)
    assert seen == {0, 1, 2} and sum(int(tk.n.sum()) for tk in ref) > 800


# ---- 5: the tie to the offline path -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", ctc64.LS)
def test_full_recompute_carries_the_offline_paths_bits(runs, L):
    r = runs(L)
    steps, labels, lengths = r.sampled("full")
    assert_array_equal(steps.view(np.uint32), r.offline.steps.view(np.uint32))
    assert_array_equal(labels, r.offline.labels)
    assert_array_equal(lengths, r.offline.lengths)
    # the incremental bank: the bound of test 1 (it is held there), labels equal where decidable; the two banks' distance is printed
    inc_steps, inc_labels, inc_lengths = r.sampled("steps")
    dec = ctc64.decidable(r.steps64)
    assert_array_equal(inc_labels[dec], r.offline.labels[dec])
    assert_array_equal(inc_lengths[dec], r.offline.lengths[dec])
    print(f"\nCTC stream bank L={L}: max |incremental - full recompute| over {len(r.keys)} windows {np.abs(inc_steps - steps).max():.2e}", end="")


# ---- 6: untouched rows ---------------------------------------------------------------------------------------------------------------------
def test_entries_past_n_post_are_left_as_they_were():
    from wwhip import _lib
    from wwhip.engine import CtcStreamBank
    e = _engine(4)
    x, S, L = SC.pcm(), SC.S, 4
    seen = set()
    for kw in (dict(want_steps=True), dict(want_steps=True, full_recompute=True), dict()):
        bank = CtcStreamBank(e, S, max_labels=3, **kw)
        try:
            for t in range(8):
                labels, lengths = np.full((S, 2, 3), -55, np.int32), np.full((S, 2), -55, np.int32)
                steps = np.full((S, 2, 19, L), -7.0, np.float32) if kw else None
                n = np.full(S, -55, np.int32)
                flags = np.array([1, t % 2, 1 if t != 5 else 3], np.uint8)   # stream 1 analysed every other tick, stream 2 frozen once
                rc = bank._lib.ww_stream_step_ctc(bank._h, _lib.ptr(np.ascontiguousarray(x[t])), _lib.ptr(flags), 3, _lib.ptr(labels),
                                                  _lib.ptr(lengths), _lib.ptr(steps), _lib.ptr(n))
                assert rc == 0
                for s in range(S):
                    k = int(n[s])
                    assert 0 <= k <= 2
                    seen.add(k)
                    assert (labels[s, k:] == -55).all() and (lengths[s, k:] == -55).all() and (lengths[s, :k] >= 0).all()
                    if steps is not None:
                        assert (steps[s, k:] == -7.0).all() and (steps[s, :k] >= 0.0).all()
        finally:
            bank.close()
    e.close()
    assert seen == {0, 1, 2}


# ---- 7: other input -----------------------------------------------------------------------------------------------------------------------
def _same_ticks(got, want, what):
    assert_array_equal(got.n, want.n, err_msg=str(what))
    assert_array_equal(got.labels, want.labels, err_msg=str(what))
    assert_array_equal(got.lengths, want.lengths, err_msg=str(what))
    assert_array_equal(got.steps.view(np.uint32), want.steps.view(np.uint32), err_msg=str(what))


def test_mulaw_bank_at_8000_equals_the_16k_bank_given_the_resampled_signal():
    """One 8 kHz mu-law bank, S = 2, 60 ticks: the ticks of a 16 kHz CTC bank fed z = D zeros, then the resampler's one-shot int16
    output for the decoded samples (``ww_stream_attach_resampler``'s rule; tests/stream_rate_pairs.py states it)."""
    from stream_rate_pairs import resampler, z_of
    from wwhip import g711
    from wwhip.engine import CtcStreamBank
    e = _engine(4)
    S, ticks, F = 2, 60, 160
    rng = np.random.default_rng(81)
    codes = rng.integers(0, 256, (S, ticks * F)).astype(np.uint8)
    codes[:, 20 * F:30 * F] = 0xFF   # (half a second of mu-law silence)
    table = g711.table("mulaw")
    rs = resampler(8000, e.ctx)
    z = np.stack([z_of(rs, table[codes[s]]) for s in range(S)])
    assert z.shape == (S, ticks * 320)
    bank, ref = CtcStreamBank(e, S, max_labels=M, want_steps=True, sample_rate=8000, sample_format="mulaw"), CtcStreamBank(e, S, max_labels=M, want_steps=True)
    try:
        assert bank.sample_formats == ["mulaw"] * S and bank.frame_bytes.tolist() == [F] * S
        ones, seen = np.ones(S, np.uint8), 0
        for t in range(ticks):
            got, want = bank.step(codes[:, t * F:(t + 1) * F], ones), ref.step(z[:, t * 320:(t + 1) * 320], ones)
            _same_ticks(got, want, ("tick", t))
            seen += int(got.n.sum())
        assert seen >= S * (2 * ticks - 5)
        for s in range(S):
            assert_array_equal(bank.window(s), ref.window(s))
    finally:
        bank.close()
        ref.close()
        e.close()


def test_per_stream_rates_give_the_bits_of_a_bank_at_that_rate_alone():
    from wwhip.engine import CtcStreamBank
    e = _engine(4)
    ticks, rates = 30, [8000, 48000]
    rng = np.random.default_rng(82)
    x = [np.clip(rng.normal(0, 3000, ticks * r // 50), -32768, 32767).astype(np.int16) for r in rates]
    bank = CtcStreamBank(e, 2, max_labels=M, want_steps=True, sample_rate=rates)
    alone = [CtcStreamBank(e, 1, max_labels=M, want_steps=True, sample_rate=r) for r in rates]
    try:
        assert bank.sample_rates.tolist() == rates and bank.frame_samples.tolist() == [160, 960]
        one = np.ones(1, np.uint8)
        for t in range(ticks):
            got = bank.step([x[i][t * r // 50:(t + 1) * r // 50] for i, r in enumerate(rates)], np.ones(2, np.uint8))
            for i, r in enumerate(rates):
                want = alone[i].step(x[i][None, t * r // 50:(t + 1) * r // 50], one)
                assert got.n[i] == want.n[0], (t, i)
                assert_array_equal(got.labels[i], want.labels[0])
                assert_array_equal(got.lengths[i], want.lengths[0])
                assert_array_equal(got.steps[i].view(np.uint32), want.steps[0].view(np.uint32))
        bank.set_rate([0], 48000)
        assert bank.sample_rates.tolist() == [48000, 48000]
    finally:
        bank.close()
        for b in alone:
            b.close()
        e.close()


# ---- 8: the stage ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [4, 8])
def test_the_wake_word_stage_is_the_rule_over_the_banks_own_labels(L):
    from wwhip import ctc
    from wwhip.context import ContextBank
    from wwhip.engine import CtcStreamBank
    from wwhip.wakeword import CtcWakewordBank
    e = _engine(L)
    tgt = SC.target(L)
    x, sp, S = SC.pcm(), SC.speech(), SC.S
    ctxs = ContextBank(S)
    events, woke = [], []
    ctxs.add_handler("activate", lambda view: events.append(int(np.flatnonzero([view is ctxs[s] for s in range(S)])[0])))
    bank = CtcStreamBank(e, S, max_labels=3)
    stage = CtcWakewordBank(S, bank=bank, target=tgt, on_wake=lambda ids: woke.extend(int(i) for i in ids))
    active, was, fired_all, per_release = [0] * S, [0] * S, [], []
    try:
        for t in range(SC.TICKS):
            if t in SC.STAGE_RELEASE:
                ctxs.is_active[:] = 0
                active = [0] * S
                per_release.append([])
            ctxs.is_speech[:] = sp[t]
            n_events = len(events)
            tick = stage(ctxs, x[t])
            want_fired, want_fall = [], []
            for s in range(S):
                n = int(tick.n[s])
                assert n == 0 or (sp[t, s] and not active[s])   # an active stream is not sampled, a silent one not analysed
                hit = n > 0 and bool(ctc.is_wakeword(tick.labels[s, :n], tick.lengths[s, :n], tgt).any())
                if hit and not active[s]:
                    active[s] = 1
                    want_fired.append(s)
                if was[s] and not sp[t, s]:
                    want_fall.append(s)
                was[s] = int(sp[t, s])
            assert stage.fired_ids.tolist() == want_fired and events[n_events:] == want_fired, (t, stage.fired_ids, want_fired)
            assert stage.fall_ids.tolist() == want_fall, (t, stage.fall_ids, want_fall)
            assert ctxs.is_active.tolist() == active
            for s in want_fall:   # the streams whose speech bit fell were reset: an all-zero window
                assert not bank.window(s).any(), (t, s)
            fired_all += want_fired
            if per_release:
                per_release[-1] += want_fired
    finally:
        stage.close()
        e.close()
    assert woke == fired_all and len(set(fired_all)) >= 2, fired_all
    for ids in per_release:   # an active stream does not fire again
        assert len(ids) == len(set(ids))
    assert len(fired_all) > len(set(fired_all))   # ... and a released one does


# ---- 9: refusals both ways, sentinels untouched ------------------------------------------------------------------------------------------------
def test_refusals_name_the_family_and_move_nothing(assets):
    from wwhip import _lib
    from wwhip.engine import CtcStreamBank, Engine, StreamBank, frontend_params
    lib = _lib.load()
    e, shipped = _engine(4), Engine(os.path.join(assets, "CRNN"))
    S, x = SC.S, SC.pcm()
    bank, twin = CtcStreamBank(e, S, max_labels=M), CtcStreamBank(e, S, max_labels=M)
    plain = StreamBank(shipped, S)
    ones = np.ones(S, np.uint8)

    def err(eng):
        return lib.ww_last_error(eng.ctx.handle).decode()
    try:
        for t in range(6):
            _same = (bank.step(x[t], ones), twin.step(x[t], ones))
            assert_array_equal(_same[0].labels, _same[1].labels)
        p = _lib.ptr
        frames = np.ascontiguousarray(x[6])
        post, n = np.full((S, 2), -7.0, np.float32), np.full(S, -55, np.int32)
        act, was, pmax = np.zeros(S, np.uint8), np.zeros(S, np.uint8), np.full(S, -7.0, np.float32)
        ids, cnt = np.full(S, -55, np.int32), np.full(4, -55, np.int32)
        thr = np.full(1, 0.5)
        offs, rows = np.array([0, 320], np.int64), np.full(2, -55, np.int64)
        one = np.zeros(1, np.int32)
        ps = _lib.PipelineState()
        ps.n_fired = -55
        calls = {
            "ww_stream_step": lambda: lib.ww_stream_step(bank._h, p(frames), p(ones), p(post), p(n)),
            "ww_stream_step_all": lambda: lib.ww_stream_step_all(bank._h, p(frames), p(ones), p(post), p(n)),
            "ww_stream_step_trigger": lambda: lib.ww_stream_step_trigger(bank._h, p(frames), p(ones), p(act), 0.5, p(was), p(pmax), p(post), p(n), p(ids),
                                                                         p(cnt[0:1]), p(ids), p(cnt[1:2])),
            "ww_stream_step_trigger_all": lambda: lib.ww_stream_step_trigger_all(bank._h, p(frames), p(ones), p(act), p(thr), p(was), p(pmax), p(post),
                                                                                 p(n), p(ids), p(ids), p(np.zeros(S, np.uint64)), p(cnt[0:1]),
                                                                                 p(ids), p(cnt[1:2])),
            "ww_pipeline_bank_step": lambda: lib.ww_pipeline_bank_step(bank._h, p(frames), C.byref(ps)),
            "ww_stream_feed_rows": lambda: lib.ww_stream_feed_rows(bank._h, p(one), 1, p(offs), p(rows)),
            "ww_stream_feed": lambda: lib.ww_stream_feed(bank._h, p(one), 1, p(frames), p(offs), 4, p(rows), p(post), None),
            "ww_stream_feed_all": lambda: lib.ww_stream_feed_all(bank._h, p(one), 1, p(frames), p(offs), 4, p(rows), p(post), None),
            "ww_stream_feed_bytes": lambda: lib.ww_stream_feed_bytes(bank._h, p(one), 1, p(frames), p(offs), 4, p(rows), p(post), None),
            "ww_stream_set_model": lambda: lib.ww_stream_set_model(bank._h, None, 0, 0),
        }
        for name, call in calls.items():
            assert call() == -1, name
            assert name in err(e) and "ww_stream_step_ctc" in err(e) and "ww_stream_create_ctc" in err(e), (name, err(e))
        assert (post == -7.0).all() and (n == -55).all() and (ids == -55).all() and (cnt == -55).all() and (rows == -55).all() and ps.n_fired == -55
        assert not act.any() and not was.any() and (pmax == -7.0).all()
        for meth in (bank.feed, bank.feed_all, bank.set_model, bank.step_trigger, bank.step_trigger_all):
            with pytest.raises(ValueError, match="CTC-trained CRNN"):
                meth()
        # its own calls, wrongly asked for
        labels, lengths, steps = np.full((S, 2, M), -55, np.int32), np.full((S, 2), -55, np.int32), np.full((S, 2, 19, 4), -7.0, np.float32)
        tgt = np.array([1, 2], np.int32)
        for m in (0, 10):
            assert lib.ww_stream_step_ctc(bank._h, p(frames), p(ones), m, p(labels), p(lengths), None, p(n)) == -1
            assert "max_labels" in err(e)
        assert lib.ww_stream_step_ctc(bank._h, p(frames), p(ones), M, p(labels), p(lengths), p(steps), p(n)) == -1
        assert "WW_STREAM_CTC_STEPS" in err(e)
        assert lib.ww_stream_step_ctc_trigger(bank._h, p(frames), p(ones), p(act), 2, p(tgt[:0]), 0, p(was), p(labels), p(lengths), None, p(n), p(ids),
                                              p(cnt[0:1]), p(ids), p(cnt[1:2])) == -1
        assert lib.ww_stream_step_ctc_trigger(bank._h, p(frames), p(ones), p(act), 1, p(tgt), 2, p(was), p(labels), p(lengths), None, p(n), p(ids),
                                              p(cnt[0:1]), p(ids), p(cnt[1:2])) == -1
        assert "target" in err(e)
        # the new calls on a shipped model's bank
        assert lib.ww_stream_step_ctc(plain._h, p(frames), p(ones), M, p(labels), p(lengths), None, p(n)) == -1
        assert "ww_stream_step_ctc" in err(shipped) and "ww_stream_create_ctc" in err(shipped)
        assert lib.ww_stream_step_ctc_trigger(plain._h, p(frames), p(ones), p(act), 2, p(tgt), 2, p(was), p(labels), p(lengths), None, p(n), p(ids),
                                              p(cnt[0:1]), p(ids), p(cnt[1:2])) == -1
        assert "ww_stream_step_ctc_trigger" in err(shipped)
        assert (labels == -55).all() and (lengths == -55).all() and (steps == -7.0).all() and (n == -55).all() and (cnt == -55).all()
        # creation
        h, fp = C.c_void_p(), frontend_params()
        assert lib.ww_stream_create_ctc(shipped.ctx.handle, shipped.handle, S, C.byref(fp), 0, C.byref(h)) == -1 and not h.value
        assert "not a CTC-trained CRNN" in err(shipped)
        assert lib.ww_stream_create_ctc(e.ctx.handle, e.handle, S, C.byref(fp), _lib.STREAM_CAUSAL, C.byref(h)) == -1 and not h.value
        assert "WW_STREAM_CAUSAL" in err(e)
        assert lib.ww_stream_create_ctc(e.ctx.handle, e.handle, S, C.byref(fp), 32, C.byref(h)) == -1 and not h.value
        with pytest.raises(ValueError, match="CTC-trained CRNN"):
            StreamBank(e, S)   # the existing bank keeps refusing a CTC model
        with pytest.raises(ValueError, match="CTC-trained CRNN"):
            CtcStreamBank(shipped, S)
        # the bank still ticks, with the bits of its twin, which was asked for nothing of this
        for t in range(6, 40):
            got, want = bank.step(x[t], ones), twin.step(x[t], ones)
            assert_array_equal(got.n, want.n)
            assert_array_equal(got.labels, want.labels)
            assert_array_equal(got.lengths, want.lengths)
        pp, pn = plain.step(x[0], ones)
        assert pn.tolist() == [0] * S
    finally:
        for b in (bank, twin, plain):
            b.close()
        e.close()
        shipped.close()
