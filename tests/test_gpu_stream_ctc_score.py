"""The forward-algorithm score in CTC stream banks on the MI355X (``ww_stream_ctc_set_targets``, ``ww_stream_step_ctc_score``,
``ww_ctc_score_trigger_bank_step``): 45 ticks of tests/stream_ctc64.py's signal, S = 3 - stream 1 toggles, stream 2 is frozen for a
while, stream 1 is reset -, L = 4, K = 2 targets, both modes, in every form of the bank.  A tick's scores are held to the bits of
``ctc_score_dev`` on the posteriors the same tick returns; those posteriors are held to float64 by tests/test_gpu_stream_ctc.py."""
import os

import numpy as np
import pytest
from numpy.testing import assert_array_equal

import ctc64
import ctc_score64 as S64
import stream_ctc64 as SC

pytestmark = pytest.mark.gpu

TICKS, S, L, M = 45, 3, 4, 9
TARGETS = [(1, 2), (0,)]
K = len(TARGETS)
SENT = -7.0
RESET_TICK = 30
FORMS = {"one launch": {}, "two launches": dict(two_launch=True), "full recompute": dict(full_recompute=True)}


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


def _score_dev(e, steps, mode):
    import torch
    n = len(steps)
    d_steps = torch.from_numpy(np.ascontiguousarray(steps, np.float32)).cuda()
    d_out = torch.full((K, n), SENT, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    e.ctc_score_dev(d_steps.data_ptr(), n, 19, L, TARGETS, mode, d_out.data_ptr())
    e.ctx.synchronize()
    return d_out.cpu().numpy()


def _raw_tick(bank, frames, flags, scored=True):
    """One tick through the library with sentinel-filled outputs -> ``(n, labels, lengths, steps, scores)``."""
    from wwhip import _lib
    p = _lib.ptr
    labels, lengths = np.full((S, 2, M), -55, np.int32), np.full((S, 2), -55, np.int32)
    steps, scores, n = np.full((S, 2, 19, L), SENT, np.float32), np.full((S, 2, K), SENT, np.float32), np.full(S, -55, np.int32)
    frames, flags = np.ascontiguousarray(frames), np.ascontiguousarray(flags)
    if scored:
        rc = bank._lib.ww_stream_step_ctc_score(bank._h, p(frames), p(flags), M, p(labels), p(lengths), p(steps), p(scores), p(n))
    else:
        rc = bank._lib.ww_stream_step_ctc(bank._h, p(frames), p(flags), M, p(labels), p(lengths), p(steps), p(n))
    _lib.raise_for(rc, bank.engine.ctx.handle)
    return n, labels, lengths, steps, scores


@pytest.mark.parametrize("mode", S64.MODES)
def test_scores_are_the_kernel_on_the_ticks_own_steps_in_every_form(engine, mode):
    from wwhip.engine import CtcStreamBank
    e = engine
    x, flags = SC.pcm(), _flags()
    scored = {k: CtcStreamBank(e, S, max_labels=M, want_steps=True, targets=TARGETS, mode=mode, **kw) for k, kw in FORMS.items()}
    plain = {k: CtcStreamBank(e, S, max_labels=M, want_steps=True, **kw) for k, kw in FORMS.items()}   # no targets: the parent's tick
    seen, windows = set(), 0
    try:
        for t in range(TICKS):
            if t == RESET_TICK:
                for b in list(scored.values()) + list(plain.values()):
                    b.reset([1])
            got = {}
            for name in FORMS:
                n, labels, lengths, steps, scores = _raw_tick(scored[name], x[t], flags[t])
                got[name] = scores
                pn, plabels, plengths, psteps, _ = _raw_tick(plain[name], x[t], flags[t], scored=False)
                # the tick itself is what it is without targets
                assert_array_equal(n, pn, err_msg=f"{name} tick {t}")
                assert_array_equal(labels, plabels, err_msg=f"{name} tick {t}")
                assert_array_equal(lengths, plengths, err_msg=f"{name} tick {t}")
                assert_array_equal(steps.view(np.uint32), psteps.view(np.uint32), err_msg=f"{name} tick {t}")
                for s in range(S):
                    k = int(n[s])
                    seen.add(k)
                    assert (scores[s, k:] == SENT).all() and (steps[s, k:] == SENT).all()
                    if not k:
                        continue
                    windows += k
                    want = _score_dev(e, steps[s, :k], mode)    # [K, k]
                    assert_array_equal(scores[s, :k].view(np.uint32), np.ascontiguousarray(want.T).view(np.uint32), err_msg=f"{name} tick {t} stream {s}")
                    if name == "full recompute":
                        w = scored[name].window(s)
                        assert_array_equal(scores[s, k - 1], e.ctc_score(w[None], TARGETS, mode)[:, 0])
                        off = e.ctc_forward(w[None], max_labels=M, want=("labels", "steps"))
                        assert_array_equal(steps[s, k - 1].view(np.uint32), off.steps[0].view(np.uint32))
                        assert_array_equal(labels[s, k - 1], off.labels[0])
                        assert lengths[s, k - 1] == off.lengths[0]
            # the incremental forms agree with one another bit for bit, scores included
            assert_array_equal(got["one launch"].view(np.uint32), got["two launches"].view(np.uint32), err_msg=f"tick {t}")
    finally:
        for b in list(scored.values()) + list(plain.values()):
            b.close()
    assert seen == {0, 1, 2} and windows > 3 * 150


def test_python_tick_carries_scores_and_set_targets_changes_them(engine):
    from wwhip.engine import CtcStreamBank
    e = engine
    x, flags = SC.pcm(), _flags()
    bank = CtcStreamBank(e, S, max_labels=2, targets=TARGETS, mode="prefix")     # (want_steps off: the scores alone)
    twin = CtcStreamBank(e, S, max_labels=2, want_steps=True)
    try:
        assert bank.n_targets == K
        for t in range(12):
            if t == 6:
                bank.set_targets([(2,), (1, 1), (0, 1, 2)], "exact")
            tick, ref = bank.step(x[t], flags[t] & 1, flags[t] >> 1), twin.step(x[t], flags[t] & 1, flags[t] >> 1)
            assert tick.steps is None and ref.scores is None
            assert_array_equal(tick.n, ref.n)
            assert_array_equal(tick.labels, ref.labels)
            tg, mode = (TARGETS, "prefix") if t < 6 else ([(2,), (1, 1), (0, 1, 2)], "exact")
            assert tick.scores.shape == (S, 2, len(tg))
            for s in range(S):
                k = int(tick.n[s])
                assert (tick.scores[s, k:] == 0).all()
                if k:
                    import torch
                    d_steps = torch.from_numpy(np.ascontiguousarray(ref.steps[s, :k])).cuda()
                    d_out = torch.full((len(tg), k), SENT, dtype=torch.float32, device="cuda")
                    torch.cuda.synchronize()
                    e.ctc_score_dev(d_steps.data_ptr(), k, 19, L, tg, mode, d_out.data_ptr())
                    e.ctx.synchronize()
                    assert_array_equal(tick.scores[s, :k], d_out.cpu().numpy().T)
    finally:
        bank.close()
        twin.close()


def test_the_wake_word_stage_fires_on_the_tick_and_slot_the_rule_names(engine):
    """``CtcWakewordBank(thresholds=)``: thresholds at the median of the scores a plain run of the same ticks gives, so that streams
    fire, and on different slots."""
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
    events, woke = [], []
    ctxs.add_handler("activate", lambda view: events.append(int(np.flatnonzero([view is ctxs[s] for s in range(S)])[0])))
    bank = CtcStreamBank(e, S, max_labels=2, targets=TARGETS, mode="prefix")
    stage = CtcWakewordBank(S, bank=bank, thresholds=thr, on_wake=lambda ids: woke.extend(int(i) for i in ids))
    active, was, fired_all, slots_all = [0] * S, [0] * S, [], []
    try:
        with pytest.raises(ValueError, match="thresholds"):
            CtcWakewordBank(S, bank=bank, thresholds=[0.5])
        for t in range(TICKS):
            if t in (15, 31):   # release: an active stream is frozen
                ctxs.is_active[:] = 0
                active = [0] * S
            ctxs.is_speech[:] = sp[t]
            n_events = len(events)
            tick = stage(ctxs, x[t])
            want_fired, want_slot, want_fall = [], [], []
            for s in range(S):
                n = int(tick.n[s])
                assert n == 0 or (sp[t, s] and not active[s])
                win = -1
                for k in range(n):
                    over = [j for j in range(K) if float(tick.scores[s, k, j]) > thr[j]]
                    if over:
                        win = max(over, key=lambda j: (tick.scores[s, k, j], -j))
                        break
                if win >= 0 and not active[s]:
                    active[s] = 1
                    want_fired.append(s)
                    want_slot.append(win)
                if was[s] and not sp[t, s]:
                    want_fall.append(s)
                was[s] = int(sp[t, s])
            assert stage.fired_ids.tolist() == want_fired and events[n_events:] == want_fired, (t, stage.fired_ids, want_fired)
            assert stage.fired_slots.tolist() == want_slot and stage.fall_ids.tolist() == want_fall, t
            assert ctxs.is_active.tolist() == active
            for s in want_fall:   # the streams whose speech bit fell were reset: an all-zero window
                assert not bank.window(s).any(), (t, s)
            fired_all += want_fired
            slots_all += want_slot
    finally:
        stage.close()
    assert woke == fired_all and len(set(fired_all)) >= 2 and len(fired_all) > len(set(fired_all)), fired_all
    print(f"\nfired {fired_all} on slots {slots_all} (thresholds {thr.tolist()})", end="")
    assert set(slots_all) <= {0, 1}


def test_refusals_move_nothing(engine, assets):
    from wwhip import _lib, ctc
    from wwhip.engine import CtcStreamBank, Engine, StreamBank
    e = engine
    lib, p = _lib.load(), _lib.ptr
    x = SC.pcm()
    tab, lens = ctc.pack_targets(TARGETS, L)
    labels_only, steps_bank = CtcStreamBank(e, S, max_labels=M), CtcStreamBank(e, S, max_labels=M, want_steps=True)
    shipped = Engine(os.path.join(assets, "CRNN"))
    plain = StreamBank(shipped, S)
    err = lambda eng: lib.ww_last_error(eng.ctx.handle).decode()
    try:
        assert lib.ww_stream_ctc_set_targets(labels_only._h, p(tab), p(lens), K, 0) == _lib.WW_EINVAL and "WW_STREAM_CTC_STEPS" in err(e)
        assert lib.ww_stream_ctc_set_targets(plain._h, p(tab), p(lens), K, 0) == _lib.WW_EINVAL and "ww_stream_create_ctc" in err(shipped)
        with pytest.raises(ValueError, match="WW_STREAM_CTC_STEPS"):
            labels_only.set_targets(TARGETS)
        for kw, word in ((dict(K=0), "K = 0"), (dict(K=9), "K = 9"), (dict(mode=2), "mode"), (dict(lens=np.array([0, 1], np.int32)), "U = 0"),
                         (dict(lens=np.array([10, 1], np.int32)), "U = 10"), (dict(tab=np.full((2, 9), 3, np.int32)), "label")):
            a = dict(tab=tab, lens=lens, K=K, mode=0)
            a.update(kw)
            assert lib.ww_stream_ctc_set_targets(steps_bank._h, p(a["tab"]), p(a["lens"]), a["K"], a["mode"]) == _lib.WW_EINVAL and word in err(e), kw
        # a tick that asks for scores before there are targets: refused, nothing moves
        ones = np.ones(S, np.uint8)
        labels, lengths = np.full((S, 2, M), -55, np.int32), np.full((S, 2), -55, np.int32)
        scores, n = np.full((S, 2, K), SENT, np.float32), np.full(S, -55, np.int32)
        frames = np.ascontiguousarray(x[0])
        for bank, eng in ((steps_bank, e), (labels_only, e), (plain, shipped)):
            assert lib.ww_stream_step_ctc_score(bank._h, p(frames), p(ones), M, p(labels), p(lengths), None, p(scores), p(n)) == _lib.WW_EINVAL
            assert "ww_stream_step_ctc_score" in err(eng)
        steps_bank.set_targets(TARGETS)
        assert lib.ww_stream_step_ctc_score(steps_bank._h, p(frames), p(ones), M, p(labels), p(lengths), None, None, p(n)) == _lib.WW_EINVAL
        assert (labels == -55).all() and (lengths == -55).all() and (scores == SENT).all() and (n == -55).all()
        with pytest.raises(ValueError):
            CtcStreamBank(e, S, targets=[(3,)])
        # the banks still tick, with one another's bits
        for t in range(10):
            got, want = steps_bank.step(x[t], ones), labels_only.step(x[t], ones)
            assert_array_equal(got.n, want.n)
            assert_array_equal(got.labels, want.labels)
            assert got.scores is not None and want.scores is None
    finally:
        for b in (labels_only, steps_bank, plain):
            b.close()
        shipped.close()
