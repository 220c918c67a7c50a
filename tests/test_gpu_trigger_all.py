"""The wake-word stage of an every-member bank on the MI355X: ``ww_stream_step_trigger_all`` / ``WakewordSetBank``, which run K wake
words on every stream and say WHICH one fired.

The yardstick is built from what was there before: K ordinary banks, one per member, stepped with the SAME shared flags (bit 0 =
``is_speech``, bit 1 = ``is_active`` as they stand before the tick), their posteriors stacked to ``[S, K, 2]``, a Python restatement
of the rule (include/wwhip.h: ww_trigger_bank_step_all) applied in the test, and the fallen streams reset on all K banks.  The
thresholds come from a first pass over those ordinary banks - per member the median of the posteriors it emits under the script with
no stream ever active -, never from the code under test.  Everything is compared tick by tick with ``np.array_equal``.

Members: ``CRNN_nosilence``, ``CRNN_nosilence_enhanced``, ``CRNN_softmax``; one causal case on ``Wavenet``, ``Wavenet_alt``."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CRNNS = ["CRNN_nosilence", "CRNN_nosilence_enhanced", "CRNN_softmax"]
WAVES = ["Wavenet", "Wavenet_alt"]
S1, TICKS1, SEED1 = 4, 150, 23
CLEAR_EVERY = 25  # is_active cleared every 25 ticks: stands in for the timeout stage


@pytest.fixture(scope="module")
def engines(assets):
    from wwhip.engine import Engine
    out = {m: Engine(os.path.join(assets, m)) for m in CRNNS + WAVES}
    yield out
    for e in out.values():
        e.close()


@pytest.fixture(scope="module")
def crnn_set(engines):
    from wwhip.engine import ModelSet
    ms = ModelSet([engines[m] for m in CRNNS])
    yield ms
    ms.close()


@pytest.fixture(scope="module")
def wave_set(engines):
    from wwhip.engine import ModelSet
    ms = ModelSet([engines[m] for m in WAVES])
    yield ms
    ms.close()


def _script(S, ticks, seed, runs=(8, 31)):
    """Frames of noise whose level moves from tick to tick, and a VAD script per stream: runs of 8 to 30 ticks of speech (``runs``),
    gaps of 1 to 4 - several falling edges per stream."""
    rng = np.random.default_rng(seed)
    level = rng.uniform(300, 6000, (ticks, S, 1))
    frames = np.clip(rng.normal(0, 1, (ticks, S, 320)) * level, -32768, 32767).astype(np.int16)
    speech = np.zeros((ticks, S), np.uint8)
    for s in range(S):
        t = int(rng.integers(0, 3))
        while t < ticks:
            n = int(rng.integers(*runs))
            speech[t:t + n, s] = 1
            t += n + int(rng.integers(1, 5))
    assert ((speech[:-1] == 1) & (speech[1:] == 0)).sum(0).min() >= 3
    return frames, speech


def _rule(post, n_post, speech, active, thr, was, pmax):
    """ww_trigger_bank_step_all restated: ``post [S, K, 2]``; ``active``, ``was``, ``pmax [S, K]`` are updated in place.  Returns
    (fired ids, winning slots, masks, fall ids)."""
    S, K = pmax.shape
    fired, slots, masks, falls = [], [], [], []
    for s in range(S):
        fall = bool(was[s]) and not speech[s]
        was[s] = 1 if speech[s] else 0
        mask, winner = 0, None
        for k in range(int(n_post[s])):
            over = []
            for j in range(K):
                p = post[s, j, k]
                if p > pmax[s, j]:
                    pmax[s, j] = p
                if float(p) > thr[j]:
                    over.append(j)
                    mask |= 1 << j
            if over and winner is None:
                top = max(post[s, j, k] for j in over)
                winner = min(j for j in over if post[s, j, k] == top)
        if winner is not None and not active[s]:
            active[s] = 1
            fired.append(s)
            slots.append(winner)
            masks.append(mask)
        if fall:
            pmax[s, :] = 0
            falls.append(s)
    return fired, slots, masks, falls


def _reference(banks, script, thr, clear_every):
    """The members' own banks under the script and the rule: per tick (post, n_post, is_active after the tick, fired, slots, masks,
    posterior_max, falls)."""
    frames, speech = script
    S, K = frames.shape[1], len(banks)
    active, was, pmax = np.zeros(S, np.uint8), np.zeros(S, np.uint8), np.zeros((S, K), np.float32)
    out = []
    for t in range(frames.shape[0]):
        if clear_every and t % clear_every == clear_every - 1:
            active[:] = 0
        got = [b.step(frames[t], speech[t], active) for b in banks]
        for _, n in got[1:]:
            assert np.array_equal(n, got[0][1])
        post, n_post = np.stack([p for p, _ in got], axis=1), got[0][1]
        fired, slots, masks, falls = _rule(post, n_post, speech[t], active, thr, was, pmax)
        if falls:
            for b in banks:
                b.reset(falls)
        out.append((post, n_post.copy(), active.copy(), fired, slots, masks, pmax.copy(), falls))
    return out


def _thresholds(make_banks, script, K):
    """Per member the median of the posteriors its own bank emits under the script when no stream is ever active."""
    banks = make_banks()
    try:
        run = _reference(banks, script, [2.0] * K, 0)
    finally:
        for b in banks:
            b.close()
    emitted = [[] for _ in range(K)]
    for post, n_post, *_ in run:
        for s in range(post.shape[0]):
            for j in range(K):
                emitted[j] += post[s, j, :n_post[s]].tolist()
    return [float(np.median(np.array(e, np.float32))) for e in emitted]


@pytest.fixture(scope="module")
def crnn_ref(engines):
    """The script, the thresholds and the reference run - computed once, left unchanged - and the condition the reference run alone
    must satisfy: at least 10 fires over at least two distinct winning slots, and a tick whose mask has two bits."""
    from wwhip.engine import StreamBank
    script = _script(S1, TICKS1, SEED1)

    def make():
        return [StreamBank(engines[m], S1) for m in CRNNS]
    thr = _thresholds(make, script, len(CRNNS))
    banks = make()
    try:
        run = _reference(banks, script, thr, CLEAR_EVERY)
    finally:
        for b in banks:
            b.close()
    n_fired = sum(len(r[3]) for r in run)
    winners = {j for r in run for j in r[4]}
    two_bits = sum(1 for r in run for m in r[5] if bin(m).count("1") >= 2)
    n_falls = sum(len(r[7]) for r in run)
    print(f"\nTRIGGER_ALL reference: thresholds {thr}, {n_fired} fires, winners {sorted(winners)}, {two_bits} masks of two bits or more, {n_falls} falls", end="")
    assert n_fired >= 10 and len(winners) >= 2 and two_bits >= 1 and n_falls >= 3 * S1, (n_fired, winners, two_bits, n_falls)
    return script, thr, run


def _assert_tick(t, stage, active, events, ref):
    post, n_post, ref_active, fired, slots, masks, pmax, falls = ref
    assert np.array_equal(stage.n_post, n_post), t
    assert np.array_equal(stage._post, post), t
    assert np.array_equal(np.asarray(active, np.uint8), ref_active), t
    assert events == (fired, slots, masks), (t, events, (fired, slots, masks))
    assert np.array_equal(stage.posterior_max, pmax), t
    assert stage.fall_ids.tolist() == falls, t


def _drive(stage, script, contexts, clear_every, run):
    """The stage under the script on ``contexts`` (a ContextBank or a list of SpeechContext), every tick held against the reference;
    returns the activate events the contexts saw."""
    frames, speech = script
    bank_form = hasattr(contexts, "emit")
    woke, seen = [], []
    stage._on_wake = lambda ids, slots: woke.append((ids.tolist(), slots.tolist()))
    if bank_form:
        contexts.add_handler("activate", lambda c: seen.append(c._s if hasattr(c, "_s") else None))
    else:
        for s, c in enumerate(contexts):
            c.add_handler("activate", lambda ctx, s=s: seen.append(s))
    last_slot, last_mask = np.full(len(contexts), -1, np.int32), np.zeros(len(contexts), np.uint64)
    for t in range(frames.shape[0]):
        woke.clear()
        n_seen = len(seen)
        if bank_form:
            if clear_every and t % clear_every == clear_every - 1:
                contexts.is_active[:] = 0
            contexts.is_speech[:] = speech[t]
        else:
            for s, c in enumerate(contexts):
                if clear_every and t % clear_every == clear_every - 1:
                    c.is_active = False
                c.is_speech = bool(speech[t, s])
        stage.step(contexts, frames[t])
        active = contexts.is_active if bank_form else [c.is_active for c in contexts]
        ids, slots = woke[0] if woke else ([], [])
        masks = [int(stage.wake_mask[s]) for s in ids]
        _assert_tick(t, stage, active, (ids, slots, masks), run[t])
        assert len(seen) - n_seen == len(ids)  # one activate per stream that fired
        last_slot[ids], last_mask[ids] = slots, masks
        assert np.array_equal(stage.wake_slot, last_slot) and np.array_equal(stage.wake_mask, last_mask)
    return seen


def test_crnn_set_trigger_equals_the_members_banks_and_the_rule(crnn_set, crnn_ref):
    """S = 4, the three CRNNs, 150 ticks of noise, several VAD falling edges per stream, ``is_active`` cleared every 25 ticks:
    ``post`` / ``n_post``, the ``is_active`` trajectory, ``fired_ids`` / ``fired_slot`` / ``fired_mask``, ``posterior_max`` and the
    fall ids equal the reference tick by tick, with ``WakewordSetBank.step`` on a ContextBank and on a list of SpeechContext."""
    from wwhip.context import ContextBank, SpeechContext
    from wwhip.wakeword import WakewordSetBank
    script, thr, run = crnn_ref
    for contexts in (ContextBank(S1), [SpeechContext() for _ in range(S1)]):
        stage = WakewordSetBank(S1, crnn_set, thresholds=thr, names=CRNNS)
        try:
            assert stage.K == 3 and stage._bank.members.tolist() == [0, 1, 2]
            seen = _drive(stage, script, contexts, CLEAR_EVERY, run)
            assert len(seen) == sum(len(r[3]) for r in run)
            s = run[-1][3][0] if run[-1][3] else next(r[3][0] for r in reversed(run) if r[3])
            assert stage.wake_word(s) == CRNNS[int(stage.wake_slot[s])]
        finally:
            stage.close()


def test_raw_entry_point_and_its_refusals(engines, crnn_set, crnn_ref):
    """``ww_stream_step_trigger_all`` through ctypes over the first 60 ticks equals the reference; on a bank that is not every-member
    it is WW_EINVAL with a text, and so is a NULL argument; ``ww_stream_step_trigger`` on the every-member bank stays refused."""
    from wwhip import _lib
    from wwhip.engine import StreamBank
    lib, p = _lib.load(), _lib.ptr
    (frames, speech), thr, run = crnn_ref
    K = 3
    bank, ordinary = StreamBank(crnn_set, S1, members="all"), StreamBank(engines[CRNNS[0]], S1)
    try:
        active, was, pmax = np.zeros(S1, np.uint8), np.zeros(S1, np.uint8), np.zeros((S1, K), np.float32)
        post, n_post = np.zeros((S1, K, 2), np.float32), np.zeros(S1, np.int32)
        fired, slot, mask, fall = np.zeros(S1, np.int32), np.zeros(S1, np.int32), np.zeros(S1, np.uint64), np.zeros(S1, np.int32)
        nf, nl, th = np.zeros(1, np.int32), np.zeros(1, np.int32), np.array(thr, np.float64)

        def call(b, t, sp=True, fn=lib.ww_stream_step_trigger_all, th_arg=None):
            f = np.ascontiguousarray(frames[t])
            return fn(b._h, p(f), p(np.ascontiguousarray(speech[t])) if sp else None, p(active), p(th) if th_arg is None else th_arg, p(was), p(pmax),
                      p(post), p(n_post), p(fired), p(slot), p(mask), p(nf), p(fall), p(nl))
        h = crnn_set.ctx.handle
        assert call(ordinary, 0) == _lib.WW_EINVAL and "ww_stream_create_set_all" in lib.ww_last_error(h).decode()
        assert call(bank, 0, sp=False) == _lib.WW_EINVAL and "NULL" in lib.ww_last_error(h).decode()
        assert lib.ww_stream_step_trigger(bank._h, p(np.ascontiguousarray(frames[0])), p(np.ascontiguousarray(speech[0])), p(active), 0.5, p(was),
                                          p(pmax), p(post), p(n_post), p(fired), p(nf), p(fall), p(nl)) == _lib.WW_EINVAL
        assert "ww_stream_step_all" in lib.ww_last_error(h).decode()
        assert not active.any() and not was.any() and not pmax.any() and not post.any()
        for t in range(60):
            if t % CLEAR_EVERY == CLEAR_EVERY - 1:
                active[:] = 0
            assert call(bank, t) == _lib.WW_OK
            rp, rn, ra, rf, rs, rm, rx, rl = run[t]
            assert np.array_equal(post, rp) and np.array_equal(n_post, rn) and np.array_equal(active, ra) and np.array_equal(pmax, rx), t
            assert fired[:nf[0]].tolist() == rf and slot[:nf[0]].tolist() == rs and [int(m) for m in mask[:nf[0]]] == rm, t
            assert fall[:nl[0]].tolist() == rl, t
    finally:
        bank.close()
        ordinary.close()


class _Source:
    def __init__(self, frames):
        self._frames, self.t = frames, 0

    def start(self):
        pass

    stop = close = start

    def read(self):
        self.t += 1
        return self._frames[self.t - 1]


def test_pipeline_takes_the_stage(crnn_set, crnn_ref):
    """``SpeechPipelineBank([VadBank, WakewordSetBank, ActivationTimeoutBank])`` over 50 ticks raises ``activate`` / ``deactivate``
    for the same streams, tick by tick, as the three stages called by hand."""
    from wwhip.activation_timeout import ActivationTimeoutBank
    from wwhip.context import ContextBank
    from wwhip.pipeline import SpeechPipelineBank
    from wwhip.vad import VadBank
    from wwhip.wakeword import WakewordSetBank
    (frames, speech), thr, _ = crnn_ref
    ticks = 50

    def stages(src):
        return [VadBank(S1, classifier=lambda f: speech[src.t - 1]), WakewordSetBank(S1, crnn_set, thresholds=thr),
                ActivationTimeoutBank(S1, min_active=60, max_active=200)]

    def watch(ctxs, log):
        ctxs.add_handler("activate", lambda c: log[-1].append(("activate", c._s)))
        ctxs.add_handler("deactivate", lambda c: log[-1].append(("deactivate", c._s)))

    src = _Source(frames)
    pipe = SpeechPipelineBank(src, stages(src), S1)
    piped, slots_piped = [], []
    watch(pipe.context, piped)
    for t in range(ticks):
        piped.append([])
        pipe.step()
        slots_piped.append(pipe._stages[1].wake_slot.copy())
    assert pipe._fused is None
    piped.append([])  # (cleanup resets the contexts: its deactivate events are not a tick's)
    pipe.cleanup()
    piped.pop()

    src = _Source(frames)
    by_hand, ctxs, hand, slots_hand = stages(src), ContextBank(S1), [], []
    watch(ctxs, hand)
    try:
        for t in range(ticks):
            hand.append([])
            f = src.read()
            for st in by_hand:
                st(ctxs, f)
            slots_hand.append(by_hand[1].wake_slot.copy())
    finally:
        by_hand[1].close()
    assert piped == hand and np.array_equal(slots_piped, slots_hand)
    kinds = {k for tick in piped for k, _ in tick}
    assert kinds == {"activate", "deactivate"}, kinds


def test_causal_wavenet_set_trigger(engines, wave_set):
    """``WakewordSetBank(causal=True)``, S = 3, K = 2, 60 ticks: equal to the restatement over the members' own causal banks."""
    from wwhip.context import ContextBank
    from wwhip.engine import StreamBank
    from wwhip.wakeword import WakewordSetBank
    S, ticks = 3, 60
    script = _script(S, ticks, 31, runs=(5, 14))

    def make():
        return [StreamBank(engines[m], S, causal=True) for m in WAVES]
    thr = _thresholds(make, script, 2)
    banks = make()
    try:
        run = _reference(banks, script, thr, 20)
    finally:
        for b in banks:
            b.close()
    assert sum(len(r[3]) for r in run) >= 3 and sum(len(r[7]) for r in run) >= 3
    stage = WakewordSetBank(S, wave_set, thresholds=thr, causal=True)
    try:
        assert stage._bank.causal and stage.K == 2
        _drive(stage, script, ContextBank(S), 20, run)
    finally:
        stage.close()
