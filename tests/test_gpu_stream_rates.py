"""Stream banks whose streams each run at their own rate on the MI355X (``ww_stream_attach_rates``, ``StreamBank(sample_rate=[...])``).

The contract (include/wwhip.h): stream s of a mixed-rate bank yields, for every call, THE BITS stream s yields in a bank that runs at
``rates[s]`` alone - the plain bank for 16000, the bank ``StreamBank(e, S, sample_rate=R)`` for any other rate.  The oracle is public
API only: per distinct rate R one uniform bank of S streams with the same flags, resets and moves; stream s's frames go into slot s
of the bank of its rate and zeros into the other slots, and only the slots of a bank's own rate are compared.  Every comparison is
BIT FOR BIT (``np.array_equal`` on the float32 posteriors' integer views, on ``n_post``, on ``bank.window(s)``): no tolerance.

Shapes: S = 7 streams, 40 ticks (the 512-sample ring fills, ticks of one and of two frames, past the CRNN's first windows), rates
[48000, 16000, 44100, 8000, 22050, 16000, 48000]: up = 1, a general up, up = 2, an odd frame length and the pass-through, two streams
per class twice, frames at byte offsets 0, 1920, 2560, 4324, 4644, 5526, 6166 of the ragged block - modulo 16: 0, 0, 0, 4, 4, 6, 6.
Stream 0 is a full-scale +-32767 square (the int16 clamp is hit), stream 5 all zeros, the rest a tone plus seeded noise.
"""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

S, TICKS = 7, 40
RATES = [48000, 16000, 44100, 8000, 22050, 16000, 48000]
FORMS = {"crnn": ("CRNN", {}), "crnn_two_launch_sync": ("CRNN", dict(two_launch=True, sync_wait=True)),
         "crnn_full_recompute": ("CRNN", dict(full_recompute=True)), "wavenet": ("Wavenet", {}), "causal": ("Wavenet", dict(causal=True))}
SET_MEMBERS = ["CRNN_nosilence", "CRNN_nosilence_enhanced"]


@pytest.fixture(scope="module")
def engines(assets):
    from wwhip.engine import Engine
    out = {m: Engine(os.path.join(assets, m)) for m in ["CRNN", "Wavenet"] + SET_MEMBERS}
    yield out
    for e in out.values():
        e.close()


_sig_cache = {}


def _signal(s, rate, seconds=TICKS / 50):
    """Stream s's int16 signal at ``rate``, computed once per (stream, rate, length) and never written to."""
    key = (s, rate, seconds)
    if key not in _sig_cache:
        n = int(round(rate * seconds))
        rng = np.random.default_rng(1000 * s + rate)
        t = np.arange(n) / rate
        if s == 0:
            x = np.where((np.arange(n) // 23) % 2 == 0, 32767, -32767).astype(np.int16)
        elif s == 5:
            x = np.zeros(n, np.int16)
        else:
            tone = 0.25 * 32768 * np.sin(2 * np.pi * (300.0 + 170.0 * s) * t)
            x = np.clip(np.rint(tone + rng.normal(0, 0.08 * 32768, n)), -32768, 32767).astype(np.int16)
        x.setflags(write=False)
        _sig_cache[key] = x
    return _sig_cache[key]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _uniform(eng, rate, **kw):
    from wwhip.engine import StreamBank
    return StreamBank(eng, S, **kw) if rate == 16000 else StreamBank(eng, S, sample_rate=rate, **kw)


def _layout(bank):
    """``ww_stream_frame_layout`` through ctypes."""
    from wwhip import _lib
    fs, fo = np.full(bank.S, -1, np.int32), np.full(bank.S + 1, -1, np.int64)
    assert _lib.load().ww_stream_frame_layout(bank._h, _lib.ptr(fs), _lib.ptr(fo)) == _lib.WW_OK
    return fs, fo


def _check_layout(bank, rates):
    fs, fo = _layout(bank)
    want = np.array([r // 50 for r in rates], np.int32)
    assert np.array_equal(fs, want) and np.array_equal(fo, np.concatenate(([0], np.cumsum(want))))
    assert np.array_equal(bank.frame_samples, fs) and np.array_equal(bank.frame_offs, fo) and np.array_equal(bank.sample_rates, rates)
    assert bank.frame_samples.dtype == np.int32 and bank.frame_offs.dtype == np.int64 and bank.sample_rates.dtype == np.int32


def _run(mixed, oracles, rates, speech=None, active=None, reset_after=None, moves=None, set_model_after=None, ticks=TICKS):
    """``mixed`` against ``oracles`` = {rate: uniform bank} tick by tick: stream s's frames (of its signal at its CURRENT rate) go to
    slot s of the oracle of that rate, zeros to the other slots; flags, resets (``reset_after[t]`` = ids or None for the whole bank),
    member moves and rate moves (``moves[t]`` = [(ids, rate)]: the oracle resets the slot in every bank, which ends it in the old
    rate's and starts it in the new rate's) are mirrored.  Posteriors and counts of every tick and the final windows are compared
    for the slots of a bank's own rate.  -> posteriors compared per stream."""
    cur = list(rates)
    seen = np.zeros(S, int)
    ones = np.ones(S, np.uint8)
    for t in range(ticks):
        sp = ones if speech is None else speech[t]
        ac = None if active is None else active[t]
        frames = [_signal(s, cur[s])[t * (cur[s] // 50):(t + 1) * (cur[s] // 50)] for s in range(S)]
        # the flat block and the per-stream sequence in turn
        got = mixed.step(np.concatenate(frames) if t % 2 else frames, sp, ac)
        for R, bank in oracles.items():
            fr = np.zeros((S, R // 50), np.int16)
            mine = [s for s in range(S) if cur[s] == R]
            for s in mine:
                fr[s] = frames[s]
            want = bank.step(fr, sp, ac)
            for s in mine:
                assert got[1][s] == want[1][s], ("tick", t, "stream", s, got[1], want[1])
                assert np.array_equal(_bits(got[0][s]), _bits(want[0][s])), ("tick", t, "stream", s, got[0][s], want[0][s])
                seen[s] += int(got[1][s])
        if reset_after and t in reset_after:
            for b in [mixed] + list(oracles.values()):
                b.reset(reset_after[t])
        if set_model_after and t in set_model_after:
            for b in [mixed] + list(oracles.values()):
                b.set_model(*set_model_after[t])
        for ids, rate in (moves or {}).get(t, []):
            mixed.set_rate(ids, rate)
            for b in oracles.values():
                b.reset(ids)
            for s in ids:
                cur[s] = rate
            _check_layout(mixed, cur)
    for s in range(S):
        assert np.array_equal(_bits(mixed.window(s)), _bits(oracles[cur[s]].window(s))), ("window of stream", s)
    return seen


def _script(seed):
    """Random VAD bits, a frozen stretch per stream (its frames are dropped whole), per-stream resets and one of the whole bank."""
    rng = np.random.default_rng(seed)
    speech = (rng.random((TICKS, S)) < 0.85).astype(np.uint8)
    active = np.zeros((TICKS, S), np.uint8)
    for s in range(S):
        a = int(rng.integers(4, 30))
        active[a:a + int(rng.integers(1, 6)), s] = 1
    return speech, active, {9: [2, 3], 17: [0], 24: None, 31: [6, 1, 4]}


def _close(*banks):
    for b in banks:
        b.close()


@pytest.mark.parametrize("form", list(FORMS))
def test_mixed_bank_equals_the_uniform_banks_slot_by_slot(engines, form):
    """Ticks in every form a bank has: the incremental CRNN in one launch (polled), in two launches with the runtime's wait,
    WW_STREAM_FULL_RECOMPUTE, the Wavenet window bank and the causal bank - with random VAD bits, frozen stretches, per-stream and
    whole-bank resets."""
    from wwhip.engine import StreamBank
    model, kw = FORMS[form]
    eng = engines[model]
    mixed = StreamBank(eng, S, sample_rate=RATES, **kw)
    oracles = {R: _uniform(eng, R, **kw) for R in sorted(set(RATES))}
    try:
        _check_layout(mixed, RATES)
        assert (mixed.frame_offs[:-1] * 2 % 16).tolist() == [0, 0, 0, 4, 4, 6, 6]
        speech, active, resets = _script(len(form))
        seen = _run(mixed, oracles, RATES, speech, active, resets)
        print("posteriors compared per stream:", seen.tolist())
        assert (seen >= 20).all(), seen
    finally:
        _close(mixed, *oracles.values())


def test_model_set_bank_with_mixed_rates(engines):
    """A ModelSet of two CRNNs, streams dealt [0, 1, 0, 1, 1, 0, 1] over the seven rates' streams; streams 2 and 6 move to the other
    member after tick 15 (set_model resets them, the resampling state included) - mirrored in the uniform set banks."""
    from wwhip.engine import ModelSet, StreamBank
    ms = ModelSet([engines[m] for m in SET_MEMBERS])
    deal = [0, 1, 0, 1, 1, 0, 1]
    mixed = StreamBank(ms, S, models=deal, sample_rate=RATES)
    oracles = {R: _uniform(ms, R, models=deal) for R in sorted(set(RATES))}
    try:
        seen = _run(mixed, oracles, RATES, set_model_after={15: ([2], 1), 16: ([6], 0)})
        assert (seen >= 20).all(), seen
    finally:
        _close(mixed, *oracles.values())
        ms.close()


def test_set_rate_mid_run(engines):
    """Stream 0 moves 48000 -> 8000 after tick 15 (a frame six times shorter: every later stream's offset moves), stream 3 moves
    8000 -> 16000 after tick 22 (into the pass-through class).  frame_samples / frame_offs equal ww_stream_frame_layout before and
    after each move."""
    from wwhip.engine import StreamBank
    eng = engines["CRNN"]
    mixed = StreamBank(eng, S, sample_rate=RATES)
    oracles = {R: _uniform(eng, R) for R in sorted(set(RATES))}
    try:
        _check_layout(mixed, RATES)
        seen = _run(mixed, oracles, RATES, moves={15: [([0], 8000)], 22: [([3], 16000)]})
        after = [8000, 16000, 44100, 16000, 22050, 16000, 48000]
        _check_layout(mixed, after)
        assert (seen >= 20).all(), seen
        with pytest.raises(ValueError, match="not among"):
            mixed.set_rate([1], 32000)
    finally:
        _close(mixed, *oracles.values())


@pytest.mark.parametrize("rate", [48000, 16000])
def test_degenerate_mixes(engines, rate):
    """``sample_rate=[48000] * S`` equals ``sample_rate=48000`` and ``[16000] * S`` the plain bank, tick by tick: a sequence always
    makes a bank with per-stream rates, of one class here."""
    from wwhip.engine import StreamBank
    eng = engines["CRNN"]
    mixed = StreamBank(eng, S, sample_rate=[rate] * S)
    oracles = {rate: _uniform(eng, rate)}
    try:
        assert mixed._mixed and not oracles[rate]._mixed
        _check_layout(mixed, [rate] * S)
        seen = _run(mixed, oracles, [rate] * S)
        assert (seen >= 2 * TICKS - 4).all(), seen
    finally:
        _close(mixed, *oracles.values())


def test_feed_on_a_causal_mixed_bank(engines):
    """Packets of seeded random lengths 1 .. 3000 at each stream's own rate to random subsets of the streams, empty packets and a
    1-sample packet at 48000 (which completes no 16 kHz sample) among them, ticks of the whole bank in between.  Oracle: the
    uniform causal banks given the same packets (each the streams of its rate) and the same ticks.  Posteriors, mel rows, the rows
    ww_stream_feed_rows predicts and a final tick are equal."""
    from wwhip import _lib
    from wwhip.engine import StreamBank
    eng = engines["Wavenet"]
    lib = _lib.load()
    mixed = StreamBank(eng, S, causal=True, sample_rate=RATES)
    oracles = {R: _uniform(eng, R, causal=True) for R in sorted(set(RATES))}
    rng = np.random.default_rng(77)
    at = np.zeros(S, int)
    ones = np.ones(S, np.uint8)
    rows_seen = np.zeros(S, int)

    def take(s, k):
        x = _signal(s, RATES[s], 6.0)
        assert at[s] + k <= len(x)
        at[s] += k
        return x[at[s] - k:at[s]]

    def feed(ids, ks):
        pk = [take(s, k) for s, k in zip(ids, ks)]
        a_ids, offs, row_offs = np.asarray(ids, np.int32), np.zeros(len(ids) + 1, np.int64), np.zeros(len(ids) + 1, np.int64)
        np.cumsum(ks, out=offs[1:])
        assert lib.ww_stream_feed_rows(mixed._h, _lib.ptr(a_ids), len(ids), _lib.ptr(offs), _lib.ptr(row_offs)) == 0
        p, m = mixed.feed(ids, pk, want_mel=True)
        assert np.diff(row_offs).tolist() == [len(v) for v in p]  # the prediction equals the rows delivered
        for R, bank in oracles.items():
            sub = [i for i, s in enumerate(ids) if RATES[s] == R]
            if not sub:
                continue
            q, n = bank.feed([ids[i] for i in sub], [pk[i] for i in sub], want_mel=True)
            for j, i in enumerate(sub):
                assert np.array_equal(_bits(p[i]), _bits(q[j])), ("posteriors of stream", ids[i], len(p[i]), len(q[j]))
                assert np.array_equal(_bits(m[i]), _bits(n[j])), ("mel rows of stream", ids[i])
                rows_seen[ids[i]] += len(p[i])

    def tick():
        frames = [take(s, RATES[s] // 50) for s in range(S)]
        got = mixed.step(frames, ones)
        for R, bank in oracles.items():
            fr = np.zeros((S, R // 50), np.int16)
            mine = [s for s in range(S) if RATES[s] == R]
            for s in mine:
                fr[s] = frames[s]
            want = bank.step(fr, ones)
            for s in mine:
                assert got[1][s] == want[1][s] and np.array_equal(_bits(got[0][s]), _bits(want[0][s])), ("tick, stream", s)
                rows_seen[s] += int(got[1][s])

    try:
        feed([0, 6], [1, 1])  # one sample at 48000: the resampling state moves and nothing else
        assert rows_seen.sum() == 0
        feed([1, 3, 5], [0, 0, 0])  # empty packets
        tick()
        for call in range(14):
            ids = [s for s in range(S) if rng.random() < 0.6]
            if not ids:
                continue
            ks = [0 if rng.random() < 0.1 else int(rng.integers(1, 3001)) for _ in ids]
            feed(ids, ks)
            if call % 4 == 3:
                tick()
                tick()
        feed(list(range(S)), [7] * S)
        tick()  # the final tick
        print("rows compared per stream:", rows_seen.tolist())
        assert (rows_seen >= 20).all(), rows_seen
        for s in range(S):
            assert np.array_equal(_bits(mixed.window(s)), _bits(oracles[RATES[s]].window(s))), ("window of stream", s)
    finally:
        _close(mixed, *oracles.values())


def test_step_trigger_through_a_wakeword_bank(engines):
    """``WakewordBank(bank=mixed)`` (``ww_stream_step_trigger``) over the 40 ticks against the same stage on the uniform banks: fired
    and fallen ids, running maxima, posteriors and counts, slot by slot.  Each stream's VAD bit falls once (the stage resets the
    stream); an activated stream stays frozen for 4 ticks and is then released, by the same rule on every side.  The threshold is
    the median over streams of the largest posterior of ticks 3 .. 14 of a plain run of the mixed bank, so some streams fire."""
    from wwhip.context import ContextBank
    from wwhip.engine import StreamBank
    from wwhip.wakeword import WakewordBank
    eng = engines["CRNN"]

    def frames_at(t):
        return [_signal(s, RATES[s])[t * (RATES[s] // 50):(t + 1) * (RATES[s] // 50)] for s in range(S)]

    probe = StreamBank(eng, S, sample_rate=RATES)
    top = np.zeros(S, np.float32)
    for t in range(15):
        p, n = probe.step(frames_at(t), np.ones(S, np.uint8))
        for s in range(S):
            if t >= 3:
                top[s] = max([top[s]] + [p[s, k] for k in range(n[s])])
    probe.close()
    thr = float(np.median(top))
    print("trigger: largest posteriors of ticks 3 .. 14", top, "threshold", thr)
    assert (top > thr).any()
    rng = np.random.default_rng(6)
    speech = np.ones((TICKS, S), np.uint8)
    for s in range(S):
        a = int(rng.integers(18, 30))
        speech[a:a + 4, s] = 0

    def stage(bank):
        return dict(wake=WakewordBank(S, posterior_threshold=thr, bank=bank), ctx=ContextBank(S), held=np.zeros(S, int))

    def step(st, t, frames):
        ctx, wake = st["ctx"], st["wake"]
        ctx.is_speech[:] = speech[t]
        post = wake.step(ctx, frames)
        out = dict(fired=set(wake._fired[:wake._counts[0]].tolist()), fall=set(wake._fall[:wake._counts[1]].tolist()),
                   post=post, n=wake.n_post.copy(), top=wake.posterior_max.copy(), active=ctx.is_active.copy())
        st["held"][ctx.is_active != 0] += 1
        release = st["held"] >= 4
        ctx.is_active[release] = 0
        st["held"][release] = 0
        return out

    mixed = stage(StreamBank(eng, S, sample_rate=RATES))
    oracles = {R: stage(_uniform(eng, R)) for R in sorted(set(RATES))}
    fired_all, fall_all = set(), []
    try:
        for t in range(TICKS):
            frames = frames_at(t)
            got = step(mixed, t, np.concatenate(frames))
            fired_all |= got["fired"]
            fall_all += sorted(got["fall"])
            for R, st in oracles.items():
                fr = np.zeros((S, R // 50), np.int16)
                mine = [s for s in range(S) if RATES[s] == R]
                for s in mine:
                    fr[s] = frames[s]
                want = step(st, t, fr)
                for s in mine:
                    assert (s in got["fired"]) == (s in want["fired"]) and (s in got["fall"]) == (s in want["fall"]), (t, s, got, want)
                    assert got["n"][s] == want["n"][s] and got["active"][s] == want["active"][s], (t, s)
                    assert np.array_equal(_bits(got["post"][s]), _bits(want["post"][s])), (t, s)
                    assert np.array_equal(_bits(got["top"][s]), _bits(want["top"][s])), (t, s)
        print("trigger: fired", sorted(fired_all), "fell", fall_all)
        assert sorted(fall_all) == list(range(S))  # every stream's VAD bit fell once
        assert fired_all >= set(np.flatnonzero(top > thr).tolist())
    finally:
        mixed["wake"].close()
        for st in oracles.values():
            st["wake"].close()


def test_refusals(engines):
    """Through ctypes, each with its status and the reason in ww_last_error: 9 classes, two classes of one rate, 11025 Hz, a class id
    out of range (its index named), an attach after a tick (WW_ESTATE), an attach on a bank that has a resampler, set_rate on a
    uniform bank and with a class out of range, ww_stream_frame_samples on a mixed bank.  The bank is usable after each WW_EINVAL.
    Argument checks all: each returns before any launch."""
    from wwhip import _lib
    from wwhip.engine import StreamBank
    from wwhip.resample import Resampler
    eng = engines["CRNN"]
    lib, ctx = _lib.load(), eng.ctx
    rs = {r: Resampler(r, 16000, ctx) for r in (8000, 11025, 22050, 24000, 32000, 44100, 48000, 88200, 96000)}
    rs48b = Resampler(48000, 16000, ctx)

    def table(*entries):
        return (C.c_void_p * len(entries))(*[None if e is None else e._h for e in entries]), len(entries)

    def attach(bank, entries, cls=None):
        t, n = table(*entries)
        a = None if cls is None else np.asarray(cls, np.int32)
        return lib.ww_stream_attach_rates(bank._h, t, n, _lib.ptr(a))

    def refused(rc, code, *words):
        assert rc == code, (rc, code, lib.ww_last_error(ctx.handle).decode())
        text = lib.ww_last_error(ctx.handle).decode()
        for w in words:
            assert w in text, (w, text)

    def usable(bank):
        fs, fo = _layout(bank)
        assert fo[-1] == fs.sum()

    bank = StreamBank(eng, S)
    try:
        nine = [rs[r] for r in (8000, 22050, 24000, 32000, 44100, 48000, 88200, 96000)] + [None]
        refused(attach(bank, nine), _lib.WW_EINVAL, "9 rate classes", "1..8")
        refused(attach(bank, []), _lib.WW_EINVAL, "0 rate classes")
        usable(bank)
        refused(attach(bank, [rs[48000], None, rs48b]), _lib.WW_EINVAL, "class 2", "48000", "same input rate")
        refused(attach(bank, [None, rs[8000], None]), _lib.WW_EINVAL, "class 2", "NULL class")
        refused(attach(bank, [None, rs[11025]]), _lib.WW_EINVAL, "class 1", "fractional")
        usable(bank)
        refused(attach(bank, [rs[48000], None], [0, 1, 0, 1, 2, 0, 0]), _lib.WW_EINVAL, "stream_rate[4] = 2", "0..1")
        refused(attach(bank, [rs[48000], None], [0, 1, 0, 1, 1, 0, -1]), _lib.WW_EINVAL, "stream_rate[6] = -1")
        refused(lib.ww_stream_set_rate(bank._h, None, 0, 0), _lib.WW_EINVAL, "no per-stream rates")
        usable(bank)
        # the refusals left a bank that takes its rates and ticks (NULL stream_rate: every stream in class 0)
        assert attach(bank, [rs[48000], None]) == _lib.WW_OK
        fs, fo = _layout(bank)
        assert fs.tolist() == [960] * S and fo.tolist() == [960 * s for s in range(S + 1)]
        refused(attach(bank, [rs[8000]]), _lib.WW_EINVAL, "already has its rates")
        refused(lib.ww_stream_attach_resampler(bank._h, rs[8000]._h), _lib.WW_EINVAL, "already has per-stream rates")
        n = C.c_int32(-1)
        refused(lib.ww_stream_frame_samples(bank._h, C.byref(n)), _lib.WW_EINVAL, "ww_stream_frame_layout")
        refused(lib.ww_stream_set_rate(bank._h, None, 0, 2), _lib.WW_EINVAL, "class 2", "0..1")
        refused(lib.ww_stream_set_rate(bank._h, None, 0, -1), _lib.WW_EINVAL, "class -1")
        bad = np.array([0, S], np.int32)
        refused(lib.ww_stream_set_rate(bank._h, _lib.ptr(bad), 2, 1), _lib.WW_EINVAL, "out of range")
        assert lib.ww_stream_set_rate(bank._h, _lib.ptr(np.array([1, 5], np.int32)), 2, 1) == _lib.WW_OK
        fs, fo = _layout(bank)
        assert fs.tolist() == [960, 320, 960, 960, 960, 320, 960] and fo[-1] == 5 * 960 + 2 * 320
    finally:
        bank.close()
    ticked = StreamBank(eng, S)
    try:
        ticked.step(np.zeros((S, 320), np.int16), np.ones(S, np.uint8))
        refused(attach(ticked, [rs[48000], None]), _lib.WW_ESTATE, "ticked")
        fs, fo = _layout(ticked)  # a plain bank: the uniform layout
        assert fs.tolist() == [320] * S and fo.tolist() == [320 * s for s in range(S + 1)]
    finally:
        ticked.close()
    b48 = StreamBank(eng, S, sample_rate=48000)
    try:
        refused(attach(b48, [rs[48000], None]), _lib.WW_EINVAL, "already has a resampler")
        fs, fo = _layout(b48)  # a single-rate bank: the uniform layout
        assert fs.tolist() == [960] * S and fo.tolist() == [960 * s for s in range(S + 1)]
        with pytest.raises(ValueError, match="runs at one rate"):
            b48.set_rate([0], 48000)
    finally:
        b48.close()
    for r in list(rs.values()) + [rs48b]:
        r.close()
