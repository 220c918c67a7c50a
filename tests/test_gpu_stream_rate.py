"""Stream banks at another rate than 16 kHz on the MI355X (``ww_stream_attach_resampler``, ``StreamBank(sample_rate=...)``).

The contract (include/wwhip.h): a bank at rate R yields, for every stream and every call, THE BITS of the same bank at 16 kHz given
``z = concat(zeros(D), y)``, ``y`` the one-shot int16 output of the resampler for the stream's samples (frames of frozen ticks left
out, a new signal after every reset), ``D = ceil(half / down)``.  The oracle is public API only: ``Resampler(rate)(x, np.int16)`` per
stream, ``z`` cut into 320-sample frames (or fed as one packet) to a 16 kHz bank of the same model, flags and front end.  Every
comparison is BIT FOR BIT (``np.array_equal`` on the float32 posteriors' integer views, on ``n_post``, on ``bank.window(s)``): the
tick kernels are the same code on the same int16 input, no tolerance is involved.

Shapes: S = 5 streams, 40 ticks (the 512-sample ring fills, ticks of one and of two frames, past the CRNN's first windows); seeded
noise plus a tone at about 0.3 of full scale, stream 0 a full-scale +-32767 square (the int16 clamp is hit), stream 4 all zeros
(stream 3 in the feed test, where stream 4 is the one that is ticked).
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from stream_rate_pairs import S, TICKS  # noqa: E402

pytestmark = pytest.mark.gpu

RATES = [48000, 44100, 8000]
FORMS = {"crnn": ("CRNN", {}), "crnn_two_launch_sync": ("CRNN", dict(two_launch=True, sync_wait=True)), "wavenet": ("Wavenet", {}),
         "causal": ("Wavenet", dict(causal=True))}
SET_MEMBERS = ["CRNN_nosilence", "CRNN_nosilence_enhanced"]


@pytest.fixture(scope="module")
def engines(assets):
    from wwhip.engine import Engine
    out = {m: Engine(os.path.join(assets, m)) for m in ["CRNN", "Wavenet"] + SET_MEMBERS}
    yield out
    for e in out.values():
        e.close()


# the signals, the oracle's z and the tick-by-tick run: shared with tests/test_gpu_stream_rate_geometries.py
from stream_rate_pairs import bits as _bits, resampler as _resampler, run_pair as _run_pair, same_windows as _same_windows  # noqa: E402
from stream_rate_pairs import same_tick as _same_tick, signals as _signals, z_of as _z  # noqa: E402


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("rate", RATES)
def test_rate_bank_equals_the_16k_bank_given_z(engines, rate, form):
    """48000 (up == 1), 44100 (general phase, up = 160) and 8000 (upsampling) through the incremental CRNN's one-launch polled bank,
    its two-launch form with the runtime's wait, the Wavenet window bank and the causal bank."""
    from wwhip.engine import StreamBank
    model, kw = FORMS[form]
    eng = engines[model]
    rs = _resampler(rate, eng.ctx)
    bank_r, bank_16 = StreamBank(eng, S, sample_rate=rate, **kw), StreamBank(eng, S, **kw)
    try:
        assert bank_r.sample_rate == rate and bank_r.frame_samples == rate // 50 and bank_16.frame_samples == 320 and bank_16.sample_rate == 16000
        seen = _run_pair(bank_r, bank_16, rs, _signals(rate))
        assert seen >= S * (2 * TICKS - 4)  # every stream delivered its windows: 77 rows in 40 ticks
    finally:
        bank_r.close()
        bank_16.close()


@pytest.mark.parametrize("form", ["crnn", "causal"])
@pytest.mark.parametrize("rate", [48000, 44100])
def test_flags_freeze_and_reset(engines, rate, form):
    """Stream 1 has is_speech off for ticks 10-19 (its samples still count), stream 2 is frozen for ticks 12-17 (the oracle's x
    leaves those frames out: the resampling state stood still), stream 3 is reset after tick 20 (a new x, a new z with D zeros)."""
    from wwhip.engine import StreamBank
    model, kw = FORMS[form]
    eng = engines[model]
    rs = _resampler(rate, eng.ctx)
    speech, active = np.ones((TICKS, S), np.uint8), np.zeros((TICKS, S), np.uint8)
    speech[10:20, 1] = 0
    active[12:18, 2] = 1
    bank_r, bank_16 = StreamBank(eng, S, sample_rate=rate, resampler=rs, **kw), StreamBank(eng, S, **kw)
    try:
        _run_pair(bank_r, bank_16, rs, _signals(rate), speech, active, reset_after={20: [3]})
    finally:
        bank_r.close()
        bank_16.close()


def test_model_set_bank_at_44100(engines):
    """A ModelSet of two CRNNs at 44100, streams dealt [0, 1, 0, 1, 1], stream 2 moved to member 1 after tick 15 (set_model resets
    it, the resampling state included) - against the same set bank at 16 kHz."""
    from wwhip.engine import ModelSet, StreamBank
    ms = ModelSet([engines[m] for m in SET_MEMBERS])
    rs = _resampler(44100, ms.ctx)
    deal = [0, 1, 0, 1, 1]
    bank_r, bank_16 = StreamBank(ms, S, models=deal, sample_rate=44100), StreamBank(ms, S, models=deal)
    try:
        _run_pair(bank_r, bank_16, rs, _signals(44100), set_model_after={15: ([2], 1)})
    finally:
        bank_r.close()
        bank_16.close()
        ms.close()


def _rows_of(fill, k):
    tot = fill + k
    rows = (tot - 512) // 160 + 1 if tot >= 512 else 0
    return rows, tot - 160 * rows


@pytest.mark.parametrize("rate", [44100, 8000])
def test_feed_at_the_banks_rate(engines, rate):
    """A causal bank at the bank's rate, 1.0 s per stream cut into ticks, packets and ticks again - the history the tick's kernel
    writes is read by the feed's splice, and the one the splice writes by a tick at a sample count that is no multiple of the frame:
      1. stream 4 (noise here: the zero stream is stream 3) advances by ticks for its first 10 frames, the others frozen meanwhile;
      2. every stream receives ONE sample - at 44100 that completes no 16 kHz sample: only the resampling state moves;
      3. random packets of 1 .. 3000 samples up to 2 frames + 7 samples before the end;
      4. two ticks of all streams (at 44100 with N up mod down != 0), 5. the last 7 samples as a packet.
    Oracle: a 16 kHz causal bank's feed of z[: floor(N up / down)] in one packet.  Posteriors, mel rows and ww_stream_feed_rows'
    prediction (which touches no state) equal bit for bit."""
    from wwhip import _lib
    from wwhip.engine import StreamBank
    eng = engines["Wavenet"]
    rs = _resampler(rate, eng.ctx)
    x = _signals(rate, 1.0)[[0, 1, 2, 4, 3]]  # stream 4 carries noise + tone, stream 3 the zeros
    assert x[4].any() and not x[3].any()
    N, F, T = x.shape[1], rate // 50, eng.window
    lib = _lib.load()
    rng = np.random.default_rng(rate + 1)
    bank_r, bank_16 = StreamBank(eng, S, causal=True, sample_rate=rate), StreamBank(eng, S, causal=True)
    posts, mels = [[] for _ in range(S)], [[] for _ in range(S)]
    at, fill = np.zeros(S, int), np.zeros(S, int)

    def advance(s, k):
        """Stream s receives k samples: -> the rows the 16 kHz framing rule gives for the samples of z they complete."""
        adv = (at[s] + k) * rs.up // rs.down - at[s] * rs.up // rs.down
        r, fill[s] = _rows_of(fill[s], adv)
        at[s] += k
        return r, adv

    def tick(active):
        p, n = bank_r.step(np.stack([x[s, at[s]:at[s] + F] for s in range(S)]), np.ones(S, np.uint8), active)
        for s in range(S):
            if active[s]:
                assert n[s] == 0
                continue
            r, adv = advance(s, F)
            assert adv == 320 and n[s] == r, (s, adv, n[s], r)
            posts[s] += [p[s, k] for k in range(r)]
            if r:
                mels[s].append(bank_r.window(s)[T - r:].copy())

    def feed(ids, ks):
        pk = [x[s, at[s]:at[s] + k] for s, k in zip(ids, ks)]
        a_ids, offs, row_offs = np.asarray(ids, np.int32), np.zeros(len(ids) + 1, np.int64), np.zeros(len(ids) + 1, np.int64)
        np.cumsum(ks, out=offs[1:])
        assert lib.ww_stream_feed_rows(bank_r._h, _lib.ptr(a_ids), len(ids), _lib.ptr(offs), _lib.ptr(row_offs)) == 0
        want = [advance(s, k) for s, k in zip(ids, ks)]
        assert np.diff(row_offs).tolist() == [r for r, _ in want]
        p, m = bank_r.feed(ids, pk, want_mel=True)
        for i, s in enumerate(ids):
            assert len(p[i]) == want[i][0] and m[i].shape == (want[i][0], eng.n_mel)
            posts[s] += list(p[i])
            mels[s].append(m[i])
        return [adv for _, adv in want]

    try:
        for t in range(10):  # 1. stream 4 by ticks, the others frozen (their frames are dropped whole)
            tick(np.array([1, 1, 1, 1, 0], np.uint8))
        assert at.tolist() == [0, 0, 0, 0, 10 * F] and len(posts[4]) == 17
        adv = feed(list(range(S)), [1] * S)  # 2.
        if rate == 44100:
            assert adv == [0] * S  # no sample of z: the call moved the resampling state and nothing else
        stop = N - 2 * F - 7
        while (at < stop).any():  # 3.
            ids = [s for s in range(S) if at[s] < stop and rng.random() < 0.6]
            if ids:
                feed(ids, [min(int(rng.integers(1, 3001)), stop - at[s]) for s in ids])
        if rate == 44100:
            assert (stop * rs.up) % rs.down != 0  # the ticks' outputs do not start on an input sample
        for t in range(2):  # 4.
            tick(np.zeros(S, np.uint8))
        feed(list(range(S)), [7] * S)  # 5.
        assert (at == N).all()
        z = [_z(rs, x[s]) for s in range(S)]
        assert all(len(v) == 16000 for v in z)
        p16, m16 = bank_16.feed(list(range(S)), z, want_mel=True)
        for s in range(S):
            assert len(posts[s]) == len(p16[s]) == 97  # (16000 - 512) // 160 + 1
            assert np.array_equal(_bits(posts[s]), _bits(p16[s])), ("posteriors of stream", s)
            assert np.array_equal(_bits(np.concatenate(mels[s])), _bits(m16[s])), ("mel rows of stream", s)
        _same_windows(bank_r, bank_16, "after the feeds")
    finally:
        bank_r.close()
        bank_16.close()


def test_pipeline_bank_at_48000(engines):
    """SpeechPipelineBank([VadBank, WakewordBank, ActivationTimeoutBank]) (ww_pipeline_bank_step) on a 48000 bank against the same
    stages on the 16 kHz bank given z: the fired / fall / deactivated ids tick by tick, the flags and the posteriors.  The VAD's raw
    decisions are given, its classifier sees the frames at the bank's rate.  z follows what the 48000 pipeline did: frames of ticks
    a stream was active in are left out, a VAD fall resets the stream (a new x)."""
    from wwhip.activation_timeout import ActivationTimeoutBank
    from wwhip.engine import StreamBank
    from wwhip.pipeline import SpeechPipelineBank
    from wwhip.vad import VadBank
    from wwhip.wakeword import WakewordBank
    rate, F = 48000, 960
    eng = engines["CRNN"]
    rs = _resampler(rate, eng.ctx)
    x = _signals(rate)
    rng = np.random.default_rng(5)
    raw = np.ones((TICKS, S), bool)
    for s in range(S):  # speech with a pause somewhere in the second half: one fall per stream
        a = int(rng.integers(18, 30))
        raw[a:a + 5, s] = False
    kw_vad = dict(frame_width=20, vad_rise_delay=40, vad_fall_delay=60)
    kw_to = dict(frame_width=20, min_active=60, max_active=200)
    # a threshold that some streams cross and some do not: the median of the streams' largest posteriors over ticks 3 .. 14 of a
    # plain run - in the pipeline every stream is in speech and none has fallen or fired by then, so it sees these posteriors
    # until one crosses: the streams above the median fire, the others have not by tick 15
    probe = StreamBank(eng, S, sample_rate=rate, resampler=rs)
    top = np.zeros(S, np.float32)
    for t in range(15):
        p, n = probe.step(x[:, t * F:(t + 1) * F], np.ones(S, np.uint8))
        for s in range(S):
            if t >= 3:
                top[s] = max([top[s]] + [p[s, k] for k in range(n[s])])
    probe.close()
    thr = float(np.median(top))
    print("pipeline: largest posteriors of ticks 3 .. 14", top, "threshold", thr)
    assert (top > thr).any()

    class Source:
        def __init__(self, frames):
            self.frames, self.t = frames, 0

        def read(self):
            self.t += 1
            return self.frames(self.t - 1)

        def start(self):
            pass

        def stop(self):
            pass

        def close(self):
            pass

    def run(bank, frames, width):
        src = Source(frames)
        seen = []

        def classify(f):
            seen.append(np.shape(f))
            return raw[src.t - 1]
        vad, wake, to = VadBank(S, classifier=classify, **kw_vad), WakewordBank(S, posterior_threshold=thr, bank=bank), ActivationTimeoutBank(S, **kw_to)
        pipe = SpeechPipelineBank(src, [vad, wake, to], S)
        assert pipe._fused is not None
        ps = pipe._fused[0]
        pipe.start()
        log = []
        for t in range(TICKS):
            before = pipe.context.is_active.astype(bool).copy()
            pipe.step()
            log.append(dict(active_before=before, fired=sorted(wake._fired[:ps.n_fired].tolist()), fall=sorted(wake._fall[:ps.n_fall].tolist()),
                            deact=sorted(to._ids[:ps.n_deact].tolist()), speech=pipe.context.is_speech.astype(bool).copy(),
                            active=pipe.context.is_active.astype(bool).copy(), post=wake._post.copy(), n=wake._n.copy()))
            yield log[-1]
        assert seen == [(S, width)] * TICKS
        pipe.stop()
        pipe.cleanup()

    bank_r = StreamBank(eng, S, sample_rate=rate, resampler=rs)
    logs_r = list(run(bank_r, lambda t: x[:, t * F:(t + 1) * F], F))
    # the oracle's z from what the 48000 pipeline did
    z_frames = np.zeros((TICKS, S, 320), np.int16)
    for s in range(S):
        cuts = sorted({0, TICKS} | {t + 1 for t in range(TICKS) if s in logs_r[t]["fall"]})
        for a, b in zip(cuts[:-1], cuts[1:]):
            live = [t for t in range(a, b) if not logs_r[t]["active_before"][s]]
            if live:
                z = _z(rs, np.concatenate([x[s, t * F:(t + 1) * F] for t in live]))
                for i, t in enumerate(live):
                    z_frames[t, s] = z[i * 320:(i + 1) * 320]
    bank_16 = StreamBank(eng, S)
    logs_16 = list(run(bank_16, lambda t: z_frames[t], 320))
    for t, (a, b) in enumerate(zip(logs_r, logs_16)):
        assert a["fired"] == b["fired"] and a["fall"] == b["fall"] and a["deact"] == b["deact"], (t, a, b)
        assert np.array_equal(a["speech"], b["speech"]) and np.array_equal(a["active"], b["active"]), t
        _same_tick((a["post"], a["n"]), (b["post"], b["n"]), ("pipeline tick", t))
    assert sum(len(a["fall"]) for a in logs_r) >= S  # every stream's VAD fell once
    fired = sorted(s for a in logs_r for s in a["fired"])
    print("pipeline: fired", fired, "deactivated", sorted(s for a in logs_r for s in a["deact"]))
    assert set(fired) >= set(np.flatnonzero(top > thr).tolist())


def test_refusals_and_frame_samples(engines):
    """Through ctypes: ww_stream_frame_samples before and after the attach; a second attach, 11025 Hz, 16000 -> 16000, an output
    rate of 8000 and a resampler of another context are WW_EINVAL with the reason in ww_last_error; an attach after a tick is
    WW_ESTATE.  In Python: frames of the wrong shape."""
    from wwhip import _lib
    from wwhip.engine import StreamBank
    from wwhip.resample import Resampler
    eng = engines["CRNN"]
    lib, ctx = _lib.load(), eng.ctx
    rs48 = _resampler(48000, ctx)

    def frame_samples(bank):
        n = C.c_int32(-1)
        assert lib.ww_stream_frame_samples(bank._h, C.byref(n)) == _lib.WW_OK
        return n.value

    def refused(bank, r, code, word):
        assert lib.ww_stream_attach_resampler(bank._h, r._h) == code
        text = lib.ww_last_error(ctx.handle).decode()
        assert word in text, text

    other = _lib.Context()
    made = [Resampler(11025, 16000, ctx), Resampler(16000, 16000, ctx), Resampler(48000, 8000, ctx), Resampler(48000, 16000, other)]
    bank = StreamBank(eng, S)
    try:
        assert frame_samples(bank) == 320
        refused(bank, made[0], _lib.WW_EINVAL, "fractional")
        refused(bank, made[1], _lib.WW_EINVAL, "plain bank")
        refused(bank, made[2], _lib.WW_EINVAL, "output rate")
        refused(bank, made[3], _lib.WW_EINVAL, "another context")
        assert frame_samples(bank) == 320
        assert lib.ww_stream_attach_resampler(bank._h, rs48._h) == _lib.WW_OK
        assert frame_samples(bank) == 960
        refused(bank, rs48, _lib.WW_EINVAL, "already")
        assert lib.ww_stream_attach_resampler(bank._h, None) == _lib.WW_EINVAL
    finally:
        bank.close()
    ticked = StreamBank(eng, S)
    try:
        ticked.step(np.zeros((S, 320), np.int16), np.ones(S, np.uint8))
        refused(ticked, rs48, -5, "ticked")  # WW_ESTATE
        assert frame_samples(ticked) == 320
    finally:
        ticked.close()
    b48 = StreamBank(eng, S, sample_rate=48000, resampler=rs48)
    try:
        with pytest.raises(ValueError, match=r"\[5, 960\] int16"):
            b48.step(np.zeros((S, 320), np.int16), np.ones(S, np.uint8))
        with pytest.raises(ValueError, match="fractional"):
            StreamBank(eng, S, sample_rate=11025)
        with pytest.raises(ValueError, match="causal|CAUSAL"):
            b48.feed([0], [np.zeros(100, np.int16)])  # (a window bank cannot be fed, at any rate)
    finally:
        b48.close()
    for r in made:
        r.close()
    other.close()
