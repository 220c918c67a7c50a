"""What the tests of stream banks at another rate than 16 kHz share (tests/test_gpu_stream_rate.py,
tests/test_gpu_stream_rate_geometries.py): the streams' signals, the oracle's 16 kHz signal z, and the tick-by-tick run of a bank at
rate R beside the 16 kHz bank given z.

The contract (include/wwhip.h): a bank at rate R yields, for every stream and every call, THE BITS of the same bank at 16 kHz given
``z = concat(zeros(D), y)``, ``y`` the one-shot int16 output of the resampler for the stream's samples (frames of frozen ticks left
out, a new signal after every reset), ``D = ceil(half / down)``.  Every comparison is BIT FOR BIT (``np.array_equal`` on the float32
posteriors' integer views, on ``n_post``, on ``bank.window(s)``)."""
import numpy as np

S, TICKS = 5, 40

_rs_cache = {}


def resampler(rate, ctx):
    """One resampler per rate for the whole run (the oracle's and, where a test passes it on, the bank's)."""
    from wwhip.resample import Resampler
    r = _rs_cache.get(rate)
    if r is None or r._h is None or r.ctx is not ctx:
        r = _rs_cache[rate] = Resampler(rate, 16000, ctx)
    return r


_sig_cache = {}


def signals(rate, seconds=TICKS / 50):
    """[S, n] int16 at ``rate``, computed once per rate and length and never written to: stream 0 a full-scale +-32767 square (the
    int16 clamp is hit), streams 1 - 3 a tone plus seeded noise at about 0.3 of full scale, stream 4 all zeros."""
    key = (rate, seconds)
    if key not in _sig_cache:
        n = int(round(rate * seconds))
        rng = np.random.default_rng(rate)
        t = np.arange(n) / rate
        x = np.zeros((S, n), np.int16)
        x[0] = np.where((np.arange(n) // 23) % 2 == 0, 32767, -32767)
        for s in (1, 2, 3):
            tone = 0.25 * 32768 * np.sin(2 * np.pi * (300.0 + 170.0 * s) * t)
            x[s] = np.clip(np.rint(tone + rng.normal(0, 0.08 * 32768, n)), -32768, 32767)
        x.setflags(write=False)
        _sig_cache[key] = x
    return _sig_cache[key]


def delay(rs):
    return -(-rs.half // rs.down)


def z_of(rs, x):
    """The stream's 16 kHz signal for the samples ``x``: D zeros, then the one-shot's int16 output, as far as ``x`` determines what
    the bank consumes - floor(N up / down) samples."""
    n = len(x) * rs.up // rs.down
    if len(x) == 0:
        return np.zeros(0, np.int16)
    y = rs(np.ascontiguousarray(x), dtype=np.int16)
    return np.concatenate((np.zeros(delay(rs), np.int16), y))[:n]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_tick(got, want, what):
    (p, n), (q, m) = got, want
    assert np.array_equal(n, m), (what, n, m)
    assert np.array_equal(bits(p), bits(q)), (what, p, q)


def same_windows(a, b, what, n_streams=S):
    for s in range(n_streams):
        assert np.array_equal(bits(a.window(s)), bits(b.window(s))), (what, "window of stream", s)


def run_pair(bank_r, bank_16, rs, x, speech=None, active=None, reset_after=None, set_model_after=None, ticks=TICKS):
    """``x`` [streams, ticks * F] through ``bank_r`` tick by tick, and the oracle's z through ``bank_16`` with the same flags, resets and
    member moves; every tick's posteriors and counts and the final windows compared.  The oracle's x leaves out the frames of
    frozen ticks and starts anew after a reset.  -> the number of posteriors seen."""
    F = bank_r.frame_samples
    n_streams = x.shape[0]
    ones = np.ones(n_streams, np.uint8)
    # the oracle's 16 kHz frames, stream by stream: per signal (between resets) the unfrozen frames, resampled in one shot
    z_frames = np.zeros((ticks, n_streams, 320), np.int16)
    for s in range(n_streams):
        cuts = [0] + [t + 1 for t, ids in (reset_after or {}).items() if s in ids] + [t + 1 for t, (ids, _) in (set_model_after or {}).items() if s in ids]
        cuts = sorted(set(cuts)) + [ticks]
        for a, b in zip(cuts[:-1], cuts[1:]):
            live = [t for t in range(a, b) if active is None or not active[t][s]]
            if not live:
                continue
            z = z_of(rs, np.concatenate([x[s, t * F:(t + 1) * F] for t in live]))
            assert len(z) == 320 * len(live)
            for i, t in enumerate(live):
                z_frames[t, s] = z[i * 320:(i + 1) * 320]
    seen = 0
    for t in range(ticks):
        sp = ones if speech is None else speech[t]
        ac = None if active is None else active[t]
        got = bank_r.step(x[:, t * F:(t + 1) * F], sp, ac)
        want = bank_16.step(z_frames[t], sp, ac)
        same_tick(got, want, ("tick", t))
        seen += int(got[1].sum())
        if reset_after and t in reset_after:
            bank_r.reset(reset_after[t])
            bank_16.reset(reset_after[t])
        if set_model_after and t in set_model_after:
            bank_r.set_model(*set_model_after[t])
            bank_16.set_model(*set_model_after[t])
    same_windows(bank_r, bank_16, "after the last tick", n_streams)
    return seen
