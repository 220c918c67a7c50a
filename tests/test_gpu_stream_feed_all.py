"""The feed of a causal bank that runs EVERY listed member of a model set on EVERY stream (``ww_stream_feed_all``,
``StreamBank.feed_all``).

The contract (include/wwhip.h): slot j of stream s yields, BIT FOR BIT, what ``ww_stream_feed`` yields on an ordinary causal bank of
member ``members[j]`` alone, given the same packets, resets and ticks - however a stream's samples are cut into ``feed_all`` packets,
calls and ``step`` ticks.  The yardstick throughout is therefore public API only: the ordinary causal banks
``StreamBank(Engine(member), S, causal=True)`` given the same packets through ``feed`` (tests/test_gpu_stream_feed.py holds those
against float64, so nothing is compared with float64 a second time here).  Every comparison is ``np.array_equal``.

Members: ``Wavenet`` (0) and ``Wavenet_alt`` (1), the shipped files as they are."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

WAVES = ["Wavenet", "Wavenet_alt"]


@pytest.fixture(scope="module")
def engines(assets):
    from wwhip.engine import Engine
    out = {m: Engine(os.path.join(assets, m)) for m in WAVES}
    yield out
    for e in out.values():
        e.close()


@pytest.fixture(scope="module")
def wave_set(engines):
    from wwhip.engine import ModelSet
    ms = ModelSet([engines[m] for m in WAVES])
    yield ms
    ms.close()


def _pcm(rng, n, rate=16000):
    t = np.arange(n) / float(rate)
    chirp = 8000.0 * np.sin(2 * np.pi * (200.0 * t + 0.5 * 3800.0 / 1.5 * np.mod(t, 1.5) * np.mod(t, 1.5)))
    return np.clip(np.rint(rng.normal(0, 2000, n) + chirp), -32768, 32767).astype(np.int16)


def _fp(precise):
    from wwhip.engine import frontend_params
    return frontend_params(precise=precise)


def _own(engines, m, S, fp=None, **kw):
    """The ordinary causal bank of member m."""
    from wwhip.engine import StreamBank
    return StreamBank(engines[WAVES[m]], S, fp, causal=True, **kw)


def _every(wave_set, S, members, fp=None, **kw):
    from wwhip.engine import StreamBank
    return StreamBank(wave_set, S, fp, causal=True, members=members, **kw)


def _cat(parts, width):
    parts = [p for p in parts if len(p)]
    return np.concatenate(parts) if parts else np.zeros((0, width), np.float32)


# ------------------------------------------------------------------------------------------ 1. any split gives the members' bits
S1, N1, MEMBERS1 = 5, 12800, [1, 0, 1]


@pytest.fixture(scope="module")
def split_refs(engines):
    """Per front-end precision: the samples, and per member its own bank's posteriors [rows] and mel rows [rows, 40] per stream, each
    stream fed as ONE packet - computed once, left unchanged."""
    out = {}
    for precise in (True, False):
        rng = np.random.default_rng(71 + precise)
        pcm = [_pcm(rng, N1) for _ in range(S1)]
        refs = {}
        for m in sorted(set(MEMBERS1)):
            bank = _own(engines, m, S1, _fp(precise))
            try:
                refs[m] = bank.feed(list(range(S1)), pcm, want_mel=True)
            finally:
                bank.close()
        out[precise] = (pcm, refs)
    return out


def _cuts(rng):
    """Per stream the events that bring its 12,800 samples: ("feed", samples) or ("tick", 320 samples)."""
    ev = [[("feed", 160)] * (N1 // 160), [("feed", 320)] * (N1 // 320), [], [("feed", N1)], []]
    left = N1
    while left:
        k = min(left, int(rng.integers(37, 701)))
        ev[2].append(("feed", k))
        left -= k
    left, tick = N1, True
    while left:
        k = 320 if tick and left >= 320 else min(left, int(rng.integers(37, 701)))
        ev[4].append(("tick" if tick and left >= 320 else "feed", k))
        left -= k
        tick = not tick
    return ev


@pytest.mark.parametrize("precise", [True, False], ids=["fe_fp64", "fe_fp32"])
@pytest.mark.parametrize("sync_wait", [False, True], ids=["polled", "waited"])
def test_any_split_gives_the_members_bits(wave_set, split_refs, sync_wait, precise):
    """S = 5, members [1, 0, 1], 12,800 samples per stream: stream 0 in 160-sample packets, 1 in 320, 2 in ragged 37..700-sample
    packets, 3 as one packet, 4 as alternating ``step`` ticks (all flags speech; the other streams are not sampled in that tick) and
    ``feed_all`` packets; the streams' r-th packets share call r.  ``posts[i][:, j]`` and ``mels[i]`` equal the own bank of member
    ``members[j]``; a pure ``step`` loop over the same samples on a twin every-member bank gives the same posteriors."""
    pcm, refs = split_refs[precise]
    ev = _cuts(np.random.default_rng(5))
    K = len(MEMBERS1)
    bank = _every(wave_set, S1, MEMBERS1, _fp(precise), sync_wait=sync_wait)
    twin = _every(wave_set, S1, MEMBERS1, _fp(precise), sync_wait=sync_wait)
    try:
        posts, mels, at = [[] for _ in range(S1)], [[] for _ in range(S1)], [0] * S1
        for r in range(max(len(e) for e in ev)):
            ids, pk = [], []
            for s in range(S1):
                if r >= len(ev[s]):
                    continue
                kind, k = ev[s][r]
                x = pcm[s][at[s]:at[s] + k]
                at[s] += k
                if kind == "feed":
                    ids.append(s)
                    pk.append(x)
                else:  # a tick that samples stream s alone: the others are active, i.e. not sampled at all
                    frames = np.zeros((S1, 320), np.int16)
                    frames[s] = x
                    active = np.ones(S1, np.uint8)
                    active[s] = 0
                    p, n = bank.step(frames, np.ones(S1, np.uint8), active)
                    assert n.sum() == n[s]
                    posts[s].append(p[s, :, :n[s]].T.copy())  # [rows, K]
                    w = bank.window(s)
                    mels[s].append(w[len(w) - n[s]:])  # (the tick's new rows are the window's newest)
            if ids:
                po, me = bank.feed_all(ids, pk, want_mel=True)
                for i, s in enumerate(ids):
                    assert po[i].shape == (len(me[i]), K)
                    posts[s].append(po[i])
                    mels[s].append(me[i])
        assert at == [N1] * S1
        ticks = []
        for t in range(N1 // 320):
            p, n = twin.step(np.stack([x[t * 320:(t + 1) * 320] for x in pcm]), np.ones(S1, np.uint8))
            ticks.append((p, n))
        for s in range(S1):
            got_p, got_m = _cat(posts[s], K), _cat(mels[s], 40)
            assert len(got_p) == (N1 - 512) // 160 + 1
            for j, m in enumerate(MEMBERS1):
                assert np.array_equal(got_p[:, j], refs[m][0][s]), f"stream {s} slot {j} (member {m}) differs from that member's own bank"
                assert np.array_equal(got_m, refs[m][1][s]), f"stream {s}: mel rows differ from member {m}'s own bank"
            stepped = _cat([p[s, :, :n[s]].T for p, n in ticks], K)
            assert np.array_equal(stepped, got_p), f"stream {s}: a pure step loop differs"
        assert np.array_equal(_cat(posts[0], K)[:, 0], _cat(posts[0], K)[:, 2]) and not np.array_equal(_cat(posts[0], K)[:, 0], _cat(posts[0], K)[:, 1])
    finally:
        bank.close()
        twin.close()


# ---------------------------------------------------------------------------------- 2. every launch form, and the state it leaves
ROWS2 = [1, 2, 16, 17, 191, 192, 193, 400]


def _forms_script(rng):
    first = [_pcm(rng, 512 + 160 * (r - 1)) for r in ROWS2]
    one_row = [_pcm(rng, 160) for _ in ROWS2]
    ticks = [np.stack([_pcm(rng, 320) for _ in ROWS2]) for _ in range(3)]
    return first, one_row, ticks


def _forms_run(bank, script, feed):
    first, one_row, ticks = script
    S = len(ROWS2)
    a = feed(list(range(S)), first, want_mel=True)
    b = feed(list(range(S)), one_row, want_mel=True)
    t = [bank.step(f, np.ones(S, np.uint8)) for f in ticks]
    return a, b, t


@pytest.fixture(scope="module")
def forms_refs(engines):
    script = _forms_script(np.random.default_rng(83))
    refs = {}
    for m in (0, 1):
        bank = _own(engines, m, len(ROWS2))
        try:
            refs[m] = _forms_run(bank, script, bank.feed)
        finally:
            bank.close()
    return script, refs


@pytest.mark.parametrize("segment", [0, 191, 256, 64])
def test_every_launch_form_and_the_state_it_leaves(wave_set, forms_refs, segment):
    """ONE call whose streams bring [1, 2, 16, 17, 191, 192, 193, 400] rows first - the one-wave tile and its edge at 16, the smallest
    twelve-wave case, one 192-row chunk and two, more rows than the 182-row pool, a second ``wave_feed_pool_kernel`` workgroup beyond
    256 -, then a 1-row packet and 3 ticks on every stream, which read the history and the logit ring the first call wrote.  K = 2,
    under the set's ``wave_seq_segment`` at 0, 191, 256 (400 rows in several segments) and 64 (below RF - 1: clamped)."""
    script, refs = forms_refs
    wave_set.set_option("wave_seq_segment", segment)
    bank = _every(wave_set, len(ROWS2), [0, 1])
    try:
        a, b, t = _forms_run(bank, script, bank.feed_all)
        for s, rows in enumerate(ROWS2):
            assert a[0][s].shape == (rows, 2) and b[0][s].shape == (1, 2)
            for j in (0, 1):
                ra, rb, rt = refs[j]
                assert np.array_equal(a[0][s][:, j], ra[0][s]), f"{rows} rows, slot {j}: the first call"
                assert np.array_equal(a[1][s], ra[1][s]) and np.array_equal(b[1][s], rb[1][s])
                assert np.array_equal(b[0][s][:, j], rb[0][s]), f"{rows} rows, slot {j}: the 1-row packet behind it"
                for i in range(3):
                    assert np.array_equal(t[i][1], rt[i][1])
                    assert np.array_equal(t[i][0][s, j], rt[i][0][s]), f"{rows} rows, slot {j}: tick {i} behind the feeds"
        assert sum(int(n.sum()) for _, n in t) > 0
    finally:
        bank.close()
        wave_set.set_option("wave_seq_segment", 0)


# --------------------------------------------------------------------------------------------------- 3. a subset, in any order
def test_a_subset_in_any_order(wave_set):
    """Streams [3, 0] of 5 fed on one bank, [0, 3] with the packets swapped on a twin: the same results; the unnamed streams' next
    tick equals that of a twin that was never fed."""
    rng = np.random.default_rng(91)
    S = 5
    banks = [_every(wave_set, S, [0, 1]) for _ in range(3)]
    try:
        warm = [np.stack([_pcm(rng, 320) for _ in range(S)]) for _ in range(3)]
        for b in banks:
            for f in warm:
                b.step(f, np.ones(S, np.uint8))
        p3, p0 = _pcm(rng, 5000), _pcm(rng, 777)
        x = banks[0].feed_all([3, 0], [p3, p0], want_mel=True)
        y = banks[1].feed_all([0, 3], [p0, p3], want_mel=True)
        assert len(x[0][0]) > 16 and 0 < len(x[0][1]) <= 16
        for k in (0, 1):
            assert np.array_equal(x[k][0], y[k][1]) and np.array_equal(x[k][1], y[k][0])
        f = np.stack([_pcm(rng, 320) for _ in range(S)])
        got = [b.step(f, np.ones(S, np.uint8)) for b in banks]
        assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1])
        for s in (1, 2, 4):
            assert got[2][1][s] > 0 and np.array_equal(got[0][0][s], got[2][0][s]) and got[0][1][s] == got[2][1][s]
        for s in (0, 3):
            assert not np.array_equal(got[0][0][s], got[2][0][s])
    finally:
        for b in banks:
            b.close()


# ------------------------------------------------------------------------------------------------------------- 4. other rates
def test_other_rates(engines, wave_set):
    """``sample_rate=[8000, 16000, 48000]``, K = 2, packets at each stream's own rate (a short one, one that leaves a tile's worth
    of rows, a long one, with a tick in between): equal to the members' own mixed-rate banks' ``feed``."""
    rates = [8000, 16000, 48000]
    rng = np.random.default_rng(97)
    calls = [[_pcm(rng, int(r * sec), r) for r in rates] for sec in (0.013, 0.11, 1.3)]
    tick = [_pcm(rng, r // 50, r) for r in rates]

    def run(bank, feed):
        out = [feed([0, 1, 2], calls[0], want_mel=True), feed([2, 0, 1], [calls[1][2], calls[1][0], calls[1][1]], want_mel=True)]
        step = bank.step(tick, np.ones(3, np.uint8))
        out.append(feed([0, 1, 2], calls[2], want_mel=True))
        return out, step

    bank = _every(wave_set, 3, [0, 1], sample_rate=rates)
    try:
        got, gstep = run(bank, bank.feed_all)
    finally:
        bank.close()
    for j in (0, 1):
        own = _own(engines, j, 3, sample_rate=rates)
        try:
            want, wstep = run(own, own.feed)
        finally:
            own.close()
        assert np.array_equal(gstep[1], wstep[1]) and np.array_equal(gstep[0][:, j], wstep[0])
        for g, w in zip(got, want):
            for i in range(3):
                assert np.array_equal(g[0][i][:, j], w[0][i]) and np.array_equal(g[1][i], w[1][i]), (j, i)
    assert sum(len(p) for p in got[2][0]) > 3 * 100


# -------------------------------------------------------------------------------------------------- 5. the contract through ctypes
def test_contract_through_ctypes(engines, wave_set):
    """Every refusal carries a text, leaves outputs preset to -7 untouched and leaves the bank where its twin is (the next tick is
    the twin's); n = 0, empty packets and packets that leave a stream below 512 samples are WW_OK and move no model state;
    ``ww_stream_feed_rows_all`` writes the ``row_offs`` the feed then produces and touches nothing; ``ww_stream_feed`` /
    ``ww_stream_feed_rows`` on the same bank are still refused."""
    from wwhip import _lib
    from wwhip.engine import StreamBank
    lib = _lib.load()
    h = wave_set.ctx.handle
    rng = np.random.default_rng(101)
    S, K = 4, 2
    bank, twin = _every(wave_set, S, [1, 0]), _every(wave_set, S, [1, 0])
    window_bank = StreamBank(wave_set, S, members=[1, 0])  # an every-member bank without WW_STREAM_CAUSAL
    ordinary = _own(engines, 0, S)
    set_bank = StreamBank(wave_set, S, causal=True, models=[0, 1, 0, 1])  # a set bank of one member per stream
    pcm = _pcm(rng, 6000)
    post = np.full((64, K), -7.0, np.float32)
    mel = np.full((64, 40), -7.0, np.float32)
    ro = np.full(8, -7, np.int64)

    def call(b, ids, offs, n=None, cap=64, p_pcm=pcm, p_offs=True, p_ro=True, p_post=True, p_ids=True, fn=None):
        ids, offs = np.asarray(ids, np.int32), np.asarray(offs, np.int64)
        return (fn or lib.ww_stream_feed_all)(b._h, _lib.ptr(ids) if p_ids else None, len(ids) if n is None else n,
                                              _lib.ptr(p_pcm) if p_pcm is not None else None, _lib.ptr(offs) if p_offs else None, cap,
                                              _lib.ptr(ro) if p_ro else None, _lib.ptr(post) if p_post else None, _lib.ptr(mel))

    def rows_call(b, ids, offs, out, fn=None):
        ids, offs = np.asarray(ids, np.int32), np.asarray(offs, np.int64)
        return (fn or lib.ww_stream_feed_rows_all)(b._h, _lib.ptr(ids), len(ids), _lib.ptr(offs), _lib.ptr(out))

    def tick_equal(what):
        f = np.stack([_pcm(rng, 320) for _ in range(S)])
        got, want = bank.step(f, np.ones(S, np.uint8)), twin.step(f, np.ones(S, np.uint8))
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), what

    try:
        warm = [_pcm(rng, k) for k in (700, 100, 3000)]
        for b in (bank, twin):
            b.feed_all([0, 1, 2], warm)
        huge = 160 * ((1 << 30) // K + 8)  # samples that come to more than 2^30 / K rows (and fewer than 2^30): nothing of pcm is read
        refused = [
            ("n < 0", None, lambda: call(bank, [0, 1], [0, 1000, 2000], n=-1)),
            ("id out of range", "out of range", lambda: call(bank, [0, S], [0, 1000, 2000])),
            ("negative id", "out of range", lambda: call(bank, [0, -1], [0, 1000, 2000])),
            ("named twice", "twice", lambda: call(bank, [1, 1], [0, 1000, 2000])),
            ("descending sample_offs", "descend", lambda: call(bank, [0, 1], [0, 2000, 1000])),
            ("cap_rows too small", "buffers hold", lambda: call(bank, [0, 1], [0, 3000, 6000], cap=30)),
            ("NULL pcm", "NULL", lambda: call(bank, [0, 1], [0, 1000, 2000], p_pcm=None)),
            ("NULL sample_offs", "NULL", lambda: call(bank, [0, 1], [0, 1000, 2000], p_offs=False)),
            ("NULL row_offs", "NULL", lambda: call(bank, [0, 1], [0, 1000, 2000], p_ro=False)),
            ("NULL post", "NULL", lambda: call(bank, [0, 1], [0, 1000, 2000], p_post=False)),
            ("NULL ids", "NULL", lambda: call(bank, [0, 1], [0, 1000, 2000], p_ids=False)),
            ("rows x K beyond 2^30", "2^30 posteriors", lambda: call(bank, [0], [0, huge], cap=1 << 40)),
            ("rows x K beyond 2^30 (rows)", "2^30 posteriors", lambda: rows_call(bank, [0], [0, huge], ro)),
            ("ww_stream_feed on this bank", "ww_stream_feed_all", lambda: call(bank, [0, 1], [0, 1000, 2000], fn=lib.ww_stream_feed)),
            ("ww_stream_feed_rows on this bank", "ww_stream_step_all", lambda: rows_call(bank, [0, 1], [0, 1000, 2000], ro, fn=lib.ww_stream_feed_rows)),
            ("not an every-member bank", "ww_stream_create_set_all", lambda: call(ordinary, [0, 1], [0, 1000, 2000])),
            ("not an every-member bank (rows)", "ww_stream_create_set_all", lambda: rows_call(ordinary, [0, 1], [0, 1000, 2000], ro)),
            ("a set bank of one member per stream", "ww_stream_create_set_all", lambda: call(set_bank, [0, 1], [0, 1000, 2000])),
            ("every-member without WW_STREAM_CAUSAL", "WW_STREAM_CAUSAL", lambda: call(window_bank, [0, 1], [0, 1000, 2000])),
            ("every-member without WW_STREAM_CAUSAL (rows)", "WW_STREAM_CAUSAL", lambda: rows_call(window_bank, [0, 1], [0, 1000, 2000], ro)),
        ]
        for what, word, f in refused:
            assert f() == _lib.WW_EINVAL, what
            text = lib.ww_last_error(h).decode()
            assert text and (word is None or word in text), (what, text)
            assert (post == -7.0).all() and (mel == -7.0).all() and (ro == -7).all(), what
            tick_equal(f"after the refusal: {what}")
        assert lib.ww_stream_feed_all(None, None, 0, None, None, 0, None, None, None) == _lib.WW_EINVAL
        for b in (ordinary, set_bank):  # those banks are as they were: their own feed works
            assert len(b.feed([0], [pcm[:2000]])[0][0]) > 0
        p, n = window_bank.step(np.zeros((S, 320), np.int16), np.ones(S, np.uint8))
        assert p.shape == (S, K, 2)
        # ---- n = 0, empty packets, packets that complete no row: WW_OK, no model state moves
        assert call(bank, [], [0], n=0) == _lib.WW_OK and ro[0] == 0
        assert call(bank, [0, 3], [5, 5, 5]) == _lib.WW_OK and list(ro[:3]) == [0, 0, 0]
        assert (post == -7.0).all() and (mel == -7.0).all()
        tick_equal("after the empty calls")
        bank.reset([3])
        twin.reset([3])
        assert call(bank, [3], [0, 511]) == _lib.WW_OK and list(ro[:2]) == [0, 0] and (post == -7.0).all()
        got = bank.feed_all([3], [pcm[511:512]], want_mel=True)        # the 512th sample completes row 0
        want = twin.feed_all([3], [pcm[:512]], want_mel=True)
        assert got[0][0].shape == (1, K) and np.array_equal(got[0][0], want[0][0]) and np.array_equal(got[1][0], want[1][0])
        tick_equal("after the packets below 512 samples")
        # ---- ww_stream_feed_rows_all: the row_offs the feed then writes, and nothing moves
        ids, offs = [2, 1, 0], [0, 1234, 1234, 6000]
        ro2 = np.full(4, -7, np.int64)
        assert rows_call(bank, ids, offs, ro2) == _lib.WW_OK and rows_call(bank, ids, offs, ro2) == _lib.WW_OK
        assert call(bank, ids, offs) == _lib.WW_OK
        assert list(ro[:4]) == list(ro2) and ro2[3] > 30 and (post[:ro2[3]] != -7.0).all() and (post[ro2[3]:] == -7.0).all()
        w = twin.feed_all(ids, [pcm[:1234], pcm[:0], pcm[1234:6000]])
        assert np.array_equal(post[:ro2[3]], np.concatenate(w[0]))
        tick_equal("after the counted feed")
    finally:
        for b in (bank, twin, window_bank, ordinary, set_bank):
            b.close()
