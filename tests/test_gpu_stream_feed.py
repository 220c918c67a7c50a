"""``StreamBank.feed`` on the MI355X: a causal bank advanced by any subset of its streams and any number of samples for each.

SAME BITS (``assert_array_equal``, nothing sampled): however a stream's samples are cut into packets, calls and ``step`` ticks, the
mel rows, the posteriors and the state left behind are those of the tick loop; a feed's posteriors are ``post_frames`` of
``Engine.sequence_forward`` over the rows it returned since the stream's reset; neither the cuts of a long packet
(``wave_seq_segment``), nor a packet's neighbours in a call, nor the order of ``ids`` show.  AGAINST FLOAT64 with the bounds the
tick's forms already hold (tests/test_gpu_frontend64.py, tests/test_gpu_wave_sequence.py).  And the refusals of the contract,
each leaving the bank as a twin that never saw the refused call.  One test runs every streaming form (CRNN and Wavenet ticks
in one and two launches, the causal tick, the feed) on samples that clip, with the clip off and with another divisor.

Inputs: seeded synthetic PCM (noise + chirp), one silent stream; both Wavenet model directories.
"""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import ref64 as R
from wave_sequence64 import WaveSeq64

pytestmark = pytest.mark.gpu

MODELS = ["Wavenet", "Wavenet_alt"]
TAU = 4e-5        # fp32 posteriors: the value tests/test_gpu_wave_sequence.py holds
TAU_REL = 9e-7    # precise front end: the value tests/test_gpu_frontend64.py holds for stream windows
TAU_FFT = 1e-6    # precise=False: likewise
PACKETS = [0, 1, 37, 159, 160, 161, 319, 320, 321, 511, 512, 513, 640, 2560, 2720, 5000, 30720, 30880, 33000]


def _pcm(rng, n):
    t = np.arange(n) / 16000.0
    chirp = 8000.0 * np.sin(2 * np.pi * (200.0 * t + 0.5 * 3800.0 / 1.5 * np.mod(t, 1.5) * np.mod(t, 1.5)))
    return np.clip(np.rint(rng.normal(0, 2000, n) + chirp), -32768, 32767).astype(np.int16)


def _rows_of(fill, k):
    """The framing rule: (rows, fill') of a stream that holds ``fill`` pending samples and receives ``k``."""
    tot = fill + k
    rows = (tot - 512) // 160 + 1 if tot >= 512 else 0
    return rows, tot - 160 * rows


@pytest.fixture(scope="module")
def engines(assets):
    from wwhip.engine import Engine
    out = {m: Engine(os.path.join(assets, m)) for m in MODELS}
    yield out
    for e in out.values():
        e.close()


def _bank(eng, S, fp=None, **kw):
    from wwhip.engine import StreamBank
    return StreamBank(eng, S, fp, causal=True, **kw)


def _tick_all(bank, eng, pcm, speech=None, active=None):
    """``pcm`` [S, ticks * 320] through ``step``; per stream the new mel rows (read back through ``window`` after each tick) and
    the posteriors, in order.  ``speech`` / ``active``: [ticks, S] or None (all speech, none active)."""
    S, T = pcm.shape[0], eng.window
    ticks = pcm.shape[1] // 320
    fill = getattr(bank, "_test_fill", np.zeros(S, int))
    mels, posts = [[] for _ in range(S)], [[] for _ in range(S)]
    ones = np.ones(S, np.uint8)
    for t in range(ticks):
        sp = ones if speech is None else speech[t]
        ac = None if active is None else active[t]
        post, n = bank.step(pcm[:, t * 320:(t + 1) * 320], sp, ac)
        for s in range(S):
            if ac is not None and ac[s]:
                assert n[s] == 0
                continue
            nf, fill[s] = _rows_of(fill[s], 320)
            assert n[s] == (nf if sp[s] else 0), (t, s)
            posts[s] += [post[s, k] for k in range(n[s])]
            if nf:
                mels[s].append(bank.window(s)[T - nf:].copy())
    bank._test_fill = fill
    return mels, posts


def _feed_all(bank, pcm, rng, sizes=PACKETS):
    """``pcm`` [S, n] through ``feed``: every call a seeded random subset of the streams (probability 0.6 each), a packet size drawn
    from ``sizes`` for each, cut to what the stream has left, until every stream is through.  Rows per call are checked against the
    closed form."""
    S, N = pcm.shape
    at = np.zeros(S, int)
    fill = getattr(bank, "_test_fill", np.zeros(S, int))
    mels, posts = [[] for _ in range(S)], [[] for _ in range(S)]
    calls = 0
    while (at < N).any():
        ids = [s for s in range(S) if at[s] < N and rng.random() < 0.6]
        ks = [min(int(rng.choice(sizes)), N - at[s]) for s in ids]
        order = rng.permutation(len(ids))
        ids, ks = [ids[i] for i in order], [ks[i] for i in order]
        p, m = bank.feed(ids, [pcm[s, at[s]:at[s] + k] for s, k in zip(ids, ks)], want_mel=True)
        calls += 1
        for i, (s, k) in enumerate(zip(ids, ks)):
            rows, fill[s] = _rows_of(fill[s], k)
            assert len(p[i]) == rows and m[i].shape == (rows, 40), (s, k, rows, len(p[i]))
            posts[s] += list(p[i])
            if rows:
                mels[s].append(m[i])
            at[s] += k
    bank._test_fill = fill
    return mels, posts, calls


def _same_streams(a, b, what):
    for s, (x, y) in enumerate(zip(a, b)):
        x = np.concatenate(x) if len(x) and isinstance(x[0], np.ndarray) else np.asarray(x, np.float32)
        y = np.concatenate(y) if len(y) and isinstance(y[0], np.ndarray) else np.asarray(y, np.float32)
        np.testing.assert_array_equal(x, y, err_msg=f"{what}: stream {s}")


def _same_windows(A, B, S, what):
    for s in range(S):
        np.testing.assert_array_equal(A.window(s), B.window(s), err_msg=f"{what}: window of stream {s}")


# ------------------------------------------------------------------------------------------ 1. any split gives the tick's bits
SPLIT_CASES = [(m, sw, None) for m in MODELS for sw in (False, True)] + [("Wavenet", False, True), ("Wavenet", False, False)]


@pytest.mark.parametrize("model,sync_wait,precise", SPLIT_CASES,
                         ids=[f"{m}-{'sync_wait' if sw else 'polled'}" + ("" if p is None else f"-preemph-precise={p}") for m, sw, p in SPLIT_CASES])
def test_any_split_gives_the_ticks_bits(engines, model, sync_wait, precise):
    """128 streams x 80,000 samples (497 rows: the logit ring wraps more than twice).  Bank A: 250 ticks.  Bank B: feeds of random
    subsets with packet sizes from PACKETS.  Posteriors, mel rows and the final windows are A's bits; then both banks take 20 ticks
    with mixed ``is_speech`` and an active stretch, a reset of some ids, and a second round (A ticks, B feeds): same bits again,
    which is what shows that the state a feed leaves is the tick's."""
    from wwhip.engine import frontend_params
    eng = engines[model]
    fp = None if precise is None else frontend_params(32767, True, 0.97, 160, precise)
    S, N = 128, 80000
    rng = np.random.default_rng(7)
    pcm = np.stack([_pcm(rng, N) for _ in range(S)])
    pcm[3] = 0
    A, B = _bank(eng, S, fp, sync_wait=sync_wait), _bank(eng, S, fp)
    try:
        ma, pa = _tick_all(A, eng, pcm)
        mb, pb, calls = _feed_all(B, pcm, np.random.default_rng(11))
        assert all(len(p) == 497 for p in pa) and calls > 10
        _same_streams(pa, pb, "round 1 posteriors")
        _same_streams(ma, mb, "round 1 mel rows")
        _same_windows(A, B, S, "round 1")
        # ---- both banks tick: mixed is_speech, an active stretch
        mid = np.stack([_pcm(rng, 20 * 320) for _ in range(S)])
        speech = (rng.random((20, S)) < 0.7).astype(np.uint8)
        active = np.zeros((20, S), np.uint8)
        active[5:9, 10:40] = 1
        ma, pa = _tick_all(A, eng, mid, speech, active)
        mb, pb = _tick_all(B, eng, mid, speech, active)
        _same_streams(pa, pb, "ticks after round 1: posteriors")
        _same_streams(ma, mb, "ticks after round 1: mel rows")
        ids = list(range(0, 21)) + [S - 1]
        for bank in (A, B):
            bank.reset(ids)
            bank._test_fill[ids] = 0
        # ---- second round
        pcm2 = np.stack([_pcm(rng, 40000) for _ in range(S)])
        ma, pa = _tick_all(A, eng, pcm2)
        mb, pb, _ = _feed_all(B, pcm2, np.random.default_rng(13))
        _same_streams(pa, pb, "round 2 posteriors")
        _same_streams(ma, mb, "round 2 mel rows")
        _same_windows(A, B, S, "round 2")
    finally:
        A.close()
        B.close()


# ---------------------------------------------------------- 1b. clip off, another divisor, samples that clip: one conversion
@pytest.mark.parametrize("divisor,clip", [(32768, False), (16384, True)], ids=["div32768-noclip", "div16384-clip"])
def test_every_form_converts_the_samples_alike(engines, assets, divisor, clip):
    """The int16 -> sample conversion (division, optional clip, pre-emphasis 0.97 against the carried sample) under parameters no
    other streaming test uses: 3 streams x 12 ticks of noise with sigma 9,000 (about 7 % of the samples clip under divisor 16,384)
    and -32768 / 32767 in the first and last sample of several ticks, where the carry is taken and used.  Through the default CRNN
    bank, the CRNN bank with ``two_launch``, the default Wavenet bank, the causal bank by ``step`` and the causal bank by ``feed``
    (7 + 633 + 3,200 samples): the streams' final mel windows are the same bits in every form, the fed rows are the causal tick's,
    and stream 0's rows pass ``check_logmel`` against the float64 front end with TAU_REL (precise), as ``test_against_float64``."""
    from wwhip.engine import Engine, StreamBank, frontend_params
    S, ticks = 3, 12
    rng = np.random.default_rng(71)
    pcm = np.clip(np.rint(rng.normal(0, 9000, (S, ticks * 320))), -32768, 32767).astype(np.int16)
    for t, (first, last) in {0: (-32768, 32767), 3: (32767, -32768), 4: (-32768, -32768), 7: (32767, 32767), 11: (-32768, 32767)}.items():
        pcm[:, t * 320] = first
        pcm[:, t * 320 + 319] = last
    if clip:
        assert 0.05 < np.mean(np.abs(pcm.astype(np.int32)) > divisor) < 0.09
    fp = frontend_params(divisor, clip, 0.97, 160, True)
    wave = engines["Wavenet"]
    crnn = Engine(os.path.join(assets, "CRNN"))
    ones = np.ones(S, np.uint8)
    windows = {}

    def ticked(name, bank):
        try:
            for t in range(ticks):
                bank.step(pcm[:, t * 320:(t + 1) * 320], ones)
            windows[name] = [bank.window(s) for s in range(S)]
        finally:
            bank.close()

    try:
        ticked("crnn", StreamBank(crnn, S, fp))
        ticked("crnn two_launch", StreamBank(crnn, S, fp, two_launch=True))
        ticked("wavenet", StreamBank(wave, S, fp))
        A, B = _bank(wave, S, fp), _bank(wave, S, fp)
        try:
            rows_tick, _ = _tick_all(A, wave, pcm)
            rows_feed = [[] for _ in range(S)]
            at = 0
            for k in (7, 633, 3200):
                _, m = B.feed(list(range(S)), [pcm[s, at:at + k] for s in range(S)], want_mel=True)
                for s in range(S):
                    rows_feed[s].append(m[s])
                at += k
            assert at == pcm.shape[1]
            windows["causal step"] = [A.window(s) for s in range(S)]
            windows["causal feed"] = [B.window(s) for s in range(S)]
        finally:
            A.close()
            B.close()
    finally:
        crnn.close()
    _same_streams(rows_tick, rows_feed, "fed rows against the causal tick's")
    n_rows = _rows_of(0, pcm.shape[1])[0]
    tail = min(min(w[0].shape[0] for w in windows.values()), n_rows)  # (a CRNN window and a Wavenet window differ in length)
    assert tail >= 20
    for name, w in windows.items():
        for s in range(S):
            np.testing.assert_array_equal(w[s][-tail:], windows["causal step"][s][-tail:], err_msg=f"{name}: window of stream {s}")
            np.testing.assert_array_equal(w[s][-tail:], np.concatenate(rows_tick[s])[-tail:], err_msg=f"{name}: window of stream {s} against its rows")
    want = R.Ref64(os.path.join(assets, "Wavenet")).logmel(pcm[0], float(divisor), clip, 0.97, 160)
    got = np.asarray(np.concatenate(rows_tick[0]), np.float64)
    assert got.shape == want.y.shape == (n_rows, 40)
    print(f"\nCONVERT divisor {divisor} clip {clip}: {n_rows} rows, mel needs tau_rel {R.needed_taus(got, want, 0.0, 0.0)[0]:.2e} (tau_rel {TAU_REL:g})", end="")
    R.check_logmel(got, want, TAU_REL, 0.0)


# ------------------------------------------------------------------ 2. a feed emits the frame posteriors of the rows it returns
FIRST_ROWS = [1, 2, 16, 17, 191, 192, 193, 4097, 5997, 59997]     # (5,997 rows = a 60 s packet, 59,997 = a 10 min packet)
FOLLOW = [[160], [480, 7, 153], [160 * 16], [160 * 17, 0, 160 * 200 + 5], [160], [33000, 160], [160 * 400], [160 * 192], [1, 159], [160 * 5000]]


@pytest.mark.parametrize("model", MODELS)
def test_a_feed_emits_the_frame_posteriors_of_its_rows(engines, model):
    """Fresh streams fed 1, 2, 16, 17, 191, 192, 193, 4,097 rows in one packet, a 60 s and a 10 min packet - all in ONE call - and
    then packets that continue them: ``sequence_forward(rows returned since the reset, pool=window)["post_frames"][:, posterior
    column]`` is the concatenation of the posteriors."""
    eng = engines[model]
    rng = np.random.default_rng(21)
    S = len(FIRST_ROWS)
    first = [_pcm(rng, 512 + 160 * (r - 1)) for r in FIRST_ROWS]
    first[1][:] = 0
    bank = _bank(eng, S)
    try:
        p, m = bank.feed(list(range(S)), first, want_mel=True)
        posts, mels = [[x] for x in p], [[x] for x in m]
        fill = [0] * S
        for s, r in enumerate(FIRST_ROWS):
            assert len(p[s]) == r and m[s].shape == (r, 40)
            fill[s] = _rows_of(0, len(first[s]))[1]
        for rnd in range(max(len(f) for f in FOLLOW)):
            ids = [s for s in range(S) if rnd < len(FOLLOW[s])]
            p, m = bank.feed(ids, [_pcm(rng, FOLLOW[s][rnd]) for s in ids], want_mel=True)
            for i, s in enumerate(ids):
                rows, fill[s] = _rows_of(fill[s], FOLLOW[s][rnd])
                assert len(p[i]) == rows and m[i].shape == (rows, 40)
                posts[s].append(p[i])
                mels[s].append(m[i])
    finally:
        bank.close()
    seqs = [np.concatenate(x) for x in mels]
    pf = eng.sequence_forward(seqs, pool=eng.window, want=("post_frames",))["post_frames"]
    for s in range(S):
        got = np.concatenate(posts[s])
        assert len(got) == len(seqs[s]) >= FIRST_ROWS[s]
        np.testing.assert_array_equal(got, pf[s][:, eng.posterior_index], err_msg=f"stream {s} ({FIRST_ROWS[s]} rows first)")


# ------------------------------------------------------------------------------------------------- 3. the cuts do not show
@pytest.mark.parametrize("model", MODELS)
def test_the_cuts_do_not_show(engines, model):
    """The long packets (4,097 rows, 60 s, 10 min) followed by a 1-row packet and 5 ticks, under ``wave_seq_segment`` at 64 (below
    RF - 1: clamped), 191, 256, 1 << 20 and 0: same bits - the follow-up is what tests the history the last segment wrote."""
    eng = engines[model]
    rng = np.random.default_rng(31)
    rows = [4097, 5997, 59997]
    S = len(rows)
    first = [_pcm(rng, 512 + 160 * (r - 1)) for r in rows]
    one = [_pcm(rng, 160) for _ in range(S)]
    ticks = np.stack([_pcm(rng, 5 * 320) for _ in range(S)])
    runs = []
    for seg in (0, 64, 191, 256, 1 << 20):
        bank = _bank(eng, S)
        try:
            with eng.options(wave_seq_segment=seg):
                p, m = bank.feed(list(range(S)), first, want_mel=True)
                p1, m1 = bank.feed(list(range(S)), one, want_mel=True)
            assert [len(x) for x in p] == rows and [len(x) for x in p1] == [1] * S
            bank._test_fill = np.full(S, _rows_of(_rows_of(0, len(first[0]))[1], 160)[1])  # (352 pending samples in every stream)
            mt, pt = _tick_all(bank, eng, ticks)
            runs.append((seg, p + p1 + [np.asarray(x, np.float32) for x in pt], m + m1 + [np.concatenate(x) for x in mt] + [bank.window(s) for s in range(S)]))
        finally:
            bank.close()
    for seg, p, m in runs[1:]:
        for i, (x, y) in enumerate(zip(runs[0][1], p)):
            np.testing.assert_array_equal(x, y, err_msg=f"segment {seg}: posteriors {i}")
        for i, (x, y) in enumerate(zip(runs[0][2], m)):
            np.testing.assert_array_equal(x, y, err_msg=f"segment {seg}: mel rows {i}")


# -------------------------------------------------------------------------------- 4. neighbours and order do not show
@pytest.mark.parametrize("model", MODELS)
def test_neighbours_and_order_do_not_show(engines, model):
    """The same packets alone (one call per stream), among the other streams' packets in one call, and with ``ids`` in another
    order - two rounds, so that the state the first left is tested as well."""
    eng = engines[model]
    rng = np.random.default_rng(41)
    sizes = [[700, 160], [512 + 160 * 15, 5000], [512 + 160 * 16, 1], [40000, 2720], [3, 508], [512 + 160 * 400, 160 * 193], [0, 5000], [160 * 20, 160 * 20]]
    S = len(sizes)
    pk = [[_pcm(rng, k) for k in ks] for ks in sizes]
    banks = [_bank(eng, S) for _ in range(3)]
    try:
        out = [[[None] * S for _ in range(2)] for _ in range(3)]
        for rnd in range(2):
            for s in range(S):
                p, m = banks[0].feed([s], [pk[s][rnd]], want_mel=True)
                out[0][rnd][s] = (p[0], m[0])
            p, m = banks[1].feed(list(range(S)), [pk[s][rnd] for s in range(S)], want_mel=True)
            for s in range(S):
                out[1][rnd][s] = (p[s], m[s])
            order = [int(i) for i in np.random.default_rng(43 + rnd).permutation(S)]
            p, m = banks[2].feed(order, [pk[s][rnd] for s in order], want_mel=True)
            for i, s in enumerate(order):
                out[2][rnd][s] = (p[i], m[i])
        for b in (1, 2):
            for rnd in range(2):
                for s in range(S):
                    np.testing.assert_array_equal(out[0][rnd][s][0], out[b][rnd][s][0], err_msg=f"bank {b} round {rnd} stream {s}: posteriors")
                    np.testing.assert_array_equal(out[0][rnd][s][1], out[b][rnd][s][1], err_msg=f"bank {b} round {rnd} stream {s}: mel rows")
            _same_windows(banks[0], banks[b], S, f"bank {b}")
    finally:
        for b in banks:
            b.close()


# ------------------------------------------------------------------------------------------------------ 5. against float64
@pytest.mark.parametrize("precise", [True, False], ids=["precise", "fast"])
@pytest.mark.parametrize("model", MODELS)
def test_against_float64(engines, assets, model, precise):
    """The signal set of ``oracle.ref64.frontend_signals(3)`` fed as packets (pre-emphasis 0.97): the returned mel rows pass
    ``check_logmel`` against the float64 front end with the stream windows' bounds (TAU_REL = 9e-7 precise, TAU_FFT = 1e-6
    otherwise), the posteriors ``check_posteriors`` against ``WaveSeq64.sequence(rows)["post_frames"]`` with TAU = 4e-5.  What
    each case needed is printed.  Measured on an MI355X, worst case of the set: mel rows tau_rel 1.6e-7 (precise), tau_fft 1.2e-7
    (precise=False) - the tick's front end measured 2.2e-7 / 2.7e-7 -, posteriors tau 1.5e-6 (Wavenet and Wavenet_alt alike)."""
    from wwhip.engine import frontend_params
    eng = engines[model]
    ref = R.Ref64(os.path.join(assets, model))
    seq64 = WaveSeq64(eng.bundle.wavenet)
    signals = R.frontend_signals(3)
    names = list(signals)
    S = len(names)
    pcm = [np.asarray(signals[n], np.int16) for n in names]
    rng = np.random.default_rng(51)
    bank = _bank(eng, S, frontend_params(32767, True, 0.97, 160, precise))
    posts, mels = [[] for _ in range(S)], [[] for _ in range(S)]
    at = [0] * S
    try:
        while any(at[s] < len(pcm[s]) for s in range(S)):
            ids = [s for s in range(S) if at[s] < len(pcm[s]) and rng.random() < 0.7]
            ks = [min(int(rng.choice([1, 160, 320, 511, 800, 2720, 5000, 33000])), len(pcm[s]) - at[s]) for s in ids]
            p, m = bank.feed(ids, [pcm[s][at[s]:at[s] + k] for s, k in zip(ids, ks)], want_mel=True)
            for i, (s, k) in enumerate(zip(ids, ks)):
                posts[s].append(p[i])
                mels[s].append(m[i])
                at[s] += k
    finally:
        bank.close()
    worst_fe, worst_p = 0.0, 0.0
    for s, n in enumerate(names):
        want = ref.logmel(pcm[s], 32767.0, True, 0.97, 160)
        got = np.concatenate(mels[s]) if mels[s] else np.zeros((0, 40), np.float32)
        assert got.shape == want.y.shape, (n, got.shape, want.y.shape)
        if not len(got):
            continue
        g64 = np.asarray(got, np.float64)
        need = R.needed_taus(g64, want, TAU_REL if not precise else 0.0, 0.0)
        w64 = seq64.sequence(got)["post_frames"][:, eng.posterior_index]
        gp = np.concatenate(posts[s])
        need_p = R.needed_tau(gp[:, None], w64[:, None])
        print(f"\nFEED64 {model} precise={precise} {n}: {len(got)} rows, mel needs tau_rel {need[0]:.2e} (tau_fft 0), tau_fft {need[1]:.2e}; "
              f"posteriors need tau {need_p:.2e} (tau {TAU:g})", end="")
        worst_fe = max(worst_fe, need[0] if precise else need[1])
        worst_p = max(worst_p, need_p)
    print(f"\nFEED64 {model} precise={precise} worst: mel {worst_fe:.2e}, posteriors {worst_p:.2e}", end="")
    for s, n in enumerate(names):
        if not mels[s] or not sum(len(x) for x in mels[s]):
            continue
        got = np.concatenate(mels[s])
        R.check_logmel(np.asarray(got, np.float64), ref.logmel(pcm[s], 32767.0, True, 0.97, 160), TAU_REL, 0.0 if precise else TAU_FFT)
        w64 = seq64.sequence(got)["post_frames"][:, eng.posterior_index]
        R.check_posteriors(np.concatenate(posts[s])[:, None], w64[:, None], TAU)


# ---------------------------------------------------------------------------------------- 6. refusals and degenerate sizes
def test_refusals_and_degenerate_sizes(engines, assets):
    """Every WW_EINVAL of the contract through ctypes, each followed by a valid feed whose result equals a twin bank's that never
    saw the refused call; a CRNN bank and a Wavenet window bank refuse; n = 0 and empty packets are WW_OK and change nothing; 511
    samples in 1-sample packets give no row, the 512th gives row 0; ww_stream_feed_rows agrees with ww_stream_feed's row_offs."""
    from wwhip import _lib
    from wwhip.engine import Engine, StreamBank
    lib = _lib.load()
    eng = engines["Wavenet"]
    rng = np.random.default_rng(61)
    S = 6
    bank, twin = _bank(eng, S), _bank(eng, S)
    pcm = _pcm(rng, 6000)
    post = np.full(64, 7.0, np.float32)
    mel = np.full((64, 40), 7.0, np.float32)
    ro = np.full(8, -1, np.int64)

    def call(b, ids, offs, n=None, cap=64, p_pcm=pcm, p_offs=True, p_ro=True, p_post=True, p_ids=True):
        ids = np.asarray(ids, np.int32)
        offs = np.asarray(offs, np.int64)
        return lib.ww_stream_feed(b._h, _lib.ptr(ids) if p_ids else None, len(ids) if n is None else n, _lib.ptr(p_pcm) if p_pcm is not None else None,
                                  _lib.ptr(offs) if p_offs else None, cap, _lib.ptr(ro) if p_ro else None, _lib.ptr(post) if p_post else None, _lib.ptr(mel))

    try:
        warm = [_pcm(rng, k) for k in (700, 100, 3000)]
        for b in (bank, twin):
            b.feed([0, 1, 2], warm)
        refused = [
            lambda: call(bank, [0, 1], [0, 1000, 2000], n=-1),                       # n < 0
            lambda: call(bank, [0, S], [0, 1000, 2000]),                             # an id out of range
            lambda: call(bank, [0, -1], [0, 1000, 2000]),
            lambda: call(bank, [1, 1], [0, 1000, 2000]),                             # an id named twice
            lambda: call(bank, [0, 1], [0, 2000, 1000]),                             # descending sample_offs
            lambda: call(bank, [0, 1], [0, 3000, 6000], cap=30),                     # cap_rows too small (3,000 samples each: more than 30 rows)
            lambda: call(bank, [0, 1], [0, 1000, 2000], p_pcm=None),                 # NULL arguments
            lambda: call(bank, [0, 1], [0, 1000, 2000], p_offs=False),
            lambda: call(bank, [0, 1], [0, 1000, 2000], p_ro=False),
            lambda: call(bank, [0, 1], [0, 1000, 2000], p_post=False),
            lambda: call(bank, [0, 1], [0, 1000, 2000], p_ids=False),
        ]
        for i, f in enumerate(refused):
            assert f() == _lib.WW_EINVAL, i
            nxt = [_pcm(rng, k) for k in (333, 1000, 160)]
            got, want = bank.feed([2, 0, 4], nxt, want_mel=True), twin.feed([2, 0, 4], nxt, want_mel=True)
            for x, y in zip(got[0] + got[1], want[0] + want[1]):
                np.testing.assert_array_equal(x, y, err_msg=f"after refusal {i}")
        assert lib.ww_stream_feed(None, None, 0, None, None, 0, None, None, None) == _lib.WW_EINVAL
        assert lib.ww_stream_feed_rows(bank._h, None, 1, _lib.ptr(np.zeros(2, np.int64)), _lib.ptr(ro)) == _lib.WW_EINVAL
        # ---- n = 0 and empty packets: WW_OK, nothing changes
        post[:] = 7.0
        assert call(bank, [], [0], n=0) == _lib.WW_OK and ro[0] == 0
        assert call(bank, [0, 3], [5, 5, 5]) == _lib.WW_OK and list(ro[:3]) == [0, 0, 0]
        assert np.all(post == 7.0)
        nxt = [_pcm(rng, k) for k in (640, 2000)]
        got, want = bank.feed([0, 3], nxt, want_mel=True), twin.feed([0, 3], nxt, want_mel=True)
        for x, y in zip(got[0] + got[1], want[0] + want[1]):
            np.testing.assert_array_equal(x, y, err_msg="after the empty calls")
        for s in range(S):
            np.testing.assert_array_equal(bank.window(s), twin.window(s))
        # ---- ww_stream_feed_rows agrees with what ww_stream_feed writes, and touches nothing
        ids = np.array([5, 1, 0], np.int32)
        offs = np.array([0, 1234, 1234, 6000], np.int64)
        ro2 = np.full(4, -1, np.int64)
        assert lib.ww_stream_feed_rows(bank._h, _lib.ptr(ids), 3, _lib.ptr(offs), _lib.ptr(ro2)) == _lib.WW_OK
        assert lib.ww_stream_feed_rows(bank._h, _lib.ptr(ids), 3, _lib.ptr(offs), _lib.ptr(ro2)) == _lib.WW_OK
        assert call(bank, ids, offs) == _lib.WW_OK
        assert list(ro[:4]) == list(ro2) and ro2[3] > 30
        twin.feed([5, 1, 0], [pcm[:1234], pcm[:0], pcm[1234:6000]])
        # ---- 511 samples one at a time: no row; the 512th gives row 0
        bank.reset()
        one = _pcm(rng, 512)
        for i in range(511):
            p, m = bank.feed([4], [one[i:i + 1]], want_mel=True)
            assert len(p[0]) == 0 and m[0].shape == (0, 40)
        p, m = bank.feed([4], [one[511:]], want_mel=True)
        fresh = _bank(eng, 1)
        try:
            p1, m1 = fresh.feed([0], [one], want_mel=True)
        finally:
            fresh.close()
        assert len(p[0]) == 1
        np.testing.assert_array_equal(p[0], p1[0])
        np.testing.assert_array_equal(m[0], m1[0])
    finally:
        bank.close()
        twin.close()
    # ---- banks that cannot be fed: a Wavenet window bank, a CRNN bank
    crnn = Engine(os.path.join(assets, "CRNN"))
    try:
        for b in (StreamBank(eng, 2), StreamBank(crnn, 2)):
            try:
                assert call(b, [0], [0, 1000]) == _lib.WW_EINVAL
                assert lib.ww_stream_feed_rows(b._h, _lib.ptr(np.zeros(1, np.int32)), 1, _lib.ptr(np.array([0, 1000], np.int64)), _lib.ptr(ro)) == _lib.WW_EINVAL
                with pytest.raises(ValueError):
                    b.feed([0], [pcm[:1000]])
                p, n = b.step(np.zeros((2, 320), np.int16), np.ones(2, np.uint8))   # the bank is as it was
                assert list(n) == [0, 0]
            finally:
                b.close()
    finally:
        crnn.close()
