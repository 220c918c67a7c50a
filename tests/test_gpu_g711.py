"""G.711 (mu-law / A-law) input on the MI355X: the resampler, the stream banks' tick and feed, and the refusals.

ONE contract (include/wwhip.h): a G.711 input yields the bits the same call yields on the decoded int16 samples.  Every comparison
here is ``assert_array_equal`` - posteriors and mel rows through their integer views - against the SAME call on the samples decoded
on the host with ``ww_g711_table``'s table (which tests/test_g711_host.py holds against ITU-T G.711's formulas): no tolerance.

Shapes.  Rates 8000 (up 2), 8050 (up 320, down 161: a frame of 161 samples, which puts the frames behind it on odd bytes) and 16000
(no filter: the decode alone).  The per-stream bank has the seven classes (8000 mu-law), (8000 A-law), (8050 mu-law), (16000
mu-law), (8000 pcm16), (16000 pcm16), (48000 pcm16), one stream each in this order: the frames start at bytes 0, 160, 320, 481, 802,
1122, 1762 - an odd byte, residues 0, 1 and 2 modulo 16, a pad byte at 801 - and when stream 3 moves to (16000 pcm16) the odd frame
has an int16 neighbour behind it too (a pad byte at 481).
"""
import ctypes as C
import os

import numpy as np
import pytest
from numpy.testing import assert_array_equal

pytestmark = pytest.mark.gpu

I16, F32, MULAW, ALAW = 0, 1, 8, 9
FMT = {"mulaw": MULAW, "alaw": ALAW}
CLASSES = [(8000, "mulaw"), (8000, "alaw"), (8050, "mulaw"), (16000, "mulaw"), (8000, "pcm16"), (16000, "pcm16"), (48000, "pcm16")]
WAVES = ["Wavenet", "Wavenet_alt"]
CRNNS = ["CRNN_nosilence", "CRNN_nosilence_enhanced"]


@pytest.fixture(scope="module")
def engines(assets):
    from wwhip.engine import Engine
    out = {m: Engine(os.path.join(assets, m)) for m in ["CRNN"] + WAVES + CRNNS}
    yield out
    for e in out.values():
        e.close()


@pytest.fixture(scope="module")
def tables():
    from wwhip import g711
    return {law: g711.table(law) for law in FMT}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _encode(x, table):
    """int16 samples -> the codes whose decoded values are nearest (the test's own encoder: the library has none)."""
    order = np.argsort(table, kind="stable")
    vals = table[order].astype(np.int64)
    i = np.clip(np.searchsorted(vals, x), 1, 255)
    i = np.where(np.abs(vals[i - 1] - x) <= np.abs(vals[i] - x), i - 1, i)
    return order[i].astype(np.uint8)


_sig_cache = {}


def _signal(s, rate, fmt, tables, seconds):
    """Stream s's signal in its format - a tone plus seeded noise, for G.711 streams as codes whose head holds all 256 codes -
    and the int16 samples it stands for; computed once and never written to."""
    key = (s, rate, fmt, seconds)
    if key not in _sig_cache:
        n = int(round(rate * seconds))
        rng = np.random.default_rng(100 * s + rate)
        t = np.arange(n) / rate
        x = np.clip(np.rint(0.3 * 32768 * np.sin(2 * np.pi * (250.0 + 130.0 * s) * t) + rng.normal(0, 0.1 * 32768, n)), -32768, 32767).astype(np.int16)
        if fmt == "pcm16":
            raw = x
        else:
            raw = _encode(x.astype(np.int64), tables[fmt])
            raw[:256] = (np.arange(256) + 37 * s) % 256  # every code, early: 160 of them in an 8 kHz stream's first frame, all by the second
            x = tables[fmt][raw]
        raw.setflags(write=False)
        x.setflags(write=False)
        _sig_cache[key] = (raw, x)
    return _sig_cache[key]


# ---- the resampler -----------------------------------------------------------------------------------------------------------------
def _resample(rs, buf, fmt, so, i0, o0, oo, out_dtype):
    """``ww_resample`` through ctypes: the caller's buffer and offset tables as they are."""
    from wwhip import _lib
    so, oo = np.ascontiguousarray(so, np.int64), np.ascontiguousarray(oo, np.int64)
    i0 = None if i0 is None else np.ascontiguousarray(i0, np.int64)
    o0 = None if o0 is None else np.ascontiguousarray(o0, np.int64)
    out = np.full(int(oo[-1]) + 3, 77, out_dtype)
    rc = _lib.load().ww_resample(rs._h, _lib.ptr(buf), fmt, _lib.ptr(so), _lib.ptr(i0), _lib.ptr(o0), _lib.ptr(oo), len(so) - 1, _lib.ptr(out),
                                 I16 if out_dtype == np.int16 else F32)
    assert rc == _lib.WW_OK, _lib.load().ww_last_error(rs.ctx.handle)
    assert (out[:int(oo[0])] == 77).all() and (out[int(oo[-1]):] == 77).all()
    return out


@pytest.mark.parametrize("rate", [8000, 8050, 16000])
def test_resampler_takes_g711_as_the_decoded_int16(rate, tables):
    """Segments of 4001, 161 and 1 samples cut from ONE byte buffer from sample 1 on (they start at bytes 1, 4002 and 4163), the
    first with every code 0 .. 255 at its head; both laws, int16 and float32 output; as a one-shot and as pieces with ``in_first`` /
    ``out_first``; each run against the same call on the decoded samples.  At 8050 Hz: up 320, down 161, 21,760 taps."""
    from wwhip.resample import Resampler, StreamResampler, out_len
    rs = Resampler(rate, 16000)
    if rate == 8050:
        assert (rs.up, rs.down, rs.taps_per_output * rs.up) == (320, 161, 21760)
    rng = np.random.default_rng(rate)
    lens = [4001, 161, 1]
    so = np.concatenate(([1], 1 + np.cumsum(lens)))
    try:
        for law, fmt in FMT.items():
            codes = rng.integers(0, 256, int(so[-1]) + 5, dtype=np.uint8)
            codes[1:257] = np.arange(256)
            pcm = tables[law][codes]
            # the pieces: segment u holds samples in_first[u] .. of its signal, and outputs out_first[u] .. are asked for
            i0 = np.array([1000, 40, 0])
            o0 = np.array([out_len(1300, rs.up, rs.down), out_len(45, rs.up, rs.down), 0])
            runs = {"one-shot": (None, None, [out_len(n, rs.up, rs.down) for n in lens]),
                    "pieces": (i0, o0, [out_len(int(i0[u]) + lens[u], rs.up, rs.down) - int(o0[u]) for u in range(3)])}
            for what, (first_in, first_out, counts) in runs.items():
                oo = np.concatenate(([2], 2 + np.cumsum(counts)))
                for dt in (np.int16, np.float32):
                    got = _resample(rs, codes, fmt, so, first_in, first_out, oo, dt)
                    want = _resample(rs, pcm, I16, so, first_in, first_out, oo, dt)
                    assert_array_equal(got.view(np.uint16 if dt == np.int16 else np.uint32), want.view(np.uint16 if dt == np.int16 else np.uint32),
                                       err_msg=f"{rate} Hz {law} {what} {np.dtype(dt)}")
                    if rate == 16000 and what == "one-shot":  # equal rates: the decoded signal itself
                        seg = pcm[1:1 + sum(lens)]
                        assert_array_equal(got[2:2 + seg.size], seg if dt == np.int16 else seg.astype(np.float32) / np.float32(32768.0))
            # the Python surface: whole clips, and a stream in packets
            clips = [codes[1:4002], codes[4002:4163]]
            for a, b in zip(rs(clips, np.float32, law=law), rs([pcm[1:4002], pcm[4002:4163]], np.float32)):
                assert_array_equal(_bits(a), _bits(b))
            st, ref = StreamResampler(rate, 16000, ctx=rs.ctx, law=law), StreamResampler(rate, 16000, ctx=rs.ctx)
            for a, b in ((1, 162), (162, 163), (163, 163), (163, 4100)):
                assert_array_equal(_bits(st.push(codes[a:b])), _bits(ref.push(pcm[a:b])))
            assert_array_equal(_bits(st.flush()), _bits(ref.flush()))
            st.close(), ref.close()
            with pytest.raises(ValueError, match="uint8 codes, not int16"):
                rs(pcm[:100], law=law)
    finally:
        rs.close()


def test_g711_wav_is_decoded_and_resampled_in_one_pass(tmp_path, tables):
    """A hand-written 8 kHz mu-law wav through ``read_wav(resample=True)``, ``wwhip.resample.load`` and ``WavInput``: the bits of
    the resampler on the decoded samples; and an A-law file at 16 kHz: the decoded samples / 32768."""
    import struct
    from wwhip.evaluate import read_wav, read_wav_pcm, wav_length
    from wwhip.io import WavInput
    from wwhip.resample import Resampler, load

    def wav(name, tag, rate, codes):
        body = struct.pack("<HHIIHHH", tag, 1, rate, rate, 1, 8, 0)
        chunks = b"fmt " + struct.pack("<I", 18) + body + b"fact" + struct.pack("<II", 4, len(codes)) + b"data" + struct.pack("<I", len(codes)) + codes.tobytes()
        p = tmp_path / name
        p.write_bytes(b"RIFF" + struct.pack("<I", 4 + len(chunks)) + b"WAVE" + chunks)
        return str(p)

    rng = np.random.default_rng(3)
    codes = rng.integers(0, 256, 3000, dtype=np.uint8)
    p8 = wav("mu8k.wav", 7, 8000, codes)
    rs = Resampler(8000, 16000)
    try:
        want = rs(tables["mulaw"][codes], np.float32)
        assert wav_length(p8, 16000, resample=True) == want.size == 6000
        for got in (read_wav(p8, 16000, resample=True), read_wav_pcm(p8, 16000, resample=True), load(p8)):
            assert_array_equal(_bits(got), _bits(want))
        assert_array_equal(WavInput(p8, resample=True)._pcm, rs(tables["mulaw"][codes], np.int16))
    finally:
        rs.close()
    p16 = wav("a16k.wav", 6, 16000, codes)
    assert_array_equal(read_wav(p16, 16000, resample=True), tables["alaw"][codes].astype(np.float32) / np.float32(32768.0))


# ---- the per-stream bank's tick ------------------------------------------------------------------------------------------------------
def _layout_bytes(bank):
    from wwhip import _lib
    fb, bo, fm = np.full(bank.S, -1, np.int32), np.full(bank.S + 1, -1, np.int64), np.full(bank.S, -1, np.int32)
    assert _lib.load().ww_stream_frame_layout_bytes(bank._h, _lib.ptr(fb), _lib.ptr(bo), _lib.ptr(fm)) == _lib.WW_OK
    return fb, bo, fm


def _frames(cur, t, tables, seconds):
    """Tick t's frames of the streams in classes ``cur``: as the formats carry them, and decoded."""
    raw, dec = [], []
    for s, (rate, fmt) in enumerate(cur):
        r, x = _signal(s, rate, fmt, tables, seconds)
        F = rate // 50
        raw.append(r[t * F:(t + 1) * F])
        dec.append(x[t * F:(t + 1) * F])
    return raw, dec


def _block(bank, raw):
    """The flat byte block of a tick, laid out by hand from ``frame_byte_offs``; the pad bytes are 0xEE."""
    blk = np.full(int(bank.frame_byte_offs[bank.S]), 0xEE, np.uint8)
    for s, a in enumerate(raw):
        blk[int(bank.frame_byte_offs[s]):int(bank.frame_byte_offs[s]) + a.nbytes] = a.view(np.uint8)
    return blk


MIXED_FORMS = {"crnn": ("CRNN", {}), "causal": ("Wavenet", dict(causal=True)), "every_member": ("crnn_set", dict(members="all"))}


@pytest.mark.parametrize("form", list(MIXED_FORMS))
def test_mixed_format_bank_equals_the_rates_bank_on_decoded_frames(engines, tables, form):
    """S = 7, one stream per class, 60 ticks with random VAD bits, frozen ticks (bit 1), a reset, and stream 3's move from (16000
    mu-law) to (16000 pcm16) and back: ``post`` and ``n_post`` of every tick equal the ``ww_stream_attach_rates`` bank's at the same
    rates fed the decoded frames.  The flat block (pad bytes 0xEE) and the per-stream arrays in turn."""
    from wwhip.engine import ModelSet, StreamBank
    S, TICKS, seconds = 7, 60, 1.2
    model, kw = MIXED_FORMS[form]
    ms = ModelSet([engines[m] for m in CRNNS]) if model == "crnn_set" else None
    eng = ms if ms is not None else engines[model]
    rates = [c[0] for c in CLASSES]
    bank = StreamBank(eng, S, sample_rate=rates, sample_format=[c[1] for c in CLASSES], **kw)
    ref = StreamBank(eng, S, sample_rate=rates, **kw)
    try:
        fb, bo, fm = _layout_bytes(bank)
        assert bo.tolist() == [0, 160, 320, 481, 802, 1122, 1762, 3682] and fb.tolist() == [160, 160, 161, 320, 320, 640, 1920]
        assert fm.tolist() == [MULAW, ALAW, MULAW, MULAW, I16, I16, I16] and bank.sample_formats == [c[1] for c in CLASSES]
        assert_array_equal(bank.frame_bytes, fb), assert_array_equal(bank.frame_byte_offs, bo)
        assert sorted(set((bo[:-1] % 16).tolist())) == [0, 1, 2]
        first = np.concatenate(_frames(CLASSES, 0, tables, seconds)[0][:4])
        assert len(set(first.tolist())) == 256  # the first tick's G.711 frames hold every code
        rng = np.random.default_rng(len(form))
        speech = (rng.random((TICKS, S)) < 0.85).astype(np.uint8)
        active = np.zeros((TICKS, S), np.uint8)
        for s in range(S):
            a = int(rng.integers(4, 50))
            active[a:a + int(rng.integers(1, 5)), s] = 1
        cur = list(CLASSES)
        seen = np.zeros(S, int)
        for t in range(TICKS):
            raw, dec = _frames(cur, t, tables, seconds)
            got = bank.step(_block(bank, raw) if t % 2 else raw, speech[t], active[t])
            want = ref.step(dec, speech[t], active[t])
            assert_array_equal(got[1], want[1], err_msg=f"n_post of tick {t}")
            assert_array_equal(_bits(got[0]), _bits(want[0]), err_msg=f"post of tick {t}")
            seen += got[1]
            if t == 14:
                bank.reset([0, 2]), ref.reset([0, 2])
            if t in (20, 35):  # stream 3: G.711 -> int16 at tick 20 (the odd frame gets an int16 neighbour and a pad byte), back at 35
                cur[3] = (16000, "pcm16") if t == 20 else (16000, "mulaw")
                bank.set_rate([3], *cur[3]), ref.set_rate([3], 16000)
                fb, bo, fm = _layout_bytes(bank)
                assert bo.tolist() == ([0, 160, 320, 482, 1122, 1442, 2082, 4002] if t == 20 else [0, 160, 320, 481, 802, 1122, 1762, 3682])
                assert_array_equal(bank.frame_byte_offs, bo)
                assert bank.sample_formats[3] == cur[3][1]
        for s in range(S):
            assert_array_equal(_bits(bank.window(s)), _bits(ref.window(s)), err_msg=f"window of stream {s}")
        assert (seen >= 20).all(), seen
    finally:
        bank.close(), ref.close()
        if ms is not None:
            ms.close()


# ---- the uniform bank ----------------------------------------------------------------------------------------------------------------
def test_uniform_mulaw_bank_equals_the_8000_bank_on_decoded_frames(engines, tables):
    """8 kHz mu-law, S = 5, 40 ticks of ``step`` against ``StreamBank(sample_rate=8000)`` on the decoded frames; then both through
    ``SpeechPipelineBank([VadBank, WakewordBank, ActivationTimeoutBank])``: the flags, the fired / fall / deactivated ids and the
    posteriors of every tick are equal.  The VAD's classifier sees what the source delivers: uint8 ``[S, 160]`` here."""
    from wwhip.activation_timeout import ActivationTimeoutBank
    from wwhip.engine import StreamBank
    from wwhip.pipeline import SpeechPipelineBank
    from wwhip.vad import VadBank
    from wwhip.wakeword import WakewordBank
    S, TICKS, F = 5, 40, 160
    eng = engines["CRNN"]
    sig = [_signal(s, 8000, "mulaw", tables, TICKS / 50) for s in range(S)]
    codes, pcm = np.stack([r for r, _ in sig]), np.stack([x for _, x in sig])
    bank, ref = StreamBank(eng, S, sample_rate=8000, sample_format="mulaw"), StreamBank(eng, S, sample_rate=8000)
    top = np.zeros(S, np.float32)
    try:
        assert bank.sample_formats == ["mulaw"] * S and bank.frame_bytes.tolist() == [160] * S and bank.frame_byte_offs.tolist() == [0, 160, 320, 480, 640, 800]
        assert ref.sample_formats == ["pcm16"] * S and ref.frame_bytes.tolist() == [320] * S
        fb, bo, fm = _layout_bytes(bank)
        assert fb.tolist() == [160] * S and bo.tolist() == [0, 160, 320, 480, 640, 800] and fm.tolist() == [MULAW] * S
        rng = np.random.default_rng(8)
        speech = (rng.random((TICKS, S)) < 0.9).astype(np.uint8)
        for t in range(TICKS):
            got = bank.step(codes[:, t * F:(t + 1) * F], speech[t])
            want = ref.step(pcm[:, t * F:(t + 1) * F], speech[t])
            assert_array_equal(got[1], want[1], err_msg=f"n_post of tick {t}")
            assert_array_equal(_bits(got[0]), _bits(want[0]), err_msg=f"post of tick {t}")
            if 3 <= t < 15:
                for s in range(S):
                    top[s] = max([top[s]] + [got[0][s, k] for k in range(got[1][s])])
        with pytest.raises(ValueError, match="not int16"):
            bank.step(pcm[:, :F], speech[0])
    finally:
        bank.close(), ref.close()
    thr = float(np.median(top))
    raw = np.ones((TICKS, S), bool)
    for s in range(S):
        a = int(rng.integers(18, 30))
        raw[a:a + 5, s] = False

    class Source:
        def __init__(self, x):
            self.x, self.t = x, 0

        def read(self):
            self.t += 1
            return self.x[:, (self.t - 1) * F:self.t * F]

        def start(self):
            pass

        stop = close = start

    def run(bank, x, dtype):
        src = Source(x)
        seen = []

        def classify(f):
            seen.append((np.shape(f), np.asarray(f).dtype))
            return raw[src.t - 1]
        vad = VadBank(S, classifier=classify, frame_width=20, vad_rise_delay=40, vad_fall_delay=60)
        wake, to = WakewordBank(S, posterior_threshold=thr, bank=bank), ActivationTimeoutBank(S, frame_width=20, min_active=60, max_active=200)
        pipe = SpeechPipelineBank(src, [vad, wake, to], S)
        assert pipe._fused is not None
        ps = pipe._fused[0]
        pipe.start()
        log = []
        for t in range(TICKS):
            pipe.step()
            log.append((sorted(wake._fired[:ps.n_fired].tolist()), sorted(wake._fall[:ps.n_fall].tolist()), sorted(to._ids[:ps.n_deact].tolist()),
                        pipe.context.is_speech.copy(), pipe.context.is_active.copy(), wake._post.copy(), wake._n.copy()))
        assert seen == [((S, F), np.dtype(dtype))] * TICKS
        pipe.stop()
        pipe.cleanup()
        return log

    bank, ref = StreamBank(eng, S, sample_rate=8000, sample_format="mulaw"), StreamBank(eng, S, sample_rate=8000)
    try:
        got, want = run(bank, codes, np.uint8), run(ref, pcm, np.int16)
    finally:
        bank.close(), ref.close()
    for t, (a, b) in enumerate(zip(got, want)):
        assert a[:3] == b[:3], (t, a[:3], b[:3])
        assert_array_equal(a[3], b[3]), assert_array_equal(a[4], b[4]), assert_array_equal(a[6], b[6])
        assert_array_equal(_bits(a[5]), _bits(b[5]), err_msg=f"pipeline tick {t}")
    assert sum(len(a[1]) for a in got) >= S  # every stream's VAD fell once


# ---- the feed ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("every", [False, True])
def test_feed_bytes_equals_feed_on_decoded_packets(engines, tables, every):
    """A causal Wavenet bank, S = 6 of the classes (48000 pcm16 left out): seeded random packets of 0, 1, an odd count and up to 2 s,
    any subset of the streams per call, interleaved with ticks - the same cuts go to the int16 bank at the same rates through
    ``ww_stream_feed``.  The rows per packet, ``post`` and ``mel`` are equal.  ``every``: through ``ww_stream_feed_bytes_all`` on a bank
    of K = 2 member slots against ``ww_stream_feed_all``."""
    from wwhip.engine import ModelSet, StreamBank
    cls = CLASSES[:6]
    S, seconds = 6, 8.0
    ms = ModelSet([engines[m] for m in WAVES]) if every else None
    eng, kw = (ms, dict(members="all")) if every else (engines["Wavenet"], {})
    rates, fmts = [c[0] for c in cls], [c[1] for c in cls]
    bank = StreamBank(eng, S, causal=True, sample_rate=rates, sample_format=fmts, **kw)
    ref = StreamBank(eng, S, causal=True, sample_rate=rates, **kw)
    feed = (lambda b, ids, pk: b.feed_all(ids, pk, want_mel=True)) if every else (lambda b, ids, pk: b.feed(ids, pk, want_mel=True))
    try:
        rng = np.random.default_rng(6 + every)
        sig = [_signal(s, r, f, tables, seconds) for s, (r, f) in enumerate(cls)]
        at = [0] * S
        rows = 0
        for call in range(9):
            if call in (3, 6):  # a tick between the feeds
                raw = [sig[s][0][at[s]:at[s] + rates[s] // 50] for s in range(S)]
                dec = [sig[s][1][at[s]:at[s] + rates[s] // 50] for s in range(S)]
                got, want = bank.step(raw, np.ones(S, np.uint8)), ref.step(dec, np.ones(S, np.uint8))
                assert_array_equal(got[1], want[1]), assert_array_equal(_bits(got[0]), _bits(want[0]))
                at = [at[s] + rates[s] // 50 for s in range(S)]
                continue
            ids = [int(s) for s in rng.permutation(S)[:int(rng.integers(1, S + 1))]] if call else list(range(S))
            sizes = [int(rng.choice([0, 1, 161, int(rng.integers(2, rates[s] // 4)) | 1, int(rng.integers(rates[s] // 2, 2 * rates[s]))])) for s in ids]
            if call == 0:
                sizes = [rates[0] * 2, 1, 161, 0, 3001, 4000]  # 2 s, 1, odd counts, an empty packet
            sizes = [min(k, sig[s][0].size - 2 * (rates[s] // 50) - at[s]) for s, k in zip(ids, sizes)]  # (room for the two ticks)
            pk_raw = [sig[s][0][at[s]:at[s] + k] for s, k in zip(ids, sizes)]
            pk_dec = [sig[s][1][at[s]:at[s] + k] for s, k in zip(ids, sizes)]
            for s, k in zip(ids, sizes):
                assert at[s] + k <= sig[s][0].size
                at[s] += k
            (gp, gm), (wp, wm) = feed(bank, ids, pk_raw), feed(ref, ids, pk_dec)
            for i in range(len(ids)):
                assert gp[i].shape == wp[i].shape and gm[i].shape == wm[i].shape, (call, ids[i])
                assert_array_equal(_bits(gp[i]), _bits(wp[i]), err_msg=f"post of call {call}, stream {ids[i]}")
                assert_array_equal(_bits(gm[i]), _bits(wm[i]), err_msg=f"mel of call {call}, stream {ids[i]}")
                rows += gm[i].shape[0]
        assert rows > 300, rows
    finally:
        bank.close(), ref.close()
        if ms is not None:
            ms.close()


def test_feed_bytes_on_a_bank_without_g711_is_feed(engines):
    """``ww_stream_feed_bytes`` on an int16 rates bank and on a plain causal bank: ``ww_stream_feed`` with byte_offs = 2 x sample_offs."""
    from wwhip import _lib
    from wwhip.engine import StreamBank
    eng = engines["Wavenet"]
    lib, h = _lib.load(), eng.ctx.handle
    rng = np.random.default_rng(12)
    for kw in (dict(sample_rate=[8000, 16000, 48000]), {}):
        a, b = StreamBank(eng, 3, causal=True, **kw), StreamBank(eng, 3, causal=True, **kw)
        try:
            pcm = rng.integers(-20000, 20000, 30000, dtype=np.int16)
            ids = np.array([2, 0, 1], np.int32)
            so = np.array([3, 9004, 9004, 25001], np.int64)
            ro_a, ro_b = np.zeros(4, np.int64), np.zeros(4, np.int64)
            post_a, post_b = np.zeros(400, np.float32), np.zeros(400, np.float32)
            mel_a, mel_b = np.zeros((400, eng.n_mel), np.float32), np.zeros((400, eng.n_mel), np.float32)
            assert lib.ww_stream_feed(a._h, _lib.ptr(ids), 3, _lib.ptr(pcm), _lib.ptr(so), 400, _lib.ptr(ro_a), _lib.ptr(post_a), _lib.ptr(mel_a)) == 0
            bo = 2 * so
            assert lib.ww_stream_feed_bytes(b._h, _lib.ptr(ids), 3, _lib.ptr(pcm), _lib.ptr(bo), 400, _lib.ptr(ro_b), _lib.ptr(post_b), _lib.ptr(mel_b)) == 0, \
                lib.ww_last_error(h)
            assert ro_a[3] > 50
            assert_array_equal(ro_a, ro_b), assert_array_equal(_bits(post_a), _bits(post_b)), assert_array_equal(_bits(mel_a), _bits(mel_b))
        finally:
            a.close(), b.close()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_reason_and_move_nothing(engines, tables):
    """Each refusal is WW_EINVAL with the reason in ``ww_last_error``, leaves its outputs untouched, and the valid call behind it
    gives the bits of a bank that never saw the refused ones."""
    from wwhip import _lib
    from wwhip.engine import StreamBank
    from wwhip.resample import Resampler
    eng = engines["Wavenet"]
    lib, h = _lib.load(), eng.ctx.handle

    def err():
        return lib.ww_last_error(h).decode()

    rs = Resampler(8000, 16000, eng.ctx)
    banks = []
    try:
        # a G.711 out_format
        codes = np.arange(256, dtype=np.int64).astype(np.uint8)
        so, oo = np.array([0, 256], np.int64), np.array([0, 512], np.int64)
        out = np.full(512, 77, np.int16)
        for fmt in (MULAW, ALAW):
            assert lib.ww_resample(rs._h, _lib.ptr(codes), MULAW, _lib.ptr(so), None, None, _lib.ptr(oo), 1, _lib.ptr(out), fmt) == _lib.WW_EINVAL
            assert "input format only" in err() and (out == 77).all()
        assert lib.ww_resample(rs._h, _lib.ptr(codes), 2, _lib.ptr(so), None, None, _lib.ptr(oo), 1, _lib.ptr(out), I16) == _lib.WW_EINVAL and (out == 77).all()
        assert lib.ww_resample(rs._h, _lib.ptr(codes), MULAW, _lib.ptr(so), None, None, _lib.ptr(oo), 1, _lib.ptr(out), I16) == _lib.WW_OK
        assert_array_equal(out, rs(tables["mulaw"][codes], np.int16))
        # the class table
        plain = StreamBank(eng, 3, causal=True)
        banks.append(plain)
        table = (C.c_void_p * 3)(rs._h, None, rs._h)
        cls = np.array([0, 1, 2], np.int32)

        def attach(fmts, n=3):
            return lib.ww_stream_attach_rates_fmt(plain._h, table, _lib.ptr(np.array(fmts, np.int32)), n, _lib.ptr(cls))
        assert attach([MULAW, I16, F32]) == _lib.WW_EINVAL and "class 2" in err() and "float32" in err()
        assert attach([MULAW, I16, 2]) == _lib.WW_EINVAL and "format 2" in err()
        assert attach([ALAW, I16, ALAW]) == _lib.WW_EINVAL and "class 2" in err() and "same input rate and format" in err()
        assert lib.ww_stream_attach_rates_fmt(plain._h, table, None, 3, _lib.ptr(cls)) == _lib.WW_EINVAL and "ww_stream_attach_rates:" in err() \
            and "same input rate" in err()  # formats == NULL: ww_stream_attach_rates and its refusals
        assert lib.ww_stream_attach_resampler_fmt(plain._h, rs._h, F32) == _lib.WW_EINVAL and "float32" in err()
        fb, bo, fm = _layout_bytes(plain)  # still a plain bank: 640-byte int16 frames
        assert fb.tolist() == [640] * 3 and bo.tolist() == [0, 640, 1280, 1920] and fm.tolist() == [I16] * 3
        assert attach([MULAW, I16, ALAW]) == _lib.WW_OK, err()
        fb, bo, fm = _layout_bytes(plain)
        assert fb.tolist() == [160, 640, 160] and bo.tolist() == [0, 160, 800, 960] and fm.tolist() == [MULAW, I16, ALAW]
        assert attach([MULAW, I16, ALAW]) == _lib.WW_EINVAL and "already" in err()
        # the calls that count int16 samples, and the packet checks, on that bank; `twin` never sees a refused call
        twin = StreamBank(eng, 3, causal=True, sample_rate=[8000, 16000, 8000], sample_format=["mulaw", "pcm16", "alaw"])
        banks.append(twin)
        fs, fo = np.full(3, -1, np.int32), np.full(4, -1, np.int64)
        assert lib.ww_stream_frame_layout(plain._h, _lib.ptr(fs), _lib.ptr(fo)) == _lib.WW_EINVAL and "ww_stream_frame_layout_bytes" in err()
        assert (fs == -1).all() and (fo == -1).all()
        n = C.c_int32(-1)
        assert lib.ww_stream_frame_samples(plain._h, C.byref(n)) == _lib.WW_EINVAL and n.value == -1
        rng = np.random.default_rng(4)
        data = rng.integers(0, 256, 40000, dtype=np.uint8)
        ids = np.array([1, 0, 2], np.int32)
        ro = np.full(4, -1, np.int64)
        post, mel = np.full(300, 77, np.float32), np.full((300, eng.n_mel), 77, np.float32)

        def feed(fn, bank, offs):
            return fn(bank._h, _lib.ptr(ids), 3, _lib.ptr(data), _lib.ptr(np.array(offs, np.int64)), 300, _lib.ptr(ro), _lib.ptr(post), _lib.ptr(mel))

        def untouched():
            return (ro == -1).all() and (post == 77).all() and (mel == 77).all()
        assert feed(lib.ww_stream_feed, plain, [0, 3000, 6000, 9000]) == _lib.WW_EINVAL and "ww_stream_feed_bytes" in err() and untouched()
        assert feed(lib.ww_stream_feed_all, plain, [0, 3000, 6000, 9000]) == _lib.WW_EINVAL and untouched()
        assert feed(lib.ww_stream_feed_bytes, plain, [0, 6001, 12000, 20001]) == _lib.WW_EINVAL and "packet 0" in err() and "odd length" in err() and untouched()
        assert feed(lib.ww_stream_feed_bytes, plain, [1, 6001, 12000, 20001]) == _lib.WW_EINVAL and "packet 0" in err() and "odd offset" in err() and untouched()
        assert feed(lib.ww_stream_feed_bytes_all, plain, [0, 6000, 12000, 20001]) == _lib.WW_EINVAL and "ww_stream_step" in err() and untouched()
        offs = [2, 6002, 12001, 20001]  # int16 from an even byte; the G.711 packets have odd lengths and start anywhere
        assert feed(lib.ww_stream_feed_bytes, plain, offs) == _lib.WW_OK, err()
        got = (ro.copy(), post.copy(), mel.copy())
        ro[:], post[:], mel[:] = -1, 77, 77
        assert feed(lib.ww_stream_feed_bytes, twin, offs) == _lib.WW_OK, err()
        assert ro[3] > 100
        assert_array_equal(got[0], ro), assert_array_equal(_bits(got[1]), _bits(post)), assert_array_equal(_bits(got[2]), _bits(mel))
        # ... and against the decoded packets through ww_stream_feed
        dec = StreamBank(eng, 3, causal=True, sample_rate=[8000, 16000, 8000])
        banks.append(dec)
        wp, wm = dec.feed([1, 0, 2], [data[2:6002].view(np.int16), tables["mulaw"][data[6002:12001]], tables["alaw"][data[12001:20001]]], want_mel=True)
        assert_array_equal(_bits(np.concatenate(wp)), _bits(post[:ro[3]])), assert_array_equal(_bits(np.concatenate(wm)), _bits(mel[:ro[3]]))
    finally:
        for b in banks:
            b.close()
        rs.close()
