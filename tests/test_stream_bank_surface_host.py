"""``StreamBank``'s one layout routine and one frames routine, on the host: the five bank kinds built through ``__new__`` with a stub
library that answers ``ww_stream_frame_layout_bytes`` - the six public layout attributes against values written out here by hand,
and the accepted frame forms staged to byte-identical blocks.  Nothing here touches a device."""
import ctypes as C

import numpy as np
import pytest

S = 3
# kind -> (per-stream form?, G.711 streams?, what the library states: frame bytes, byte offsets, formats (WW_SAMPLE_*: 0, 8, 9),
#          and by hand: frame_samples, frame_offs, sample_rates, sample_formats)
KINDS = {
    "plain": (False, False, [640, 640, 640], [0, 640, 1280, 1920], [0, 0, 0],
              320, [0, 320, 640, 960], [16000, 16000, 16000], ["pcm16", "pcm16", "pcm16"]),
    "uniform 8000 pcm16": (False, False, [320, 320, 320], [0, 320, 640, 960], [0, 0, 0],
                           160, [0, 160, 320, 480], [8000, 8000, 8000], ["pcm16", "pcm16", "pcm16"]),
    "uniform 8000 mulaw": (False, True, [160, 160, 160], [0, 160, 320, 480], [8, 8, 8],
                           160, None, [8000, 8000, 8000], ["mulaw", "mulaw", "mulaw"]),
    "per-stream pcm16": (True, False, [1920, 640, 320], [0, 1920, 2560, 2880], [0, 0, 0],
                         [960, 320, 160], [0, 960, 1280, 1440], [48000, 16000, 8000], ["pcm16", "pcm16", "pcm16"]),
    # (8050 Hz mu-law: a frame of 161 bytes, so the int16 frame behind it starts behind one pad byte)
    "per-stream g711": (True, True, [161, 640, 160], [0, 162, 802, 962], [8, 0, 9],
                        [161, 320, 160], None, [8050, 16000, 8000], ["mulaw", "pcm16", "alaw"]),
}


class _StubLib:
    """Answers ``ww_stream_frame_layout_bytes`` from a table and counts the calls; any other entry point is an AttributeError."""

    def __init__(self, fb, bo, fm):
        self.fb, self.bo, self.fm = np.array(fb, np.int32), np.array(bo, np.int64), np.array(fm, np.int32)
        self.calls = 0

    def ww_stream_frame_layout_bytes(self, h, p_fb, p_bo, p_fm):
        self.calls += 1
        for dst, src in ((p_fb, self.fb), (p_bo, self.bo), (p_fm, self.fm)):
            C.memmove(dst, src.ctypes.data, src.nbytes)
        return 0


class _Eng:
    class ctx:
        handle = None


def _bank(kind):
    from wwhip.engine import StreamBank
    mixed, g711, fb, bo, fm = KINDS[kind][:5]
    bank = StreamBank.__new__(StreamBank)
    bank.S, bank._mixed, bank._g711, bank._keep, bank._h, bank.engine = S, mixed, g711, None, None, _Eng()
    bank._lib = _StubLib(fb, bo, fm)
    bank._read_layout()
    assert bank._lib.calls == 1
    return bank


def _staged(bank, frames):
    """The bytes at the address ``_frames_address`` returns: the caller's array on the fast path, else the block the bank keeps."""
    bank._keep = None
    addr = bank._frames_address(frames)
    block = frames if bank._keep is None else bank._keep
    assert addr == block.ctypes.data and block.flags.c_contiguous
    return block.tobytes()


@pytest.mark.parametrize("kind", list(KINDS))
def test_layout_attributes_against_values_written_by_hand(kind):
    """``frame_bytes``, ``frame_byte_offs``, ``sample_formats``, ``frame_samples``, ``frame_offs`` and ``sample_rates`` of each bank
    kind from ONE routine and one library call: a bank at one rate keeps its scalar ``frame_samples``, a bank with G.711 streams has
    no ``frame_offs``, the others' are the byte offsets halved."""
    _, _, fb, bo, _, frame_samples, frame_offs, rates, names = KINDS[kind]
    bank = _bank(kind)
    assert bank.frame_bytes.dtype == np.int32 and bank.frame_bytes.tolist() == fb
    assert bank.frame_byte_offs.dtype == np.int64 and bank.frame_byte_offs.tolist() == bo
    assert bank.sample_formats == names
    if isinstance(frame_samples, int):
        assert type(bank.frame_samples) is int and bank.frame_samples == frame_samples
    else:
        assert bank.frame_samples.dtype == np.int32 and bank.frame_samples.tolist() == frame_samples
    if frame_offs is None:
        assert bank.frame_offs is None
    else:
        assert bank.frame_offs.dtype == np.int64 and bank.frame_offs.tolist() == frame_offs
    assert bank.sample_rates.dtype == np.int32 and bank.sample_rates.tolist() == rates


# kind -> (StreamBank's keywords, the library calls its construction makes in order, the classes it keeps)
BUILDS = {
    "plain": ({}, ["ww_stream_create", "ww_stream_frame_layout_bytes"], None),
    "uniform 8000 pcm16": ({"sample_rate": 8000}, ["ww_stream_create", "ww_stream_attach_resampler", "ww_stream_frame_layout_bytes"], None),
    "uniform 8000 mulaw": ({"sample_rate": 8000, "sample_format": "mulaw"},
                           ["ww_stream_create", "ww_stream_attach_resampler_fmt", "ww_stream_frame_layout_bytes"], None),
    "per-stream pcm16": ({"sample_rate": [48000, 16000, 8000]}, ["ww_stream_create", "ww_stream_attach_rates", "ww_stream_frame_layout_bytes"],
                         [(48000, "pcm16"), (16000, "pcm16"), (8000, "pcm16")]),
    "per-stream g711": ({"sample_rate": [8050, 16000, 8000], "sample_format": ["mulaw", "pcm16", "alaw"]},
                        ["ww_stream_create", "ww_stream_attach_rates_fmt", "ww_stream_frame_layout_bytes"],
                        [(8050, "mulaw"), (16000, "pcm16"), (8000, "alaw")]),
}


class _RecordingLib(_StubLib):
    """The stub that also creates a bank and takes whatever attach call it is given, by name."""

    def __init__(self, fb, bo, fm):
        super().__init__(fb, bo, fm)
        self.names = []

    def ww_stream_frame_layout_bytes(self, *a):
        self.names.append("ww_stream_frame_layout_bytes")
        return super().ww_stream_frame_layout_bytes(*a)

    def __getattr__(self, name):
        if not name.startswith("ww_stream_"):
            raise AttributeError(name)

        def call(*a):
            self.names.append(name)
            if name == "ww_stream_create":
                a[-1]._obj.value = 0x1000  # the handle, through byref
            return 0
        return call


@pytest.mark.parametrize("kind", list(BUILDS))
def test_one_construction_path_makes_each_kinds_calls(kind, monkeypatch):
    """``StreamBank(...)`` of each kind against a recording stub: one create, the kind's one attach call (none on a plain bank; a
    scalar rate with a scalar format stays the uniform bank), one layout read - and a sequence of rates stays the per-stream form
    even with one distinct rate, as does a scalar 16000 Hz with a G.711 format."""
    from wwhip import _lib, engine, resample

    class _Rs:
        def __init__(self, rate_in, rate_out, ctx):
            self.rate_in, self._h = rate_in, 0x2000 + rate_in

        def close(self):
            pass

    class _Engine(_Eng):
        handle = None

    kw, calls, classes = BUILDS[kind]
    lib = _RecordingLib(*KINDS[kind][2:5])
    monkeypatch.setattr(_lib, "load", lambda: lib)
    monkeypatch.setattr(resample, "Resampler", _Rs)
    bank = engine.StreamBank(_Engine(), S, **kw)
    assert lib.names == calls
    assert bank._classes == classes and bank._mixed == kind.startswith("per-stream") and bank._g711 == (KINDS[kind][1])
    assert bank.sample_rate == (None if bank._mixed else KINDS[kind][7][0])
    assert bank.sample_rates.tolist() == KINDS[kind][7]
    bank._h = None  # (nothing to destroy)
    if kind != "plain":
        return
    # the same 16 kHz pcm16 frames asked for per stream, and 16 kHz G.711: the per-stream form, not the plain or the uniform bank
    for kw2, attach, layout in (({"sample_rate": [16000, 16000, 16000]}, "ww_stream_attach_rates", KINDS["plain"][2:5]),
                                ({"sample_rate": 16000, "sample_format": "mulaw"}, "ww_stream_attach_rates_fmt",
                                 ([320, 320, 320], [0, 320, 640, 960], [8, 8, 8]))):
        lib2 = _RecordingLib(*layout)
        monkeypatch.setattr(_lib, "load", lambda: lib2)
        b2 = engine.StreamBank(_Engine(), S, **kw2)
        assert lib2.names == ["ww_stream_create", attach, "ww_stream_frame_layout_bytes"] and b2._mixed and len(b2._classes) == 1
        b2._h = None


@pytest.mark.parametrize("kind", list(KINDS))
def test_accepted_frame_forms_stage_byte_identical_blocks(kind):
    """The flat block, S per-stream arrays and - where every stream's frame has one length and one dtype - the 2-D array come to the
    same bytes at the address the library is given: each stream's samples at its ``frame_byte_offs``, the pad byte zero.  The
    bank's own dtype, contiguous and of its own shape, is passed without a copy."""
    mixed, g711, fb, bo, fm = KINDS[kind][:5]
    bank = _bank(kind)
    rng = np.random.default_rng(len(kind))
    per = [rng.integers(0, 256, fb[s], dtype=np.uint8) if fm[s] else rng.integers(-32768, 32768, fb[s] // 2).astype(np.int16) for s in range(S)]
    want = np.zeros(bo[S], np.uint8)
    for s in range(S):
        want[bo[s]:bo[s] + fb[s]] = per[s].view(np.uint8)
    want = want.tobytes()
    flat = np.frombuffer(want, np.uint8 if g711 else np.int16)
    assert _staged(bank, flat) == want
    assert _staged(bank, per) == want
    if mixed:
        bank._keep = None
        bank._frames_address(flat.copy())
        assert bank._keep is None  # the flat block of a per-stream bank is its fast path
    else:
        two_d = np.stack(per)
        assert _staged(bank, two_d) == want
        assert bank._keep is None  # [S, frame_samples] of the bank's dtype: no copy
    if not g711:  # a bank without G.711 streams converts what it is given to int16, as it always did
        assert _staged(bank, flat.astype(np.int32)) == want
        assert _staged(bank, [p.astype(np.int64) for p in per]) == want
    else:         # one with them refuses an array of the other kind
        with pytest.raises(ValueError, match="uint8"):
            bank._frames_address(np.zeros(bo[S] // 2, np.int16))
