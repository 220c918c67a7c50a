"""G.711 (mu-law / A-law) input, on the host: the decode table against ITU-T G.711's integer formulas, csrc/stream_formats.h under
Address + UB sanitizer (a stand-alone program), the ctypes binding of the six new entry points, what ``StreamBank(sample_format=)``
refuses before it touches a device, and the RIFF reader for G.711 wav files."""
import ctypes as C
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CSRC = os.path.join(_ROOT, "wakeword-detection_amd", "csrc")
NEW_SYMBOLS = ["ww_g711_table", "ww_stream_attach_rates_fmt", "ww_stream_attach_resampler_fmt", "ww_stream_frame_layout_bytes",
               "ww_stream_feed_bytes", "ww_stream_feed_bytes_all"]
MULAW, ALAW = 8, 9


def mulaw_formula(code):
    v = ~code & 0xFF
    t = (((v & 0x0F) << 3) + 0x84) << ((v & 0x70) >> 4)
    return 0x84 - t if v & 0x80 else t - 0x84


def alaw_formula(code):
    v = code ^ 0x55
    t = (v & 0x0F) << 4
    seg = (v & 0x70) >> 4
    t = t + 8 if seg == 0 else (t + 0x108) << (seg - 1)
    return t if v & 0x80 else -t


def _table(fmt):
    from wwhip import _lib
    t = np.full(256, 12345, np.int16)
    return _lib.load().ww_g711_table(fmt, _lib.ptr(t)), t


def test_table_is_g711_for_all_codes():
    """``ww_g711_table`` against the issue's formulas for all 256 codes of both laws, the spot values, and ``audioop`` where this
    interpreter still has it; other formats are WW_EINVAL and write nothing."""
    from wwhip import g711
    rc, mu = _table(MULAW)
    assert rc == 0
    np.testing.assert_array_equal(mu, np.array([mulaw_formula(c) for c in range(256)], np.int16))
    rc, al = _table(ALAW)
    assert rc == 0
    np.testing.assert_array_equal(al, np.array([alaw_formula(c) for c in range(256)], np.int16))
    assert (mu[0x00], mu[0x7F], mu[0x80], mu[0xFF]) == (-32124, 0, 32124, 0)
    assert (al[0x55], al[0xD5], al[0x2A], al[0xAA]) == (-8, 8, -32256, 32256)
    assert (mu.min(), mu.max(), len(set(mu.tolist()))) == (-32124, 32124, 255)
    assert (al.min(), al.max(), len(set(al.tolist()))) == (-32256, 32256, 256)
    try:
        import audioop
    except ImportError:
        audioop = None
    if audioop is not None:
        codes = bytes(range(256))
        np.testing.assert_array_equal(mu, np.frombuffer(audioop.ulaw2lin(codes, 2), np.int16))
        np.testing.assert_array_equal(al, np.frombuffer(audioop.alaw2lin(codes, 2), np.int16))
    for bad in (2, 10, 0, 1):
        rc, t = _table(bad)
        assert rc == -1 and (t == 12345).all()
    from wwhip import _lib
    assert _lib.load().ww_g711_table(MULAW, None) == -1
    np.testing.assert_array_equal(g711.table("mulaw"), mu)
    np.testing.assert_array_equal(g711.table("alaw"), al)
    codes = np.arange(512, dtype=np.int64).astype(np.uint8).reshape(2, 256)
    np.testing.assert_array_equal(g711.decode(codes, "alaw"), al[codes])
    assert g711.decode(codes, "mulaw").dtype == np.int16
    with pytest.raises(ValueError, match="unknown G.711 law"):
        g711.table("ulaw")
    with pytest.raises(ValueError, match="uint8"):
        g711.decode(np.zeros(4, np.int16), "mulaw")


def _no_sanitizer_runtime(output):
    """Did a -fsanitize build fail because this clang ships no runtime for it?  (tests/test_stream_rate_host.py's rule.)"""
    return re.search(r"libclang_rt\.|unsupported (option|argument)[^\n]*-fsanitize", output) is not None


@pytest.fixture(scope="module")
def check_run(tmp_path_factory):
    """tests/native/stream_formats_check.cpp compiled with Address + UB sanitizer and run once, as a child process (nothing is loaded
    into this interpreter): the finished process, or a skip where there is no compiler or no sanitizer runtime."""
    cxx = "/opt/rocm/lib/llvm/bin/clang++"
    if not os.path.exists(cxx):
        cxx = shutil.which("clang++")
    if cxx is None:
        pytest.skip("no clang++ in this image")
    exe = tmp_path_factory.mktemp("stream_formats") / "stream_formats_check"
    b = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-I" + _CSRC,
                        os.path.join(_ROOT, "tests", "native", "stream_formats_check.cpp"), "-o", str(exe)], capture_output=True, text=True)
    if b.returncode != 0 and _no_sanitizer_runtime(b.stderr + b.stdout):
        pytest.skip("this clang has no sanitizer runtime: " + b.stderr[-300:])
    assert b.returncode == 0, b.stderr[-2000:]
    return subprocess.run([str(exe)], capture_output=True, text=True, timeout=120,
                          env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1"))


def test_stream_formats_header_under_sanitizers(check_run):
    """csrc/stream_formats.h - (rate, format) classes and their refusals, the byte layout (int16 frames on even bytes, G.711 frames
    anywhere, pad bytes in front of int16 frames only, ascending offsets, the right total), its maximum over random move scripts,
    the all-int16 bank against stream_rates.h, and the packet refusals - compiled alone with Address + UB sanitizer and checked on
    the CPU (tests/native/stream_formats_check.cpp lists the properties)."""
    r = check_run
    last = r.stdout.strip().splitlines()[-1] if r.stdout.strip() else ""
    assert r.returncode == 0 and last.startswith("ok ") and not r.stderr.strip(), (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    assert int(last.split()[1]) > 100000
    lay = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("layout ")]
    assert len(lay) == 1
    f = lay[0]
    bar = f.index("|")
    # (8000 mu-law), (8000 A-law), (8000 pcm16), (16000 mu-law), (16000 pcm16), (8050 mu-law), (48000 pcm16): the pad byte behind the odd frame
    assert [int(v) for v in f[2:bar]] == [160, 160, 320, 320, 640, 161, 1920]
    assert [int(v) for v in f[bar + 1:]] == [0, 160, 320, 640, 960, 1600, 1762, 3682]


def test_stream_formats_header_is_host_only():
    """stream_formats.h includes no HIP header and calls no HIP function (the text rule of stream_rate.h and stream_rates.h), builds
    on stream_rates.h, is what common.h and the build's dependency list name, and stream_rate.h knows nothing of it."""
    text = open(os.path.join(_CSRC, "stream_formats.h")).read()
    code = re.sub(r"//[^\n]*", "", text)
    assert "hip/" not in code and "common.h" not in code and not re.search(r"\bhip[A-Z]\w*\(", code)
    assert "__global__" not in code and "__shared__" not in code and "__device__" not in code
    assert '#include "stream_rates.h"' in code
    assert "stream_formats" not in open(os.path.join(_CSRC, "stream_rate.h")).read()
    assert "stream_formats" not in re.sub(r"//[^\n]*", "", open(os.path.join(_CSRC, "stream_rates.h")).read())
    assert '#include "stream_formats.h"' in open(os.path.join(_CSRC, "common.h")).read()
    assert '"stream_formats.h"' in open(os.path.join(_ROOT, "wakeword-detection_amd", "wwhip", "_build.py")).read()


def test_binding_covers_the_new_entry_points():
    from wwhip import _lib
    header = open(os.path.join(_ROOT, "include", "wwhip.h")).read()
    assert re.search(r"#define WW_ABI 4\b", header) and _lib.ABI == 4
    assert re.search(r"#define WW_SAMPLE_MULAW 8\b", header) and re.search(r"#define WW_SAMPLE_ALAW 9\b", header)
    assert (_lib.SAMPLE_MULAW, _lib.SAMPLE_ALAW) == (8, 9)
    assert not re.search(r"#define WW_SAMPLE_\w+ 2\b", header)  # value 2 stays no format
    for name in NEW_SYMBOLS:
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert m, f"{name} is not declared in include/wwhip.h"
        assert name in _lib.SYMBOLS, f"{name} is not bound in wwhip/_lib.py"
        assert len(_lib.SYMBOLS[name][1]) == m.group(1).count(",") + 1, name
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name


def test_host_detectable_errors_raise_before_any_device_call(monkeypatch):
    from wwhip import _lib
    from wwhip.engine import StreamBank

    def no_native(*a, **k):
        raise AssertionError("a host-detectable error reached the native library")
    monkeypatch.setattr(_lib, "load", no_native)
    monkeypatch.setattr(_lib, "default_context", no_native)

    class _Eng:
        n_models = 1

    with pytest.raises(ValueError, match=r"one format per stream \(3\), got 2"):
        StreamBank(_Eng(), 3, sample_rate=8000, sample_format=["mulaw", "alaw"])
    with pytest.raises(ValueError, match="unknown sample format 'ulaw'"):
        StreamBank(_Eng(), 2, sample_rate=8000, sample_format="ulaw")
    with pytest.raises(ValueError, match="unknown sample format"):
        StreamBank(_Eng(), 2, sample_rate=[8000, 16000], sample_format=["mulaw", 7])
    with pytest.raises(ValueError, match="fractional frame"):
        StreamBank(_Eng(), 2, sample_rate=[8000, 11025], sample_format=["mulaw", "pcm16"])
    with pytest.raises(ValueError, match="9 distinct"):
        StreamBank(_Eng(), 9, sample_rate=[8000, 8000, 8000, 16000, 16000, 16000, 48000, 48000, 48000], sample_format=["pcm16", "mulaw", "alaw"] * 3)
    # a per-stream bank's frames: the flat uint8 block, or one array per stream of the stream's own dtype
    bank = StreamBank.__new__(StreamBank)
    bank.S, bank._mixed, bank._g711, bank._keep, bank._h = 3, True, True, None, None
    bank._dtype, bank._shape = np.dtype(np.uint8), (962,)
    bank.sample_formats = ["mulaw", "pcm16", "alaw"]
    bank.frame_samples = np.array([161, 320, 160], np.int32)
    bank.frame_bytes = np.array([161, 640, 160], np.int32)
    bank.frame_byte_offs = np.array([0, 162, 802, 962], np.int64)
    good = [np.zeros(161, np.uint8), np.zeros(320, np.int16), np.zeros(160, np.uint8)]
    assert bank._frames_address(good) != 0 and bank._keep.dtype == np.uint8 and bank._keep.size == 962
    assert bank._frames_address(np.zeros(962, np.uint8)) != 0
    with pytest.raises(ValueError, match="stream 1 reads pcm16: its samples are int16, not uint8"):
        bank._frames_address([good[0], np.zeros(640, np.uint8), good[2]])
    with pytest.raises(ValueError, match="stream 0 reads mulaw: its samples are uint8, not int16"):
        bank._frames_address([np.zeros(161, np.int16), good[1], good[2]])
    with pytest.raises(ValueError, match="stream 2's frame has 160 samples, got 161"):
        bank._frames_address([good[0], good[1], np.zeros(161, np.uint8)])
    with pytest.raises(ValueError, match="962 bytes"):
        bank._frames_address(np.zeros(963, np.uint8))
    with pytest.raises(ValueError, match="is uint8"):
        bank._frames_address(np.zeros(481, np.int16))
    with pytest.raises(ValueError, match="one array per stream"):
        bank._frames_address(good[:2])
    # the per-stream arrays land where the layout says, the pad byte stays zero
    fr = [np.full(161, 7, np.uint8), np.full(320, 0x0102, np.int16), np.full(160, 9, np.uint8)]
    bank._frames_address(fr)
    assert bank._keep[:161].tolist() == [7] * 161 and bank._keep[161] == 0 and bank._keep[802:].tolist() == [9] * 160
    np.testing.assert_array_equal(bank._keep[162:802].view(np.int16), fr[1])
    # packets are checked the same way, before the library is asked anything
    bank.n_members = 0
    with pytest.raises(ValueError, match="stream 1 reads pcm16"):
        bank.feed([0, 1], [np.zeros(5, np.uint8), np.zeros(5, np.uint8)])
    with pytest.raises(ValueError, match="stream 2 reads alaw"):
        bank.feed([2], [np.zeros(5, np.int16)])
    bank._classes = [(8050, "mulaw"), (16000, "pcm16"), (8000, "alaw"), (8000, "mulaw")]
    with pytest.raises(ValueError, match="names 2 of the bank's classes"):
        bank.set_rate([0], 8000)
    with pytest.raises(ValueError, match="names 0 of the bank's classes"):
        bank.set_rate([0], 8050, "alaw")
    with pytest.raises(ValueError, match="unknown sample format"):
        bank.set_rate([0], 8000, "g722")
    # the uniform bank: [S, F] uint8
    uni = StreamBank.__new__(StreamBank)
    uni.S, uni._mixed, uni._g711, uni._keep, uni._shape, uni._dtype = 2, False, True, None, (2, 160), np.dtype(np.uint8)
    uni.sample_formats, uni.frame_byte_offs = ["mulaw", "mulaw"], np.array([0, 160, 320], np.int64)
    assert uni._frames_address(np.zeros((2, 160), np.uint8)) != 0
    with pytest.raises(ValueError, match="not int16"):
        uni._frames_address(np.zeros((2, 160), np.int16))
    with pytest.raises(ValueError, match=r"\[2, 160\] uint8"):
        uni._frames_address(np.zeros((2, 161), np.uint8))


def _wav(path, tag, bits, codes, rate=8000, channels=1, fmt_size=18, fact=True, extra=True):
    """A G.711 wav written by hand: RIFF | fmt (16 or 18 bytes) | [fact] | [an odd-sized chunk of an unknown kind + its pad] | data."""
    body = struct.pack("<HHIIHH", tag, channels, rate, rate * channels * bits // 8, channels * bits // 8, bits)
    if fmt_size == 18:
        body += struct.pack("<H", 0)
    chunks = b"fmt " + struct.pack("<I", len(body)) + body
    if fact:
        chunks += b"fact" + struct.pack("<II", 4, len(codes) // channels)
    if extra:
        chunks += b"LIST" + struct.pack("<I", 5) + b"abcde" + b"\0"
    chunks += b"data" + struct.pack("<I", len(codes)) + bytes(codes)
    if len(codes) & 1:
        chunks += b"\0"
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 4 + len(chunks)) + b"WAVE" + chunks)
    return str(path)


def test_wav_reader_parses_handwritten_g711_files(tmp_path):
    """Hand-written mu-law and A-law wavs - the 18-byte ``fmt `` with a ``fact`` chunk and a chunk of an unknown kind, and the bare
    16-byte ``fmt `` - parse to their codes, which decode to the formulas' samples; ``wave`` cannot open them, a tag-7 file with 16
    bits per sample is refused, and without ``resample=True`` the evaluators' readers say what to do."""
    import wave
    from wwhip import g711
    from wwhip.evaluate import read_wav, wav_length
    rng = np.random.default_rng(711)
    codes = np.concatenate([np.arange(256, dtype=np.int64).astype(np.uint8), rng.integers(0, 256, 745, dtype=np.uint8)])  # (odd length: a pad byte)
    for law, tag, formula in (("mulaw", 7, mulaw_formula), ("alaw", 6, alaw_formula)):
        want = np.array([formula(int(c)) for c in codes], np.int16)
        for fmt_size, fact, extra in ((18, True, True), (16, False, False)):
            p = _wav(tmp_path / f"{law}_{fmt_size}.wav", tag, 8, codes, fmt_size=fmt_size, fact=fact, extra=extra)
            with pytest.raises(wave.Error):
                wave.open(p, "rb")
            g = g711.read_wav(p)
            assert (g.law, g.rate, g.channels, g.frames) == (law, 8000, 1, codes.size)
            np.testing.assert_array_equal(g.codes[:, 0], codes)
            np.testing.assert_array_equal(g711.decode(g.codes[:, 0], g.law), want)
            h = g711.read_wav(p, header_only=True)
            assert (h.law, h.rate, h.channels, h.frames, h.codes) == (law, 8000, 1, codes.size, None)
            assert wav_length(p, 16000, resample=True) == 2 * codes.size
            with pytest.raises(ValueError, match="sample rate 8000 != 16000"):
                read_wav(p)
            with pytest.raises(ValueError, match="resample=True"):
                wav_length(p, 8000)
    st = _wav(tmp_path / "stereo.wav", 7, 8, codes[:1000], channels=2)
    g = g711.read_wav(st)
    assert (g.channels, g.frames) == (2, 500)
    np.testing.assert_array_equal(g.codes, codes[:1000].reshape(500, 2))
    with pytest.raises(ValueError, match="8 bits per sample, not 16"):
        g711.read_wav(_wav(tmp_path / "bad_bits.wav", 7, 16, codes[:100]))
    with pytest.raises(ValueError, match="16 or 18 bytes"):
        body = struct.pack("<HHIIHH", 6, 1, 8000, 8000, 1, 8) + b"\0" * 4
        with open(tmp_path / "bad_fmt.wav", "wb") as f:
            f.write(b"RIFF" + struct.pack("<I", 4 + 8 + len(body)) + b"WAVE" + b"fmt " + struct.pack("<I", len(body)) + body)
        g711.read_wav(str(tmp_path / "bad_fmt.wav"))
    # a PCM16 wav is none of this reader's business
    with wave.open(str(tmp_path / "pcm.wav"), "wb") as w:
        w.setnchannels(1), w.setsampwidth(2), w.setframerate(16000)
        w.writeframes(np.arange(100, dtype=np.int16).tobytes())
    assert g711.read_wav(str(tmp_path / "pcm.wav")) is None
    np.testing.assert_array_equal(read_wav(str(tmp_path / "pcm.wav")), np.arange(100, dtype=np.float32) / np.float32(32768.0))
    with pytest.raises(ValueError, match="not a RIFF/WAVE"):
        (tmp_path / "junk.wav").write_bytes(b"not a wav file at all")
        g711.read_wav(str(tmp_path / "junk.wav"))
