"""G.711 (ITU-T) audio: one byte per sample, mu-law or A-law, as a telephony leg carries it.

The decoded value of a code is the 16-bit sample ``audioop.ulaw2lin(b, 2)`` / ``audioop.alaw2lin(b, 2)`` give (``include/wwhip.h``
states the integer formulas).  The library decodes in the kernels that read the samples - :class:`wwhip.resample.Resampler` takes
``law="mulaw"`` / ``law="alaw"`` and uint8 arrays - so nothing here is on a hot path: :func:`table` and :func:`decode` are for tests,
tools and callers that want the int16 signal on the host, and :func:`read_wav` is the small RIFF reader for G.711 wav files, which
the ``wave`` module refuses (``unknown format: 7``).
"""
from __future__ import annotations

import ctypes as C
import struct
from typing import NamedTuple, Optional

import numpy as np

LAWS = {"mulaw": 8, "alaw": 9}  # include/wwhip.h: WW_SAMPLE_MULAW, WW_SAMPLE_ALAW
_WAV_TAGS = {7: "mulaw", 6: "alaw"}  # WAVE_FORMAT_MULAW, WAVE_FORMAT_ALAW


def sample_format(law: str) -> int:
    """The library's sample format of a law name."""
    try:
        return LAWS[law]
    except (KeyError, TypeError):
        raise ValueError(f"unknown G.711 law {law!r}: 'mulaw' or 'alaw'") from None


def table(law: str) -> np.ndarray:
    """The 256 decoded int16 values of ``law``, from the library (``ww_g711_table``; host only, no GPU)."""
    from . import _lib
    t = np.zeros(256, np.int16)
    rc = _lib.load().ww_g711_table(sample_format(law), _lib.ptr(t))
    if rc != _lib.WW_OK:
        raise ValueError(f"ww_g711_table refused {law!r} ({rc})")
    return t


def decode(codes, law: str) -> np.ndarray:
    """uint8 codes (any shape) -> the int16 samples."""
    codes = np.asarray(codes)
    if codes.dtype != np.uint8:
        raise ValueError(f"G.711 codes are uint8, not {codes.dtype}")
    return table(law)[codes]


class G711Wav(NamedTuple):
    law: str
    rate: int
    channels: int
    frames: int
    codes: Optional[np.ndarray]  # uint8 [frames, channels]; None when only the header was asked for


def read_wav(path: str, header_only: bool = False) -> Optional[G711Wav]:
    """A G.711 wav: ``fmt `` tag 6 (A-law) or 7 (mu-law), 8 bits per sample, a 16- or 18-byte ``fmt `` chunk; ``fact`` and chunks of
    unknown kinds are skipped.  Returns None for a RIFF/WAVE file of another format tag (PCM: the ``wave`` module's business);
    raises ``ValueError`` for a file that is not RIFF/WAVE or a G.711 header that is not as described."""
    with open(path, "rb") as f:
        head = f.read(12)
        if len(head) < 12 or head[:4] != b"RIFF" or head[8:12] != b"WAVE":
            raise ValueError(f"{path}: not a RIFF/WAVE file")
        fmt = None
        while True:
            ck = f.read(8)
            if len(ck) < 8:
                raise ValueError(f"{path}: no data chunk" if fmt else f"{path}: no fmt chunk")
            kind, size = ck[:4], struct.unpack("<I", ck[4:])[0]
            if kind == b"fmt ":
                body = f.read(size)
                if len(body) != size or size < 16:
                    raise ValueError(f"{path}: truncated fmt chunk")
                tag, channels, rate, _, _, bits = struct.unpack("<HHIIHH", body[:16])
                if tag not in _WAV_TAGS:
                    return None
                if size not in (16, 18):
                    raise ValueError(f"{path}: a G.711 fmt chunk has 16 or 18 bytes, not {size}")
                if bits != 8:
                    raise ValueError(f"{path}: G.711 has 8 bits per sample, not {bits}")
                if channels < 1 or rate < 1:
                    raise ValueError(f"{path}: {channels} channels at {rate} Hz")
                fmt = (_WAV_TAGS[tag], int(rate), int(channels))
            elif kind == b"data":
                if fmt is None:
                    raise ValueError(f"{path}: data chunk in front of the fmt chunk")
                law, rate, channels = fmt
                if header_only:
                    return G711Wav(law, rate, channels, size // channels, None)
                raw = f.read(size)
                frames = len(raw) // channels
                codes = np.frombuffer(raw, np.uint8)[:frames * channels].reshape(frames, channels)
                return G711Wav(law, rate, channels, frames, codes)
            else:
                f.seek(size, 1)
            if size & 1:
                f.seek(1, 1)  # chunks are word-aligned
