"""Sample-rate conversion in front of the 16 kHz pipeline: where the reference's entry points call
``librosa.load(path, sr=16000)`` (``utils/evaluate_models.py:46``, ``utils/filter_dataset_to_h5.py:70``).

NOT librosa's bits: librosa resamples with third-party filters (``soxr_hq``, ``kaiser_best`` in older versions).  The transform
here is a rational-ratio polyphase windowed-sinc filter stated once in float64 (:func:`design`) and evaluated in fp32 by the
kernels of ``csrc/resample.hip``::

    g = gcd(rate_in, rate_out); up = rate_out / g; down = rate_in / g; L = rate_in * up
    f2 = rolloff * min(rate_in, rate_out) / L;  half = ceil(zeros / f2)
    h[i] = up * f2 * sinc(f2 * i) * kaiser(2 * half + 1, beta)[i + half],  i = -half .. half
    y[m] = sum_k h[m * down - k * up] * x[k]   over |m * down - k * up| <= half,   m = 0 .. ceil(n * up / down) - 1

which is ``scipy.signal.resample_poly(x, up, down, window=h / up)``.  ``x`` reads as zero outside the clip; int16 input is scaled
by exactly 1 / 32768 as librosa does.  When ``rate_in == rate_out`` there is no filter and the output is the input bit for bit.

An output sample's bits depend on its index ``m``, the filter and the input samples of its span only (one fp32 ``fmaf`` chain in
ascending ``k``): not on the batch, the launch, or how a stream was cut - :class:`StreamResampler` delivers the one-shot's bits.

:func:`design` and the range arithmetic need no GPU; :class:`Resampler` does (there is no CPU fallback).
"""
from __future__ import annotations

import ctypes as C
import math
import threading
import wave
from typing import Callable, List, Optional, Sequence, Tuple, Union

import numpy as np

ZEROS, ROLLOFF, BETA = 32, 0.945, 14.769656459379492


def ratio(rate_in: int, rate_out: int) -> Tuple[int, int]:
    """``(up, down)`` of ``rate_in -> rate_out`` in lowest terms."""
    rate_in, rate_out = int(rate_in), int(rate_out)
    if rate_in <= 0 or rate_out <= 0:
        raise ValueError(f"sample rates must be positive ({rate_in} -> {rate_out})")
    g = math.gcd(rate_in, rate_out)
    return rate_out // g, rate_in // g


def design(rate_in: int, rate_out: int, zeros: int = ZEROS, rolloff: float = ROLLOFF, beta: float = BETA) -> Tuple[int, int, int, np.ndarray]:
    """The filter in float64: ``(up, down, half, h)`` with ``h[i + half]`` the tap at offset ``i`` on the common grid
    ``L = rate_in * up``.  Equal rates: ``(1, 1, 0, [1.0])``."""
    up, down = ratio(rate_in, rate_out)
    if up == 1 and down == 1:
        return 1, 1, 0, np.ones(1, np.float64)
    L = float(int(rate_in) * up)
    f2 = float(rolloff) * float(min(int(rate_in), int(rate_out))) / L
    half = int(np.ceil(float(zeros) / f2))
    i = np.arange(-half, half + 1, dtype=np.float64)
    h = up * f2 * np.sinc(f2 * i) * np.kaiser(2 * half + 1, float(beta))
    return up, down, half, h


def taps_per_output(up: int, half: int) -> int:
    return -(-(2 * half + 1) // up)


def out_len(n: int, up: int, down: int) -> int:
    """``ceil(n * up / down)``: librosa's output length."""
    return -(-int(n) * up // down)


def history(up: int, half: int) -> int:
    """Samples in front of ``floor(m * down / up)`` that output ``m`` can reach: ``ceil(half / up)``."""
    return -(-half // up)


def determined(n_in: int, up: int, down: int, half: int) -> int:
    """Outputs fixed by the first ``n_in`` samples of a signal that goes on: output ``m`` is, once input
    ``floor((m * down + half) / up)`` has arrived."""
    return max(0, (int(n_in) * up - half - 1) // down + 1)


def first_needed(m: int, up: int, down: int, half: int) -> int:
    """Index of the first input sample output ``m`` reads (clamped at 0)."""
    return max(0, -(-(int(m) * down - half) // up))


_SAMPLE = {np.dtype(np.int16): 0, np.dtype(np.float32): 1}


def _sample_format(dtype, law: Optional[str] = None) -> int:
    """The library's format of samples of ``dtype``; with ``law`` ("mulaw" / "alaw"): of G.711 codes, which are uint8."""
    if law is not None:
        from .g711 import sample_format
        fmt = sample_format(law)
        if np.dtype(dtype) != np.uint8:
            raise ValueError(f"{law} samples are uint8 codes, not {np.dtype(dtype)}")
        return fmt
    try:
        return _SAMPLE[np.dtype(dtype)]
    except KeyError:
        raise ValueError(f"samples are int16 or float32, not {np.dtype(dtype)}") from None


class Resampler:
    """One ``ww_resampler``: the filter of ``rate_in -> rate_out`` resident on the context's device."""

    def __init__(self, rate_in: int, rate_out: int = 16000, ctx=None, zeros: int = ZEROS, rolloff: float = ROLLOFF, beta: float = BETA) -> None:
        from . import _lib
        self._lib = _lib
        self.ctx = ctx if ctx is not None else _lib.default_context()
        self.rate_in, self.rate_out = int(rate_in), int(rate_out)
        params = _lib.ResamplerParams(float(rolloff), float(beta), int(zeros), 0)
        h = C.c_void_p()
        self._h = None
        _lib.raise_for(_lib.load().ww_resampler_create(self.ctx.handle, self.rate_in, self.rate_out, C.byref(params), C.byref(h)), self.ctx.handle)
        self._h = h
        info = _lib.ResampleInfo()
        _lib.raise_for(_lib.load().ww_resampler_info(self._h, C.byref(info)), self.ctx.handle)
        self.up, self.down, self.half = int(info.up), int(info.down), int(info.half)
        self.taps_per_output, self.table_bytes = int(info.taps_per_output), int(info.table_bytes)
        _lib.register("resamplers", self)

    def out_len(self, n: int) -> int:
        return out_len(n, self.up, self.down)

    @property
    def history(self) -> int:
        return history(self.up, self.half)

    def ranges(self, segments: Sequence[np.ndarray], in_first: Optional[Sequence[int]], out_first: Optional[Sequence[int]],
               counts: Sequence[int], dtype=np.float32, law: Optional[str] = None) -> List[np.ndarray]:
        """Outputs ``[out_first[u], out_first[u] + counts[u])`` of the signals whose samples ``in_first[u] ..`` are
        ``segments[u]`` (all int16 or all float32; with ``law``: all uint8 G.711 codes, decoded in the kernels), in ONE launch;
        samples outside a segment read as zero."""
        lib = self._lib
        out_fmt = _sample_format(dtype)
        if len(segments) == 0:
            return []
        kinds = {np.asarray(s).dtype for s in segments}
        if len(kinds) != 1:
            raise ValueError("the segments of one call are all int16 or all float32")
        in_fmt = _sample_format(kinds.pop(), law)
        segs = [np.ascontiguousarray(s).reshape(-1) for s in segments]
        so = np.zeros(len(segs) + 1, np.int64)
        np.cumsum([len(s) for s in segs], out=so[1:])
        oo = np.zeros(len(segs) + 1, np.int64)
        np.cumsum(np.asarray(counts, np.int64), out=oo[1:])
        x = np.concatenate(segs) if len(segs) > 1 else segs[0]
        y = np.empty(int(oo[-1]), np.dtype(dtype))
        i0 = None if in_first is None else np.ascontiguousarray(in_first, np.int64)
        o0 = None if out_first is None else np.ascontiguousarray(out_first, np.int64)
        rc = lib.load().ww_resample(self._h, lib.ptr(x) if x.size else None, in_fmt, lib.ptr(so), lib.ptr(i0), lib.ptr(o0), lib.ptr(oo), len(segs),
                                    lib.ptr(y) if y.size else None, out_fmt)
        lib.raise_for(rc, self.ctx.handle)
        return [y[oo[u]:oo[u + 1]] for u in range(len(segs))]

    def range(self, x: np.ndarray, in_first: int, out_first: int, count: int, dtype=np.float32, law: Optional[str] = None) -> np.ndarray:
        return self.ranges([x], [in_first], [out_first], [count], dtype, law)[0]

    def __call__(self, clips: Union[np.ndarray, Sequence[np.ndarray]], dtype=np.float32, law: Optional[str] = None):
        """Whole clips (int16 or float32; ``law="mulaw"`` / ``"alaw"``: uint8 G.711 codes): a list in, a list of ``dtype`` arrays
        out; one array in, one out.  G.711 clips give the bits their decoded int16 samples give."""
        single = isinstance(clips, np.ndarray)
        segs = [clips] if single else list(clips)
        out = self.ranges(segs, None, None, [self.out_len(np.asarray(s).size) for s in segs], dtype, law)
        return out[0] if single else out

    def resample_dev(self, d_in: int, in_dtype, sample_offs: np.ndarray, out_offs: np.ndarray, d_out: int, out_dtype=np.float32,
                     in_first: Optional[np.ndarray] = None, out_first: Optional[np.ndarray] = None, law: Optional[str] = None) -> None:
        """``ww_resample_dev``: device addresses (``tensor.data_ptr()``), host offset tables (int64, ``n_seg + 1`` entries);
        enqueued on the context's stream, no synchronisation.  ``law``: the input is uint8 G.711 codes (``in_dtype`` uint8)."""
        lib = self._lib
        so, oo = np.ascontiguousarray(sample_offs, np.int64), np.ascontiguousarray(out_offs, np.int64)
        if len(so) != len(oo) or len(so) < 1:
            raise ValueError("sample_offs and out_offs have n_seg + 1 entries each")
        i0 = None if in_first is None else np.ascontiguousarray(in_first, np.int64)
        o0 = None if out_first is None else np.ascontiguousarray(out_first, np.int64)
        rc = lib.load().ww_resample_dev(self._h, C.c_void_p(d_in), _sample_format(in_dtype, law), lib.ptr(so), lib.ptr(i0), lib.ptr(o0), lib.ptr(oo),
                                        len(so) - 1, C.c_void_p(d_out), _sample_format(out_dtype))
        lib.raise_for(rc, self.ctx.handle)

    def close(self) -> None:
        if self._h and not self._lib.is_shutdown():
            self._lib.load().ww_resampler_destroy(self._h)
        self._h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass


class StreamResampler:
    """A signal that arrives in packets of any size.  ``push(packet)`` returns the outputs the samples so far determine,
    ``flush()`` the tail against zeros; concatenated they are the one-shot's bits, whatever the packet sizes.

    Between calls the object keeps the samples the next output can still reach: from ``first_needed(next output)`` on, which is
    at most ``2 * ceil(half / up) + ceil(down / up)`` samples - ``ceil(half / up)`` behind the centre of the next output, and as
    many ahead of it that have arrived but do not yet determine it.  During a push the packet is appended to them.  The arithmetic
    is the kernel's: ``backend(samples, in_first, out_first, count) -> outputs`` defaults to :meth:`Resampler.range`.
    ``law="mulaw"`` / ``"alaw"``: the packets are uint8 G.711 codes (kept as codes between calls, decoded in the kernels)."""

    def __init__(self, rate_in: int, rate_out: int = 16000, ctx=None, backend: Optional[Callable] = None, dtype=np.float32,
                 zeros: int = ZEROS, rolloff: float = ROLLOFF, beta: float = BETA, law: Optional[str] = None) -> None:
        self.up, self.down = ratio(rate_in, rate_out)
        self.dtype = np.dtype(dtype)
        self.law = law
        if law is not None:
            _sample_format(np.uint8, law)
            if backend is not None:
                raise ValueError("a G.711 stream is decoded by the library's kernels: no backend")
        if backend is None:
            self._rs = Resampler(rate_in, rate_out, ctx, zeros, rolloff, beta)
            self.half = self._rs.half
            backend = lambda x, i0, o0, n: self._rs.range(x, i0, o0, n, self.dtype, self.law)  # noqa: E731
        else:
            self._rs = None
            self.half = design(rate_in, rate_out, zeros, rolloff, beta)[2] if (self.up, self.down) != (1, 1) else 0
        self._backend = backend
        self.reset()

    def reset(self) -> None:
        self._hist: Optional[np.ndarray] = None  # samples [_hist_first, n_in) of the signal
        self._hist_first = 0
        self.n_in = 0
        self.n_out = 0

    def _emit(self, buf: np.ndarray, upto: int) -> np.ndarray:
        count = upto - self.n_out
        if count <= 0:
            return np.zeros(0, self.dtype)
        y = self._backend(buf, self._hist_first, self.n_out, count)
        self.n_out = upto
        return y

    def push(self, packet: np.ndarray) -> np.ndarray:
        packet = np.ascontiguousarray(packet).reshape(-1)
        _sample_format(packet.dtype, self.law)
        if self._hist is None:
            self._hist = packet[:0].copy()
        elif packet.dtype != self._hist.dtype:
            raise ValueError(f"this stream's samples are {self._hist.dtype}, not {packet.dtype}")
        buf = np.concatenate((self._hist, packet)) if len(packet) else self._hist
        self.n_in += len(packet)
        y = self._emit(buf, determined(self.n_in, self.up, self.down, self.half))
        keep = first_needed(self.n_out, self.up, self.down, self.half)
        if keep > self._hist_first:
            buf = buf[keep - self._hist_first:]
            self._hist_first = keep
        self._hist = buf if buf.base is None else buf.copy()  # (never a view of a long-gone packet)
        return y

    def flush(self) -> np.ndarray:
        """The outputs that were waiting for samples, computed against zeros: ``ceil(n * up / down)`` in all."""
        buf = self._hist if self._hist is not None else np.zeros(0, np.uint8 if self.law else np.float32)
        return self._emit(buf, out_len(self.n_in, self.up, self.down))

    def close(self) -> None:
        if self._rs is not None:
            self._rs.close()


_tls = threading.local()


def _cached(rate_in: int, rate_out: int, device: int = 0) -> Resampler:
    """The calling thread's default-filter resampler of a rate pair (one ``ww_ctx`` per host thread)."""
    from . import _lib
    ctx = _lib.default_context(device)
    cache = _tls.__dict__.setdefault("rs", {})
    r = cache.get((rate_in, rate_out, device))
    if r is None or r._h is None or r.ctx is not ctx:
        r = cache[(rate_in, rate_out, device)] = Resampler(rate_in, rate_out, ctx)
    return r


def _g711_wav(path: str, header_only: bool = False):
    """The file as :class:`wwhip.g711.G711Wav` when it is a G.711 wav; None for everything else (which ``wave`` then judges)."""
    from .g711 import read_wav
    try:
        return read_wav(path, header_only)
    except ValueError as e:
        if "not a RIFF/WAVE" in str(e):
            return None
        raise


def read_pcm16(path: str) -> Tuple[np.ndarray, int]:
    """A PCM16 wav as ``(int16 [frames, channels], rate)``."""
    with wave.open(path, "rb") as w:
        if w.getsampwidth() != 2:
            raise ValueError(f"{path}: only 16-bit PCM is supported")
        raw = np.frombuffer(w.readframes(w.getnframes()), dtype=np.int16)
        return raw.reshape(-1, w.getnchannels()), w.getframerate()


def load(path: str, sr: int = 16000, mono: bool = True, device: int = 0) -> np.ndarray:
    """The reference's ``librosa.load(path, sr=16000)`` call shape for PCM16 wavs at ANY rate: float32 in [-1, 1) at ``sr``,
    channels averaged as :func:`wwhip.evaluate.read_wav` does (``mono=False``: ``[channels, n]``).  The filter is this module's,
    not librosa's.  Plugs into the ``loader=`` hook of ``get_posterior`` / ``get_posterior_sharded`` / ``DatasetFilter``.
    A G.711 wav (mu-law or A-law) is read too: a mono file's (and with ``mono=False`` every channel's) bytes go up once and are
    decoded and resampled in one device pass - also when the file is at ``sr`` already, where the pass is the decode alone."""
    g = _g711_wav(str(path))
    if g is not None:
        if g.channels == 1 or not mono:
            codes = [np.ascontiguousarray(g.codes[:, c]) for c in range(g.channels)]
            out = _cached(g.rate, int(sr), device)(codes, np.float32, law=g.law)
            return out[0] if mono else np.stack(out)
        from .g711 import decode
        pcm, rate = decode(g.codes, g.law), g.rate  # channels are averaged as decoded samples: a host pass, as for PCM16
    else:
        pcm, rate = read_pcm16(str(path))
    ch = pcm.shape[1]
    if mono and ch > 1:
        clips: List[np.ndarray] = [(pcm.astype(np.float32).mean(axis=1) / np.float32(32768.0)).astype(np.float32)]
    else:
        clips = [np.ascontiguousarray(pcm[:, c]) for c in range(ch)]
    if rate == sr:
        out = [c if c.dtype == np.float32 else c.astype(np.float32) / np.float32(32768.0) for c in clips]
    else:
        out = _cached(rate, int(sr), device)(clips, np.float32)
    return out[0] if mono else np.stack(out)
