"""Host-side handle on one uploaded model: thin, typed wrappers over the C ABI.

Everything here forwards to ``libwwhip.so``; nothing is computed in Python/NumPy apart from
argument marshalling.  The reference-shaped classes (``Filter``, ``TFLiteModel``,
``WakewordTrigger``, ``get_posterior`` ...) are built on top of this in the sibling modules.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from . import weights as W


def frontend_params(pcm_divisor: float = 32767.0, clip: bool = True, pre_emphasis: float = 0.0,
                    hop: int = 160, precise: bool = True) -> _lib.FrontendParams:
    return _lib.FrontendParams(float(pcm_divisor), int(bool(clip)), float(pre_emphasis), int(hop), int(bool(precise)))


def _events_args(planes: int, n: int, threshold, seg_offs):
    """The host arrays of a detection-event call, checked: one fp64 threshold per plane (a scalar serves all) and the int64 segment
    offsets (``None``: one segment)."""
    thr = np.asarray(threshold, np.float64)
    if thr.ndim == 0:
        thr = np.full(planes, float(thr))
    thr = np.ascontiguousarray(thr.ravel())
    if thr.size != planes:
        raise ValueError(f"threshold: one value, or one per plane ({planes}), got {thr.size}")
    offs = None
    if seg_offs is not None:
        offs = np.ascontiguousarray(seg_offs, dtype=np.int64)
        if offs.ndim != 1 or offs.size < 1:
            raise ValueError("seg_offs must be a 1-D array of n_seg + 1 row offsets")
    return thr, offs


def _events_call(fn, ctx, post_arg, n: int, planes: int, threshold, seg_offs, window: int, cap: Optional[int], want_counts: bool):
    """``ww_posterior_events`` / ``ww_posterior_events_dev`` into an array of :data:`wwhip._lib.EVENT_DTYPE`.  ``cap`` = ``None``: room
    for 4,096 events first, and where the call reports more, once more with room for all of them; a number: that many at the most
    (the first ``cap`` in plane, segment, start order)."""
    thr, offs = _events_args(planes, n, threshold, seg_offs)
    counts = np.zeros(planes, np.int64)
    total = C.c_int64(0)
    room = 4096 if cap is None else int(cap)
    while True:
        ev = np.zeros(max(room, 0), _lib.EVENT_DTYPE)
        _lib.raise_for(fn(ctx.handle, post_arg, int(n), int(planes), _lib.ptr(offs), 0 if offs is None else int(offs.size - 1), int(window),
                          _lib.ptr(thr), _lib.ptr(ev) if room > 0 else None, room, C.addressof(total), _lib.ptr(counts)), ctx.handle)
        if cap is not None or total.value <= room:
            break
        room = int(total.value)
    ev = ev[:min(int(total.value), max(room, 0))]
    return (ev, counts, int(total.value)) if want_counts else ev


def _events_host(ctx, post, threshold, seg_offs, window, cap, want_counts):
    p = np.ascontiguousarray(post, dtype=np.float32)
    if p.ndim == 1:
        p = p[None]
    if p.ndim != 2:
        raise ValueError("post must be 1-D, or [planes, n]")
    return _events_call(_lib.load().ww_posterior_events, ctx, _lib.ptr(p), p.shape[1], p.shape[0], threshold, seg_offs, window, cap, want_counts)


def _events_dev(ctx, d_post_ptr, n, planes, threshold, seg_offs, window, cap, want_counts):
    return _events_call(_lib.load().ww_posterior_events_dev, ctx, C.c_void_p(d_post_ptr) if d_post_ptr else None, n, planes, threshold, seg_offs,
                        window, cap, want_counts)


class Engine:
    """A model directory (filter/encode/detect ``.tflite``) resident on one MI355X."""

    def __init__(self, model_dir: str, device: int = 0, ctx: Optional[_lib.Context] = None,
                 precision: str = "fp32", weights_fp16: bool = False, bundle: Optional["W.ModelBundle"] = None) -> None:
        """``bundle``: the model as a :class:`wwhip.weights.ModelBundle` instead of a directory to read (``model_dir`` is then only a
        name) - how a CTC-trained CRNN arrives (``weights.crnn_ctc_params``)."""
        self._weights_fp16 = bool(weights_fp16)
        self._given_bundle = bundle
        self.bundle = bundle if bundle is not None else W.load_model_dir(model_dir)
        if weights_fp16:  # the reference's float16-quantised model variant (weights.quantize_fp16)
            self.bundle = W.quantize_fp16(self.bundle)
        self.blob = W.pack_blob(self.bundle)
        self.ctx = ctx if ctx is not None else _lib.default_context(device)
        self._lib = _lib.load()
        h = C.c_void_p()
        buf = np.frombuffer(self.blob, dtype=np.uint8)
        _lib.raise_for(self._lib.ww_model_load(self.ctx.handle, _lib.ptr(buf), buf.size, C.byref(h)), self.ctx.handle)
        self._model = h
        info = _lib.ModelInfo()
        _lib.raise_for(self._lib.ww_model_get_info(h, C.byref(info)), self.ctx.handle)
        self.kind = info.kind
        self.window = info.window
        self.n_mel = info.n_mel
        self.n_bins = info.n_bins
        self.n_out = info.n_out
        self.enc_shape = (info.enc_rows, info.enc_width)
        hk = C.c_int32(0)
        _lib.raise_for(self._lib.ww_model_head_kind(h, C.byref(hk)), self.ctx.handle)
        self.head_kind = int(hk.value)  # _lib.HEAD_SIGMOID | HEAD_SOFTMAX | HEAD_CTC
        # a CRNN's recurrent layers: cell (_lib.CELL_GRU | CELL_LSTM), units per direction, width of the head's first layer
        self.cell = self.units = self.head_units = None
        if self.kind == _lib.KIND_CRNN:
            rk = [C.c_int32(0) for _ in range(3)]
            _lib.raise_for(self._lib.ww_model_rnn_kind(h, *(C.byref(v) for v in rk)), self.ctx.handle)
            self.cell, self.units, self.head_units = (int(v.value) for v in rk)
        self.model_dir = model_dir
        _lib.register("models", self)
        self._options = {"crnn_split_at": 1024, "crnn_slide_min": 64, "crnn_tail_mfma": 1, "wavenet_rowmajor": 0, "wave_seq_segment": 0}  # the library's defaults
        self.precision = "fp32"
        if precision != "fp32":
            self.set_precision(precision)

    def set_precision(self, precision: str) -> None:
        """``"fp32"`` (default, fp32 MFMA) or ``"bf16x3"`` (Wavenet blocks as three bf16 MFMAs on
        split operands, fp32 accumulate; see ``ww_model_set_precision`` in include/wwhip.h)."""
        modes = {"fp32": _lib.PRECISION_FP32, "bf16x3": _lib.PRECISION_BF16X3}
        if precision not in modes:
            raise ValueError(f"precision must be one of {sorted(modes)}")
        self._chk(self._lib.ww_model_set_precision(self._model, modes[precision]))
        self.precision = precision

    def set_option(self, key: str, value: int) -> None:
        """Per-model dispatch options (``ww_model_set_option``): ``"crnn_split_at"`` - explicit-window launches above
        this many windows take front + tail kernels (0 = always one fused kernel); ``"crnn_slide_min"`` - regular
        sliding windows take the once-per-sequence form from this many windows on (0 = never); ``"crnn_tail_mfma"`` - the recurrences
        of those two forms for sixteen windows per workgroup on the matrix pipe: 1 (default) from 9,216 windows per launch on,
        2 always, 0 never (one window per workgroup on the vector ALU), any other value is refused; ``"wavenet_rowmajor"`` - 1: the fp32 Wavenet's row-major block loop of rounds 1-2 instead of the
        transposed one; ``"wave_seq_segment"`` - rows per independently computed segment of :meth:`sequence_forward` (0 = the
        library's choice; the same bits for every value)."""
        keys = {"crnn_split_at": _lib.OPT_CRNN_SPLIT_AT, "crnn_slide_min": _lib.OPT_CRNN_SLIDE_MIN,
                "crnn_tail_mfma": _lib.OPT_CRNN_TAIL_MFMA, "wavenet_rowmajor": _lib.OPT_WAVENET_ROWMAJOR,
                "wave_seq_segment": _lib.OPT_WAVE_SEQ_SEGMENT}
        if key not in keys:
            raise ValueError(f"option must be one of {sorted(keys)}")
        self._chk(self._lib.ww_model_set_option(self._model, keys[key], int(value)))
        self._options[key] = int(value)

    def options(self, **kv):
        """Context manager: the given options for the duration of a ``with`` block, the previous values afterwards."""
        import contextlib

        @contextlib.contextmanager
        def scope():
            old = {k: self._options[k] for k in kv}
            try:
                for k, v in kv.items():
                    self.set_option(k, v)
                yield self
            finally:
                for k, v in old.items():
                    self.set_option(k, v)
        return scope()

    def lane(self, k: int) -> "Engine":
        """Lane ``k`` of this engine: ``self`` for 0, otherwise a twin on a context (HIP stream) of its own - the same files, the
        same precision and dispatch options (brought in line at every call), its own 0.9 MB of weights.  Independent launches dealt
        to the lanes run beside each other on the GPU, which one stream's order forbids: the sharded evaluators give consecutive
        chunks to alternating lanes (wwhip/evaluate.py, as bench.py does with whole steps)."""
        if k == 0:
            return self
        lanes = self.__dict__.setdefault("_lanes", {})
        e = lanes.get(k)
        if e is None or e.handle is None:
            e = lanes[k] = Engine(self.model_dir, device=self.ctx.device, ctx=_lib.Context(self.ctx.device), precision=self.precision,
                                  weights_fp16=self._weights_fp16, bundle=self._given_bundle)
        if e.precision != self.precision:
            e.set_precision(self.precision)
        for key, v in self._options.items():
            if e._options[key] != v:
                e.set_option(key, v)
        return e

    # ------------------------------------------------------------------ properties
    @property
    def handle(self):
        return self._model

    @property
    def posterior_index(self) -> int:
        return self.bundle.posterior_index

    @property
    def is_crnn(self) -> bool:
        return self.kind == _lib.KIND_CRNN

    def close(self) -> None:
        for e in self.__dict__.pop("_lanes", {}).values():  # the twins on contexts of their own (lane) go with their engine
            e.close()
        if self._model and not _lib.is_shutdown():
            self._lib.ww_model_free(self._model)
        self._model = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc: int) -> None:
        _lib.raise_for(rc, self.ctx.handle)

    # ------------------------------------------------------------------ front end
    def num_frames(self, n_samples: int, hop: int = 160) -> int:
        return int(self._lib.ww_num_frames(int(n_samples), int(hop)))

    def logmel(self, pcm: Sequence[np.ndarray], fp: Optional[_lib.FrontendParams] = None) -> List[np.ndarray]:
        """List of int16 (or float32) utterances -> list of ``[frames, 40]`` log-mel arrays."""
        fp = fp or frontend_params()
        if len(pcm) == 0:
            return []
        is_f32 = np.asarray(pcm[0]).dtype != np.int16
        dt = np.float32 if is_f32 else np.int16
        arrs = [np.ascontiguousarray(p, dtype=dt).ravel() for p in pcm]
        # pad every utterance start to a multiple of 8 samples so device loads stay aligned
        offs = np.zeros(len(arrs) + 1, np.int64)
        for i, a in enumerate(arrs):
            offs[i + 1] = offs[i] + a.size
        flat = np.concatenate(arrs) if arrs else np.zeros(0, dt)
        foffs = np.zeros(len(arrs) + 1, np.int64)
        total = sum(self.num_frames(a.size, fp.hop) for a in arrs)
        mel = np.empty((total, self.n_mel), np.float32)
        fn = self._lib.ww_logmel_f32 if is_f32 else self._lib.ww_logmel
        self._chk(fn(self.ctx.handle, self._model, _lib.ptr(flat), _lib.ptr(offs), len(arrs), C.byref(fp),
                     _lib.ptr(mel), _lib.ptr(foffs)))
        return [mel[foffs[i]:foffs[i + 1]] for i in range(len(arrs))]

    def stft_mag(self, frames: np.ndarray, precise: bool = True) -> np.ndarray:
        f = np.ascontiguousarray(frames, dtype=np.float32).reshape(-1, 512)
        mag = np.empty((f.shape[0], self.n_bins), np.float32)
        self._chk(self._lib.ww_stft_mag(self.ctx.handle, self._model, _lib.ptr(f), f.shape[0], int(precise), _lib.ptr(mag)))
        return mag

    def filter_apply(self, mag: np.ndarray) -> np.ndarray:
        """``[n, 257]`` STFT magnitudes -> ``[n, 40]`` log-mel (filter.tflite alone)."""
        a = np.ascontiguousarray(mag, dtype=np.float32)
        if a.ndim != 2 or a.shape[1] != self.n_bins:
            raise ValueError(f"Cannot set tensor: Dimension mismatch. Got {a.shape} but expected (n, {self.n_bins})")
        mel = np.empty((a.shape[0], self.n_mel), np.float32)
        self._chk(self._lib.ww_filter_apply(self.ctx.handle, self._model, _lib.ptr(a), a.shape[0], _lib.ptr(mel)))
        return mel

    def detect(self, enc: np.ndarray) -> np.ndarray:
        """Encoder outputs ``[n, enc_rows, enc_width]`` -> detect rows ``[n, n_out]`` (detect.tflite alone)."""
        e = np.ascontiguousarray(enc, dtype=np.float32)
        per = self.enc_shape[0] * self.enc_shape[1]
        if e.size % per != 0 or e.size == 0:
            raise ValueError(f"Cannot set tensor: Dimension mismatch. Got {e.shape} but expected (n,) + {self.enc_shape}")
        n = e.size // per
        out = np.empty((n, self.n_out), np.float32)
        self._chk(self._lib.ww_detect(self.ctx.handle, self._model, _lib.ptr(e), n, _lib.ptr(out)))
        return out

    # ------------------------------------------------------------------ models
    def forward(self, windows: np.ndarray, want_enc: bool = False):
        """``[B, window, 40]`` -> detect rows ``[B, n_out]`` (and encoder output)."""
        w = np.ascontiguousarray(windows, dtype=np.float32)
        if w.ndim == 2:
            w = w[None]
        if w.ndim != 3 or w.shape[1] != self.window or w.shape[2] != self.n_mel:
            raise ValueError(f"Cannot set tensor: Dimension mismatch. Got {tuple(w.shape[1:])} but expected "
                             f"{(self.window, self.n_mel)} per window")
        out = np.empty((w.shape[0], self.n_out), np.float32)
        enc = np.empty((w.shape[0],) + self.enc_shape, np.float32) if want_enc else None
        self._chk(self._lib.ww_forward_enc(self.ctx.handle, self._model, _lib.ptr(w), w.shape[0], _lib.ptr(out), _lib.ptr(enc)))
        return (out, enc) if want_enc else out

    def slide_forward(self, mel: np.ndarray, hop: int = 2) -> np.ndarray:
        m = np.ascontiguousarray(mel, dtype=np.float32)
        if m.ndim != 2 or m.shape[1] != self.n_mel:
            raise ValueError(f"mel must be [rows, {self.n_mel}]")
        rows = m.shape[0]
        nw = (rows - self.window) // hop + 1 if rows >= self.window else 0
        out = np.empty((nw, self.n_out), np.float32)
        got = C.c_int64(0)
        self._chk(self._lib.ww_slide_forward(self.ctx.handle, self._model, _lib.ptr(m), rows, int(hop), _lib.ptr(out), C.byref(got)))
        assert got.value == nw
        return out

    # ------------------------------------------------------------------ CTC-trained CRNNs (include/wwhip.h: ww_ctc_*)
    @property
    def is_ctc(self) -> bool:
        return self.head_kind == _lib.HEAD_CTC

    CTC_STEPS = 19  # rows of posteriors per window: the standard geometry's conv positions
    CTC_OUTPUTS = ("labels", "steps", "enc")

    def _ctc_want(self, want, max_labels: int, allowed) -> None:
        bad = [k for k in want if k not in allowed]
        if bad:
            raise ValueError(f"want takes {allowed}, not {bad}")
        if not 1 <= int(max_labels) <= self.CTC_STEPS:
            raise ValueError(f"max_labels {max_labels} outside 1..{self.CTC_STEPS}")

    def ctc_forward(self, windows: np.ndarray, max_labels: int = 2, want: Sequence[str] = ("labels",)):
        """``[B, window, 40]`` -> :class:`wwhip.ctc.CtcResult`: the greedy-CTC-decoded labels of every window (``labels [B, max_labels]``
        padded with -1, ``lengths [B]`` the whole decoded length), and on request (``want``) the posteriors ``steps [B, 19, n_out]``
        and layer 2's step outputs ``enc [B, 19, 64]`` (``ww_ctc_forward``; wwdetect/CRNN/evaluate.py:100-150)."""
        from .ctc import CtcResult
        self._ctc_want(want, max_labels, self.CTC_OUTPUTS)
        w = np.ascontiguousarray(windows, dtype=np.float32)
        if w.ndim == 2:
            w = w[None]
        if w.ndim != 3 or w.shape[1] != self.window or w.shape[2] != self.n_mel:
            raise ValueError(f"Cannot set tensor: Dimension mismatch. Got {tuple(w.shape[1:])} but expected "
                             f"{(self.window, self.n_mel)} per window")
        n = w.shape[0]
        labels, lengths = np.full((n, int(max_labels)), -1, np.int32), np.zeros(n, np.int32)
        steps = np.empty((n, self.CTC_STEPS, self.n_out), np.float32) if "steps" in want else None
        enc = np.empty((n, self.CTC_STEPS, self.enc_shape[1]), np.float32) if "enc" in want else None
        self._chk(self._lib.ww_ctc_forward(self.ctx.handle, self._model, _lib.ptr(w), n, int(max_labels), _lib.ptr(labels), _lib.ptr(lengths),
                                           _lib.ptr(steps), _lib.ptr(enc)))
        return CtcResult(labels, lengths, steps, enc)

    def ctc_slide_forward(self, mel: np.ndarray, hop: int = 2, max_labels: int = 2, want: Sequence[str] = ("labels",)):
        """Windows sliding over one ``[rows, 40]`` sequence (``ww_ctc_slide_forward``); ``want``: ``"labels"``, ``"steps"``."""
        from .ctc import CtcResult
        self._ctc_want(want, max_labels, ("labels", "steps"))
        m = np.ascontiguousarray(mel, dtype=np.float32)
        if m.ndim != 2 or m.shape[1] != self.n_mel:
            raise ValueError(f"mel must be [rows, {self.n_mel}]")
        if hop < 1:
            raise ValueError("hop must be positive")
        rows = m.shape[0]
        nw = (rows - self.window) // hop + 1 if rows >= self.window else 0
        labels, lengths = np.full((nw, int(max_labels)), -1, np.int32), np.zeros(nw, np.int32)
        steps = np.empty((nw, self.CTC_STEPS, self.n_out), np.float32) if "steps" in want else None
        got = C.c_int64(0)
        self._chk(self._lib.ww_ctc_slide_forward(self.ctx.handle, self._model, _lib.ptr(m), rows, int(hop), int(max_labels), _lib.ptr(labels),
                                                 _lib.ptr(lengths), _lib.ptr(steps), C.byref(got)))
        assert got.value == nw
        return CtcResult(labels, lengths, steps, None)

    def ctc_forward_windows_dev(self, d_mel_ptr: int, mel_rows: int, d_win_row_ptr: int, d_win_valid_ptr: int, n_windows: int,
                                max_labels: int, d_labels_ptr: int, d_lengths_ptr: int, d_steps_ptr: int = 0, d_enc_ptr: int = 0) -> None:
        """``ww_ctc_forward_windows_dev`` on device addresses (enqueued on the context's stream; 0 = no such output)."""
        self._chk(self._lib.ww_ctc_forward_windows_dev(self.ctx.handle, self._model, _vp(d_mel_ptr), int(mel_rows), _vp(d_win_row_ptr),
                                                       _vp(d_win_valid_ptr), int(n_windows), int(max_labels), _vp(d_labels_ptr),
                                                       _vp(d_lengths_ptr), _vp(d_steps_ptr), _vp(d_enc_ptr)))

    def ctc_greedy_dev(self, d_steps_ptr: int, n: int, T: int, L: int, max_labels: int, d_labels_ptr: int, d_lengths_ptr: int) -> None:
        """``ww_ctc_greedy_dev``: the decode alone on device posteriors ``[n, T, L]`` (any model; the context is this engine's)."""
        self._chk(self._lib.ww_ctc_greedy_dev(self.ctx.handle, _vp(d_steps_ptr), int(n), int(T), int(L), int(max_labels), _vp(d_labels_ptr),
                                              _vp(d_lengths_ptr)))

    # the forward-algorithm score (include/wwhip.h: ww_ctc_score_*; wwhip.ctc.score is its float64 statement)
    def _ctc_score_args(self, targets, mode, L: int):
        from . import ctc
        table, lens = ctc.pack_targets(targets, L)
        return table, lens, len(lens), ctc.score_mode(mode)

    def ctc_score(self, windows: np.ndarray, targets=((1, 2),), mode="exact", max_labels: int = 0):
        """``[B, window, 40]`` -> ``scores [K, B]`` float32: per target (a tuple of labels; ``[HEY][SNIPS]`` by default) and window the
        probability that the window's decode is (``mode="exact"``, the CTC loss's quantity) or starts with (``"prefix"``) the target,
        from the posteriors :meth:`ctc_forward` returns as ``steps`` (``ww_ctc_score``).  Plane ``k`` is a posterior track for
        :func:`wwhip.evaluate.far_frr` and the event calls.  With ``max_labels > 0`` the greedy decode comes with it:
        ``(scores, CtcResult(labels, lengths))``."""
        from .ctc import CtcResult
        table, lens, K, md = self._ctc_score_args(targets, mode, self.n_out)
        w = np.ascontiguousarray(windows, dtype=np.float32)
        if w.ndim == 2:
            w = w[None]
        if w.ndim != 3 or w.shape[1] != self.window or w.shape[2] != self.n_mel:
            raise ValueError(f"Cannot set tensor: Dimension mismatch. Got {tuple(w.shape[1:])} but expected "
                             f"{(self.window, self.n_mel)} per window")
        n, m = w.shape[0], int(max_labels)
        scores = np.empty((K, n), np.float32)
        labels, lengths = (np.full((n, m), -1, np.int32), np.zeros(n, np.int32)) if m else (None, None)
        self._chk(self._lib.ww_ctc_score(self.ctx.handle, self._model, _lib.ptr(w), n, _lib.ptr(table), _lib.ptr(lens), K, md, _lib.ptr(scores),
                                         m, _lib.ptr(labels), _lib.ptr(lengths)))
        return (scores, CtcResult(labels, lengths)) if m else scores

    def ctc_slide_score(self, mel: np.ndarray, hop: int = 2, targets=((1, 2),), mode="exact", max_labels: int = 0):
        """:meth:`ctc_score` of the windows sliding over one ``[rows, 40]`` sequence (``ww_ctc_slide_score``): ``scores [K, n_windows]``."""
        from .ctc import CtcResult
        table, lens, K, md = self._ctc_score_args(targets, mode, self.n_out)
        mm = np.ascontiguousarray(mel, dtype=np.float32)
        if mm.ndim != 2 or mm.shape[1] != self.n_mel:
            raise ValueError(f"mel must be [rows, {self.n_mel}]")
        if hop < 1:
            raise ValueError("hop must be positive")
        rows, m = mm.shape[0], int(max_labels)
        nw = (rows - self.window) // hop + 1 if rows >= self.window else 0
        scores = np.empty((K, nw), np.float32)
        labels, lengths = (np.full((nw, m), -1, np.int32), np.zeros(nw, np.int32)) if m else (None, None)
        got = C.c_int64(0)
        self._chk(self._lib.ww_ctc_slide_score(self.ctx.handle, self._model, _lib.ptr(mm), rows, int(hop), _lib.ptr(table), _lib.ptr(lens), K, md,
                                               _lib.ptr(scores), m, _lib.ptr(labels), _lib.ptr(lengths), C.byref(got)))
        assert got.value == nw
        return (scores, CtcResult(labels, lengths)) if m else scores

    def ctc_score_windows_dev(self, d_mel_ptr: int, mel_rows: int, d_win_row_ptr: int, d_win_valid_ptr: int, n_windows: int, targets, mode,
                              d_score_ptr: int, max_labels: int = 0, d_labels_ptr: int = 0, d_lengths_ptr: int = 0) -> None:
        """``ww_ctc_score_windows_dev`` on device addresses: ``d_score [K, n_windows]`` (enqueued on the context's stream)."""
        table, lens, K, md = self._ctc_score_args(targets, mode, self.n_out)
        self._chk(self._lib.ww_ctc_score_windows_dev(self.ctx.handle, self._model, _vp(d_mel_ptr), int(mel_rows), _vp(d_win_row_ptr),
                                                     _vp(d_win_valid_ptr), int(n_windows), _lib.ptr(table), _lib.ptr(lens), K, md,
                                                     _vp(d_score_ptr), int(max_labels), _vp(d_labels_ptr), _vp(d_lengths_ptr)))

    def ctc_score_dev(self, d_steps_ptr: int, n: int, T: int, L: int, targets, mode, d_score_ptr: int) -> None:
        """``ww_ctc_score_dev``: the score kernel alone on device posteriors ``[n, T, L]`` -> ``d_score [K, n]`` (any model; the
        context is this engine's)."""
        table, lens, K, md = self._ctc_score_args(targets, mode, int(L))
        self._chk(self._lib.ww_ctc_score_dev(self.ctx.handle, _vp(d_steps_ptr), int(n), int(T), int(L), _lib.ptr(table), _lib.ptr(lens), K, md,
                                             _vp(d_score_ptr)))

    # the Viterbi alignment (include/wwhip.h: ww_ctc_align_*; wwhip.ctc.align is its float64 statement)
    @staticmethod
    def _ctc_alignment(value, span, lens):
        from .ctc import CtcAlignment
        return CtcAlignment(value, span[:, :, :int(lens.max())].astype(np.int32))

    def ctc_align(self, windows: np.ndarray, targets=((1, 2),), mode="exact", max_labels: int = 0):
        """``[B, window, 40]`` -> :class:`~wwhip.ctc.CtcAlignment` ``(value [K, B] float32, span [K, B, U_max, 2] int32)``: per target
        and window the most probable path that reads (``mode="exact"``) or completes (``"prefix"``) the target, from the posteriors
        :meth:`ctc_forward` returns as ``steps`` - its probability, and the first and last conv step it spends on each label
        (``ww_ctc_align``; ``wwhip.ctc.span_rows`` / ``span_seconds`` turn steps into mel rows and time).  With ``max_labels > 0``
        the greedy decode comes with it: ``(alignment, CtcResult(labels, lengths))``."""
        from .ctc import CtcResult
        table, lens, K, md = self._ctc_score_args(targets, mode, self.n_out)
        w = np.ascontiguousarray(windows, dtype=np.float32)
        if w.ndim == 2:
            w = w[None]
        if w.ndim != 3 or w.shape[1] != self.window or w.shape[2] != self.n_mel:
            raise ValueError(f"Cannot set tensor: Dimension mismatch. Got {tuple(w.shape[1:])} but expected "
                             f"{(self.window, self.n_mel)} per window")
        n, m = w.shape[0], int(max_labels)
        value, span = np.empty((K, n), np.float32), np.empty((K, n, _lib.CTC_SCORE_MAX_TARGET, 2), np.int8)
        labels, lengths = (np.full((n, m), -1, np.int32), np.zeros(n, np.int32)) if m else (None, None)
        self._chk(self._lib.ww_ctc_align(self.ctx.handle, self._model, _lib.ptr(w), n, _lib.ptr(table), _lib.ptr(lens), K, md, _lib.ptr(value),
                                         _lib.ptr(span), m, _lib.ptr(labels), _lib.ptr(lengths)))
        al = self._ctc_alignment(value, span, lens)
        return (al, CtcResult(labels, lengths)) if m else al

    def ctc_slide_align(self, mel: np.ndarray, hop: int = 2, targets=((1, 2),), mode="exact", max_labels: int = 0):
        """:meth:`ctc_align` of the windows sliding over one ``[rows, 40]`` sequence (``ww_ctc_slide_align``): window ``i`` starts at
        row ``i * hop`` (``wwhip.ctc.span_rows(al.span, np.arange(n) * hop)`` places the spans on the sequence)."""
        from .ctc import CtcResult
        table, lens, K, md = self._ctc_score_args(targets, mode, self.n_out)
        mm = np.ascontiguousarray(mel, dtype=np.float32)
        if mm.ndim != 2 or mm.shape[1] != self.n_mel:
            raise ValueError(f"mel must be [rows, {self.n_mel}]")
        if hop < 1:
            raise ValueError("hop must be positive")
        rows, m = mm.shape[0], int(max_labels)
        nw = (rows - self.window) // hop + 1 if rows >= self.window else 0
        value, span = np.empty((K, nw), np.float32), np.empty((K, nw, _lib.CTC_SCORE_MAX_TARGET, 2), np.int8)
        labels, lengths = (np.full((nw, m), -1, np.int32), np.zeros(nw, np.int32)) if m else (None, None)
        got = C.c_int64(0)
        self._chk(self._lib.ww_ctc_slide_align(self.ctx.handle, self._model, _lib.ptr(mm), rows, int(hop), _lib.ptr(table), _lib.ptr(lens), K, md,
                                               _lib.ptr(value), _lib.ptr(span), m, _lib.ptr(labels), _lib.ptr(lengths), C.byref(got)))
        assert got.value == nw
        al = self._ctc_alignment(value, span, lens)
        return (al, CtcResult(labels, lengths)) if m else al

    def ctc_align_windows_dev(self, d_mel_ptr: int, mel_rows: int, d_win_row_ptr: int, d_win_valid_ptr: int, n_windows: int, targets, mode,
                              d_value_ptr: int, d_span_ptr: int, max_labels: int = 0, d_labels_ptr: int = 0, d_lengths_ptr: int = 0) -> None:
        """``ww_ctc_align_windows_dev`` on device addresses: ``d_value [K, n_windows]`` float32 and ``d_span [K, n_windows, 9, 2]`` int8
        (enqueued on the context's stream)."""
        table, lens, K, md = self._ctc_score_args(targets, mode, self.n_out)
        self._chk(self._lib.ww_ctc_align_windows_dev(self.ctx.handle, self._model, _vp(d_mel_ptr), int(mel_rows), _vp(d_win_row_ptr),
                                                     _vp(d_win_valid_ptr), int(n_windows), _lib.ptr(table), _lib.ptr(lens), K, md,
                                                     _vp(d_value_ptr), _vp(d_span_ptr), int(max_labels), _vp(d_labels_ptr), _vp(d_lengths_ptr)))

    def ctc_align_dev(self, d_steps_ptr: int, n: int, T: int, L: int, targets, mode, d_value_ptr: int, d_span_ptr: int) -> None:
        """``ww_ctc_align_dev``: the align kernel alone on device posteriors ``[n, T, L]`` -> ``d_value [K, n]`` float32 and
        ``d_span [K, n, 9, 2]`` int8 (any model; the context is this engine's)."""
        table, lens, K, md = self._ctc_score_args(targets, mode, int(L))
        self._chk(self._lib.ww_ctc_align_dev(self.ctx.handle, _vp(d_steps_ptr), int(n), int(T), int(L), _lib.ptr(table), _lib.ptr(lens), K, md,
                                             _vp(d_value_ptr), _vp(d_span_ptr)))

    # the forward-backward occupancy (include/wwhip.h: ww_ctc_occupancy_*; wwhip.ctc.occupancy is its float64 statement)
    def _ctc_occupancy_out(self, K: int, n: int, want_classes: bool):
        value, occ = np.empty((K, n), np.float32), np.empty((K, n, self.CTC_STEPS, _lib.CTC_SCORE_MAX_TARGET), np.float32)
        return value, occ, (np.empty((K, n, self.CTC_STEPS, self.n_out), np.float32) if want_classes else None)

    def ctc_occupancy(self, windows: np.ndarray, targets=((1, 2),), mode="exact", want_classes: bool = False, max_labels: int = 0):
        """``[B, window, 40]`` -> :class:`~wwhip.ctc.CtcOccupancy` ``(value [K, B], occ [K, B, 19, 9], cls [K, B, 19, n_out] | None)``:
        per target and window, over ALL the paths that read (``mode="exact"``) or complete (``"prefix"``) the target, the share of
        each conv step that each label holds - the soft counterpart of :meth:`ctc_align`'s span; in prefix mode the last label's
        column is the distribution of the completion step (``ww_ctc_occupancy``).  ``value`` carries :meth:`ctc_score`'s bits.
        ``want_classes`` (exact mode only) adds the per-class shares, whose difference from the posteriors is the CTC loss's
        gradient (``CtcOccupancy.grad``).  With ``max_labels > 0`` the greedy decode comes with it:
        ``(occupancy, CtcResult(labels, lengths))``."""
        from .ctc import CtcOccupancy, CtcResult
        table, lens, K, md = self._ctc_score_args(targets, mode, self.n_out)
        w = np.ascontiguousarray(windows, dtype=np.float32)
        if w.ndim == 2:
            w = w[None]
        if w.ndim != 3 or w.shape[1] != self.window or w.shape[2] != self.n_mel:
            raise ValueError(f"Cannot set tensor: Dimension mismatch. Got {tuple(w.shape[1:])} but expected "
                             f"{(self.window, self.n_mel)} per window")
        n, m = w.shape[0], int(max_labels)
        value, occ, cls = self._ctc_occupancy_out(K, n, want_classes)
        labels, lengths = (np.full((n, m), -1, np.int32), np.zeros(n, np.int32)) if m else (None, None)
        self._chk(self._lib.ww_ctc_occupancy(self.ctx.handle, self._model, _lib.ptr(w), n, _lib.ptr(table), _lib.ptr(lens), K, md, _lib.ptr(value),
                                             _lib.ptr(occ), _lib.ptr(cls), m, _lib.ptr(labels), _lib.ptr(lengths)))
        oc = CtcOccupancy(value, occ, cls)
        return (oc, CtcResult(labels, lengths)) if m else oc

    def ctc_slide_occupancy(self, mel: np.ndarray, hop: int = 2, targets=((1, 2),), mode="exact", want_classes: bool = False, max_labels: int = 0):
        """:meth:`ctc_occupancy` of the windows sliding over one ``[rows, 40]`` sequence (``ww_ctc_slide_occupancy``): window ``i``
        starts at row ``i * hop``."""
        from .ctc import CtcOccupancy, CtcResult
        table, lens, K, md = self._ctc_score_args(targets, mode, self.n_out)
        mm = np.ascontiguousarray(mel, dtype=np.float32)
        if mm.ndim != 2 or mm.shape[1] != self.n_mel:
            raise ValueError(f"mel must be [rows, {self.n_mel}]")
        if hop < 1:
            raise ValueError("hop must be positive")
        rows, m = mm.shape[0], int(max_labels)
        nw = (rows - self.window) // hop + 1 if rows >= self.window else 0
        value, occ, cls = self._ctc_occupancy_out(K, nw, want_classes)
        labels, lengths = (np.full((nw, m), -1, np.int32), np.zeros(nw, np.int32)) if m else (None, None)
        got = C.c_int64(0)
        self._chk(self._lib.ww_ctc_slide_occupancy(self.ctx.handle, self._model, _lib.ptr(mm), rows, int(hop), _lib.ptr(table), _lib.ptr(lens), K, md,
                                                   _lib.ptr(value), _lib.ptr(occ), _lib.ptr(cls), m, _lib.ptr(labels), _lib.ptr(lengths),
                                                   C.byref(got)))
        assert got.value == nw
        oc = CtcOccupancy(value, occ, cls)
        return (oc, CtcResult(labels, lengths)) if m else oc

    def ctc_occupancy_windows_dev(self, d_mel_ptr: int, mel_rows: int, d_win_row_ptr: int, d_win_valid_ptr: int, n_windows: int, targets, mode,
                                  d_value_ptr: int, d_occ_ptr: int, d_cls_ptr: int = 0, max_labels: int = 0, d_labels_ptr: int = 0,
                                  d_lengths_ptr: int = 0) -> None:
        """``ww_ctc_occupancy_windows_dev`` on device addresses: ``d_value [K, n_windows]``, ``d_occ [K, n_windows, 19, 9]`` and (0 = none)
        ``d_cls [K, n_windows, 19, n_out]`` float32 (enqueued on the context's stream)."""
        table, lens, K, md = self._ctc_score_args(targets, mode, self.n_out)
        self._chk(self._lib.ww_ctc_occupancy_windows_dev(self.ctx.handle, self._model, _vp(d_mel_ptr), int(mel_rows), _vp(d_win_row_ptr),
                                                         _vp(d_win_valid_ptr), int(n_windows), _lib.ptr(table), _lib.ptr(lens), K, md,
                                                         _vp(d_value_ptr), _vp(d_occ_ptr), _vp(d_cls_ptr), int(max_labels), _vp(d_labels_ptr),
                                                         _vp(d_lengths_ptr)))

    def ctc_occupancy_dev(self, d_steps_ptr: int, n: int, T: int, L: int, targets, mode, d_value_ptr: int, d_occ_ptr: int, d_cls_ptr: int = 0) -> None:
        """``ww_ctc_occupancy_dev``: the occupancy kernel alone on device posteriors ``[n, T, L]`` -> ``d_value [K, n]``,
        ``d_occ [K, n, T, 9]`` and (0 = none) ``d_cls [K, n, T, L]`` float32 (any model; the context is this engine's)."""
        table, lens, K, md = self._ctc_score_args(targets, mode, int(L))
        self._chk(self._lib.ww_ctc_occupancy_dev(self.ctx.handle, _vp(d_steps_ptr), int(n), int(T), int(L), _lib.ptr(table), _lib.ptr(lens), K, md,
                                                 _vp(d_value_ptr), _vp(d_occ_ptr), _vp(d_cls_ptr)))

    # the prefix beam search (include/wwhip.h: ww_ctc_beam_*; wwhip.ctc.beam_search is its float64 statement)
    def _ctc_beam_out(self, n: int, beam_width: int, top_paths: int, max_labels):
        W, P = int(beam_width), int(top_paths)
        M = self.CTC_STEPS if max_labels is None else int(max_labels)
        # (shapes only: the library names the rule a bad argument breaks)
        return W, P, M, (np.full((n, max(P, 1), max(M, 1)), -1, np.int32), np.full((n, max(P, 1)), -1, np.int32), np.zeros((n, max(P, 1)), np.float32))

    def ctc_beam(self, windows: np.ndarray, beam_width: int, top_paths: int = 1, max_labels: Optional[int] = None):
        """``[B, window, 40]`` -> :class:`~wwhip.ctc.CtcBeam` ``(labels [B, P, max_labels], lengths [B, P], probs [B, P])``: the
        ``top_paths`` most probable label strings of every window and their probabilities, by prefix beam search of width
        ``beam_width`` over the posteriors :meth:`ctc_forward` returns as ``steps`` (``ww_ctc_beam``; ``K.ctc_decode(greedy=False)``'s
        question, the statement in ``csrc/ctc_beam.h``).  An absent path has length -1 and probability 0."""
        from .ctc import CtcBeam
        w = np.ascontiguousarray(windows, dtype=np.float32)
        if w.ndim == 2:
            w = w[None]
        if w.ndim != 3 or w.shape[1] != self.window or w.shape[2] != self.n_mel:
            raise ValueError(f"Cannot set tensor: Dimension mismatch. Got {tuple(w.shape[1:])} but expected "
                             f"{(self.window, self.n_mel)} per window")
        n = w.shape[0]
        W, P, M, (labels, lengths, probs) = self._ctc_beam_out(n, beam_width, top_paths, max_labels)
        self._chk(self._lib.ww_ctc_beam(self.ctx.handle, self._model, _lib.ptr(w), n, W, P, M, _lib.ptr(labels), _lib.ptr(lengths), _lib.ptr(probs)))
        return CtcBeam(labels, lengths, probs)

    def ctc_slide_beam(self, mel: np.ndarray, hop: int = 2, beam_width: int = 8, top_paths: int = 1, max_labels: Optional[int] = None):
        """:meth:`ctc_beam` of the windows sliding over one ``[rows, 40]`` sequence (``ww_ctc_slide_beam``)."""
        from .ctc import CtcBeam
        mm = np.ascontiguousarray(mel, dtype=np.float32)
        if mm.ndim != 2 or mm.shape[1] != self.n_mel:
            raise ValueError(f"mel must be [rows, {self.n_mel}]")
        if hop < 1:
            raise ValueError("hop must be positive")
        rows = mm.shape[0]
        nw = (rows - self.window) // hop + 1 if rows >= self.window else 0
        W, P, M, (labels, lengths, probs) = self._ctc_beam_out(nw, beam_width, top_paths, max_labels)
        got = C.c_int64(0)
        self._chk(self._lib.ww_ctc_slide_beam(self.ctx.handle, self._model, _lib.ptr(mm), rows, int(hop), W, P, M, _lib.ptr(labels), _lib.ptr(lengths),
                                              _lib.ptr(probs), C.byref(got)))
        assert got.value == nw
        return CtcBeam(labels, lengths, probs)

    def ctc_beam_windows_dev(self, d_mel_ptr: int, mel_rows: int, d_win_row_ptr: int, d_win_valid_ptr: int, n_windows: int, beam_width: int,
                             top_paths: int, max_labels: int, d_labels_ptr: int, d_lengths_ptr: int, d_prob_ptr: int) -> None:
        """``ww_ctc_beam_windows_dev`` on device addresses: ``d_labels [n_windows, P, max_labels]`` int32, ``d_lengths`` and ``d_prob``
        ``[n_windows, P]`` (enqueued on the context's stream)."""
        self._chk(self._lib.ww_ctc_beam_windows_dev(self.ctx.handle, self._model, _vp(d_mel_ptr), int(mel_rows), _vp(d_win_row_ptr),
                                                    _vp(d_win_valid_ptr), int(n_windows), int(beam_width), int(top_paths), int(max_labels),
                                                    _vp(d_labels_ptr), _vp(d_lengths_ptr), _vp(d_prob_ptr)))

    def ctc_beam_dev(self, d_steps_ptr: int, n: int, T: int, L: int, beam_width: int, top_paths: int, max_labels: int, d_labels_ptr: int,
                     d_lengths_ptr: int, d_prob_ptr: int) -> None:
        """``ww_ctc_beam_dev``: the beam kernel alone on device posteriors ``[n, T, L]`` (any model; the context is this engine's)."""
        self._chk(self._lib.ww_ctc_beam_dev(self.ctx.handle, _vp(d_steps_ptr), int(n), int(T), int(L), int(beam_width), int(top_paths),
                                            int(max_labels), _vp(d_labels_ptr), _vp(d_lengths_ptr), _vp(d_prob_ptr)))

    SEQUENCE_OUTPUTS = ("enc", "logits", "post_frames", "post")

    def sequence_forward(self, mels, pool: Optional[int] = None, want: Sequence[str] = ("post",)) -> dict:
        """The fp32 Wavenet on whole mel sequences of any length (``ww_wave_sequence``): the reference's model with
        ``timesteps=None`` - causal taps read zeros in front of row 0, nothing else is padded.  This is NOT the TFLite window form
        of :meth:`forward` / :meth:`slide_forward`, whose windows each pad their own left edge; for a sequence of exactly
        ``window`` rows the two coincide, bit for bit.

        ``mels``: a list of ``[L_i, n_mel]`` arrays (or one such array).  ``want``: any of ``"enc"`` (``[L_i, 32]`` skip sums),
        ``"logits"`` (``[L_i, n_out]``, the head before the max over time), ``"post_frames"`` (``[L_i, n_out]``: softmax of the
        maximum over the last ``pool`` rows; ``pool=None``: the model's window, ``0``: from row 0) and ``"post"`` (``[n_out]``:
        softmax of the maximum over the whole sequence).  Returns ``{name: list of arrays, one per sequence}``; an empty
        sequence's ``post`` is NaN."""
        want, seqs, offs, mel = _sequence_batch(mels, self.n_mel, want)
        total = int(offs[-1])
        pool = self.window if pool is None else int(pool)
        bufs = _sequence_buffers(self.n_out, self.enc_shape[1], want, None, total, len(seqs))
        self._chk(self._lib.ww_wave_sequence(self.ctx.handle, self._model, _lib.ptr(mel), total, _lib.ptr(offs), len(seqs), pool,
                                             _lib.ptr(bufs["enc"]), _lib.ptr(bufs["logits"]), _lib.ptr(bufs["post_frames"]),
                                             _lib.ptr(bufs["post"])))
        return _per_sequence(bufs, want, offs)

    def wave_sequence_dev(self, d_mel_ptr: int, total_rows: int, row_offs: np.ndarray, pool: Optional[int] = None, d_enc_ptr: int = 0,
                          d_logits_ptr: int = 0, d_post_frames_ptr: int = 0, d_post_ptr: int = 0) -> None:
        """:meth:`sequence_forward` on device buffers (``ww_wave_sequence_dev``): sequence ``s`` is rows ``[row_offs[s],
        row_offs[s + 1])`` of the mel buffer (``row_offs``: a host array); the per-row outputs are indexed by mel row, ``post`` by
        sequence; a pointer of 0 leaves that output out.  Enqueued on the context's stream, not waited for."""
        offs = _row_offs(row_offs)
        self._chk(self._lib.ww_wave_sequence_dev(self.ctx.handle, self._model, _vp(d_mel_ptr), int(total_rows), _lib.ptr(offs), int(offs.size - 1),
                                                 self.window if pool is None else int(pool), _vp(d_enc_ptr), _vp(d_logits_ptr),
                                                 _vp(d_post_frames_ptr), _vp(d_post_ptr)))

    # ------------------------------------------------------------------ evaluator
    def far_frr(self, pos: np.ndarray, neg: np.ndarray, thresholds: np.ndarray, num_wakewords: float, hours: float,
                window: int = 30, want_smoothed: bool = False):
        pos = np.ascontiguousarray(pos, dtype=np.float32).ravel()
        neg = np.ascontiguousarray(neg, dtype=np.float32).ravel()
        thr = np.ascontiguousarray(thresholds, dtype=np.float64).ravel()
        frr = np.empty(thr.size, np.float64)
        fa = np.empty(thr.size, np.float64)
        cnt = np.empty(thr.size, np.int64)
        sm = np.empty(neg.size, np.float64) if want_smoothed else None
        self._chk(self._lib.ww_far_frr(self.ctx.handle, _lib.ptr(pos), pos.size, _lib.ptr(neg), neg.size, int(window),
                                       _lib.ptr(thr), thr.size, float(num_wakewords), float(hours), _lib.ptr(frr),
                                       _lib.ptr(fa), _lib.ptr(cnt), _lib.ptr(sm)))
        return (frr, fa, cnt, sm) if want_smoothed else (frr, fa, cnt)

    def far_frr_dev(self, d_pos_ptr: int, n_pos: int, d_neg_ptr: int, n_neg: int, thresholds: np.ndarray, num_wakewords: float,
                    hours: float, window: int = 30):
        """:meth:`far_frr` over posteriors that are already on the device (``ww_far_frr_dev``): only the counters come back."""
        thr = np.ascontiguousarray(thresholds, dtype=np.float64).ravel()
        frr, fa, cnt = np.empty(thr.size, np.float64), np.empty(thr.size, np.float64), np.empty(thr.size, np.int64)
        self._chk(self._lib.ww_far_frr_dev(self.ctx.handle, C.c_void_p(d_pos_ptr), int(n_pos), C.c_void_p(d_neg_ptr), int(n_neg),
                                           int(window), _lib.ptr(thr), thr.size, float(num_wakewords), float(hours), _lib.ptr(frr),
                                           _lib.ptr(fa), _lib.ptr(cnt), None))
        return frr, fa, cnt

    def posterior_pick_dev(self, d_rows_ptr: int, n: int, d_out_ptr: int, d_seg_offs_ptr: int = 0, n_seg: int = 0) -> None:
        """Element ``posterior_index`` of ``n`` detect rows on the device -> ``d_out``: one value per row, or - with a device
        table of ``n_seg + 1`` row offsets - the maximum of each run (``ww_posterior_pick_dev``).  Enqueued, not waited for."""
        self._chk(self._lib.ww_posterior_pick_dev(self.ctx.handle, C.c_void_p(d_rows_ptr), int(n), self.n_out, self.posterior_index,
                                                  C.c_void_p(d_seg_offs_ptr) if d_seg_offs_ptr else None, int(n_seg),
                                                  C.c_void_p(d_out_ptr)))

    def posterior_events(self, post, threshold, seg_offs=None, window: int = 30, cap: Optional[int] = None, want_counts: bool = False):
        """Where the smoothed posterior is above the threshold (``ww_posterior_events``, include/wwhip.h states the rule): ``post`` is
        1-D or ``[planes, n]`` float32, ``threshold`` one value or one per plane, ``seg_offs`` ``n_seg + 1`` ascending row offsets
        (``None``: one segment; smoothing and runs never cross a boundary).  Returns the events as an array of
        ``wwhip._lib.EVENT_DTYPE`` (``plane, seg, start, end, peak, peak_value``; rows relative to the segment) in plane, segment, start
        order; with ``want_counts`` also the totals per plane and overall.  ``cap`` limits how many are returned."""
        return _events_host(self.ctx, post, threshold, seg_offs, window, cap, want_counts)

    def posterior_events_dev(self, d_post_ptr: int, n: int, threshold, seg_offs=None, window: int = 30, planes: int = 1,
                             cap: Optional[int] = None, want_counts: bool = False):
        """:meth:`posterior_events` over ``[planes, n]`` float32 posteriors that are already on the device
        (``ww_posterior_events_dev``): offsets and thresholds go up, only the events come back."""
        return _events_dev(self.ctx, d_post_ptr, n, planes, threshold, seg_offs, window, cap, want_counts)

    # ------------------------------------------------------------------ device-resident paths (torch plumbing)
    def clips_forward_dev(self, d_pcm_ptr: int, n_clips: int, samples_per_clip: int, d_out_ptr: int,
                          fp: Optional[_lib.FrontendParams] = None) -> None:
        fp = fp or frontend_params()
        self._chk(self._lib.ww_clips_forward_dev(self.ctx.handle, self._model, C.c_void_p(d_pcm_ptr), int(n_clips),
                                                 int(samples_per_clip), C.byref(fp), C.c_void_p(d_out_ptr)))

    def logmel_dev(self, d_pcm_ptr: int, d_sample_offs_ptr: int, d_frame_offs_ptr: int, n_utt: int, total_frames: int,
                   max_frames: int, d_mel_ptr: int, fp: Optional[_lib.FrontendParams] = None) -> None:
        fp = fp or frontend_params()
        self._chk(self._lib.ww_logmel_dev(self.ctx.handle, self._model, C.c_void_p(d_pcm_ptr), C.c_void_p(d_sample_offs_ptr),
                                          C.c_void_p(d_frame_offs_ptr), int(n_utt), int(total_frames), int(max_frames),
                                          C.byref(fp), C.c_void_p(d_mel_ptr)))

    def forward_windows_dev(self, d_mel_ptr: int, mel_rows: int, d_win_row_ptr: int, d_win_valid_ptr: int,
                            n_windows: int, d_out_ptr: int) -> None:
        self._chk(self._lib.ww_forward_windows_dev(self.ctx.handle, self._model, C.c_void_p(d_mel_ptr), int(mel_rows),
                                                   C.c_void_p(d_win_row_ptr), C.c_void_p(d_win_valid_ptr), int(n_windows),
                                                   C.c_void_p(d_out_ptr)))

    def forward_segments_dev(self, d_mel_ptr: int, mel_rows: int, seg_row0: np.ndarray, seg_nw: np.ndarray, hop: int,
                             d_out_ptr: int) -> None:
        """Several mel sequences in one device buffer, each slid over with ``hop`` (``ww_forward_segments_dev``): sequence
        ``s`` has ``seg_nw[s]`` complete windows starting at row ``seg_row0[s]``; detect rows go to ``d_out`` sequence by
        sequence.  The descriptor arrays are host arrays."""
        r0 = np.ascontiguousarray(seg_row0, dtype=np.int64)
        nw = np.ascontiguousarray(seg_nw, dtype=np.int32)
        if r0.shape != nw.shape or r0.ndim != 1:
            raise ValueError("seg_row0 and seg_nw must be 1-D arrays of the same length")
        self._chk(self._lib.ww_forward_segments_dev(self.ctx.handle, self._model, C.c_void_p(d_mel_ptr), int(mel_rows),
                                                    _lib.ptr(r0), _lib.ptr(nw), int(r0.size), int(hop), C.c_void_p(d_out_ptr)))


def _sequence_batch(mels, n_mel: int, want):
    """The arguments of a ``sequence_forward`` call, checked: ``(want, sequences, row offsets, the sequences back to back)``."""
    if isinstance(mels, np.ndarray) and mels.ndim == 2:
        mels = [mels]
    want = tuple(want)
    bad = [k for k in want if k not in Engine.SEQUENCE_OUTPUTS]
    if bad:
        raise ValueError(f"want must be drawn from {Engine.SEQUENCE_OUTPUTS}, got {bad}")
    seqs = [np.ascontiguousarray(m, dtype=np.float32).reshape(-1, n_mel) if np.size(m) == 0 else np.ascontiguousarray(m, dtype=np.float32)
            for m in mels]
    for m in seqs:
        if m.ndim != 2 or m.shape[1] != n_mel:
            raise ValueError(f"every sequence must be [rows, {n_mel}]")
    offs = np.zeros(len(seqs) + 1, np.int64)
    np.cumsum([m.shape[0] for m in seqs], out=offs[1:])
    mel = np.concatenate(seqs) if seqs else np.zeros((0, n_mel), np.float32)
    return want, seqs, offs, mel


def _sequence_buffers(n_out: int, enc_width: int, want, planes: Optional[int], total: int, n_seq: int) -> dict:
    """Host outputs of a sequence call (``planes=None``: the one plane of a single model or of the by-sequence form); ``post``
    starts as NaN."""
    lead = () if planes is None else (planes,)
    shapes = {"enc": (total, enc_width), "logits": (total, n_out), "post_frames": (total, n_out), "post": (n_seq, n_out)}
    return {k: (np.full(lead + shapes[k], np.nan, np.float32) if k == "post" else np.empty(lead + shapes[k], np.float32)) if k in want
            else None for k in Engine.SEQUENCE_OUTPUTS}


def _per_sequence(bufs: dict, want, offs: np.ndarray) -> dict:
    """One plane's buffers as ``{name: list of arrays, one per sequence}``."""
    n = offs.size - 1
    return {k: [bufs[k][i] for i in range(n)] if k == "post" else [bufs[k][offs[i]:offs[i + 1]] for i in range(n)] for k in want}


def _row_offs(row_offs) -> np.ndarray:
    offs = np.ascontiguousarray(row_offs, dtype=np.int64)
    if offs.ndim != 1 or offs.size < 1:
        raise ValueError("row_offs must be a 1-D array of n_seq + 1 offsets")
    return offs


def _vp(p: int):
    """A device address as a ``void *`` argument; 0 is NULL."""
    return C.c_void_p(p) if p else None


def _member_ids(ids, n: int, n_models: int, what: str) -> np.ndarray:
    """``ids`` as the int32 table the library takes: ``n`` entries, each a member of a set of ``n_models`` (``ValueError`` otherwise:
    the library would refuse them too - ``WW_EINVAL`` - but a list of the wrong length it cannot see)."""
    a = np.asarray(ids)
    if a.ndim != 1 or a.size != n:
        per = {"models": "stream", "seq_model": "sequence"}.get(what, "window")
        raise ValueError(f"{what} must have one entry per {per} ({n}), got shape {a.shape}")
    if a.size and (not np.issubdtype(a.dtype, np.integer) or a.min() < 0 or a.max() >= n_models):
        raise ValueError(f"{what} must be integers in [0, {n_models}): the set's members")
    return np.ascontiguousarray(a, dtype=np.int32)


class ModelSet:
    """Several model directories of ONE geometry resident as one ``ww_model_set``: every launch and every :class:`StreamBank` built
    on it serves all of them - window ``w`` by member ``model_ids[w]``, stream ``s`` by member ``models[s]`` - behind one front
    end.  Member ``k`` through the set gives the bits ``Engine(member k)`` gives.  fp32 only; what may be one set:
    ``ww_model_set_create`` in include/wwhip.h (same kind, info, geometry and filter; ``ValueError`` otherwise).

    ``model_dirs``: directories, or :class:`Engine` objects of the caller's (left open by :meth:`close`)."""

    def __init__(self, model_dirs: Sequence, device: int = 0, ctx: Optional[_lib.Context] = None) -> None:
        members = list(model_dirs)
        if not 1 <= len(members) <= _lib.SET_MAX_MODELS:
            raise ValueError(f"a model set has 1..{_lib.SET_MAX_MODELS} members, not {len(members)}")
        self._own: List[Engine] = []
        self.engines: List[Engine] = []
        self._set = None
        try:
            for m in members:
                if isinstance(m, Engine):
                    self.engines.append(m)
                else:
                    ctx = ctx if ctx is not None else (self.engines[0].ctx if self.engines else _lib.default_context(device))
                    e = Engine(m, device=device, ctx=ctx)
                    self._own.append(e)
                    self.engines.append(e)
            self.ctx = self.engines[0].ctx
            self._lib = _lib.load()
            arr = (C.c_void_p * len(self.engines))(*[e.handle.value for e in self.engines])
            h = C.c_void_p()
            _lib.raise_for(self._lib.ww_model_set_create(self.ctx.handle, arr, len(self.engines), C.byref(h)), self.ctx.handle)
            self._set = h
        except Exception:
            for e in self._own:
                e.close()
            raise
        info, n = _lib.ModelInfo(), C.c_int32(0)
        _lib.raise_for(self._lib.ww_model_set_info(h, C.byref(info), C.byref(n)), self.ctx.handle)
        self.n_models = int(n.value)
        self.kind, self.window, self.n_mel, self.n_bins, self.n_out = info.kind, info.window, info.n_mel, info.n_bins, info.n_out
        self.enc_shape = (info.enc_rows, info.enc_width)
        self.names = [os.path.basename(os.path.normpath(e.model_dir)) for e in self.engines]
        _lib.register("sets", self)

    @property
    def handle(self):
        return self._set

    @property
    def posterior_index(self) -> int:
        return self.engines[0].posterior_index

    @property
    def is_crnn(self) -> bool:
        return self.kind == _lib.KIND_CRNN

    def __len__(self) -> int:
        return self.n_models

    def logmel(self, pcm: Sequence[np.ndarray], fp: Optional[_lib.FrontendParams] = None) -> List[np.ndarray]:
        """The set's one front end (member 0's; every member's filter is the same bytes)."""
        return self.engines[0].logmel(pcm, fp)

    def forward_windows_dev(self, d_mel_ptr: int, mel_rows: int, d_win_row_ptr: int, d_win_valid_ptr: int, model_ids, n_windows: int,
                            d_out_ptr: int, d_enc_ptr: int = 0) -> None:
        """``ww_set_forward_windows_dev``: :meth:`Engine.forward_windows_dev` with window ``w`` evaluated by member
        ``model_ids[w]`` (a host array).  Enqueued on the context's stream, not waited for."""
        ids = _member_ids(model_ids, int(n_windows), self.n_models, "model_ids")
        _lib.raise_for(self._lib.ww_set_forward_windows_dev(self.ctx.handle, self._set, C.c_void_p(d_mel_ptr), int(mel_rows),
                                                            C.c_void_p(d_win_row_ptr), C.c_void_p(d_win_valid_ptr), _lib.ptr(ids), int(n_windows),
                                                            C.c_void_p(d_out_ptr), C.c_void_p(d_enc_ptr) if d_enc_ptr else None), self.ctx.handle)

    def _windows(self, windows: np.ndarray) -> np.ndarray:
        w = np.ascontiguousarray(windows, dtype=np.float32)
        if w.ndim == 2:
            w = w[None]
        if w.ndim != 3 or w.shape[1] != self.window or w.shape[2] != self.n_mel:
            raise ValueError(f"Cannot set tensor: Dimension mismatch. Got {tuple(w.shape[1:])} but expected "
                             f"{(self.window, self.n_mel)} per window")
        return w

    def _launch(self, w: np.ndarray, win: np.ndarray, ids: np.ndarray, want_enc: bool):
        """One upload of the mel, one launch over the windows ``win`` (indices into ``w``), window ``i`` by member ``ids[i]``."""
        import torch
        dev = torch.device("cuda", self.ctx.device)
        n = int(win.size)
        out = torch.empty((n, self.n_out), dtype=torch.float32, device=dev)
        enc = torch.empty((n,) + self.enc_shape, dtype=torch.float32, device=dev) if want_enc else None
        if n:
            d_mel = torch.from_numpy(w.reshape(-1, self.n_mel)).to(dev)
            d_row = torch.from_numpy(win.astype(np.int64) * self.window).to(dev)
            d_valid = torch.full((n,), self.window, dtype=torch.int32, device=dev)
            torch.cuda.synchronize(dev)  # (torch's stream is not the context's)
            self.forward_windows_dev(d_mel.data_ptr(), w.shape[0] * self.window, d_row.data_ptr(), d_valid.data_ptr(), ids, n,
                                     out.data_ptr(), enc.data_ptr() if want_enc else 0)
            self.ctx.synchronize()
        return (out.cpu().numpy(), enc.cpu().numpy()) if want_enc else out.cpu().numpy()

    def forward(self, windows: np.ndarray, model_ids, want_enc: bool = False):
        """``[B, window, 40]`` -> detect rows ``[B, n_out]`` (and encoder output), window ``b`` by member ``model_ids[b]``."""
        w = self._windows(windows)
        ids = _member_ids(model_ids, w.shape[0], self.n_models, "model_ids")
        return self._launch(w, np.arange(w.shape[0]), ids, want_enc)

    def forward_all(self, windows: np.ndarray, want_enc: bool = False):
        """``[B, window, 40]`` -> ``[K, B, n_out]``: every window by every member - the table built on the host, ONE launch of
        ``K * B`` windows over ONE upload of the mel (K :meth:`Engine.forward` calls upload it K times and launch K times)."""
        w = self._windows(windows)
        B, K = w.shape[0], self.n_models
        got = self._launch(w, np.tile(np.arange(B), K), np.repeat(np.arange(K, dtype=np.int32), B), want_enc)
        if want_enc:
            return got[0].reshape(K, B, self.n_out), got[1].reshape((K, B) + self.enc_shape)
        return got.reshape(K, B, self.n_out)

    def _slots(self, members) -> Optional[np.ndarray]:
        """``members`` as the call's slot table (``None`` = every member in order): any number of ids, duplicates allowed."""
        if members is None:
            return None
        a = np.asarray(members)
        return _member_ids(a, a.size if a.ndim == 1 else -1, self.n_models, "members")

    def posterior_events(self, post, thresholds, seg_offs=None, window: int = 30, cap: Optional[int] = None, want_counts: bool = False):
        """:meth:`Engine.posterior_events` with one plane and one threshold per member: ``post`` is ``[n_models, n]``."""
        p = np.asarray(post)
        if p.ndim != 2 or p.shape[0] != self.n_models:
            raise ValueError(f"post must be [{self.n_models}, n]: one plane per member, got shape {p.shape}")
        return _events_host(self.ctx, p, thresholds, seg_offs, window, cap, want_counts)

    def posterior_events_dev(self, d_post_ptr: int, n: int, thresholds, seg_offs=None, window: int = 30, cap: Optional[int] = None,
                             want_counts: bool = False):
        """:meth:`Engine.posterior_events_dev` over ``[n_models, n]`` device posteriors, one threshold per member."""
        return _events_dev(self.ctx, d_post_ptr, n, self.n_models, thresholds, seg_offs, window, cap, want_counts)

    def set_option(self, key: str, value: int) -> None:
        """``ww_set_option``: ``"crnn_slide_min"`` / ``"crnn_tail_mfma"`` (:meth:`Engine.set_option`'s meanings) for the set's
        sliding launches, ``"wave_seq_segment"`` (likewise) for the cuts of :meth:`sequence_forward` /
        :meth:`sequence_forward_all`.  They move the launch form, never the bits."""
        keys = {"crnn_slide_min": _lib.OPT_CRNN_SLIDE_MIN, "crnn_tail_mfma": _lib.OPT_CRNN_TAIL_MFMA,
                "wave_seq_segment": _lib.OPT_WAVE_SEQ_SEGMENT}
        if key not in keys:
            raise ValueError(f"a model set takes the options {sorted(keys)}, not {key!r}")
        _lib.raise_for(self._lib.ww_set_option(self._set, keys[key], int(value)), self.ctx.handle)

    def forward_segments_dev(self, d_mel_ptr: int, mel_rows: int, seg_row0: np.ndarray, seg_nw: np.ndarray, hop: int, d_out_ptr: int,
                             members=None) -> None:
        """``ww_set_forward_segments_dev``: :meth:`Engine.forward_segments_dev` by every member of ``members`` (``None``: all, in
        order) in one call - ``d_out`` is ``[len(members), sum(seg_nw), n_out]``, plane ``k`` what member ``members[k]`` gives on
        its own.  A CRNN set slides with ONE rows-kernel launch and ONE tail launch per group of sequences, whatever the number
        of members.  The descriptor arrays are host arrays.  Enqueued on the context's stream, not waited for."""
        r0 = np.ascontiguousarray(seg_row0, dtype=np.int64)
        nw = np.ascontiguousarray(seg_nw, dtype=np.int32)
        if r0.shape != nw.shape or r0.ndim != 1:
            raise ValueError("seg_row0 and seg_nw must be 1-D arrays of the same length")
        ids = self._slots(members)
        _lib.raise_for(self._lib.ww_set_forward_segments_dev(self.ctx.handle, self._set, C.c_void_p(d_mel_ptr), int(mel_rows), _lib.ptr(r0),
                                                             _lib.ptr(nw), int(r0.size), int(hop), _lib.ptr(ids) if ids is not None else None,
                                                             int(ids.size) if ids is not None else 0, C.c_void_p(d_out_ptr)), self.ctx.handle)

    def slide_forward_all(self, mel: np.ndarray, hop: int = 2, members=None) -> np.ndarray:
        """``[rows, 40]`` -> ``[K', n_windows, n_out]``: :meth:`Engine.slide_forward` by every member of ``members`` (``None``: all)
        over ONE upload of the sequence (``ww_set_slide_forward``)."""
        mel = np.ascontiguousarray(mel, dtype=np.float32)
        if mel.ndim != 2 or mel.shape[1] != self.n_mel:
            raise ValueError(f"mel must be [rows, {self.n_mel}], got {mel.shape}")
        ids = self._slots(members)
        k = self.n_models if ids is None else int(ids.size)
        rows = mel.shape[0]
        nw = max(0, (rows - self.window) // hop + 1) if rows >= self.window and hop > 0 else 0
        out = np.empty((k, nw, self.n_out), np.float32)
        n = C.c_int64(0)
        _lib.raise_for(self._lib.ww_set_slide_forward(self.ctx.handle, self._set, _lib.ptr(mel), rows, int(hop),
                                                      _lib.ptr(ids) if ids is not None else None, int(ids.size) if ids is not None else 0,
                                                      _lib.ptr(out), C.byref(n)), self.ctx.handle)
        assert n.value == nw, (n.value, nw)
        return out

    def sequence_forward(self, mels, model_ids, pool: Optional[int] = None, want: Sequence[str] = ("post",)) -> dict:
        """:meth:`Engine.sequence_forward` with sequence ``s`` evaluated by member ``model_ids[s]`` (``ww_set_wave_sequence``): one
        upload, one launch of the model kernel over all sequences, whoever their members are.  Same arguments otherwise, the
        same return shape, and for every sequence the bits its member's engine gives on it alone.  Wavenet sets only."""
        want, seqs, offs, mel = _sequence_batch(mels, self.n_mel, want)
        ids = _member_ids(model_ids, len(seqs), self.n_models, "seq_model")
        total = int(offs[-1])
        bufs = _sequence_buffers(self.n_out, self.enc_shape[1], want, None, total, len(seqs))
        _lib.raise_for(self._lib.ww_set_wave_sequence(self.ctx.handle, self._set, _lib.ptr(mel), total, _lib.ptr(offs), len(seqs), _lib.ptr(ids),
                                                      self.window if pool is None else int(pool), _lib.ptr(bufs["enc"]),
                                                      _lib.ptr(bufs["logits"]), _lib.ptr(bufs["post_frames"]), _lib.ptr(bufs["post"])),
                       self.ctx.handle)
        return _per_sequence(bufs, want, offs)

    def sequence_forward_all(self, mels, members=None, pool: Optional[int] = None, want: Sequence[str] = ("post",)) -> dict:
        """Every sequence by every member of ``members`` (``None``: all, in order; any number of ids, duplicates allowed) over ONE
        upload of the mel (``ww_set_wave_sequence_all``) - the checkpoint loop of the reference's ``eval_models`` on whole
        recordings.  Returns ``{name: [per slot][per sequence]}``: entry ``[k]`` is what ``Engine(member members[k])
        .sequence_forward(mels, pool, want)[name]`` returns, bit for bit."""
        want, seqs, offs, mel = _sequence_batch(mels, self.n_mel, want)
        ids = self._slots(members)
        k = self.n_models if ids is None else int(ids.size)
        total = int(offs[-1])
        bufs = _sequence_buffers(self.n_out, self.enc_shape[1], want, k, total, len(seqs))
        _lib.raise_for(self._lib.ww_set_wave_sequence_all(self.ctx.handle, self._set, _lib.ptr(mel), total, _lib.ptr(offs), len(seqs),
                                                          self.window if pool is None else int(pool), _lib.ptr(ids) if ids is not None else None,
                                                          k if ids is not None else 0, _lib.ptr(bufs["enc"]), _lib.ptr(bufs["logits"]),
                                                          _lib.ptr(bufs["post_frames"]), _lib.ptr(bufs["post"])), self.ctx.handle)
        return {name: [_per_sequence({name: bufs[name][j]}, (name,), offs)[name] for j in range(k)] for name in want}

    def wave_sequence_dev(self, d_mel_ptr: int, total_rows: int, row_offs: np.ndarray, model_ids, pool: Optional[int] = None,
                          d_enc_ptr: int = 0, d_logits_ptr: int = 0, d_post_frames_ptr: int = 0, d_post_ptr: int = 0) -> None:
        """:meth:`sequence_forward` on device buffers (``ww_set_wave_sequence_dev``): :meth:`Engine.wave_sequence_dev` with
        sequence ``s`` by member ``model_ids[s]`` (a host array).  Enqueued on the context's stream, not waited for."""
        offs = _row_offs(row_offs)
        ids = _member_ids(model_ids, int(offs.size - 1), self.n_models, "seq_model")
        _lib.raise_for(self._lib.ww_set_wave_sequence_dev(self.ctx.handle, self._set, _vp(d_mel_ptr), int(total_rows), _lib.ptr(offs),
                                                          int(offs.size - 1), _lib.ptr(ids), self.window if pool is None else int(pool),
                                                          _vp(d_enc_ptr), _vp(d_logits_ptr), _vp(d_post_frames_ptr), _vp(d_post_ptr)), self.ctx.handle)

    def wave_sequence_all_dev(self, d_mel_ptr: int, total_rows: int, row_offs: np.ndarray, members=None, pool: Optional[int] = None,
                              d_enc_ptr: int = 0, d_logits_ptr: int = 0, d_post_frames_ptr: int = 0, d_post_ptr: int = 0) -> None:
        """:meth:`sequence_forward_all` on device buffers (``ww_set_wave_sequence_all_dev``): plane ``k`` of every output -
        ``[len(members), total_rows, ...]``, ``post`` ``[len(members), n_seq, n_out]`` - is member ``members[k]``'s.  Enqueued on
        the context's stream, not waited for."""
        offs = _row_offs(row_offs)
        ids = self._slots(members)
        _lib.raise_for(self._lib.ww_set_wave_sequence_all_dev(self.ctx.handle, self._set, _vp(d_mel_ptr), int(total_rows), _lib.ptr(offs),
                                                              int(offs.size - 1), self.window if pool is None else int(pool),
                                                              _lib.ptr(ids) if ids is not None else None, int(ids.size) if ids is not None else 0,
                                                              _vp(d_enc_ptr), _vp(d_logits_ptr), _vp(d_post_frames_ptr), _vp(d_post_ptr)),
                       self.ctx.handle)

    def close(self) -> None:
        if self._set and not _lib.is_shutdown():
            self._lib.ww_model_set_destroy(self._set)
        self._set = None
        for e in self._own:
            e.close()
        self._own = []

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass


MAX_RATES = 8  # WW_STREAM_MAX_RATES
MAX_MEMBER_SLOTS = 64  # WW_ALL_MAX_MEMBERS (csrc/stream_all.h)


def _member_slots(members, engine, n_streams: int, models, full_recompute: bool) -> np.ndarray:
    """``members=`` of a :class:`StreamBank` -> the ``int32[K]`` member slots.  Everything that can be refused without a device is
    refused here."""
    if not isinstance(engine, ModelSet):
        raise ValueError("members= names members of a ModelSet: this bank is built on one Engine")
    if models is not None:
        raise ValueError("members= (every listed member on every stream) and models= (one member per stream) are mutually exclusive")
    if full_recompute:
        raise ValueError("full_recompute is not offered on a ModelSet")
    if isinstance(members, str):
        if members != "all":
            raise ValueError(f"members must be \"all\" or a list of member ids, got {members!r}")
        a = np.arange(engine.n_models, dtype=np.int32)
    else:
        a = np.asarray(members)
        if a.ndim != 1 or a.size == 0 or not np.issubdtype(a.dtype, np.integer) or a.min() < 0 or a.max() >= engine.n_models:
            raise ValueError(f"members must be a non-empty list of integers in [0, {engine.n_models}): the set's members")
        a = np.ascontiguousarray(a, dtype=np.int32)
    if a.size > MAX_MEMBER_SLOTS:
        raise ValueError(f"{a.size} member slots: a bank runs at most {MAX_MEMBER_SLOTS} on every stream")
    if n_streams * a.size > 65535:
        raise ValueError(f"{n_streams} streams x {a.size} member slots: a bank has at most 65535 of them")
    return a


def _stream_rates(sample_rate, n_streams: int, resampler) -> np.ndarray:
    """``sample_rate`` given per stream -> the ``int32[S]`` rates.  Everything that can be refused without a device is refused here."""
    if resampler is not None:
        raise ValueError("resampler= belongs to a bank at ONE rate: a bank with per-stream rates creates and owns its resamplers")
    rates = np.asarray(sample_rate)
    if rates.ndim != 1 or rates.size != n_streams:
        raise ValueError(f"sample_rate must name one rate per stream ({n_streams}), got {rates.size if rates.ndim == 1 else rates.shape}")
    if rates.dtype.kind not in "iu":
        raise ValueError("sample_rate must be whole numbers of Hz")
    rates = rates.astype(np.int64)
    for r in rates.tolist():
        if r <= 0 or r % 50:
            raise ValueError(f"sample_rate {r}: a 20 ms frame must be a whole number of samples "
                             "(rates with a fractional frame are not offered in the tick)")
    if len(set(rates.tolist())) > MAX_RATES:
        raise ValueError(f"{len(set(rates.tolist()))} distinct sample rates: a bank has at most {MAX_RATES} rate classes")
    return rates.astype(np.int32)


SAMPLE_FORMATS = {"pcm16": _lib.SAMPLE_I16, "mulaw": _lib.SAMPLE_MULAW, "alaw": _lib.SAMPLE_ALAW}  # a stream's format -> WW_SAMPLE_*
_FORMAT_NAMES = {v: k for k, v in SAMPLE_FORMATS.items()}
_FORMAT_DTYPE = {"pcm16": np.dtype(np.int16), "mulaw": np.dtype(np.uint8), "alaw": np.dtype(np.uint8)}


def _stream_formats(sample_format, n_streams: int) -> List[str]:
    """``sample_format`` -> one format name per stream.  Everything that can be refused without a device is refused here."""
    names = [sample_format] * n_streams if isinstance(sample_format, str) else list(sample_format)
    if len(names) != n_streams:
        raise ValueError(f"sample_format must name one format per stream ({n_streams}), got {len(names)}")
    for f in names:
        if not isinstance(f, str) or f not in SAMPLE_FORMATS:
            raise ValueError(f"unknown sample format {f!r}: one of {', '.join(SAMPLE_FORMATS)}")
    return names


def _stream_classes(sample_rate, sample_format, resampler, n_streams: int):
    """What ``StreamBank`` was asked for -> (rates, one format name per stream, per-stream form?).  A scalar rate with pcm16 streams,
    or a scalar rate other than 16000 with a scalar format, is the bank at ONE rate - plain at 16000, else uniform; ``rates`` is that
    rate, ``resampler``'s input rate where one is given.  Anything else is the per-stream form, even with one distinct rate:
    ``rates`` is ``int32[S]``.  Everything that can be refused without a device is refused here."""
    names = _stream_formats(sample_format, n_streams)
    scalar = isinstance(sample_rate, (int, np.integer))
    g711 = any(f != "pcm16" for f in names)
    if not scalar or (g711 and not (isinstance(sample_format, str) and int(sample_rate) != 16000)):
        rates = _stream_rates([int(sample_rate)] * n_streams if scalar else sample_rate, n_streams, resampler)
        pairs = set(zip(rates.tolist(), names))
        if len(pairs) > MAX_RATES:
            raise ValueError(f"{len(pairs)} distinct (rate, format) pairs: a bank has at most {MAX_RATES} classes")
        return rates, names, True
    rate = int(sample_rate if resampler is None else resampler.rate_in)
    if resampler is not None and int(sample_rate) not in (16000, rate):
        raise ValueError(f"sample_rate = {sample_rate}, but the resampler reads {rate} Hz")
    if rate <= 0 or rate % 50:
        raise ValueError(f"sample_rate {rate}: a 20 ms frame must be a whole number of samples "
                         "(rates with a fractional frame are not offered in the tick)")
    if resampler is not None and rate == 16000:
        raise ValueError("a resampler from 16000 Hz: that is a plain bank")
    return rate, names, False


def _checked_samples(a, fmt: str, what: str) -> np.ndarray:
    """``a`` as a flat contiguous array of the dtype ``fmt`` is carried in - int16 for pcm16, uint8 codes for mulaw / alaw; an array
    of the other kind is refused, not converted."""
    a = np.asarray(a)
    if a.dtype != _FORMAT_DTYPE[fmt]:
        raise ValueError(f"{what} reads {fmt}: its samples are {_FORMAT_DTYPE[fmt]}, not {a.dtype}")
    return np.ascontiguousarray(a).ravel()


class StreamBank:
    """S device-resident streams advanced 20 ms per :meth:`step` (``ww_stream_*``)."""
    _mixed = False  # the per-stream form (ww_stream_attach_rates[_fmt]): every stream in a (rate, format) class of its own choosing
    _g711 = False  # some class reads G.711 (sample_format=): frames and packets are byte blocks
    members, n_members = None, 0  # the member slots of a bank that runs every listed member on every stream (members=)

    def _no_every(self, what: str) -> None:
        if self.n_members:
            raise ValueError(f"{what}: this bank runs every listed member on every stream (members=): it has step, feed_all, "
                             "step_trigger_all, reset, window and set_rate")

    def __init__(self, engine, n_streams: int, fp: Optional[_lib.FrontendParams] = None,
                 full_recompute: bool = False, two_launch: bool = False, sync_wait: bool = False, causal: bool = False,
                 models: Optional[Sequence[int]] = None, sample_rate: int = 16000, resampler=None, members=None,
                 sample_format="pcm16") -> None:
        """``full_recompute``: every streaming CRNN window recomputed from its mel rows (``WW_STREAM_FULL_RECOMPUTE``)
        instead of the incremental kernel.  ``two_launch``: the incremental CRNN's tick as a front-end kernel + a model kernel
        (``WW_STREAM_TWO_LAUNCH``; default: ONE launch per tick).  ``sync_wait``: wait for a tick with ``hipStreamSynchronize``
        instead of polling its posteriors in page-locked memory (``WW_STREAM_SYNC_WAIT``).  Same bits in every form.
        ``causal`` (fp32 Wavenet only, ``WW_STREAM_CAUSAL``): another model reading, not another form - the bank advances
        :meth:`Engine.sequence_forward` row by row from cached activations; a posterior is ``post_frames`` of the stream's rows
        since its last reset (every sampled row advances the state; rows that arrive while ``is_speech`` is set emit).
        ``engine`` may be a :class:`ModelSet`: stream ``s`` is then served by member ``models[s]`` (default: all by member 0;
        ``ww_stream_create_set``) and :meth:`set_model` moves streams between members; ``full_recompute`` is refused.
        ``sample_rate`` other than 16000: the bank runs at that rate (``ww_stream_attach_resampler``) - :meth:`step` takes
        ``[S, frame_samples]`` frames, ``frame_samples = sample_rate / 50``, :meth:`feed` packets at that rate, and every stream
        yields the bits of the 16 kHz bank given its resampled signal behind ``D`` zeros (``include/wwhip.h``).  The bank creates
        and owns a ``Resampler(sample_rate, 16000, ctx)``, or takes ``resampler`` (which must outlive it).
        ``sample_rate`` as a SEQUENCE of S rates (up to 8 distinct ones; always this form, even with one distinct rate): stream
        ``s`` runs at ``sample_rate[s]`` (``ww_stream_attach_rates``) and yields the bits it yields in a bank at that rate alone.
        :attr:`sample_rates`, :attr:`frame_samples` (``int32[S]``) and :attr:`frame_offs` (``int64[S + 1]``) describe a tick's
        frames: ONE flat int16 block of ``frame_offs[S]`` samples, stream ``s``'s ``sample_rate[s] / 50`` samples from
        ``frame_offs[s]`` - or a sequence of S per-stream arrays, which is concatenated.  :meth:`feed` takes each stream's packet
        at that stream's rate, :meth:`set_rate` moves streams to another of the bank's rates.  The bank creates and owns one
        ``Resampler(r, 16000, ctx)`` per distinct rate other than 16000.
        ``members="all"`` or a list of member ids of a :class:`ModelSet` (up to 64, repeats allowed; not together with ``models``):
        EVERY listed member runs on EVERY stream (``ww_stream_create_set_all``) - one front end per stream, K = ``n_members`` model
        states.  :meth:`step` takes the frames of S streams as always and returns ``(post[S, K, 2], n[S])``: ``post[s, j]`` is the
        bits a bank of member ``members[j]`` alone yields.  :meth:`reset`, :meth:`window`, :meth:`set_rate` and ``sample_rate`` work
        as before; a causal bank of this kind is fed in packets by :meth:`feed_all`, and :meth:`step_trigger_all` is its wake-word
        stage (``wwhip.wakeword.WakewordSetBank``); :meth:`feed`, :meth:`set_model` and :meth:`step_trigger` raise ``ValueError``.
        ``sample_format``: ``"pcm16"`` (the default), ``"mulaw"`` or ``"alaw"`` - G.711, one byte per sample, as a telephony leg
        carries it, decoded in the kernels that read the samples -, or a sequence of S of them.  A G.711 stream yields the bits it
        yields given its decoded int16 samples.  A scalar rate other than 16000 with a scalar format is the uniform bank
        (``ww_stream_attach_resampler_fmt``): :meth:`step` takes ``[S, frame_samples]`` uint8.  Anything else is the per-stream form
        (``ww_stream_attach_rates_fmt``; a class is a (rate, format) pair, up to 8): :meth:`step` takes the flat uint8 block of
        ``frame_byte_offs[S]`` bytes - stream ``s``'s ``frame_bytes[s]`` bytes from ``frame_byte_offs[s]``; an int16 frame starts on
        an even byte, behind one pad byte where needed - or S per-stream arrays, int16 for a pcm16 stream and uint8 for a G.711
        one (an array of the other kind is refused).  :meth:`feed` / :meth:`feed_all` take per-stream packets the same way, and
        :meth:`set_rate` takes the format beside the rate.  :attr:`sample_formats`, :attr:`frame_bytes` and
        :attr:`frame_byte_offs` are there on every bank."""
        self.engine = engine
        self.S = int(n_streams)
        # ---- what was asked for, and every refusal that needs no device
        rates, names, self._mixed = _stream_classes(sample_rate, sample_format, resampler, self.S)
        self._g711 = any(f != "pcm16" for f in names)
        self.sample_rate = None if self._mixed else rates
        self._classes = list(dict.fromkeys(zip(rates.tolist(), names))) if self._mixed else None  # (rate, format) pairs in class order
        self.members = None if members is None else _member_slots(members, engine, self.S, models, full_recompute)
        self.n_members = 0 if self.members is None else int(self.members.size)
        is_set = isinstance(engine, ModelSet)
        if models is not None and not is_set:
            raise ValueError("models= names the members of a ModelSet: this bank is built on one Engine")
        if is_set and full_recompute:
            raise ValueError("full_recompute is not offered on a ModelSet")
        ids = _member_ids(models, self.S, engine.n_models, "models") if models is not None else None
        # ---- the bank, its one attach call, its layout
        self._resampler, self._own_resampler, self._class_rs = resampler, False, []
        self._create(fp, full_recompute, two_launch, sync_wait, causal, ids)
        try:
            self._attach(rates, names)
            self._read_layout()
            assert (self.sample_rates == rates).all(), (self.sample_rates, rates)
        except Exception:
            self.close()
            raise
        self._tick_arrays()

    def _create(self, fp, full_recompute, two_launch, sync_wait, causal, ids) -> None:
        engine = self.engine
        self._lib = _lib.load()
        fp = fp or frontend_params()
        h = C.c_void_p()
        flags = ((_lib.STREAM_FULL_RECOMPUTE if full_recompute else 0) | (_lib.STREAM_TWO_LAUNCH if two_launch else 0)
                 | (_lib.STREAM_SYNC_WAIT if sync_wait else 0) | (_lib.STREAM_CAUSAL if causal else 0))
        self.causal = bool(causal)
        if self.n_members:
            _lib.raise_for(self._lib.ww_stream_create_set_all(engine.ctx.handle, engine.handle, self.S, _lib.ptr(self.members), self.n_members,
                                                              C.byref(fp), flags, C.byref(h)), engine.ctx.handle)
        elif isinstance(engine, ModelSet):
            _lib.raise_for(self._lib.ww_stream_create_set(engine.ctx.handle, engine.handle, self.S, _lib.ptr(ids), C.byref(fp), flags, C.byref(h)),
                           engine.ctx.handle)
        else:
            _lib.raise_for(self._lib.ww_stream_create(engine.ctx.handle, engine.handle, self.S, C.byref(fp), flags, C.byref(h)),
                           engine.ctx.handle)
        self._h = h
        _lib.register("streams", self)

    def _attach(self, rates, names: List[str]) -> None:
        """The bank's one attach call: none (a plain bank), ``ww_stream_attach_resampler[_fmt]`` (the uniform bank: ``rates`` is its one
        rate) or ``ww_stream_attach_rates[_fmt]`` (the per-stream form: ``rates[s]``, ``names[s]`` name stream ``s``'s class)."""
        if not self._mixed and rates == 16000:
            return
        from .resample import Resampler
        lib, ctx = self._lib, self.engine.ctx
        if not self._mixed:
            if self._resampler is None:
                self._resampler, self._own_resampler = Resampler(rates, 16000, ctx), True
            rc = (lib.ww_stream_attach_resampler_fmt(self._h, self._resampler._h, SAMPLE_FORMATS[names[0]]) if self._g711
                  else lib.ww_stream_attach_resampler(self._h, self._resampler._h))
        else:
            classes, by_rate = self._classes, {}  # (two formats of one rate share the rate's resampler)
            for r, _ in classes:
                if r != 16000 and r not in by_rate:
                    by_rate[r] = Resampler(r, 16000, ctx)
                    self._class_rs.append(by_rate[r])
            table = (C.c_void_p * len(classes))(*[None if r == 16000 else by_rate[r]._h for r, _ in classes])
            cls = np.array([classes.index(c) for c in zip(rates.tolist(), names)], np.int32)
            if self._g711:
                fm = np.array([SAMPLE_FORMATS[f] for _, f in classes], np.int32)
                rc = lib.ww_stream_attach_rates_fmt(self._h, table, _lib.ptr(fm), len(classes), _lib.ptr(cls))
            else:
                rc = lib.ww_stream_attach_rates(self._h, table, len(classes), _lib.ptr(cls))
        _lib.raise_for(rc, ctx.handle)

    def _read_layout(self) -> None:
        """A tick's frames as the library states them (``ww_stream_frame_layout_bytes``, which answers on every bank): the six public
        layout attributes, and the dtype and shape :meth:`_frames_address` passes without a second look.  Read again after a
        :meth:`set_rate`.  ``frame_offs`` counts int16 samples: a bank with G.711 streams has none, and a bank without them has no pad
        bytes, so its sample offsets are the byte offsets halved."""
        S = self.S
        fb, bo, fm = np.zeros(S, np.int32), np.zeros(S + 1, np.int64), np.zeros(S, np.int32)
        _lib.raise_for(self._lib.ww_stream_frame_layout_bytes(self._h, _lib.ptr(fb), _lib.ptr(bo), _lib.ptr(fm)), self.engine.ctx.handle)
        fs = fb // np.where(fm == _lib.SAMPLE_I16, 2, 1).astype(np.int32)
        self.frame_bytes, self.frame_byte_offs, self.sample_formats = fb, bo, [_FORMAT_NAMES[int(v)] for v in fm]
        self.frame_samples, self.sample_rates = (fs if self._mixed else int(fs[0])), fs * 50
        self.frame_offs = None if self._g711 else bo // 2
        self._dtype = np.dtype(np.uint8 if self._g711 else np.int16)
        self._shape = (int(bo[S]) // self._dtype.itemsize,) if self._mixed else (S, int(fs[0]))

    def _tick_arrays(self) -> None:
        self._post = np.zeros((self.S, self.n_members, 2) if self.n_members else (self.S, 2), np.float32)
        self._n = np.zeros(self.S, np.int32)
        self._flags = np.zeros(self.S, np.uint8)
        # a tick is host-paced (spokestack/pipeline.py:25-28): the addresses of the bank's own arrays are taken once, not per call
        self._p_post, self._p_n, self._p_flags = (C.c_void_p(a.ctypes.data) for a in (self._post, self._n, self._flags))
        self._step = self._lib.ww_stream_step_all if self.n_members else self._lib.ww_stream_step
        self._keep = None

    def _stage_frames(self, frames) -> np.ndarray:
        """A tick's frames in any accepted form -> the block the library reads, placed and checked by the layout.  A whole block -
        the flat one of ``frame_byte_offs[S]`` bytes, on a bank at one rate also ``[S, frame_samples]`` or anything numpy stacks to
        it - is passed on; S per-stream arrays (the per-stream form) go to ``frame_byte_offs[s]`` each, pad bytes zero.  A bank
        without G.711 streams converts to int16; one with them refuses an array of the other kind."""
        S, total = self.S, int(self.frame_byte_offs[self.S])
        holds = f"{total} bytes" if self._g711 else f"{total // 2} int16 samples"
        which = "ww_stream_frame_layout_bytes" if self._g711 else "ww_stream_frame_layout"
        if not self._mixed or (type(frames) is np.ndarray and frames.ndim == 1 and frames.dtype != object):
            if not self._g711:
                f = np.ascontiguousarray(frames, dtype=np.int16)
            elif np.asarray(frames).dtype != np.uint8:
                raise ValueError(f"the block of a bank with G.711 streams is uint8 ({holds}: {which}), not {np.asarray(frames).dtype}")
            else:
                f = np.ascontiguousarray(frames)
            if f.shape != self._shape and f.shape != (total // self._dtype.itemsize,):
                raise ValueError(f"frames must hold {holds} ({which}), got {f.size}" if self._mixed
                                 else f"frames must be [{S}, {self._shape[1]}] {self._dtype}")
            return f
        if len(frames) != S:
            raise ValueError(f"frames must be one array per stream ({S}) or the flat block of {holds}")
        block = np.zeros(total, np.uint8)
        for s, a in enumerate(frames):
            a = (_checked_samples(a, self.sample_formats[s], f"stream {s}") if self._g711 else np.ascontiguousarray(a, dtype=np.int16).ravel())
            at = int(self.frame_byte_offs[s])
            if a.nbytes != self.frame_bytes[s]:
                raise ValueError(f"stream {s}'s frame has {int(self.frame_bytes[s]) // a.itemsize} samples, got {a.size} (frames must hold {holds})")
            block[at:at + a.nbytes] = a.view(np.uint8)
        return block

    def _frames_address(self, frames: np.ndarray) -> int:
        f = frames
        if not (type(f) is np.ndarray and f.dtype == self._dtype and f.flags.c_contiguous and f.shape == self._shape):
            f = self._keep = self._stage_frames(frames)  # (kept alive until the call has returned)
        try:
            return C.addressof(C.c_char.from_buffer(f))  # (a third of the cost of f.ctypes.data_as)
        except (TypeError, ValueError):                   # a read-only array
            return f.ctypes.data

    def step_trigger(self, frames: np.ndarray, p_is_speech, p_is_active, threshold: float, p_state) -> None:
        """The wake-word stage of all streams as ONE library call (``ww_stream_step_trigger``): the tick, the trigger logic of
        ``WakewordTrigger.__call__`` over its posteriors and the reset of the streams whose VAD bit fell.  Every argument but
        ``frames`` is an address taken once with ``_lib.addr`` (``WakewordBank`` owns the arrays): ``p_state`` =
        (was_speech, posterior_max, post, n_post, fired_ids, n_fired, fall_ids, n_fall)."""
        self._no_every("step_trigger")
        rc = self._lib.ww_stream_step_trigger(self._h, self._frames_address(frames), p_is_speech, p_is_active, threshold, *p_state)
        if rc:
            _lib.raise_for(rc, self.engine.ctx.handle)

    def step(self, frames: np.ndarray, is_speech: np.ndarray, is_active: Optional[np.ndarray] = None) -> Tuple[np.ndarray, np.ndarray]:
        pf = self._frames_address(frames)
        sp = is_speech
        if not (type(sp) is np.ndarray and sp.dtype == np.uint8 and sp.ndim == 1):
            sp = np.ascontiguousarray(is_speech, dtype=np.uint8).ravel()
        if sp.size != self.S:
            raise ValueError("is_speech must have one entry per stream")
        np.bitwise_and(sp, 1, out=self._flags)
        if is_active is not None:
            self._flags |= (np.ascontiguousarray(is_active, dtype=np.uint8).ravel() & 1) << 1
        rc = self._step(self._h, pf, self._p_flags, self._p_post, self._p_n)
        if rc:
            _lib.raise_for(rc, self.engine.ctx.handle)
        return self._post.copy(), self._n.copy()  # the caller owns what it gets (like TFLiteModel's get_tensor copies)

    TIMELINE_PHASES = ("plan", "frames_in", "launch_1", "launch_2", "wait", "copy_out")

    def timeline(self, reset: bool = False) -> dict:
        """Mean host-side microseconds per phase of ``ww_stream_step`` since the last reset (``ww_stream_timeline``)."""
        ns = (C.c_double * len(self.TIMELINE_PHASES))()
        ticks = C.c_int64(0)
        _lib.raise_for(self._lib.ww_stream_timeline(self._h, ns, C.byref(ticks), int(reset)), self.engine.ctx.handle)
        out = {k: ns[i] * 1e-3 for i, k in enumerate(self.TIMELINE_PHASES)}
        out["ticks"] = int(ticks.value)
        return out

    def reset(self, ids: Optional[Sequence[int]] = None) -> None:
        if ids is None:
            _lib.raise_for(self._lib.ww_stream_reset(self._h, None, 0), self.engine.ctx.handle)
        else:
            a = np.ascontiguousarray(ids, dtype=np.int32)
            _lib.raise_for(self._lib.ww_stream_reset(self._h, _lib.ptr(a), a.size), self.engine.ctx.handle)

    def set_model(self, ids: Optional[Sequence[int]], model: int) -> None:
        """Move the listed streams (``None``: all) to member ``model`` of the bank's :class:`ModelSet` and reset them
        (``ww_stream_set_model``: a stream's cached activations belong to the model that made them)."""
        self._no_every("set_model")
        if not isinstance(self.engine, ModelSet):
            raise ValueError("set_model: this bank was not built on a ModelSet")
        if not 0 <= int(model) < self.engine.n_models:
            raise ValueError(f"model must be in [0, {self.engine.n_models})")
        a = None if ids is None else np.ascontiguousarray(ids, dtype=np.int32).ravel()
        if a is not None and a.size and (a.min() < 0 or a.max() >= self.S):
            raise ValueError("stream id out of range")
        _lib.raise_for(self._lib.ww_stream_set_model(self._h, _lib.ptr(a), 0 if a is None else a.size, int(model)), self.engine.ctx.handle)

    def set_rate(self, ids: Optional[Sequence[int]], rate: int, sample_format: Optional[str] = None) -> None:
        """Move the listed streams (``None``: all) to ``rate`` Hz, one of the rates the bank was built with, and reset them
        (``ww_stream_set_rate``: the next sample is the first of a new signal).  ``frame_samples``, ``frame_offs`` and
        ``sample_rates`` are read again: the layout of a tick's frames changes with the move.  A bank built with ``sample_format``:
        the streams move to the class (``rate``, ``sample_format``); the format may be left out where the bank has the rate in one
        format only."""
        if not self._mixed:
            raise ValueError("set_rate: this bank runs at one rate (sample_rate was not given per stream)")
        if not self._g711 and sample_format not in (None, "pcm16"):
            raise ValueError(f"set_rate: this bank's streams all read pcm16, not {sample_format}")
        if sample_format is not None and sample_format not in SAMPLE_FORMATS:
            raise ValueError(f"unknown sample format {sample_format!r}: one of {', '.join(SAMPLE_FORMATS)}")
        hits = [k for k, c in enumerate(self._classes) if c[0] == int(rate) and sample_format in (None, c[1])]
        if len(hits) != 1:
            raise ValueError(f"set_rate: ({rate} Hz, {sample_format}) names {len(hits)} of the bank's classes {self._classes}" if self._g711
                             else f"set_rate: {rate} Hz is not among the bank's rates {[c[0] for c in self._classes]}")
        a = None if ids is None else np.ascontiguousarray(ids, dtype=np.int32).ravel()
        if a is not None and a.size and (a.min() < 0 or a.max() >= self.S):
            raise ValueError("stream id out of range")
        _lib.raise_for(self._lib.ww_stream_set_rate(self._h, _lib.ptr(a), 0 if a is None else a.size, hits[0]), self.engine.ctx.handle)
        self._read_layout()

    def window(self, stream: int) -> np.ndarray:
        """Stream ``stream``'s newest ``[window, n_mel]`` mel window, the block the model reads (``ww_stream_window``: a
        read-out; the bank's state is left as it is)."""
        out = np.empty((self.engine.window, self.engine.n_mel), np.float32)
        _lib.raise_for(self._lib.ww_stream_window(self._h, int(stream), _lib.ptr(out)), self.engine.ctx.handle)
        return out

    def feed(self, ids: Sequence[int], packets: Sequence[np.ndarray], want_mel: bool = False):
        """A causal bank advanced by any subset of its streams and any number of samples for each (``ww_stream_feed``):
        stream ``ids[i]`` receives the int16 samples ``packets[i]``.  Returns ``(posts, mels)``: per listed stream the posteriors
        of its new mel rows ``[rows]`` and, with ``want_mel``, the rows themselves ``[rows, n_mel]`` (``mels`` is ``None``
        otherwise).  However the samples are cut into packets, calls and :meth:`step` ticks, the results are the same bits.
        A bank at another rate, or with per-stream rates: each packet is at its stream's own rate."""
        self._no_every("feed")
        return self._feed(ids, packets, want_mel, False)

    def _feed(self, ids: Sequence[int], packets: Sequence[np.ndarray], want_mel: bool, every: bool):
        """:meth:`feed` (``every`` false) and :meth:`feed_all`: the call's ids and packets staged as one buffer, the library asked for
        the rows the call will produce (``ww_stream_feed_rows[_all]``), then fed (``ww_stream_feed[_all]``), and the results cut per
        listed stream.  A bank with G.711 streams feeds bytes (``ww_stream_feed_bytes[_all]``): ``packets[i]`` is int16 for a pcm16
        stream and uint8 for a G.711 one, and as an int16 packet starts on an even byte of the gapless buffer the int16 packets go
        first; the results come back in the caller's order."""
        a_ids = np.ascontiguousarray(ids, dtype=np.int32).ravel()
        n = int(a_ids.size)
        if len(packets) != n:
            raise ValueError("one packet per listed stream")
        back = range(n)
        if self._g711:
            if n and (a_ids.min() < 0 or a_ids.max() >= self.S):
                raise ValueError("stream id out of range")
            pk = [_checked_samples(p, self.sample_formats[int(s)], f"stream {int(s)}") for s, p in zip(a_ids, packets)]
            order = sorted(range(n), key=lambda i: pk[i].dtype != np.int16)  # (stable: int16 packets first)
            a_ids = np.ascontiguousarray(a_ids[order]) if n else a_ids
            pk, back = [pk[i] for i in order], np.argsort(order) if n else []
        else:
            pk = [np.ascontiguousarray(p, dtype=np.int16).ravel() for p in packets]
        counts = np.zeros(n + 1, np.int64)  # the packets' samples: ww_stream_feed_rows counts these on every bank
        np.cumsum([p.size for p in pk], out=counts[1:])
        offs = counts  # where packet i lies in the buffer: in samples, or on a bank with G.711 streams in bytes
        if self._g711:
            offs = np.zeros(n + 1, np.int64)
            np.cumsum([p.nbytes for p in pk], out=offs[1:])
            pk = [p.view(np.uint8) for p in pk]
        data = np.concatenate(pk) if n and offs[n] else np.zeros(2, np.uint8)
        row_offs = np.zeros(n + 1, np.int64)
        lib, h = self._lib, self.engine.ctx.handle
        rows_fn, feed_fn = {(False, False): (lib.ww_stream_feed_rows, lib.ww_stream_feed),
                            (False, True): (lib.ww_stream_feed_rows_all, lib.ww_stream_feed_all),
                            (True, False): (lib.ww_stream_feed_rows, lib.ww_stream_feed_bytes),
                            (True, True): (lib.ww_stream_feed_rows_all, lib.ww_stream_feed_bytes_all)}[self._g711, every]
        _lib.raise_for(rows_fn(self._h, _lib.ptr(a_ids), n, _lib.ptr(counts), _lib.ptr(row_offs)), h)
        rows = int(row_offs[n])
        post = np.empty((max(rows, 1), self.n_members) if every else max(rows, 1), np.float32)
        mel = np.empty((max(rows, 1), self.engine.n_mel), np.float32) if want_mel else None
        _lib.raise_for(feed_fn(self._h, _lib.ptr(a_ids), n, _lib.ptr(data), _lib.ptr(offs), rows, _lib.ptr(row_offs), _lib.ptr(post),
                               _lib.ptr(mel) if want_mel else None), h)
        posts = [post[row_offs[j]:row_offs[j + 1]].copy() for j in back]
        mels = [mel[row_offs[j]:row_offs[j + 1]].copy() for j in back] if want_mel else None
        return posts, mels

    def feed_all(self, ids: Sequence[int], packets: Sequence[np.ndarray], want_mel: bool = False):
        """:meth:`feed` on a causal bank that runs every listed member on every stream (``members=``; ``ww_stream_feed_all``):
        the same arguments; ``posts[i]`` is ``[rows_i, K]`` - column ``j`` is the bits :meth:`feed` yields on a causal bank of member
        ``members[j]`` alone -, ``mels`` as :meth:`feed`'s (one set of rows per stream, whatever K is).  The samples of a stream may
        be cut into ``feed_all`` packets, calls and :meth:`step` ticks in any way."""
        if not self.n_members:
            raise ValueError("feed_all: this bank was not built with members=: an ordinary causal bank takes feed")
        return self._feed(ids, packets, want_mel, True)

    def step_trigger_all(self, frames: np.ndarray, p_is_speech, p_is_active, p_thresholds, p_state) -> None:
        """The wake-word stage of an every-member bank as ONE library call (``ww_stream_step_trigger_all``); every argument but
        ``frames`` is an address taken once (``WakewordSetBank`` owns the arrays): ``p_state`` = (was_speech, posterior_max, post,
        n_post, fired_ids, fired_slot, fired_mask, n_fired, fall_ids, n_fall)."""
        if not self.n_members:
            raise ValueError("step_trigger_all: this bank was not built with members=: an ordinary bank takes step_trigger")
        rc = self._lib.ww_stream_step_trigger_all(self._h, self._frames_address(frames), p_is_speech, p_is_active, p_thresholds, *p_state)
        if rc:
            _lib.raise_for(rc, self.engine.ctx.handle)

    def close(self) -> None:
        if self._h and not _lib.is_shutdown():
            self._lib.ww_stream_destroy(self._h)
        self._h = None
        if getattr(self, "_own_resampler", False):  # (behind the bank: it borrows the tap table)
            self._resampler.close()
            self._own_resampler = False
        for r in getattr(self, "_class_rs", []):
            if r is not None:
                r.close()
        self._class_rs = []

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass


class CtcTick(NamedTuple):
    """What :meth:`CtcStreamBank.step` returns: ``labels [S, 2, max_labels]`` int32 padded with -1, ``lengths [S, 2]`` int32 (the whole
    decoded length, which may exceed ``max_labels``), ``n [S]`` the windows each stream delivered this tick (0, 1 or 2; entries at
    or past ``n[s]`` are -1 / 0 / 0), on a ``want_steps`` bank ``steps [S, 2, 19, L]``, and on a bank with ``targets``
    ``scores [S, 2, K]`` float32: the forward-algorithm score of window k of stream s for target j (``wwhip.ctc.score``)."""
    labels: np.ndarray
    lengths: np.ndarray
    n: np.ndarray
    steps: Optional[np.ndarray] = None
    scores: Optional[np.ndarray] = None
    align_values: Optional[np.ndarray] = None  # an ``align=True`` bank: [S, 2, K] float32, the best path's probability
    spans: Optional[np.ndarray] = None         # and [S, 2, K, U_max, 2] int32, its first / last step per label (wwhip.ctc.align)
    beam_labels: Optional[np.ndarray] = None   # a ``beam_width=`` bank: [S, 2, P, M] int32 padded with -1 (wwhip.ctc.beam_search)
    beam_lengths: Optional[np.ndarray] = None  # [S, 2, P] int32, -1: the path is absent
    beam_probs: Optional[np.ndarray] = None    # [S, 2, P] float32, descending


class CtcStreamBank(StreamBank):
    """S device-resident streams on one CTC-trained CRNN, advanced 20 ms per :meth:`step` (``ww_stream_create_ctc``,
    ``ww_stream_step_ctc``): per tick and stream the greedy-decoded labels of its 0, 1 or 2 new windows.

    ``max_labels`` (1..9): labels kept per window.  ``want_steps``: the bank also returns every window's ``[19, L]`` posteriors
    (``WW_STREAM_CTC_STEPS``; it then always waits for the stream).  ``two_launch`` / ``sync_wait``: :class:`StreamBank`'s, same bits in
    every form.  ``full_recompute``: a tick's windows through the offline path's kernels - the bits of :meth:`Engine.ctc_forward` on
    :meth:`window`; the incremental forms agree with it within the float32 bound of the recurrences.  ``sample_rate``,
    ``sample_format`` and ``resampler`` are :class:`StreamBank`'s.  :meth:`reset`, :meth:`window`, :meth:`set_rate`,
    :meth:`timeline`, :meth:`close` and the frame-layout attributes work as there; :meth:`feed`, :meth:`set_model` and the other
    banks' trigger stages are refused.

    ``targets`` (label tuples, at most 8 of at most 9 labels) and ``mode`` (``"exact"`` / ``"prefix"``): every tick also gives the
    windows' forward-algorithm scores, ``CtcTick.scores`` - one more small launch behind the tick's, over the posteriors, so the
    bank keeps them (``WW_STREAM_CTC_STEPS``) whether or not ``want_steps`` returns them.  :meth:`set_targets` changes them.  With ``align=True`` a tick also gives the
    windows' Viterbi alignment for the same targets and mode, ``CtcTick.align_values`` / ``CtcTick.spans`` (``wwhip.ctc.align``;
    ``ww_stream_step_ctc_align``: one launch more).

    ``beam_width`` (1..64) with ``top_paths`` (1..min(beam_width, 8)) and ``beam_max_labels`` (1..19, all 19 by default): every tick
    also gives the ``top_paths`` most probable label strings of its windows by prefix beam search, ``CtcTick.beam_labels`` /
    ``beam_lengths`` / ``beam_probs`` (``wwhip.ctc.beam_search``; ``ww_stream_step_ctc_beam``: one more small launch over the
    tick's posteriors, which the bank then keeps).  ``targets=`` together with ``beam_width=`` is not built: ``ValueError``."""
    MAX_LABELS = _lib.STREAM_CTC_MAX_LABELS

    def __init__(self, engine, n_streams: int, fp: Optional[_lib.FrontendParams] = None, max_labels: int = 2, want_steps: bool = False,
                 two_launch: bool = False, sync_wait: bool = False, full_recompute: bool = False, sample_rate=16000,
                 sample_format="pcm16", resampler=None, targets=None, mode="exact", align: bool = False, beam_width: Optional[int] = None, top_paths: int = 1,
                 beam_max_labels: Optional[int] = None) -> None:
        if beam_width is not None and targets is not None:
            raise ValueError("CtcStreamBank: targets= together with beam_width= is not built (a tick carries the scores or the beam)")
        self.beam_width = None if beam_width is None else int(beam_width)
        if self.beam_width is not None:  # (refused here, before a bank exists)
            from . import ctc
            _, self.top_paths, self.beam_max_labels = ctc._beam_args(Engine.CTC_STEPS, getattr(engine, "n_out", 2), self.beam_width, top_paths, beam_max_labels)
        if align and targets is None:
            raise ValueError("CtcStreamBank(align=True) aligns the bank's targets: give targets=")
        self.align = bool(align)
        if isinstance(engine, ModelSet) or not getattr(engine, "is_ctc", False):
            raise ValueError("CtcStreamBank runs one CTC-trained CRNN (an Engine whose is_ctc is true); StreamBank runs the other models")
        if not 1 <= int(max_labels) <= self.MAX_LABELS:
            raise ValueError(f"max_labels {max_labels} outside 1..{self.MAX_LABELS}: a streamed window carries at most {self.MAX_LABELS} labels")
        self.max_labels, self.want_steps = int(max_labels), bool(want_steps)
        self.n_targets = 0
        self._keep_steps = self.want_steps or targets is not None or self.beam_width is not None
        if targets is not None:  # (refused here, before a bank exists)
            from . import ctc
            ctc.pack_targets(targets, engine.n_out), ctc.score_mode(mode)
        super().__init__(engine, n_streams, fp, full_recompute=full_recompute, two_launch=two_launch, sync_wait=sync_wait,
                         sample_rate=sample_rate, resampler=resampler, sample_format=sample_format)
        if targets is not None:
            self.set_targets(targets, mode)

    def set_targets(self, targets, mode="exact") -> None:
        """The targets and mode of :attr:`CtcTick.scores` from the next tick on (``ww_stream_ctc_set_targets``); the bank must have
        been created with ``targets`` or ``want_steps``."""
        from . import ctc
        table, lens = ctc.pack_targets(targets, self.engine.n_out)
        _lib.raise_for(self._lib.ww_stream_ctc_set_targets(self._h, _lib.ptr(table), _lib.ptr(lens), len(lens), ctc.score_mode(mode)),
                       self.engine.ctx.handle)
        self.n_targets = len(lens)
        self.target_lens = lens.copy()
        self._scores = np.zeros((self.S, 2, self.n_targets), np.float32)
        self._p_scores = C.c_void_p(self._scores.ctypes.data)
        if self.align:
            self._umax = int(lens.max())
            self._align_values = np.zeros((self.S, 2, self.n_targets), np.float32)
            self._spans = np.full((self.S, 2, self.n_targets, _lib.CTC_SCORE_MAX_TARGET, 2), -1, np.int8)
            self._p_align_values, self._p_spans = C.c_void_p(self._align_values.ctypes.data), C.c_void_p(self._spans.ctypes.data)

    def _create(self, fp, full_recompute, two_launch, sync_wait, causal, ids) -> None:
        engine = self.engine
        self._lib = _lib.load()
        fp = fp or frontend_params()
        h = C.c_void_p()
        flags = ((_lib.STREAM_FULL_RECOMPUTE if full_recompute else 0) | (_lib.STREAM_TWO_LAUNCH if two_launch else 0)
                 | (_lib.STREAM_SYNC_WAIT if sync_wait else 0) | (_lib.STREAM_CTC_STEPS if self._keep_steps else 0))
        self.causal = False
        _lib.raise_for(self._lib.ww_stream_create_ctc(engine.ctx.handle, engine.handle, self.S, C.byref(fp), flags, C.byref(h)), engine.ctx.handle)
        self._h = h
        _lib.register("streams", self)

    def _tick_arrays(self) -> None:
        S, M = self.S, self.max_labels
        self._labels = np.full((S, 2, M), -1, np.int32)
        self._lengths = np.zeros((S, 2), np.int32)
        self._steps = np.zeros((S, 2, Engine.CTC_STEPS, self.engine.n_out), np.float32) if self.want_steps else None
        self._n = np.zeros(S, np.int32)
        self._flags = np.zeros(S, np.uint8)
        self._p_labels, self._p_lengths, self._p_n, self._p_flags = (C.c_void_p(a.ctypes.data) for a in (self._labels, self._lengths, self._n, self._flags))
        self._p_steps = C.c_void_p(self._steps.ctypes.data) if self.want_steps else None
        self._keep = None
        if self.beam_width is not None:
            P, BM = self.top_paths, self.beam_max_labels
            self._beam_labels, self._beam_lengths = np.full((S, 2, P, BM), -1, np.int32), np.full((S, 2, P), -1, np.int32)
            self._beam_probs = np.zeros((S, 2, P), np.float32)
            self._p_beam = tuple(C.c_void_p(a.ctypes.data) for a in (self._beam_labels, self._beam_lengths, self._beam_probs))

    def step(self, frames: np.ndarray, is_speech: np.ndarray, is_active: Optional[np.ndarray] = None) -> CtcTick:
        pf = self._frames_address(frames)
        sp = np.ascontiguousarray(is_speech, dtype=np.uint8).ravel()
        if sp.size != self.S:
            raise ValueError("is_speech must have one entry per stream")
        np.bitwise_and(sp, 1, out=self._flags)
        if is_active is not None:
            self._flags |= (np.ascontiguousarray(is_active, dtype=np.uint8).ravel() & 1) << 1
        self._clear()
        if self.beam_width is not None:
            rc = self._lib.ww_stream_step_ctc_beam(self._h, pf, self._p_flags, self.max_labels, self._p_labels, self._p_lengths, self._p_steps,
                                                   self.beam_width, self.top_paths, self.beam_max_labels, *self._p_beam, self._p_n)
        elif self.n_targets and self.align:
            rc = self._lib.ww_stream_step_ctc_align(self._h, pf, self._p_flags, self.max_labels, self._p_labels, self._p_lengths, self._p_steps,
                                                    self._p_scores, self._p_align_values, self._p_spans, self._p_n)
        elif self.n_targets:
            rc = self._lib.ww_stream_step_ctc_score(self._h, pf, self._p_flags, self.max_labels, self._p_labels, self._p_lengths, self._p_steps,
                                                    self._p_scores, self._p_n)
        else:
            rc = self._lib.ww_stream_step_ctc(self._h, pf, self._p_flags, self.max_labels, self._p_labels, self._p_lengths, self._p_steps, self._p_n)
        if rc:
            _lib.raise_for(rc, self.engine.ctx.handle)
        return self._tick()

    def _clear(self) -> None:
        # (the library leaves entries at or past n[s] as they were: what the caller gets there is -1 / 0 / 0, not the last tick's)
        self._labels[:] = -1
        self._lengths[:] = 0
        if self._steps is not None:
            self._steps[:] = 0.0
        if self.n_targets:
            self._scores[:] = 0.0
        if self.n_targets and self.align:
            self._align_values[:] = 0.0
            self._spans[:] = -1
        if self.beam_width is not None:
            self._beam_labels[:] = -1
            self._beam_lengths[:] = -1
            self._beam_probs[:] = 0.0

    def _tick(self) -> CtcTick:
        return CtcTick(self._labels.copy(), self._lengths.copy(), self._n.copy(), None if self._steps is None else self._steps.copy(),
                       self._scores.copy() if self.n_targets else None,
                       self._align_values.copy() if self.n_targets and self.align else None,
                       self._spans[:, :, :, :self._umax].astype(np.int32) if self.n_targets and self.align else None,
                       *((self._beam_labels.copy(), self._beam_lengths.copy(), self._beam_probs.copy()) if self.beam_width is not None else ()))

    def step_ctc_trigger(self, frames: np.ndarray, p_is_speech, p_is_active, p_target, n_target: int, p_state) -> CtcTick:
        """The wake-word stage of all streams as ONE library call (``ww_stream_step_ctc_trigger``): the tick, the label rule over
        its decodes and the reset of the streams whose VAD bit fell.  ``p_state`` = (was_speech, fired_ids, n_fired, fall_ids,
        n_fall), addresses taken once (``CtcWakewordBank`` owns the arrays)."""
        was_speech, fired, n_fired, fall, n_fall = p_state
        self._clear()
        rc = self._lib.ww_stream_step_ctc_trigger(self._h, self._frames_address(frames), p_is_speech, p_is_active, self.max_labels, p_target,
                                                  int(n_target), was_speech, self._p_labels, self._p_lengths, self._p_steps, self._p_n,
                                                  fired, n_fired, fall, n_fall)
        if rc:
            _lib.raise_for(rc, self.engine.ctx.handle)
        return self._tick()

    def _refuse(self, what: str):
        raise ValueError(f"{what}: this bank runs a CTC-trained CRNN: it has step, step_ctc_trigger, reset, window, set_rate and timeline")

    def step_trigger(self, *a, **k):
        self._refuse("step_trigger")

    def step_trigger_all(self, *a, **k):
        self._refuse("step_trigger_all")

    def feed(self, *a, **k):
        self._refuse("feed")

    def feed_all(self, *a, **k):
        self._refuse("feed_all")

    def set_model(self, *a, **k):
        self._refuse("set_model")
