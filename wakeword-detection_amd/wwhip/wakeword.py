"""Streaming wake-word stage with the surface of the reference's ``WakewordTrigger``
(``spokestack/wakeword/tflite.py:20-250``).  Per 20 ms frame the reference normalises,
pre-emphasises, pushes 320 samples through a Python ring, and for every completed STFT frame
(while ``context.is_speech``) runs filter -> slide window -> encode -> detect.  Here all of
that state lives on the GPU in a one-stream :class:`StreamBank`; this class keeps only the
host logic: VAD-edge reset, activation, running maximum.

:class:`WakewordBank` is the many-stream form used by BASELINE config 5.
"""
from __future__ import annotations

import logging
from typing import Callable, Optional, Sequence, Tuple

import numpy as np

from . import ctc
from .context import SpeechContext
from .engine import StreamBank, frontend_params
from .models import engine_for

_LOG = logging.getLogger(__name__)


class WakewordTrigger:
    def __init__(self, pre_emphasis: float = 0.0, sample_rate: int = 16000, fft_window_type: str = "hann",
                 fft_hop_length: int = 10, model_dir: str = "", model_type: str = "",
                 posterior_threshold: float = 0.5, on_wake: Optional[Callable[[], None]] = None, device: int = 0,
                 superframe_len: int = 0, causal: bool = False, **kwargs) -> None:
        # causal (fp32 Wavenet only): the posteriors come from the sequence form advanced row by row (StreamBank(causal=True))
        # instead of from a window recomputed per row; the trigger logic below is the same
        self.pre_emphasis = pre_emphasis
        self.hop_length = int(fft_hop_length * sample_rate / 1000)
        if fft_window_type != "hann":
            raise ValueError("Invalid fft_window_type")
        self.model_type = model_type.upper()
        if self.model_type not in ("CRNN", "WAVENET"):
            # the reference fails later with AttributeError; fail early instead
            raise ValueError(f"model_type must be 'CRNN' or 'Wavenet', got {model_type!r}")
        self._engine = engine_for(model_dir, device)
        if self._engine.is_crnn != (self.model_type == "CRNN"):
            raise ValueError(f"model_dir holds a {'CRNN' if self._engine.is_crnn else 'Wavenet'} model, "
                             f"model_type says {model_type}")
        self._window_size = (self._engine.n_bins - 1) * 2
        self.mel_length = self._engine.window
        self.mel_width = self._engine.n_mel
        self.encode_length, self.encode_width = self._engine.enc_shape
        self._bank = StreamBank(self._engine, 1, frontend_params(32767.0, True, pre_emphasis, self.hop_length, True), causal=causal)
        self._posterior_threshold = posterior_threshold
        self._posterior_max = 0.0
        self._is_speech = False
        self._on_wake = on_wake  # replaces the pydub audio reply (tflite.py:111-121,238)
        # superframe_len > 0 selects the experimental trigger of utils/CRNN_files/tflite.py:252-263
        # (shortest path over a superframe of posteriors instead of the 0.5 threshold)
        from .wfst import SuperframeDetector
        self._superframe = SuperframeDetector(superframe_len) if superframe_len > 0 else None

    def __call__(self, context: SpeechContext, frame) -> None:
        vad_fall = self._is_speech and not context.is_speech
        self._is_speech = context.is_speech
        if not context.is_active:
            self._sample(context, frame)
        if vad_fall:
            if not context.is_active:
                _LOG.info(f"wake: {self._posterior_max}")
            self.reset()

    def _sample(self, context: SpeechContext, frame) -> None:
        f = np.asarray(frame, dtype=np.int16).reshape(1, -1)
        if f.shape[1] != 320:
            raise ValueError("WakewordTrigger expects 20 ms frames of 320 int16 samples")
        post, n = self._bank.step(f, np.array([1 if context.is_speech else 0], np.uint8))
        for k in range(int(n[0])):
            posterior = float(post[0, k])
            if posterior > self._posterior_max:
                self._posterior_max = posterior
            if self._superframe is not None:
                fire = self._superframe.push(posterior)
            else:
                fire = posterior > self._posterior_threshold
            if fire and not context.is_active:
                _LOG.info(f"AWAKE!: {self._posterior_max}")
                if self._on_wake is not None:
                    self._on_wake()
                context.is_active = True

    def reset(self) -> None:
        self._bank.reset()
        self._posterior_max = 0.0
        if self._superframe is not None:
            self._superframe.reset()

    def close(self) -> None:
        self.reset()


def _flag_addresses(stage, contexts):
    """The addresses of the ``is_speech`` and ``is_active`` arrays a banked stage's tick reads and writes: a ``ContextBank``'s own
    (taken once per bank: its arrays are the state), or the stage's scratch arrays filled from a sequence of S ``SpeechContext``
    objects (the slow form)."""
    from . import _lib
    if hasattr(contexts, "emit"):
        b = stage._bound
        if b is None or b[0] is not contexts:
            if len(contexts) != stage.S:
                raise ValueError("one context per stream")
            b = stage._bound = (contexts, _lib.addr(contexts.is_speech), _lib.addr(contexts.is_active))
        return b[1], b[2]
    if len(contexts) != stage.S:
        raise ValueError("one context per stream")
    sc = stage._scratch
    if sc is None:
        speech, active = np.zeros(stage.S, np.uint8), np.zeros(stage.S, np.uint8)
        sc = stage._scratch = (speech, active, _lib.addr(speech), _lib.addr(active))
    sc[0][:] = [c.is_speech for c in contexts]
    sc[1][:] = [c.is_active for c in contexts]
    return sc[2], sc[3]


def _activate(contexts, ids) -> None:
    """The streams that fired: one ``activate`` event on a ``ContextBank`` (the tick has set its flags), else each context's flag."""
    if hasattr(contexts, "emit"):
        contexts.emit("activate", ids)
    else:
        for s in ids:
            contexts[int(s)].is_active = True  # (the setter raises the activate event)


class WakewordBank:
    """S streams in lock step: the batched form of :class:`WakewordTrigger` - one kernel launch per 20 ms tick for all streams,
    and the trigger's host logic (VAD-edge reset, running maximum, threshold, activation; tflite.py:134-146,232-239) as one pass
    over arrays inside the same library call (``ww_stream_step_trigger``).

    ``contexts`` is a :class:`~wwhip.context.ContextBank` - the stage then reads and writes the bank's flag arrays in place and
    raises ``activate`` events for the streams that fired, no per-stream Python otherwise - or, as before, a sequence of S
    ``SpeechContext`` objects (their flags are gathered and written back one by one: the slow form).  ``frames`` is what the
    bank's :meth:`~wwhip.engine.StreamBank.step` takes and is passed through unchanged: ``[S, frame_samples]``, or for a bank with
    per-stream rates the flat ragged block (or the S per-stream arrays)."""

    def __init__(self, n_streams: int, model_dir: str = "", posterior_threshold: float = 0.5, pre_emphasis: float = 0.0,
                 device: int = 0, on_wake: Optional[Callable[[np.ndarray], None]] = None, bank=None, causal: bool = False) -> None:
        # causal: the bank this stage builds is StreamBank(causal=True) (fp32 Wavenet only); a bank= of the caller's is taken as it is
        from . import _lib
        self.S = int(n_streams)
        if bank is None:
            if not model_dir:
                raise ValueError("WakewordBank needs model_dir (or bank=: a StreamBank built on an Engine of the caller's)")
            self._engine = engine_for(model_dir, device)
            bank = StreamBank(self._engine, self.S, frontend_params(32767.0, True, pre_emphasis, 160, True), causal=causal)
        elif getattr(bank, "n_members", 0):
            raise ValueError("WakewordBank: this bank runs every listed member on every stream (members=): the trigger stage has one "
                             "posterior per stream and cannot say which wake word fired")
        self._bank = bank  # (anything with StreamBank's step_trigger / reset / close: the host-only tests pass a stub)
        self.threshold = float(posterior_threshold)
        self._on_wake = on_wake  # called with the ids of the streams that woke up this tick
        self.posterior_max = np.zeros(self.S, np.float32)
        self._was_speech = np.zeros(self.S, np.uint8)
        self._post = np.zeros((self.S, 2), np.float32)
        self._n = np.zeros(self.S, np.int32)
        self._fired = np.zeros(self.S, np.int32)
        self._fall = np.zeros(self.S, np.int32)
        self._counts = np.zeros(2, np.int32)
        self._p_state = (_lib.addr(self._was_speech), _lib.addr(self.posterior_max), _lib.addr(self._post), _lib.addr(self._n),
                         _lib.addr(self._fired), _lib.addr(self._counts[0:1]), _lib.addr(self._fall), _lib.addr(self._counts[1:2]))
        self._bound = None     # (the ContextBank, the addresses of its two flag arrays)
        self._scratch = None   # flag arrays for the sequence-of-contexts form

    @property
    def n_post(self) -> np.ndarray:
        """Posteriors per stream delivered by the last tick (0, 1 or 2)."""
        return self._n

    def step(self, contexts, frames: np.ndarray) -> np.ndarray:
        p_speech, p_active = _flag_addresses(self, contexts)
        self._bank.step_trigger(frames, p_speech, p_active, self.threshold, self._p_state)
        nf = self._counts[0]
        if nf:
            ids = self._fired[:nf].copy()
            if self._on_wake is not None:
                self._on_wake(ids)
            _activate(contexts, ids)
        return self._post.copy()

    __call__ = step  # the stage form: bank(contexts, frames)

    def reset(self) -> None:
        self._bank.reset()
        self.posterior_max[:] = 0.0

    def close(self) -> None:
        self._bank.close()


class WakewordSetBank:
    """The wake-word stage of S streams that listen for SEVERAL wake words at once: an every-member
    :class:`~wwhip.engine.StreamBank` (``StreamBank(model_set, S, members=...)``: one front end per stream, K member slots) and
    :class:`WakewordBank`'s host logic with K slots per stream, inside one library call per tick
    (``ww_stream_step_trigger_all``).  The rule (tflite.py:134-146,232-239 per stream): a running maximum per slot, cleared for all
    slots on the VAD falling edge; slot ``j`` exceeds when its posterior is above ``thresholds[j]``; a stream that is not active fires
    when any slot exceeds - ``activate`` is raised once per stream, as the reference's context has one flag - and the stage says which
    wake word it was: :attr:`wake_slot` ``[S]`` (int32; -1 until a stream first fires, then its last winner: on the earliest row on
    which any slot exceeded, the exceeding slot with the greatest posterior, the lowest among equals), :attr:`wake_mask` ``[S]``
    (uint64; bit ``j``: slot ``j`` exceeded in the tick of the stream's last fire) and :attr:`posterior_max` ``[S, K]``.

    ``thresholds``: one value for every slot, or one per slot.  ``names``: one name per slot, for :meth:`wake_word`.  ``bank=``: an
    every-member bank of the caller's (``model_set`` / ``members`` / ``pre_emphasis`` / ``causal`` are then not looked at).
    ``on_wake(ids, slots)`` is called with the streams that fired this tick and their winning slots.  ``contexts`` and ``frames``
    of :meth:`step` are :meth:`WakewordBank.step`'s; it returns the tick's posteriors ``[S, K, 2]``."""

    def __init__(self, n_streams: int, model_set=None, members="all", thresholds=0.5, names: Optional[Sequence[str]] = None, bank=None,
                 pre_emphasis: float = 0.0, causal: bool = False, on_wake: Optional[Callable[[np.ndarray, np.ndarray], None]] = None) -> None:
        self.S = int(n_streams)
        if bank is None:
            if model_set is None:
                raise ValueError("WakewordSetBank needs model_set (a ModelSet), or bank=: a StreamBank built with members=")
            bank = StreamBank(model_set, self.S, frontend_params(32767.0, True, pre_emphasis, 160, True), causal=causal, members=members)
            owned = True
        else:
            owned = False
            if not getattr(bank, "n_members", 0):
                raise ValueError("WakewordSetBank: this bank was not built with members= (one model per stream): its stage is WakewordBank")
            if getattr(bank, "S", self.S) != self.S:
                raise ValueError(f"WakewordSetBank: the bank has {bank.S} streams, the stage {self.S}")
        self._bank = bank  # (anything with StreamBank's n_members / step_trigger_all / reset / close: the host-only tests pass a stub)
        self.K = K = int(bank.n_members)
        try:
            th = np.asarray(thresholds, np.float64)
            if th.ndim == 0:
                th = np.full(K, float(th))
            if th.ndim != 1 or th.size != K:
                raise ValueError(f"thresholds: one value, or one per member slot ({K}), got {np.shape(thresholds)}")
            if names is not None and len(names) != K:
                raise ValueError(f"names: one per member slot ({K}), got {len(names)}")
        except ValueError:
            if owned:
                bank.close()
            raise
        from . import _lib
        self.thresholds = np.ascontiguousarray(th)
        self.names = None if names is None else [str(x) for x in names]
        self._on_wake = on_wake
        self.posterior_max = np.zeros((self.S, K), np.float32)
        self.wake_slot = np.full(self.S, -1, np.int32)
        self.wake_mask = np.zeros(self.S, np.uint64)
        self._was_speech = np.zeros(self.S, np.uint8)
        self._post = np.zeros((self.S, K, 2), np.float32)
        self._n = np.zeros(self.S, np.int32)
        self._fired = np.zeros(self.S, np.int32)
        self._fired_slot = np.zeros(self.S, np.int32)
        self._fired_mask = np.zeros(self.S, np.uint64)
        self._fall = np.zeros(self.S, np.int32)
        self._counts = np.zeros(2, np.int32)
        a = _lib.addr
        self._p_thresholds = a(self.thresholds)
        self._p_state = (a(self._was_speech), a(self.posterior_max), a(self._post), a(self._n), a(self._fired), a(self._fired_slot),
                         a(self._fired_mask), a(self._counts[0:1]), a(self._fall), a(self._counts[1:2]))
        self._bound = None     # (the ContextBank, the addresses of its two flag arrays)
        self._scratch = None   # flag arrays for the sequence-of-contexts form

    @property
    def n_members(self) -> int:
        return self.K

    @property
    def n_post(self) -> np.ndarray:
        """Posteriors per stream and slot delivered by the last tick (0, 1 or 2)."""
        return self._n

    @property
    def fall_ids(self) -> np.ndarray:
        """The streams whose VAD bit fell in the last tick (they were reset)."""
        return self._fall[:self._counts[1]].copy()

    def wake_word(self, stream: int) -> Optional[str]:
        """The name of the wake word stream ``stream`` last woke to; ``None`` before its first fire."""
        if self.names is None:
            raise ValueError("wake_word: the stage was built without names=")
        j = int(self.wake_slot[int(stream)])
        return None if j < 0 else self.names[j]

    def _fires(self):
        nf = self._counts[0]
        if not nf:
            return None
        ids, slots = self._fired[:nf].copy(), self._fired_slot[:nf].copy()
        self.wake_slot[ids] = slots
        self.wake_mask[ids] = self._fired_mask[:nf]
        if self._on_wake is not None:
            self._on_wake(ids, slots)
        return ids

    def step(self, contexts, frames: np.ndarray) -> np.ndarray:
        p_speech, p_active = _flag_addresses(self, contexts)
        self._bank.step_trigger_all(frames, p_speech, p_active, self._p_thresholds, self._p_state)
        ids = self._fires()
        if ids is not None:
            _activate(contexts, ids)
        return self._post.copy()

    __call__ = step  # the stage form: bank(contexts, frames)

    def reset(self) -> None:
        self._bank.reset()
        self.posterior_max[:] = 0.0

    def close(self) -> None:
        self._bank.close()


class CtcWakewordBank:
    """The wake-word stage of S streams on a CTC-trained CRNN: a :class:`~wwhip.engine.CtcStreamBank` and the trigger's host logic
    inside one library call per tick (``ww_stream_step_ctc_trigger``).  :class:`WakewordBank`'s bookkeeping - the VAD edge, the
    reset of the streams whose speech bit fell, ``activate`` once per stream - with another firing rule: a stream that is not active
    fires on the first window of the tick whose decode starts with ``target`` (``wwhip.ctc.is_wakeword``; the reference's
    ``eval_CTC`` with ``[HEY][SNIPS]``).

    ``engine``: an :class:`~wwhip.engine.Engine` on a CTC-trained CRNN, from which the stage builds its bank; or ``bank=``: a
    ``CtcStreamBank`` of the caller's (``engine`` / ``pre_emphasis`` are then not looked at), whose ``max_labels`` must reach
    ``len(target)``.  ``on_wake(ids)`` is called with the streams that fired this tick.  ``contexts`` and ``frames`` of :meth:`step`
    are :meth:`WakewordBank.step`'s; it returns the tick (:class:`~wwhip.engine.CtcTick`).

    ``thresholds`` (one per target of the bank; a number for one target): the SCORE rule instead - a stream that is not active fires
    on the first window of the tick whose forward-algorithm score (``wwhip.ctc.score``, ``CtcTick.scores``) for some target ``j``
    exceeds ``thresholds[j]``, :class:`WakewordSetBank`'s comparison (``ww_ctc_score_trigger_bank_step``); :attr:`fired_slots` names
    the target.  The stage's own bank then scores ``targets`` (default: ``target`` alone) in ``mode``; a ``bank=`` of the caller's
    must have been created with targets, as many as there are thresholds.

    ``align=True`` (with the score rule): the bank also aligns its targets (``CtcStreamBank(align=True)``, ``CtcTick.spans``), and on
    a fire the stage records WHERE the word lies: :meth:`wake_span_rows`."""

    def __init__(self, n_streams: int, engine=None, target: Sequence[int] = ctc.WAKEWORD, bank=None, pre_emphasis: float = 0.0,
                 on_wake: Optional[Callable[[np.ndarray], None]] = None, thresholds=None, targets=None, mode: str = "prefix",
                 align: bool = False) -> None:
        from . import _lib
        from .engine import CtcStreamBank
        self.S = int(n_streams)
        self.thresholds = None
        self.align = bool(align)
        if self.align and thresholds is None:
            raise ValueError("CtcWakewordBank(align=True) records the span of the target whose score fired: it needs thresholds=")
        if thresholds is not None:
            self._init_score_rule(engine, bank, pre_emphasis, on_wake, thresholds, targets if targets is not None else [tuple(target)], mode)
            return
        t = np.asarray(target)
        if t.ndim != 1 or t.size < 1 or t.dtype.kind not in "iu" or t.min() < 0 or t.max() > 7:
            raise ValueError("target must be a non-empty sequence of labels 0..7")
        if t.size > _lib.STREAM_CTC_MAX_LABELS:
            raise ValueError(f"target has {t.size} labels: a streamed window carries at most {_lib.STREAM_CTC_MAX_LABELS}")
        if bank is None:
            if engine is None:
                raise ValueError("CtcWakewordBank needs engine (an Engine on a CTC-trained CRNN), or bank=: a CtcStreamBank")
            bank = CtcStreamBank(engine, self.S, frontend_params(32767.0, True, pre_emphasis, 160, True), max_labels=max(2, int(t.size)))
        else:
            if not hasattr(bank, "step_ctc_trigger"):
                raise ValueError("CtcWakewordBank: this bank does not decode labels (a StreamBank): its stage is WakewordBank")
            if getattr(bank, "S", self.S) != self.S:
                raise ValueError(f"CtcWakewordBank: the bank has {bank.S} streams, the stage {self.S}")
            if int(bank.max_labels) < t.size:
                raise ValueError(f"CtcWakewordBank: the bank keeps {bank.max_labels} labels per window, the target has {t.size}")
        self._bank = bank  # (anything with CtcStreamBank's max_labels / step_ctc_trigger / reset / close: the host-only tests pass a stub)
        self.target = np.ascontiguousarray(t, np.int32)
        self._on_wake = on_wake
        self._was_speech = np.zeros(self.S, np.uint8)
        self._fired = np.zeros(self.S, np.int32)
        self._fall = np.zeros(self.S, np.int32)
        self._counts = np.zeros(2, np.int32)
        self._n = np.zeros(self.S, np.int32)
        a = _lib.addr
        self._p_target = a(self.target)
        self._p_state = (a(self._was_speech), a(self._fired), a(self._counts[0:1]), a(self._fall), a(self._counts[1:2]))
        self._bound = None     # (the ContextBank, the addresses of its two flag arrays)
        self._scratch = None   # flag arrays for the sequence-of-contexts form

    def _init_score_rule(self, engine, bank, pre_emphasis, on_wake, thresholds, targets, mode) -> None:
        from . import _lib
        from .engine import CtcStreamBank
        thr = np.atleast_1d(np.asarray(thresholds, np.float64))
        if thr.ndim != 1 or not np.all(np.isfinite(thr)):
            raise ValueError("thresholds must be finite numbers, one per target")
        if bank is None:
            if engine is None:
                raise ValueError("CtcWakewordBank needs engine (an Engine on a CTC-trained CRNN), or bank=: a CtcStreamBank")
            if len(targets) != thr.size:
                raise ValueError(f"CtcWakewordBank: {thr.size} thresholds for {len(targets)} targets")
            bank = CtcStreamBank(engine, self.S, frontend_params(32767.0, True, pre_emphasis, 160, True), targets=targets, mode=mode,
                                 align=self.align)
        else:
            if getattr(bank, "S", self.S) != self.S:
                raise ValueError(f"CtcWakewordBank: the bank has {bank.S} streams, the stage {self.S}")
            if self.align and not getattr(bank, "align", False):
                raise ValueError("CtcWakewordBank(align=True): the bank does not align its targets (CtcStreamBank(..., align=True))")
            if int(getattr(bank, "n_targets", 0)) != thr.size:
                raise ValueError(f"CtcWakewordBank: {thr.size} thresholds, but the bank scores {getattr(bank, 'n_targets', 0)} targets "
                                 "(CtcStreamBank(..., targets=))")
        self._bank = bank
        self.thresholds = np.ascontiguousarray(thr)
        self._on_wake = on_wake
        self._was_speech = np.zeros(self.S, np.uint8)
        self._fired = np.zeros(self.S, np.int32)
        self._fired_slot = np.zeros(self.S, np.int32)
        self._fall = np.zeros(self.S, np.int32)
        self._counts = np.zeros(2, np.int32)
        self._n = np.zeros(self.S, np.int32)
        self._lib = _lib.load()
        self._bound = None
        self._scratch = None
        # align=True: the windows a stream has delivered since its last reset, and the rows of the word on its last fire
        self._seen = np.zeros(self.S, np.int64)
        self._wake_rows = np.full((self.S, 2), -1, np.int64)

    def _record_spans(self, tick) -> None:
        """On a fire: the fired target's span on the window that fired, as rows of the stream (:meth:`wake_span_rows`)."""
        for s, j in zip(self._fired[:self._counts[0]], self._fired_slot[:self._counts[0]]):
            over = (tick.scores[s, :tick.n[s]].astype(np.float64) > self.thresholds).any(axis=1)
            k = int(np.argmax(over))  # the first window of the tick on which a threshold was exceeded
            sp, U = tick.spans[s, k, j], int(self._bank.target_lens[j])
            self._wake_rows[s] = ctc.span_rows([sp[0, 0], sp[U - 1, 1]], int(self._seen[s]) + k - (ctc.WINDOW_ROWS - 1))

    def wake_span_rows(self, s: int) -> Tuple[int, int]:
        """``align=True``: where the word lay when stream ``s`` last fired - the first mel row of the fired target's first label and
        the last row of its last label (``wwhip.ctc.span_rows`` over the fired window's span).  Rows are the stream's own: row ``r``
        is the newest row of the ``r``-th window (0-based) the stream has delivered since its last reset, so the fired window covers
        rows ``r - 150 .. r`` and a row below 0 lies in the silence in front of the stream.  ``(-1, -1)``: the stream has not fired,
        or the fired target had no path in the bank's mode (its alignment value was 0)."""
        if not self.align:
            raise ValueError("wake_span_rows belongs to a stage created with align=True")
        return int(self._wake_rows[s, 0]), int(self._wake_rows[s, 1])

    def _step_scores(self, contexts, frames):
        from . import _lib
        p_speech, p_active = _flag_addresses(self, contexts)
        S = self.S
        speech, active = (contexts.is_speech, contexts.is_active) if hasattr(contexts, "emit") else self._scratch[:2]
        tick = self._bank.step(frames, speech, active)
        n, scores = np.ascontiguousarray(tick.n, np.int32), np.ascontiguousarray(tick.scores, np.float32)
        rc = self._lib.ww_ctc_score_trigger_bank_step(S, int(self.thresholds.size), p_speech, p_active, _lib.ptr(scores), _lib.ptr(n),
                                                      _lib.ptr(self.thresholds), _lib.ptr(self._was_speech), _lib.ptr(self._fired),
                                                      _lib.ptr(self._fired_slot), _lib.ptr(self._counts[0:1]), _lib.ptr(self._fall),
                                                      _lib.ptr(self._counts[1:2]))
        if rc:
            raise ValueError("ww_ctc_score_trigger_bank_step refused its arguments")
        if self.align:
            self._record_spans(tick)
            self._seen += n
            self._seen[self._fall[:self._counts[1]]] = 0
        if self._counts[1]:
            self._bank.reset(self._fall[:self._counts[1]].copy())
        return tick

    @property
    def n_post(self) -> np.ndarray:
        """Windows per stream delivered by the last tick (0, 1 or 2)."""
        return self._n

    @property
    def fired_ids(self) -> np.ndarray:
        """The streams that fired in the last tick."""
        return self._fired[:self._counts[0]].copy()

    @property
    def fired_slots(self) -> np.ndarray:
        """Score rule: for each of :attr:`fired_ids` the target whose threshold was exceeded (the greatest score among several)."""
        if self.thresholds is None:
            raise ValueError("fired_slots belongs to the score rule (thresholds=)")
        return self._fired_slot[:self._counts[0]].copy()

    @property
    def fall_ids(self) -> np.ndarray:
        """The streams whose VAD bit fell in the last tick (they were reset)."""
        return self._fall[:self._counts[1]].copy()

    def step(self, contexts, frames: np.ndarray):
        if self.thresholds is not None:
            tick = self._step_scores(contexts, frames)
        else:
            p_speech, p_active = _flag_addresses(self, contexts)
            tick = self._bank.step_ctc_trigger(frames, p_speech, p_active, self._p_target, int(self.target.size), self._p_state)
        self._n = tick.n
        nf = self._counts[0]
        if nf:
            ids = self._fired[:nf].copy()
            if self._on_wake is not None:
                self._on_wake(ids)
            _activate(contexts, ids)
        return tick

    __call__ = step  # the stage form: bank(contexts, frames)

    def reset(self) -> None:
        self._bank.reset()
        if self.thresholds is not None:
            self._seen[:] = 0

    def close(self) -> None:
        self._bank.close()
