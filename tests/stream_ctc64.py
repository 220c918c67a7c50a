"""The script the CTC stream-bank tests play (tests/test_stream_ctc_host.py, tests/test_gpu_stream_ctc.py) and its float64 statement.
Host only: NumPy, ``ctc64`` (the models of ``ctc64.model(L)`` and ``Ctc64``), ``oracle.ref64`` (the float64 front end) and ``wwhip.ctc``.

170 ticks of 320 samples for S = 3 streams: 340 mel rows on stream 0, which wraps the 144-slot cache of projected rows twice and
passes the 151-row fill of the window.  Seeded int16 noise whose level moves from tick to tick (a seeded gain per stream and tick:
windows over plain stationary noise all read alike).  The speech mask: stream 0 always on but for the two ticks on which the whole
bank is silent; stream 1 toggles; stream 2 is frozen by the active bit for 20 ticks.  ``reset([1])`` in front of tick 90.

The float64 statement of a tick: the rows a stream has delivered since its last reset (``ref64``'s float64 front end over the frames the
reference's framing rule cuts: one whenever 512 samples are buffered, then the oldest 160 dropped; a frame is analysed only while
the speech bit is set, and not sampled at all while the active bit is), ``ref64.stream_windows`` over them, ``Ctc64.sequence``,
``ctc.greedy_decode``.
"""
from __future__ import annotations

import numpy as np

import ctc64
from oracle import ref64 as R

TICKS, S, CHUNK, T = 170, 3, 320, 151
SEED = 4107
RESET_TICK, RESET_IDS = 90, (1,)
SILENT = (60, 61)                 # the whole bank's speech bits are 0
FROZEN = (2, 100, 120)            # stream 2's active bit is set on ticks 100..119
STAGE_RELEASE = (75, 140)         # the stage test clears every is_active flag in front of these ticks (an active stream is frozen)


def pcm() -> np.ndarray:
    """``[TICKS, S, 320]`` int16."""
    rng = np.random.default_rng(SEED)
    gain = 10.0 ** rng.uniform(1.5, 4.0, (TICKS, S, 1))
    gain = np.where(rng.random((TICKS, S, 1)) < 0.15, 1.0, gain)   # (some near-silent ticks)
    return np.clip(rng.normal(0.0, 1.0, (TICKS, S, CHUNK)) * gain, -32768, 32767).astype(np.int16)


def speech() -> np.ndarray:
    """``[TICKS, S]`` uint8."""
    m = np.ones((TICKS, S), np.uint8)
    t = np.arange(TICKS)
    m[:, 1] = ~(((t >= 40) & (t < 50)) | ((t >= 130) & (t < 135)) | (t == 151))
    m[list(SILENT), :] = 0
    return m


def active() -> np.ndarray:
    """``[TICKS, S]`` uint8."""
    a = np.zeros((TICKS, S), np.uint8)
    a[FROZEN[1]:FROZEN[2], FROZEN[0]] = 1
    return a


def sampled(t: int) -> bool:
    return t % 5 == 0 or 70 <= t <= 78


class Stream64:
    """One stream's framing and float64 mel rows: ``tick(samples, speech, active)`` -> the rows the tick delivers (0, 1 or 2)."""

    def __init__(self, filt) -> None:
        self.filt = filt
        self.pend = np.zeros(0, np.float32)
        self.rows = np.zeros((0, 40), np.float64)   # since the last reset

    def reset(self) -> None:
        self.pend = np.zeros(0, np.float32)
        self.rows = np.zeros((0, 40), np.float64)

    def tick(self, samples: np.ndarray, sp: int, act: int) -> int:
        if act:
            return 0
        self.pend = np.concatenate([self.pend, R.quantise(samples)])
        n = 0
        while len(self.pend) >= R.WIN:
            if sp:
                self.rows = np.concatenate([self.rows, R.logmel64_samples(self.filt, self.pend[:R.WIN], R.WIN).y])
                n += 1
            self.pend = self.pend[160:]
        return n

    def window(self, back: int = 0) -> np.ndarray:
        """The ``[151, 40]`` window that ends at the newest row (``back`` = 1: at the one before it)."""
        return R.stream_windows(self.rows, T)[len(self.rows) - 1 - back]


_cache: dict = {}


def play():
    """``(n [TICKS, S], windows {(t, s, k): [151, 40] float64})`` of every window of every tick (k = 0, 1 in the tick's order), once
    per process."""
    if "play" not in _cache:
        filt = ctc64.model(4).filt   # (the three models share one filter)
        x, sp, act = pcm(), speech(), active()
        st = [Stream64(filt) for _ in range(S)]
        n = np.zeros((TICKS, S), np.int32)
        wins = {}
        for t in range(TICKS):
            if t == RESET_TICK:
                for s in RESET_IDS:
                    st[s].reset()
            for s in range(S):
                n[t, s] = st[s].tick(x[t, s], int(sp[t, s]), int(act[t, s]))
                for k in range(n[t, s]):
                    wins[(t, s, k)] = st[s].window(n[t, s] - 1 - k)
        _cache["play"] = (n, wins)
    return _cache["play"]


def sample_keys():
    """The (t, s, k) the GPU test samples: at every 5th tick and at ticks 70..78 the newest window of each stream that delivered one."""
    n, _ = play()
    return [(t, s, int(n[t, s]) - 1) for t in range(TICKS) if sampled(t) for s in range(S) if n[t, s]]


def reference(L: int, keys=None):
    """``(keys, steps64 [len(keys), 19, L])`` of the L-class model over the float64 windows of ``keys`` (default: ``sample_keys()``)."""
    tag = (L, None if keys is None else tuple(keys))
    if tag not in _cache:
        _, wins = play()
        ks = sample_keys() if keys is None else list(keys)
        steps, _ = ctc64.Ctc64(ctc64.model(L).crnn).sequence(np.stack([wins[k] for k in ks]))
        steps.setflags(write=False)
        _cache[tag] = (ks, steps)
    return _cache[tag]


def target(L: int):
    """The stage test's target: the first two labels of the first sampled reference window that decodes to two or more."""
    _, steps = reference(L)
    labels, lengths = ctc64.decode64(steps, 2)
    i = int(np.flatnonzero(lengths >= 2)[0])
    return tuple(int(c) for c in labels[i])


def stage64(L: int, tgt):
    """The stage test's 170 ticks in float64: ``CtcWakewordBank``'s rule over the float64 decodes - a stream's flags are its speech bit
    and its own is_active (set when it fires, cleared for every stream in front of the ticks of ``STAGE_RELEASE``); an active stream is
    not sampled; a stream whose speech bit fell is reset behind the tick.  Returns ``[(tick, [fired ids])]``."""
    from wwhip import ctc
    model = ctc64.Ctc64(ctc64.model(L).crnn)
    filt = ctc64.model(L).filt
    x, sp = pcm(), speech()
    st = [Stream64(filt) for _ in range(S)]
    is_active, was = [0] * S, [0] * S
    out = []
    for t in range(TICKS):
        if t in STAGE_RELEASE:
            is_active = [0] * S
        fired = []
        for s in range(S):
            n = st[s].tick(x[t, s], int(sp[t, s]), is_active[s])
            hit = False
            if n:
                steps, _ = model.sequence(np.stack([st[s].window(n - 1 - k) for k in range(n)]))
                labels, lengths = ctc.greedy_decode(steps, len(tgt))
                hit = bool(ctc.is_wakeword(labels, lengths, tgt).any())
            if hit and not is_active[s]:
                is_active[s] = 1
                fired.append(s)
            if was[s] and not sp[t, s]:
                st[s].reset()
            was[s] = int(sp[t, s])
        if fired:
            out.append((t, fired))
    return out
