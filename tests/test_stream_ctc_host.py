"""CTC stream banks without a GPU: the conditions tests/test_gpu_stream_ctc.py relies on, asserted on the float64 reference alone
(tests/stream_ctc64.py: ``ref64``'s float64 front end over the script's PCM, ``Ctc64``, ``ctc.greedy_decode``); csrc/stream_ctc.h as a
stand-alone program under Address + UB sanitizer (tests/native/stream_ctc_check.cpp, run as a child process: nothing is loaded into
this interpreter); and the refusals and argument checks of ``CtcStreamBank`` / ``CtcWakewordBank`` against a stub bank."""
import os
import re
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CSRC = os.path.join(_ROOT, "wakeword-detection_amd", "csrc")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctc64  # noqa: E402
import stream_ctc64 as SC  # noqa: E402


# ---- the script, in float64 ---------------------------------------------------------------------------------------------------------
def test_the_script_wraps_the_cache_and_fills_the_window():
    n, wins = SC.play()
    sp, act = SC.speech(), SC.active()
    assert n.shape == (SC.TICKS, SC.S) and n.min() == 0 and n.max() == 2
    assert n[:, 0].sum() > 2 * 144 and n[:, 0].sum() > 151          # the 144-slot cache twice, the 151-row fill
    assert (sp.sum(axis=1) == 0).sum() == 2 and (n[list(SC.SILENT)] == 0).all()   # two whole-bank silent ticks
    assert (sp[:, 0] == 0).sum() == 2 and 0 < (sp[:, 1] == 0).sum() < SC.TICKS // 2
    s, a, b = SC.FROZEN
    assert b - a == 20 and (n[a:b, s] == 0).all() and act.sum() == 20
    assert sum(1 for (t, _, _) in wins if t == SC.RESET_TICK) > 0    # the reset tick delivers windows, of a stream that starts afresh
    t0 = min(t for t in range(SC.RESET_TICK, SC.TICKS) if n[t, 1])
    assert not wins[(t0, 1, 0)][:-1].any() and wins[(t0, 1, 0)][-1].any()


@pytest.mark.parametrize("L", ctc64.LS)
def test_sampled_windows_are_decidable_and_varied(L):
    keys, steps = SC.reference(L)
    assert len(keys) > 80 and steps.shape == (len(keys), 19, L)
    dec = ctc64.decidable(steps)
    assert (~dec).sum() <= 0.05 * len(keys), (L, int((~dec).sum()), len(keys))
    _, lengths = ctc64.decode64(steps, 9)
    assert (lengths == 0).any() and (lengths >= 2).any(), np.bincount(lengths)


@pytest.mark.parametrize("L", ctc64.LS)
def test_the_stage_fires_on_two_streams_in_float64(L):
    tgt = SC.target(L)
    assert len(tgt) == 2
    fires = SC.stage64(L, tgt)
    streams = {s for _, ids in fires for s in ids}
    assert len(streams) >= 2, fires
    # an active stream does not fire again: between two releases a stream fires once at the most
    for lo, hi in zip((0,) + SC.STAGE_RELEASE, SC.STAGE_RELEASE + (SC.TICKS,)):
        ids = [s for t, f in fires if lo <= t < hi for s in f]
        assert len(ids) == len(set(ids)), fires


# ---- csrc/stream_ctc.h under the sanitizers -------------------------------------------------------------------------------------------
def _no_sanitizer_runtime(output):
    """Did a -fsanitize build fail because this clang ships no runtime for it?  (tests/test_stream_rates_host.py's rule.)"""
    return re.search(r"libclang_rt\.|unsupported (option|argument)[^\n]*-fsanitize", output) is not None


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    cxx = "/opt/rocm/lib/llvm/bin/clang++"
    if not os.path.exists(cxx):
        cxx = shutil.which("clang++")
    if cxx is None:
        pytest.skip("no clang++ in this image")
    d = tmp_path_factory.mktemp("stream_ctc")
    exe = d / "stream_ctc_check"
    b = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-I" + _CSRC,
                        os.path.join(_ROOT, "tests", "native", "stream_ctc_check.cpp"), "-o", str(exe)], capture_output=True, text=True)
    if b.returncode != 0 and _no_sanitizer_runtime(b.stderr + b.stdout):
        pytest.skip("this clang has no sanitizer runtime: " + b.stderr[-300:])
    assert b.returncode == 0, b.stderr[-2000:]

    def run(packs, trigs):
        f = d / "cases.bin"
        with open(f, "wb") as fh:
            fh.write(struct.pack("<i", len(packs)))
            for length, labels in packs:
                fh.write(struct.pack("<10i", length, *labels))
            fh.write(struct.pack("<i", len(trigs)))
            for c in trigs:
                fh.write(struct.pack("<3i", c["S"], c["m"], len(c["target"])))
                fh.write(np.asarray(c["target"], "<i4").tobytes())
                for s in range(c["S"]):
                    fh.write(struct.pack("<4i", c["speech"][s], c["active"][s], c["was"][s], c["n"][s]))
                    fh.write(np.ascontiguousarray(c["labels"][s], "<i4").tobytes())
                    fh.write(np.ascontiguousarray(c["lengths"][s], "<i4").tobytes())
        r = subprocess.run([str(exe), str(f)], capture_output=True, text=True, timeout=120,
                           env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1"))
        assert r.returncode == 0 and not r.stderr.strip(), (r.returncode, r.stdout[-300:], r.stderr[-3000:])
        lines = r.stdout.strip().splitlines()
        assert lines[-1] == f"ok {len(packs)} {len(trigs)}" and len(lines) == len(packs) + len(trigs) + 1, lines[-1]
        return lines[:len(packs)], lines[len(packs):-1]
    return run


def _pack_cases(seed=7):
    rng = np.random.default_rng(seed)
    out = [(length, [int(c) if i < length else -1 for i, c in enumerate(rng.integers(0, 7, 9))]) for length in range(20) for _ in range(20)]
    out.append((19, [6] * 9))
    out.append((0, [-1] * 9))
    return out


def _trigger_cases(seed=11, n=600):
    """Seeded ticks of the stage: activity, falling edges and n_post of 0, 1 and 2; decodes that start with the target, that are
    the target cut short, that carry it in the second window only."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        S, m = int(rng.integers(1, 7)), int(rng.integers(1, 10))
        nt = int(rng.integers(1, m + 1))
        target = rng.integers(0, 3, nt)
        labels = rng.integers(0, 3, (S, 2, m)).astype(np.int32)
        lengths = rng.integers(0, 20, (S, 2)).astype(np.int32)
        for s in range(S):
            for k in range(2):
                if rng.random() < 0.5:
                    labels[s, k, :nt] = target       # starts with the target - if its length reaches it
                labels[s, k, min(int(lengths[s, k]), m):] = -1
        out.append(dict(S=S, m=m, target=target, labels=labels, lengths=lengths, n=rng.integers(0, 3, S), speech=rng.integers(0, 2, S),
                        active=rng.integers(0, 2, S), was=rng.integers(0, 2, S)))
    return out


def _stage_rule(c):
    """The stage's rule in plain Python with ``ctc.is_wakeword`` as the firing rule: (fired, fall, is_active', was_speech')."""
    from wwhip import ctc
    fired, fall, act, was = [], [], list(c["active"]), list(c["was"])
    for s in range(c["S"]):
        n = int(c["n"][s])
        hit = n > 0 and bool(ctc.is_wakeword(c["labels"][s, :n], c["lengths"][s, :n], c["target"]).any())
        if hit and not act[s]:
            act[s] = 1
            fired.append(s)
        if was[s] and not c["speech"][s]:
            fall.append(s)
        was[s] = int(c["speech"][s])
    return fired, fall, act, was


def test_pack_unpack_and_the_trigger_rule_under_the_sanitizers(check_exe):
    packs, trigs = _pack_cases(), _trigger_cases()
    got_p, got_t = check_exe(packs, trigs)
    for (length, labels), line in zip(packs, got_p):
        word = (length << 27) | sum((c & 7) << (3 * i) for i, c in enumerate(labels) if i < min(length, 9))
        assert line == "P " + " ".join(str(v) for v in [word, length] + [c if i < length else -1 for i, c in enumerate(labels)]), (length, labels)
    kinds = set()
    for c, line in zip(trigs, got_t):
        fired, fall, act, was = _stage_rule(c)
        want = "T " + " | ".join(" ".join(str(int(v)) for v in part) for part in ([len(fired)] + fired, [len(fall)] + fall, act, was))
        assert line == want, (c, line, want)
        kinds.update({("fired", bool(fired)), ("fall", bool(fall)), ("n", tuple(sorted(set(int(v) for v in c["n"]))))})
    assert ("fired", True) in kinds and ("fired", False) in kinds and ("fall", True) in kinds
    assert {v for k, v in kinds if k == "n" for v in v} == {0, 1, 2}


# ---- the Python classes against a stub ----------------------------------------------------------------------------------------------------
class _StubCtcBank:
    """Stands where ``CtcStreamBank`` stands in ``CtcWakewordBank``: 'delivers' scripted decodes (an active stream is not sampled, a
    frame is analysed only while the stream's VAD bit is set), then runs the library's host pass ``ww_ctc_trigger_bank_step`` exactly
    as ``ww_stream_step_ctc_trigger`` does after the tick."""

    def __init__(self, S, max_labels, script, flags):
        from wwhip import _lib
        self.lib, self.S, self.max_labels = _lib.load(), S, max_labels
        self.script, self.flags, self.t, self.resets = script, flags, 0, 0

    def step_ctc_trigger(self, frames, p_speech, p_active, p_target, n_target, st):
        from wwhip import _lib
        from wwhip.engine import CtcTick
        speech, active = self.flags()
        labels, lengths, n = (np.ascontiguousarray(a) for a in self.script[self.t])
        n = np.where((speech != 0) & (active == 0), n, 0).astype(np.int32)
        self.t += 1
        assert self.lib.ww_ctc_trigger_bank_step(self.S, p_speech, p_active, _lib.ptr(labels), _lib.ptr(lengths), _lib.ptr(n), self.max_labels,
                                                 p_target, n_target, *st) == 0
        return CtcTick(labels, lengths, n, None)

    def reset(self, ids=None):
        self.resets += 1

    def close(self):
        pass


def test_ctc_wakeword_bank_against_a_stub_bank():
    from wwhip.context import ContextBank
    from wwhip.wakeword import CtcWakewordBank
    S, M, ticks = 4, 3, 60
    rng = np.random.default_rng(5)
    script = []
    for _ in range(ticks):
        labels = rng.integers(0, 3, (S, 2, M)).astype(np.int32)
        lengths = rng.integers(0, 5, (S, 2)).astype(np.int32)
        for s in range(S):
            for k in range(2):
                labels[s, k, min(int(lengths[s, k]), M):] = -1
        script.append((labels, lengths, rng.integers(0, 3, S).astype(np.int32)))
    ctxs = ContextBank(S)
    events = []
    ctxs.add_handler("activate", lambda view: events.append(int(view.s) if hasattr(view, "s") else None))
    woke = []
    stub = _StubCtcBank(S, M, script, lambda: (ctxs.is_speech, ctxs.is_active))
    stage = CtcWakewordBank(S, bank=stub, target=(1, 2), on_wake=lambda ids: woke.append([int(i) for i in ids]))
    active, was, want_wakes = np.zeros(S, np.uint8), np.zeros(S, np.uint8), []
    for t in range(ticks):
        ctxs.is_speech[:] = rng.integers(0, 4, S) > 0
        if t % 13 == 12:
            ctxs.is_active[:] = 0
            active[:] = 0
        c = dict(S=S, labels=script[t][0], lengths=script[t][1], target=(1, 2), speech=ctxs.is_speech.copy(), active=active, was=was,
                 n=np.where((ctxs.is_speech != 0) & (active == 0), script[t][2], 0))
        fired, fall, act, was_new = _stage_rule(c)
        tick = stage(ctxs, np.zeros((S, 320), np.int16))
        assert (tick.n == c["n"]).all() and (stage.n_post == c["n"]).all()
        assert stage.fired_ids.tolist() == fired and stage.fall_ids.tolist() == fall, t
        assert ctxs.is_active.tolist() == act
        if fired:
            want_wakes.append(fired)
        active, was = np.asarray(act, np.uint8), np.asarray(was_new, np.uint8)
    assert woke == want_wakes and len(woke) >= 2
    assert len(events) == sum(len(w) for w in woke)   # one activate event per stream that fired
    stage.reset()
    assert stub.resets == 1
    stage.close()


def test_ctc_wakeword_bank_argument_checks():
    from wwhip.wakeword import CtcWakewordBank
    stub = _StubCtcBank(3, 2, [], lambda: None)
    with pytest.raises(ValueError, match="needs engine"):
        CtcWakewordBank(3)
    with pytest.raises(ValueError, match="non-empty"):
        CtcWakewordBank(3, bank=stub, target=())
    with pytest.raises(ValueError, match="0..7"):
        CtcWakewordBank(3, bank=stub, target=(1, 8))
    with pytest.raises(ValueError, match="at most 9"):
        CtcWakewordBank(3, bank=stub, target=(1,) * 10)
    with pytest.raises(ValueError, match="keeps 2 labels"):
        CtcWakewordBank(3, bank=stub, target=(1, 2, 1))
    with pytest.raises(ValueError, match="has 3 streams"):
        CtcWakewordBank(4, bank=stub)
    with pytest.raises(ValueError, match="does not decode labels"):
        CtcWakewordBank(3, bank=object())
    with pytest.raises(ValueError, match="one context per stream"):
        CtcWakewordBank(3, bank=stub)([None] * 2, np.zeros((3, 320), np.int16))


def test_ctc_stream_bank_refuses_before_it_touches_a_device():
    from wwhip.engine import CtcStreamBank

    class _Eng:
        is_ctc = True

    class _Other:
        is_ctc = False

    with pytest.raises(ValueError, match="CTC-trained CRNN"):
        CtcStreamBank(_Other(), 2)
    for m in (0, 10, -1):
        with pytest.raises(ValueError, match="outside 1..9"):
            CtcStreamBank(_Eng(), 2, max_labels=m)
    with pytest.raises(ValueError, match="unknown sample format"):
        CtcStreamBank(_Eng(), 2, sample_format="flac")
    with pytest.raises(ValueError, match="whole number of samples"):
        CtcStreamBank(_Eng(), 2, sample_rate=11025)


def test_the_fused_pipeline_declines_the_ctc_stage():
    """``SpeechPipelineBank`` takes ``ww_pipeline_bank_step`` for exactly VadBank, WakewordBank, ActivationTimeoutBank: the CTC stage
    is a stage like any other and runs in the stage-by-stage loop."""
    from wwhip.activation_timeout import ActivationTimeoutBank
    from wwhip.pipeline import SpeechPipelineBank
    from wwhip.vad import VadBank
    from wwhip.wakeword import CtcWakewordBank, WakewordBank
    S = 2
    stage = CtcWakewordBank(S, bank=_StubCtcBank(S, 2, [], lambda: None))
    assert type(stage) is not WakewordBank and not isinstance(stage, WakewordBank)
    pipe = SpeechPipelineBank(None, [VadBank(S), stage, ActivationTimeoutBank(S)], S)
    assert getattr(pipe, "_fused", None) is None
