"""Stream banks that run every listed member of a model set on every stream, on the host: csrc/stream_all.h under Address + UB
sanitizer (a stand-alone program), the ctypes binding of the three new entry points, and the errors that
``StreamBank(model_set, S, members=...)``, ``WakewordBank`` and ``SpeechPipelineBank`` find before they touch the native library."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CSRC = os.path.join(_ROOT, "wakeword-detection_amd", "csrc")
NEW_SYMBOLS = ["ww_stream_create_set_all", "ww_stream_step_all", "ww_stream_members"]


def _no_sanitizer_runtime(output):
    """Did a -fsanitize build fail because this clang ships no runtime for it?  (tests/test_stream_rates_host.py's rule.)"""
    return re.search(r"libclang_rt\.|unsupported (option|argument)[^\n]*-fsanitize", output) is not None


@pytest.fixture(scope="module")
def check_run(tmp_path_factory):
    """tests/native/stream_all_check.cpp compiled with Address + UB sanitizer and run once, as a child process (nothing is loaded
    into this interpreter): the finished process, or a skip where there is no compiler or no sanitizer runtime."""
    cxx = "/opt/rocm/lib/llvm/bin/clang++"
    if not os.path.exists(cxx):
        cxx = shutil.which("clang++")
    if cxx is None:
        pytest.skip("no clang++ in this image")
    exe = tmp_path_factory.mktemp("stream_all") / "stream_all_check"
    b = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-I" + _CSRC,
                        os.path.join(_ROOT, "tests", "native", "stream_all_check.cpp"), "-o", str(exe)], capture_output=True, text=True)
    if b.returncode != 0 and _no_sanitizer_runtime(b.stderr + b.stdout):
        pytest.skip("this clang has no sanitizer runtime: " + b.stderr[-300:])
    assert b.returncode == 0, b.stderr[-2000:]
    return subprocess.run([str(exe)], capture_output=True, text=True, timeout=120,
                          env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1"))


def test_stream_all_header_under_sanitizers(check_run):
    """csrc/stream_all.h - the virtual-stream arithmetic, the member table, a tick's control words, descriptors, tag slots and post
    scatter in the three launch forms over K in {1, 3, 5} and S in {1, 5} with ring wraps and resets, and every refusal - compiled
    alone with Address + UB sanitizer and checked on the CPU (tests/native/stream_all_check.cpp lists the properties)."""
    r = check_run
    last = r.stdout.strip().splitlines()[-1] if r.stdout.strip() else ""
    assert r.returncode == 0 and last.startswith("ok ") and not r.stderr.strip(), (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    assert int(last.split()[1]) > 100000


def test_stream_all_header_is_host_only_and_is_the_ticks_one_plan():
    """stream_all.h includes no HIP header and calls no HIP function, and streams.hip plans a tick nowhere else: the ordinary bank
    is the K = 1 case of the same body."""
    text = open(os.path.join(_CSRC, "stream_all.h")).read()
    code = re.sub(r"//[^\n]*", "", text)
    assert "hip/" not in code and "common.h" not in code and not re.search(r"\bhip[A-Z]\w*\(", code)
    assert "__global__" not in code and "__shared__" not in code and "__device__" not in code
    streams = re.sub(r"//[^\n]*", "", open(os.path.join(_CSRC, "streams.hip")).read())
    assert '#include "stream_all.h"' in streams
    assert streams.count("sa_tick_stream(") == 1 and streams.count("static int stream_step_impl(") == 1
    assert len(re.findall(r"\bstream_step_impl\(", streams)) == 2  # its definition and its one caller
    assert "h_ctl[s * 4" not in streams and "h_win_aux[nw" not in streams


def test_binding_covers_the_new_entry_points():
    from wwhip import _lib
    header = open(os.path.join(_ROOT, "include", "wwhip.h")).read()
    assert re.search(r"#define WW_ABI 4\b", header) and _lib.ABI == 4
    limits = open(os.path.join(_CSRC, "stream_all.h")).read()
    from wwhip import engine
    assert re.search(r"#define WW_ALL_MAX_MEMBERS %d\b" % engine.MAX_MEMBER_SLOTS, limits) and engine.MAX_MEMBER_SLOTS == 64
    assert re.search(r"#define WW_ALL_MAX_VIRTUAL 65535\b", limits)
    for name in NEW_SYMBOLS:
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert m, f"{name} is not declared in include/wwhip.h"
        assert name in _lib.SYMBOLS, f"{name} is not bound in wwhip/_lib.py"
        assert len(_lib.SYMBOLS[name][1]) == m.group(1).count(",") + 1, name
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name


def test_host_detectable_errors_raise_before_any_native_call(monkeypatch):
    from wwhip import _lib
    from wwhip import engine
    from wwhip.engine import ModelSet, StreamBank
    from wwhip.pipeline import SpeechPipelineBank
    from wwhip.wakeword import WakewordBank

    def no_native(*a, **k):
        raise AssertionError("a host-detectable error reached the native library")
    monkeypatch.setattr(_lib, "load", no_native)
    monkeypatch.setattr(_lib, "default_context", no_native)
    monkeypatch.setattr(_lib, "addr", no_native)

    class _Eng:
        n_models = 1

    mset = ModelSet.__new__(ModelSet)
    mset.n_models, mset._h = 3, None
    with pytest.raises(ValueError, match="built on one Engine"):
        StreamBank(_Eng(), 2, members="all")
    with pytest.raises(ValueError, match="mutually exclusive"):
        StreamBank(mset, 2, members="all", models=[0, 1])
    with pytest.raises(ValueError, match="full_recompute"):
        StreamBank(mset, 2, members=[0], full_recompute=True)
    with pytest.raises(ValueError, match='"all" or a list'):
        StreamBank(mset, 2, members="every")
    for bad in ([], [0, 3], [-1], [0.5], [[0, 1]]):
        with pytest.raises(ValueError, match=r"integers in \[0, 3\)"):
            StreamBank(mset, 2, members=bad)
    with pytest.raises(ValueError, match="65 member slots"):
        StreamBank(mset, 2, members=[0] * 65)
    with pytest.raises(ValueError, match="at most 65535"):
        StreamBank(mset, 16384, members=[0, 1, 2, 0])
    assert engine._member_slots("all", mset, 5, None, False).tolist() == [0, 1, 2]
    assert engine._member_slots([2, 0, 2], mset, 21845, None, False).tolist() == [2, 0, 2]
    # a bank of that kind: feed, set_model and step_trigger are refused, and so are the stages that need one posterior per stream
    bank = StreamBank.__new__(StreamBank)
    bank.engine, bank.S, bank._h = mset, 2, None
    bank.members, bank.n_members = np.array([0, 1, 2], np.int32), 3
    with pytest.raises(ValueError, match="feed: this bank runs every listed member"):
        bank.feed([0], [np.zeros(320, np.int16)])
    with pytest.raises(ValueError, match="set_model: this bank runs every listed member"):
        bank.set_model([0], 1)
    with pytest.raises(ValueError, match="step_trigger: this bank runs every listed member"):
        bank.step_trigger(np.zeros((2, 320), np.int16), 0, 0, 0.5, ())
    with pytest.raises(ValueError, match="cannot say which wake word fired"):
        WakewordBank(2, bank=bank)
    stage = WakewordBank.__new__(WakewordBank)
    stage._bank = bank
    with pytest.raises(ValueError, match="has no trigger stage"):
        SpeechPipelineBank(None, [stage], 2)
    ordinary = StreamBank.__new__(StreamBank)
    assert ordinary.members is None and ordinary.n_members == 0
