"""The Wavenet's sequence form over a model set, on the host: the planner of a set's launch under Address + UB sanitizer (a
stand-alone program), the ctypes binding of the four new entry points, the errors ``ModelSet`` finds before it touches a device,
and the rule that a ``_dev`` entry point synchronises nothing."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CSRC = os.path.join(_ROOT, "wakeword-detection_amd", "csrc")
NEW_SYMBOLS = ["ww_set_wave_sequence_dev", "ww_set_wave_sequence", "ww_set_wave_sequence_all_dev", "ww_set_wave_sequence_all"]


def _no_sanitizer_runtime(output):
    """Did a -fsanitize build fail because this clang ships no runtime for it?  (tests/test_host_logic.py's rule: the driver's or
    the linker's own words, not the word "sanitizer".)"""
    return re.search(r"libclang_rt\.|unsupported (option|argument)[^\n]*-fsanitize", output) is not None


def test_set_planner_under_sanitizers(tmp_path):
    """csrc/launch_plan.h's wave_seq_make_plan over 600 random offset lists (empty sequences, lengths around the chunk and
    the receptive field, rows in front of and behind the sequences), explicit and library-chosen segment lengths, slot counts 1,
    2, 3, 64, 65, 1024 with an id per plane, and the by-sequence form: the cuts are those of the plan without ids (the single
    model's) segment for segment; every (sequence row, plane) has exactly one owner segment and no other row has one; the warm-up
    is min(s0, rf - 1); seg_seq names each segment's sequence; the table sizes are what the plan reserved; one plane reproduces
    the single model's plan, which reserves neither ids nor seg_seq.  csrc/model_set.h's
    ww_set_check_ids on ``seq_model`` and ``members``.  (tests/native/set_wave_seq_check.cpp; a child process, nothing is loaded
    into this interpreter.)"""
    cxx = "/opt/rocm/lib/llvm/bin/clang++"
    if not os.path.exists(cxx):
        cxx = shutil.which("clang++")
    if cxx is None:
        pytest.skip("no clang++ in this image")
    exe = tmp_path / "set_wave_seq_check"
    b = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-I" + _CSRC,
                        os.path.join(_ROOT, "tests", "native", "set_wave_seq_check.cpp"), "-o", str(exe)], capture_output=True, text=True)
    if b.returncode != 0 and _no_sanitizer_runtime(b.stderr + b.stdout):
        pytest.skip("this clang has no sanitizer runtime: " + b.stderr[-300:])
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1"))
    assert r.returncode == 0 and r.stdout.startswith("ok ") and not r.stderr.strip(), (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    assert int(r.stdout.split()[1]) > 100000


def test_binding_covers_the_new_entry_points():
    """include/wwhip.h declares the four, wwhip/_lib.py binds each with as many arguments as the declaration has, the library
    exports them, and ``ModelSet`` has the methods; WW_ABI stays 4."""
    from wwhip import _lib
    header = open(os.path.join(_ROOT, "include", "wwhip.h")).read()
    assert re.search(r"#define WW_ABI 4\b", header) and _lib.ABI == 4
    for name in NEW_SYMBOLS:
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert m, f"{name} is not declared in include/wwhip.h"
        assert name in _lib.SYMBOLS, f"{name} is not bound in wwhip/_lib.py"
        assert len(_lib.SYMBOLS[name][1]) == m.group(1).count(",") + 1, name
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
    from wwhip.engine import ModelSet
    for name in ("sequence_forward", "sequence_forward_all", "wave_sequence_dev", "wave_sequence_all_dev", "set_option"):
        assert callable(getattr(ModelSet, name)), name
    assert _lib.OPT_WAVE_SEQ_SEGMENT == 5


def test_host_detectable_errors_raise_before_any_native_call():
    from wwhip.engine import ModelSet

    class NoNative:
        def __getattr__(self, name):
            raise AssertionError(f"a host-detectable error reached the native library ({name})")
    ms = ModelSet.__new__(ModelSet)
    ms.window, ms.n_mel, ms.n_models, ms.n_out, ms.enc_shape, ms._set, ms._own, ms._lib = 182, 40, 2, 2, (182, 32), None, [], NoNative()
    seqs = [np.zeros((5, 40), np.float32), np.zeros((0, 40), np.float32), np.zeros((200, 40), np.float32)]
    with pytest.raises(ValueError, match="want"):
        ms.sequence_forward(seqs, [0, 1, 0], want=("post", "posterior"))
    with pytest.raises(ValueError, match="want"):
        ms.sequence_forward_all(seqs, want=("encoder",))
    with pytest.raises(ValueError, match=r"\[rows, 40\]"):
        ms.sequence_forward([np.zeros((5, 39), np.float32)], [0])
    with pytest.raises(ValueError, match=r"\[rows, 40\]"):
        ms.sequence_forward_all([np.zeros((5, 40), np.float32), np.zeros(40, np.float32)])
    with pytest.raises(ValueError, match="one entry per sequence"):
        ms.sequence_forward(seqs, [0, 1])
    with pytest.raises(ValueError, match="one entry per sequence"):
        ms.sequence_forward(seqs, [[0, 1, 0]])
    with pytest.raises(ValueError, match="seq_model"):
        ms.sequence_forward(seqs, [0, 1.5, 0])
    with pytest.raises(ValueError, match="seq_model"):
        ms.sequence_forward(seqs, [0, 2, 0])
    with pytest.raises(ValueError, match="seq_model"):
        ms.sequence_forward(seqs, [0, -1, 0])
    with pytest.raises(ValueError, match="members"):
        ms.sequence_forward_all(seqs, members=[0, 2])
    with pytest.raises(ValueError, match="members"):
        ms.sequence_forward_all(seqs, members=[-1])
    with pytest.raises(ValueError, match="members"):
        ms.sequence_forward_all(seqs, members=[0.5])
    with pytest.raises(ValueError, match="members"):
        ms.sequence_forward_all(seqs, members=[[0, 1]])
    offs = np.array([0, 5, 5, 205], np.int64)
    with pytest.raises(ValueError, match="one entry per sequence"):
        ms.wave_sequence_dev(0, 205, offs, [0, 1])
    with pytest.raises(ValueError, match="seq_model"):
        ms.wave_sequence_dev(0, 205, offs, [0, 1, 2])
    with pytest.raises(ValueError, match="row_offs"):
        ms.wave_sequence_dev(0, 205, np.zeros((2, 2), np.int64), [0])
    with pytest.raises(ValueError, match="members"):
        ms.wave_sequence_all_dev(0, 205, offs, members=[2])
    with pytest.raises(ValueError, match="row_offs"):
        ms.wave_sequence_all_dev(0, 205, np.zeros(0, np.int64))
    with pytest.raises(ValueError, match="options"):
        ms.set_option("wavenet_rowmajor", 1)
    with pytest.raises(ValueError, match="options"):
        ms.set_option("crnn_split_at", 0)


def _body(api, name):
    m, = re.finditer(r"^[A-Za-z_][A-Za-z0-9_ \*]*\b" + name + r"\(", api, flags=re.M)
    open_brace = api.index("{", m.end())
    return api[open_brace:api.index("\n}\n", open_brace)]


def test_the_dev_entry_points_synchronise_nothing():
    """The bodies of ww_wave_sequence_dev, ww_set_wave_sequence_dev and ww_set_wave_sequence_all_dev - and of every function
    between them and wave_seq_run, the one path of a model and a model set - hold no hipStreamSynchronize, hipDeviceSynchronize
    or hipEventSynchronize; the tables go through wave_seq_run's one tb.send."""
    api = open(os.path.join(_CSRC, "api.hip")).read()
    for name in ("ww_wave_sequence_dev", "ww_set_wave_sequence_dev", "ww_set_wave_sequence_all_dev"):
        body = _body(api, name)
        assert "wave_seq_dev(" in body, name
        for sync in ("hipStreamSynchronize", "hipDeviceSynchronize", "hipEventSynchronize"):
            assert sync not in body, (name, sync)
    chain = {"wave_seq_dev": "wave_seq_run(", "wave_seq_check": "wave_seq_validate(", "wave_seq_plan_of": "wave_seq_make_plan(",
             "wave_seq_run": "tb.send("}
    for name, callee in chain.items():
        body = _body(api, name)
        assert callee in body, (name, callee)
        for sync in ("hipStreamSynchronize", "hipDeviceSynchronize", "hipEventSynchronize"):
            assert sync not in body, (name, sync)
    assert "wave_seq_check(" in _body(api, "wave_seq_dev") and "wave_seq_plan_of(" in _body(api, "wave_seq_dev")
    # one definition each of what the set shares with the single model
    assert len(re.findall(r"^static int wave_seq_run\(", api, re.M)) == 1 and len(re.findall(r"^static int wave_seq_validate\(", api, re.M)) == 1
