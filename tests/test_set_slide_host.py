"""A model set's sliding form on the host: the group planner with its window cap and the member-list check under Address + UB
sanitizer (a stand-alone program), the ctypes binding of the three new entry points, and the errors ``ModelSet`` finds before it
touches a device."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CSRC = os.path.join(_ROOT, "wakeword-detection_amd", "csrc")
NEW_SYMBOLS = ["ww_set_forward_segments_dev", "ww_set_slide_forward", "ww_set_option"]


def _no_sanitizer_runtime(output):
    """Did a -fsanitize build fail because this clang ships no runtime for it?  (tests/test_host_logic.py's rule: the driver's or
    the linker's own words, not the word "sanitizer".)"""
    return re.search(r"libclang_rt\.|unsupported (option|argument)[^\n]*-fsanitize", output) is not None


def test_group_planner_and_member_list_under_sanitizers(tmp_path):
    """csrc/launch_plan.h's crnn_plan_group with caps 40, 48 and WW_SEG_GROUP (alone and as the budget of 2 and 3 members) over
    sequence lists that hold 0, 1, 16, 17 windows and a sequence larger than the cap: no group splits a sequence, members x windows
    of a group stay at or below the budget unless the group is one sequence, the concatenated tiles and i0 are the default plan's
    shifted by the group bases, and every interior field, left edge and right edge has exactly one owner tile.  csrc/model_set.h's
    ww_set_check_ids on the call's member list: NULL, duplicates, -1 and K refused with the index named.
    (tests/native/set_slide_check.cpp; a child process, nothing is loaded into this interpreter.)"""
    cxx = "/opt/rocm/lib/llvm/bin/clang++"
    if not os.path.exists(cxx):
        cxx = shutil.which("clang++")
    if cxx is None:
        pytest.skip("no clang++ in this image")
    exe = tmp_path / "set_slide_check"
    b = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-I" + _CSRC,
                        os.path.join(_ROOT, "tests", "native", "set_slide_check.cpp"), "-o", str(exe)], capture_output=True, text=True)
    if b.returncode != 0 and _no_sanitizer_runtime(b.stderr + b.stdout):
        pytest.skip("this clang has no sanitizer runtime: " + b.stderr[-300:])
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1"))
    assert r.returncode == 0 and r.stdout.startswith("ok ") and not r.stderr.strip(), (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    assert int(r.stdout.split()[1]) > 5000


def test_binding_covers_the_new_entry_points():
    """include/wwhip.h declares them, wwhip/_lib.py binds each with as many arguments as the declaration has, and the library
    exports them; WW_ABI stays 4."""
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
    from wwhip import evaluate
    from wwhip.engine import ModelSet
    for name in ("forward_segments_dev", "slide_forward_all", "set_option"):
        assert callable(getattr(ModelSet, name)), name
    assert callable(evaluate.clip_posteriors_set) and callable(evaluate.evaluate_testset_set)


def test_host_detectable_errors_raise_before_any_device_call(monkeypatch):
    from wwhip import _lib
    from wwhip.engine import ModelSet

    class NoNative:
        def __getattr__(self, name):
            raise AssertionError(f"a host-detectable error reached the native library ({name})")
    ms = ModelSet.__new__(ModelSet)
    ms.window, ms.n_mel, ms.n_models, ms.n_out, ms.enc_shape, ms._set, ms._own, ms._lib = 151, 40, 3, 2, (1, 64), None, [], NoNative()
    with pytest.raises(ValueError, match="options"):
        ms.set_option("crnn_split_at", 0)
    with pytest.raises(ValueError, match="members"):
        ms.slide_forward_all(np.zeros((200, 40), np.float32), members=[0, 3])
    with pytest.raises(ValueError, match="members"):
        ms.slide_forward_all(np.zeros((200, 40), np.float32), members=[-1])
    with pytest.raises(ValueError, match="members"):
        ms.slide_forward_all(np.zeros((200, 40), np.float32), members=[[0, 1]])
    with pytest.raises(ValueError, match="mel must be"):
        ms.slide_forward_all(np.zeros((200, 39), np.float32))
    with pytest.raises(ValueError, match="same length"):
        ms.forward_segments_dev(0, 0, np.zeros(2, np.int64), np.zeros(3, np.int32), 2, 0)
    with pytest.raises(ValueError, match="members"):
        ms.forward_segments_dev(0, 0, np.zeros(2, np.int64), np.zeros(2, np.int32), 2, 0, members=[1.5])
    ids = ms._slots([1, 1, 2, 0, 1])  # any number of slots, duplicates allowed
    assert ids.dtype == np.int32 and ids.tolist() == [1, 1, 2, 0, 1] and ms._slots(None) is None and ms._slots([]).size == 0
    assert _lib.OPT_CRNN_SLIDE_MIN == 2 and _lib.OPT_CRNN_TAIL_MFMA == 3
