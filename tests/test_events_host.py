"""Detection events on the host: the planner of csrc/events_plan.h under Address + UB sanitizer (a stand-alone program), the binding of
``ww_posterior_events`` / ``ww_posterior_events_dev`` and ``ww_event``, and the float64 restatement tests/events64.py pinned on
hand-written cases."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CSRC = os.path.join(_ROOT, "wakeword-detection_amd", "csrc")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import events64 as E  # noqa: E402

NEW_SYMBOLS = ["ww_posterior_events_dev", "ww_posterior_events"]


def _no_sanitizer_runtime(output):
    """Did a -fsanitize build fail because this clang ships no runtime for it?  (tests/test_stream_rates_host.py's rule.)"""
    return re.search(r"libclang_rt\.|unsupported (option|argument)[^\n]*-fsanitize", output) is not None


@pytest.fixture(scope="module")
def check_run(tmp_path_factory):
    """tests/native/events_plan_check.cpp compiled with Address + UB sanitizer and run once, as a child process (nothing is loaded into
    this interpreter): the finished process, or a skip where there is no compiler or no sanitizer runtime."""
    cxx = "/opt/rocm/lib/llvm/bin/clang++"
    if not os.path.exists(cxx):
        cxx = shutil.which("clang++")
    if cxx is None:
        pytest.skip("no clang++ in this image")
    exe = tmp_path_factory.mktemp("events_plan") / "events_plan_check"
    b = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-I" + _CSRC,
                        os.path.join(_ROOT, "tests", "native", "events_plan_check.cpp"), "-o", str(exe)], capture_output=True, text=True)
    if b.returncode != 0 and _no_sanitizer_runtime(b.stderr + b.stdout):
        pytest.skip("this clang has no sanitizer runtime: " + b.stderr[-300:])
    assert b.returncode == 0, b.stderr[-2000:]
    return subprocess.run([str(exe)], capture_output=True, text=True, timeout=120,
                          env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1"))


def test_planner_under_sanitizers(check_run):
    """Every refusal, the tile counts and the capacity arithmetic at n = 0, 1, tile - 1, tile, tile + 1 and 2^40 rows, and the scratch
    layout (tests/native/events_plan_check.cpp lists the properties)."""
    r = check_run
    last = r.stdout.strip().splitlines()[-1] if r.stdout.strip() else ""
    assert r.returncode == 0 and last.startswith("ok ") and not r.stderr.strip(), (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    assert int(last.split()[1]) > 1000


def test_the_planner_header_is_host_only_and_listed_for_the_build():
    text = re.sub(r"//[^\n]*", "", open(os.path.join(_CSRC, "events_plan.h")).read())
    assert "hip/" not in text and "__global__" not in text and "__device__" not in text
    assert '"events_plan.h"' in open(os.path.join(_ROOT, "wakeword-detection_amd", "wwhip", "_build.py")).read()
    api = re.sub(r"//[^\n]*", "", open(os.path.join(_CSRC, "api.hip")).read())
    assert len(re.findall(r"\bev_check\(", api)) == 1 and len(re.findall(r"\bev_make_plan\(", api)) == 1


def test_binding_covers_the_new_entry_points():
    from wwhip import _lib
    header = open(os.path.join(_ROOT, "include", "wwhip.h")).read()
    assert re.search(r"#define WW_ABI 4\b", header) and _lib.ABI == 4
    for name in NEW_SYMBOLS:
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert m, f"{name} is not declared in include/wwhip.h"
        assert name in _lib.SYMBOLS, f"{name} is not bound in wwhip/_lib.py"
        assert len(_lib.SYMBOLS[name][1]) == m.group(1).count(",") + 1 == 12, name
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
    assert b"ABI 4" in lib.ww_version()


def test_event_dtype_mirrors_the_struct():
    """``ww_event`` as the header declares it - field order, C types, natural alignment - against ``_lib.EVENT_DTYPE``."""
    from wwhip import _lib
    header = open(os.path.join(_ROOT, "include", "wwhip.h")).read()
    m = re.search(r"typedef struct ww_event \{(.*?)\} ww_event;", header, flags=re.S)
    assert m
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    size = {"int32_t": 4, "int64_t": 8, "double": 8}
    kind = {"int32_t": np.int32, "int64_t": np.int64, "double": np.float64}
    off, fields = 0, []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        ctype, names = decl.split(None, 1)
        for name in (x.strip() for x in names.split(",")):
            off = (off + size[ctype] - 1) // size[ctype] * size[ctype]
            fields.append((name, kind[ctype], off))
            off += size[ctype]
    assert off == 40 and [f[0] for f in fields] == ["plane", "seg", "start", "end", "peak", "peak_value"]
    dt = _lib.EVENT_DTYPE
    assert dt.itemsize == 40 and list(dt.names) == [f[0] for f in fields]
    for name, k, o in fields:
        assert dt.fields[name][0] == np.dtype(k) and dt.fields[name][1] == o, name


# ---- the float64 restatement, pinned
WFST_1 = [[0.8, 0.2], [0.9, 0.1], [0.5, 0.5], [0.4, 0.6], [0.2, 0.8], [0.6, 0.4], [0.3, 0.7], [0.4, 0.6], [0.5, 0.5], [0.9, 0.1]]
WFST_2 = [[0.8, 0.2], [0.9, 0.1], [0.5, 0.5], [0.55, 0.45], [0.2, 0.8], [0.6, 0.4], [0.7, 0.3], [0.8, 0.2], [0.3, 0.7], [0.9, 0.1]]


def _f32(x):
    return float(np.float32(x))


def test_restatement_on_the_wfst_lists():
    """The wake-word column of the two ``test_posterior`` lists of wwdetect/wfst.py at threshold 0.5, unsmoothed: 0.5 itself is not
    above; list 1 leaves the wake word at row 5 and re-enters it, list 2 has two single-row events."""
    p1, p2 = np.array(WFST_1, np.float32)[:, 1], np.array(WFST_2, np.float32)[:, 1]
    ev, _ = E.events(p1, 0.5, win=0)
    assert ev == [(0, 0, 3, 5, 4, _f32(0.8)), (0, 0, 6, 8, 6, _f32(0.7))]
    ev, _ = E.events(p2, 0.5, win=0)
    assert ev == [(0, 0, 4, 5, 4, _f32(0.8)), (0, 0, 8, 9, 8, _f32(0.7))]
    # both lists as two segments of one plane, and as two planes with their own thresholds
    ev, _ = E.events(np.concatenate([p1, p2]), 0.5, seg_offs=[0, 10, 20], win=0)
    assert [e[:5] for e in ev] == [(0, 0, 3, 5, 4), (0, 0, 6, 8, 6), (0, 1, 4, 5, 4), (0, 1, 8, 9, 8)]
    ev, _ = E.events(np.stack([p1, p2]), [0.65, 0.75], win=0)
    assert [e[:5] for e in ev] == [(0, 0, 4, 5, 4), (0, 0, 6, 7, 6), (1, 0, 4, 5, 4)]
    # smoothed with three taps: list 1's means 0.633, 0.6, 0.633, 0.567, 0.6 of rows 3..7 are above, 0.4 on either side is not: one
    # run; rows 3 and 5 share the greatest value but for their last bits, whichever np.convolve makes greater is the peak
    ev, sms = E.events(p1, 0.5, win=3)
    want = np.convolve(p1.astype(np.float64), np.ones(3) / 3, "same")
    assert np.array_equal(sms[0][0], want) and abs(want[4] - 0.6) < 1e-7 and abs(want[2] - 0.4) < 1e-7 and abs(want[8] - 0.4) < 1e-7
    assert len(ev) == 1 and ev[0][:4] == (0, 0, 3, 8) and ev[0][4] == 3 + int(np.argmax(want[3:8])) and ev[0][4] in (3, 5)
    assert ev[0][5] == want[ev[0][4]] and E.peak_gap(sms, ev[0]) < 1e-7


def test_restatement_hand_cases():
    one = np.float32(1.0)
    # a run to the segment's end and a run from the next segment's first row are two events; an empty segment has none
    p = np.array([0, 1, 1, 1, 1, 0, 0, 1], np.float32)
    ev, _ = E.events(p, 0.5, seg_offs=[0, 3, 3, 5, 8], win=0)
    assert ev == [(0, 0, 1, 3, 1, 1.0), (0, 2, 0, 2, 0, 1.0), (0, 3, 2, 3, 2, 1.0)]
    # one segment: the same rows are two events, and their number is the reference's count of rising edges
    ev, _ = E.events(p, 0.5, win=0)
    assert [e[2:4] for e in ev] == [(1, 5), (7, 8)]
    # a plateau: the first of equal greatest values; a later greater value moves the peak
    ev, _ = E.events(np.array([0.75, 0.75, 0.75], np.float32), 0.5, win=0)
    assert ev == [(0, 0, 0, 3, 0, 0.75)]
    ev, _ = E.events(np.array([0.6, 0.75, 0.75, 0.9, 0.9, 0.1], np.float32), 0.5, win=0)
    assert ev == [(0, 0, 0, 5, 3, _f32(0.9))]
    # a NaN row is not above: it ends a run
    ev, _ = E.events(np.array([1, np.nan, 1], np.float32), 0.5, win=0)
    assert [e[2:5] for e in ev] == [(0, 1, 0), (2, 3, 2)]
    # win = 2 takes rows i - 1 and i ((win - 1) // 2 = 0 rows ahead); win = 1 is the identity
    assert np.array_equal(E.smooth([one, 0, 0, one], 2), [0.5, 0.5, 0.0, 0.5])
    assert np.array_equal(E.smooth([one, 0, 0, one], 1), [1, 0, 0, 1])
    # a segment shorter than the window: the centre of the full convolution, clipped to the segment
    assert np.allclose(E.smooth([one, one, one], 30), [3 / 30] * 3, rtol=0, atol=1e-15)
    assert np.allclose(E.smooth(np.ones(20, np.float32), 30), (np.minimum(np.arange(20) + 14, 19) - np.maximum(np.arange(20) - 15, 0) + 1) / 30, rtol=0, atol=1e-15)
    # at least win rows: literally np.convolve 'same'
    x = np.random.default_rng(3).random(50).astype(np.float32)
    assert np.array_equal(E.smooth(x, 30), np.convolve(x.astype(np.float64), np.ones((30,)) / 30, mode="same"))
    ev, sms = E.events(x, 0.45)
    assert E.margin(sms, 0.45) > 0 and all(E.peak_gap(sms, e) >= 0 for e in ev)
    # the count is the reference's: rising edges of (smoothed > threshold)
    sm = sms[0][0]
    above = sm > 0.45
    assert len(ev) == int(above[0]) + int((above[1:] & ~above[:-1]).sum())
