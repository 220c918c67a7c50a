"""csrc/ctc_score.h on the host: tests/native/ctc_score_check.cpp, a stand-alone program built with Address + UB sanitizer and run as a
child process (nothing is loaded into this interpreter), against the sequential float32 form of ``wwhip.ctc.score`` - the same
operations in the same order, so the same bits - on 3,000 seeded tables: T 1..64, L 2..12, U 1..9, repeated labels, a third of the
tables on a grid of sixteenths."""
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CSRC = os.path.join(_ROOT, "wakeword-detection_amd", "csrc")

N_RANDOM = 3000


def _no_sanitizer_runtime(output):
    """Did a -fsanitize build fail because this clang ships no runtime for it?  (tests/test_stream_rates_host.py's rule.)"""
    return re.search(r"libclang_rt\.|unsupported (option|argument)[^\n]*-fsanitize", output) is not None


def random_tables(seed: int = 20261, n: int = N_RANDOM):
    """``[(steps [T, L] float32, target)]``.  The first tables walk every (T, U) corner; a third lie on a grid of sixteenths (exact
    zeros and ties), a third carry a blank that wins often; every fourth target is one label repeated."""
    rng = np.random.default_rng(seed)
    corners = [(T, U) for T in (1, 2, 3, 17, 18, 19, 63, 64) for U in (1, 2, 8, 9)]
    out = []
    for i in range(n):
        T, U = corners[i] if i < len(corners) else (int(rng.integers(1, 65)), int(rng.integers(1, 10)))
        L = int(rng.integers(2, 13))
        s = rng.dirichlet(np.full(L, 0.4), T).astype(np.float32)
        if i % 3 == 0:
            s = np.round(s * 16) / np.float32(16)
        elif i % 3 == 1:
            s[:, L - 1] += np.float32(0.5)
        c = rng.integers(0, L - 1, U)
        if i % 4 == 0:
            c[:] = c[0]
        elif i % 4 == 1 and U >= 2:
            c[1] = c[0]
        out.append((np.ascontiguousarray(s, np.float32), tuple(int(v) for v in c)))
    return out


@pytest.fixture(scope="module")
def score_exe(tmp_path_factory):
    cxx = "/opt/rocm/lib/llvm/bin/clang++"
    if not os.path.exists(cxx):
        cxx = shutil.which("clang++")
    if cxx is None:
        pytest.skip("no clang++ in this image")
    d = tmp_path_factory.mktemp("ctc_score")
    exe = d / "ctc_score_check"
    b = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-I" + _CSRC,
                        os.path.join(_ROOT, "tests", "native", "ctc_score_check.cpp"), "-o", str(exe)], capture_output=True, text=True)
    if b.returncode != 0 and _no_sanitizer_runtime(b.stderr + b.stdout):
        pytest.skip("this clang has no sanitizer runtime: " + b.stderr[-300:])
    assert b.returncode == 0, b.stderr[-2000:]

    def run(tables, expect_ok=True):
        f = d / "tables.bin"
        with open(f, "wb") as fh:
            fh.write(struct.pack("<i", len(tables)))
            for steps, c in tables:
                fh.write(struct.pack("<iii", steps.shape[0], steps.shape[1], len(c)))
                fh.write(np.asarray(c, np.int32).tobytes())
                fh.write(np.ascontiguousarray(steps, np.float32).tobytes())
        r = subprocess.run([str(exe), str(f)], capture_output=True, text=True, timeout=120,
                           env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1"))
        if not expect_ok:
            return r
        assert r.returncode == 0 and not r.stderr.strip(), (r.returncode, r.stdout[-300:], r.stderr[-3000:])
        lines = r.stdout.strip().splitlines()
        assert lines[-1] == f"ok {len(tables)}" and len(lines) == len(tables) + 1, lines[-1]
        return np.array([[int(x, 16) for x in ln.split()] for ln in lines[:-1]], np.uint32)
    return run


def test_random_tables_carry_the_float32_statements_bits(score_exe):
    from wwhip import ctc
    tables = random_tables()
    got = score_exe(tables)
    zeros = positive = 0
    for i, ((steps, c), row) in enumerate(zip(tables, got)):
        want = [ctc.score(steps, [c], mode, np.float32)[0, 0] for mode in ("exact", "prefix")]
        assert row.tolist() == [int(np.float32(v).view(np.uint32)) for v in want], (i, steps.shape, c, row, want)
        zeros += want[0] == 0
        positive += want[0] > 0
    assert zeros > 100 and positive > 1000   # both: targets the steps cannot hold, and scores


def test_hand_cases(score_exe):
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import ctc64
    one_hot = ctc64._rows([3, 1, 1, 3, 3, 2, 2, 3], 4, hi=1.0)
    one = np.float32(1).view(np.uint32)
    got = score_exe([(one_hot, (1, 2)), (one_hot, (2, 1)), (one_hot, (1,)), (one_hot[:1], (1,)), (one_hot[:2], (1, 1))])
    assert got.tolist() == [[one, one], [0, 0], [0, one], [0, 0], [0, 0]]


def test_the_argument_check_refuses_what_the_entry_points_refuse(score_exe):
    y = np.full((3, 4), 0.25, np.float32)
    for steps, c, word in ((y, (3,), "label"), (y, (-1,), "label"), (np.full((65, 4), 0.25, np.float32), (0,), "T = 65"),
                           (np.full((3, 1), 1.0, np.float32), (0,), "L = 1"), (np.full((3, 65), 0.01, np.float32), (0,), "L = 65")):
        r = score_exe([(steps, c)], expect_ok=False)
        assert r.returncode == 2 and word in r.stderr, (c, r.stderr[-300:])
