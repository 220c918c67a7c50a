"""The mel tail of the batch front ends (LM_MEL_REQ_* and LM_MEL_COMPUTE in csrc/frontend.hip: table fetches, filter, log and
park of a wave's 4 x n_mel tile), pinned bit for bit.

Every case runs ``Engine.logmel`` on a small batch regenerated from a seed and asserts ``array_equal`` with the rows recorded
under ``tests/golden/mel_tail/`` from the library as it stood before the tail's table fetches were moved, and agreement with
the float64 front end of oracle/ref64.py under the rule of tests/test_gpu_frontend64.py (its taus and its ``_logmel``).  The
batches are the smallest that reach each way through the tail: a wave with one valid row, a second wave that holds a single
row (the non-contiguous store), tiles that straddle clip boundaries (generic staging), a clip without a frame, both kernels
(``precise`` on: logmel_rows_kernel, off: logmel_kernel) and a filterbank whose bands cannot start on 16-byte boundaries
(``melv_aligned == 0``: the scalar-read branch), reached as tests/test_gpu_parity.py reaches it."""
import dataclasses
import os

import numpy as np
import pytest

from oracle import ref64 as R
from test_gpu_frontend64 import TAU_FFT, TAU_REL, TOL_SWEEP, _logmel

pytestmark = pytest.mark.gpu

SEED = 20
# name -> (clip lengths in samples, precise, filterbank)
CASES = {
    "one_frame": ((512,), True, "model"),
    "five_frames": ((512 + 4 * 160,), True, "model"),
    "three_clips": ((1500, 1500, 1500), True, "model"),
    "ragged_no_frame": ((1500, 300, 512 + 4 * 160, 511, 700), True, "model"),
    "five_frames_fast": ((512 + 4 * 160,), False, "model"),
    "three_clips_fast": ((1500, 1500, 1500), False, "model"),
    "unaligned_three_clips": ((1500, 1500, 1500), True, "unaligned"),
    "unaligned_three_clips_fast": ((1500, 1500, 1500), False, "unaligned"),
    "unaligned_five_frames": ((512 + 4 * 160,), True, "unaligned"),
}


def batch(name):
    """The case's clips: Gaussian noise of sigma 3000 as int16, from SEED and the case's place in CASES."""
    rng = np.random.default_rng([SEED, list(CASES).index(name)])
    return [np.clip(rng.normal(0, 3000, n), -32768, 32767).astype(np.int16) for n in CASES[name][0]]


def unaligned_bank():
    """The "unaligned" filterbank of tests/test_gpu_parity.py::test_logmel_with_other_filterbanks: the widest band has 36
    taps and starts on an odd bin, so pack_filter cannot round first bins down to multiples of 4."""
    rng = np.random.default_rng(91)
    w = np.zeros((40, 257), np.float32)
    for b, (s, n) in enumerate([(217, 36), (181, 34), (150, 31)] + [(3 * i + 1, 5 + i % 7) for i in range(37)]):
        w[b, s:s + n] = rng.uniform(0.05, 1.0, n).astype(np.float32)
    return w


def make_front_ends(assets):
    """filterbank name -> (Engine, the float64 front end on the same filter)."""
    from wwhip import weights as W
    from wwhip.engine import Engine
    path = os.path.join(assets, "CRNN")
    real = W.load_model_dir
    swapped = lambda p: (lambda b: dataclasses.replace(b, filt=dataclasses.replace(b.filt, weight=unaligned_bank())))(real(p))  # noqa: E731
    out = {"model": (Engine(path), R.FrontEnd64(path))}
    W.load_model_dir = swapped
    try:
        fe = R.FrontEnd64(path)
        out["unaligned"] = (Engine(path), fe)
    finally:
        W.load_model_dir = real
    assert np.array_equal(fe.filt.weight, unaligned_bank()) and not np.array_equal(out["model"][1].filt.weight, fe.filt.weight)
    return out


@pytest.fixture(scope="module")
def front_ends(assets):
    out = make_front_ends(assets)
    yield out
    for e, _ in out.values():
        e.close()


def run_case(front_ends, name):
    """(rows of every clip as Engine.logmel returned them, the float64 rows of every clip)."""
    from wwhip.engine import frontend_params
    lengths, precise, bank = CASES[name]
    e, fe = front_ends[bank]
    pcm = batch(name)
    got = e.logmel(pcm, frontend_params(precise=precise))
    want = [fe.logmel(p) for p in pcm]
    return got, want


@pytest.mark.parametrize("name", list(CASES))
def test_mel_tail_bits_and_float64(front_ends, golden, name):
    """Rows equal to the recorded ones bit for bit, and within the float64 rule.  Measured on an MI355X: no case needs any
    tau_rel or tau_fft (the rule's two ulps of the log cover them: max|dy| 3.2e-7 .. 5.1e-7 over the nine); every case
    array_equal with the recorded rows before the move and in each form of it that was measured."""
    lengths, precise, bank = CASES[name]
    got, want = run_case(front_ends, name)
    frames = [(n - 512) // 160 + 1 if n >= 512 else 0 for n in lengths]
    assert [g.shape for g in got] == [(f, 40) for f in frames] == [w.y.shape for w in want], name
    rows = np.concatenate(got)
    assert rows.dtype == np.float32 and np.isfinite(rows).all()
    pinned = np.load(os.path.join(golden, "mel_tail", name + ".npy"))
    assert pinned.dtype == np.float32 and pinned.shape == rows.shape
    _logmel(f"mel tail {name}", rows, R.LogMel64.concat(want), TAU_REL, 0.0 if precise else TAU_FFT, TOL_SWEEP if precise else None)
    assert np.array_equal(rows.view(np.uint32), pinned.view(np.uint32)), (name, int((rows != pinned).sum()), float(np.abs(rows - pinned).max()))
