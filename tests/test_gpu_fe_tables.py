"""logmel_rows_kernel (csrc/frontend.hip) with a constant table (the Hann half table) in a block of LDS that the waves of a
workgroup share: rows pinned bit for bit at the smallest batches at which that form can go wrong.

The workgroup fills the table block once and meets at ONE barrier before the first table read, so a wave without rows (past the
launch's last row, or with no valid row) must fetch its share, pass the barrier and store nothing; the workgroups of a launch go
round-robin over eight residues.  A workgroup is four waves of four frames:

  one_frame            one clip of 512 samples: one live row in wave 0, every other wave of the workgroup has none
  wg_plus_one          17 frames: a second workgroup whose first wave has one row and whose other waves have none
  two_wg_plus_one      33 frames: the same behind two full workgroups
  xcd_plus_one         132 frames: one workgroup per residue and one more, of one wave
  xcd_twice_plus_one   260 frames: two workgroups per residue and one more, of one wave with four rows
  three_clips          three clips of 147 frames: tiles cross clip boundaries (frame-by-frame staging) beside waves on the contiguous path
  no_frame_between     a clip too short for a frame between two clips that have frames
  ragged               ragged lengths (every call here goes through the offset-table search: uniform_nf = 0)
  f32                  float32 samples (ww_logmel_f32)
  preemph              pre-emphasis 0.97: the generic-staging instances (SIMPLE = false)

Every int16 case runs twice: through ``Engine.logmel`` (host buffers; 32-bit sample indices) and through ``Engine.logmel_dev``
(the 64-bit index instances, as tests/test_gpu_extents.py::test_front_end reaches them) with the mel buffer between guards of
16,384 floats - more than the rows of every surplus wave of these grids - which must stay untouched.  The host call stages its
output in a buffer of the library's own, and float32 samples have no device entry point: those runs (the f32 case altogether) have
no guards to put round the mel buffer.  What the guards watch, the exit of a wave without rows, is the same code in all six
instances.  Equal clips by arithmetic (uniform_nf > 0), where surplus waves now compute their row lookup in front of the barrier,
are not reached here: ww_clips_forward_dev returns no rows; tests/test_gpu_clips64.py pins that path against Engine.logmel.  The expected rows under tests/golden/fe_tables/ were recorded on
an MI355X with the library as it stood BEFORE the tables moved; comparison is ``assert_array_equal`` on the bits."""
import os

import numpy as np
import pytest

import extents as X

pytestmark = pytest.mark.gpu

SEED = 24
MEL_GUARD = 16384


def _samples(frames: int) -> int:
    return 512 + 160 * (frames - 1)


# name -> (clip lengths in samples, dtype, pre-emphasis)
CASES = {
    "one_frame": ((512,), np.int16, 0.0),
    "wg_plus_one": ((_samples(17),), np.int16, 0.0),
    "two_wg_plus_one": ((_samples(33),), np.int16, 0.0),
    "xcd_plus_one": ((_samples(132),), np.int16, 0.0),
    "xcd_twice_plus_one": ((_samples(260),), np.int16, 0.0),
    "three_clips": ((24000, 24000, 24000), np.int16, 0.0),
    "no_frame_between": ((1500, 300, 2000), np.int16, 0.0),
    "ragged": ((1500, 777, _samples(5), 511, 700, 5000, 513), np.int16, 0.0),
    "f32": ((3000, 1501, 512), np.float32, 0.0),
    "preemph": ((1500, 1500, 512, 1500), np.int16, 0.97),
}


def batch(name):
    """The case's clips: Gaussian noise of sigma 3000 (int16, or that / 32768 as float32), from SEED and the case's place in CASES."""
    lengths, dtype, _ = CASES[name]
    rng = np.random.default_rng([SEED, list(CASES).index(name)])
    clips = [np.clip(rng.normal(0, 3000, n), -32768, 32767).astype(np.int16) for n in lengths]
    return clips if dtype == np.int16 else [(c.astype(np.float32) / np.float32(32768.0)).astype(np.float32) for c in clips]


def params(name):
    from wwhip.engine import frontend_params
    return frontend_params(pre_emphasis=CASES[name][2])


def frames_of(name):
    return [(n - 512) // 160 + 1 if n >= 512 else 0 for n in CASES[name][0]]


@pytest.fixture(scope="module")
def engine(assets):
    from wwhip.engine import Engine
    e = Engine(os.path.join(assets, "CRNN"))
    yield e
    e.close()


def host_rows(e, name):
    got = e.logmel(batch(name), params(name))
    assert [g.shape for g in got] == [(f, 40) for f in frames_of(name)], name
    return np.concatenate(got)


def device_rows(e, name):
    """``logmel_dev`` on the case, the mel buffer between guards: (rows, the Guarded)."""
    import torch
    clips, frames = batch(name), frames_of(name)
    soffs = np.concatenate([[0], np.cumsum([len(c) for c in clips])]).astype(np.int64)
    foffs = np.concatenate([[0], np.cumsum(frames)]).astype(np.int64)
    total = int(foffs[-1])
    flat = np.concatenate(clips + [np.zeros(16, np.int16)])  # the padding the host form puts behind the last sample
    d_pcm, d_so, d_fo = torch.from_numpy(flat).cuda(), torch.from_numpy(soffs).cuda(), torch.from_numpy(foffs).cuda()
    assert d_pcm.data_ptr() % 16 == 0
    mel = X.Guarded(np.full((total, e.n_mel), X.SENTINEL, np.float32), X.SENTINEL, width=MEL_GUARD, device=True)
    torch.cuda.synchronize()
    e.logmel_dev(d_pcm.data_ptr(), d_so.data_ptr(), d_fo.data_ptr(), len(clips), total, max(frames), mel.ptr, params(name))
    e.ctx.synchronize()
    return mel.read(), mel


@pytest.mark.parametrize("name", list(CASES))
def test_rows_are_the_recorded_bits(engine, golden, name):
    """Both entry points give the rows recorded before the tables moved, and nothing is written outside them."""
    pinned = np.load(os.path.join(golden, "fe_tables", name + ".npy"))
    assert pinned.dtype == np.float32 and pinned.shape == (sum(frames_of(name)), 40) and np.isfinite(pinned).all()
    rows = host_rows(engine, name)
    np.testing.assert_array_equal(rows.view(np.uint32), pinned.view(np.uint32), err_msg=f"{name}: Engine.logmel")
    if CASES[name][1] == np.int16:
        dev, mel = device_rows(engine, name)
        mel.check_guards(f"{name}: logmel_dev")
        np.testing.assert_array_equal(dev.view(np.uint32), pinned.view(np.uint32), err_msg=f"{name}: logmel_dev")
