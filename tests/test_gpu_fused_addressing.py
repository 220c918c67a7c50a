"""crnn_fused_kernel (fp32) and crnn_fused_bf16_kernel on every shipped standard-geometry CRNN: the clip path at the sizes where
the staging and the conv change what they see, and explicit windows in the one-kernel form against front + either tail.

The fp32 kernels address W_x1 as a scalar k-step base + a 32-bit lane offset + an immediate (csrc/crnn.hip, PJ_W_KSTEP).  A wrong
W_x1 address or a wrong staging / conv offset gives garbage, not a last-bit difference, so the clip path is held to the C oracle
under the clip-path parity test's tolerance; the one-kernel form and the tails share one association of every sum (DESIGN.md
4.3), so their posteriors are equal bit for bit."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CRNNS = ["CRNN", "CRNN_softmax", "CRNN_nosilence", "CRNN_nosilence_enhanced"]
PRECISIONS = ["fp32", "bf16x3"]
TOL_POST = 1e-4   # tests/test_gpu_parity.py: test_clips_forward_dev
# one frame; 20 frames: the first size at which a conv position (t = 1: mel rows 2..21) sees no padding; the benchmark's
SAMPLES = (512, 3552, 24000)


@pytest.fixture(scope="module")
def engines(assets):
    from wwhip.engine import Engine
    out = {(m, p): Engine(os.path.join(assets, m), precision=p) for m in CRNNS for p in PRECISIONS}
    yield out
    for e in out.values():
        e.close()


@pytest.fixture(scope="module")
def clips():
    rng = np.random.default_rng(2710)
    return {s: np.clip(rng.normal(0, 2500, (3, s)), -32768, 32767).astype(np.int16) for s in SAMPLES}


@pytest.fixture(scope="module")
def clip_reference(engines, clips):
    """The C oracle's logmel + forward per clip, as bench.py's CPU path composes them; once per model."""
    from oracle.cpu import CpuOracle
    out = {}
    for m in CRNNS:
        e = engines[(m, "fp32")]
        ora = CpuOracle(e.blob)
        for s, pcm in clips.items():
            wins = np.zeros((len(pcm), e.window, 40), np.float32)
            for i, c in enumerate(pcm):
                mel = ora.logmel(c)
                n = min(len(mel), e.window)
                wins[i, :n] = mel[:n]
            out[(m, s)] = ora.forward(wins)
    return out


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", CRNNS)
def test_clip_path_against_oracle(engines, clips, clip_reference, name, precision):
    import torch
    from wwhip.engine import frontend_params
    e = engines[(name, precision)]
    assert e.is_crnn and e.window == 151
    for s in SAMPLES:
        want = clip_reference[(name, s)]
        for B in (1, 3):
            d_pcm = torch.from_numpy(clips[s][:B].copy()).cuda()
            d_out = torch.full((B, e.n_out), -1.0, dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            e.clips_forward_dev(d_pcm.data_ptr(), B, s, d_out.data_ptr(), frontend_params())
            e.ctx.synchronize()
            got = d_out.cpu().numpy()
            err = float(np.abs(got - want[:B]).max())
            print(f"\nFUSED-ADDR {name} {precision} {B} x {s} samples: max|dp| {err:.2e}", end="")
            assert np.isfinite(got).all()
            assert err < TOL_POST, (name, precision, B, s, err)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", CRNNS)
def test_explicit_windows_fused_head_equals_tail_head(engines, name, precision):
    """Five explicit windows, the last one partly valid: the one-kernel form against front + vector tail and front + matrix tail
    (each tail has a head of its own), bit for bit; anchored to the oracle on the zero-padded windows."""
    import torch
    from oracle.cpu import CpuOracle
    e = engines[(name, precision)]
    rng = np.random.default_rng(2711)
    T, rows = e.window, 300
    mel = rng.uniform(0, 6.5, (rows, 40)).astype(np.float32)
    win_row = np.array([0, 7, 40, 149, rows - 100], np.int64)
    win_valid = np.array([T, T, T, T, 100], np.int32)
    nw = len(win_row)
    d_mel = torch.from_numpy(mel).cuda()
    d_row, d_valid = torch.from_numpy(win_row).cuda(), torch.from_numpy(win_valid).cuda()

    def run():
        d_out = torch.full((nw, e.n_out), -1.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        e.forward_windows_dev(d_mel.data_ptr(), rows, d_row.data_ptr(), d_valid.data_ptr(), nw, d_out.data_ptr())
        e.ctx.synchronize()
        return d_out.cpu().numpy()

    with e.options(crnn_split_at=0):
        fused = run()
    assert np.isfinite(fused).all()
    for mfma in (0, 2):
        with e.options(crnn_split_at=1, crnn_tail_mfma=mfma):
            np.testing.assert_array_equal(run(), fused, err_msg=f"{name} {precision} tail_mfma {mfma}")
    wins = np.zeros((nw, T, 40), np.float32)
    for i, (r, v) in enumerate(zip(win_row, win_valid)):
        wins[i, :v] = mel[r:r + v]
    err = float(np.abs(fused - CpuOracle(e.blob).forward(wins)).max())
    print(f"\nFUSED-ADDR {name} {precision} explicit windows vs oracle: max|dp| {err:.2e}", end="")
    assert err < TOL_POST
