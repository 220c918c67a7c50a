"""The clip path's two kernels where their tiling has edges.

Conv: the CRNN conv's K = 100 taps are 25 operand quads, six k-blocks of four quads and ONE last quad whose MFMA carries k = 96..99
in its four k-lanes (csrc/crnn.hip, CV_MFMA_LAST).  Every kernel that runs the conv - crnn_fused_kernel, <front> + either tail,
crnn_rows_kernel with all three weight sets - is checked against the C oracle and against each other, bit for bit.

Front end: logmel_rows_kernel's waves own four consecutive GLOBAL mel rows, so tiles run across clips.  Batches whose clip
boundaries fall inside a tile, between tiles and past the last row, on every staging path, against the float64 front end of
oracle/ref64.py under tests/test_gpu_frontend64.py's tolerances, and a clip alone against the same clip inside the batch."""
import os

import numpy as np
import pytest

from oracle import ref64 as R

pytestmark = pytest.mark.gpu

# Of the 7 model directories five hold a CRNN.  The first four have the standard geometry (32 channels, 5 x 20 taps, stride 2 x 8) and
# run the conv this file is about (CV_MFMA_LAST in crnn_fused_kernel, crnn_rows_kernel, crnn_stream_kernel).  CRNN_old has another
# conv geometry and goes through conv_generic_kernel + gemm_nt_kernel: it does not touch that code and rides along as a control.
CRNNS = ["CRNN", "CRNN_softmax", "CRNN_nosilence", "CRNN_nosilence_enhanced", "CRNN_old"]
TOL_MEL = 1e-4     # tests/test_gpu_parity.py: test_logmel_golden
TOL_POST = 1e-4    # tests/test_gpu_parity.py: test_forward_vs_oracle_batch
TAU_REL = 9e-7     # tests/test_gpu_frontend64.py: precise front end
TOL_SWEEP = 2e-5   # tests/test_gpu_frontend64.py: the absolute rule


@pytest.fixture(scope="module")
def engines(assets):
    from wwhip.engine import Engine
    out = {m: Engine(os.path.join(assets, m)) for m in CRNNS}
    yield out
    for e in out.values():
        e.close()


@pytest.fixture(scope="module")
def windows():
    """Five windows: random, all zeros, partial validity, negative values under the conv's last four time taps (input rows
    8 t + 10 .. 8 t + 13 for output position t), random."""
    rng = np.random.default_rng(1018)
    w = rng.uniform(0, 6.5, (5, 151, 40)).astype(np.float32)
    w[1] = 0
    w[2, 120:] = 0
    last_taps = np.nonzero((np.arange(151) % 8 >= 2) & (np.arange(151) % 8 <= 5))[0]
    w[3, last_taps] = -rng.uniform(0, 6.5, (len(last_taps), 40)).astype(np.float32)
    return w


# ---------------------------------------------------------------- conv
@pytest.mark.parametrize("name", CRNNS)
def test_conv_last_quad_every_dispatch(engines, windows, name):
    """Fused kernel against the C oracle; front + vector tail and front + matrix tail (crnn_split_at = 1) equal the fused kernel
    bit for bit."""
    from oracle.cpu import CpuOracle
    e = engines[name]
    assert e.is_crnn and e.window == 151
    want = CpuOracle(e.blob).forward(windows)
    with e.options(crnn_split_at=0):
        fused = e.forward(windows)
    err = float(np.abs(fused - want).max())
    print(f"\nCLIP-TRIMS {name} fused vs oracle: max|dp| {err:.2e}", end="")
    assert fused.shape == want.shape
    assert err < TOL_POST
    for mfma in (0, 2):
        with e.options(crnn_split_at=1, crnn_tail_mfma=mfma):
            np.testing.assert_array_equal(e.forward(windows), fused)


@pytest.mark.parametrize("name", CRNNS)
def test_conv_last_quad_rows_path(engines, name):
    """slide_forward at hop 8 over a 70-window sequence runs crnn_rows_kernel (interior fields and both edge weight sets) and a
    gathering tail (CRNN_old: the generic kernels, see CRNNS).  The rows path's own rule (tests/test_gpu_parity.py, test_crnn_sliding_rows_path_matches_per_window_kernels):
    both tails give the same bits, and the per-window kernels on the same windows agree within 2e-6; the oracle within 1e-4."""
    from oracle.cpu import CpuOracle
    e = engines[name]
    rng = np.random.default_rng(1019)
    T, hop, nw = e.window, 8, 70
    mel = rng.uniform(0, 6.5, ((nw - 1) * hop + T, 40)).astype(np.float32)
    mel[rng.integers(0, len(mel), 4)] = 0
    with e.options(crnn_tail_mfma=2):
        got = e.slide_forward(mel, hop)
    with e.options(crnn_tail_mfma=0):
        np.testing.assert_array_equal(e.slide_forward(mel, hop), got)
    assert got.shape[0] == nw
    wins = np.stack([mel[i * hop:i * hop + T] for i in range(nw)])
    with e.options(crnn_split_at=0):
        ref = e.forward(wins)
    # (not array_equal: the rows path's tails gather projected rows and associate the layer-1 sums as the per-window kernels
    # do, but its posteriors have differed from theirs in the last bits since before this conv - measured 2.4e-7 at most, on
    # the parent's library and on this one alike)
    d = float(np.abs(got - ref).max())
    print(f"\nCLIP-TRIMS {name} rows path vs fused: max|dp| {d:.2e}", end="")
    assert d < 2e-6
    idx = np.arange(0, nw, 7)
    assert np.abs(got[idx] - CpuOracle(e.blob).forward(wins[idx])).max() < TOL_POST


# ---------------------------------------------------------------- front end
def _clip(rng, n):
    return np.clip(rng.normal(0, 6000, n), -32768, 32767).astype(np.int16)


def _samples(frames):
    return 512 + 160 * (frames - 1)


def _batches():
    rng = np.random.default_rng(1020)
    ragged = [_clip(rng, _samples(f)) for f in (1, 3, 4, 5, 7, 8, 9, 13)] + [_clip(rng, 300)]
    equal = [_clip(rng, 24000) for _ in range(3)]
    odd = [_clip(rng, n) for n in (2001, 1777, 3333, 515, 999, 1231)]
    return {
        "a ragged": (ragged, (32767.0, True, 0.0, 160)),       # 50 rows: boundaries inside tiles and between them, a last tile of 2 rows
        # 3 x 147 rows = 441, equal clips through ww_logmel's offset tables (the equal-clips arithmetic, magic multiply included, is
        # ww_clips_forward_dev's alone: tests/test_gpu_clips64.py, test_logmel_equal_clips_arithmetic_lookup_equals_offset_tables)
        "b equal": (equal, (32767.0, True, 0.0, 160)),
        "c odd": (odd, (32768.0, True, 0.0, 160)),             # clips start at odd sample offsets
        "d generic": (ragged + odd, (32768.0, False, 0.97, 160)),  # pre-emphasis: generic staging
    }


@pytest.fixture(scope="module")
def ref(assets):
    return R.Ref64(os.path.join(assets, "CRNN"))


@pytest.mark.parametrize("case", list(_batches()))
def test_frontend_tiles_across_clips(engines, ref, case):
    from wwhip.engine import frontend_params
    e = engines["CRNN"]
    pcm, fpar = _batches()[case]
    fp = frontend_params(*fpar, True)
    got = e.logmel(pcm, fp)
    want = [ref.logmel(p, *fpar) for p in pcm]
    for g, w in zip(got, want):
        assert g.shape == w.y.shape
    assert got[-1].shape[0] == 0 or case != "a ragged"   # the 300-sample clip has no frame
    allg, allw = np.concatenate(got), R.LogMel64.concat(want)
    R.check_logmel(np.asarray(allg, np.float64), allw, TAU_REL, 0.0)
    assert np.abs(allg - allw.y).max() < TOL_SWEEP
    for i, p in enumerate(pcm):   # alone, the clip's rows sit in other tiles and waves
        np.testing.assert_array_equal(e.logmel([p], fp)[0], got[i])


def test_frontend_tiles_across_clips_float_input(engines, ref):
    from wwhip.engine import frontend_params
    e = engines["CRNN"]
    pcm = _batches()["a ragged"][0] + _batches()["c odd"][0]
    x = [p.astype(np.float32) / np.float32(12000.0) for p in pcm]
    fp = frontend_params(32767.0, True, 0.0, 160, True)
    got = e.logmel(x, fp)
    want = R.LogMel64.concat([ref.logmel_f32(v, 0.0, 160) for v in x])
    allg = np.concatenate(got)
    R.check_logmel(np.asarray(allg, np.float64), want, TAU_REL, 0.0)
    assert np.abs(allg - want.y).max() < TOL_SWEEP
    for i, v in enumerate(x):
        np.testing.assert_array_equal(e.logmel([v], fp)[0], got[i])


def test_frontend_golden_clips_in_one_batch(engines, golden):
    """The five clips tests/golden/frontend.npz holds log-mel for (147, 47, 22, 35 and 74 rows: 325 rows, clip boundaries at rows
    147, 194, 216, 251 - inside tiles) as one batch, with test_logmel_golden's two settings (the second: pre-emphasis, generic staging).  The golden rows are the float64 reference's values
    rounded to fp32, not this kernel's bits, so they are held to test_logmel_golden's rule; a clip alone equals the clip in the
    batch bit for bit."""
    from wwhip.engine import frontend_params
    e = engines["CRNN"]
    z = np.load(os.path.join(golden, "frontend.npz"))
    names = ["noise_chirp", "quiet", "silence", "fullscale", "ragged"]
    pcm = [z[n + ".pcm"] for n in names]
    for div, clip, pre in ((32767, True, 0.0), (32768, False, 0.97)):   # the two settings the golden rows were made with
        fp = frontend_params(float(div), clip, pre, 160, True)
        got = e.logmel(pcm, fp)
        for n, p, g in zip(names, pcm, got):
            want = z[f"{n}.div{div}.mel"]
            assert g.shape == want.shape, n
            d = float(np.abs(g - want).max())
            print(f"\nCLIP-TRIMS golden {n} div {div}: max|dy| {d:.2e}", end="")
            assert d < TOL_MEL, (n, d)
            np.testing.assert_array_equal(e.logmel([p], fp)[0], g)
