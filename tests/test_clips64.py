"""tests/clips64.py pinned on the CPU: the clip sets are deterministic, their float64 posteriors cross several logit units away
from both saturated ends (so that check_posteriors' relative term decides, not its fp32-ulp term), and the fp32 C oracle composed
the same way meets the float64 reference in logit space at every geometry of the table."""
import os

import numpy as np
import pytest

import clips64 as K
from oracle import ref64 as R
from oracle.cpu import CpuOracle
from wwhip import weights as W

MODELS = ["CRNN", "CRNN_softmax", "Wavenet"]
TAU_ORACLE = 2e-5   # tests/test_ref64.py: test_fp32_oracle_meets_the_float64_reference


@pytest.fixture(scope="module")
def refs(assets):
    oracles = {m: CpuOracle(W.pack_blob(W.load_model_dir(os.path.join(assets, m)))) for m in MODELS}
    return K.ClipRefs(oracles, {m: R.Ref64(os.path.join(assets, m)) for m in MODELS})


def test_geometry_table_reaches_what_it_names(refs):
    """Frame counts against the two window lengths: the rows named for nf = 0, 3, 4, T, T + 1 and nf > T have them."""
    for name, T in (("CRNN", 151), ("Wavenet", 182)):
        assert refs.oracles[name].window == T
        nf = {g: K.num_frames(K.geometry(g, T)[0], K.geometry(g, T)[4]) for g in K.GEOMETRY_IDS}
        assert (nf["a"], nf["b"], nf["c"], nf["d"], nf["e"], nf["f"], nf["g"], nf["h"]) == (0, 3, 4, 20, 147, T, T + 1, 197)
        assert (nf["i-24001"], nf["i-993"], nf["j"], nf["k-12001"], nf["k-16513"]) == (147, 4, 4, 144, 201)
        assert (nf["l"], nf["m"], nf["n"]) == (118, 46, 189)
        assert all(nf[g] > T for g in ("g", "h", "k-16513", "n"))
        # logmel_kernel's tiles of 16 frames per clip
        assert [(nf[g] + 15) // 16 for g in K.FAST_FRONTEND_IDS] == [1, 10, 13]
    assert len(K.PRECISE_IDS) == 16 and len(K.FAST_FRONTEND_IDS) == 3


@pytest.mark.parametrize("name", MODELS)
def test_clip_set_is_deterministic_and_sized(refs, name):
    ora = refs.oracles[name]
    for samples, n_clips in ((400, 24), (24001, 18), (32001, 16)):
        a = K.clip_set(ora, samples)
        assert a.dtype == np.int16 and a.shape == (n_clips, samples)
        K._STREAMS.clear()   # a second stream, built from scratch
        np.testing.assert_array_equal(K.clip_set(ora, samples), a)
    src = K.clip_stream(ora)
    np.testing.assert_array_equal(K.clip_set(ora, 993)[3], src[3 * K.STRIDE:3 * K.STRIDE + 993])


@pytest.mark.parametrize("name", MODELS)
def test_clip_posteriors_cross_the_decision_range(refs, name):
    """At the benchmark's length + 1 (e), at nf = T (f) and at 32,001 samples (h) the float64 posteriors of the clip set span at
    least 6 logit units, none above 1 - 1e-3 and none below 1e-7.  Measured logit ranges (e, f, h):
    CRNN -13.7 .. -1.7, -15.6 .. -0.9, -15.6 .. -0.9; CRNN_softmax -7.8 .. 4.2, -8.9 .. 3.3, -8.9 .. 3.3;
    Wavenet -6.7 .. 1.0, -6.7 .. 0.7, -6.7 .. 0.7 (f and h share their clips' first T frames, which is all the window sees)."""
    for gid in ("e", "f", "h"):
        p64 = refs.want64(name, gid)
        lo, hi = K.spans(p64)
        print(f"\nCLIPS64 {name} {gid}: logit {lo:.1f} .. {hi:.1f}, {len(p64)} clips", end="")
        assert hi - lo >= 6.0, (gid, lo, hi)
        post = p64[:, -1]   # (the posterior column, as in the ranges above; a two-column softmax row's other column is 1 - p)
        assert post.max() <= 1.0 - 1e-3 and post.min() >= 1e-7, (gid, post.min(), post.max())


@pytest.mark.parametrize("name", ["CRNN", "Wavenet"])
def test_zero_frame_clips_are_the_all_zero_window(refs, name):
    ora, ref = refs.oracles[name], refs.refs[name]
    want = ref.forward(np.zeros((1, ora.window, ora.n_mel), np.float32))[0][0]
    got = refs.want64(name, "a")
    assert len(got) == 24
    np.testing.assert_array_equal(got, np.broadcast_to(want, got.shape))


@pytest.mark.parametrize("name,gids", [("CRNN", K.GEOMETRY_IDS), ("Wavenet", K.GEOMETRY_IDS),
                                       ("CRNN_softmax", ["e", "f", "h", "i-24001"])])
def test_fp32_oracle_clip_path_meets_the_float64_reference(refs, name, gids):
    """CpuOracle.logmel -> zero-padded window -> CpuOracle.forward against Ref64.logmel -> window -> Ref64.forward on the whole
    clip set of every geometry, under the constant of test_fp32_oracle_meets_the_float64_reference.  Measured worst needed tau:
    CRNN 1.1e-5 (i-24001; 9.5e-6 at n, 9.1e-6 at l), Wavenet 2.1e-6 (i-24001), CRNN_softmax 7.8e-6 (e)."""
    ora = refs.oracles[name]
    worst = (-1.0, "")
    for gid in gids:
        samples, divisor, clip, pre, hop, _ = K.geometry(gid, ora.window)
        got = K.oracle_clip_posteriors(ora, K.clip_set(ora, samples), divisor, clip, pre, hop)
        want = refs.want64(name, gid)
        need = R.needed_tau(got, want)
        print(f"\nCLIPS64 {name} {gid}: C oracle needs tau {need:.2e}", end="")
        worst = max(worst, (need, gid))
        R.check_posteriors(got, want, tau=TAU_ORACLE)
    print(f"\nCLIPS64 {name}: worst {worst[0]:.2e} at {worst[1]}", end="")
