"""The yardsticks of tests/test_gpu_geometry64.py, pinned on the CPU (no GPU, no HIP library).

``geometry64.Crnn64`` - the CRNN in float64 written from ``CrnnParams`` - against ``oracle.ref64.Ref64``, the op-by-op reading of
the shipped flatbuffers; every row of ``geometry64.GEOMETRIES`` against the fp32 C oracle, which reads the packed blob by section
name in C and shares nothing with geometry64.py; and the conditions that keep the rows' windows useful (posteriors away from
saturation, encoder outputs not mostly zero)."""
import os

import numpy as np
import pytest

import geometry64 as G
from oracle import ref64 as R

TOL64 = 2e-14      # Crnn64 against Ref64: two float64 evaluations in different summation orders, 10x the worst measured (1.7e-15)
TOL_ORACLE = 1e-4  # float64 against the fp32 C oracle, absolute, posteriors and encodings


@pytest.mark.parametrize("name", ["CRNN", "CRNN_softmax", "CRNN_old"])
def test_crnn64_is_ref64_on_the_shipped_models(assets, name):
    """Posteriors and encodings of the shipped CRNNs: Crnn64 from load_model_dir's parameters against Ref64 on the same windows.
    Measured: posterior 2.2e-16 (CRNN_softmax), encoding 1.7e-15 (CRNN_old); the bound is 10x the worst, 2e-14."""
    from wwhip import weights as W
    d = os.path.join(assets, name)
    b = W.load_model_dir(d)
    wins = np.concatenate([G.windows(31, 5, b.crnn.n_frames, 40), np.zeros((1, b.crnn.n_frames, 40), np.float32)])
    post, enc = G.Crnn64(b.crnn).forward(wins)
    out64, enc64 = R.Ref64(d).forward(wins)
    dp, de = np.abs(post - out64).max(), np.abs(enc - enc64.reshape(enc.shape)).max()
    print(f"\nGEOMETRY64 {name}: Crnn64 - Ref64 posterior {dp:.2e}, encoding {de:.2e}", end="")
    assert dp <= TOL64 and de <= TOL64


@pytest.fixture(scope="module")
def refs():
    """row -> (bundle, windows, post64, enc64), once per module."""
    cache = {}

    def get(name):
        if name not in cache:
            b = G.GEOMETRIES[name].bundle()
            wins = G.row_windows(name)
            cache[name] = (b, wins) + G.reference(b).forward(wins)
        return cache[name]
    return get


@pytest.mark.parametrize("name", list(G.GEOMETRIES))
def test_geometries_are_what_the_table_says(name):
    g = G.GEOMETRIES[name]
    b = g.bundle()
    if g.kind == "crnn":
        c = b.crnn
        want = {"c-std-n8": (20, 19, 640), "c-std-n3-sigmoid": (20, 19, 640), "c-t150": (20, 19, 640), "c-one-step": (1, 1, 1),
                "c-feat63": (9, 30, 63), "c-feat65": (5, 12, 65), "c-c64": (9, 31, 576), "c-lds-limit": (16, 64, 48)}[name]
        assert (c.out_f, c.out_t, c.out_f * c.conv_w.shape[0]) == want
        assert c.n_frames * c.n_mel <= 16384 and c.units == 32
        if name == "c-t150":
            assert (c.pad_f, c.pad_t) == ((1, 2), (7, 7))
        if name == "c-lds-limit":
            assert c.n_frames * c.n_mel == 16384 and b.filt.n_mel == 32
        standard = (c.conv_w.shape, c.n_mel, c.n_frames, c.stride_f, c.stride_t, c.pad_f[0], c.pad_t[0]) == ((32, 5, 20), 40, 151, 2, 8, 1, 6)
        assert standard == g.standard
    else:
        w = b.wavenet
        assert w.channels == 16 and w.skip_channels == 32 and w.skip_order == list(range(len(w.blocks)))
        assert 1 <= w.n_frames <= 192 and 1 <= len(w.blocks) <= 32 and all(1 <= k.dilation <= 8 for k in w.blocks)
    assert b.filt.n_mel == g.n_mel and b.n_out == g.n_out


@pytest.mark.parametrize("name", [n for n, g in G.GEOMETRIES.items() if G.oracle_takes(g)])
def test_float64_against_the_c_oracle(refs, name):
    """The independent reading of the blob: CpuOracle(blob_of(bundle)).forward within 1e-4 absolute of the float64 reference,
    posteriors and encodings.  Measured: 4.2e-7 / 9.5e-6 at the worst (w-t183, both; the CRNN rows 2.9e-7 / 4.3e-7)."""
    from oracle.cpu import CpuOracle
    from wwhip import weights as W
    b, wins, post64, enc64 = refs(name)
    out, enc = CpuOracle(G.blob_of(b)).forward(wins, want_enc=True)
    dp, de = np.abs(out - post64).max(), np.abs(enc.reshape(enc64.shape) - enc64).max()
    print(f"\nGEOMETRY64 {name}: oracle - float64 posterior {dp:.2e}, encoding {de:.2e}", end="")
    assert dp < TOL_ORACLE and de < TOL_ORACLE


def test_the_oracle_leaves_out_only_w_max():
    assert [n for n, g in G.GEOMETRIES.items() if not G.oracle_takes(g)] == ["w-max"]


@pytest.mark.parametrize("name", list(G.GEOMETRIES))
def test_the_inputs_stay_useful(refs, name):
    """On the float64 reference alone, for the windows the GPU tests run: min(p, 1 - p) of the posterior_index column is >= 1e-3 in
    at least 90 % of the windows, and at least half of the encoder entries are non-zero.  w-t100-odd (NOUT 1: its posterior is
    identically 1) is exempt from the first and is checked through logits and encodings on the GPU."""
    b, wins, post64, enc64 = refs(name)
    assert np.isfinite(post64).all() and np.isfinite(enc64).all()
    p = post64[:, b.posterior_index]
    tail = np.minimum(p, 1.0 - p)
    live = float((enc64 != 0).mean())
    print(f"\nGEOMETRY64 {name}: p in [{p.min():.4f}, {p.max():.4f}], {float((tail >= 1e-3).mean()):.0%} of tails >= 1e-3, "
          f"{live:.0%} of the encoder non-zero, max|enc| {np.abs(enc64).max():.3g}", end="")
    if name == "w-t100-odd":
        assert (post64 == 1.0).all()
    else:
        assert (tail >= 1e-3).mean() >= 0.9
    assert live >= 0.5
