"""``rnn64.Rnn64`` - the float64 reading of a CRNN of either cell - against two readings it shares no code with.

* On GRU / 32 bundles (``geometry64``'s rows) it is ``geometry64.Crnn64``, to 1e-14.
* Its recurrent layers are ``torch.nn.GRU`` / ``torch.nn.LSTM`` (double, bidirectional) on mapped weights for every (cell, H): torch's
  GRU gates are r, z, n with ``h = (1 - z) n + z h`` (the permutation z, r, h -> r, z, n) and both biases; torch's LSTM gates are
  i, f, g, o - Keras' order - with Keras' one bias in ``bias_ih`` and zeros in ``bias_hh``.  Bound 1e-13 (seen: 2e-16 / 5e-16 on a
  9-step, 48-unit case: the two differ by the association of a 48-term sum).
"""
import numpy as np
import pytest

import geometry64 as G
import rnn64 as R


@pytest.mark.parametrize("name", ["c-t150", "c-feat63", "c-one-step"])
def test_rnn64_is_crnn64_on_gru32(name):
    bundle = G.GEOMETRIES[name].bundle()
    assert bundle.crnn.cell == R.GRU and bundle.crnn.units == 32 and bundle.crnn.head_units == 64
    wins = G.row_windows(name, 5)
    p, e = R.Rnn64(bundle.crnn).forward(wins)
    p0, e0 = G.Crnn64(bundle.crnn).forward(wins)
    assert np.abs(e - e0).max() <= 1e-14 and np.abs(p - p0).max() <= 1e-14


def _torch_layer(cell, dirs, H, n_in):
    import torch
    net = (torch.nn.GRU if cell == R.GRU else torch.nn.LSTM)(n_in, H, batch_first=True, bidirectional=True).double()
    perm = np.r_[H:2 * H, 0:H, 2 * H:3 * H] if cell == R.GRU else np.arange(4 * H)   # z, r, h -> r, z, n; i, f, c, o as they are
    with torch.no_grad():
        for suffix, (w_x, b_x, w_h, b_h) in zip(("", "_reverse"), dirs):
            getattr(net, "weight_ih_l0" + suffix).copy_(torch.from_numpy(w_x[perm]))
            getattr(net, "weight_hh_l0" + suffix).copy_(torch.from_numpy(w_h[perm]))
            getattr(net, "bias_ih_l0" + suffix).copy_(torch.from_numpy(b_x[perm]))
            getattr(net, "bias_hh_l0" + suffix).copy_(torch.from_numpy(np.zeros_like(b_x) if b_h is None else b_h[perm]))
    return net


@pytest.mark.parametrize("cell", [R.GRU, R.LSTM])
@pytest.mark.parametrize("H", [16, 32, 48, 64])
def test_layers_are_torch_layers(cell, H):
    import torch
    bundle = R.synthetic_rnn(seed=400 + H + cell, cell=cell, H=H, F=64, T=20, n_mel=40, C=3, KF=8, KT=4, SF=8, ST=2, same=False, n_out=2, head=1)
    ref = R.Rnn64(bundle.crnn)
    assert bundle.crnn.out_t == 9
    feat = ref.features(G.windows(77, 3, 20, 40))
    seq = ref.sequences(feat)
    with torch.no_grad():
        want_seq, _ = _torch_layer(cell, ref.l1, H, feat.shape[2])(torch.from_numpy(feat))
        want2, _ = _torch_layer(cell, ref.l2, H, 2 * H)(torch.from_numpy(seq))
    want2 = want2.numpy()
    d1 = np.abs(seq - want_seq.numpy()).max()
    enc = np.concatenate([ref.layer(seq, ref.l2[0], False)[:, -1], ref.layer(seq, ref.l2[1], True)[:, 0]], axis=1)
    d2 = np.abs(enc - np.concatenate([want2[:, -1, :H], want2[:, 0, H:]], axis=1)).max()
    print(f"\nRNN64 cell {cell} H {H}: layer 1 differs from torch by {d1:.1e}, layer 2's last states by {d2:.1e}", end="")
    assert d1 <= 1e-13 and d2 <= 1e-13
    np.testing.assert_array_equal(enc, ref.encode(G.windows(77, 3, 20, 40)))


def test_rows_are_what_the_gpu_test_needs():
    """The ten device rows: all seven new (cell, H) pairs at the standard conv, the three heads, and the three edge convs."""
    std = [r for r in R.ROWS.values() if r.args["T"] == 151]
    assert sorted((r.args["cell"], r.args["H"]) for r in std) == sorted((c, h) for c in (0, 1) for h in (16, 32, 48, 64) if (c, h) != (0, 32))
    assert {(r.args["F"], r.args["head"], r.args["n_out"]) for r in std} >= {(64, 0, 1), (64, 1, 2), (40, 1, 8)}
    assert len(R.ROWS) <= 10
    steps = {n: R.ROWS[n].bundle().crnn.out_t for n in ("lstm48-one-step", "gru64-f1-feat63", "lstm64-two-steps")}
    assert steps == {"lstm48-one-step": 1, "gru64-f1-feat63": 30, "lstm64-two-steps": 2}
    assert R.ROWS["gru64-f1-feat63"].bundle().crnn.head_units == 1
