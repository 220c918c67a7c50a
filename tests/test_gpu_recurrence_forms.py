"""The GRU step loop (csrc/crnn.hip: cf_recurrence) in every form that runs it, against the one that does not.

cf_recurrence is the body of crnn_fused_kernel, crnn_stream_kernel, crnn_fused_bf16_kernel and gru_tail_kernel: a wave's direction
and time position are scalar there, and the loop runs over pairs of steps.  gru_tail16_kernel (front + matrix tail) has a step
loop of its own on the matrix pipe and shares only the association of the sums, so it is the independent
reference: posteriors AND encodings of the three dispatch forms must be equal bit for bit.  The encodings are the last states of
the forward and the backward recurrence of layer 2 - a wrong direction, a wrong time order or a wrong ping-pong slot shows there
even where a saturated posterior hides it."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MODELS = ["CRNN", "CRNN_softmax"]            # sigmoid head (width 1), softmax head (width 2)
SET_MEMBERS = ["CRNN_nosilence", "CRNN_softmax"]
WINDOW_COUNTS = (1, 2, 3, 17)
TOL_POST = 1e-4   # tests/test_gpu_parity.py: test_stream_bank_matches_batch_path
FORMS = {"fused": {"crnn_split_at": 0}, "front + vector tail": {"crnn_split_at": 1, "crnn_tail_mfma": 0},
         "front + matrix tail": {"crnn_split_at": 1, "crnn_tail_mfma": 2}}


@pytest.fixture(scope="module")
def engines(assets):
    from wwhip.engine import Engine
    out = {m: Engine(os.path.join(assets, m)) for m in sorted(set(MODELS + SET_MEMBERS))}
    yield out
    for e in out.values():
        e.close()


def _windows(seed, nw, T, valid):
    """nw windows whose first `valid` rows hold log-mel-like values and whose other rows are zero (a partly valid window)."""
    rng = np.random.default_rng(seed)
    w = np.zeros((nw, T, 40), np.float32)
    w[:, :valid] = rng.uniform(0, 6.5, (nw, valid, 40)).astype(np.float32)
    return w


@pytest.mark.parametrize("nw", WINDOW_COUNTS)
@pytest.mark.parametrize("name", MODELS)
def test_dispatch_forms_equal_bits(engines, name, nw):
    """Default dispatch (the fused kernel at these sizes), front + vector tail, front + matrix tail: the same posteriors and the
    same encodings, at 1, 20, 147 and T valid rows.  The same windows through forward_windows_dev with the validity as a number
    (rows past it are not read at all) give those posteriors too, in every form."""
    import torch
    e = engines[name]
    T = e.window
    before = dict(e._options)
    for valid in (1, 20, 147, T):
        wins = _windows(1000 * nw + valid, nw, T, valid)
        ref_out, ref_enc = e.forward(wins, want_enc=True)   # default dispatch
        assert np.isfinite(ref_out).all() and np.isfinite(ref_enc).all()
        assert np.abs(ref_enc).max() > 0
        d_mel = torch.from_numpy(wins.reshape(-1, 40)).cuda()
        d_row = torch.arange(nw, dtype=torch.int64, device="cuda") * T
        d_valid = torch.full((nw,), valid, dtype=torch.int32, device="cuda")
        for form, opts in FORMS.items():
            with e.options(**opts):
                out, enc = e.forward(wins, want_enc=True)
                d_out = torch.full((nw, e.n_out), -1.0, dtype=torch.float32, device="cuda")
                torch.cuda.synchronize()
                e.forward_windows_dev(d_mel.data_ptr(), nw * T, d_row.data_ptr(), d_valid.data_ptr(), nw, d_out.data_ptr())
                e.ctx.synchronize()
            what = f"{name}, {nw} windows, {valid} valid rows, {form}"
            np.testing.assert_array_equal(out, ref_out, err_msg=what)
            np.testing.assert_array_equal(enc, ref_enc, err_msg=what)
            np.testing.assert_array_equal(d_out.cpu().numpy(), ref_out, err_msg=what + ", validity as a number")
    assert e._options == before


def test_model_set_batch_equals_single_model_calls(engines):
    """One model-set batch of 3 windows over 2 members (the SET instantiation of the fused kernel) against each member's own
    call: equal bits, posteriors and encodings."""
    from wwhip.engine import ModelSet
    ms = ModelSet([engines[m] for m in SET_MEMBERS])
    try:
        wins = _windows(77, 3, ms.window, ms.window)
        ids = np.array([0, 1, 0], np.int32)
        out, enc = ms.forward(wins, ids, want_enc=True)
        for k, m in enumerate(SET_MEMBERS):
            sel = ids == k
            want_out, want_enc = engines[m].forward(wins[sel], want_enc=True)
            np.testing.assert_array_equal(out[sel], want_out, err_msg=m)
            np.testing.assert_array_equal(enc[sel].reshape(want_enc.shape), want_enc, err_msg=m)
    finally:
        ms.close()


@pytest.mark.parametrize("name", MODELS)
def test_stream_bank_against_batch_path(engines, name):
    """A 4-stream bank for 40 ticks (crnn_stream_kernel: one window per stream and tick) against the batch path on the same rows:
    the batch front end's log-mel, windows sliding by one row from an all-zero window, Engine.forward.  The two front ends differ
    in their last bits, so the rule is test_stream_bank_matches_batch_path's: every posterior within TOL_POST."""
    from wwhip.engine import StreamBank
    e = engines[name]
    S, ticks, T = 4, 40, e.window
    rng = np.random.default_rng(43)
    pcm = np.clip(rng.normal(0, 2500, (S, ticks * 320)), -32768, 32767).astype(np.int16)
    bank = StreamBank(e, S)
    posts = [[] for _ in range(S)]
    speech = np.ones(S, np.uint8)
    for t in range(ticks):
        p, n = bank.step(pcm[:, t * 320:(t + 1) * 320], speech)
        for s in range(S):
            posts[s] += [float(p[s, k]) for k in range(n[s])]
    bank.close()
    mels = e.logmel(list(pcm))
    for s in range(S):
        hist = np.concatenate([np.zeros((T, 40), np.float32), mels[s]])
        wins = np.stack([hist[i:i + T] for i in range(1, len(mels[s]) + 1)])
        want = e.forward(wins)[:, e.posterior_index]
        assert len(posts[s]) == len(mels[s]) == len(want) > ticks
        err = float(np.abs(np.array(posts[s]) - want).max())
        print(f"\nRECURRENCE-FORMS {name} stream {s}: max|stream - batch| {err:.2e}", end="")
        assert err < TOL_POST, (name, s, err)
