"""The prefix beam search on the MI355X: ctc_beam_kernel's bits against the host function of the same header
(``ww_ctc_beam_rows``), its strings and probabilities against the float64 statement (``wwhip.ctc.beam_search``) where float64
decides, the rows it writes, the model forms end to end, the evaluator's beam rule and the refusals.

Shapes: n = 1, 3, 5, 70 (four sequences share a workgroup: 5 leaves three dead waves); T = 1, 2, 19; L = 2 (every extension repeats
the last label) and 8; W = 1 (no partner), 2, 7 (no power of two), 64 (a full wave whose beam is not full in the first steps);
P = 1 and min(W, 8).  Bound: ``csrc/ctc_beam.h``'s derived (3T + 2) 2^-24, through ``wwhip.ctc.beam_rel_bound``."""
import os

import numpy as np
import pytest

import ctc64
import ctc_beam64 as B64

pytestmark = pytest.mark.gpu

SENT_I, SENT_F = -77, -7.0
PAD = 96


@pytest.fixture(scope="module")
def models():
    from wwhip.engine import Engine
    cache = {}

    def get(L):
        if L not in cache:
            b, wins, _, _ = ctc64.reference(L)
            e = Engine(f"synthetic-ctc-{L}", bundle=b)
            cache[L] = (e, wins, e.ctc_forward(wins, max_labels=19, want=("labels", "steps")))
        return cache[L]
    yield get
    for e, _, _ in cache.values():
        e.close()


def _beam_dev(e, steps, W, P, M, n=None):
    """``ctc_beam_dev`` on host posteriors ``[n, T, L]``: the outputs start as sentinels with ``PAD`` words behind rows ``[0, n)``,
    which must come back untouched."""
    import torch
    from wwhip.ctc import CtcBeam
    n0, T, L = steps.shape
    n = n0 if n is None else n
    d_steps = torch.from_numpy(np.ascontiguousarray(steps, np.float32)).cuda() if n0 else torch.zeros(1, device="cuda")
    d_lab = torch.full((n * P * M + PAD,), SENT_I, dtype=torch.int32, device="cuda")
    d_len = torch.full((n * P + PAD,), SENT_I, dtype=torch.int32, device="cuda")
    d_prob = torch.full((n * P + PAD,), SENT_F, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    e.ctc_beam_dev(d_steps.data_ptr(), n, T, L, W, P, M, d_lab.data_ptr(), d_len.data_ptr(), d_prob.data_ptr())
    e.ctx.synchronize()
    lab, ln, pr = d_lab.cpu().numpy(), d_len.cpu().numpy(), d_prob.cpu().numpy()
    assert (lab[n * P * M:] == SENT_I).all() and (ln[n * P:] == SENT_I).all() and (pr[n * P:] == SENT_F).all(), "written past row n"
    return CtcBeam(lab[:n * P * M].reshape(n, P, M), ln[:n * P].reshape(n, P), pr[:n * P].reshape(n, P))


# ---- 1: the kernel's bits ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 2, 19])
@pytest.mark.parametrize("L", [2, 8])
def test_kernel_bits_equal_the_host_function(models, T, L):
    from wwhip import ctc
    e = models(2)[0]
    rng = np.random.default_rng(100 * T + L)
    present = absent = 0
    for n in (1, 3, 5, 70):
        y = B64.tables(rng, n, T, L)
        y[n // 2] = B64.sixteenths(rng, 1, T, L)[0]
        for W in (1, 2, 7, 64):
            for P in sorted({1, min(W, 8)}):
                for M in sorted({1, T}):
                    got, want = _beam_dev(e, y, W, P, M), ctc.beam_rows(y, W, P, M)
                    B64.same_bits(got, want, f"n={n} T={T} L={L} W={W} P={P} M={M}")
                    present += int((want.lengths >= 0).sum())
                    absent += int((want.lengths < 0).sum())
    assert present > 0 and (absent > 0 or T > 1)   # (T = 1 holds at most L strings: places past them are absent)


def test_grid_of_sixteenths_ties_and_exact_zeros(models):
    from wwhip import ctc
    e = models(2)[0]
    rng = np.random.default_rng(16)
    ties = 0
    for L in (3, 4, 8):
        y = B64.sixteenths(rng, 70, 19, L)
        y[:8, 5:] = np.float32(1.0 / L)   # flat rows: many equal totals
        for W, P in ((2, 2), (7, 7), (64, 8)):
            got, want = _beam_dev(e, y, W, P, 19), ctc.beam_rows(y, W, P, 19)
            B64.same_bits(got, want, f"L={L} W={W}")
            ties += int((want.probs[:, :-1] == want.probs[:, 1:])[want.lengths[:, 1:] >= 0].sum()) if P > 1 else 0
    assert ties > 0


def test_zero_sequences_write_nothing(models):
    e = models(2)[0]
    got = _beam_dev(e, np.zeros((0, 19, 4), np.float32), 8, 2, 19)
    assert got.labels.size == 0


def test_nan_posteriors_reach_their_own_outputs_alone(models):
    from wwhip import ctc
    e = models(2)[0]
    rng = np.random.default_rng(6)
    for L, W, P in ((4, 8, 4), (8, 64, 8), (2, 1, 1)):
        y = B64.tables(rng, 70, 19, L)
        clean = _beam_dev(e, y, W, P, 19)
        y[33] = np.nan   # (every total of the sequence is NaN; one NaN row alone may be outranked by candidates of probability 0)
        got = _beam_dev(e, y, W, P, 19)
        host = ctc.beam_rows(y, W, P, 19)   # (the strings of a NaN sequence are the key order's; a NaN's own bits are not compared)
        np.testing.assert_array_equal(got.labels, host.labels)
        np.testing.assert_array_equal(got.lengths, host.lengths)
        np.testing.assert_array_equal(got.probs, host.probs)
        keep = np.arange(70) != 33
        B64.same_bits(type(got)(got.labels[keep], got.lengths[keep], got.probs[keep]),
                      type(got)(clean.labels[keep], clean.lengths[keep], clean.probs[keep]))
        assert np.isnan(got.probs[33]).any()


# ---- 2: against float64 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", ctc64.LS)
@pytest.mark.parametrize("W", [2, 8, 64])
def test_kernel_against_the_float64_statement_where_float64_decides(models, L, W):
    from wwhip import ctc
    e = models(2)[0]
    P = min(4, W)
    y = ctc64.reference(L)[2].astype(np.float32)
    bound = ctc.beam_rel_bound(19)
    trace = []
    want = ctc.beam_search(y, W, P, 19, np.float64, trace=trace)
    got = _beam_dev(e, y, W, P, 19)
    ok = B64.decidable(trace, W, P, bound)
    print(f"\nL={L} W={W}: {int((~ok).sum())} of {len(ok)} windows undecidable at 2 x (3T + 2) 2^-24", end="")
    assert (~ok).sum() <= 0.1 * len(ok)   # (a condition of the test, ctc64's convention - not a measurement)
    np.testing.assert_array_equal(got.labels[ok], want.labels[ok])
    np.testing.assert_array_equal(got.lengths[ok], want.lengths[ok])
    err = np.abs(got.probs[ok].astype(np.float64) - want.probs[ok])
    lim = bound * want.probs[ok] + 5 * 19 * 20 * 2.0 ** -126
    print(f"; worst probability error {float((err / lim).max()):.3f} of the bound", end="")
    assert (err <= lim).all()
    # the most probable string is not the collapse of the most probable path
    g_lab, g_len = ctc.greedy_decode(y, 19)
    differs = (got.lengths[:, 0] != g_len) | (got.labels[:, 0] != g_lab).any(axis=1)
    print(f"; top path differs from the greedy decode on {int(differs.sum())} windows", end="")
    assert differs.sum() >= 1


# ---- 3: the model forms ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", ctc64.LS)
@pytest.mark.parametrize("n", [1, 3, 70])
def test_engine_beam_is_the_kernel_on_the_engines_own_steps(models, L, n):
    e, wins, full = models(L)
    fwd = e.ctc_forward(wins[:n], max_labels=3, want=("steps",))
    np.testing.assert_array_equal(fwd.steps, full.steps[:n])
    for W, P, M in ((8, 4, 19), (64, 8, 5), (1, 1, 2)):
        want = _beam_dev(e, fwd.steps, W, P, M)
        got = e.ctc_beam(wins[:n], W, P, M)
        assert got.labels.shape == (n, P, M) and got.probs.dtype == np.float32
        B64.same_bits(got, want, f"L={L} n={n} W={W}")
    np.testing.assert_array_equal(e.ctc_beam(wins[:n], 8).labels.shape, (n, 1, 19))
    assert np.isfinite(e.ctc_beam(wins[:n], 8).log_probs).all()


@pytest.mark.parametrize("L", ctc64.LS)
def test_slide_and_windows_dev_forms(models, L):
    import torch
    import ctc_score64 as S64
    e, wins, full = models(L)
    mel, cut = S64.slide_mel(L), S64.slide_windows(L)
    got = e.ctc_slide_beam(mel, 2, 8, 3, 6)
    B64.same_bits(got, e.ctc_beam(cut, 8, 3, 6), "slide")
    assert e.ctc_slide_beam(mel[:150], 2, 8, 3, 6).labels.shape == (0, 3, 6)
    # descriptors on the same rows, into sentinel-filled buffers
    n, T, F = wins.shape
    W, P, M = 8, 2, 4
    d_mel = torch.from_numpy(wins.reshape(-1, F)).cuda()
    d_row, d_valid = torch.from_numpy(np.arange(n, dtype=np.int64) * T).cuda(), torch.full((n,), T, dtype=torch.int32, device="cuda")
    d_lab = torch.full((n * P * M + PAD,), SENT_I, dtype=torch.int32, device="cuda")
    d_len = torch.full((n * P + PAD,), SENT_I, dtype=torch.int32, device="cuda")
    d_prob = torch.full((n * P + PAD,), SENT_F, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    e.ctc_beam_windows_dev(d_mel.data_ptr(), n * T, d_row.data_ptr(), d_valid.data_ptr(), n, W, P, M, d_lab.data_ptr(), d_len.data_ptr(), d_prob.data_ptr())
    e.ctx.synchronize()
    lab, ln, pr = d_lab.cpu().numpy(), d_len.cpu().numpy(), d_prob.cpu().numpy()
    assert (lab[n * P * M:] == SENT_I).all() and (ln[n * P:] == SENT_I).all() and (pr[n * P:] == SENT_F).all()
    want = e.ctc_beam(wins, W, P, M)
    B64.same_bits(type(want)(lab[:n * P * M].reshape(n, P, M), ln[:n * P].reshape(n, P), pr[:n * P].reshape(n, P)), want, "windows_dev")


def test_evaluate_ctc_with_a_beam_applies_the_rule_to_the_top_path(models):
    from wwhip import ctc
    from wwhip.evaluate import evaluate_ctc
    e, wins, _ = models(4)
    rng = np.random.default_rng(11)
    lens = rng.integers(60, 201, 40)
    long = np.concatenate([wins[i] for i in range(40, 44)])
    clips = [long[o:o + n].copy() for o, n in zip(rng.integers(0, len(long) - 200, 40), lens)]
    hot = rng.integers(0, 2, 40)
    padded = np.zeros((40, 151, 40), np.float32)
    for i, c in enumerate(clips):
        padded[i, :min(len(c), 151)] = c[:151]
    top = e.ctc_beam(padded, 8, 1, 2)
    want = ctc.is_wakeword(top.labels[:, 0], top.lengths[:, 0])
    got = evaluate_ctc(e, clips, hot, beam_width=8)
    np.testing.assert_array_equal(np.asarray(got["predicted"]).astype(bool), want)
    np.testing.assert_array_equal(got["beam_probs"].view(np.uint32), top.probs[:, 0].view(np.uint32))
    assert "beam_probs" not in evaluate_ctc(e, clips, hot)


# ---- 4: refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_come_before_anything_is_written(models, assets):
    import torch
    from wwhip import _lib, ctc
    from wwhip.engine import Engine
    e, wins, _ = models(4)
    d_steps = torch.full((4, 19, 4), 0.25, dtype=torch.float32, device="cuda")
    d_lab = torch.full((4 * 8 * 19,), SENT_I, dtype=torch.int32, device="cuda")
    d_len = torch.full((64,), SENT_I, dtype=torch.int32, device="cuda")
    d_prob = torch.full((64,), SENT_F, dtype=torch.float32, device="cuda")
    cases = [(dict(T=0), "T = 0"), (dict(T=20), "T = 20"), (dict(L=1), "L = 1"), (dict(L=9), "L = 9"), (dict(W=0), "beam_width = 0"),
             (dict(W=65), "beam_width = 65"), (dict(P=0), "top_paths = 0"), (dict(P=9), "top_paths = 9"), (dict(W=3, P=4), "top_paths = 4"),
             (dict(M=0), "max_labels = 0"), (dict(M=20), "max_labels = 20"), (dict(lab=None), "NULL"), (dict(prob=None), "NULL"), (dict(steps=None), "NULL")]
    for kw, word in cases:
        a = dict(T=19, L=4, W=8, P=2, M=19, steps=d_steps.data_ptr(), lab=d_lab.data_ptr(), ln=d_len.data_ptr(), prob=d_prob.data_ptr())
        a.update(kw)
        rc = e._lib.ww_ctc_beam_dev(e.ctx.handle, a["steps"], 4, a["T"], a["L"], a["W"], a["P"], a["M"], a["lab"], a["ln"], a["prob"])
        text = (e._lib.ww_last_error(e.ctx.handle) or b"").decode()
        assert rc == _lib.WW_EINVAL and word in text and "ww_ctc_beam_dev" in text, (kw, rc, text)
    e.ctx.synchronize()
    assert (d_lab.cpu().numpy() == SENT_I).all() and (d_len.cpu().numpy() == SENT_I).all() and (d_prob.cpu().numpy() == SENT_F).all()
    # the model forms: the same rules, and the model itself
    lab, ln, pr = np.full((3, 8, 19), SENT_I, np.int32), np.full((3, 8), SENT_I, np.int32), np.full((3, 8), SENT_F, np.float32)
    for W, P, M, word in ((0, 1, 19, "beam_width"), (65, 1, 19, "beam_width"), (8, 9, 19, "top_paths"), (2, 3, 19, "top_paths"), (8, 1, 20, "max_labels")):
        rc = e._lib.ww_ctc_beam(e.ctx.handle, e.handle, _lib.ptr(wins[:3]), 3, W, P, M, _lib.ptr(lab), _lib.ptr(ln), _lib.ptr(pr))
        assert rc == _lib.WW_EINVAL and word in (e._lib.ww_last_error(e.ctx.handle) or b"").decode(), (W, P, M)
    assert e._lib.ww_ctc_beam(e.ctx.handle, e.handle, _lib.ptr(wins[:3]), 3, 8, 1, 19, _lib.ptr(lab), None, _lib.ptr(pr)) == _lib.WW_EINVAL
    assert (lab == SENT_I).all() and (ln == SENT_I).all() and (pr == SENT_F).all()
    with pytest.raises(ValueError, match="beam_width"):
        e.ctc_beam(wins[:3], 65)
    # split-bf16 mode and a model that is no CTC model
    e.set_precision("bf16x3")
    try:
        with pytest.raises(ValueError):
            e.ctc_beam(wins[:3], 8)
        with pytest.raises(ValueError):
            e.ctc_slide_beam(np.zeros((200, 40), np.float32), 2, 8)
    finally:
        e.set_precision("fp32")
    plain = Engine(os.path.join(assets, "CRNN_softmax"))
    try:
        with pytest.raises(ValueError, match="not a CTC"):
            plain.ctc_beam(np.zeros((1, plain.window, plain.n_mel), np.float32), 8)
        # the kernel alone takes any posteriors, whatever the engine's model
        y = np.full((3, 5, 4), 0.25, np.float32)
        B64.same_bits(_beam_dev(plain, y, 8, 2, 5), ctc.beam_rows(y, 8, 2, 5))
    finally:
        plain.close()
