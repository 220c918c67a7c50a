"""CTC-trained CRNNs on the MI355X: gru_tail_ctc_kernel's posteriors and layer-2 sequence against float64 (tests/ctc64.py), its decode
against the numpy statement - exactly -, the invariances of the launch forms, the evaluator, and the refusals both ways.

Shapes: the standard geometry (T = 151, 40 bands), L = 2, 4, 8 classes, n = 1, 3, 70 windows (``ctc64.windows``).  Bounds are the
project's constants for the same recurrences (tests/test_gpu_ref64.py); the needed values are printed (``pytest -s``)."""
import ctypes as C
import os

import numpy as np
import pytest

import ctc64
from oracle import ref64 as R

pytestmark = pytest.mark.gpu

TAU, TAU_E = ctc64.TAU, ctc64.TAU_E
ALL = ("labels", "steps", "enc")
SENT = -7.0


class Model:
    def __init__(self, L):
        from wwhip.engine import Engine
        self.L = L
        self.bundle, self.wins, self.steps64, self.enc64 = ctc64.reference(L)
        self.engine = Engine(f"synthetic-ctc-{L}", bundle=self.bundle)
        self.full = self.engine.ctc_forward(self.wins, max_labels=19, want=ALL)

    def close(self):
        self.engine.close()


@pytest.fixture(scope="module")
def models():
    cache = {}

    def get(L):
        if L not in cache:
            cache[L] = Model(L)
        return cache[L]
    yield get
    for m in cache.values():
        m.close()


def _same(a, b, what):
    for name in ("labels", "lengths", "steps", "enc"):
        x, y = getattr(a, name), getattr(b, name)
        if x is not None and y is not None:
            np.testing.assert_array_equal(x, y, err_msg=f"{what}: {name}")


def _row(res, i):
    from wwhip.ctc import CtcResult
    return CtcResult(*[None if a is None else a[i:i + 1] for a in res])


def _windows_dev(e, mel, rows, valid, max_labels=19):
    """``ctc_forward_windows_dev`` over descriptors; every output buffer starts as a sentinel."""
    import torch
    from wwhip.ctc import CtcResult
    n, L = len(rows), e.n_out
    d_mel = torch.from_numpy(np.ascontiguousarray(mel, np.float32)).cuda()
    d_row, d_valid = torch.from_numpy(np.asarray(rows, np.int64)).cuda(), torch.from_numpy(np.asarray(valid, np.int32)).cuda()
    d_lab = torch.full((n, max_labels), -9, dtype=torch.int32, device="cuda")
    d_len = torch.full((n,), -9, dtype=torch.int32, device="cuda")
    d_steps = torch.full((n, 19, L), SENT, dtype=torch.float32, device="cuda")
    d_enc = torch.full((n, 19, 64), SENT, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    e.ctc_forward_windows_dev(d_mel.data_ptr(), d_mel.shape[0], d_row.data_ptr(), d_valid.data_ptr(), n, max_labels, d_lab.data_ptr(),
                              d_len.data_ptr(), d_steps.data_ptr(), d_enc.data_ptr())
    e.ctx.synchronize()
    return CtcResult(d_lab.cpu().numpy(), d_len.cpu().numpy(), d_steps.cpu().numpy(), d_enc.cpu().numpy())


# ---- 1: against float64 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", ctc64.LS)
def test_steps_and_enc_against_float64(models, L):
    m = models(L)
    assert m.engine.is_ctc and m.engine.head_kind == 2 and m.engine.n_out == L and m.engine.enc_shape == (19, 64)
    got, want = m.full.steps, m.steps64
    assert got.shape == want.shape and np.isfinite(got).all() and got.min() >= 0.0 and got.max() <= 1.0
    need_e = float(R.enc_ratios(m.full.enc, m.enc64, 1.0).max())
    print(f"\nCTC L={L}: posteriors need tau {R.needed_tau(got.reshape(-1, L), want.reshape(-1, L)):.2e} (tau {TAU:g}), max|dp| "
          f"{np.abs(got - want).max():.2e}; layer-2 sequence needs tau_e {need_e:.2e} (tau_e {TAU_E:g})", end="")
    R.check_posteriors(got.reshape(-1, L), want.reshape(-1, L), TAU)
    R.check_enc(m.full.enc, m.enc64, TAU_E)
    np.testing.assert_allclose(got.sum(axis=2), 1.0, atol=4e-7)


# ---- 2: the decode, exactly ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", ctc64.LS)
@pytest.mark.parametrize("max_labels", [19, 2, 1])
def test_decode_is_the_numpy_statement_of_the_engines_own_steps(models, L, max_labels):
    import torch
    from wwhip import ctc
    m = models(L)
    res = m.full if max_labels == 19 else m.engine.ctc_forward(m.wins, max_labels=max_labels, want=("labels", "steps"))
    np.testing.assert_array_equal(res.steps, m.full.steps)
    labels, lengths = ctc.greedy_decode(res.steps, max_labels)
    np.testing.assert_array_equal(res.labels, labels)
    np.testing.assert_array_equal(res.lengths, lengths)
    # the decode alone (ww_ctc_greedy_dev) on the same posteriors
    n = len(m.wins)
    d_steps = torch.from_numpy(res.steps).cuda()
    d_lab = torch.full((n, max_labels), -9, dtype=torch.int32, device="cuda")
    d_len = torch.full((n,), -9, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    m.engine.ctc_greedy_dev(d_steps.data_ptr(), n, 19, L, max_labels, d_lab.data_ptr(), d_len.data_ptr())
    m.engine.ctx.synchronize()
    np.testing.assert_array_equal(d_lab.cpu().numpy(), labels)
    np.testing.assert_array_equal(d_len.cpu().numpy(), lengths)


def test_greedy_dev_on_other_shapes(models):
    """T and L beyond the model's: T = 1 and 4096, L = 2 and 64, ties included (values on a grid of eighths)."""
    import torch
    from wwhip import ctc
    e = models(2).engine
    rng = np.random.default_rng(5)
    for n, T, L, M in ((3, 1, 2, 1), (2, 4096, 64, 4096), (130, 37, 5, 7), (65, 19, 64, 19)):
        s = (np.round(rng.random((n, T, L)) * 8) / 8).astype(np.float32)
        d_steps = torch.from_numpy(s).cuda()
        d_lab = torch.full((n, M), -9, dtype=torch.int32, device="cuda")
        d_len = torch.full((n,), -9, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        e.ctc_greedy_dev(d_steps.data_ptr(), n, T, L, M, d_lab.data_ptr(), d_len.data_ptr())
        e.ctx.synchronize()
        labels, lengths = ctc.greedy_decode(s, M)
        np.testing.assert_array_equal(d_lab.cpu().numpy(), labels)
        np.testing.assert_array_equal(d_len.cpu().numpy(), lengths)


# ---- 3: against the float64 decode, where float64 decides -----------------------------------------------------------------------------------
@pytest.mark.parametrize("L", ctc64.LS)
def test_labels_against_float64_on_decidable_windows(models, L):
    m = models(L)
    d = ctc64.decidable(m.steps64)
    assert (~d).sum() <= 0.1 * len(d)
    labels64, lengths64 = ctc64.decode64(m.steps64, 19)
    assert (lengths64 >= 2).any() and (lengths64 == 0).any()
    print(f"\nCTC L={L}: {int((~d).sum())} of {len(d)} windows undecidable; decoded lengths {np.bincount(lengths64).tolist()}", end="")
    np.testing.assert_array_equal(m.full.labels[d], labels64[d])
    np.testing.assert_array_equal(m.full.lengths[d], lengths64[d])


# ---- 4: invariance ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", ctc64.LS)
def test_batch_size_and_descriptors(models, L):
    m = models(L)
    e = m.engine
    _same(e.ctc_forward(m.wins[:1], 19, ALL), _row(m.full, 0), "n = 1 against row 0 of n = 70")
    three = e.ctc_forward(m.wins[:3], 19, ALL)
    for i in range(3):
        _same(_row(three, i), _row(m.full, i), f"n = 3, row {i}")
    n, T, F = m.wins.shape
    dev = _windows_dev(e, m.wins.reshape(-1, F), np.arange(n) * T, np.full(n, T))
    _same(dev, m.full, "descriptors on the same rows")
    assert (dev.steps != SENT).all() and (dev.enc != SENT).all() and (dev.lengths >= 0).all()


@pytest.mark.parametrize("L", [4])
def test_partial_clip_is_zero_padded_on_the_device(models, L):
    m = models(L)
    e = m.engine
    T, F = m.wins.shape[1:]
    clip = m.wins[5].copy()                   # rows 100.. hold other values than zero in the mel buffer: they must not be read
    padded = clip.copy()
    padded[100:] = 0.0
    dev = _windows_dev(e, np.concatenate([clip, m.wins[6]]), [0, 0, T], [100, T, T])
    _same(_row(dev, 0), e.ctc_forward(padded[None], 19, ALL), "100 valid rows against the rows zero-padded by hand")
    _same(_row(dev, 1), _row(m.full, 5), "the whole clip")
    _same(_row(dev, 2), _row(m.full, 6), "the next clip")
    assert not np.array_equal(dev.steps[0], dev.steps[1])


@pytest.mark.parametrize("L", ctc64.LS)
def test_slide_forms_agree_with_cut_windows(models, L):
    """300 rows at hop 2 = 75 windows, on both sides of crnn_slide_min (64, the default: where the other heads take crnn_rows_kernel;
    0 = never), against the windows cut out and given to ctc_forward: the same bits.  The library keeps that promise by running
    ONE front kernel either way (crnn_rows_kernel's projected rows differ from it in their last bits), which the profile shows."""
    m = models(L)
    e = m.engine
    mel = np.concatenate([m.wins[7], m.wins[8]])[:300]
    cut = np.stack([mel[i:i + 151] for i in range(0, 300 - 151 + 1, 2)])
    assert len(cut) == 75
    want = e.ctc_forward(cut, 3, ("labels", "steps"))
    e.ctx.profile(True)
    rows_form = e.ctc_slide_forward(mel, 2, 3, ("labels", "steps"))
    prof_rows = e.ctx.profile_read()
    with e.options(crnn_slide_min=0):
        front_form = e.ctc_slide_forward(mel, 2, 3, ("labels", "steps"))
    prof_front = e.ctx.profile_read()
    e.ctx.profile(False)
    for prof in (prof_rows, prof_front):
        assert sorted(prof) == ["crnn_fused_kernel<front>", "gru_tail_ctc_kernel"], prof
    _same(rows_form, want, "sliding, slide_min 64")
    _same(front_form, want, "sliding, slide_min 0")
    short = e.ctc_slide_forward(mel[:150], 2)
    assert short.labels.shape == (0, 2) and short.lengths.shape == (0,)


# ---- 5: the evaluator ------------------------------------------------------------------------------------------------------------------
def test_evaluate_ctc_is_the_per_clip_path(models):
    from wwhip import ctc
    from wwhip.evaluate import ctc_statistics, evaluate_ctc
    m = models(4)
    e = m.engine
    rng = np.random.default_rng(11)
    lens = rng.integers(60, 201, 40)
    lens[:2] = (60, 200)
    long = np.concatenate([m.wins[i] for i in range(40, 44)])
    clips = [long[o:o + n].copy() for o, n in zip(rng.integers(0, len(long) - 200, 40), lens)]
    hot = rng.integers(0, 2, 40)
    got = evaluate_ctc(e, clips, hot)
    pred = []
    for i, c in enumerate(clips):
        w = np.zeros((151, 40), np.float32)
        w[:min(len(c), 151)] = c[:151]
        one = e.ctc_forward(w[None], 2)
        np.testing.assert_array_equal(got["labels"][i], one.labels[0], err_msg=f"clip {i} ({len(c)} frames)")
        assert got["lengths"][i] == one.lengths[0], i
        assert got["decoded"][i] == ctc.label_string(one.labels[0], one.lengths[0])
        pred.append(bool(ctc.is_wakeword(one.labels, one.lengths)[0]))
    assert got["predicted"].tolist() == pred
    want = ctc_statistics(hot, pred)
    assert all(got[k] == want[k] for k in want)
    assert got["tp"] + got["fp"] + got["tn"] + got["fn"] == 40


# ---- 6: refusals, both ways ----------------------------------------------------------------------------------------------------------------
def _refused(lib, ctx, rc, needle):
    from wwhip import _lib
    assert rc == _lib.WW_EINVAL, rc
    msg = lib.ww_last_error(ctx).decode()
    assert needle in msg, msg


def test_existing_entry_points_refuse_a_ctc_model(models):
    """Every entry point that evaluates the two-layer detect head answers a CTC model with WW_EINVAL and a message that names the
    ww_ctc_* family; buffers of the right sizes, pre-filled, come back untouched, and no stream bank or model set is made."""
    import torch
    from wwhip import _lib
    from wwhip.engine import frontend_params
    m = models(4)
    e = m.engine
    lib, ctx, h = _lib.load(), e.ctx.handle, e.handle
    p = _lib.ptr
    wins = np.ascontiguousarray(m.wins[:3])
    out = np.full((3, 4), SENT, np.float32)
    enc = np.full((3, 19, 64), SENT, np.float32)
    _refused(lib, ctx, lib.ww_forward(ctx, h, p(wins), 3, p(out)), "ww_ctc_forward")
    _refused(lib, ctx, lib.ww_forward_enc(ctx, h, p(wins), 3, p(out), p(enc)), "ww_ctc_forward")
    _refused(lib, ctx, lib.ww_detect(ctx, h, p(enc), 3, p(out)), "ww_ctc_forward")
    nw = C.c_int64(-5)
    mel = np.ascontiguousarray(wins.reshape(-1, 40))
    slide_out = np.full((152, 4), SENT, np.float32)
    _refused(lib, ctx, lib.ww_slide_forward(ctx, h, p(mel), mel.shape[0], 2, p(slide_out), C.byref(nw)), "ww_ctc_slide_forward")
    assert nw.value == -5
    post = np.full((2, 4), SENT, np.float32)
    offs = np.array([0, 151, 453], np.int64)
    _refused(lib, ctx, lib.ww_wave_sequence(ctx, h, p(mel), mel.shape[0], p(offs), 2, 0, None, None, None, p(post)), "ww_ctc_forward")
    assert (out == SENT).all() and (enc == SENT).all() and (slide_out == SENT).all() and (post == SENT).all()
    # device forms
    d_mel = torch.from_numpy(mel).cuda()
    d_row = torch.arange(3, dtype=torch.int64, device="cuda") * 151
    d_valid = torch.full((3,), 151, dtype=torch.int32, device="cuda")
    d_out = torch.full((152, 4), SENT, dtype=torch.float32, device="cuda")
    d_pcm = torch.zeros((2, 24000), dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    vp = lambda t: C.c_void_p(t.data_ptr())
    _refused(lib, ctx, lib.ww_forward_windows_dev(ctx, h, vp(d_mel), mel.shape[0], vp(d_row), vp(d_valid), 3, vp(d_out)), "ww_ctc_forward")
    seg_row0, seg_nw = np.array([0], np.int64), np.array([152], np.int32)
    _refused(lib, ctx, lib.ww_forward_segments_dev(ctx, h, vp(d_mel), mel.shape[0], p(seg_row0), p(seg_nw), 1, 2, vp(d_out)), "ww_ctc_forward")
    fp = frontend_params()
    _refused(lib, ctx, lib.ww_clips_forward_dev(ctx, h, vp(d_pcm), 2, 24000, C.byref(fp), vp(d_out)), "ww_ctc_forward")
    _refused(lib, ctx, lib.ww_wave_sequence_dev(ctx, h, vp(d_mel), mel.shape[0], p(offs), 2, 0, None, None, None, vp(d_out)), "ww_ctc_forward")
    e.ctx.synchronize()
    assert (d_out.cpu().numpy() == SENT).all()
    # objects built from a model
    for flags in (0, _lib.STREAM_FULL_RECOMPUTE, _lib.STREAM_TWO_LAUNCH):
        st = C.c_void_p(0)
        _refused(lib, ctx, lib.ww_stream_create(ctx, h, 2, C.byref(fp), flags, C.byref(st)), "ww_ctc_forward")
        assert not st.value
    arr = (C.c_void_p * 2)(h.value, h.value)
    ms = C.c_void_p(0)
    rc = lib.ww_model_set_create(ctx, arr, 2, C.byref(ms))
    _refused(lib, ctx, rc, "ww_ctc_forward")
    assert not ms.value
    # the Python surface raises the library's ValueError
    with pytest.raises(ValueError, match="ww_ctc_forward"):
        e.forward(wins)
    with pytest.raises(ValueError, match="ww_ctc_slide_forward"):
        e.slide_forward(mel)
    with pytest.raises(ValueError, match="CTC"):
        e.posterior_index
    # and the model still runs
    _same(e.ctc_forward(wins, 19, ALL), CtcResultOf(m.full, 3), "after the refusals")


def CtcResultOf(res, n):
    from wwhip.ctc import CtcResult
    return CtcResult(*[None if a is None else a[:n] for a in res])


def _ctc_calls(lib, ctx, h, n_out, wins):
    """Every model entry point of the family on model ``h``: ``[(name, status, buffers that must keep their sentinel)]``."""
    import torch
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    vp = lambda t: C.c_void_p(t.data_ptr())
    n = len(wins)
    mel = np.ascontiguousarray(wins.reshape(-1, 40))
    rows = (mel.shape[0] - 151) // 2 + 1   # what a slide at hop 2 would write if it were not refused
    lab, ln = np.full((rows, 2), -9, np.int32), np.full(rows, -9, np.int32)
    steps, enc = np.full((rows, 19, n_out), SENT, np.float32), np.full((n, 19, 64), SENT, np.float32)
    out = []
    out.append(("ww_ctc_forward", lib.ww_ctc_forward(ctx, h, p(wins), n, 2, p(lab), p(ln), p(steps), p(enc))))
    nw = C.c_int64(-5)
    out.append(("ww_ctc_slide_forward", lib.ww_ctc_slide_forward(ctx, h, p(mel), mel.shape[0], 2, 2, p(lab), p(ln), p(steps), C.byref(nw))))
    assert nw.value == -5
    d_mel = torch.from_numpy(mel).cuda()
    d_row = torch.arange(n, dtype=torch.int64, device="cuda") * 151
    d_valid = torch.full((n,), 151, dtype=torch.int32, device="cuda")
    d_lab = torch.full((n, 2), -9, dtype=torch.int32, device="cuda")
    d_len = torch.full((n,), -9, dtype=torch.int32, device="cuda")
    d_steps = torch.full((n, 19, n_out), SENT, dtype=torch.float32, device="cuda")
    d_enc = torch.full((n, 19, 64), SENT, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    out.append(("ww_ctc_forward_windows_dev", lib.ww_ctc_forward_windows_dev(ctx, h, vp(d_mel), mel.shape[0], vp(d_row), vp(d_valid), n, 2, vp(d_lab),
                                                                             vp(d_len), vp(d_steps), vp(d_enc))))
    torch.cuda.synchronize()
    assert (lab == -9).all() and (ln == -9).all() and (steps == SENT).all() and (enc == SENT).all()
    assert (d_lab.cpu().numpy() == -9).all() and (d_len.cpu().numpy() == -9).all()
    assert (d_steps.cpu().numpy() == SENT).all() and (d_enc.cpu().numpy() == SENT).all()
    return out


@pytest.mark.parametrize("name", ["CRNN", "CRNN_softmax", "Wavenet"])
def test_ctc_entry_points_refuse_the_shipped_models(assets, name):
    from wwhip import _lib
    from wwhip.engine import Engine
    e = Engine(os.path.join(assets, name))
    assert not e.is_ctc and e.head_kind == (_lib.HEAD_SIGMOID if name == "CRNN" else _lib.HEAD_SOFTMAX)
    lib = _lib.load()
    wins = np.ascontiguousarray(ctc64.G.windows(3, 3, e.window, 40))
    before = e.forward(wins)
    for call, rc in _ctc_calls(lib, e.ctx.handle, e.handle, e.n_out, wins):
        assert rc == _lib.WW_EINVAL, (call, rc)
        assert "not a CTC-trained CRNN" in lib.ww_last_error(e.ctx.handle).decode(), call
    with pytest.raises(ValueError, match="not a CTC"):
        e.ctc_forward(wins)
    np.testing.assert_array_equal(e.forward(wins), before)   # the shipped model still gives its posteriors
    e.close()


def test_ctc_entry_points_refuse_bf16x3_and_bad_arguments(models):
    from wwhip import _lib
    m = models(2)
    e = m.engine
    lib, ctx, h = _lib.load(), e.ctx.handle, e.handle
    wins = np.ascontiguousarray(m.wins[:3])
    e.set_precision("bf16x3")
    try:
        for call, rc in _ctc_calls(lib, ctx, h, 2, wins):
            assert rc == _lib.WW_EINVAL, (call, rc)
            assert "WW_PRECISION_FP32" in lib.ww_last_error(ctx).decode(), call
    finally:
        e.set_precision("fp32")
    p = _lib.ptr
    lab, ln = np.full((3, 19), -9, np.int32), np.full(3, -9, np.int32)
    for max_labels in (0, 20, -1):
        assert lib.ww_ctc_forward(ctx, h, p(wins), 3, max_labels, p(lab), p(ln), None, None) == _lib.WW_EINVAL
    assert lib.ww_ctc_forward(ctx, h, p(wins), 3, 2, None, p(ln), None, None) == _lib.WW_EINVAL
    assert lib.ww_ctc_forward(ctx, h, p(wins), 3, 2, p(lab), None, None, None) == _lib.WW_EINVAL
    assert lib.ww_ctc_forward(ctx, h, None, 3, 2, p(lab), p(ln), None, None) == _lib.WW_EINVAL
    assert lib.ww_ctc_forward(ctx, h, p(wins), -1, 2, p(lab), p(ln), None, None) == _lib.WW_EINVAL
    assert lib.ww_ctc_forward(ctx, h, p(wins), 0, 2, p(lab), p(ln), None, None) == _lib.WW_OK   # n = 0: nothing written
    assert (lab == -9).all() and (ln == -9).all()
    for T, L, M in ((0, 4, 1), (4097, 4, 1), (19, 1, 1), (19, 65, 1), (19, 4, 0), (19, 4, 20)):
        assert lib.ww_ctc_greedy_dev(ctx, None, 1, T, L, M, None, None) == _lib.WW_EINVAL, (T, L, M)
    _same(e.ctc_forward(wins, 19, ALL), CtcResultOf(m.full, 3), "after the refusals")
