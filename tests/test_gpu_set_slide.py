"""Model sets, sliding: ``ww_set_forward_segments_dev`` / ``ww_set_slide_forward`` / ``ww_set_option`` and the evaluator on a set.

The yardstick is the library's single-model path: plane ``k`` of a set's call equals what ``Engine(member k)`` gives on the same
rows BIT FOR BIT (``np.testing.assert_array_equal``).  Two facts of the single-model library decide which bits those are
(tests/test_gpu_parity.py holds both): the two tails give the same bits, and so do all one-kernel forms, but the ROWS form of the
layer-1 projection (every row on a 16-row MFMA tile) and the FUSED form (rows 16..18 on the 4x4x1 tile, four partial sums joined at
the end) associate three rows' sums differently - ``test_crnn_sliding_rows_path_matches_per_window_kernels`` holds them together within 2e-6, not bit for bit.
So where the set is forced into the rows form below the single model's own threshold of 64 windows, the engine it is compared
against runs in the same form (the same ``crnn_slide_min``): equality bit for bit, and against the engine at its defaults (the
fused kernel) the parity test's 2e-6, with the figure printed.  At the defaults both sides change form at 64 windows together.

Every output buffer is pre-filled with -7 and holds one guard row behind the call's rows, which must stay -7.  The planes of a call
lie back to back (``[slots][W][n_out]`` is the interface), so the guard row lies behind the last plane; a call of one slot
(``members=[1]``) has its one plane guarded, and a plane that ran over into its successor would break the successor's equality.

Members as in tests/test_gpu_model_set.py: ``CRNN_nosilence``, ``CRNN_nosilence_enhanced``, ``CRNN_softmax`` and ``Wavenet``,
``Wavenet_alt``."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import ref64 as R

pytestmark = pytest.mark.gpu

CRNNS = ["CRNN_nosilence", "CRNN_nosilence_enhanced", "CRNN_softmax"]
WAVES = ["Wavenet", "Wavenet_alt"]
TAU = 4e-5  # fp32 posteriors against Ref64: tests/test_gpu_ref64.py:21
ROWS_VS_FUSED = 2e-6  # rows form against fused form of ONE model: tests/test_gpu_parity.py::test_crnn_sliding_rows_path_matches_per_window_kernels
HOPS = [1, 2, 3, 8]                    # field strides 1, 2, 1, 8
WINDOWS = [1, 16, 17, 33, 63, 64, 65]  # per member; the set's default takes the rows form from 64 on
FORMS = {"defaults": {}, "rows_vector_tail": {"crnn_slide_min": 1, "crnn_tail_mfma": 0}, "rows_matrix_tail": {"crnn_slide_min": 1, "crnn_tail_mfma": 2}}


@pytest.fixture(scope="module")
def engines(assets):
    from wwhip.engine import Engine
    out = {m: Engine(os.path.join(assets, m)) for m in CRNNS + WAVES}
    yield out
    for e in out.values():
        e.close()


@pytest.fixture(scope="module")
def crnn_set(engines):
    from wwhip.engine import ModelSet
    ms = ModelSet([engines[m] for m in CRNNS])
    yield ms
    ms.close()


@pytest.fixture(scope="module")
def wave_set(engines):
    from wwhip.engine import ModelSet
    ms = ModelSet([engines[m] for m in WAVES])
    yield ms
    ms.close()


class _Forms:
    """The set's two dispatch options for the duration of a ``with`` block, the library's defaults afterwards."""

    def __init__(self, ms, form):
        self.ms, self.kv = ms, FORMS[form]

    def __enter__(self):
        for k, v in self.kv.items():
            self.ms.set_option(k, v)

    def __exit__(self, *exc):
        self.ms.set_option("crnn_slide_min", 64)
        self.ms.set_option("crnn_tail_mfma", 1)


def _mel(seed, rows, n_mel=40):
    return np.random.default_rng(seed).uniform(0, 6.5, (rows, n_mel)).astype(np.float32)


def _slide_all(ms, mel, hop, members=None):
    """``ww_set_slide_forward`` into a host buffer of the call's rows + one guard row, all -7 before the call."""
    from wwhip import _lib
    lib = _lib.load()
    ids = None if members is None else np.asarray(members, np.int32)
    k = ms.n_models if ids is None else ids.size
    rows = mel.shape[0]
    nw = (rows - ms.window) // hop + 1 if rows >= ms.window else 0
    out = np.full((k * nw + 1, ms.n_out), -7.0, np.float32)
    n = C.c_int64(-1)
    rc = lib.ww_set_slide_forward(ms.ctx.handle, ms.handle, _lib.ptr(mel), rows, hop, _lib.ptr(ids), 0 if ids is None else ids.size,
                                  _lib.ptr(out), C.byref(n))
    assert rc == _lib.WW_OK, lib.ww_last_error(ms.ctx.handle)
    assert n.value == nw
    assert (out[-1] == -7.0).all(), "guard row"
    return out[:-1].reshape(k, nw, ms.n_out)


@pytest.fixture(scope="module")
def one_sequence_refs(engines):
    """Engine(member).slide_forward for every (hop, windows) of test 1, at the engine's defaults (fused kernel below 64 windows, rows
    form from there on) and with the rows form from 1 window on: computed once, shared by the three forms, left unchanged."""
    T = 151
    refs = {}
    for hop in HOPS:
        for nw in WINDOWS:
            mel = _mel(1000 * hop + nw, T + (nw - 1) * hop)
            want = np.stack([engines[m].slide_forward(mel, hop) for m in CRNNS])
            rows = []
            for m in CRNNS:
                with engines[m].options(crnn_slide_min=1):
                    rows.append(engines[m].slide_forward(mel, hop))
            rows = np.stack(rows)
            assert want.shape == rows.shape == (3, nw, 2)
            if nw >= 64:
                np.testing.assert_array_equal(rows, want)  # (the engine's own default from 64 windows on)
            want.setflags(write=False)
            rows.setflags(write=False)
            refs[hop, nw] = (mel, want, rows)
    return refs


@pytest.mark.parametrize("form", list(FORMS))
def test_one_sequence_every_form(crnn_set, engines, assets, one_sequence_refs, form):
    """hop in {1, 2, 3, 8} x windows per member in {1, 16, 17, 33, 63, 64, 65}: ``slide_forward_all(mel, hop)[k]`` equals
    ``Engine(member k).slide_forward(mel, hop)`` - at the set's defaults (rows form from 64 windows on, explicit windows below) and
    with the rows form forced from 1 window on, on the vector tail and on the matrix tail (one partial tile, two tiles, a group of
    sixteen plus one).  Forced below 64 windows the equality is with the engine in the rows form too (module docstring), and the
    engine at its defaults is within ROWS_VS_FUSED.  17 windows at hop 2 also equal ``forward_all`` on the materialised windows (at
    the defaults bit for bit; the forced rows form within ROWS_VS_FUSED of that fused launch) and lie within TAU of Ref64.
    Measured on an MI355X: forced rows form against the engines' fused kernel, max |difference| over the sweep 2.98e-07, and 2.38e-07 between
    the 17 windows' forced rows form and ``forward_all``."""
    T = crnn_set.window
    forced = form != "defaults"
    worst = 0.0
    with _Forms(crnn_set, form):
        for (hop, nw), (mel, want, rows) in one_sequence_refs.items():
            got = _slide_all(crnn_set, mel, hop)
            np.testing.assert_array_equal(got, rows if forced else want, err_msg=f"{form}: hop {hop}, {nw} windows")
            if forced:
                worst = max(worst, float(np.abs(got - want).max()))
        mel, want, rows = one_sequence_refs[2, 17]
        same_form = rows if forced else want
        np.testing.assert_array_equal(crnn_set.slide_forward_all(mel, 2), same_form)
        np.testing.assert_array_equal(crnn_set.slide_forward_all(mel, 2, members=[2, 0, 2]), same_form[[2, 0, 2]])
        got = _slide_all(crnn_set, mel, 2)
    wins = np.stack([mel[2 * i: 2 * i + T] for i in range(17)])
    every = crnn_set.forward_all(wins)
    print(f"\n{form}: max |set - engines at their defaults| over the sweep {worst:.2e}, 17 windows against forward_all "
          f"{float(np.abs(got - every).max()):.2e} (rows against fused: {ROWS_VS_FUSED:g})", end="")
    assert worst <= ROWS_VS_FUSED
    if forced:
        assert float(np.abs(got - every).max()) <= ROWS_VS_FUSED
    else:
        np.testing.assert_array_equal(got, every)
    for k, name in enumerate(CRNNS):
        want64 = R.Ref64(os.path.join(assets, name)).forward(wins)[0]
        print(f"\nREF64 sliding set member {name} ({form}): needs tau {R.needed_tau(got[k], want64):.2e} (tau {TAU:g})", end="")
        R.check_posteriors(got[k], want64, TAU)


def _segments_buffer(seed, seg_nw, hop, T, first_row=7):
    """Sequences of seg_nw windows in one buffer, 5 to 30 rows of other finite data between them, the first at row ``first_row``."""
    rng = np.random.default_rng(seed)
    row0, at = [], first_row
    for nw in seg_nw:
        row0.append(at)
        at += (T + (nw - 1) * hop if nw else 0) + int(rng.integers(5, 31))
    return _mel(seed + 1, at), np.asarray(row0, np.int64), np.asarray(seg_nw, np.int32)


def _engine_segments(e, d_mel, mel_rows, row0, seg_nw, hop):
    import torch
    W = int(seg_nw.sum())
    out = torch.full((W + 1, e.n_out), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    e.forward_segments_dev(d_mel.data_ptr(), mel_rows, row0, seg_nw, hop, out.data_ptr())
    e.ctx.synchronize()
    out = out.cpu().numpy()
    assert (out[-1] == -7.0).all()
    return out[:-1]


def _set_segments(ms, d_mel, mel_rows, row0, seg_nw, hop, members):
    import torch
    W, k = int(seg_nw.sum()), ms.n_models if members is None else len(members)
    out = torch.full((k * W + 1, ms.n_out), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ms.forward_segments_dev(d_mel.data_ptr(), mel_rows, row0, seg_nw, hop, out.data_ptr(), members=members)
    ms.ctx.synchronize()
    out = out.cpu().numpy()
    assert (out[-1] == -7.0).all(), "guard row"
    return out[:-1].reshape(k, W, ms.n_out)


@pytest.mark.parametrize("tail", [0, 2])
def test_several_sequences(crnn_set, engines, tail):
    """seg_nw = [0, 1, 16, 17, 40] at hop 2 in one buffer (first sequence at row 7, 5 to 30 rows of other data between sequences):
    plane k equals ``Engine.forward_segments_dev`` of member members[k] on the same buffer and tables, for members None, [2, 0], [1],
    [1, 1] - the rows form forced, on the vector and on the matrix tail."""
    import torch
    mel, row0, seg_nw = _segments_buffer(21, [0, 1, 16, 17, 40], 2, crnn_set.window)
    assert row0[0] == 7
    d_mel = torch.from_numpy(mel).cuda()
    want = [_engine_segments(engines[m], d_mel, len(mel), row0, seg_nw, 2) for m in CRNNS]
    crnn_set.set_option("crnn_slide_min", 1)
    crnn_set.set_option("crnn_tail_mfma", tail)
    try:
        for members in (None, [2, 0], [1], [1, 1]):
            got = _set_segments(crnn_set, d_mel, len(mel), row0, seg_nw, 2, members)
            for slot, k in enumerate(range(3) if members is None else members):
                np.testing.assert_array_equal(got[slot], want[k], err_msg=f"members {members}, slot {slot}")
    finally:
        crnn_set.set_option("crnn_slide_min", 64)
        crnn_set.set_option("crnn_tail_mfma", 1)


def test_across_a_group_cut(crnn_set, engines):
    """Three members, two sequences of 5,500 windows at hop 8: 3 x 11,000 exceeds the group bound of 32,768, so the set runs two
    groups of 5,500 windows per member (the vector tail: below 9,216) where each engine runs one group of 11,000 (the matrix tail) -
    the same bits."""
    import torch
    mel, row0, seg_nw = _segments_buffer(31, [5500, 5500], 8, crnn_set.window)
    assert mel.nbytes < 15 << 20
    d_mel = torch.from_numpy(mel).cuda()
    got = _set_segments(crnn_set, d_mel, len(mel), row0, seg_nw, 8, None)
    for k, m in enumerate(CRNNS):
        np.testing.assert_array_equal(got[k], _engine_segments(engines[m], d_mel, len(mel), row0, seg_nw, 8), err_msg=m)


def test_wavenets(wave_set, engines):
    """hop 2, 1 and 17 windows, both members and members=[1] alone: equal to ``Engine.slide_forward``; several sequences through
    the device entry point equal ``Engine.forward_segments_dev``."""
    import torch
    T = wave_set.window
    for nw in (1, 17):
        mel = _mel(40 + nw, T + (nw - 1) * 2)
        want = np.stack([engines[m].slide_forward(mel, 2) for m in WAVES])
        np.testing.assert_array_equal(_slide_all(wave_set, mel, 2), want, err_msg=f"{nw} windows")
        np.testing.assert_array_equal(_slide_all(wave_set, mel, 2, [1]), want[[1]], err_msg=f"{nw} windows, members=[1]")
        np.testing.assert_array_equal(wave_set.slide_forward_all(mel, 2, members=[1]), want[[1]])
    mel, row0, seg_nw = _segments_buffer(44, [0, 1, 17], 2, T)
    d_mel = torch.from_numpy(mel).cuda()
    got = _set_segments(wave_set, d_mel, len(mel), row0, seg_nw, 2, [1, 0])
    for slot, k in enumerate([1, 0]):
        np.testing.assert_array_equal(got[slot], _engine_segments(engines[WAVES[k]], d_mel, len(mel), row0, seg_nw, 2))


def test_refusals(crnn_set, engines):
    """Every WW_EINVAL of ``ww_set_forward_segments_dev`` (a NULL argument, a set of another context, hop <= 0, n_seg < 0,
    n_members < 0, a negative seg_nw, windows that leave the mel buffer, a member id outside the set) carries a ``ww_last_error``
    text and leaves d_out all -7; n_seg = 0, W = 0 and n_members = 0 are WW_OK and write nothing; ``ww_set_option`` takes its two
    keys only."""
    import torch
    from wwhip import _lib
    lib = _lib.load()
    ctx, K, T = crnn_set.ctx, crnn_set.n_models, crnn_set.window
    mel, row0, seg_nw = _segments_buffer(51, [3, 0, 70], 2, T)
    W = int(seg_nw.sum())
    d_mel = torch.from_numpy(mel).cuda()
    out = torch.full((K * W + 1, crnn_set.n_out), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    other = _lib.Context(ctx.device)
    OMIT = object()

    def call(c=ctx.handle, s=OMIT, m=OMIT, rows=len(mel), r0=row0, nw=seg_nw, n_seg=None, hop=2, members=None, n_members=None, o=OMIT):
        ids = None if members is None else np.asarray(members, np.int32)
        rc = lib.ww_set_forward_segments_dev(c, crnn_set.handle if s is OMIT else s, C.c_void_p(d_mel.data_ptr()) if m is OMIT else m, rows,
                                             _lib.ptr(None if r0 is None else np.ascontiguousarray(r0, np.int64)),
                                             _lib.ptr(None if nw is None else np.ascontiguousarray(nw, np.int32)),
                                             len(seg_nw) if n_seg is None else n_seg, hop, _lib.ptr(ids),
                                             (0 if ids is None else ids.size) if n_members is None else n_members,
                                             C.c_void_p(out.data_ptr()) if o is OMIT else o)
        ctx.synchronize()
        return rc, c

    def refused(res, word=None):
        rc, c = res
        assert rc == _lib.WW_EINVAL, rc
        text = lib.ww_last_error(c).decode()
        assert len(text) > 8 and (word is None or word in text), text
        assert (out.cpu().numpy() == -7.0).all(), text

    try:
        refused(call(c=None), "NULL")
        refused(call(s=None), "NULL")
        refused(call(m=None), "NULL")
        refused(call(o=None), "NULL")
        refused(call(r0=None), "NULL")
        refused(call(nw=None), "NULL")
        refused(call(c=other.handle), "another context")
        refused(call(hop=0), "hop")
        refused(call(hop=-2), "hop")
        refused(call(n_seg=-1), "sequence count")
        refused(call(members=[0], n_members=-1), "member count")
        refused(call(nw=[3, -1, 70]), "sequence 1")
        refused(call(rows=int(row0[2]) + 69 * 2 + T - 1), "sequence 2")  # one row short of the last window's last row
        refused(call(r0=[-1, 0, int(row0[2])]), "sequence 0")
        refused(call(members=[0, -1]), "members[1] = -1")
        refused(call(members=[K, 0, 1]), f"members[0] = {K}")
        for ok in (call(n_seg=0), call(nw=[0, 0, 0]), call(members=[0], n_members=0), call(r0=None, nw=None, n_seg=0)):
            assert ok[0] == _lib.WW_OK
            assert (out.cpu().numpy() == -7.0).all()
        # the host form: the same refusals before a byte moves; the count per member is reported where there is one
        host = np.full((K * W + 1, crnn_set.n_out), -7.0, np.float32)
        n = C.c_int64(-1)
        for kw in ({"hop": 0}, {"ids": [0, K]}, {"n_members": -1}):
            ids = np.asarray(kw.get("ids", [0]), np.int32)
            rc = lib.ww_set_slide_forward(ctx.handle, crnn_set.handle, _lib.ptr(mel), len(mel), kw.get("hop", 2), _lib.ptr(ids),
                                          kw.get("n_members", ids.size), _lib.ptr(host), C.byref(n))
            assert rc == _lib.WW_EINVAL and len(lib.ww_last_error(ctx.handle)) > 8 and (host == -7.0).all(), kw
        rc = lib.ww_set_slide_forward(ctx.handle, crnn_set.handle, _lib.ptr(mel[:T - 1]), T - 1, 2, None, 0, _lib.ptr(host), C.byref(n))
        assert rc == _lib.WW_OK and n.value == 0 and (host == -7.0).all()
        # the options
        assert lib.ww_set_option(crnn_set.handle, _lib.OPT_CRNN_SPLIT_AT, 0) == _lib.WW_EINVAL
        assert lib.ww_set_option(crnn_set.handle, _lib.OPT_WAVENET_ROWMAJOR, 1) == _lib.WW_EINVAL
        assert lib.ww_set_option(crnn_set.handle, _lib.OPT_CRNN_TAIL_MFMA, 3) == _lib.WW_EINVAL
        assert lib.ww_set_option(crnn_set.handle, _lib.OPT_CRNN_SLIDE_MIN, -1) == _lib.WW_EINVAL
        assert lib.ww_set_option(None, _lib.OPT_CRNN_SLIDE_MIN, 1) == _lib.WW_EINVAL
        # a valid call after all of it, unchanged
        got = _set_segments(crnn_set, d_mel, len(mel), row0, seg_nw, 2, [1])
        np.testing.assert_array_equal(got[0], _engine_segments(engines[CRNNS[1]], d_mel, len(mel), row0, seg_nw, 2))
    finally:
        other.close()


def _engine_segments_rc(e, d_mel, mel_rows, row0, seg_nw, hop, out):
    """``ww_forward_segments_dev`` by its status, a context synchronise behind it."""
    from wwhip import _lib
    r0, nw = np.ascontiguousarray(row0, np.int64), np.ascontiguousarray(seg_nw, np.int32)
    rc = _lib.load().ww_forward_segments_dev(e.ctx.handle, e.handle, C.c_void_p(d_mel.data_ptr()), mel_rows, _lib.ptr(r0), _lib.ptr(nw), len(nw), hop,
                                             C.c_void_p(out.data_ptr()))
    e.ctx.synchronize()
    return rc


@pytest.mark.parametrize("name", [CRNNS[0], WAVES[0]])
def test_single_model_refusals(engines, name):
    """``ww_forward_segments_dev`` of one model (the CRNN's rows form, the Wavenet's explicit-window list) on test_refusals' sequences
    [3, 0, 70] at hop 2: a negative seg_nw, windows that leave the mel buffer and a negative seg_row0 are WW_EINVAL, name their
    sequence in ``ww_last_error`` and leave d_out all -7; a valid call afterwards has the bits of the one before them."""
    import torch
    from wwhip import _lib
    e = engines[name]
    T = e.window
    mel, row0, seg_nw = _segments_buffer(51, [3, 0, 70], 2, T)
    d_mel = torch.from_numpy(mel).cuda()
    before = _engine_segments(e, d_mel, len(mel), row0, seg_nw, 2)
    assert np.isfinite(before).all() and (before != -7.0).all()
    out = torch.full((int(seg_nw.sum()) + 1, e.n_out), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    for word, kw in (("sequence 1", {"seg_nw": [3, -1, 70]}),
                     ("sequence 2", {"mel_rows": int(row0[2]) + 69 * 2 + T - 1}),  # one row short of the last window's last row
                     ("sequence 0", {"row0": [-1, 0, int(row0[2])]})):
        rc = _engine_segments_rc(e, d_mel, kw.get("mel_rows", len(mel)), kw.get("row0", row0), kw.get("seg_nw", seg_nw), 2, out)
        text = _lib.load().ww_last_error(e.ctx.handle).decode()
        assert rc == _lib.WW_EINVAL and word in text, (rc, text)
        assert (out.cpu().numpy() == -7.0).all(), text
    np.testing.assert_array_equal(_engine_segments(e, d_mel, len(mel), row0, seg_nw, 2), before)


def test_refusal_above_a_group_enqueues_nothing(engines):
    """The CRNN's rows form over three sequences of 16,385 windows at hop 2 (tests/test_gpu_launch_tables.py's: any two exceed a group
    of 32,768 windows, so the call is three groups), the third moved one row down so that its last window ends one row past the
    mel buffer: WW_EINVAL naming sequence 2, and none of the 3 x 16,385 rows of d_out written - the first two groups are not
    launched either."""
    import torch
    from wwhip import _lib
    e = engines[CRNNS[0]]
    T, hop, nw = e.window, 2, 16385
    span = (nw - 1) * hop + T
    row0 = np.array([1, 1 + span + 3, 1 + span + 3 + span], np.int64)
    rows = int(row0[2]) + span
    mel = np.random.default_rng(78).uniform(0, 6.5, (rows, 40)).astype(np.float32)
    assert mel.nbytes < 17 << 20
    d_mel = torch.from_numpy(mel).cuda()
    out = torch.full((3 * nw, e.n_out), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    row0[2] += 1
    rc = _engine_segments_rc(e, d_mel, rows, row0, [nw] * 3, hop, out)
    text = _lib.load().ww_last_error(e.ctx.handle).decode()
    assert rc == _lib.WW_EINVAL and "sequence 2" in text, (rc, text)
    assert (out.cpu().numpy() == -7.0).all()


def _clips():
    """12 seeded synthetic clips of 0.02 to 1.2 s: one under 512 samples (no frame of its own), one shorter than either model's
    window after the 2 x 0.5 s of padding (no sliding window), mixed labels."""
    from wwhip.evaluate import synth_clip
    rng = np.random.default_rng(61)
    lens = [320, 4800] + [int(n) for n in np.linspace(9600, 19200, 10)]
    clips = [synth_clip(rng, n) for n in lens]
    labels = [1, 0, 1, 0, 0, 1, 1, 0, 1, 0, 0, 1]
    return clips, labels


@pytest.mark.parametrize("kind", ["crnn", "wavenet", "crnn_alone"])
def test_evaluator(crnn_set, wave_set, engines, kind):
    """``evaluate_testset_set(ms, clips, labels)[k]`` is ``evaluate_testset(Engine k, clips, labels)``: every array with
    assert_array_equal, every scalar with == - for the three CRNNs, the two Wavenets and a set of a single CRNN member."""
    from wwhip.engine import ModelSet
    from wwhip.evaluate import evaluate_testset, evaluate_testset_set
    ms, names = {"crnn": (crnn_set, CRNNS), "wavenet": (wave_set, WAVES)}.get(kind) or (ModelSet([engines[CRNNS[0]]]), CRNNS[:1])
    clips, labels = _clips()
    assert min(len(c) for c in clips) < 512 and len(clips) == 12 and 0 < sum(labels) < 12
    try:
        got = evaluate_testset_set(ms, clips, labels)
    finally:
        if kind == "crnn_alone":
            ms.close()
    assert len(got) == len(names)
    for k, name in enumerate(names):
        want = evaluate_testset(engines[name], clips, labels)
        assert set(got[k]) == set(want)
        assert len(want["negatives"]) > 20 and len(want["positives"]) == sum(labels)
        for key, w in want.items():
            g = got[k][key]
            if isinstance(w, np.ndarray):
                assert g.dtype == w.dtype and g.shape == w.shape, (name, key)
                np.testing.assert_array_equal(g, w, err_msg=f"{name}: {key}")
            else:
                assert w == w, (name, key)  # (not a NaN: == would not hold it against itself)
                assert g == w, (name, key, g, w)
