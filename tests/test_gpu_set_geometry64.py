"""Model sets (``ww_model_set``, ``wwhip.ModelSet``) at every geometry a set accepts, on the MI355X, against float64.

Every other set test builds its sets from the shipped directories: CRNNs with softmax-2 heads, Wavenets of T = 182, 40 bands, 24
blocks, NOUT 2.  ``tests/sets64.py`` builds families of three same-geometry synthetic members - standard-conv CRNNs with heads of
8 softmax, 3 sigmoid and ONE sigmoid unit, and every Wavenet row of ``geometry64.GEOMETRIES`` (T 1 .. 192, 13 / 39 / 40 bands, 1 .. 32
blocks, NOUT 1 .. 16) - and reads them in float64; ``tests/test_sets64.py`` shows on the CPU that those readings tell the members of
a family apart.  Here every form of the library that runs a set runs every family, and every check asserts two things:

(i)  the bits of the member's own ``Engine`` in the same form at the same launch size (``np.testing.assert_array_equal``);
(ii) the project's bound against float64 through tests/test_gpu_geometry64.py's ``_post`` / ``_enc`` / ``_logits``, which print the
     needed value in the ``GEO64`` line format (``pytest -s``): TAU 4e-5 and TAU_E 1.2e-5 on windows, TAU_STREAM 3e-4 on banks (whose
     float64 windows are cut from ``Engine.logmel``'s rows), tests/test_gpu_wave_sequence.py's TAU_Z 3.6e-5 on the sequence form.

``w-t100-odd`` (softmax of one value) has posteriors identically 1: its encodings (``want_enc``) and the sequence form's logits
carry (ii).  What a set cannot take is pinned as a refusal: a ``ValueError`` (WW_EINVAL) and an empty profile table.

A bank emits ONE number per window - the posterior in column ``posterior_index`` (``NOUT == 1 ? 0 : 1``) - and up to two windows
per 20 ms tick: ``post`` is ``[S, 2]``, ``[S, K, 2]`` on an every-member bank, whatever NOUT is.
"""
import numpy as np
import pytest

import geometry64 as G
import sets64 as S64
from oracle import ref64 as R
from test_gpu_geometry64 import FORMS, TAU, TAU_E, TAU_STREAM, _enc, _logits, _post, _windows_dev
from test_gpu_rnn_cells import _launched
from test_gpu_trigger_all import _reference
from test_gpu_wave_sequence import ALL
from test_gpu_wave_sequence import TAU as SEQ_TAU
from test_gpu_wave_sequence import TAU_E as SEQ_TAU_E
from test_gpu_wave_sequence import TAU_Z

pytestmark = pytest.mark.gpu

IDS9 = [0, 1, 2, 2, 1, 0, 1, 2, 0]
VALID9 = [3, 2, 1, 0, 3, 2, 0, 3, 1]   # which of {0, 1, T - 1, T}: every member sees a whole window and two partial ones
ROWS_VS_FUSED = 2e-6                   # tests/test_gpu_set_slide.py (tests/test_gpu_parity.py): rows form against fused form of ONE model


class Fam:
    """A family of sets64 on the device: one ``Engine`` per member and their ``ModelSet``."""

    def __init__(self, name):
        from wwhip.engine import ModelSet
        self.name, self.f = name, S64.family(name)
        self.engines = [G.engine_for(b) for b in self.f.bundles]
        self.set = ModelSet(self.engines)
        self.ctx = self.set.ctx
        assert (self.set.n_models, self.set.window, self.set.n_mel, self.set.n_out) == (S64.K, self.f.T, self.f.n_mel, self.f.n_out)
        assert self.set.posterior_index == self.f.col

    def close(self):
        self.set.close()
        for e in self.engines:
            e.close()


@pytest.fixture(scope="module")
def fams():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = Fam(name)
        return cache[name]
    yield get
    for m in cache.values():
        m.close()


def _set_windows_dev(ms, wins, valid, ids, want_enc=True):
    """``ModelSet.forward_windows_dev`` over ``wins`` with ``valid[w]`` valid rows each, window w by member ids[w]; the output
    buffers start as -1."""
    import torch
    nw, T, F = wins.shape
    d_mel = torch.from_numpy(np.ascontiguousarray(wins).reshape(-1, F)).cuda()
    d_row = torch.arange(nw, dtype=torch.int64, device="cuda") * T
    d_valid = torch.from_numpy(np.asarray(valid, np.int32)).cuda()
    d_out = torch.full((nw, ms.n_out), -1.0, dtype=torch.float32, device="cuda")
    d_enc = torch.full((nw,) + ms.enc_shape, -1.0, dtype=torch.float32, device="cuda") if want_enc else None
    torch.cuda.synchronize()
    ms.forward_windows_dev(d_mel.data_ptr(), nw * T, d_row.data_ptr(), d_valid.data_ptr(), ids, nw, d_out.data_ptr(),
                           d_enc.data_ptr() if want_enc else 0)
    ms.ctx.synchronize()
    return d_out.cpu().numpy(), (d_enc.cpu().numpy() if want_enc else None)


def _float64_windows(m, case, got, enc, wins, ids, tau=TAU):
    """(ii) on windows: rows ``got`` / ``enc`` of windows ``wins``, window w by member ids[w]."""
    f = m.f
    for k in range(S64.K):
        sel = [w for w in range(len(wins)) if ids[w] == k]
        if not sel:
            continue
        p64, e64 = f.ref64(k, wins[sel])
        if f.n_out > 1 or f.kind == "crnn":
            _post(f"{case}, member {k}", got[sel], p64, tau)
        else:
            assert (got[sel] == 1.0).all(), case
        if enc is not None:
            _enc(f"{case}, member {k}", enc[sel].reshape(e64.shape), e64, TAU_E)


def _refused(ctx, call, match=None):
    """``call`` raises ValueError (WW_EINVAL) and launches nothing (tests/test_gpu_rnn_cells.py::test_refusals' rule)."""
    def inner():
        with pytest.raises(ValueError, match=match):
            call()
    _, names = _launched(ctx, inner)
    assert names == set(), names


# ---------------------------------------------------------------------------------------------------- a. windows
@pytest.mark.parametrize("name", list(S64.ROWS))
def test_windows(fams, name):
    """forward_windows_dev (with encoder rows), forward and forward_all(want_enc=True): 9 windows with {0, 1, T - 1, T} valid rows
    (capped to T), members [0, 1, 2, 2, 1, 0, 1, 2, 0] - every row the bits of the member's forward_windows_dev row at the same
    launch size, every encoder row the bits of the member's Engine.forward on the zero-padded windows.  A CRNN set has ONE window
    form (crnn_fused_kernel<set>): it is held against the member in each of the three dispatch forms of FORMS, which give equal
    bits; ``crnn_tail_mfma`` through ModelSet.set_option leaves the bits as they are, ``crnn_split_at`` is refused there.  Wavenet
    families once more at 300 windows by w % 3 (the four-wave form above 256).  A set of ONE member equals the engine.
    Measured on an MI355X (needed tau / tau_e, the worst over the forms): c-std-n8 3.8e-7 / 3.3e-7, c-std-n3-sigmoid 1.1e-7 / 3.0e-7,
    c-std-n1-sigmoid 0 (every posterior within 4 fp32 ulps) / 3.2e-7, w-t1 2.2e-7 / 5.9e-7, w-t16 2.2e-7 / 4.8e-7, w-t17-m13 4.7e-7 /
    2.9e-7, w-t100-odd - / 3.3e-7, w-t183 1.6e-6 / 6.3e-7 (300 windows), w-max 2.5e-7 / 5.8e-7."""
    from wwhip import _lib
    from wwhip.engine import ModelSet
    m = fams(name)
    f, ms, T = m.f, m.set, m.f.T
    vals = [min(v, T) for v in (0, 1, max(T - 1, 0), T)]
    valid = [vals[i] for i in VALID9]
    wins = f.wins[:9]
    cut = wins.copy()
    for w, v in enumerate(valid):
        cut[w, v:] = 0.0
    forms = FORMS if f.kind == "crnn" else {"default": {}}
    got, enc = _set_windows_dev(ms, wins, valid, IDS9)
    _float64_windows(m, f"{name} set forward_windows_dev, valid rows {valid}", got, enc, cut, IDS9)
    host, host_enc = ms.forward(cut, IDS9, want_enc=True)
    np.testing.assert_array_equal(host, got, err_msg="ModelSet.forward against forward_windows_dev")
    np.testing.assert_array_equal(host_enc, enc)
    every, every_enc = ms.forward_all(cut, want_enc=True)
    assert every.shape == (S64.K, 9, f.n_out) and every_enc.shape == (S64.K, 9) + ms.enc_shape
    for form, opts in forms.items():
        if f.kind == "crnn":
            ms.set_option("crnn_tail_mfma", opts.get("crnn_tail_mfma", 1))
        try:
            again, again_enc = _set_windows_dev(ms, wins, valid, IDS9)
        finally:
            if f.kind == "crnn":
                ms.set_option("crnn_tail_mfma", 1)
        np.testing.assert_array_equal(again, got, err_msg=form)
        np.testing.assert_array_equal(again_enc, enc, err_msg=form)
        for k, e in enumerate(m.engines):
            with e.options(**opts):
                rows = _windows_dev(e, wins, valid)
                rows_padded, e_enc = e.forward(cut, want_enc=True)
            np.testing.assert_array_equal(rows_padded, rows, err_msg=f"{form}: member {k}, zero-padded against valid rows")
            sel = [w for w in range(9) if IDS9[w] == k]
            np.testing.assert_array_equal(got[sel], rows[sel], err_msg=f"{form}: windows of member {k}")
            np.testing.assert_array_equal(enc[sel], e_enc.reshape((9,) + ms.enc_shape)[sel], err_msg=f"{form}: encoder rows of member {k}")
            np.testing.assert_array_equal(every[k], rows, err_msg=f"{form}: forward_all, member {k}")
            np.testing.assert_array_equal(every_enc[k], e_enc.reshape((9,) + ms.enc_shape), err_msg=f"{form}: forward_all encoder, member {k}")
    for k in range(S64.K):
        _float64_windows(m, f"{name} set forward_all", every[k], every_enc[k], cut, [k] * 9)
    if f.kind == "crnn":   # the window form of a set is not an option: the key is refused, by the wrapper and by the library
        _refused(m.ctx, lambda: ms.set_option("crnn_split_at", 0), "crnn_split_at")
        lib = _lib.load()
        _, names = _launched(m.ctx, lambda: lib.ww_set_option(ms.handle, _lib.OPT_CRNN_SPLIT_AT, 0))
        assert lib.ww_set_option(ms.handle, _lib.OPT_CRNN_SPLIT_AT, 0) == _lib.WW_EINVAL and names == set()
        np.testing.assert_array_equal(_set_windows_dev(ms, wins, valid, IDS9)[0], got)
    else:
        idx = np.random.default_rng(71).permutation(np.resize(np.arange(len(f.wins)), 300))
        big, ids = f.wins[idx], [w % S64.K for w in range(300)]
        full = [T] * 300
        got300, enc300 = _set_windows_dev(ms, big, full, ids)
        for k, e in enumerate(m.engines):
            rows = _windows_dev(e, big, full)
            e_enc = e.forward(big, want_enc=True)[1].reshape((300,) + ms.enc_shape)
            sel = [w for w in range(300) if ids[w] == k]
            np.testing.assert_array_equal(got300[sel], rows[sel], err_msg=f"300 windows, member {k}")
            np.testing.assert_array_equal(enc300[sel], e_enc[sel], err_msg=f"300 windows, encoder rows of member {k}")
        _float64_windows(m, f"{name} set forward_windows_dev, 300 windows", got300, enc300, big, ids)
    one = ModelSet([m.engines[1]])
    try:
        p1, e1 = one.forward(cut, [0] * 9, want_enc=True)
    finally:
        one.close()
    pe, ee = m.engines[1].forward(cut, want_enc=True)
    np.testing.assert_array_equal(p1, pe)
    np.testing.assert_array_equal(e1, ee.reshape(e1.shape))
    _float64_windows(m, f"{name} set of one member", p1, e1, cut, [1] * 9)


# ---------------------------------------------------------------------------------------------------- b. sliding
def _sliding(mel, T, hop):
    return np.ascontiguousarray(np.lib.stride_tricks.sliding_window_view(mel, (T, mel.shape[1]))[::hop, 0])


def _engine_segments(e, d_mel, mel_rows, row0, seg_nw, hop):
    import torch
    W = int(np.sum(seg_nw))
    out = torch.full((W + 1, e.n_out), -1.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    e.forward_segments_dev(d_mel.data_ptr(), mel_rows, row0, seg_nw, hop, out.data_ptr())
    e.ctx.synchronize()
    out = out.cpu().numpy()
    assert (out[-1] == -1.0).all(), "guard row"
    return out[:-1]


def _set_segments(ms, d_mel, mel_rows, row0, seg_nw, hop, members):
    import torch
    W, k = int(np.sum(seg_nw)), ms.n_models if members is None else len(members)
    out = torch.full((k * W + 1, ms.n_out), -1.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ms.forward_segments_dev(d_mel.data_ptr(), mel_rows, row0, seg_nw, hop, out.data_ptr(), members=members)
    ms.ctx.synchronize()
    out = out.cpu().numpy()
    assert (out[-1] == -1.0).all(), "guard row behind the last plane"
    return out[:-1].reshape(k, W, ms.n_out)


@pytest.mark.parametrize("name", list(S64.ROWS))
def test_sliding(fams, name):
    """slide_forward_all / forward_segments_dev.  CRNN families: hops 1, 2 and 3 over 65 windows (crnn_rows_kernel<set> and its tail
    at the defaults, which the engine takes at 65 windows too) and over 10 (explicit windows on both sides at the defaults; then the
    rows form forced on both sides with ``crnn_slide_min`` = 1, on the vector and on the matrix tail: the same bits, and within
    ROWS_VS_FUSED of the fused form).  Wavenet families: hops 1 and 3 over 12 windows.  members=[2, 0, 2]: slots 0 and 2 carry the
    same bits.  Two sequences in one forward_segments_dev call (5 and 4 windows at hop 2, the first at row 3, 7 rows of other data
    between them), plane k against the member's own forward_segments_dev - which slides in the rows form whatever the count, so
    the set is given ``crnn_slide_min`` = 1 (tests/test_gpu_set_slide.py).  Measured on an MI355X (needed tau, the worst over hops, counts and forms): c-std-n8 9.7e-7 (two sequences),
    c-std-n3-sigmoid 7.5e-7, c-std-n1-sigmoid 7.1e-7 (both 65 windows), w-t1 3.5e-7, w-t16 3.9e-7, w-t17-m13 5.3e-7, w-t183 3.0e-6
    (hop 1), w-max 3.4e-7; w-t100-odd's rows are identically 1."""
    import torch
    m = fams(name)
    f, ms, T = m.f, m.set, m.f.T
    crnn = f.kind == "crnn"
    for hop in (1, 2, 3):
        if not crnn and hop == 2:
            continue
        for nw in ((65, 10) if crnn else (12,)):
            mel = f.mel(T + hop * (nw - 1), seed=hop)
            sw = _sliding(mel, T, hop)
            assert len(sw) == nw
            got = ms.slide_forward_all(mel, hop)
            assert got.shape == (S64.K, nw, f.n_out)
            for k, e in enumerate(m.engines):
                np.testing.assert_array_equal(got[k], e.slide_forward(mel, hop), err_msg=f"hop {hop}, {nw} windows, member {k}")
                _float64_windows(m, f"{name} slide_forward_all hop {hop}, {nw} windows", got[k], None, sw, [k] * nw)
            if crnn and nw == 10:
                for tail in (0, 2):
                    ms.set_option("crnn_slide_min", 1)
                    ms.set_option("crnn_tail_mfma", tail)
                    try:
                        rows = ms.slide_forward_all(mel, hop)
                    finally:
                        ms.set_option("crnn_slide_min", 64)
                        ms.set_option("crnn_tail_mfma", 1)
                    for k, e in enumerate(m.engines):
                        with e.options(crnn_slide_min=1, crnn_tail_mfma=tail):
                            np.testing.assert_array_equal(rows[k], e.slide_forward(mel, hop), err_msg=f"rows form, tail {tail}, hop {hop}, member {k}")
                        _float64_windows(m, f"{name} slide_forward_all hop {hop}, 10 windows, rows form, tail {tail}", rows[k], None, sw, [k] * nw)
                    assert np.abs(rows - got).max() <= ROWS_VS_FUSED
    mel = f.mel(T + 3 * 11, seed=3)
    rep = ms.slide_forward_all(mel, 3, members=[2, 0, 2])
    np.testing.assert_array_equal(rep[0], rep[2])
    np.testing.assert_array_equal(rep[0], m.engines[2].slide_forward(mel, 3))
    np.testing.assert_array_equal(rep[1], m.engines[0].slide_forward(mel, 3))
    _float64_windows(m, f"{name} slide_forward_all members=[2, 0, 2]", rep[2], None, _sliding(mel, T, 3), [2] * 12)
    # two sequences in one buffer
    hop, seg_nw = 2, np.array([5, 4], np.int32)
    len0, len1 = T + hop * 4, T + hop * 3
    row0 = np.array([3, 3 + len0 + 7], np.int64)
    buf = f.mel(int(row0[1]) + len1 + 5, seed=9)
    d_mel = torch.from_numpy(buf).cuda()
    if crnn:
        ms.set_option("crnn_slide_min", 1)
    try:
        for members in (None, [2, 0, 2]):
            got = _set_segments(ms, d_mel, len(buf), row0, seg_nw, hop, members)
            for slot, k in enumerate(range(S64.K) if members is None else members):
                np.testing.assert_array_equal(got[slot], _engine_segments(m.engines[k], d_mel, len(buf), row0, seg_nw, hop),
                                              err_msg=f"two sequences, members {members}, slot {slot}")
                sw = np.concatenate([_sliding(buf[row0[0]:row0[0] + len0], T, hop), _sliding(buf[row0[1]:row0[1] + len1], T, hop)])
                _float64_windows(m, f"{name} forward_segments_dev, two sequences, members {members}, slot {slot}", got[slot], None, sw, [k] * 9)
    finally:
        if crnn:
            ms.set_option("crnn_slide_min", 64)


# ---------------------------------------------------------------------------------------------------- c. the sequence form
@pytest.mark.parametrize("name", S64.WAVE_FAMILIES)
def test_sequence_form(fams, name):
    """sequence_forward_all(want=ALL) and sequence_forward with per-sequence members in one ragged call at lengths 1, T - 1, T,
    T + 1, 2 T + 5 and 500: the bits of the member's Engine.sequence_forward, and WaveSeq64 within tests/test_gpu_wave_sequence.py's
    bounds; once more with ``wave_seq_segment`` = 200 (the 500-row sequence in three segments): the same bits.
    Measured on an MI355X (needed tau_e / tau_z / tau over post and post_frames): w-t1 9.2e-7 / 1.2e-6 / 1.7e-6, w-t16 7.3e-7 / 1.3e-6 /
    8.6e-7, w-t17-m13 6.1e-7 / 8.6e-7 / 6.3e-7, w-t100-odd 3.5e-7 / 1.3e-6 / -, w-t183 7.0e-7 / 2.3e-6 / 1.9e-6 (371 rows), w-max
    7.1e-7 / 6.7e-7 / 2.8e-7."""
    m = fams(name)
    f, ms, T = m.f, m.set, m.f.T
    lengths = [n for n in dict.fromkeys((1, T - 1, T, T + 1, 2 * T + 5, 500)) if n >= 1]
    seqs = [np.ascontiguousarray(G.windows(S64.WINDOW_SEED + 500 + i, 1, L, f.n_mel)[0]) for i, L in enumerate(lengths)]
    every = ms.sequence_forward_all(seqs, want=ALL)
    ids = [i % S64.K for i in range(len(seqs))]
    mixed = ms.sequence_forward(seqs, ids, want=ALL)
    ms.set_option("wave_seq_segment", 200)
    try:
        cut_every = ms.sequence_forward_all(seqs, members=[2, 0, 2], want=ALL)
        cut_mixed = ms.sequence_forward(seqs, ids, want=ALL)
    finally:
        ms.set_option("wave_seq_segment", 0)
    for k, e in enumerate(m.engines):
        own = e.sequence_forward(seqs, want=ALL)
        for i, (L, x) in enumerate(zip(lengths, seqs)):
            lab = f"{name} set sequence of {L} rows, member {k}"
            for key in ALL:
                np.testing.assert_array_equal(every[key][k][i], own[key][i], err_msg=f"{lab}: {key}")
                if ids[i] == k:
                    np.testing.assert_array_equal(mixed[key][i], own[key][i], err_msg=f"{lab}: {key}, per-sequence members")
                    np.testing.assert_array_equal(cut_mixed[key][i], own[key][i], err_msg=f"{lab}: {key}, per-sequence members, wave_seq_segment")
                for slot, kk in enumerate([2, 0, 2]):
                    if kk == k:
                        np.testing.assert_array_equal(cut_every[key][slot][i], own[key][i], err_msg=f"{lab}: {key}, slot {slot}, wave_seq_segment")
            want = f.seq64(k, x)
            _enc(lab, every["enc"][k][i], want["enc"], SEQ_TAU_E)
            _logits(lab, every["logits"][k][i], want["logits"], TAU_Z)
            if f.n_out > 1:
                _post(lab + ", post", every["post"][k][i][None], want["post"][None], SEQ_TAU)
                _post(lab + ", post_frames", every["post_frames"][k][i], want["post_frames"], SEQ_TAU)
            else:
                assert (every["post"][k][i] == 1.0).all() and (every["post_frames"][k][i] == 1.0).all()


# ---------------------------------------------------------------------------------------------------- d / e. banks
def _script(f, S, ticks, seed, resets):
    """PCM of the family's, ``is_speech`` about 80 %, ``is_active`` about 10 %, and ``resets``: tick -> stream ids reset before it."""
    rng = np.random.default_rng(seed)
    return dict(pcm=f.pcm(S, ticks, seed=seed), S=S, ticks=ticks, speech=(rng.random((ticks, S)) < 0.8).astype(np.uint8),
                active=(rng.random((ticks, S)) < 0.1).astype(np.uint8), resets=resets)


def _run(bank, sc, before=None):
    """The script through one bank: (post [ticks, S, ...], n_post [ticks, S]).  ``before``: tick -> a call on the bank."""
    posts, ns = [], []
    for t in range(sc["ticks"]):
        if t in sc["resets"]:
            bank.reset(sc["resets"][t])
        if before and t in before:
            before[t](bank)
        p, n = bank.step(sc["pcm"][:, t * 320:(t + 1) * 320], sc["speech"][t], sc["active"][t])
        posts.append(p)
        ns.append(n)
    return np.stack(posts), np.stack(ns)


def _emitted(post, n, s, ticks=None):
    """Stream s's posteriors in order, over the ticks ``ticks`` (default: all); ``post [ticks, S, 2]``."""
    return np.array([post[t, s, j] for t in (range(len(post)) if ticks is None else ticks) for j in range(n[t, s])], np.float32)


def _stream_float64(m, sc, s, spans, causal):
    """What float64 says stream ``s`` emits under the script, span by span: ``spans`` = [(first tick, end tick, member)], each
    starting with a reset (or the bank's creation).  Ticks whose bit 1 is set are dropped whole; a mel row belongs to the tick that
    brings its last sample and is emitted when that tick's bit 0 is set.  A window bank's window ring takes the emitted rows
    alone (csrc/stream_all.h: sa_tick_stream - a row that arrives outside speech is computed and dropped): its posteriors are
    those of the hop-1 windows, from a zero window, over the EMITTED rows.  A causal bank's state takes every row: its posteriors
    are post_frames of all rows since the reset, at the emitted ones.  The rows are ``Engine.logmel``'s of the kept samples."""
    f = m.f
    out = []
    for t0, t1, k in spans:
        kept = [t for t in range(t0, t1) if not sc["active"][t, s]]
        x = np.concatenate([sc["pcm"][s, t * 320:(t + 1) * 320] for t in kept]) if kept else np.zeros(0, np.int16)
        n_rows = (len(x) - 512) // 160 + 1 if len(x) >= 512 else 0
        if not n_rows:
            out.append(np.zeros(0))
            continue
        emit = np.array([bool(sc["speech"][kept[-(-(512 + 160 * r) // 320) - 1], s]) for r in range(n_rows)])
        mel = m.engines[0].logmel([x])[0]
        assert len(mel) == n_rows
        if causal:
            out.append(f.seq64(k, mel)["post_frames"][emit, f.col])
        else:
            sw = np.ascontiguousarray(R.stream_windows(mel[emit], f.T)) if emit.any() else np.zeros((0, f.T, f.n_mel), np.float32)
            out.append(f.ref64(k, sw)[0][:, f.col] if len(sw) else np.zeros(0))
    return out


def _bank_float64(m, case, got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (case, got.shape, want.shape)
    if m.f.n_out == 1 and m.f.kind == "wavenet":
        assert (got == 1.0).all() and len(got) > 0, case
    else:
        _post(case, got[:, None], want[:, None], TAU_STREAM, absolute=False)


BANK_MODES = ([(n, "window") for n in S64.ROWS] + [(n, "causal") for n in S64.WAVE_FAMILIES])


def _bank_forms(m, mode, S):
    """The forms a family's bank takes: form -> (StreamBank's flags, the kernels every tick of the form launches, by the profile's
    names).  The profile names a kernel, not its template arguments: the SET instantiation of a tick kernel carries the name of the
    single-model one, so what the names pin is the FORM - one launch or two, window or causal - in which the set bank runs, the
    member's own bank beside it."""
    if mode == "causal":
        return {"causal": (dict(causal=True), {"stream_frontend_kernel", "wavenet_seq_kernel<stream>"})}
    if m.f.kind == "crnn":
        return {"one launch": ({}, {"crnn_stream_kernel<tick>"}), "two launches": (dict(two_launch=True), {"stream_frontend_kernel", "crnn_stream_kernel"})}
    two = (dict(two_launch=True), {"stream_frontend_kernel", "wavenet_kernel"})
    if m.f.n_mel == 40 and m.f.T <= 182:   # ww_wave_tick_capable (csrc/wavenet.hip) at 4 streams
        return {"one launch": ({}, {"wavenet_kernel<tick>"}), "two launches": two}
    return {"default": ({}, two[1])}


def _tick_kernels(bank, sc):
    def three():
        for t in range(3):
            bank.step(sc["pcm"][:, t * 320:(t + 1) * 320], np.ones(sc["S"], np.uint8))
    _, names = _launched(bank.engine.ctx, three)
    bank.reset()
    return names


@pytest.mark.parametrize("name,mode", BANK_MODES)
def test_member_banks(fams, name, mode):
    """StreamBank(set, 4, models=[0, 1, 2, 1]), 100 ticks of 320 samples, is_speech about 80 % and is_active about 10 % at random,
    reset([1]) before tick 40 and set_model([3], 0) before tick 60.  (i) every stream against the bank of its member's own engine
    under the same frames, flags and resets - stream 3 against member 1's before the move and against member 0's, reset at tick 60,
    after it.  (ii) float64 on the hop-1 windows of Engine.logmel's rows (a causal bank: post_frames of those rows).  CRNN families
    and w-t1 / w-t16: one launch per tick and two, the same bits; the other Wavenet families (13 / 39 bands, T above 182) take the
    two-launch form alone; all Wavenet families also as causal banks.  The set bank launches the kernels of the member's bank in
    the same form.  Measured on an MI355X (needed tau at TAU_STREAM 3e-4; window bank, then causal bank): c-std-n8 4.7e-7,
    c-std-n3-sigmoid 7.8e-7, c-std-n1-sigmoid 2.9e-7, w-t1 7.2e-7 / 1.4e-6, w-t16 1.1e-7 / 4.4e-7, w-t17-m13 4.8e-7 / 5.6e-7, w-t183
    9.6e-7 / 1.8e-6, w-max 1.3e-7 / 1.1e-7; w-t100-odd emits 1.0 alone."""
    from wwhip.engine import StreamBank
    m = fams(name)
    f, S, ticks, models = m.f, 4, 100, [0, 1, 2, 1]
    sc = _script(f, S, ticks, 3, {40: [1]})
    causal = mode == "causal"
    forms = _bank_forms(m, mode, S)
    runs = {}
    for form, (kw, kernels) in forms.items():
        bank = StreamBank(m.set, S, models=models, **kw)
        try:
            names = _tick_kernels(bank, sc)
            assert kernels <= names and ("launch" not in form or ("stream_frontend_kernel" in names) == (form == "two launches")), (form, names)
            runs[form] = _run(bank, sc, {60: lambda b: b.set_model([3], 0)})
        finally:
            bank.close()
        own = []
        for e in m.engines:
            b = StreamBank(e, S, **kw)
            try:
                assert _tick_kernels(b, sc) == names, form
                own.append(_run(b, sc, {60: lambda b: b.reset([3])}))
            finally:
                b.close()
        post, n = runs[form]
        assert post.shape == (ticks, S, 2) and n.max() == 2
        for s in range(S):
            for t0, t1, k in ([(0, ticks, models[s])] if s != 3 else [(0, 60, 1), (60, ticks, 0)]):
                np.testing.assert_array_equal(n[t0:t1, s], own[k][1][t0:t1, s], err_msg=f"{form}: n_post of stream {s}")
                np.testing.assert_array_equal(post[t0:t1, s], own[k][0][t0:t1, s], err_msg=f"{form}: stream {s} against member {k}'s bank")
    first = next(iter(runs.values()))
    for form, r in runs.items():
        np.testing.assert_array_equal(r[0], first[0], err_msg=form)
        np.testing.assert_array_equal(r[1], first[1], err_msg=form)
    post, n = first
    spans = {0: [(0, ticks, 0)], 1: [(0, 40, 1), (40, ticks, 1)], 2: [(0, ticks, 2)], 3: [(0, 60, 1), (60, ticks, 0)]}
    for s in range(S):
        want = np.concatenate(_stream_float64(m, sc, s, spans[s], causal))
        assert len(want) > 100
        _bank_float64(m, f"{name} set bank ({mode}), stream {s} by member {[k for _, _, k in spans[s]]}", _emitted(post, n, s), want)


@pytest.mark.parametrize("name,mode", BANK_MODES)
def test_every_member_banks(fams, name, mode):
    """StreamBank(set, 3, members=[0, 1, 2]), 100 ticks under random flags with reset([2]) before tick 50: ``post`` is [3, 3, 2] per
    tick - (stream, member slot, window of the tick) - and ``post[:, j]`` the bits of member j's own bank, ``n_post`` and
    ``window(s)`` equal to every bank's.  (ii) float64 on stream 0, every slot.  Causal banks: ``feed_all`` in packets of 1, 159,
    160, 161 and 5,000 samples gives the bits ``step`` gives with every VAD bit set.  members=[2, 0, 2] once on c-std-n8 and once on
    w-max: slots 0 and 2 carry the same bits.  Measured on an MI355X (needed tau at TAU_STREAM 3e-4; window bank, then causal bank by step and feed_all):
    c-std-n8 5.2e-7, c-std-n3-sigmoid 7.0e-7, c-std-n1-sigmoid 3.0e-7, w-t1 7.2e-7 / 1.3e-6, w-t16 4.0e-7 / 4.4e-7, w-t17-m13 2.8e-7 /
    5.6e-7, w-t183 6.4e-7 / 1.4e-6, w-max 0 / 0 (within 4 fp32 ulps); w-t100-odd emits 1.0 alone."""
    from wwhip.engine import StreamBank
    m = fams(name)
    f, S, ticks = m.f, 3, 100
    causal = mode == "causal"
    kw = dict(causal=True) if causal else {}
    sc = _script(f, S, ticks, 3, {50: [2]})   # (streams 0 .. 2 of test_member_banks' script: the float64 windows are shared)
    sc["pcm"] = f.pcm(4, ticks, seed=3)[:S]
    sc4 = _script(f, 4, ticks, 3, {})
    sc["speech"], sc["active"] = sc4["speech"][:, :S].copy(), sc4["active"][:, :S].copy()
    wins = {}

    def run(bank):
        out = _run(bank, sc)
        wins[id(bank)] = np.stack([bank.window(s) for s in range(S)])
        return out + (wins[id(bank)],)
    own = []
    for e in m.engines:
        b = StreamBank(e, S, **kw)
        try:
            own.append(run(b))
        finally:
            b.close()
    lists = [[0, 1, 2]] + ([[2, 0, 2]] if name in ("c-std-n8", "w-max") and not causal else [])
    for members in lists:
        bank = StreamBank(m.set, S, members=members, **kw)
        try:
            post, n, w = run(bank)
        finally:
            bank.close()
        assert post.shape == (ticks, S, len(members), 2)
        for j, k in enumerate(members):
            np.testing.assert_array_equal(n, own[k][1], err_msg=f"members {members}: n_post against member {k}'s bank")
            np.testing.assert_array_equal(post[:, :, j, :], own[k][0], err_msg=f"members {members}: slot {j} against member {k}'s bank")
            np.testing.assert_array_equal(w, own[k][2], err_msg="window(s)")
        if members == [2, 0, 2]:
            np.testing.assert_array_equal(post[:, :, 0, :], post[:, :, 2, :])
        for j, k in enumerate(members):
            want = np.concatenate(_stream_float64(m, sc, 0, [(0, ticks, k)], causal))
            _bank_float64(m, f"{name} every-member bank ({mode}), members {members}, stream 0, slot {j}", _emitted(post[:, :, j, :], n, 0), want)
    if not causal:
        return
    ones = dict(sc, speech=np.ones((ticks, S), np.uint8), active=np.zeros((ticks, S), np.uint8), resets={})
    bank = StreamBank(m.set, S, members=[0, 1, 2], causal=True)
    try:
        post, n = _run(bank, ones)
    finally:
        bank.close()
    bank = StreamBank(m.set, S, members=[0, 1, 2], causal=True)
    fed = [[] for _ in range(S)]
    try:
        total = ticks * 320
        at, sizes, c = np.zeros(S, int), (1, 159, 160, 161, 5000), 0
        while (at < total).any():
            ids = [s for s in range(S) if at[s] < total]
            ks = [min(sizes[(c + s) % len(sizes)], total - at[s]) for s in ids]
            p, _ = bank.feed_all(ids, [sc["pcm"][s, at[s]:at[s] + q] for s, q in zip(ids, ks)])
            for i, (s, q) in enumerate(zip(ids, ks)):
                assert p[i].ndim == 2 and p[i].shape[1] == S64.K
                fed[s].append(p[i])
                at[s] += q
            c += 1
    finally:
        bank.close()
    for s in range(S):
        rows = np.concatenate(fed[s])
        assert len(rows) == (total - 512) // 160 + 1
        for j in range(S64.K):
            np.testing.assert_array_equal(rows[:, j], _emitted(post[:, :, j, :], n, s), err_msg=f"feed_all against step, stream {s}, slot {j}")
    for j in range(S64.K):
        want = np.concatenate(_stream_float64(m, ones, 0, [(0, ticks, j)], True))
        _bank_float64(m, f"{name} every-member causal bank, feed_all, stream 0, slot {j}", np.concatenate(fed[0])[:, j], want)


def test_bank_refusals(fams):
    """What a set's bank cannot be: full_recompute on any set, a causal bank of a CRNN set, member ids outside the set - each a
    ValueError, with nothing launched."""
    from wwhip.engine import StreamBank
    c, w = fams("c-std-n8"), fams("w-t17-m13")
    _refused(c.ctx, lambda: StreamBank(c.set, 2, full_recompute=True), "full_recompute")
    _refused(c.ctx, lambda: StreamBank(c.set, 2, members=[0, 1], full_recompute=True), "full_recompute")
    _refused(c.ctx, lambda: StreamBank(c.set, 2, causal=True), "CAUSAL")
    _refused(c.ctx, lambda: StreamBank(c.set, 2, members=[0, 1], causal=True), "CAUSAL")
    _refused(w.ctx, lambda: StreamBank(w.set, 2, models=[0, 3]))
    _refused(w.ctx, lambda: StreamBank(w.set, 2, members=[0, 3]))
    _refused(c.ctx, lambda: c.set.sequence_forward([c.f.mel(10)], [0]), "Wavenet")


# ---------------------------------------------------------------------------------------------------- f. trigger
@pytest.mark.parametrize("name", S64.TRIGGER_FAMILIES)
def test_trigger(fams, name):
    """ww_stream_step_trigger_all on the NOUT 1, 3, 8 and 16 families: 3 streams, 40 ticks, every VAD bit set, ``is_active`` cleared
    before every tick, the thresholds tests/test_sets64.py vets (from the float64 posteriors of the script alone, none within 100
    TAU_STREAM of a posterior).  Posteriors, fired ids, winning slots and masks equal, tick by tick, what the rule of
    tests/test_gpu_trigger_all.py gives on the members' own banks - and the fired ids, slots and masks what it gives on the float64
    posteriors in column ``posterior_index``: a bank that picked the column for another head width would fire elsewhere.
    Measured on an MI355X (needed tau of the emitted posteriors at TAU_STREAM 3e-4): c-std-n1-sigmoid 2.5e-7, c-std-n3-sigmoid 9.4e-7,
    c-std-n8 4.8e-7, w-max 2.1e-7; the fired ids, slots and masks agreed on every tick."""
    from wwhip import _lib
    from wwhip.engine import StreamBank
    m = fams(name)
    f, S, ticks = m.f, S64.TRIGGER_STREAMS, S64.TRIGGER_TICKS
    lib, p = _lib.load(), _lib.ptr
    post64 = f.trigger_post64()
    thr = S64.trigger_thresholds(post64, 100 * TAU_STREAM)
    pcm = f.pcm(S, ticks, seed=7)
    frames = np.ascontiguousarray(pcm.reshape(S, ticks, 320).transpose(1, 0, 2))
    speech = np.ones((ticks, S), np.uint8)
    banks = [StreamBank(e, S) for e in m.engines]
    try:
        run = _reference(banks, (frames, speech), thr, 1)
    finally:
        for b in banks:
            b.close()
    bank = StreamBank(m.set, S, members=[0, 1, 2])
    got_events, emitted = [], [[[] for _ in range(S)] for _ in range(S64.K)]
    try:
        active, was, pmax = np.zeros(S, np.uint8), np.zeros(S, np.uint8), np.zeros((S, S64.K), np.float32)
        post, n_post = np.zeros((S, S64.K, 2), np.float32), np.zeros(S, np.int32)
        fired, slot, mask, fall = np.zeros(S, np.int32), np.zeros(S, np.int32), np.zeros(S, np.uint64), np.zeros(S, np.int32)
        nf, nl, th = np.zeros(1, np.int32), np.zeros(1, np.int32), np.array(thr, np.float64)
        for t in range(ticks):
            active[:] = 0
            rc = lib.ww_stream_step_trigger_all(bank._h, p(frames[t]), p(speech[t]), p(active), p(th), p(was), p(pmax), p(post), p(n_post),
                                                p(fired), p(slot), p(mask), p(nf), p(fall), p(nl))
            assert rc == _lib.WW_OK, lib.ww_last_error(m.ctx.handle)
            rp, rn, ra, rf, rs, rm, rx, rl = run[t]
            assert np.array_equal(post, rp) and np.array_equal(n_post, rn) and np.array_equal(active, ra) and np.array_equal(pmax, rx), t
            events = (fired[:nf[0]].tolist(), slot[:nf[0]].tolist(), [int(x) for x in mask[:nf[0]]])
            assert events == (rf, rs, rm) and fall[:nl[0]].tolist() == rl == [], t
            got_events.append(events)
            for j in range(S64.K):
                for s in range(S):
                    emitted[j][s] += post[s, j, :n_post[s]].tolist()
    finally:
        bank.close()
    n_ticks = np.stack([r[1] for r in run])
    assert n_ticks.sum(axis=0).tolist() == [post64.shape[2]] * S
    want_events = S64.trigger_expectation(post64, thr, n_ticks)
    assert got_events == want_events
    assert any(0 < bin(x).count("1") < S64.K for _, _, ms_ in got_events for x in ms_) and sum(len(e[0]) for e in got_events) >= ticks
    for j in range(S64.K):
        _bank_float64(m, f"{name} every-member trigger bank, slot {j}", np.concatenate([emitted[j][s] for s in range(S)]),
                      np.concatenate(list(post64[j])))


# ---------------------------------------------------------------------------------------------------- g. clip evaluation
@pytest.mark.parametrize("name", ["c-std-n8", "c-std-n1-sigmoid"])
def test_clip_evaluation(fams, name):
    """wwhip.evaluate.clip_posteriors_set over 5 clips of 1.5 s: member k's one-window value is column ``posterior_index`` of the
    window clips_forward_dev evaluates on member k's engine, within tests/test_gpu_rnn_cells.py::test_clip_and_plugin_paths' rule
    (1e-4 absolute: the clip pass stages the clips its own way), and within TAU_STREAM of float64 on the zero-padded window of
    Engine.logmel's rows; with ``crnn_slide_min`` = 1 the sliding lists are the bits clip_posteriors gives on the member's engine.
    Measured on an MI355X: max|one-window value - clips_forward_dev's| 0 on both families; needed tau c-std-n8 8.1e-8,
    c-std-n1-sigmoid 1.1e-7."""
    import torch
    from wwhip.engine import frontend_params
    from wwhip.evaluate import clip_posteriors, clip_posteriors_set
    m = fams(name)
    f, ms = m.f, m.set
    pcm = f.pcm(5, 75, seed=5)
    assert pcm.shape == (5, 24000)
    ms.set_option("crnn_slide_min", 1)
    try:
        one, sliding = clip_posteriors_set(ms, list(pcm))
    finally:
        ms.set_option("crnn_slide_min", 64)
    assert one.shape == (S64.K, 5) and len(sliding) == S64.K
    wins = np.zeros((5, f.T, f.n_mel), np.float32)
    for i, mel in enumerate(m.engines[0].logmel(list(pcm))):
        n = min(len(mel), f.T)
        wins[i, :n] = mel[:n]
    d_pcm = torch.from_numpy(pcm).cuda()
    for k, e in enumerate(m.engines):
        d_out = torch.full((5, e.n_out), -1.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        e.clips_forward_dev(d_pcm.data_ptr(), 5, 24000, d_out.data_ptr(), frontend_params())
        e.ctx.synchronize()
        got = d_out.cpu().numpy()
        np.testing.assert_array_equal(got, e.forward(wins))
        print(f"\nGEO64 {name} clip_posteriors_set member {k}: max|one - clips_forward_dev| {np.abs(one[k] - got[:, f.col]).max():.2e}", end="")
        assert np.abs(one[k] - got[:, f.col]).max() < 1e-4
        _post(f"{name} clip_posteriors_set, member {k}", one[k][:, None], f.ref64(k, wins)[0][:, f.col][:, None], TAU_STREAM, absolute=False)
        own_one, own_sliding = clip_posteriors(e, list(pcm))
        np.testing.assert_array_equal(one[k], own_one)
        assert len(sliding[k]) == 5
        for i in range(5):
            assert len(own_sliding[i]) > 0
            np.testing.assert_array_equal(sliding[k][i], own_sliding[i], err_msg=f"member {k}, clip {i}")
