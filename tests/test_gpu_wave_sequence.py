"""The Wavenet's sequence form on the MI355X: ``Engine.sequence_forward`` and the causal ``StreamBank``.

Two kinds of checks.  SAME BITS as what exists (``assert_array_equal``): a sequence of exactly ``T`` rows is the window form; a
late row's encoder output is the last row of the window that ends there; neither the cuts of a long sequence nor its neighbours
in a ragged call show in any output; a causal bank driven tick by tick emits ``post_frames`` of the rows it produced.  And
AGAINST FLOAT64 (tests/wave_sequence64.py, pinned to ``oracle.ref64`` by tests/test_wave_sequence64.py) through ``oracle.ref64``'s
checks with the bounds tests/test_gpu_ref64.py holds for the fp32 window kernel - the per-row arithmetic is the same.

Inputs: seeded synthetic PCM (noise + chirp) through ``Engine.logmel``, seeded random mel, all-floor rows (silence) and constant
rows, at lengths 1, 15, 16, 17, 180, 181, 182, 183, 500, 4,097 and 20,011 rows, for both Wavenet model directories.
"""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import ref64 as R
from wave_sequence64 import WaveSeq64

pytestmark = pytest.mark.gpu

MODELS = ["Wavenet", "Wavenet_alt"]
LENGTHS = [1, 15, 16, 17, 180, 181, 182, 183, 500, 4097, 20011]
TAU = 4e-5       # fp32 posteriors: the value tests/test_gpu_ref64.py holds for the window kernel
TAU_E = 1.2e-5   # fp32 encoder output, relative to max(1, max|row|): likewise
# head logits, max|z - z64| / max(1, max|z64 row|): the project had no bound.  Measured on these inputs on an MI355X: 2.0e-6
# (Wavenet), 9.0e-6 (Wavenet_alt); the bound is 4x the larger, as the project's other tolerances are.
TAU_Z = 3.6e-5
ALL = ("enc", "logits", "post_frames", "post")


def _pcm(rng, n):
    t = np.arange(n) / 16000.0
    chirp = 8000.0 * np.sin(2 * np.pi * (200.0 * t + 0.5 * 3800.0 / 1.5 * np.mod(t, 1.5) * np.mod(t, 1.5)))
    return np.clip(np.rint(rng.normal(0, 2000, n) + chirp), -32768, 32767).astype(np.int16)


def _random_mel(rng, rows):
    base = np.cumsum(rng.normal(0, 0.15, (rows, 40)), axis=0)
    base -= base.mean(axis=0)
    return np.maximum(base + rng.normal(0, 0.5, (rows, 40)), -2.0).astype(np.float32)


@pytest.fixture(scope="module")
def engines(assets):
    from wwhip.engine import Engine
    out = {m: Engine(os.path.join(assets, m)) for m in MODELS}
    yield out
    for e in out.values():
        e.close()


@pytest.fixture(scope="module")
def seq64(engines):
    return {m: WaveSeq64(e.bundle.wavenet) for m, e in engines.items()}


@pytest.fixture(scope="module")
def cases(engines):
    """name -> list of (label, mel [L, 40]) - the same inputs for every test of a model."""
    out = {}
    for name, eng in engines.items():
        rng = np.random.default_rng(2024)
        long_mel = eng.logmel([_pcm(rng, 512 + 160 * (max(LENGTHS) - 1))])[0]
        assert len(long_mel) == max(LENGTHS)
        floor_row = eng.logmel([np.zeros(512, np.int16)])[0][0]
        seqs = []
        for i, L in enumerate(LENGTHS):  # PCM through the front end: every length, cut from different places of the recording
            a = 0 if L == max(LENGTHS) else (37 * i) % (len(long_mel) - L)
            seqs.append((f"pcm{L}", np.ascontiguousarray(long_mel[a:a + L])))
        for L in (1, 17, 183, 500, 4097):
            seqs.append((f"random{L}", _random_mel(rng, L)))
        for L in (16, 182, 500):
            seqs.append((f"silence{L}", np.tile(floor_row, (L, 1))))
            seqs.append((f"constant{L}", np.full((L, 40), np.float32(0.75))))
        out[name] = seqs
    return out


@pytest.fixture(scope="module")
def results(engines, cases):
    """Every case of a model in ONE ragged call, all four outputs."""
    out = {}
    for name, eng in engines.items():
        got = eng.sequence_forward([m for _, m in cases[name]], want=ALL)
        out[name] = {lab: {k: got[k][i] for k in ALL} for i, (lab, _) in enumerate(cases[name])}
    return out


def _same(a, b, what):
    for k in ALL:
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{what}: {k}")


# ---------------------------------------------------------------------------------------------- same bits as what exists
@pytest.mark.parametrize("model", MODELS)
def test_a_window_long_sequence_is_the_window_form(engines, cases, results, model):
    """L == T: ``post`` is ``Engine.forward``'s row and ``enc`` is ``forward(want_enc=True)``'s - alone and inside the ragged batch."""
    eng = engines[model]
    for lab, mel in cases[model]:
        if len(mel) != eng.window:
            continue
        post, enc = eng.forward(mel, want_enc=True)
        alone = eng.sequence_forward([mel], want=ALL)
        for got, how in ((alone_i(alone), "alone"), (results[model][lab], "in the batch")):
            np.testing.assert_array_equal(got["post"], post[0], err_msg=f"{lab} {how}")
            np.testing.assert_array_equal(got["enc"], enc[0], err_msg=f"{lab} {how}")
            # P = T over T rows: the last frame posterior pools the whole window
            np.testing.assert_array_equal(got["post_frames"][-1], post[0], err_msg=f"{lab} {how}")


def alone_i(d, i=0):
    return {k: d[k][i] for k in ALL}


@pytest.mark.parametrize("model", MODELS)
def test_a_late_row_is_the_last_row_of_the_window_that_ends_there(engines, cases, results, model):
    """For t >= T - 1, ``enc[t]`` equals row T - 1 of the encoder output of the window ending at t, bit for bit."""
    eng = engines[model]
    T = eng.window
    for lab in ("pcm183", "pcm500", "random500", "silence500", "pcm4097", "pcm20011"):
        mel = dict(cases[model])[lab]
        ts = np.arange(T - 1, len(mel)) if len(mel) <= 500 else np.unique(np.r_[T - 1, np.arange(T + 5, len(mel), max(1, len(mel) // 300)), len(mel) - 1])
        wins = np.stack([mel[t - T + 1:t + 1] for t in ts])
        _, enc = eng.forward(wins, want_enc=True)
        np.testing.assert_array_equal(results[model][lab]["enc"][ts], enc[:, T - 1], err_msg=lab)


@pytest.mark.parametrize("model", MODELS)
def test_the_cuts_do_not_show(engines, cases, results, model):
    """``wave_seq_segment`` at 256, at a value larger than any sequence and at 0 (the library's choice): identical outputs, all
    four arrays, for the longest sequences and the whole ragged batch."""
    eng = engines[model]
    labs = [lab for lab, m in cases[model]]
    mels = [m for _, m in cases[model]]
    for seg in (256, 1 << 20, 191, 0):
        with eng.options(wave_seq_segment=seg):
            got = eng.sequence_forward(mels, want=ALL)
        for i, lab in enumerate(labs):
            _same(alone_i(got, i), results[model][lab], f"{lab} at segment {seg}")


@pytest.mark.parametrize("model", MODELS)
def test_neighbours_do_not_show(engines, cases, results, model):
    """A sequence alone and the same sequence between others in one call."""
    eng = engines[model]
    for lab, mel in cases[model]:
        if len(mel) > 5000:
            continue
        _same(alone_i(eng.sequence_forward([mel], want=ALL)), results[model][lab], lab)
    # a single output asked for on its own is the same array
    lab, mel = cases[model][8]
    for k in ALL:
        np.testing.assert_array_equal(eng.sequence_forward(mel, want=(k,))[k][0], results[model][lab][k], err_msg=k)


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("pool", [0, 1, 50, 128, 1000])
def test_other_pools(engines, cases, model, pool):
    """``post_frames`` at other pool lengths: softmax of the literal trailing maximum of the call's own ``logits`` (a maximum is
    exact) to within 4 x 2^-23 (expf within 2 ulps, the sum and the quotient half an ulp each: under 4 fp32 ulps of a value that is
    at most 1); ``pool=0`` ends in ``post``."""
    eng = engines[model]
    mels = [m for lab, m in cases[model] if lab in ("pcm17", "pcm183", "pcm500", "random4097")]
    got = eng.sequence_forward(mels, pool=pool, want=("logits", "post_frames", "post"))
    for z, pf, post in zip(got["logits"], got["post_frames"], got["post"]):
        m = z.copy()
        P = len(z) if pool == 0 else min(pool, len(z))
        for k in range(1, P):
            m[k:] = np.maximum(m[k:], z[:-k])
        e = np.exp(m.astype(np.float64) - m.max(axis=1, keepdims=True))
        want = e / e.sum(axis=1, keepdims=True)
        assert np.abs(pf - want).max() <= 4 * 2.0 ** -23
        if pool == 0:
            np.testing.assert_array_equal(pf[-1], post)


def _drive(eng, S, ticks, seed, sync_wait):
    """A causal bank tick by tick.  Returns per stream: the mel rows the bank produced, split at its resets, and per row whether
    (and what) it emitted."""
    from wwhip.engine import StreamBank
    rng = np.random.default_rng(seed)
    T = eng.window
    bank = StreamBank(eng, S, sync_wait=sync_wait, causal=True)
    pcm = np.stack([_pcm(rng, ticks * 320) for _ in range(S)])
    pcm[3] = 0                                               # a silent stream
    speech = (rng.random((ticks, S)) < 0.7).astype(np.uint8)
    speech[:, 5] = 1
    speech[:, 6] = 0                                         # a stream that never emits
    active = np.zeros((ticks, S), np.uint8)
    active[60:75, 10:40] = 1                                 # an active stretch: the stream stands still
    active[200:203, 7] = 1
    fill = np.zeros(S, int)
    segs = [[[]] for _ in range(S)]                          # stream -> segments -> (mel row, emitted posterior or None)
    try:
        for t in range(ticks):
            if t == 150:
                ids = list(range(0, 21)) + [S - 1]
                bank.reset(ids)
                for s in ids:
                    fill[s] = 0
                    segs[s].append([])
            if t == 220:
                bank.reset()
                fill[:] = 0
                for s in range(S):
                    segs[s].append([])
            post, n = bank.step(pcm[:, t * 320:(t + 1) * 320], speech[t], active[t])
            for s in range(S):
                nf = 0
                if not active[t, s]:
                    tot = fill[s] + 320
                    nf = (tot - 512) // 160 + 1 if tot >= 512 else 0
                    fill[s] = tot - nf * 160
                emit = nf if speech[t, s] and not active[t, s] else 0
                assert n[s] == emit, (t, s, n[s], emit)
                if nf:
                    win = bank.window(s)
                    for k in range(nf):
                        segs[s][-1].append((win[T - nf + k].copy(), post[s, k] if emit else None))
    finally:
        bank.close()
    return segs


@pytest.mark.parametrize("sync_wait", [False, True], ids=["polled", "sync_wait"])
@pytest.mark.parametrize("model", MODELS)
def test_a_causal_bank_emits_the_frame_posteriors_of_its_own_rows(engines, model, sync_wait):
    """128 streams, 300 ticks, mixed ``is_speech``, an active stretch, a reset of some streams and one of all: every emitted
    posterior equals ``post_frames[t][posterior column]`` of ``sequence_forward`` over the mel rows the bank itself produced
    since the stream's last reset (read back through ``StreamBank.window`` after each tick), and ``n_post`` follows the sample
    count and the flags."""
    eng = engines[model]
    S, ticks = 128, 300
    segs = _drive(eng, S, ticks, 99, sync_wait)
    seqs, emitted = [], []
    for s in range(S):
        for seg in segs[s]:
            if seg:
                seqs.append(np.stack([r for r, _ in seg]))
                emitted.append([p for _, p in seg])
    assert sum(len(x) for x in seqs) > S * ticks and max(len(x) for x in seqs) > eng.window
    pf = eng.sequence_forward(seqs, want=("post_frames",))["post_frames"]
    n = 0
    for f, em in zip(pf, emitted):
        idx = [i for i, p in enumerate(em) if p is not None]
        np.testing.assert_array_equal(np.array([em[i] for i in idx], np.float32), f[idx, eng.posterior_index])
        n += len(idx)
    assert n > S * ticks // 2


# ---------------------------------------------------------------------------------------------- against float64
@pytest.mark.parametrize("model", MODELS)
def test_against_float64(engines, seq64, cases, results, model):
    """``check_enc`` on ``enc`` (every row a row of the check) with TAU_E = 1.2e-5, ``check_posteriors`` on ``post`` and
    ``post_frames`` with TAU = 4e-5, ``logits`` within TAU_Z = 3.6e-5 of max(1, max|z64 row|) (4x the measured).  Measured on an
    MI355X, worst case of Wavenet / Wavenet_alt: enc needs 7.6e-7 / 3.7e-6, post 2.1e-6 / 5.4e-6, post_frames 2.2e-6 / 7.7e-6,
    logits 2.0e-6 / 9.0e-6."""
    worst = dict(enc=0.0, post=0.0, post_frames=0.0, logits=0.0)
    for lab, mel in cases[model]:
        want = seq64[model].sequence(mel)
        got = results[model][lab]
        need_e = float(R.enc_ratios(got["enc"], want["enc"], 1.0).max())
        need_p = R.needed_tau(got["post"][None], want["post"][None])
        need_f = R.needed_tau(got["post_frames"], want["post_frames"])
        need_z = float((np.abs(got["logits"] - want["logits"]).max(axis=1) / np.maximum(1.0, np.abs(want["logits"]).max(axis=1))).max())
        print(f"\nSEQ64 {model} {lab}: enc needs {need_e:.2e} (tau_e {TAU_E:g}), post {need_p:.2e}, post_frames {need_f:.2e} "
              f"(tau {TAU:g}), logits {need_z:.2e} (tau_z {TAU_Z:g})", end="")
        for k, v in (("enc", need_e), ("post", need_p), ("post_frames", need_f), ("logits", need_z)):
            worst[k] = max(worst[k], v)
    print(f"\nSEQ64 {model} worst: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()), end="")
    for lab, mel in cases[model]:
        want = seq64[model].sequence(mel)
        got = results[model][lab]
        R.check_enc(got["enc"], want["enc"], TAU_E)
        R.check_posteriors(got["post"][None], want["post"][None], TAU)
        R.check_posteriors(got["post_frames"], want["post_frames"], TAU)
        dz = np.abs(got["logits"] - want["logits"]).max(axis=1) / np.maximum(1.0, np.abs(want["logits"]).max(axis=1))
        assert dz.max() <= TAU_Z, (lab, float(dz.max()))


# ---------------------------------------------------------------------------------------------- refusals, degenerate sizes
def test_refusals_and_degenerate_sizes(engines, assets):
    from wwhip import _lib
    from wwhip.engine import Engine, frontend_params
    lib = _lib.load()
    eng = engines["Wavenet"]
    mel = _random_mel(np.random.default_rng(3), 400)
    offs = np.array([0, 100, 100, 400], np.int64)
    post = np.full((3, eng.n_out), 7.0, np.float32)
    pf = np.full((400, eng.n_out), 7.0, np.float32)

    def call(e, offs, n_seq, pool, total=400):
        return lib.ww_wave_sequence(e.ctx.handle, e.handle, _lib.ptr(mel), total, _lib.ptr(offs), n_seq, pool, None, None, _lib.ptr(pf), _lib.ptr(post))

    assert call(eng, offs, 3, eng.window) == _lib.WW_OK
    assert np.all(post[1] == 7.0) and not np.any(post[[0, 2]] == 7.0) and not np.any(pf == 7.0)  # an empty sequence is a no-op
    post[:] = 7.0
    assert call(eng, offs, 0, eng.window) == _lib.WW_OK and np.all(post == 7.0)                  # no sequences
    assert call(eng, np.array([5, 5], np.int64), 1, 0) == _lib.WW_OK and np.all(post == 7.0)     # only empty ones
    assert call(eng, offs, -1, eng.window) == _lib.WW_EINVAL
    assert call(eng, offs, 3, -1) == _lib.WW_EINVAL
    assert call(eng, np.array([0, 200, 100, 400], np.int64), 3, 0) == _lib.WW_EINVAL             # descending offsets
    assert call(eng, offs, 3, 0, total=399) == _lib.WW_EINVAL                                    # offsets leave the buffer
    assert lib.ww_wave_sequence_dev(eng.ctx.handle, eng.handle, None, 400, _lib.ptr(offs), 3, -1, None, None, None, None) == _lib.WW_EINVAL
    with pytest.raises(ValueError):
        eng.sequence_forward([mel], want=("posterior",))
    for kw in (dict(model="CRNN"), dict(model="Wavenet", precision="bf16x3")):
        other = Engine(os.path.join(assets, kw["model"]), precision=kw.get("precision", "fp32"))
        try:
            assert call(other, offs, 3, 0) == _lib.WW_EINVAL, kw
            h = C.c_void_p()
            fp = frontend_params()
            assert lib.ww_stream_create(other.ctx.handle, other.handle, 4, C.byref(fp), _lib.STREAM_CAUSAL, C.byref(h)) == _lib.WW_EINVAL, kw
        finally:
            other.close()
    h = C.c_void_p()
    fp = frontend_params()
    assert lib.ww_stream_create(eng.ctx.handle, eng.handle, 4, C.byref(fp), _lib.STREAM_CAUSAL | _lib.STREAM_FULL_RECOMPUTE,
                                C.byref(h)) == _lib.WW_EINVAL
    assert not h.value


# ------------------------------------------------- one path for a model and a model set: outputs asked for, rows outside, bad calls
EDGE_LENGTHS = [0, 1, 180, 181, 193, 400]   # around the receptive field (181) and a chunk (192); 400 rows at 256: two segments
EDGE_FRONT, EDGE_BEHIND = 7, 5              # rows of the buffers in front of the first sequence and behind the last
EDGE_SEGMENT = 256                          # test_the_cuts_do_not_show's: the 400-row sequence is cut
EDGE_EMPTY = EDGE_LENGTHS.index(0)
SENTINEL = -7.0


@pytest.fixture(scope="module")
def edge(engines):
    """The small batch of the tests below, per model: its sequences, all four outputs of ONE ``sequence_forward`` call (computed
    once, never written to) and a one-member ``ModelSet`` on the same engine, both cutting at EDGE_SEGMENT."""
    from wwhip.engine import ModelSet
    rng = np.random.default_rng(20261020)
    seqs = [_random_mel(rng, n) if n else np.zeros((0, 40), np.float32) for n in EDGE_LENGTHS]
    out, sets = {}, []
    for name, eng in engines.items():
        ms = ModelSet([eng])
        ms.set_option("wave_seq_segment", EDGE_SEGMENT)
        sets.append(ms)
        with eng.options(wave_seq_segment=EDGE_SEGMENT):
            ref = eng.sequence_forward(seqs, want=ALL)
        for k in ALL:
            for a in ref[k]:
                a.setflags(write=False)
        out[name] = (seqs, ref, ms)
    yield out
    for ms in sets:
        ms.close()


@pytest.mark.parametrize("model", MODELS)
def test_every_subset_of_the_outputs_carries_the_same_bits(engines, edge, model):
    """Every non-empty subset of the four outputs, through ``Engine.sequence_forward`` and through a one-member set's
    ``sequence_forward_all``: what comes back is what was asked for, and each array equals the all-four call's, bit for bit -
    whether the logits and the pooling buffers are the caller's or the plan's scratch."""
    import itertools
    eng = engines[model]
    seqs, ref, ms = edge[model]
    for r in range(1, len(ALL) + 1):
        for want in itertools.combinations(ALL, r):
            with eng.options(wave_seq_segment=EDGE_SEGMENT):
                one = eng.sequence_forward(seqs, want=want)
            every = ms.sequence_forward_all(seqs, want=want)
            assert tuple(one) == want and tuple(every) == want
            for k in want:
                assert len(one[k]) == len(every[k][0]) == len(seqs) and len(every[k]) == 1
                for i in range(len(seqs)):
                    if k == "post" and i == EDGE_EMPTY:
                        assert np.isnan(one[k][i]).all() and np.isnan(every[k][0][i]).all()
                        continue
                    np.testing.assert_array_equal(one[k][i], ref[k][i], err_msg=f"model, want {want}: {k} of sequence {i}")
                    np.testing.assert_array_equal(every[k][0][i], ref[k][i], err_msg=f"set, want {want}: {k} of sequence {i}")


def _edge_buffers(seqs, n_out):
    """The batch in one buffer with EDGE_FRONT rows of NaN in front and EDGE_BEHIND behind, its offsets, and outputs full of SENTINEL."""
    mel = np.concatenate([np.full((EDGE_FRONT, 40), np.nan, np.float32)] + seqs + [np.full((EDGE_BEHIND, 40), np.nan, np.float32)])
    offs = (EDGE_FRONT + np.concatenate([[0], np.cumsum(EDGE_LENGTHS)])).astype(np.int64)
    total = len(mel)
    shape = {"enc": (total, 32), "logits": (total, n_out), "post_frames": (total, n_out), "post": (len(seqs), n_out)}
    return mel, offs, {k: np.full(shape[k], SENTINEL, np.float32) for k in ALL}


def _check_edge(got, offs, ref, what):
    """Rows of sequence i are the reference's; every other row, and the empty sequence's ``post``, is still SENTINEL."""
    for i in range(len(EDGE_LENGTHS)):
        a, b = int(offs[i]), int(offs[i + 1])
        for k in ("enc", "logits", "post_frames"):
            np.testing.assert_array_equal(got[k][a:b], ref[k][i], err_msg=f"{what}: {k} of sequence {i}")
        if i != EDGE_EMPTY:
            np.testing.assert_array_equal(got["post"][i], ref["post"][i], err_msg=f"{what}: post of sequence {i}")
    for k in ("enc", "logits", "post_frames"):
        assert (got[k][:int(offs[0])] == SENTINEL).all() and (got[k][int(offs[-1]):] == SENTINEL).all(), (what, k)
        assert len(got[k][:int(offs[0])]) == EDGE_FRONT and len(got[k][int(offs[-1]):]) == EDGE_BEHIND
    assert (got["post"][EDGE_EMPTY] == SENTINEL).all(), what


@pytest.mark.parametrize("model", MODELS)
def test_rows_outside_the_sequences_are_neither_read_nor_written(engines, edge, model):
    """``ww_wave_sequence`` and ``ww_wave_sequence_dev`` on buffers with rows in front of the first sequence and behind the last:
    those mel rows hold NaN and the results are the unpoisoned run's, bit for bit; those output rows, and the empty sequence's
    ``post``, keep the bytes they had."""
    import torch
    from wwhip import _lib
    lib = _lib.load()
    eng = engines[model]
    seqs, ref, _ = edge[model]
    mel, offs, host = _edge_buffers(seqs, eng.n_out)
    with eng.options(wave_seq_segment=EDGE_SEGMENT):
        rc = lib.ww_wave_sequence(eng.ctx.handle, eng.handle, _lib.ptr(mel), len(mel), _lib.ptr(offs), len(seqs), eng.window,
                                  *[_lib.ptr(host[k]) for k in ALL])
        assert rc == _lib.WW_OK, lib.ww_last_error(eng.ctx.handle)
        _check_edge(host, offs, ref, "host")
        d_mel = torch.from_numpy(mel).cuda()
        dev = {k: torch.full(v.shape, SENTINEL, dtype=torch.float32, device="cuda") for k, v in host.items()}
        torch.cuda.synchronize()
        eng.wave_sequence_dev(d_mel.data_ptr(), len(mel), offs, None, *[dev[k].data_ptr() for k in ALL])
        eng.ctx.synchronize()
        _check_edge({k: v.cpu().numpy() for k, v in dev.items()}, offs, ref, "dev")


def test_one_table_of_bad_calls_for_the_six_entry_points(engines, edge, assets):
    """Negative ``n_seq``, pool and rows, descending offsets, offsets past ``total_rows``, NULL mel with a non-empty sequence, a
    CRNN model / set and - single model - a split-bf16 model: WW_EINVAL from each of the six entry points, with outputs full of
    SENTINEL untouched.  ``n_seq == 0``, only empty sequences and no output pointer: WW_OK, outputs untouched."""
    import torch
    from wwhip import _lib
    from wwhip.engine import Engine, ModelSet
    lib = _lib.load()
    eng = engines["Wavenet"]
    seqs, _, ms = edge["Wavenet"]
    ctx = eng.ctx.handle
    mel, offs, host = _edge_buffers(seqs, eng.n_out)
    total, n_seq = len(mel), len(seqs)
    d_mel = torch.from_numpy(mel).cuda()
    dev = {k: torch.full(v.shape, SENTINEL, dtype=torch.float32, device="cuda") for k, v in host.items()}
    torch.cuda.synchronize()
    crnn = Engine(os.path.join(assets, "CRNN_nosilence"), ctx=eng.ctx)
    crnn_set = ModelSet([crnn])
    bf16 = Engine(os.path.join(assets, "Wavenet"), precision="bf16x3", ctx=eng.ctx)
    member0 = np.zeros(1, np.int32)
    route0 = np.zeros(n_seq, np.int32)
    OMIT = object()

    def entry(name):
        """-> call(**changes) for the entry point, and the models it refuses"""
        on_dev = name.endswith("_dev")
        single = not name.startswith("ww_set_")
        good = eng.handle if single else ms.handle
        the_mel = C.c_void_p(d_mel.data_ptr()) if on_dev else _lib.ptr(mel)
        outs = [C.c_void_p(dev[k].data_ptr()) for k in ALL] if on_dev else [_lib.ptr(host[k]) for k in ALL]

        def call(model=good, m=OMIT, rows=total, ro=offs, n=n_seq, pool=50, o=OMIT):
            ro = np.ascontiguousarray(ro, np.int64)
            args = [ctx, model, the_mel if m is OMIT else m, rows, _lib.ptr(ro), n]
            if single:
                args += [pool]
            elif "_all" in name:
                args += [pool, _lib.ptr(member0), 1]
            else:
                args += [_lib.ptr(route0), pool]
            rc = getattr(lib, name)(*args, *(outs if o is OMIT else [None] * 4))
            eng.ctx.synchronize()
            return rc
        return call, ([crnn.handle, bf16.handle] if single else [crnn_set.handle])

    def untouched():
        return all((v == SENTINEL).all() for v in host.values()) and all(bool((v == SENTINEL).all()) for v in dev.values())

    down = offs.copy()
    down[4] = down[3] - 1
    empty = np.full(n_seq + 1, 9, np.int64)
    try:
        for name in ("ww_wave_sequence", "ww_wave_sequence_dev", "ww_set_wave_sequence", "ww_set_wave_sequence_dev",
                     "ww_set_wave_sequence_all", "ww_set_wave_sequence_all_dev"):
            call, refused_models = entry(name)
            bad = [dict(n=-1), dict(pool=-1), dict(rows=-1), dict(ro=down), dict(rows=total - EDGE_BEHIND - 1), dict(m=None)]
            bad += [dict(model=h) for h in refused_models]
            for kw in bad:
                assert call(**kw) == _lib.WW_EINVAL, (name, kw)
                assert len(lib.ww_last_error(ctx)) > 8, (name, kw)
                assert untouched(), (name, kw)
            for kw in (dict(n=0), dict(ro=empty), dict(o=None)):
                assert call(**kw) == _lib.WW_OK, (name, kw, lib.ww_last_error(ctx))
                assert untouched(), (name, kw)
    finally:
        crnn_set.close()
        crnn.close()
        bf16.close()
