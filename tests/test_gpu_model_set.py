"""Model sets (``ww_model_set``, ``wwhip.ModelSet``): several models of one geometry behind one launch and one stream bank.

The yardstick is the library's own single-model path: member ``k`` evaluated through a set equals ``Engine(member k)`` BIT FOR BIT
(``np.testing.assert_array_equal``) - a batch row against the member's ``forward_windows_dev`` row at the same launch size, a stream
of a mixed bank against the same stream of a bank of its member alone.  The batch rows are also held against the float64 statement
of ``oracle/ref64.py`` with the fp32 posterior bound of ``tests/test_gpu_ref64.py:21`` (``TAU = 4e-5``).

Members: ``CRNN_nosilence``, ``CRNN_nosilence_enhanced``, ``CRNN_softmax`` (one geometry, softmax heads) and ``Wavenet``,
``Wavenet_alt`` (same sizes, dilations, block order and residual convs) - the shipped files as they are: set creation accepts
both groups, so no member had to be built from a perturbed blob."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import ref64 as R

pytestmark = pytest.mark.gpu

CRNNS = ["CRNN_nosilence", "CRNN_nosilence_enhanced", "CRNN_softmax"]
WAVES = ["Wavenet", "Wavenet_alt"]
TAU = 4e-5  # fp32 posteriors against Ref64: tests/test_gpu_ref64.py:21


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


def _member_rows(e, d_mel, mel_rows, d_row, d_valid, n):
    import torch
    out = torch.full((n, e.n_out), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    e.forward_windows_dev(d_mel.data_ptr(), mel_rows, d_row.data_ptr(), d_valid.data_ptr(), n, out.data_ptr())
    e.ctx.synchronize()
    return out.cpu().numpy()


def _set_rows(ms, d_mel, mel_rows, d_row, d_valid, ids, n, want_enc):
    import torch
    out = torch.full((n, ms.n_out), -7.0, dtype=torch.float32, device="cuda")
    enc = torch.full((n,) + ms.enc_shape, -7.0, dtype=torch.float32, device="cuda") if want_enc else None
    torch.cuda.synchronize()
    ms.forward_windows_dev(d_mel.data_ptr(), mel_rows, d_row.data_ptr(), d_valid.data_ptr(), ids, n, out.data_ptr(),
                           enc.data_ptr() if want_enc else 0)
    ms.ctx.synchronize()
    return out.cpu().numpy(), (enc.cpu().numpy() if want_enc else None)


def _padded(mel, rows, valid, T):
    wins = np.zeros((len(rows), T, mel.shape[1]), np.float32)
    for i, (r, v) in enumerate(zip(rows, valid)):
        wins[i, :v] = mel[r:r + v]
    return wins


def _batch_case(ms, members, assets, names, rows, valid, ids, seed, with_ref64=True):
    """Windows of partial validity over a random mel, window w by member ids[w]: every row (and encoder row) equals the member
    engine's, bit for bit; ``forward_all`` row [k] equals member k on all windows; with ``with_ref64`` every row is within the
    Ref64 bound."""
    import torch
    T, n = ms.window, len(rows)
    rng = np.random.default_rng(seed)
    mel = rng.uniform(0, 6.5, (400, ms.n_mel)).astype(np.float32)
    d_mel = torch.from_numpy(mel).cuda()
    d_row = torch.from_numpy(np.asarray(rows, np.int64)).cuda()
    d_valid = torch.from_numpy(np.asarray(valid, np.int32)).cuda()
    per_member = [_member_rows(e, d_mel, 400, d_row, d_valid, n) for e in members]
    got, enc = _set_rows(ms, d_mel, 400, d_row, d_valid, ids, n, True)
    wins = _padded(mel, rows, valid, T)
    for w in range(n):
        np.testing.assert_array_equal(got[w], per_member[ids[w]][w], err_msg=f"window {w} by member {ids[w]}")
    # the encoder rows: member k on ALL n windows in one launch (the set's launch size, so the same launch form), row w by ids[w]
    enc_member = [e.forward(wins, want_enc=True)[1] for e in members]
    for w in range(n):
        np.testing.assert_array_equal(enc[w], enc_member[ids[w]][w].reshape(enc[w].shape), err_msg=f"encoder rows of window {w}")
    every, every_enc = ms.forward_all(wins, want_enc=True)
    assert every.shape == (len(members), n, ms.n_out)
    for k in range(len(members)):
        np.testing.assert_array_equal(every[k], per_member[k], err_msg=f"forward_all, member {k}")
        np.testing.assert_array_equal(every_enc[k], enc_member[k].reshape(every_enc[k].shape), err_msg=f"forward_all encoder, member {k}")
    if with_ref64:
        for k, name in enumerate(names):
            sel = [w for w in range(n) if ids[w] == k]
            want64 = R.Ref64(os.path.join(assets, name)).forward(wins[sel])[0]
            print(f"\nREF64 set member {name}: needs tau {R.needed_tau(got[sel], want64):.2e} (tau {TAU:g})", end="")
            R.check_posteriors(got[sel], want64, TAU)
    return got


def test_batch_crnn(crnn_set, engines, assets):
    """8 windows over a 400-row mel, valid rows {151, 151, 40, 1, 151, 97, 151, 3}, members [0, 1, 2, 2, 1, 0, 1, 2]."""
    rows = [0, 7, 100, 399, 249, 13, 200, 397]
    valid = [151, 151, 40, 1, 151, 97, 151, 3]
    _batch_case(crnn_set, [engines[m] for m in CRNNS], assets, CRNNS, rows, valid, [0, 1, 2, 2, 1, 0, 1, 2], 11)


def test_batch_wavenet(wave_set, engines, assets):
    """The same check with 6 windows (twelve-wave form), and 300 windows by members w % 2 (the four-wave form above 256) against the
    members at the same launch size: posteriors, encoder rows and ``forward_all`` bit for bit (Ref64 on the 6 windows only: its
    float64 Wavenet over 300 windows is minutes)."""
    rows = [0, 9, 100, 399, 218, 397]
    valid = [182, 182, 40, 1, 182, 3]
    members = [engines[m] for m in WAVES]
    _batch_case(wave_set, members, assets, WAVES, rows, valid, [0, 1, 1, 0, 1, 0], 12)
    rng = np.random.default_rng(13)
    rows = rng.integers(0, 400 - 182, 300).tolist()
    valid = np.where(rng.uniform(size=300) < 0.8, 182, rng.integers(1, 182, 300)).tolist()
    _batch_case(wave_set, members, assets, WAVES, rows, valid, [w % 2 for w in range(300)], 14, with_ref64=False)


def _tick_inputs(seed, ticks, S):
    rng = np.random.default_rng(seed)
    pcm = np.clip(rng.normal(0, 2500, (ticks, S, 320)), -32768, 32767).astype(np.int16)
    speech = (rng.uniform(size=(ticks, S)) < 0.85).astype(np.uint8)
    speech[:, 0] = 1                      # one stream never pauses: its rings wrap
    speech[20:23] = 0                     # whole ticks without a window
    active = np.zeros((ticks, S), np.uint8)
    active[ticks // 3:ticks // 3 + 8, S - 2] = 1  # an active stretch: the stream is not sampled
    return pcm, speech, active


def _run_bank(bank, pcm, speech, active, resets, t0=0):
    out = []
    for t in range(t0, len(pcm)):
        for ids in resets.get(t, []):
            bank.reset(ids)
        out.append(bank.step(pcm[t], speech[t], active[t]))
    return out


def _mixed_bank_case(ms, members, models, ticks, seed, fp, resets, **kw):
    """A bank whose stream s is served by member models[s] against one bank per member, all fed the same frames: post and n_post of
    stream s equal those of the bank of models[s], every tick, bit for bit."""
    from wwhip.engine import StreamBank
    S = len(models)
    pcm, speech, active = _tick_inputs(seed, ticks, S)
    bank = StreamBank(ms, S, fp, models=models, **kw)
    try:
        got = _run_bank(bank, pcm, speech, active, resets)
    finally:
        bank.close()
    n_total = 0
    for k, e in enumerate(members):
        solo = StreamBank(e, S, fp, **kw)
        try:
            want = _run_bank(solo, pcm, speech, active, resets)
        finally:
            solo.close()
        sel = [s for s in range(S) if models[s] == k]
        for t, ((p, n), (p1, n1)) in enumerate(zip(got, want)):
            np.testing.assert_array_equal(n[sel], n1[sel], err_msg=f"tick {t}, member {k}")
            np.testing.assert_array_equal(p[sel], p1[sel], err_msg=f"tick {t}, member {k}")
            n_total += int(n[sel].sum())
    return n_total


@pytest.mark.parametrize("two_launch", [False, True])
@pytest.mark.parametrize("sync_wait", [False, True])
def test_crnn_bank(crnn_set, engines, two_launch, sync_wait):
    """S = 6, members [0, 1, 2, 0, 1, 2], 100 ticks (stream 0: 180 rows before the bank's reset - past the 152 slots of the mel ring
    and the 144 of the projected-row cache), speech with gaps, an active stretch, a single-stream and a whole-bank reset,
    pre-emphasis 0.97."""
    from wwhip.engine import frontend_params
    n = _mixed_bank_case(crnn_set, [engines[m] for m in CRNNS], [0, 1, 2, 0, 1, 2], 100, 31, frontend_params(pre_emphasis=0.97),
                         {50: [[1]], 90: [None]}, two_launch=two_launch, sync_wait=sync_wait)
    assert n > 800


@pytest.mark.parametrize("form", ["one_launch", "two_launch", "causal"])
def test_wavenet_banks(wave_set, engines, form):
    """S = 4, members [0, 1, 1, 0], 40 ticks: the window bank in one launch per tick (wavenet_kernel<..., TICK, SET>) and in two
    (front-end kernel + wavenet_kernel<..., SET> over the tick's window table), and the causal bank by tick."""
    from wwhip.engine import frontend_params
    kw = {"one_launch": {}, "two_launch": {"two_launch": True}, "causal": {"causal": True}}[form]
    n = _mixed_bank_case(wave_set, [engines[m] for m in WAVES], [0, 1, 1, 0], 40, 32, frontend_params(pre_emphasis=0.97),
                         {15: [[2]], 30: [None]}, **kw)
    assert n > 100


def test_causal_bank_feed(wave_set, engines):
    """The causal bank by ``feed``: packets of {0, 100, 320, 511, 3000, 8000} samples (8,000 samples are 47 rows: the twelve-wave
    form) - rows, posteriors and a following ``step`` equal the single-model causal banks'."""
    from wwhip.engine import StreamBank
    models, S = [0, 1, 1, 0], 4
    rng = np.random.default_rng(33)
    sizes = [0, 100, 320, 511, 3000, 8000]
    calls = []
    for c in range(5):
        ids = [s for s in range(S) if rng.uniform() < 0.8] or [0]
        ks = [8000 if (c == 1 and i == 0) else int(rng.choice(sizes)) for i in range(len(ids))]
        calls.append((ids, [np.clip(rng.normal(0, 2500, k), -32768, 32767).astype(np.int16) for k in ks]))
    last = np.clip(rng.normal(0, 2500, (S, 320)), -32768, 32767).astype(np.int16)

    def run(eng, **kw):
        bank = StreamBank(eng, S, causal=True, **kw)
        try:
            out = [bank.feed(ids, pk, want_mel=True) for ids, pk in calls]
            return out, bank.step(last, np.ones(S, np.uint8))
        finally:
            bank.close()

    got, got_step = run(wave_set, models=models)
    rows = 0
    for k, name in enumerate(WAVES):
        want, want_step = run(engines[name])
        sel = [s for s in range(S) if models[s] == k]
        np.testing.assert_array_equal(got_step[1][sel], want_step[1][sel])
        np.testing.assert_array_equal(got_step[0][sel], want_step[0][sel])
        for (ids, _), (gp, gm), (wp, wm) in zip(calls, got, want):
            for i, s in enumerate(ids):
                if models[s] == k:
                    np.testing.assert_array_equal(gm[i], wm[i])
                    np.testing.assert_array_equal(gp[i], wp[i])
                    rows += len(gp[i])
    assert rows > 60


def test_set_model(crnn_set, engines):
    """Stream 2 of a CRNN bank moves from member 0 to member 1 at tick 30: from there on it is a fresh member-1 stream fed from
    tick 30; every other stream - and stream 2 before the call - is what a twin bank that never saw the call yields."""
    from wwhip.engine import StreamBank
    models, S, ticks = [0, 1, 0, 2, 1, 2], 6, 60
    pcm, speech, active = _tick_inputs(34, ticks, S)
    active[:] = 0
    bank, twin = StreamBank(crnn_set, S, models=models), StreamBank(crnn_set, S, models=models)
    fresh = StreamBank(engines[CRNNS[1]], S)
    try:
        for t in range(ticks):
            if t == 30:
                bank.set_model([2], 1)
            p, n = bank.step(pcm[t], speech[t])
            p2, n2 = twin.step(pcm[t], speech[t])
            rest = [s for s in range(S) if s != 2 or t < 30]
            np.testing.assert_array_equal(n[rest], n2[rest], err_msg=f"tick {t}")
            np.testing.assert_array_equal(p[rest], p2[rest], err_msg=f"tick {t}")
            if t >= 30:
                p3, n3 = fresh.step(pcm[t], speech[t])
                assert n[2] == n3[2], t
                np.testing.assert_array_equal(p[2], p3[2], err_msg=f"tick {t}")
    finally:
        for b in (bank, twin, fresh):
            b.close()


def test_contract(assets, engines, crnn_set):
    """Every WW_EINVAL of the set calls through ctypes, each followed by a valid call whose result is unchanged; n_windows = 0;
    a member freed after set creation; ww_model_set_info."""
    import torch
    from wwhip import _lib
    from wwhip.engine import Engine, ModelSet, StreamBank, frontend_params
    lib = _lib.load()
    ctx = crnn_set.ctx
    rng = np.random.default_rng(35)
    wins = rng.uniform(0, 6.5, (3, crnn_set.window, 40)).astype(np.float32)
    base = crnn_set.forward(wins, [2, 0, 1])

    def refused(rc, word=None):
        assert rc == _lib.WW_EINVAL, rc
        text = lib.ww_last_error(ctx.handle).decode()
        assert len(text) > 10 and (word is None or word in text), text
        np.testing.assert_array_equal(crnn_set.forward(wins, [2, 0, 1]), base)  # a valid call, unchanged

    def create(handles, n=None):
        arr = (C.c_void_p * max(len(handles), 1))(*[getattr(x, "value", x) for x in handles])
        h = C.c_void_p()
        rc = lib.ww_model_set_create(ctx.handle, arr, len(handles) if n is None else n, C.byref(h))
        assert rc != _lib.WW_OK or h.value
        if rc == _lib.WW_OK:
            lib.ww_model_set_destroy(h)
        return rc

    soft = engines["CRNN_softmax"]
    extra = {m: Engine(os.path.join(assets, m)) for m in ("CRNN", "CRNN_old")}
    bf16 = Engine(os.path.join(assets, "CRNN_softmax"), precision="bf16x3")
    try:
        assert create([soft.handle, engines["CRNN_nosilence"].handle]) == _lib.WW_OK
        refused(create([soft.handle, engines["Wavenet"].handle]), "kind")
        refused(create([extra["CRNN"].handle, soft.handle]), "info")          # n_out 1 / 2
        refused(create([extra["CRNN_old"].handle, soft.handle]), "generic")   # another conv geometry
        refused(create([soft.handle, bf16.handle]), "bf16")
        refused(create([soft.handle], n=0), "members")
        refused(create([soft.handle] * 65), "members")
        refused(create([soft.handle, None]), "NULL")
    finally:
        for e in list(extra.values()) + [bf16]:
            e.close()

    # ---- win_model out of range: nothing is launched
    K = crnn_set.n_models
    d_mel = torch.from_numpy(wins.reshape(-1, 40)).cuda()
    d_row = torch.arange(3, dtype=torch.int64, device="cuda") * crnn_set.window
    d_valid = torch.full((3,), crnn_set.window, dtype=torch.int32, device="cuda")
    out = torch.full((3, crnn_set.n_out), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()

    def windows(ids, n=3):
        a = np.asarray(ids, np.int32)
        rc = lib.ww_set_forward_windows_dev(ctx.handle, crnn_set.handle, C.c_void_p(d_mel.data_ptr()), 3 * crnn_set.window,
                                            C.c_void_p(d_row.data_ptr()), C.c_void_p(d_valid.data_ptr()), _lib.ptr(a), n,
                                            C.c_void_p(out.data_ptr()), None)
        ctx.synchronize()
        return rc

    for bad in ([0, -1, 1], [0, 1, K]):
        refused(windows(bad), "win_model")
        assert (out.cpu().numpy() == -7.0).all()
    assert windows([0, 1, 2], n=0) == _lib.WW_OK and (out.cpu().numpy() == -7.0).all()
    refused(windows([0, 1, 2], n=-1))
    assert windows([2, 0, 1]) == _lib.WW_OK
    np.testing.assert_array_equal(out.cpu().numpy(), base)

    # ---- banks
    fp = frontend_params()

    def create_bank(models, flags=0):
        a = None if models is None else np.asarray(models, np.int32)
        h = C.c_void_p()
        rc = lib.ww_stream_create_set(ctx.handle, crnn_set.handle, 2, _lib.ptr(a), C.byref(fp), flags, C.byref(h))
        if rc == _lib.WW_OK:
            lib.ww_stream_destroy(h)
        return rc

    assert create_bank(None) == _lib.WW_OK and create_bank([K - 1, 0]) == _lib.WW_OK
    refused(create_bank([0, K]), "stream_model")
    refused(create_bank([-1, 0]), "stream_model")
    refused(create_bank([0, 0], _lib.STREAM_FULL_RECOMPUTE), "FULL_RECOMPUTE")
    plain = StreamBank(soft, 2)
    mixed = StreamBank(crnn_set, 2, models=[0, 1])
    try:
        one = np.asarray([0], np.int32)
        refused(lib.ww_stream_set_model(plain._h, _lib.ptr(one), 1, 0), "set")
        refused(lib.ww_stream_set_model(mixed._h, _lib.ptr(one), 1, K), "model")
        refused(lib.ww_stream_set_model(mixed._h, _lib.ptr(np.asarray([2], np.int32)), 1, 0), "id")
        assert lib.ww_stream_set_model(mixed._h, _lib.ptr(one), 1, 2) == _lib.WW_OK
        assert lib.ww_stream_set_model(mixed._h, None, 0, 1) == _lib.WW_OK
    finally:
        plain.close()
        mixed.close()

    # ---- the common info; a member freed after set creation leaves the set working
    info, n = _lib.ModelInfo(), C.c_int32(0)
    assert lib.ww_model_set_info(crnn_set.handle, C.byref(info), C.byref(n)) == _lib.WW_OK
    assert (n.value, info.kind, info.window, info.n_mel, info.n_bins, info.n_out, info.enc_rows, info.enc_width) == \
        (3, _lib.KIND_CRNN, 151, 40, 257, 2, 1, 64)
    own = [Engine(os.path.join(assets, m)) for m in CRNNS]
    ms = ModelSet(own)
    for e in own:
        e.close()
    try:
        np.testing.assert_array_equal(ms.forward(wins, [2, 0, 1]), base)
    finally:
        ms.close()
