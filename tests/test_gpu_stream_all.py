"""Stream banks that run EVERY listed member of a model set on EVERY stream (``ww_stream_create_set_all``,
``StreamBank(model_set, S, members=...)``).

The yardstick everywhere: K ordinary banks, each built on the single ``Engine`` of one member, given the same frames, the same flags
and the same resets.  ``post[:, j, :]`` of the every-member bank equals bank j's ``post`` BIT FOR BIT (``np.array_equal``), ``n_post``
equals every bank's, ``window(s)`` equals bank 0's.  The references are computed once per script and shared by the forms.

Members: ``CRNN_nosilence``, ``CRNN_nosilence_enhanced``, ``CRNN_softmax`` (tests/test_gpu_model_set.py) and ``Wavenet``,
``Wavenet_alt`` (tests/test_gpu_set_sequence.py), the shipped files as they are."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CRNNS = ["CRNN_nosilence", "CRNN_nosilence_enhanced", "CRNN_softmax"]
WAVES = ["Wavenet", "Wavenet_alt"]
FORMS = {"one_launch": {}, "one_launch_sync": {"sync_wait": True}, "two_launch": {"two_launch": True},
         "two_launch_sync": {"two_launch": True, "sync_wait": True}}


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


def _script(S, ticks, seed, reset_every=(40, 61), samples=320):
    """Frames, per-stream flags (bit 0 about 80 %, bit 1 about 10 %) and resets of random streams every 40 to 60 ticks."""
    rng = np.random.default_rng(seed)
    frames = np.clip(rng.normal(0, 2500, (ticks, S, samples)), -32768, 32767).astype(np.int16)
    speech = (rng.random((ticks, S)) < 0.8).astype(np.uint8)
    active = (rng.random((ticks, S)) < 0.1).astype(np.uint8)
    resets, t = {}, int(rng.integers(*reset_every))
    while t < ticks:
        resets[t] = sorted(set(rng.integers(0, S, max(1, S // 3)).tolist()))
        t += int(rng.integers(*reset_every))
    return frames, speech, active, resets


def _run(bank, script, window_every=37):
    """The script through one bank: (post per tick, n_post per tick, the windows read on the way)."""
    frames, speech, active, resets = script
    posts, ns, wins = [], [], []
    for t in range(frames.shape[0]):
        if t in resets:
            bank.reset(resets[t])
        p, n = bank.step(frames[t], speech[t], active[t])
        posts.append(p)
        ns.append(n)
        if t % window_every == window_every - 1 or t == frames.shape[0] - 1:
            wins.append(bank.window(t % bank.S))
    return np.stack(posts), np.stack(ns), np.stack(wins)


def _assert_equals_members(got, refs, members):
    """got: the every-member bank's run; refs[m]: the run of the ordinary bank of member m."""
    post, n, wins = got
    assert post.shape[2:] == (len(members), 2)
    for j, m in enumerate(members):
        rp, rn, _ = refs[m]
        assert np.array_equal(n, rn), f"n_post differs from the bank of member {m}"
        assert np.array_equal(post[:, :, j, :], rp), f"slot {j} (member {m}) differs from that member's own bank"
    assert np.array_equal(wins, refs[members[0]][2])
    assert n.max() == 2 and n.min() == 0 and (post != 0).any()


def _fp(precise):
    from wwhip.engine import frontend_params
    return frontend_params(precise=precise)


S1, TICKS1 = 5, 330


@pytest.fixture(scope="module")
def crnn_refs(engines):
    """Per front-end precision: the script, and the three members' ordinary banks run over it - computed once, left unchanged."""
    from wwhip.engine import StreamBank
    out = {}
    for precise in (True, False):
        script = _script(S1, TICKS1, 11 + precise)
        refs = {}
        for m, name in enumerate(CRNNS):
            bank = StreamBank(engines[name], S1, _fp(precise))
            refs[m] = _run(bank, script)
            bank.close()
        out[precise] = (script, refs)
    return out


@pytest.mark.parametrize("precise", [True, False], ids=["fe_fp64", "fe_fp32"])
@pytest.mark.parametrize("form", list(FORMS))
def test_crnn_every_member_equals_the_members_own_banks(crnn_set, crnn_refs, form, precise):
    """S = 5, members [0, 1, 2], 330 ticks (the mel ring of 152 slots and the cache ring of 144 wrap more than twice), random flags,
    resets every 40 to 60 ticks; one launch and two, polled and waited for, fp64 and fp32 transform (crnn_stream_kernel<2, true, true>
    and <1, true, true>)."""
    from wwhip.engine import StreamBank
    script, refs = crnn_refs[precise]
    bank = StreamBank(crnn_set, S1, _fp(precise), members=[0, 1, 2], **FORMS[form])
    try:
        assert bank.n_members == 3 and bank.members.tolist() == [0, 1, 2]
        _assert_equals_members(_run(bank, script), refs, [0, 1, 2])
    finally:
        bank.close()


def test_repeated_members_and_one_slot(crnn_set, crnn_refs):
    """Members [2, 0, 2]: slots 0 and 2 carry the same bits (member 2's).  K = 1, "all" and the default order: an every-member bank of
    one slot yields the bits of the ordinary set bank of that member."""
    from wwhip.engine import StreamBank
    script, refs = crnn_refs[True]
    bank = StreamBank(crnn_set, S1, members=[2, 0, 2])
    try:
        got = _run(bank, script)
        _assert_equals_members(got, refs, [2, 0, 2])
        assert np.array_equal(got[0][:, :, 0, :], got[0][:, :, 2, :])
    finally:
        bank.close()
    one = StreamBank(crnn_set, S1, members=[1])
    ordinary = StreamBank(crnn_set, S1, models=[1] * S1)
    try:
        got, want = _run(one, script), _run(ordinary, script)
        assert got[0].shape == (TICKS1, S1, 1, 2)
        assert np.array_equal(got[0][:, :, 0, :], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
        _assert_equals_members(got, refs, [1])
    finally:
        one.close()
        ordinary.close()
    every = StreamBank(crnn_set, 2, members="all")
    try:
        assert every.members.tolist() == [0, 1, 2] and every.step(np.zeros((2, 320), np.int16), np.ones(2, np.uint8))[0].shape == (2, 3, 2)
    finally:
        every.close()


def test_more_workgroups_than_are_resident(engines, crnn_set):
    """S = 200, K = 3: 1200 workgroups in the one launch, above what two per CU hold at once - a stream's later workgroups start
    after its writer has finished.  40 ticks, mixed flags, one reset."""
    from wwhip.engine import StreamBank
    S, ticks = 200, 40
    script = _script(S, ticks, 5, reset_every=(20, 21))
    refs = {}
    for m, name in enumerate(CRNNS):
        b = StreamBank(engines[name], S)
        refs[m] = _run(b, script, window_every=13)
        b.close()
    bank = StreamBank(crnn_set, S, members="all")
    try:
        assert len(script[3]) == 1
        _assert_equals_members(_run(bank, script, window_every=13), refs, [0, 1, 2])
    finally:
        bank.close()


@pytest.mark.parametrize("causal", [False, True], ids=["window_bank", "causal"])
def test_wavenet_every_member(engines, wave_set, causal):
    """The Wavenet window bank (two launches) and the causal tick: S = 4, K = 2, 200 ticks, mixed flags, one reset - against the
    members' own banks of the same reading (causal against causal)."""
    from wwhip.engine import StreamBank
    S, ticks = 4, 200
    script = _script(S, ticks, 21, reset_every=(90, 91))
    script = script[:3] + ({90: script[3][90]},)
    refs = {}
    for m, name in enumerate(WAVES):
        b = StreamBank(engines[name], S, causal=causal)
        refs[m] = _run(b, script)
        b.close()
    bank = StreamBank(wave_set, S, members="all", causal=causal)
    try:
        _assert_equals_members(_run(bank, script), refs, [0, 1])
    finally:
        bank.close()


def _run_rates(banks, rates, ticks, seed, move=None):
    """The same frames (each stream's at its own rate) through every bank; ``move`` = (tick, ids, rate): one set_rate on the way."""
    rng = np.random.default_rng(seed)
    S = banks[0].S
    rates = list(rates)
    out = [([], [], []) for _ in banks]
    for t in range(ticks):
        if move and t == move[0]:
            for b in banks:
                b.set_rate(move[1], move[2])
            for s in move[1]:
                rates[s] = move[2]
        per = [np.clip(rng.normal(0, 2500, r // 50), -32768, 32767).astype(np.int16) for r in rates]
        speech = (rng.random(S) < 0.8).astype(np.uint8)
        active = (rng.random(S) < 0.1).astype(np.uint8)
        for b, o in zip(banks, out):
            p, n = b.step(per if b._mixed else np.stack(per), speech, active)
            o[0].append(p)
            o[1].append(n)
            if t % 20 == 19:
                o[2].append(b.window(t % S))
    return [tuple(np.stack(x) for x in o) for o in out]


@pytest.mark.parametrize("rates", [48000, [8000, 16000, 48000]], ids=["uniform_48k", "mixed"])
def test_rates(engines, crnn_set, rates):
    """S = 3 at 48 kHz, and at 8 / 16 / 48 kHz with one set_rate on the way: 60 ticks against the three ordinary banks at the same
    rates."""
    from wwhip.engine import StreamBank
    S, ticks = 3, 60
    banks = [StreamBank(crnn_set, S, members="all", sample_rate=rates)] + [StreamBank(engines[m], S, sample_rate=rates) for m in CRNNS]
    try:
        mixed = not isinstance(rates, int)
        runs = _run_rates(banks, rates if mixed else [rates] * S, ticks, 31, move=(30, [0], 48000) if mixed else None)
        if mixed:
            assert banks[0].sample_rates.tolist() == [48000, 16000, 48000]
        _assert_equals_members(runs[0], {m: runs[1 + m] for m in range(3)}, [0, 1, 2])
    finally:
        for b in banks:
            b.close()


def test_contract_through_ctypes(engines, crnn_set, wave_set):
    """Every WW_EINVAL of the new surface carries a ww_last_error text, and after each the bank's next tick equals a twin's that never
    saw the refused call; ww_stream_members on both kinds of bank; S K = 65536 is refused at creation."""
    from wwhip import _lib
    from wwhip.engine import StreamBank, frontend_params
    lib, ctx = _lib.load(), crnn_set.ctx
    S, K = 3, 3
    rng = np.random.default_rng(41)
    ones = np.ones(S, np.uint8)

    def refused(rc, *words):
        text = lib.ww_last_error(ctx.handle).decode()
        assert rc == _lib.WW_EINVAL, (rc, text)
        assert len(text) > 8
        for w in words:
            assert w in text, (w, text)

    def same_next_tick(bank, twin):
        f = np.clip(rng.normal(0, 2500, (S, 320)), -32768, 32767).astype(np.int16)
        (p, n), (tp, tn) = bank.step(f, ones), twin.step(f, ones)
        assert np.array_equal(p, tp) and np.array_equal(n, tn)
        assert np.array_equal(bank.window(1), twin.window(1))

    post = np.full((S, K, 2), -7.0, np.float32)
    n_post = np.full(S, -7, np.int32)
    frames = np.zeros((S, 320), np.int16)
    ids = np.array([0], np.int32)
    offs, row_offs = np.array([0, 320], np.int64), np.zeros(2, np.int64)
    u8 = [np.zeros(S, np.uint8) for _ in range(3)]
    pmax, i32 = np.zeros(S, np.float32), [np.zeros(S, np.int32) for _ in range(2)]
    cnt = [C.c_int32(0), C.c_int32(0)]
    ps = _lib.PipelineState()
    for every_kw, twin_kw, wset in (({"members": "all"}, {"members": "all"}, crnn_set), ({"members": "all", "causal": True},) * 2 + (wave_set,)):
        Kb = 3 if wset is crnn_set else 2
        bank, twin = StreamBank(wset, S, **every_kw), StreamBank(wset, S, **twin_kw)
        try:
            same_next_tick(bank, twin)
            calls = {
                "ww_stream_step": lambda: lib.ww_stream_step(bank._h, _lib.ptr(frames), _lib.ptr(ones), _lib.ptr(post), _lib.ptr(n_post)),
                "ww_stream_step_trigger": lambda: lib.ww_stream_step_trigger(
                    bank._h, _lib.ptr(frames), _lib.ptr(u8[0]), _lib.ptr(u8[1]), 0.5, _lib.ptr(u8[2]), _lib.ptr(pmax), _lib.ptr(post), _lib.ptr(n_post),
                    _lib.ptr(i32[0]), C.byref(cnt[0]), _lib.ptr(i32[1]), C.byref(cnt[1])),
                "ww_pipeline_bank_step": lambda: lib.ww_pipeline_bank_step(bank._h, _lib.ptr(frames), C.byref(ps)),
                "ww_stream_set_model": lambda: lib.ww_stream_set_model(bank._h, None, 0, 1),
                "ww_stream_feed": lambda: lib.ww_stream_feed(bank._h, _lib.ptr(ids), 1, _lib.ptr(frames), _lib.ptr(offs), 8, _lib.ptr(row_offs),
                                                             _lib.ptr(post), None),
                "ww_stream_feed_rows": lambda: lib.ww_stream_feed_rows(bank._h, _lib.ptr(ids), 1, _lib.ptr(offs), _lib.ptr(row_offs)),
            }
            for name, call in calls.items():
                refused(call(), name, "ww_stream_step_all")
                assert (post == -7.0).all() and (n_post == -7).all(), name
                same_next_tick(bank, twin)
            mem, nm = np.full(8, -1, np.int32), C.c_int32(-1)
            assert lib.ww_stream_members(bank._h, _lib.ptr(mem), C.byref(nm)) == _lib.WW_OK
            assert nm.value == Kb and mem[:Kb].tolist() == list(range(Kb)) and (mem[Kb:] == -1).all()
            nm = C.c_int32(-1)
            assert lib.ww_stream_members(bank._h, None, C.byref(nm)) == _lib.WW_OK and nm.value == Kb
            refused(lib.ww_stream_members(bank._h, _lib.ptr(mem), None), "NULL")
        finally:
            bank.close()
            twin.close()
    # an ordinary bank (of an Engine and of the set): ww_stream_step_all is refused, ww_stream_members says 0
    for eng, kw in ((engines[CRNNS[0]], {}), (crnn_set, {"models": [0, 1, 2]})):
        bank, twin = StreamBank(eng, S, **kw), StreamBank(eng, S, **kw)
        try:
            same_next_tick(bank, twin)
            refused(lib.ww_stream_step_all(bank._h, _lib.ptr(frames), _lib.ptr(ones), _lib.ptr(post), _lib.ptr(n_post)), "ww_stream_step_all",
                    "ww_stream_create_set_all")
            assert (post == -7.0).all() and (n_post == -7).all()
            same_next_tick(bank, twin)
            mem, nm = np.full(4, -1, np.int32), C.c_int32(-1)
            assert lib.ww_stream_members(bank._h, _lib.ptr(mem), C.byref(nm)) == _lib.WW_OK and nm.value == 0 and (mem == -1).all()
        finally:
            bank.close()
            twin.close()
    # ---- creation
    fp = frontend_params()

    def create(S_, members, flags=0, wset=crnn_set, n=None):
        h = C.c_void_p()
        a = None if members is None else np.asarray(members, np.int32)
        rc = lib.ww_stream_create_set_all(ctx.handle, wset.handle, S_, _lib.ptr(a), (0 if a is None else a.size) if n is None else n, C.byref(fp),
                                          flags, C.byref(h))
        if rc == _lib.WW_OK:
            assert lib.ww_stream_destroy(h) == _lib.WW_OK
        else:
            assert not h.value
        return rc
    refused(create(16384, [0, 1, 2, 0]), "65536")
    refused(create(65535, [0, 1]), "131070")
    refused(create(2, [0] * 65), "65 member slots")
    refused(create(2, [0], n=0), "0 member slots")
    refused(create(2, [0, 3]), "members[1] = 3", "0..2")
    refused(create(2, [-1]), "members[0] = -1")
    refused(create(0, [0]), "stream count")
    refused(create(2, [0], _lib.STREAM_FULL_RECOMPUTE), "WW_STREAM_FULL_RECOMPUTE")
    refused(create(2, [0], 64), "0x40")
    refused(create(2, [0], _lib.STREAM_CAUSAL), "WW_STREAM_CAUSAL")  # a CRNN set has no causal form
    assert create(2, None) == _lib.WW_OK and create(2, [2, 2], _lib.STREAM_TWO_LAUNCH | _lib.STREAM_SYNC_WAIT) == _lib.WW_OK
    assert create(2, [1, 0], _lib.STREAM_CAUSAL, wave_set) == _lib.WW_OK
