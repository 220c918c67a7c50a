"""The Wavenet's sequence form over a model set (``ww_set_wave_sequence*``, ``ModelSet.sequence_forward[_all]``).

The yardstick is the library's own single-model path: every output of sequence ``s`` in plane ``k`` equals, BIT FOR BIT
(``np.testing.assert_array_equal``), what ``Engine(member).sequence_forward`` returns for that sequence - wherever the cuts fall
and whatever the neighbouring sequences, the other slots and the size of the call are.  (That path is held against float64 by
tests/test_gpu_wave_sequence.py.)  Rows outside every sequence are neither read - they hold NaN here - nor written, in every plane.

The set is ``ModelSet([Wavenet, Wavenet_alt])`` from the shipped files; the sequences are seeded random mel in [0, 6] of 1, 16, 181,
182, 200 and 450 rows and one empty sequence: 181 and 182 straddle the receptive field and the window, 450 rows at
``wave_seq_segment=256`` are two segments, the second with a 180-row warm-up."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

WAVES = ["Wavenet", "Wavenet_alt"]
CRNNS = ["CRNN_nosilence", "CRNN_nosilence_enhanced"]
LENGTHS = [1, 16, 0, 181, 182, 200, 450]
ROUTE = [0, 1, 1, 0, 1, 0, 0]
ALL = ("enc", "logits", "post_frames", "post")
POOLS = (None, 0, 50)
EMPTY = LENGTHS.index(0)


@pytest.fixture(scope="module")
def engines(assets):
    from wwhip.engine import Engine
    out = {m: Engine(os.path.join(assets, m)) for m in WAVES + CRNNS}
    yield out
    for e in out.values():
        e.close()


@pytest.fixture(scope="module")
def wave_set(engines):
    from wwhip.engine import ModelSet
    ms = ModelSet([engines[m] for m in WAVES])
    yield ms
    ms.close()


@pytest.fixture(scope="module")
def seqs():
    rng = np.random.default_rng(20261020)
    return [rng.uniform(0.0, 6.0, (n, 40)).astype(np.float32) for n in LENGTHS]


@pytest.fixture(scope="module")
def refs(engines, seqs):
    """[member][pool] -> what the member's engine returns on the list: computed once, never written to."""
    out = [{p: engines[m].sequence_forward(seqs, pool=p, want=ALL) for p in POOLS} for m in WAVES]
    for per_pool in out:
        for got in per_pool.values():
            for k in ALL:
                for a in got[k]:
                    a.setflags(write=False)
    return out


def _same_list(got, want, what):
    """One plane (``{name: [per sequence]}``) against a reference of the same shape."""
    for k in ALL:
        assert len(got[k]) == len(want[k]) == len(LENGTHS)
        for i in range(len(LENGTHS)):
            assert got[k][i].shape == want[k][i].shape, (what, k, i)
            np.testing.assert_array_equal(got[k][i], want[k][i], err_msg=f"{what}: {k} of sequence {i} ({LENGTHS[i]} rows)")


# ------------------------------------------------------------------------------------------------------------- 1. all members
@pytest.mark.parametrize("pool", POOLS)
@pytest.mark.parametrize("slots", [None, [1, 0, 1], [0]])
def test_every_slot_equals_its_member_alone(wave_set, seqs, refs, slots, pool):
    got = wave_set.sequence_forward_all(seqs, members=slots, pool=pool, want=ALL)
    members = list(range(len(WAVES))) if slots is None else slots
    for name in ALL:
        assert len(got[name]) == len(members)
    for k, m in enumerate(members):
        _same_list({name: got[name][k] for name in ALL}, refs[m][pool], f"slot {k} = member {m}, pool {pool}")
        assert np.isnan(got["post"][k][EMPTY]).all()                       # an empty sequence has no posterior
        assert all(np.isfinite(got["post"][k][i]).all() for i in range(len(LENGTHS)) if i != EMPTY)
    # ``want`` decides what comes back, the bits do not depend on it
    post_only = wave_set.sequence_forward_all(seqs, members=slots, pool=pool)
    assert list(post_only) == ["post"]
    for k in range(len(members)):
        for i in range(len(LENGTHS)):
            np.testing.assert_array_equal(post_only["post"][k][i], got["post"][k][i])


# ------------------------------------------------------------------------------------------------------------------ 2. routing
def test_each_sequence_by_its_own_member(wave_set, engines, seqs, refs):
    """``model_ids = [0, 1, 1, 0, 1, 0, 0]``: each sequence's outputs equal that member alone on that sequence ALONE - and,
    therefore, the member's row of the whole list."""
    for pool in POOLS:
        got = wave_set.sequence_forward(seqs, ROUTE, pool=pool, want=ALL)
        for i, m in enumerate(ROUTE):
            for k in ALL:
                np.testing.assert_array_equal(got[k][i], refs[m][pool][k][i], err_msg=f"pool {pool}: {k} of sequence {i} by member {m}")
    got = wave_set.sequence_forward(seqs, ROUTE, want=ALL)
    for i, m in enumerate(ROUTE):
        alone = engines[WAVES[m]].sequence_forward([seqs[i]], want=ALL)
        for k in ALL:
            np.testing.assert_array_equal(got[k][i], alone[k][0], err_msg=f"{k} of sequence {i} against member {m} on it alone")
    assert np.isnan(got["post"][EMPTY]).all()
    # a routed call of one member is that member's slot
    for m in range(len(WAVES)):
        _same_list(wave_set.sequence_forward(seqs, [m] * len(seqs), want=ALL), refs[m][None], f"every sequence by member {m}")


# --------------------------------------------------------------------------------------------------------------------- 3. cuts
def test_the_cuts_do_not_show(wave_set, seqs, refs):
    """``wave_seq_segment`` at 256 (450 rows: two segments), above every length and at 0: identical outputs in both forms."""
    try:
        for seg in (256, 1 << 20, 0):
            wave_set.set_option("wave_seq_segment", seg)
            every = wave_set.sequence_forward_all(seqs, members=[1, 0, 1], want=ALL)
            for k, m in enumerate([1, 0, 1]):
                _same_list({name: every[name][k] for name in ALL}, refs[m][None], f"segment {seg}, slot {k}")
            routed = wave_set.sequence_forward(seqs, ROUTE, pool=50, want=ALL)
            for i, m in enumerate(ROUTE):
                for k in ALL:
                    np.testing.assert_array_equal(routed[k][i], refs[m][50][k][i], err_msg=f"segment {seg}: {k} of sequence {i}")
    finally:
        wave_set.set_option("wave_seq_segment", 0)


# ------------------------------------------------------------------------------------------------------- 4. untouched bytes
FRONT, GAP, BEHIND = 5, 11, 9
FIRST = 4   # sequences [0, FIRST) lie in front of the gap, the others behind it


def _layout(seqs):
    """The sequences in one buffer with rows of NaN in front of, between and behind them.  Offsets are consecutive, so one call
    cannot leave rows between ITS sequences: the two groups are two calls over the same buffers, and each call's rows outside its
    own group - the gap and the other group among them - must stay as they are."""
    parts, at, offs = [np.full((FRONT, 40), np.nan, np.float32)], FRONT, [[], []]
    for g, group in enumerate((seqs[:FIRST], seqs[FIRST:])):
        offs[g].append(at)
        for s in group:
            parts.append(s)
            at += len(s)
            offs[g].append(at)
        parts.append(np.full((GAP if g == 0 else BEHIND, 40), np.nan, np.float32))
        at += GAP if g == 0 else BEHIND
    return np.concatenate(parts), [np.asarray(o, np.int64) for o in offs]


class _DevOut:
    """The four outputs of a device call as tensors full of -7; ``planes=None``: the by-sequence form's one plane."""

    def __init__(self, planes, total, n_seq, n_out, skip=()):
        import torch
        lead = () if planes is None else (planes,)
        shape = {"enc": (total, 32), "logits": (total, n_out), "post_frames": (total, n_out), "post": (n_seq, n_out)}
        self.t = {k: torch.full(lead + shape[k], -7.0, dtype=torch.float32, device="cuda") for k in ALL}
        self.skip = set(skip)
        torch.cuda.synchronize()

    def ptr(self, k):
        return 0 if k in self.skip else self.t[k].data_ptr()

    def host(self):
        return {k: v.cpu().numpy() for k, v in self.t.items()}


def _run_all(ms, d_mel, total, offs, slots, pool, out):
    ms.wave_sequence_all_dev(d_mel.data_ptr(), total, offs, slots, pool, out.ptr("enc"), out.ptr("logits"), out.ptr("post_frames"), out.ptr("post"))
    ms.ctx.synchronize()
    return out.host()


def _run_routed(ms, d_mel, total, offs, ids, pool, out):
    ms.wave_sequence_dev(d_mel.data_ptr(), total, offs, ids, pool, out.ptr("enc"), out.ptr("logits"), out.ptr("post_frames"), out.ptr("post"))
    ms.ctx.synchronize()
    return out.host()


def _check_plane(got, plane, offs, seq0, member_ref, written, what):
    """Rows [offs[i], offs[i + 1]) of the plane are sequence seq0 + i of the reference; ``written`` collects them."""
    for i in range(len(offs) - 1):
        a, b = int(offs[i]), int(offs[i + 1])
        for k in ("enc", "logits", "post_frames"):
            np.testing.assert_array_equal(got[k][plane][a:b], member_ref[k][seq0 + i], err_msg=f"{what}: {k} of sequence {seq0 + i}")
            written[k][plane][a:b] = True
        if b > a:
            np.testing.assert_array_equal(got["post"][plane][i], member_ref["post"][seq0 + i], err_msg=f"{what}: post of sequence {seq0 + i}")
            written["post"][plane][i] = True


def test_rows_outside_the_sequences_are_neither_read_nor_written(wave_set, seqs, refs):
    import torch
    mel, (offs_a, offs_b) = _layout(seqs)
    total, n_out = len(mel), wave_set.n_out
    d_mel = torch.from_numpy(mel).cuda()
    slots, pool = [1, 0, 1], 50
    # every sequence by every slot: group A, then group B over the same buffers (post has a row per sequence of ITS call: B's
    # rows go to a buffer of their own)
    out_a = _DevOut(len(slots), total, len(offs_a) - 1, n_out)
    got = _run_all(wave_set, d_mel, total, offs_a, slots, pool, out_a)
    written = {k: np.zeros(v.shape, bool) for k, v in got.items()}
    for k, m in enumerate(slots):
        _check_plane(got, k, offs_a, 0, refs[m][pool], written, f"group A, slot {k}")
    for k in ALL:
        assert (got[k][~written[k]] == -7.0).all(), k          # front, gap, group B's rows, behind; the empty sequence's post row
    assert not written["post"][:, EMPTY].any() and written["post"].sum() == len(slots) * (FIRST - 1) * n_out
    out_b = _DevOut(len(slots), total, len(offs_b) - 1, n_out)
    for k in ("enc", "logits", "post_frames"):
        out_b.t[k] = out_a.t[k]
    got_b = _run_all(wave_set, d_mel, total, offs_b, slots, pool, out_b)
    post_b = np.zeros(got_b["post"].shape, bool)
    written_b = dict(written, post=post_b)
    for k, m in enumerate(slots):
        _check_plane(got_b, k, offs_b, FIRST, refs[m][pool], written_b, f"group B, slot {k}")
        _check_plane(dict(got_b, post=got["post"]), k, offs_a, 0, refs[m][pool], written, f"group A after B, slot {k}")  # A's rows: as they were
    for k in ("enc", "logits", "post_frames"):
        assert (got_b[k][~written[k]] == -7.0).all() and (~written[k]).sum() == len(slots) * (FRONT + GAP + BEHIND) * got_b[k].shape[-1], k
    assert post_b.all()
    # a pointer left out: that buffer is not written, the others carry the same bits
    for skip in (("enc",), ("logits",), ("logits", "post"), ("enc", "logits", "post_frames")):
        part = _run_all(wave_set, d_mel, total, offs_a, slots, pool, _DevOut(len(slots), total, len(offs_a) - 1, n_out, skip))
        for k in ALL:
            if k in skip:
                assert (part[k] == -7.0).all(), (skip, k)
            else:
                np.testing.assert_array_equal(part[k], got[k], err_msg=f"{k} without {skip}")
    # the by-sequence form: one plane, each sequence by its member
    mel_c = np.concatenate([mel[:FRONT]] + seqs + [mel[-BEHIND:]])  # (all seven sequences as one call: no gap)
    offs_c = FRONT + np.concatenate([[0], np.cumsum(LENGTHS)]).astype(np.int64)
    d_mel_c = torch.from_numpy(mel_c).cuda()
    routed = _run_routed(wave_set, d_mel_c, len(mel_c), offs_c, ROUTE, None, _DevOut(None, len(mel_c), len(LENGTHS), n_out))
    for i, m in enumerate(ROUTE):
        a, b = int(offs_c[i]), int(offs_c[i + 1])
        for k in ("enc", "logits", "post_frames"):
            np.testing.assert_array_equal(routed[k][a:b], refs[m][None][k][i], err_msg=f"routed {k} of sequence {i}")
        if i != EMPTY:
            np.testing.assert_array_equal(routed["post"][i], refs[m][None]["post"][i])
    assert (routed["post"][EMPTY] == -7.0).all()
    for k in ("enc", "logits", "post_frames"):
        assert (routed[k][:FRONT] == -7.0).all() and (routed[k][-BEHIND:] == -7.0).all(), k
    part = _run_routed(wave_set, d_mel_c, len(mel_c), offs_c, ROUTE, None, _DevOut(None, len(mel_c), len(LENGTHS), n_out, ("logits", "enc")))
    assert (part["enc"] == -7.0).all() and (part["logits"] == -7.0).all()
    np.testing.assert_array_equal(part["post_frames"], routed["post_frames"])
    np.testing.assert_array_equal(part["post"], routed["post"])


def test_more_slots_than_one_launch_takes(wave_set, seqs, refs):
    """1,025 slots (duplicates; the model kernel takes 1,024 planes per launch): the last slot, alone in the second launch, and
    slots on both sides of the cut carry their member's bits."""
    slots = [k % 2 for k in range(1024)] + [1]
    got = wave_set.sequence_forward_all(seqs, members=slots, pool=50, want=("logits", "post_frames", "post"))
    for k in (0, 1, 511, 1022, 1023, 1024):
        for name in ("logits", "post_frames", "post"):
            for i in range(len(LENGTHS)):
                np.testing.assert_array_equal(got[name][k][i], refs[slots[k]][50][name][i], err_msg=f"slot {k}: {name} of sequence {i}")


# ------------------------------------------------------------------------------------- 5. refusals and degenerate sizes (ctypes)
def test_refusals_and_no_ops(wave_set, engines, seqs, refs):
    """Every WW_EINVAL of the four entry points carries a ``ww_last_error`` text and leaves the outputs all -7; the named no-ops are
    WW_OK and write nothing; a valid call afterwards has the bits of the first test."""
    import torch
    from wwhip import _lib
    from wwhip.engine import ModelSet
    lib = _lib.load()
    ctx, K, n_out = wave_set.ctx, wave_set.n_models, wave_set.n_out
    mel = np.concatenate(seqs)
    offs = np.concatenate([[0], np.cumsum(LENGTHS)]).astype(np.int64)
    total, n_seq = len(mel), len(LENGTHS)
    d_mel = torch.from_numpy(mel).cuda()
    slots = [1, 0, 1]
    out = _DevOut(len(slots), total, n_seq, n_out)
    other = _lib.Context(ctx.device)
    crnn_set = ModelSet([engines[m] for m in CRNNS])
    OMIT = object()
    vp = lambda t: C.c_void_p(t.data_ptr())

    def outs(o):
        return [None] * 4 if o is None else [vp(out.t[k]) for k in ALL]

    def call_all(c=ctx.handle, s=OMIT, m=OMIT, rows=total, ro=offs, n=n_seq, pool=50, members=slots, n_members=None, o=OMIT):
        ids = None if members is None else np.asarray(members, np.int32)
        rc = lib.ww_set_wave_sequence_all_dev(c, wave_set.handle if s is OMIT else s, vp(d_mel) if m is OMIT else m, rows,
                                              _lib.ptr(None if ro is None else np.ascontiguousarray(ro, np.int64)), n, pool, _lib.ptr(ids),
                                              (0 if ids is None else ids.size) if n_members is None else n_members, *outs(o))
        ctx.synchronize()
        return rc, c

    def call_routed(c=ctx.handle, s=OMIT, m=OMIT, rows=total, ro=offs, n=n_seq, pool=50, ids=ROUTE, o=OMIT):
        ids = None if ids is None else np.asarray(ids, np.int32)
        rc = lib.ww_set_wave_sequence_dev(c, wave_set.handle if s is OMIT else s, vp(d_mel) if m is OMIT else m, rows,
                                          _lib.ptr(None if ro is None else np.ascontiguousarray(ro, np.int64)), n, _lib.ptr(ids), pool, *outs(o))
        ctx.synchronize()
        return rc, c

    def untouched():
        return all((v == -7.0).all() for v in out.host().values())

    def refused(res, word):
        rc, c = res
        text = lib.ww_last_error(c).decode()
        assert rc == _lib.WW_EINVAL, (rc, word, text)
        assert len(text) > 8 and word in text, (word, text)
        assert untouched(), word

    down = offs.copy()
    down[4] = down[3] - 1
    try:
        for call in (call_all, call_routed):
            refused(call(c=None), "NULL")
            refused(call(s=None), "NULL")
            refused(call(m=None), "NULL mel")
            refused(call(c=other.handle), "another context")
            refused(call(s=crnn_set.handle), "no causal reading")
            refused(call(n=-1), "sequence count")
            refused(call(pool=-1), "pool")
            refused(call(ro=down), "descend at sequence 3")
            refused(call(rows=total - 1), "leave the mel buffer")
            refused(call(ro=offs - 1), "leave the mel buffer")
            refused(call(ro=None), "row_offs is NULL")
        refused(call_all(members=[0], n_members=-1), "member count")
        refused(call_all(members=[0, K]), f"members[1] = {K}")
        refused(call_all(members=[-1, 0]), "members[0] = -1")
        refused(call_routed(ids=[0, 1, 1, 0, K, 0, 0]), f"seq_model[4] = {K}")
        refused(call_routed(ids=[0, 1, 1, 0, 1, 0, -2]), "seq_model[6] = -2")
        empty = np.full(n_seq + 1, 7, np.int64)
        for ok in (call_all(n=0), call_all(ro=None, n=0), call_all(ro=empty), call_all(members=[0], n_members=0), call_all(o=None),
                   call_all(m=None, ro=empty), call_routed(n=0), call_routed(ro=empty), call_routed(o=None), call_routed(ids=None, o=None)):
            assert ok[0] == _lib.WW_OK, lib.ww_last_error(ctx.handle)
            assert untouched()
        # the host forms: the same checks before a byte moves
        host = {k: np.full(tuple(out.t[k].shape), -7.0, np.float32) for k in ALL}
        hp = [_lib.ptr(host[k]) for k in ALL]
        ids3, bad3, route, bad_route = (np.asarray(a, np.int32) for a in (slots, [0, K, 1], ROUTE, [0, 1, 1, 0, 1, 0, K]))
        for rc in (lib.ww_set_wave_sequence_all(ctx.handle, wave_set.handle, None, total, _lib.ptr(offs), n_seq, 50, _lib.ptr(ids3), 3, *hp),
                   lib.ww_set_wave_sequence_all(ctx.handle, wave_set.handle, _lib.ptr(mel), total, _lib.ptr(offs), n_seq, 50, _lib.ptr(bad3), 3, *hp),
                   lib.ww_set_wave_sequence_all(ctx.handle, crnn_set.handle, _lib.ptr(mel), total, _lib.ptr(offs), n_seq, 50, _lib.ptr(ids3), 3, *hp),
                   lib.ww_set_wave_sequence(ctx.handle, wave_set.handle, _lib.ptr(mel), total, _lib.ptr(offs), n_seq, _lib.ptr(bad_route), 50, *hp),
                   lib.ww_set_wave_sequence(ctx.handle, wave_set.handle, _lib.ptr(mel), total, _lib.ptr(down), n_seq, _lib.ptr(route), 50, *hp)):
            assert rc == _lib.WW_EINVAL and len(lib.ww_last_error(ctx.handle)) > 8
            assert all((v == -7.0).all() for v in host.values())
        assert lib.ww_set_wave_sequence_all(ctx.handle, wave_set.handle, _lib.ptr(mel), total, _lib.ptr(offs), n_seq, 50, _lib.ptr(ids3), 0, *hp) == _lib.WW_OK
        assert lib.ww_set_wave_sequence(ctx.handle, wave_set.handle, _lib.ptr(mel), total, _lib.ptr(offs), 0, None, 50, *hp) == _lib.WW_OK
        assert all((v == -7.0).all() for v in host.values())
        # the option
        assert lib.ww_set_option(wave_set.handle, _lib.OPT_WAVE_SEQ_SEGMENT, -1) == _lib.WW_EINVAL
        assert lib.ww_set_option(wave_set.handle, _lib.OPT_WAVE_SEQ_SEGMENT, 1 << 31) == _lib.WW_EINVAL
        assert lib.ww_set_option(wave_set.handle, _lib.OPT_CRNN_SPLIT_AT, 0) == _lib.WW_EINVAL
        assert lib.ww_set_option(wave_set.handle, _lib.OPT_WAVENET_ROWMAJOR, 1) == _lib.WW_EINVAL
        # a valid call after all of it: the bits of the first test, and NULL seq_model is member 0
        assert call_all()[0] == _lib.WW_OK, lib.ww_last_error(ctx.handle)
        got = out.host()
        for k, m in enumerate(slots):
            _check_plane(got, k, offs, 0, refs[m][50], {name: np.zeros(v.shape, bool) for name, v in got.items()}, f"after the refusals, slot {k}")
        assert (got["post"][:, EMPTY] == -7.0).all()
        one = _DevOut(None, total, n_seq, n_out)
        rc = lib.ww_set_wave_sequence_dev(ctx.handle, wave_set.handle, vp(d_mel), total, _lib.ptr(offs), n_seq, None, 50, *[vp(one.t[k]) for k in ALL])
        ctx.synchronize()
        assert rc == _lib.WW_OK, lib.ww_last_error(ctx.handle)
        got0 = {k: v[None] for k, v in one.host().items()}
        _check_plane(got0, 0, offs, 0, refs[0][50], {name: np.zeros(v.shape, bool) for name, v in got0.items()}, "NULL seq_model")
    finally:
        crnn_set.close()
        other.close()
