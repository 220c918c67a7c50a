"""CTC-trained CRNNs on the host: the bundle and its blob, what the loader's host half (csrc/model_pack.h, under Address + UB
sanitizer through tests/test_host_logic.py's ``pack_check`` program) takes and refuses, the numpy decode on hand-written cases, the
wake-word rule, the conditions the GPU test's float64 comparison rests on, and the evaluator's ratios."""
import dataclasses
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctc64  # noqa: E402
import geometry64 as G  # noqa: E402
from test_host_logic import PACK_MODELS, WW_EBLOB, _geom_words, _no_f64_digest, pack_blobs, pack_check, pack_golden  # noqa: E402,F401

from wwhip import ctc  # noqa: E402
from wwhip import weights as W  # noqa: E402


def _patch_meta(blob: bytes, section: str, word: int, value: int) -> bytes:
    b = bytearray(blob)
    n = struct.unpack_from("<I", b, 12)[0]
    for i in range(n):
        e = 16 + 32 * i
        if bytes(b[e:e + 24]).rstrip(b"\0") == section.encode():
            off = struct.unpack_from("<I", b, e + 24)[0]
            struct.pack_into("<i", b, off + 4 * word, value)
            return bytes(b)
    raise AssertionError(section)


# ---- (a) bundle, blob ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", ctc64.LS)
def test_bundle_round_trip(L):
    b = ctc64.model(L)
    c = b.crnn
    assert c.head_kind == W.HEAD_CTC == 2 and c.head_w1 is None and c.head_b1 is None and c.n_out == b.n_out == L
    assert c.head_w2.shape == (L, 64) and c.head_b2.shape == (L,)
    u = W.unpack_blob(W.pack_blob(b))
    assert "crnn.head_w1" not in u and "crnn.head_b1" not in u
    assert u["crnn.meta"][13] == 2 and u["crnn.meta"][12] == L
    np.testing.assert_array_equal(u["crnn.head_w2"].reshape(L, 64), c.head_w2)
    np.testing.assert_array_equal(u["crnn.head_b2"], c.head_b2)
    np.testing.assert_array_equal(u["crnn.g2b.wh"].reshape(96, 32), c.gru2[1].w_h)
    with pytest.raises(ValueError, match="CTC"):
        b.posterior_index
    q = W.quantize_fp16(b)   # (does not trip over the missing first layer)
    assert q.crnn.head_w1 is None and q.crnn.head_kind == 2
    np.testing.assert_array_equal(q.crnn.head_w2, c.head_w2.astype(np.float16).astype(np.float32))


def test_ctc_params_refuses_a_misshapen_head():
    base = ctc64.model(4).crnn
    for w, b in ((np.zeros((4, 63)), np.zeros(4)), (np.zeros((4, 64)), np.zeros(5)), (np.zeros(64), np.zeros(1))):
        with pytest.raises(ValueError):
            W.crnn_ctc_params(base, w, b)


@pytest.mark.parametrize("name", PACK_MODELS)
def test_shipped_blobs_pack_as_before(pack_check, pack_blobs, pack_golden, name):  # noqa: F811
    """Heads 0 and 1 are untouched: every array the loader packs for a shipped model has the recorded size and digest."""
    (status, msg, arrays, _), = pack_check(pack_blobs[name])
    assert status == 0, msg
    assert _no_f64_digest(arrays) == pack_golden[name]
    assert "crnn.head_w1" in W.unpack_blob(pack_blobs[name]) or "CRNN" not in name


# ---- (b) the loader --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", ctc64.LS)
def test_loader_takes_a_ctc_head(pack_check, L):  # noqa: F811
    (status, msg, arrays, other), = pack_check(W.pack_blob(ctc64.model(L)))
    assert status == 0 and arrays, msg
    geom = _geom_words(other, "crnn")
    assert int(geom["HEAD"]) == 2 and int(geom["NOUT"]) == L
    sizes = {n: b for n, _, b, _ in arrays}
    # a zero-filled first layer of the usual size: no kernel argument of any form is a null pointer
    assert sizes["crnn.w1"] == 64 * 64 * 4 and sizes["crnn.b1"] == 64 * 4 and sizes["crnn.w2"] == L * 64 * 4
    zeros_w1 = next(h for n, _, _, h in arrays if n == "crnn.w1")
    (_, _, arrays8, _), = pack_check(W.pack_blob(ctc64.model(8 if L != 8 else 4)))
    assert zeros_w1 == next(h for n, _, _, h in arrays8 if n == "crnn.w1")   # (the same bytes whatever the model: zeros)


def _refused_blobs():
    std4 = ctc64.model(4)
    one = dataclasses.replace(std4, crnn=W.crnn_ctc_params(std4.crnn, np.zeros((1, 64), np.float32), np.zeros(1, np.float32)))
    nine = dataclasses.replace(std4, crnn=W.crnn_ctc_params(std4.crnn, np.zeros((9, 64), np.float32), np.zeros(9, np.float32)))
    gen = G.GEOMETRIES["c-t150"].bundle()
    gen = dataclasses.replace(gen, crnn=W.crnn_ctc_params(gen.crnn, gen.crnn.head_w2, gen.crnn.head_b2))
    softmax4 = G.synthetic_crnn(seed=311, **G._STD, n_out=4, head=G.SMX)
    return {
        "NOUT=1": W.pack_blob(one),
        "NOUT=9": W.pack_blob(nine),
        "generic geometry": W.pack_blob(gen),
        "HEAD=3": _patch_meta(W.pack_blob(softmax4), "crnn.meta", 13, 3),
        "HEAD=-1": _patch_meta(W.pack_blob(softmax4), "crnn.meta", 13, -1),
        "carries head_w1": _patch_meta(W.pack_blob(softmax4), "crnn.meta", 13, 2),
    }


@pytest.mark.parametrize("name", ["NOUT=1", "NOUT=9", "generic geometry", "HEAD=3", "HEAD=-1", "carries head_w1"])
def test_loader_refuses(pack_check, name):  # noqa: F811
    """Never a loaded model that a launch would have to refuse: WW_EBLOB, a message, no arrays."""
    (status, msg, arrays, _), = pack_check(_refused_blobs()[name])
    assert status == WW_EBLOB and msg.strip() and not arrays, (name, status, msg)


# ---- (c) the decode ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ctc64.hand_cases(), ids=lambda c: c[0])
def test_greedy_decode_hand_cases(case):
    _, steps, m, want_labels, want_length = case
    labels, lengths = ctc.greedy_decode(steps, m)
    assert labels.dtype == np.int32 and lengths.dtype == np.int32 and labels.shape == (1, m)
    assert labels[0].tolist() == want_labels and int(lengths[0]) == want_length


def test_greedy_decode_batch_and_defaults():
    cases = [c for c in ctc64.hand_cases() if c[1].shape == (19, 4)]
    labels, lengths = ctc.greedy_decode(np.stack([c[1] for c in cases]))   # max_labels defaults to T
    assert labels.shape == (len(cases), 19)
    for (_, s, _, _, n), row, ln in zip(cases, labels, lengths):
        assert ln == n and (row[n:] == -1).all() and (row[:n] >= 0).all()
    with pytest.raises(ValueError):
        ctc.greedy_decode(np.zeros((3, 1)))


# ---- (d) the wake-word rule ----------------------------------------------------------------------------------------------------------
def test_is_wakeword():
    rows = [([1, 2], 2, True), ([1, 2, 0], 3, True), ([1], 1, False), ([2, 1], 2, False), ([], 0, False)]
    for lab, n, want in rows:
        padded = np.array([(lab + [-1, -1, -1])[:3]], np.int32)
        assert bool(ctc.is_wakeword(padded, [n])[0]) is want, lab
        assert bool(ctc.is_wakeword(padded[:, :2], [n])[0]) is want, lab   # (max_labels = 2 is all the rule reads)
    assert ctc.is_wakeword(np.array([[1, 2], [1, -1], [1, 2]], np.int32), [2, 1, 5]).tolist() == [True, False, True]
    assert not ctc.is_wakeword(np.array([[1]], np.int32), [2])[0]             # one label kept: a two-label target cannot be read
    assert ctc.LABELS == ("[OTHER]", "[HEY]", "[SNIPS]")
    assert ctc.label_string([1, 2], 2) == "[HEY][SNIPS]" and ctc.label_string([0, -1], 1) == "[OTHER]" and ctc.label_string([1, 2], 5).endswith("...")


# ---- (e) what the GPU test's float64 comparison rests on ------------------------------------------------------------------------------
@pytest.mark.parametrize("L", ctc64.LS)
def test_reference_is_decidable_and_varied(L):
    _, w, steps, enc = ctc64.reference(L)
    assert steps.shape == (ctc64.N_WINDOWS, 19, L) and enc.shape == (ctc64.N_WINDOWS, 19, 64)
    np.testing.assert_allclose(steps.sum(axis=2), 1.0, atol=1e-12)
    d = ctc64.decidable(steps)
    assert (~d).sum() <= 0.1 * ctc64.N_WINDOWS, int((~d).sum())
    _, lengths = ctc64.decode64(steps)
    assert (lengths >= 2).any() and (lengths == 0).any(), np.bincount(lengths).tolist()
    # row t's halves are layer 2's states AT row t: the last states Crnn64.encode keeps are the forward half of row 18 and the
    # backward half of row 0
    one = ctc64.Ctc64(ctc64.model(L).crnn)
    last = one.encode(w[:3])
    np.testing.assert_allclose(np.concatenate([enc[:3, 18, :32], enc[:3, 0, 32:]], axis=1), last, rtol=0, atol=1e-12)


def test_decidable_is_the_stated_margin():
    p = np.array([[[0.5, 0.5 - 1e-9]], [[0.6, 0.4]], [[0.5 + 3e-5, 0.5 - 3e-5]], [[0.5 + 1e-5, 0.5 - 1e-5]]])
    # margins: 2 * 4e-5 * 0.5 = 4e-5 (+ 8 ulps of 0.5 = 4.8e-7): 0.2 and 6e-5 clear it, 1e-9 and 2e-5 do not
    assert ctc64.decidable(p).tolist() == [False, True, True, False]


# ---- (f) the evaluator's ratios ----------------------------------------------------------------------------------------------------
def test_ctc_statistics():
    from wwhip.evaluate import ctc_statistics
    y = [1] * 6 + [0] * 14
    p = [1, 1, 1, 1, 0, 0] + [1, 1, 1] + [0] * 11     # tp 4, fn 2, fp 3, tn 11
    s = ctc_statistics(y, p)
    assert (s["tp"], s["fn"], s["fp"], s["tn"]) == (4, 2, 3, 11)
    assert s["precision"] == 4 / 7 and s["recall"] == 4 / 6
    assert s["balanced accuracy"] == (4 / 6 + 11 / 14) / 2
    none = ctc_statistics([0, 0, 0], [0, 0, 0])
    assert none["precision"] == 0.0 and none["recall"] == 0.0 and none["balanced accuracy"] == 1.0   # (only the class that occurs)
    with pytest.raises(ValueError):
        ctc_statistics([0, 1], [0])
