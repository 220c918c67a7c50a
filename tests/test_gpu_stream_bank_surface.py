"""``StreamBank``'s surface on the MI355X: whatever form a tick's frames are given in, and however a causal bank's samples are cut
into packets, the bank yields the same bits.  S = 3 streams, 3 ticks; every comparison is ``assert_array_equal`` on the integer
views of the posteriors.  (The CRNN has no causal form: the feed part runs on the fp32 Wavenet.)"""
import os

import numpy as np
import pytest
from numpy.testing import assert_array_equal

pytestmark = pytest.mark.gpu

S, TICKS = 3, 3
WAVES = ["Wavenet", "Wavenet_alt"]
KINDS = {
    "plain": {},
    "uniform 8000 pcm16": {"sample_rate": 8000},
    "uniform 8000 mulaw": {"sample_rate": 8000, "sample_format": "mulaw"},
    "per-stream pcm16": {"sample_rate": [48000, 16000, 8000]},
    "per-stream g711": {"sample_rate": [8050, 16000, 8000], "sample_format": ["mulaw", "pcm16", "alaw"]},
}


@pytest.fixture(scope="module")
def engines(assets):
    from wwhip.engine import Engine
    out = {m: Engine(os.path.join(assets, m)) for m in ["CRNN"] + WAVES}
    yield out
    for e in out.values():
        e.close()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _samples(rng, n, fmt):
    """n samples of a stream that reads ``fmt``: G.711 codes, or a tone plus noise as int16."""
    if fmt != "pcm16":
        return rng.integers(0, 256, n, dtype=np.uint8)
    return np.clip(np.rint(6000 * np.sin(np.arange(n) * 0.05) + rng.normal(0, 2500, n)), -32768, 32767).astype(np.int16)


def _ticks(bank, frames):
    out = [bank.step(f, np.ones(S, np.uint8)) for f in frames]
    return np.stack([_bits(p) for p, _ in out]), np.stack([n for _, n in out])


@pytest.mark.parametrize("model,causal", [("CRNN", False), ("Wavenet", True)])
def test_every_frame_form_and_packet_cut_yields_the_same_bits(engines, model, causal):
    """Part 1, on the five bank kinds: ``step`` given the flat block, S per-stream arrays and - where every stream's frame has one
    length and one dtype - the ``[S, frame_samples]`` array returns identical ``post`` bits and ``n``, tick by tick.
    Part 2, on the causal bank: ``feed`` given each stream's samples as one packet and as three returns identical bits, on a bank of
    pcm16 streams and on one with a G.711 stream."""
    from wwhip.engine import StreamBank
    eng = engines[model]
    rng = np.random.default_rng(7)
    for kind, kw in KINDS.items():
        probe = StreamBank(eng, S, causal=causal, **kw)
        fs, fb, bo, names = np.broadcast_to(probe.frame_samples, S), probe.frame_bytes, probe.frame_byte_offs, probe.sample_formats
        probe.close()
        g711 = any(f != "pcm16" for f in names)
        per = [[_samples(rng, int(fs[s]), names[s]) for s in range(S)] for _ in range(TICKS)]
        flat = []
        for t in range(TICKS):
            block = np.zeros(int(bo[S]), np.uint8)
            for s in range(S):
                block[bo[s]:bo[s] + fb[s]] = per[t][s].view(np.uint8)
            flat.append(block if g711 else block.view(np.int16))
        forms = {"flat": flat, "per-stream": per}
        if len(set(fs.tolist())) == 1 and len(set(names)) == 1:
            forms["2-D"] = [np.stack(p) for p in per]
        assert ("2-D" in forms) == (not kind.startswith("per-stream"))
        got = {}
        for form, frames in forms.items():
            bank = StreamBank(eng, S, causal=causal, **kw)
            got[form] = _ticks(bank, frames)
            bank.close()
        post, n = got["flat"]
        assert n.sum() > 0, kind  # (three ticks complete a first frame on every kind: something is compared)
        for form in forms:
            assert_array_equal(got[form][1], n, err_msg=f"{kind}: n of {form}")
            assert_array_equal(got[form][0], post, err_msg=f"{kind}: post of {form}")
    if not causal:
        return
    for kw in ({}, {"sample_rate": [8000, 16000, 8000], "sample_format": ["mulaw", "pcm16", "pcm16"]}):
        names = kw.get("sample_format", ["pcm16"] * S)
        rates = kw.get("sample_rate", [16000] * S)
        sig = [_samples(rng, rates[s] // 10 + 37 * s, names[s]) for s in range(S)]  # 100 ms and a little: several rows
        one = StreamBank(eng, S, causal=True, **kw)
        whole, _ = one.feed([0, 1, 2], sig)
        one.close()
        three = StreamBank(eng, S, causal=True, **kw)
        parts = [[] for _ in range(S)]
        cuts = [[0, len(x) // 3, 2 * len(x) // 3 + 1, len(x)] for x in sig]  # (an odd cut among them)
        for k in range(3):
            posts, _ = three.feed([2, 0, 1], [sig[s][cuts[s][k]:cuts[s][k + 1]] for s in (2, 0, 1)])
            for s, p in zip((2, 0, 1), posts):
                parts[s].append(p)
        three.close()
        assert sum(p.size for p in whole) > 0
        for s in range(S):
            assert_array_equal(_bits(np.concatenate(parts[s])), _bits(whole[s]), err_msg=f"stream {s} of {names}")


def test_feed_all_columns_are_the_members_feeds(engines):
    """``feed_all`` on a causal ``members="all"`` bank of a two-member Wavenet set: column ``j`` is ``feed`` on a bank of member ``j``."""
    from wwhip.engine import ModelSet, StreamBank
    rng = np.random.default_rng(11)
    sig = [_samples(rng, 1600 + 41 * s, "pcm16") for s in range(S)]
    ms = ModelSet([engines[m] for m in WAVES])
    try:
        every = StreamBank(ms, S, causal=True, members="all")
        posts, _ = every.feed_all([0, 1, 2], sig)
        every.close()
        assert all(p.shape[1] == 2 and p.shape[0] > 0 for p in posts)
        for j, m in enumerate(WAVES):
            alone = StreamBank(engines[m], S, causal=True)
            want, _ = alone.feed([0, 1, 2], sig)
            alone.close()
            for s in range(S):
                assert_array_equal(_bits(posts[s][:, j]), _bits(want[s]), err_msg=f"member {j}, stream {s}")
    finally:
        ms.close()
