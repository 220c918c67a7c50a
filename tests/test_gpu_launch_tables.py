"""Launch tables on their way to the device (csrc/common.h: ww_tables): every call that builds tables on the host
sends them through the context's two page-locked slots with one asynchronous copy and returns without waiting for anything -
its host arrays are free the moment it returns.  What the planners put INTO the tables is checked on the CPU
(tests/native/launch_plan_check.cpp); the feed's cuts are pinned bit for bit by tests/test_gpu_stream_feed.py."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# What a caller's arrays are overwritten with right after the call returns.  Zero, not wild values: a library that read an array
# late would plan from offsets and counts that are in bounds wherever a kernel uses them (a shared GPU is no place for a wild
# index), and the test would still fail - zero counts and offsets make the call a no-op or move its rows, so its output, zeroed
# beforehand, differs from the expected one, which is asserted to be non-zero.
OVERWRITE = 0


@pytest.fixture(scope="module")
def engines(assets):
    from wwhip.engine import Engine
    out = {m: Engine(os.path.join(assets, m)) for m in ("CRNN", "Wavenet")}
    assert out["CRNN"].ctx is out["Wavenet"].ctx  # one context: one stream, one pair of slots
    yield out
    for e in out.values():
        e.close()


def _segments(T, hop, seg_nw, gaps):
    rows, r = [], 0
    for nw, gap in zip(seg_nw, gaps):
        r += int(gap)
        rows.append(r)
        r += ((int(nw) - 1) * hop + T) if nw else 11
    return np.array(rows, np.int64), r


@pytest.mark.parametrize("name", ["CRNN", "Wavenet"])
def test_three_users_share_two_slots_and_sources_die_early(engines, name):
    """resample_dev (44.1 -> 16 kHz, two segments), forward_segments_dev (the window counts of
    test_forward_segments_dev_matches_explicit_windows at hop 2: the CRNN's tile path, the Wavenet's explicit-list fallback) and
    wave_sequence_dev (sequences of 1, 200 and 450 rows; on the Wavenet engine, which shares the context) enqueued back to back on
    one context with no synchronise in between: three uploads, so the third takes the first one's slot.  Each call's host offset
    and segment arrays are overwritten the moment it returns.  After ONE synchronise every result has the bits of the same call
    made alone with a synchronise behind it."""
    import torch
    from wwhip.resample import Resampler
    e, wv = engines[name], engines["Wavenet"]
    ctx = e.ctx
    rs = Resampler(44100, 16000, ctx=ctx)
    rng = np.random.default_rng(77)
    T, hop = e.window, 2
    # inputs and outputs on the device; the host tables are made afresh for every call (tables())
    lens = [3001, 4100]
    d_pcm = torch.from_numpy(np.clip(rng.normal(0, 3000, sum(lens)), -32768, 32767).astype(np.int16)).cuda()
    outs = [rs.out_len(n) for n in lens]
    seg_nw0 = [40, 0, 1, 15, 16, 17, 333, 2]
    seg_row0_0, rows = _segments(T, hop, seg_nw0, [0, 5, 3, 0, 7, 1, 2, 9])
    d_mel = torch.from_numpy(rng.uniform(0, 6.5, (rows + 4, 40)).astype(np.float32)).cuda()
    seq_offs0 = [0, 1, 201, 651]
    d_seq = torch.from_numpy(rng.uniform(0, 6.5, (seq_offs0[-1], 40)).astype(np.float32)).cuda()
    n_seq = len(seq_offs0) - 1

    def buffers():
        return {"y": torch.zeros(sum(outs), dtype=torch.float32, device="cuda"),
                "seg": torch.zeros((sum(seg_nw0), e.n_out), dtype=torch.float32, device="cuda"),
                "enc": torch.zeros((seq_offs0[-1], 32), dtype=torch.float32, device="cuda"),
                "logits": torch.zeros((seq_offs0[-1], wv.n_out), dtype=torch.float32, device="cuda"),
                "post_frames": torch.zeros((seq_offs0[-1], wv.n_out), dtype=torch.float32, device="cuda"),
                "post": torch.zeros((n_seq, wv.n_out), dtype=torch.float32, device="cuda")}

    def tables():
        return {"so": np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), "oo": np.concatenate([[0], np.cumsum(outs)]).astype(np.int64),
                "row0": seg_row0_0.copy(), "nw": np.array(seg_nw0, np.int32), "offs": np.array(seq_offs0, np.int64)}

    def resample(b, t):
        rs.resample_dev(d_pcm.data_ptr(), np.int16, t["so"], t["oo"], b["y"].data_ptr())
        return "so", "oo"

    def segments(b, t):
        e.forward_segments_dev(d_mel.data_ptr(), len(d_mel), t["row0"], t["nw"], hop, b["seg"].data_ptr())
        return "row0", "nw"

    def sequences(b, t):
        wv.wave_sequence_dev(d_seq.data_ptr(), len(d_seq), t["offs"], None, b["enc"].data_ptr(), b["logits"].data_ptr(),
                             b["post_frames"].data_ptr(), b["post"].data_ptr())
        return ("offs",)

    calls = (resample, segments, sequences)
    want = buffers()
    torch.cuda.synchronize()
    for call in calls:  # each alone, a synchronise behind it
        call(want, tables())
        ctx.synchronize()
    want = {k: v.cpu().numpy() for k, v in want.items()}
    assert all(np.abs(v).max() > 0 for v in want.values())
    got, t = buffers(), tables()
    torch.cuda.synchronize()
    for call in calls:
        for key in call(got, t):
            t[key][:] = OVERWRITE
    ctx.synchronize()
    for k, v in got.items():
        np.testing.assert_array_equal(v.cpu().numpy(), want[k], err_msg=k)
    rs.close()


def test_groups_of_one_call_alternate_the_slots(engines):
    """forward_segments_dev over three sequences of 16,385 windows at hop 2: any two exceed the 32,768 windows of a group, so the
    call uploads three groups' tables and the third waits for slot 0 while the first group's kernels may still run.  The result
    has the bits of the three sequences run one call each with a synchronise between; 64 sampled windows agree with
    Engine.forward on the explicit windows within test_forward_segments_dev_matches_explicit_windows' 2e-6."""
    import torch
    e = engines["CRNN"]
    T, hop, nw = e.window, 2, 16385
    rng = np.random.default_rng(78)
    seg_row0, rows = _segments(T, hop, [nw] * 3, [1, 3, 0])
    mel = rng.uniform(0, 6.5, (rows, 40)).astype(np.float32)
    d_mel = torch.from_numpy(mel).cuda()
    d_one, d_all = (torch.zeros((3 * nw, e.n_out), dtype=torch.float32, device="cuda") for _ in range(2))
    torch.cuda.synchronize()
    for s in range(3):
        e.forward_segments_dev(d_mel.data_ptr(), rows, seg_row0[s:s + 1].copy(), np.array([nw], np.int32), hop, d_one[s * nw:].data_ptr())
        e.ctx.synchronize()
    row0, cnt = seg_row0.copy(), np.full(3, nw, np.int32)
    e.forward_segments_dev(d_mel.data_ptr(), rows, row0, cnt, hop, d_all.data_ptr())
    row0[:], cnt[:] = OVERWRITE, OVERWRITE
    e.ctx.synchronize()
    got = d_all.cpu().numpy()
    np.testing.assert_array_equal(got, d_one.cpu().numpy())
    idx = np.sort(rng.choice(3 * nw, 64, replace=False))
    idx[0], idx[-1] = 0, 3 * nw - 1
    wins = np.stack([mel[seg_row0[w // nw] + (w % nw) * hop:][:T] for w in idx])
    err = float(np.abs(got[idx] - e.forward(wins)).max())
    assert err < 2e-6, err
