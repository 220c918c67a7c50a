"""CRNNs with LSTM cells or 16, 48, 64 units, and heads of another width than 64, on the MI355X against float64.

``tests/rnn64.py`` builds ten synthetic models (``ROWS``: the seven (cell, H) pairs besides the shipped GRU / 32 at the standard conv -
among them heads of F = 64 / sigmoid 1, F = 64 / softmax 2 and F = 40 / softmax 8 - an LSTM-48 on a conv of one step and one live
feature, a GRU-64 with a head of ONE unit on 30 steps of 63 features, an LSTM-64 on a conv of two steps) and reads them in float64
(``Rnn64``, pinned by ``tests/test_rnn64.py``).  Every row runs conv_generic_kernel -> gemm_nt_kernel -> rnn_layer_kernel<CELL, H> ->
gemm_nt_kernel -> rnn_layer_kernel -> crnn_head_kernel; together they cover 4 lanes per unit, idle lanes, two-wave directions, SEQP
pads of 32 and of 32 on 96, and GEMM N of 96 .. 512.  Bounds are the project's, as tests/test_gpu_geometry64.py states them (TAU 4e-5
for posteriors, TAU_E 1.2e-5 for encodings, TAU_STREAM 3e-4), through the same ``oracle.ref64`` checks with the needed value printed in
the ``GEO64`` line format (``pytest -s``).

Measured on an MI355X (one run): the figures in the docstrings below.
"""
import numpy as np
import pytest

import geometry64 as G
import rnn64 as R
from oracle import ref64 as R64  # noqa: F401  (the checks behind _post / _enc)
from test_gpu_geometry64 import TAU, TAU_E, TAU_STREAM, _enc, _pcm, _post, _stream_case, _validity_case

pytestmark = pytest.mark.gpu


class Row:
    """One row of rnn64.ROWS on the device with its float64 reading (test_gpu_geometry64.Row's attributes: its helpers take either)."""

    def __init__(self, name):
        self.name, self.g = name, R.ROWS[name]
        self.bundle = self.g.bundle()
        self.ref = R.Rnn64(self.bundle.crnn)
        self.wins = R.row_windows(name)
        self.memo = {}
        self.post64, self.enc64 = self.ref64(self.wins)
        self.oracle = None   # (the fp32 C oracle reads GRUs of 32 units only)
        self.engine = G.engine_for(self.bundle)
        self.col = self.bundle.posterior_index
        self.extra = []

    def ref64(self, wins):
        keys = [w.tobytes() for w in wins]
        new = {k: i for i, k in enumerate(keys) if k not in self.memo}
        if new:
            idx = list(new.values())
            p, e = self.ref.forward(wins[idx])
            for n, i in enumerate(idx):
                self.memo[keys[i]] = (p[n], e[n])
        return np.array([self.memo[k][0] for k in keys]), np.array([self.memo[k][1] for k in keys])

    def oracle_post(self, wins):
        return None

    def fresh_engine(self):
        e = G.engine_for(self.bundle)
        self.extra.append(e)
        return e

    def close(self):
        for e in self.extra + [self.engine]:
            e.close()


@pytest.fixture(scope="module")
def rows():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = Row(name)
        return cache[name]
    yield get
    for r in cache.values():
        r.close()


def _launched(ctx, call):
    """The kernels ``call`` launches, by the names the library's profile gives them."""
    ctx.synchronize()
    ctx.profile(True)
    try:
        ctx.profile_read()   # (a read empties the table)
        out = call()
        after = ctx.profile_read()
    finally:
        ctx.profile(False)
    return out, {k for k, v in after.items() if v["calls"] > 0}


@pytest.mark.parametrize("name", list(R.ROWS))
def test_forward(rows, name):
    """Engine.forward with encoder output at 1 and 70 windows, and the kernels it launches.  Measured: tau 1.0e-6 (gru64, 70 windows: a state sum of 64
    terms where the GRU / 32 rows of tests/test_gpu_geometry64.py, at 8.7e-7, have 32), tau_e 5.0e-7 (gru16, 70 windows)."""
    r = rows(name)
    e, p = r.engine, r.bundle.crnn
    assert (e.window, e.n_mel, e.n_out, e.enc_shape) == (r.g.T, r.g.n_mel, p.n_out, (1, 2 * p.units))
    assert (e.cell, e.units, e.head_units) == (p.cell, p.units, p.head_units)
    for n in (1, 70):
        (got, enc), names = _launched(e.ctx, lambda: e.forward(r.wins[:n], want_enc=True))
        assert names == {"conv_generic_kernel", "gemm_nt_kernel<gru1,generic>", "rnn_layer_kernel<seq>", "gemm_nt_kernel<gru2,generic>",
                         "rnn_layer_kernel<last>", "crnn_head_kernel"}, names
        _post(f"{name} forward, {n} windows", got, r.post64[:n], TAU)
        _enc(f"{name} forward, {n} windows", enc.reshape(r.enc64[:n].shape), r.enc64[:n], TAU_E)


@pytest.mark.parametrize("name", list(R.ROWS))
def test_forms(rows, name):
    """forward_windows_dev with 0, 1, T - 1 and T valid rows, slide_forward at hop 2 over 9 windows, detect alone on the float64
    encodings cast to fp32.  Measured: tau 6.5e-7 (gru48, slide_forward), 1.4e-7 (gru48, forward_windows_dev), detect alone 3.8e-7 (gru64)."""
    r = rows(name)
    e, T = r.engine, r.g.T
    _validity_case(r, sorted({0, 1, T - 1, T}), TAU, "")
    mel = np.concatenate(list(r.wins[:4]))[:T + 2 * 8]
    assert len(mel) == T + 16
    sw = np.ascontiguousarray(np.lib.stride_tricks.sliding_window_view(mel, (T, r.g.n_mel))[::2, 0])
    assert len(sw) == 9
    _post(f"{name} slide_forward hop 2, 9 windows", e.slide_forward(mel, 2), r.ref64(sw)[0], TAU)
    enc32 = r.enc64.astype(np.float32)
    _post(f"{name} detect alone, {len(enc32)} rows", e.detect(enc32), r.ref.detect(enc32), TAU)


@pytest.mark.parametrize("name", list(R.ROWS))
def test_same_bits_whatever_the_history(rows, name):
    """A 1-window forward on a fresh engine, and on an engine that has just run the 70-window call (whose workspace then holds 70
    windows' rows, pad columns included): equal bits.  Two engines share the context's workspace, so the second call of the fresh
    one repeats the comparison the other way round."""
    r = rows(name)
    fresh = r.fresh_engine()
    first = fresh.forward(r.wins[:1], want_enc=True)
    r.engine.forward(r.wins, want_enc=True)
    after = r.engine.forward(r.wins[:1], want_enc=True)
    again = fresh.forward(r.wins[:1], want_enc=True)
    for a, b in ((first, after), (first, again)):
        np.testing.assert_array_equal(a[0], b[0])
        np.testing.assert_array_equal(a[1], b[1])


def test_lstm32_stream_bank(rows):
    """LSTM-32 at the standard conv: its bank cannot be the incremental kernel's and takes the table form (per-window kernels over the
    layered path).  The default bank and a full_recompute bank, 4 streams x 60 ticks, against float64 on the hop-1 windows of
    Engine.logmel's rows, and the same bits from both.  Measured: tau 0 (every posterior within 4 fp32 ulps), max|dp| 1.5e-7, both forms."""
    r = rows("lstm32")
    got = _stream_case(r, r.engine, _pcm(6, 4, 60 * 320), 60, [("default", {}), ("full_recompute", dict(full_recompute=True))], TAU_STREAM)
    assert got["default"] == got["full_recompute"]


@pytest.mark.parametrize("name", ["lstm32", "gru48"])
def test_clip_and_plugin_paths(rows, name):
    """The paths above the window calls: clips_forward_dev on 5 clips of 1.5 s equals Engine.forward on the zero-padded windows built
    from Engine.logmel of the same clips, bit for bit (tests/test_gpu_clips64.py's rule: both sides run the same kernels on the same
    rows); wwhip.evaluate.clip_posteriors reports that window's posterior to within the absolute rule on fp32 rows (1e-4: its clip
    pass stages the clips its own way) and a sliding list per clip; a WakewordBank over a StreamBank, stage by stage as smoke() drives
    it, sees the posteriors a StreamBank alone emits for the same frames, bit for bit; a bank at 8 kHz mu-law emits two posteriors
    per 20 ms frame once its front end is under way, all of them posteriors."""
    import torch
    from wwhip.activation_timeout import ActivationTimeoutBank
    from wwhip.context import ContextBank
    from wwhip.vad import VadBank
    from wwhip.engine import StreamBank, frontend_params
    from wwhip.evaluate import clip_posteriors
    from wwhip.wakeword import WakewordBank
    r = rows(name)
    e = r.engine
    pcm = _pcm(21, 5, 24000)
    d_pcm = torch.from_numpy(pcm).cuda()
    d_out = torch.full((5, e.n_out), -1.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    e.clips_forward_dev(d_pcm.data_ptr(), 5, 24000, d_out.data_ptr(), frontend_params())
    e.ctx.synchronize()
    got = d_out.cpu().numpy()
    wins = np.zeros((5, e.window, 40), np.float32)
    for i, m in enumerate(e.logmel(list(pcm))):
        n = min(len(m), e.window)
        wins[i, :n] = m[:n]
    np.testing.assert_array_equal(got, e.forward(wins))
    one, sliding = clip_posteriors(e, list(pcm))
    assert one.shape == (5,) and np.abs(one - got[:, r.col]).max() < 1e-4
    assert len(sliding) == 5 and all(len(s) > 0 and np.isfinite(s).all() for s in sliding)
    S, ticks = 3, 14
    bank = StreamBank(e, S)
    posts = [[] for _ in range(S)]
    for t in range(ticks):
        p, k = bank.step(pcm[:S, t * 320:(t + 1) * 320], np.ones(S, np.uint8))
        for s in range(S):
            posts[s] += [float(p[s, j]) for j in range(k[s])]
    bank.close()
    ctxs, vad, timeout = ContextBank(S), VadBank(S), ActivationTimeoutBank(S)
    wake = WakewordBank(S, posterior_threshold=2.0, bank=StreamBank(e, S))
    seen = [[] for _ in range(S)]
    for t in range(ticks):
        f = pcm[:S, t * 320:(t + 1) * 320]
        vad(ctxs, f, raw=np.ones(S, bool))
        p = wake.step(ctxs, f)
        timeout(ctxs, f)
        for s in range(S):
            seen[s] += [float(p[s, j]) for j in range(wake.n_post[s])]
    wake.close()
    assert seen == posts and all(len(x) > 0 for x in posts) and not ctxs.is_active.any()
    codes = np.random.default_rng(22).integers(0, 256, (S, ticks * 160)).astype(np.uint8)   # any byte is a mu-law sample
    bank = StreamBank(e, S, sample_rate=8000, sample_format="mulaw")
    try:
        n = 0
        for t in range(ticks):
            p, k = bank.step(codes[:, t * 160:(t + 1) * 160], np.ones(S, np.uint8))
            for s in range(S):
                n += int(k[s])
                assert all(0.0 <= float(p[s, j]) <= 1.0 for j in range(k[s]))
        assert n >= S * (2 * ticks - 5)
    finally:
        bank.close()


def test_refusals(rows):
    """What refuses a generic-geometry CRNN refuses these: a ModelSet of two such models, a CtcStreamBank and ctc_forward on one -
    WW_EINVAL (a ValueError) before any launch."""
    from wwhip.engine import CtcStreamBank, ModelSet
    r = rows("lstm32")
    e = r.engine

    def refused():
        with pytest.raises(ValueError, match="cell 1"):
            ModelSet([e, e])
        with pytest.raises(ValueError, match="CTC-trained CRNN"):
            CtcStreamBank(e, 2)
        with pytest.raises(ValueError, match="CTC-trained CRNN"):
            e.ctc_forward(r.wins[:2])
    _, names = _launched(e.ctx, refused)
    assert names == set(), names
    g = rows("gru48").engine
    with pytest.raises(ValueError, match="48 units"):
        ModelSet([g, g])
