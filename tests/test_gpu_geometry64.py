"""Every model geometry the loader accepts, on the MI355X, against float64.

The shipped models are three geometries; ``ww_model_load`` takes far more, and the kernels carry runtime parameters for all of
it.  ``tests/geometry64.py`` builds synthetic models at the edges of what the loader takes (``GEOMETRIES``: widths of the head,
a window one row short of the standard one, one live feature column, OF C = 63 / 65 / 576, T n_mel = 16,384, a Wavenet of one
row and one block, of 17 rows and 13 bands, of an odd block count, of T = 183 and one with every bound met at once) and reads them
in float64; ``tests/test_geometry64.py`` pins those readings on the CPU.  Here every form of the library that can run a row runs
it, through ``oracle.ref64.check_posteriors`` / ``check_enc`` with the needed value printed (``pytest -s``) and the fp32 C
oracle's own needed value beside it.  Bounds are the project's constants (tests/test_gpu_ref64.py, tests/test_gpu_wave_sequence.py).
Every output buffer handed to a ``_dev`` call is pre-filled with -1 and checked finite and within [0, 1]."""
import numpy as np
import pytest

import geometry64 as G
from oracle import ref64 as R

pytestmark = pytest.mark.gpu

TOL_POST = 1e-4     # the absolute rule on fp32 rows
TAU = 4e-5          # tests/test_gpu_ref64.py
TAU_E = 1.2e-5
TAU_BF16 = 6.5e-4
TAU_E_BF16 = 1.5e-4
TAU_STREAM = 3e-4
TAU_Z = 3.6e-5      # tests/test_gpu_wave_sequence.py
TAU_REL = 9e-7      # tests/test_gpu_frontend64.py
TAU_FFT = 1e-6
ALL = ("enc", "logits", "post_frames", "post")
FORMS = {"fused": {"crnn_split_at": 0}, "front + vector tail": {"crnn_split_at": 1, "crnn_tail_mfma": 0},
         "front + matrix tail": {"crnn_split_at": 1, "crnn_tail_mfma": 2}}   # tests/test_gpu_recurrence_forms.py


class Row:
    """One row of GEOMETRIES on the device with its float64 reading; references of further windows are memoised by their bytes."""

    def __init__(self, name):
        from oracle.cpu import CpuOracle
        from wwhip import weights as W
        self.name, self.g = name, G.GEOMETRIES[name]
        self.bundle = self.g.bundle()
        self.ref = G.reference(self.bundle)
        self.wins = G.row_windows(name)
        self.memo = {}
        self.post64, self.enc64 = self.ref64(self.wins)
        self.oracle = CpuOracle(G.blob_of(self.bundle)) if G.oracle_takes(self.g) else None
        self.engine = G.engine_for(self.bundle)
        self.col = self.bundle.posterior_index
        self.extra = []

    def ref64(self, wins):
        """(post64, enc64) of ``wins``, each distinct window evaluated once."""
        keys = [w.tobytes() for w in wins]
        new = {k: i for i, k in enumerate(keys) if k not in self.memo}
        if new:
            idx = list(new.values())
            p, e = self.ref.forward(wins[idx])
            for n, i in enumerate(idx):
                self.memo[keys[i]] = (p[n], e[n])
        return np.array([self.memo[k][0] for k in keys]), np.array([self.memo[k][1] for k in keys])

    def oracle_post(self, wins):
        return None if self.oracle is None else self.oracle.forward(wins)

    def engine_with(self, **kw):
        e = G.engine_for(self.bundle, **kw)
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


def _need(x):
    return "n/a" if x is None else f"{x:.2e}"


def _post(case, got, want64, tau, ora=None, absolute=True):
    got = np.asarray(got, np.float64).reshape(np.shape(want64))
    assert np.isfinite(got).all() and got.min() >= 0.0 and got.max() <= 1.0, case
    o = None if ora is None else R.needed_tau(np.asarray(ora, np.float64).reshape(np.shape(want64)), want64)
    print(f"\nGEO64 {case}: posterior needs tau {R.needed_tau(got, want64):.2e} (tau {tau:g}; the C oracle needs {_need(o)}), "
          f"max|dp| {np.abs(got - want64).max():.2e}", end="")
    R.check_posteriors(got, want64, tau)
    if absolute:
        assert np.abs(got - want64).max() < TOL_POST, case


def _enc(case, got, want64, tau_e, ora=None):
    assert np.isfinite(np.asarray(got)).all(), case
    need = float(R.enc_ratios(got, want64, 1.0).max())
    o = None if ora is None else float(R.enc_ratios(ora, want64, 1.0).max())
    print(f"\nGEO64 {case}: encoder needs tau_e {need:.2e} (tau_e {tau_e:g}; the C oracle needs {_need(o)})", end="")
    R.check_enc(got, want64, tau_e)


def _logits(case, got, want64, tau_z):
    got, want64 = np.asarray(got, np.float64), np.asarray(want64, np.float64).reshape(np.shape(got))
    dz = np.abs(got - want64).max(axis=-1) / np.maximum(1.0, np.abs(want64).max(axis=-1))
    print(f"\nGEO64 {case}: logits need tau_z {dz.max():.2e} (tau_z {tau_z:g})", end="")
    assert np.isfinite(got).all() and dz.max() <= tau_z, (case, float(dz.max()))


def _tiled(n_have, n, rng):
    return rng.choice(n_have, n, replace=False) if n < n_have else rng.permutation(np.resize(np.arange(n_have), n))


def _windows_dev(e, wins, valid):
    """``forward_windows_dev`` over ``wins`` with ``valid[w]`` valid rows each; the output buffer starts as -1."""
    import torch
    nw, T, F = wins.shape
    d_mel = torch.from_numpy(np.ascontiguousarray(wins).reshape(-1, F)).cuda()
    d_row = torch.arange(nw, dtype=torch.int64, device="cuda") * T
    d_valid = torch.from_numpy(np.asarray(valid, np.int32)).cuda()
    d_out = torch.full((nw, e.n_out), -1.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    e.forward_windows_dev(d_mel.data_ptr(), nw * T, d_row.data_ptr(), d_valid.data_ptr(), nw, d_out.data_ptr())
    e.ctx.synchronize()
    return d_out.cpu().numpy()


def _validity_case(r, valids, tau, what):
    """Windows whose rows from ``valid`` on hold other values than zero in the mel buffer: they must not be read.  Reference: the
    windows with those rows zero."""
    e = r.engine
    wins = r.wins[:len(valids)].copy()
    cut = wins.copy()
    for w, v in enumerate(valids):
        cut[w, v:] = 0.0
    want, _ = r.ref64(cut)
    _post(f"{r.name} forward_windows_dev, valid rows {list(valids)}{what}", _windows_dev(e, wins, valids), want, tau, r.oracle_post(cut))


def _pcm(seed, S, n):
    """[S, n] int16: noise whose level steps every 0.2 s (several decades), plus a chirp."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / 16000.0
    out = np.empty((S, n), np.int16)
    for s in range(S):
        level = np.repeat(np.exp(rng.uniform(np.log(30), np.log(6000), n // 3200 + 1)), 3200)[:n]
        chirp = 3000.0 * np.sin(2 * np.pi * (200.0 + 900.0 * s + 1500.0 * t) * t)
        out[s] = np.clip(np.rint(rng.normal(0, 1, n) * level + chirp), -32768, 32767)
    return out


def _run_bank(e, pcm, ticks, **flags):
    from wwhip.engine import StreamBank
    S = len(pcm)
    bank = StreamBank(e, S, **flags)
    posts = [[] for _ in range(S)]
    try:
        for t in range(ticks):
            p, k = bank.step(pcm[:, t * 320:(t + 1) * 320], np.ones(S, np.uint8))
            assert p.shape == (S, 2)
            for s in range(S):
                posts[s] += [float(p[s, j]) for j in range(k[s])]
    finally:
        bank.close()
    return posts


def _stream_case(r, e, pcm, ticks, forms, tau, what=""):
    """Window banks in the given forms against float64 on the hop-1 windows of ``Engine.logmel``'s rows.  Returns the posteriors
    per form."""
    mels = r.engine.logmel(list(pcm))
    want, ora = [], []
    for m in mels:
        sw = np.ascontiguousarray(R.stream_windows(m, r.g.T))
        want.append(r.ref64(sw)[0][:, r.col])
        ora.append(None if r.oracle is None else r.oracle.forward(sw)[:, r.col])
    want = np.concatenate(want)
    ora = None if r.oracle is None else np.concatenate(ora)
    got = {}
    for form, flags in forms:
        posts = _run_bank(e, pcm, ticks, **flags)
        for s in range(len(pcm)):
            assert len(posts[s]) == len(mels[s]), (form, s)
        got[form] = posts
        _post(f"{r.name}{what} stream bank, {form}, {len(pcm)} streams x {ticks} ticks", np.concatenate(posts)[:, None], want[:, None], tau,
              None if ora is None else ora[:, None], absolute=False)
    return got


# ---------------------------------------------------------------------------------------------------- every row: Engine.forward
@pytest.mark.parametrize("name", list(G.GEOMETRIES))
def test_forward(rows, name):
    """Engine.forward with encoder output at 1, 13 and 70 windows; Wavenets also at 300 (the four-wave form) and in both block
    loops.  w-t100-odd (NOUT 1: posterior identically 1) is checked through sequence_forward's logits and encodings on its T-row
    windows as well.  Measured on an MI355X: tau 1.4e-6 (w-t183, 70 windows, row-major loop; the C oracle needs 1.1e-6 there),
    tau_e 6.7e-7 (w-t183; the C oracle 4.9e-7), tau_z 1.4e-6 (w-t100-odd); the CRNN rows tau <= 8.7e-7.  On the small Wavenets (w-t1,
    w-t16, w-t17-m13) the kernels need up to 2.9e-7 where the C oracle needs under 1e-8: needed_tau counts only what exceeds 4 fp32
    ulps of p, the oracle (libm expf / tanhf, IEEE division) lands inside those, and the kernels' v_exp_f32 / v_rcp_f32 gates (~1 ulp
    each, |error| ~2e-7 in a gate) land one or two ulps outside: max|dp| there is 2.1e-7, five ulps of p = 0.4."""
    r = rows(name)
    e = r.engine
    assert (e.window, e.n_mel, e.n_out) == (r.g.T, r.g.n_mel, r.g.n_out)
    ora = None if r.oracle is None else r.oracle.forward(r.wins, want_enc=True)
    loops = (0, 1) if r.g.kind == "wavenet" else (None,)
    for rm in loops:
        opts = {} if rm is None else {"wavenet_rowmajor": rm}
        tag = "" if rm is None else f", wavenet_rowmajor={rm}"
        with e.options(**opts):
            for n in (1, 13, 70) + ((300,) if r.g.kind == "wavenet" else ()):
                idx = np.arange(n) if n <= len(r.wins) else _tiled(len(r.wins), n, np.random.default_rng(71))
                got, enc = e.forward(r.wins[idx], want_enc=True)
                _post(f"{name} forward, {n} windows{tag}", got, r.post64[idx], TAU, None if ora is None else ora[0][idx])
                _enc(f"{name} forward, {n} windows{tag}", enc.reshape(r.enc64[idx].shape), r.enc64[idx], TAU_E,
                     None if ora is None else ora[1][idx].reshape(r.enc64[idx].shape))
    if name == "w-t100-odd":
        got = e.sequence_forward(list(r.wins[:13]), want=("logits", "enc"))
        _logits(f"{name} sequence_forward on T rows", np.array(got["logits"]), r.ref.logits(r.wins[:13]), TAU_Z)
        _enc(f"{name} sequence_forward on T rows", np.array(got["enc"]), r.enc64[:13], TAU_E)
        assert (e.forward(r.wins) == 1.0).all()


# ---------------------------------------------------------------------------------------------------- standard-geometry CRNN rows
@pytest.mark.parametrize("name", G.STANDARD_ROWS)
def test_standard_dispatch_forms(rows, name):
    """Fused, front + vector tail, front + matrix tail at 1 and 17 windows: equal bits (posteriors and encodings), each against
    float64.  Measured: tau 4.7e-7 (c-std-n8; the C oracle 6.6e-7), tau_e 2.5e-7 (c-std-n3-sigmoid)."""
    r = rows(name)
    e = r.engine
    for n in (1, 17):
        wins = r.wins[:n]
        ora = r.oracle_post(wins)
        got = {}
        for form, opts in FORMS.items():
            with e.options(**opts):
                got[form] = e.forward(wins, want_enc=True)
            _post(f"{name} {form}, {n} windows", got[form][0], r.post64[:n], TAU, ora)
            _enc(f"{name} {form}, {n} windows", got[form][1], r.enc64[:n], TAU_E)
        for form in list(FORMS)[1:]:
            np.testing.assert_array_equal(got[form][0], got["fused"][0], err_msg=f"{name} {form}")
            np.testing.assert_array_equal(got[form][1], got["fused"][1], err_msg=f"{name} {form}")


@pytest.mark.parametrize("name", G.STANDARD_ROWS)
def test_standard_slide_and_validity(rows, name):
    """slide_forward at hops 1, 2 and 3 over 65 windows (crnn_rows_kernel and its tail) and over 10; forward_windows_dev with 0, 1,
    100 and T valid rows in every dispatch form.  Measured: tau 5.8e-7 (c-std-n8, hop 2, 10 windows; the C oracle 3.8e-7)."""
    r = rows(name)
    e, T = r.engine, r.g.T
    mel = np.concatenate(list(r.wins[:3]))
    for hop in (1, 2, 3):
        for nw in (65, 10):
            seq = mel[:T + hop * (nw - 1)]
            sw = np.ascontiguousarray(np.lib.stride_tricks.sliding_window_view(seq, (T, r.g.n_mel))[::hop, 0])
            assert len(sw) == nw
            _post(f"{name} slide_forward hop {hop}, {nw} windows", e.slide_forward(seq, hop), r.ref64(sw)[0], TAU, r.oracle_post(sw))
    for form, opts in FORMS.items():
        with e.options(**opts):
            _validity_case(r, (0, 1, 100, T), TAU, f", {form}")


@pytest.mark.parametrize("name", G.STANDARD_ROWS)
def test_standard_bf16x3(rows, name):
    """Engine(precision="bf16x3") (crnn_fused_bf16_kernel) at 1 and 70 windows.  Measured: tau 1.2e-5, tau_e 6.9e-6 (c-std-n3-sigmoid;
    the fp32 C oracle 4.1e-7: the rest is the split-bf16 products' 16 mantissa bits, as on the shipped CRNNs, 3e-5 .. 1e-4)."""
    r = rows(name)
    e = r.engine_with(precision="bf16x3")
    for n in (1, 70):
        got, enc = e.forward(r.wins[:n], want_enc=True)
        _post(f"{name} bf16x3, {n} windows", got, r.post64[:n], TAU_BF16, r.oracle_post(r.wins[:n]), absolute=False)
        _enc(f"{name} bf16x3, {n} windows", enc, r.enc64[:n], TAU_E_BF16)


@pytest.mark.parametrize("name", G.STANDARD_ROWS)
def test_standard_stream_bank(rows, name):
    """A StreamBank of 4 streams for 100 ticks: the default one-launch tick (crnn_stream_kernel), two launches, full_recompute -
    against float64 on the hop-1 windows of Engine.logmel's rows; one launch and two launches give the same bits.  Measured: tau 3.7e-7 (c-std-n8, one launch;
    the C oracle on the same windows 5.2e-7)."""
    r = rows(name)
    got = _stream_case(r, r.engine, _pcm(5, 4, 100 * 320), 100,
                       [("one launch", {}), ("two launches", dict(two_launch=True)), ("full_recompute", dict(full_recompute=True))], TAU_STREAM)
    assert got["one launch"] == got["two launches"]


# ---------------------------------------------------------------------------------------------------- generic CRNN rows
@pytest.mark.parametrize("name", G.GENERIC_ROWS)
def test_generic_forms(rows, name):
    """conv_generic_kernel -> gemm_nt_kernel -> gru_generic_kernel -> crnn_detect_kernel: forward_windows_dev with 0, 1, T - 1 and T
    valid rows, slide_forward at hop 2 over 9 windows, detect alone on the float64 encodings cast to fp32.  A ModelSet of generic
    models is refused when it is created.  (StreamBank(two_launch=True) is not refused for a generic model: the flag has no meaning
    for the table form and is ignored.)  Measured: tau 8.7e-7 (c-lds-limit, slide_forward; the C oracle 6.8e-7), detect alone 7.1e-7
    (c-t150).  c-lds-limit's conv asks for exactly 65,536 bytes of dynamic LDS and launches as it is."""
    from wwhip.engine import ModelSet
    r = rows(name)
    e, T = r.engine, r.g.T
    _validity_case(r, (0, 1, T - 1, T), TAU, "")
    mel = np.concatenate(list(r.wins[:4]))[:T + 2 * 8]
    if len(mel) == T + 16:
        sw = np.ascontiguousarray(np.lib.stride_tricks.sliding_window_view(mel, (T, r.g.n_mel))[::2, 0])
        assert len(sw) == 9
        _post(f"{name} slide_forward hop 2, 9 windows", e.slide_forward(mel, 2), r.ref64(sw)[0], TAU, r.oracle_post(sw))
    else:
        raise AssertionError("four windows must cover T + 16 rows")
    enc32 = r.enc64.astype(np.float32)
    _post(f"{name} detect alone, {len(enc32)} rows", e.detect(enc32), r.ref.detect(enc32), TAU)
    with pytest.raises(Exception, match="generic conv geometry"):
        ModelSet([e, e])


def test_c_t150_stream_bank(rows):
    """c-t150 is one row short of the standard window: its bank cannot be the incremental kernel's and must take the table form
    (per-window kernels over the generic path) - seen only through its results: the default bank and a full_recompute bank against
    float64, and the same bits from both.  Measured: tau 1.3e-6 (the C oracle 8.7e-7)."""
    r = rows("c-t150")
    got = _stream_case(r, r.engine, _pcm(6, 4, 60 * 320), 60, [("default", {}), ("full_recompute", dict(full_recompute=True))], TAU_STREAM)
    assert got["default"] == got["full_recompute"]


# ---------------------------------------------------------------------------------------------------- Wavenet rows
@pytest.mark.parametrize("name", G.WAVE_ROWS)
def test_wavenet_forms(rows, name):
    """precision="bf16x3" at 1 and 300 windows; detect alone, with rows whose only non-zero time step is row 0 / row T - 1;
    slide_forward at hops 1 and 3; forward_windows_dev with 0, 1, T - 1 and T valid rows.  Measured: fp32 tau 1.1e-6 (w-t183, slide_forward hop 3; the C
    oracle 1.2e-6); split-bf16 tau 3.6e-5, tau_e 2.3e-5 (w-t183, 300 windows; the fp32 C oracle 1.1e-6 - the split-bf16 products over 24
    blocks, a quarter of what the shipped Wavenet needs, 1.6e-4)."""
    r = rows(name)
    e, T, F = r.engine, r.g.T, r.g.n_mel
    rng = np.random.default_rng(79)
    nout1 = r.g.n_out == 1
    b = r.engine_with(precision="bf16x3")
    for n in (1, 300):
        idx = np.arange(n) if n <= len(r.wins) else _tiled(len(r.wins), n, rng)
        got, enc = b.forward(r.wins[idx], want_enc=True)
        _post(f"{name} bf16x3, {n} windows", got, r.post64[idx], TAU_BF16, r.oracle_post(r.wins[idx]), absolute=False)
        _enc(f"{name} bf16x3, {n} windows", enc, r.enc64[idx], TAU_E_BF16)
    edge = np.zeros((8, T, G.WS), np.float32)
    edge[:4, -1] = rng.uniform(0.0, 3.0, (4, G.WS))
    edge[4:, 0] = rng.uniform(0.0, 3.0, (4, G.WS))
    enc32 = np.concatenate([r.enc64[:12].astype(np.float32), edge])
    _post(f"{name} detect alone, {len(enc32)} rows", e.detect(enc32), r.ref.detect(enc32), TAU)
    mel = np.concatenate(list(r.wins[:40]))
    for hop in (1, 3):
        seq = mel[:T + hop * 11]
        sw = np.ascontiguousarray(np.lib.stride_tricks.sliding_window_view(seq, (T, F))[::hop, 0])
        assert len(sw) == 12
        _post(f"{name} slide_forward hop {hop}, 12 windows", e.slide_forward(seq, hop), r.ref64(sw)[0], TAU, r.oracle_post(sw))
    _validity_case(r, sorted({0, min(1, T), max(T - 1, 0), T}), TAU, "")
    assert nout1 == (name == "w-t100-odd")


@pytest.mark.parametrize("name", G.WAVE_ROWS)
def test_wavenet_sequence_form(rows, name):
    """sequence_forward(want=ALL) in one ragged call at lengths 1, T - 1, T, T + 1, 2 T + 5 and 500 against WaveSeq64.sequence with
    tests/test_gpu_wave_sequence.py's bounds; once more with wave_seq_segment small enough to cut the 500-row sequence: the same
    bits.  Measured: tau_e 9.5e-7 (w-t16), tau_z 2.8e-6 (w-t183), tau 7.8e-7 (w-t183, post_frames)."""
    r = rows(name)
    e, T, F = r.engine, r.g.T, r.g.n_mel
    lengths = [n for n in dict.fromkeys((1, T - 1, T, T + 1, 2 * T + 5, 500)) if n >= 1]
    seqs = [np.ascontiguousarray(G.windows(1000 + i, 1, L, F)[0]) for i, L in enumerate(lengths)]
    got = e.sequence_forward(seqs, want=ALL)
    with e.options(wave_seq_segment=200):   # the 500-row sequence in three segments, the 2 T + 5 ones of the long rows in two
        cut = e.sequence_forward(seqs, want=ALL)
    for i, (L, x) in enumerate(zip(lengths, seqs)):
        want = r.ref.seq.sequence(x)
        lab = f"{name} sequence of {L} rows"
        _enc(lab, got["enc"][i], want["enc"], TAU_E)
        _logits(lab, got["logits"][i], want["logits"], TAU_Z)
        if r.g.n_out > 1:
            _post(lab + ", post", got["post"][i][None], want["post"][None], TAU)
            _post(lab + ", post_frames", got["post_frames"][i], want["post_frames"], TAU)
        else:
            assert (got["post"][i] == 1.0).all() and (got["post_frames"][i] == 1.0).all()
        for k in ALL:
            np.testing.assert_array_equal(cut[k][i], got[k][i], err_msg=f"{lab}: {k} with wave_seq_segment set")


@pytest.mark.parametrize("name", ["w-t17-m13", "w-t100-odd", "w-max"])
def test_wavenet_causal_bank(rows, name):
    """A causal StreamBank of 3 streams: driven by step for 60 ticks, and by feed in packets of 1, 159, 160, 161 and 5,000 samples.
    Both emit sequence_forward's post_frames over the bank's own mel rows, bit for bit, and each other's bits; those rows'
    sequence_forward outputs against WaveSeq64 in float64 (w-t100-odd's post_frames are identically 1: its encodings and logits
    carry the check).  Measured: tau_e 4.7e-7 (w-max), tau_z 1.4e-6 (w-t100-odd), tau 1.2e-7 (w-t17-m13)."""
    from wwhip.engine import StreamBank
    r = rows(name)
    e, S, n = r.engine, 3, 60 * 320
    pcm = _pcm(9, S, n)
    stepped = _run_bank(e, pcm, 60, causal=True)
    bank = StreamBank(e, S, causal=True)
    posts, mels = [[] for _ in range(S)], [[] for _ in range(S)]
    try:
        at, sizes, k = np.zeros(S, int), (1, 159, 160, 161, 5000), 0
        while (at < n).any():
            ids = [s for s in range(S) if at[s] < n]
            ks = [min(sizes[(k + s) % len(sizes)], n - at[s]) for s in ids]
            p, m = bank.feed(ids, [pcm[s, at[s]:at[s] + c] for s, c in zip(ids, ks)], want_mel=True)
            for i, (s, c) in enumerate(zip(ids, ks)):
                assert len(p[i]) == len(m[i]) and m[i].shape[1:] == (r.g.n_mel,)
                posts[s].append(p[i])
                mels[s].append(m[i])
                at[s] += c
            k += 1
    finally:
        bank.close()
    seqs = [np.concatenate(x) for x in mels]
    got = e.sequence_forward(seqs, pool=e.window, want=ALL)
    for s in range(S):
        fed = np.concatenate(posts[s])
        assert len(fed) == len(seqs[s]) == (n - 512) // 160 + 1
        np.testing.assert_array_equal(fed, got["post_frames"][s][:, r.col], err_msg=f"{name} stream {s}: feed")
        np.testing.assert_array_equal(np.array(stepped[s], np.float32), fed, err_msg=f"{name} stream {s}: step against feed")
        want = r.ref.seq.sequence(seqs[s])
        lab = f"{name} causal bank, stream {s}, {len(fed)} rows"
        _enc(lab, got["enc"][s], want["enc"], TAU_E)
        _logits(lab, got["logits"][s], want["logits"], TAU_Z)
        if r.g.n_out > 1:
            _post(lab, fed[:, None], want["post_frames"][:, r.col][:, None], TAU)
        else:
            assert (fed == 1.0).all()


@pytest.mark.parametrize("name", ["w-t16", "w-t17-m13", "w-t100-odd", "w-t183"])
def test_wavenet_window_bank(rows, name):
    """A window StreamBank of 4 streams for 60 ticks against float64 on the hop-1 windows of Engine.logmel's rows.  w-t17-m13 and
    w-t100-odd (13 and 39 bands) and w-t183 (T) cannot take the one-launch tick (ww_wave_tick_capable) and run the front-end
    kernel + the window kernel; w-t16 can: its one-launch and two-launch banks give the same bits.  Measured: tau 2.8e-7 (w-t16; the C
    oracle 2.0e-7)."""
    r = rows(name)
    forms = [("default", {})] + ([("two launches", dict(two_launch=True))] if name == "w-t16" else [])
    pcm = _pcm(11, 4, 60 * 320)
    if r.g.n_out == 1:   # the posterior is identically 1: the bank's rows carry no figure, only their count and value
        for posts in (_run_bank(r.engine, pcm, 60, **flags) for _, flags in forms):
            assert all(len(p) == (60 * 320 - 512) // 160 + 1 and set(p) == {1.0} for p in posts)
        return
    got = _stream_case(r, r.engine, pcm, 60, forms, TAU_STREAM)
    if name == "w-t16":
        assert got["default"] == got["two launches"]


# ---------------------------------------------------------------------------------------------------- front end at another band count
@pytest.mark.parametrize("name", ["c-lds-limit", "w-t17-m13"])
def test_front_end_at_another_band_count(rows, name):
    """Engine.logmel with a filter of 32 / 13 bands on oracle.ref64.frontend_signals(3), precise and fast, against the float64
    front end with the cut filter (tests/test_gpu_frontend64.py's constants).  Measured: precise tau_rel 1.0e-7; fast tau_fft 1.2e-7
    (at tau_rel 9e-7), both rows."""
    from wwhip.engine import frontend_params
    r = rows(name)
    pcm = list(R.frontend_signals(3).values())
    want = R.LogMel64.concat([R.logmel64_samples(r.bundle.filt, R.quantise(p)) for p in pcm])
    for precise, tau_fft in ((True, 0.0), (False, TAU_FFT)):
        got = r.engine.logmel(pcm, frontend_params(precise=precise))
        got = np.asarray(np.concatenate(got), np.float64)
        assert got.shape == want.y.shape and np.isfinite(got).all(), (name, got.shape, want.y.shape)
        need = R.needed_taus(got, want, TAU_REL if tau_fft else 0.0, 0.0)
        print(f"\nGEO64 {name} logmel precise={precise}: needs tau_rel {need[0]:.2e} (tau_fft 0), tau_fft {need[1]:.2e} "
              f"(tau_rel {TAU_REL if tau_fft else 0:g}); max|dy| {np.abs(got - want.y).max():.2e}", end="")
        R.check_logmel(got, want, TAU_REL, tau_fft)
