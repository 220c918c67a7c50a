"""The HIP path against the float64 reference (oracle/ref64.py), in logit space.

Every case checks posteriors with ``check_posteriors`` - ``|p - p64| <= tau * min(p64, 1 - p64)`` plus a few fp32 ulps -
on mel windows whose posteriors cover each model's whole logit range (``decision_windows``), and keeps the absolute
``|dp| < 1e-4`` rule of the other tests as well.  Each case prints the tau it needed (``pytest -s``); every tau below is
about 4x the worst measured on an MI355X, quoted in the test's docstring."""
import os

import numpy as np
import pytest

from oracle import ref64 as R

pytestmark = pytest.mark.gpu

MODELS = ["CRNN", "CRNN_softmax", "Wavenet", "Wavenet_alt", "CRNN_nosilence", "CRNN_nosilence_enhanced", "CRNN_old"]
SEED = 7            # decision windows (tests/test_ref64.py pins their coverage)
STREAM_SEED = 5     # the streaming input (tests/test_ref64.py pins its logit span)
STREAM_TICKS = 100
TOL_POST = 1e-4     # the absolute rule of tests/test_gpu_parity.py, kept
TAU = 4e-5          # fp32 posteriors (measured 9.8e-6)
TAU_E = 1.2e-5      # fp32 encoder output, relative to max(1, max|row|) (measured 2.9e-6)
TAU_BF16 = 6.5e-4   # precision="bf16x3" posteriors (measured 1.6e-4)
TAU_E_BF16 = 1.5e-4  # precision="bf16x3" encoder output (measured 3.7e-5)
TAU_STREAM = 3e-4   # streaming, after the front end (measured 7.6e-5)
TAU_STREAM_BF16 = 2.1e-4  # precision="bf16x3" stream banks (measured 5.15e-5)
TOL_FILTER = 3e-6   # filter.tflite alone: absolute log-mel (measured 7.8e-7)


def _post(case, got, want64, tau):
    got = np.asarray(got, np.float64).reshape(np.shape(want64))
    print(f"\nREF64 {case}: posterior needs tau {R.needed_tau(got, want64):.2e} (tau {tau:g}), "
          f"max|dp| {np.abs(got - want64).max():.2e}", end="")
    ratio = R.check_posteriors(got, want64, tau)
    assert np.abs(got - want64).max() < TOL_POST, case
    return ratio


def _enc(case, got, want64, tau_e):
    need = float(R.enc_ratios(got, want64, 1.0).max())
    print(f"\nREF64 {case}: encoder needs tau_e {need:.2e} (tau_e {tau_e:g})", end="")
    return R.check_enc(got, want64, tau_e)


@pytest.fixture(scope="module")
def engines(assets):
    from wwhip.engine import Engine
    out = {m: Engine(os.path.join(assets, m)) for m in MODELS}
    yield out
    for e in out.values():
        e.close()


@pytest.fixture(scope="module")
def oracles(engines):
    from oracle.cpu import CpuOracle
    return {m: CpuOracle(e.blob) for m, e in engines.items()}


@pytest.fixture(scope="module")
def ref(assets, oracles):
    """name -> (Ref64, decision windows, out64, enc64), computed once per module."""
    cache = {}

    def get(name):
        if name not in cache:
            r = R.Ref64(os.path.join(assets, name))
            wins = R.decision_windows(oracles[name], oracles[name].window, SEED)
            cache[name] = (r, wins) + r.forward(wins)
        return cache[name]
    return get


def _ref_windows(r, wins, memo):
    """Ref64 posteriors of many windows, each distinct window evaluated once."""
    out = []
    for w in wins:
        k = w.tobytes()
        if k not in memo:
            memo[k] = r.forward(w[None])[0][0]
        out.append(memo[k])
    return np.array(out)


def _tiled(n_dec, n, rng):
    """Row indices for a batch of ``n`` decision windows: every window (cyclically) at shuffled positions."""
    if n < n_dec:
        return rng.choice(n_dec, n, replace=False)
    return rng.permutation(np.resize(np.arange(n_dec), n))


# ---------------------------------------------------------------- a. Engine.forward, every model
@pytest.mark.parametrize("name", MODELS)
def test_forward_decision_windows(engines, oracles, ref, name):
    """Decision windows one per launch and at shuffled positions of a 70-window batch of random windows, encoder output
    included.  Measured: tau 9.8e-6 (CRNN_nosilence), tau_e 2.9e-6 (CRNN_old)."""
    e = engines[name]
    _, wins, out64, enc64 = ref(name)
    one = np.concatenate([e.forward(w[None]) for w in wins])
    _post(f"{name} forward, one window per launch", one, out64, TAU)
    rng = np.random.default_rng(61)
    batch = rng.uniform(0, 6.5, (70, e.window, 40)).astype(np.float32)
    pos = rng.choice(70, len(wins), replace=False)
    batch[pos] = wins
    got, enc = e.forward(batch, want_enc=True)
    _post(f"{name} forward, in a batch of 70", got[pos], out64, TAU)
    _enc(f"{name} forward, in a batch of 70", enc[pos], enc64, TAU_E)
    rest = np.setdiff1d(np.arange(70), pos)
    assert np.abs(got[rest] - oracles[name].forward(batch[rest])).max() < TOL_POST


# ---------------------------------------------------------------- b. CRNN launch forms
def _slide_seqs(wins, T):
    """Two mel sequences of concatenated decision windows (low, high and middle logits): 80 and 40 windows at hop 2."""
    n = len(wins) - 2
    a = np.concatenate([wins[n // 4], wins[n - 1], wins[n // 2]])[:T + 2 * 79]
    b = np.concatenate([wins[n - 1], wins[1]])[:T + 2 * 39]
    return a, b


@pytest.mark.parametrize("name", ["CRNN", "CRNN_softmax"])
def test_crnn_launch_forms(engines, ref, name):
    """One fused kernel, front + tail (gru_tail_kernel and gru_tail16_kernel), slide_forward with >= 64 windows
    (crnn_rows_kernel) and fewer, forward_segments_dev over two sequences - every slid window against Ref64.
    Measured: tau 5.6e-6 (CRNN, 80 slid windows), tau_e 1.4e-6."""
    import torch
    e = engines[name]
    r, wins, out64, enc64 = ref(name)
    T = e.window
    with e.options(crnn_split_at=0):
        got, enc = e.forward(wins, want_enc=True)
    _post(f"{name} fused kernel", got, out64, TAU)
    _enc(f"{name} fused kernel", enc, enc64, TAU_E)
    for mfma in (0, 2):
        with e.options(crnn_split_at=1, crnn_tail_mfma=mfma):
            got, enc = e.forward(wins, want_enc=True)
        _post(f"{name} front + tail, crnn_tail_mfma={mfma}", got, out64, TAU)
        _enc(f"{name} front + tail, crnn_tail_mfma={mfma}", enc, enc64, TAU_E)
    memo = {}
    seqs = _slide_seqs(wins, T)
    want = []
    for seq, nw in zip(seqs, (80, 40)):
        sw = np.lib.stride_tricks.sliding_window_view(seq, (T, 40))[::2, 0]
        assert len(sw) == nw
        w64 = _ref_windows(r, sw, memo)
        want.append(w64)
        _post(f"{name} slide_forward hop 2, {nw} windows", e.slide_forward(seq, 2), w64, TAU)
        with e.options(crnn_tail_mfma=2):
            _post(f"{name} slide_forward hop 2, {nw} windows, crnn_tail_mfma=2", e.slide_forward(seq, 2), w64, TAU)
    mel = np.concatenate(seqs)
    d_mel = torch.from_numpy(mel).cuda()
    d_out = torch.zeros((120, e.n_out), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    e.forward_segments_dev(d_mel.data_ptr(), len(mel), np.array([0, len(seqs[0])], np.int64), np.array([80, 40], np.int32), 2,
                           d_out.data_ptr())
    e.ctx.synchronize()
    _post(f"{name} forward_segments_dev, 80 + 40 windows", d_out.cpu().numpy(), np.concatenate(want), TAU)


# ---------------------------------------------------------------- c. the generic CRNN path
def test_crnn_generic_path_batch_sizes(engines, ref):
    """CRNN_old (conv_generic_kernel -> gemm_nt_kernel -> gru_generic_kernel) at 1, 7, 64, 65 and 333 windows: the GEMM's
    M tails and its m-tile rounding, decision windows at every position.  Measured: tau 6.0e-6, tau_e 2.9e-6."""
    e = engines["CRNN_old"]
    _, wins, out64, enc64 = ref("CRNN_old")
    rng = np.random.default_rng(67)
    for n in (1, 7, 64, 65, 333):
        idx = _tiled(len(wins), n, rng)
        got, enc = e.forward(wins[idx], want_enc=True)
        _post(f"CRNN_old batch {n}", got, out64[idx], TAU)
        _enc(f"CRNN_old batch {n}", enc, enc64[idx], TAU_E)


# ---------------------------------------------------------------- d. Wavenet block loop forms
@pytest.mark.parametrize("name", ["Wavenet", "Wavenet_alt"])
def test_wavenet_block_loop_forms(engines, ref, name):
    """fp32 Wavenet, transposed and row-major block loop (wavenet_rowmajor 0 and 1), at the decision windows and in a
    300-window launch (four waves x three tiles).  Measured: tau 6.4e-6 (Wavenet, transposed), tau_e 1.5e-6."""
    e = engines[name]
    _, wins, out64, enc64 = ref(name)
    idx = _tiled(len(wins), 300, np.random.default_rng(71))
    for rm in (0, 1):
        with e.options(wavenet_rowmajor=rm):
            got, enc = e.forward(wins, want_enc=True)
            big, big_enc = e.forward(wins[idx], want_enc=True)
        _post(f"{name} wavenet_rowmajor={rm}", got, out64, TAU)
        _enc(f"{name} wavenet_rowmajor={rm}", enc, enc64, TAU_E)
        _post(f"{name} wavenet_rowmajor={rm}, 300 windows", big, out64[idx], TAU)
        _enc(f"{name} wavenet_rowmajor={rm}, 300 windows", big_enc, enc64[idx], TAU_E)


# ---------------------------------------------------------------- e. split-bf16
@pytest.mark.parametrize("name", ["CRNN", "CRNN_softmax", "CRNN_nosilence_enhanced", "Wavenet", "Wavenet_alt"])
def test_bf16x3_decision_windows(assets, ref, name):
    """precision="bf16x3" at the decision windows and in a 300-window launch.  Measured: tau 1.6e-4 (Wavenet), tau_e 3.7e-5
    (Wavenet); the CRNNs 3e-5 .. 1e-4."""
    from wwhip.engine import Engine
    _, wins, out64, enc64 = ref(name)
    e = Engine(os.path.join(assets, name), precision="bf16x3")
    try:
        got, enc = e.forward(wins, want_enc=True)
        _post(f"{name} bf16x3", got, out64, TAU_BF16)
        _enc(f"{name} bf16x3", enc, enc64, TAU_E_BF16)
        idx = _tiled(len(wins), 300, np.random.default_rng(73))
        got, enc = e.forward(wins[idx], want_enc=True)
        _post(f"{name} bf16x3, 300 windows", got, out64[idx], TAU_BF16)
        _enc(f"{name} bf16x3, 300 windows", enc, enc64[idx], TAU_E_BF16)
    finally:
        e.close()


# ---------------------------------------------------------------- f. detect and filter alone, both sides of the staging switch
@pytest.mark.parametrize("name,sizes,lo,hi", [("CRNN", (1, 3, 1100), -1.0, 1.0), ("CRNN_softmax", (1, 3, 1100), -1.0, 1.0),
                                              ("Wavenet", (1, 11, 12, 40), 0.0, 3.0), ("Wavenet_alt", (1, 11, 12, 40), 0.0, 3.0)])
def test_detect_alone(engines, ref, name, sizes, lo, hi):
    """Engine.detect (ww_detect) on the decision windows' float64 encoder outputs cast to fp32 and random rows in the
    encoder's range, below and above WW_SMALL_IO_BYTES (256 KB: 12 Wavenet rows, ~1,000 CRNN rows) - against Ref64.detect
    of the same fp32 rows.  Wavenet rows whose last (or first) time step alone is non-zero put the head's max over time at
    the edges of its loop.  Measured: tau 2.0e-6."""
    e = engines[name]
    r, _, _, enc64 = ref(name)
    rng = np.random.default_rng(79)
    shape = (-1,) + e.enc_shape
    rows = [enc64.astype(np.float32).reshape(shape), rng.uniform(lo, hi, (24,) + e.enc_shape).astype(np.float32)]
    if not e.is_crnn:
        edge = np.zeros((8,) + e.enc_shape, np.float32)
        edge[:4, -1] = rng.uniform(lo, hi, (4, e.enc_shape[1]))
        edge[4:, 0] = rng.uniform(lo, hi, (4, e.enc_shape[1]))
        rows.append(edge)
    rows = np.concatenate(rows)
    want = r.detect(rows.reshape((len(rows),) + enc64.shape[1:]))
    for n in sizes + (len(rows),):
        idx = _tiled(len(rows), n, rng)
        _post(f"{name} detect n={n}", e.detect(rows[idx]), want[idx], TAU)


@pytest.mark.parametrize("name", ["CRNN", "Wavenet"])
def test_filter_alone(engines, ref, name):
    """Engine.filter_apply (ww_filter_apply) at 1, 220, 221 and 5,000 rows (the staging switch at ~221 rows): rows of real
    STFT magnitude, zero rows and a full-scale tone, against Ref64.filter.  Measured: max|d log-mel| 7.8e-7."""
    from oracle.cpu import stft_mag
    e = engines[name]
    r = ref(name)[0]
    rng = np.random.default_rng(83)
    t = np.arange(16000) / 16000.0
    x = rng.normal(0, 0.05, 16000) * np.linspace(0, 1, 16000) + 0.3 * np.sin(2 * np.pi * 440 * t)
    frames = np.lib.stride_tricks.sliding_window_view(x, 512)[::160][:90]
    tone = 0.999 * np.sin(2 * np.pi * 1000 * t[:512 * 3]).reshape(3, 512)
    mag = np.concatenate([stft_mag(frames.astype(np.float32)), np.zeros((3, 257), np.float32), stft_mag(tone.astype(np.float32))])
    want = r.filter(mag)
    for n in (1, 220, 221, 5000):
        idx = _tiled(len(mag), n, rng)
        got = e.filter_apply(mag[idx])
        err = float(np.abs(got - want[idx]).max())
        print(f"\nREF64 {name} filter n={n}: max|d log-mel| {err:.2e} (bound {TOL_FILTER:g})", end="")
        assert err < TOL_FILTER, (n, err)


SMALL_IO_BYTES = 256 << 10  # WW_SMALL_IO_BYTES (csrc/api.hip): up to here a host-pointer call stages in pinned memory


def _need(n_bytes):
    """ww_bump::need: what a staged buffer takes, a multiple of 256 bytes."""
    return (n_bytes + 255) & ~255


@pytest.mark.parametrize("name", ["CRNN", "Wavenet"])
def test_forward_with_enc_either_side_of_the_staging_switch(engines, ref, name):
    """Engine.forward(want_enc=True) (ww_forward_enc) at the largest window count whose mel, posteriors and encoder rows
    stage in pinned memory and at the next one, which goes through the device arena: 10 and 11 windows of 151 x 40 (CRNN),
    4 and 5 of 182 x 40 (Wavenet)."""
    e = engines[name]
    _, wins, out64, enc64 = ref(name)

    def staged(n):
        return _need(n * e.window * e.n_mel * 4) + _need(n * e.n_out * 4) + _need(n * e.enc_shape[0] * e.enc_shape[1] * 4)
    n_pin = max(n for n in range(1, 65) if staged(n) <= SMALL_IO_BYTES)
    assert n_pin == {"CRNN": 10, "Wavenet": 4}[name]
    rng = np.random.default_rng(89)
    for n in (n_pin, n_pin + 1):
        idx = _tiled(len(wins), n, rng)
        got, enc = e.forward(wins[idx], want_enc=True)
        _post(f"{name} forward with enc, {n} windows", got, out64[idx], TAU)
        _enc(f"{name} forward with enc, {n} windows", enc, enc64[idx], TAU_E)


@pytest.mark.parametrize("name", ["CRNN", "Wavenet"])
def test_slide_forward_hop_1_at_64_and_65_windows(engines, ref, name):
    """Engine.slide_forward at hop 1 over 64 and 65 windows: bytes far below SMALL_IO_BYTES, which stage in pinned memory up
    to 64 windows and in the device arena above (the CRNN also changes kernel form at 64 windows, crnn_slide_min) - every slid window against
    Ref64."""
    e = engines[name]
    r, wins, _, _ = ref(name)
    T = e.window
    seq = _slide_seqs(wins, T)[0][:T + 64]
    sw = np.lib.stride_tricks.sliding_window_view(seq, (T, 40))[:, 0]
    assert len(sw) == 65
    want = r.forward(sw)[0]
    for nw in (64, 65):
        _post(f"{name} slide_forward hop 1, {nw} windows", e.slide_forward(seq[:T + nw - 1], 1), want[:nw], TAU)


# ---------------------------------------------------------------- g. streaming
STREAM_S = 8


@pytest.fixture(scope="module")
def stream_ref(engines, oracles, ref):
    """name -> (pcm, want, want64), computed once per module: 8 streams offset in time by 2 ticks each on a PCM stream whose
    posteriors cross the decision range; ``want[s]``: the C oracle's log-mel rows, Ref64 on the hop-1 windows (as
    test_stream_bank_matches_batch_path builds them); ``want64[s]`` for two of the streams: the float64 front end's rows
    (Ref64.logmel) instead of the C oracle's."""
    cache = {}

    def get(name):
        if name in cache:
            return cache[name]
        e, ora = engines[name], oracles[name]
        r = ref(name)[0]
        S, n = STREAM_S, STREAM_TICKS * 320
        src = R.decision_stream(ora, n, STREAM_SEED)
        pcm = np.stack([np.concatenate([np.zeros(2 * s * 320, np.int16), src])[:n] for s in range(S)])
        memo, want = {}, []
        for s in range(S):
            want.append(_ref_windows(r, R.stream_windows(ora.logmel(pcm[s]), e.window), memo)[:, e.posterior_index])
        assert len(memo) <= len(want[0]) + 1    # the delayed streams share stream 0's windows
        # the same streams with the float64 front end's rows (Ref64.logmel: its silence rows are not exactly 0, so the delayed streams
        # do not share windows with stream 0 - streams 0 and S - 1 stand for them)
        memo64, want64 = {}, {}
        for s in (0, S - 1):
            mel64 = r.logmel(pcm[s]).y.astype(np.float32)
            want64[s] = _ref_windows(r, R.stream_windows(mel64, e.window), memo64)[:, e.posterior_index]
        cache[name] = (pcm, want, want64)
        return cache[name]
    return get


def _run_bank(e, pcm, **flags):
    """The posteriors of every stream of a StreamBank over STREAM_TICKS ticks of 20 ms."""
    from wwhip.engine import StreamBank
    S = len(pcm)
    bank = StreamBank(e, S, **flags)
    posts = [[] for _ in range(S)]
    try:
        for t in range(STREAM_TICKS):
            p, k = bank.step(pcm[:, t * 320:(t + 1) * 320], np.ones(S, np.uint8))
            for s in range(S):
                posts[s] += [float(p[s, j]) for j in range(k[s])]
    finally:
        bank.close()
    return posts


def _stream_post(case, posts, want, want64, tau):
    S = len(posts)
    for s in range(S):
        assert len(posts[s]) == len(want[s])
    _post(f"{case}, {S} streams", np.concatenate(posts)[:, None], np.concatenate(want)[:, None], tau)
    _post(f"{case}, streams 0 and {S - 1} against Ref64.logmel rows",
          np.concatenate([posts[s] for s in want64])[:, None], np.concatenate(list(want64.values()))[:, None], tau)


@pytest.mark.parametrize("name", ["CRNN", "Wavenet"])
def test_stream_bank_vs_float64(engines, stream_ref, name):
    """StreamBank's default one-launch tick and a full_recompute bank, 8 streams offset in time by 2 ticks each, on a PCM
    stream whose posteriors cross the decision range; reference: the C oracle's log-mel rows, Ref64 on the hop-1 windows
    (as test_stream_bank_matches_batch_path builds them), and for two of the streams the float64 front end's rows
    (Ref64.logmel) instead of the C oracle's.  Measured: tau 7.6e-5 (CRNN: the GPU front end's log-mel rows are
    not the oracle's to the last bit), 4.5e-6 (Wavenet); against Ref64.logmel rows 6.2e-5 (CRNN), 4.1e-6 (Wavenet) - the CRNN's
    tau is its sensitivity to fp32 log-mel rows, not a front-end error, so TAU_STREAM stays."""
    pcm, want, want64 = stream_ref(name)
    for full in (False, True):
        posts = _run_bank(engines[name], pcm, full_recompute=full)
        _stream_post(f"{name} stream bank full_recompute={full}", posts, want, want64, TAU_STREAM)


BF16_BANKS = {"Wavenet": [("one launch", {}), ("two launches, waited", dict(two_launch=True, sync_wait=True)),
                          ("full_recompute", dict(full_recompute=True))],
              "CRNN": [("default", {}), ("full_recompute", dict(full_recompute=True))]}


@pytest.mark.parametrize("name", ["CRNN", "Wavenet"])
def test_stream_bank_bf16x3_vs_float64(assets, engines, stream_ref, name):
    """The stream banks of a precision="bf16x3" engine on test_stream_bank_vs_float64's streams and references.  Wavenet: the default
    one-launch tick (the bf16x3 tick kernel), the two-launch form waited for, and a full_recompute bank.  CRNN: the default bank -
    its incremental kernel is fp32 by design, so it is held to the fp32 banks' TAU_STREAM - and a full_recompute bank (the fused
    bf16 kernel).  Every figure is printed before anything is asserted.  Measured, against the C oracle's rows / against
    Ref64.logmel rows: Wavenet tau 3.61e-5 / 3.57e-5 in all three forms (max|dp| 7.7e-7); CRNN full_recompute 5.15e-5 / 4.94e-5
    (max|dp| 1.6e-5); CRNN default 7.56e-5 / 6.14e-5 - the fp32 banks' figures, as it is their kernel.  TAU_STREAM_BF16 is four times
    the worst of the bf16 kernels' figures.
    Without a tolerance: the Wavenet's one-launch and two-launch banks give the same bits on this input, and the CRNN's default
    bank gives the bits of the fp32 engine's default bank."""
    from wwhip.engine import Engine
    pcm, want, want64 = stream_ref(name)
    e = Engine(os.path.join(assets, name), precision="bf16x3")
    try:
        posts = {form: _run_bank(e, pcm, **flags) for form, flags in BF16_BANKS[name]}
    finally:
        e.close()
    flat = lambda ps, which: np.concatenate([ps[s] for s in which])
    for form, ps in posts.items():
        for s in range(STREAM_S):
            assert len(ps[s]) == len(want[s]), (form, s)
        for what, which, w in (("the C oracle's rows", range(STREAM_S), want), ("Ref64.logmel rows", list(want64), want64)):
            g, w64 = flat(ps, which), flat(w, which)
            print(f"\nREF64 {name} bf16x3 stream bank, {form}, against {what}: needs tau {R.needed_tau(g[:, None], w64[:, None]):.2e}, "
                  f"max|dp| {np.abs(g - w64).max():.2e}", end="")
    for form, ps in posts.items():
        tau = TAU_STREAM if (name, form) == ("CRNN", "default") else TAU_STREAM_BF16
        _stream_post(f"{name} bf16x3 stream bank, {form}", ps, want, want64, tau)
    if name == "Wavenet":
        assert posts["one launch"] == posts["two launches, waited"]
    else:
        assert posts["default"] == _run_bank(engines[name], pcm)
