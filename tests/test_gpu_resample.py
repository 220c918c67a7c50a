"""The resampler's kernels (csrc/resample.hip) through Resampler / StreamResampler / load and the C ABI, against the float64
statement of tests/resample64.py.

The error bound is derived, not measured: an output is a tpp-term fp32 fmaf chain over taps rounded once from float64, so
|y - y64| <= (tpp + 2) * 2^-24 * A[m], A[m] = sum |h| |x| - the running-error bound of a tpp-term fp32 sum in any order plus
one rounding per tap.  Everything that says "same bits" is assert_array_equal."""
import ctypes as C
import os
import sys
import wave

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resample64 as R64  # noqa: E402

pytestmark = pytest.mark.gpu

RATES = R64.RATES
U = 2.0 ** -24
_CACHE = {}


def _pcm(rng, n, rate):
    t = np.arange(n) / float(rate)
    chirp = 8000.0 * np.sin(2 * np.pi * (200.0 * t + 0.5 * 3800.0 / 1.5 * np.mod(t, 1.5) * np.mod(t, 1.5)))
    return np.clip(np.rint(rng.normal(0, 2000, n) + chirp), -32768, 32767).astype(np.int16)


def _square(n):
    return np.where((np.arange(n) // 37) % 2 == 0, 32767, -32768).astype(np.int16)


def _cases(rate):
    """Per rate, built once: int16 and float32 clips with their float64 outputs and bound sums."""
    if rate in _CACHE:
        return _CACHE[rate]
    up, down, half, _ = R64.design(rate)
    rng = np.random.default_rng(rate)
    lengths = [1, 2, 3, down - 1, down, down + 1, 1000, 16001]
    i16 = [_pcm(rng, n, rate) for n in lengths] + [np.zeros(1000, np.int16), _square(16001)]
    f32 = [(_pcm(rng, n, rate).astype(np.float32) / np.float32(32768.0)) * np.float32(0.999) for n in lengths] + [np.zeros(1000, np.float32)]
    if rate in (48000, 44100):
        i16.append(_pcm(rng, 160000, rate))
    c = {"up": up, "down": down, "half": half, "tpp": R64.tpp(up, half), "i16": i16, "f32": f32, "silent": {"i16": 8, "f32": 8}}
    for k in ("i16", "f32"):
        c[k + "_y"] = [R64.resample(x, rate) for x in c[k]]
        c[k + "_A"] = [R64.bound_sum(x, rate) for x in c[k]]
    _CACHE[rate] = c
    return c


@pytest.fixture(scope="module")
def rs():
    from wwhip.resample import Resampler
    made = {r: Resampler(r, 16000) for r in RATES}
    yield made
    for r in made.values():
        r.close()


@pytest.fixture(scope="module")
def batch(rs):
    """Every rate's cases through ONE ragged call per sample format (computed once, shared)."""
    out = {}
    for r in RATES:
        c = _cases(r)
        out[r] = {k: rs[r](c[k], np.float32) for k in ("i16", "f32")}
    return out


@pytest.mark.parametrize("rate", RATES)
def test_against_float64_within_the_derived_bound(rs, batch, rate):
    c = _cases(rate)
    assert (rs[rate].up, rs[rate].down, rs[rate].half, rs[rate].taps_per_output) == (c["up"], c["down"], c["half"], c["tpp"])
    worst = 0.0
    for k in ("i16", "f32"):
        for x, y, y64, A in zip(c[k], batch[rate][k], c[k + "_y"], c[k + "_A"]):
            assert y.dtype == np.float32 and y.shape == y64.shape == (rs[rate].out_len(len(x)),)
            bound = (c["tpp"] + 2) * U * A
            err = np.abs(y.astype(np.float64) - y64)
            used = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
            worst = max(worst, used)
            assert (err <= bound).all(), (rate, k, len(x), used)
        assert not batch[rate][k][c["silent"][k]].any() and batch[rate][k][c["silent"][k]].shape == (rs[rate].out_len(1000),)
    print(f"{rate}: worst used fraction of (tpp + 2) 2^-24 A = {worst:.3f}")


def test_equal_rates_are_the_input_bit_for_bit():
    from wwhip.resample import Resampler
    r = Resampler(16000, 16000)
    c = _cases(48000)
    for x, y in zip(c["i16"][:10], r(c["i16"][:10])):
        np.testing.assert_array_equal(y, x.astype(np.float32) / np.float32(32768.0))
    for x, y in zip(c["f32"], r(c["f32"])):
        np.testing.assert_array_equal(y, x)
    np.testing.assert_array_equal(r(c["i16"][7], np.int16), c["i16"][7])
    assert (r.up, r.down, r.half, r.table_bytes) == (1, 1, 0, 0)
    r.close()


@pytest.mark.parametrize("rate", RATES)
def test_a_clip_alone_has_the_bits_it_has_in_a_ragged_batch(rs, batch, rate):
    c = _cases(rate)
    for k in ("i16", "f32"):
        for x, y in zip(c[k], batch[rate][k]):
            np.testing.assert_array_equal(rs[rate](x), y)


@pytest.mark.parametrize("rate", (48000, 44100))
def test_pieces_with_exact_history_are_the_one_shot(rs, batch, rate):
    c, r = _cases(rate), rs[rate]
    x, one = c["i16"][-1], batch[rate]["i16"][-1]
    assert len(x) == 160000
    up, down, half = c["up"], c["down"], c["half"]
    hist = -(-half // up)
    cuts = [0, 1, 17771, 40960 + 3, len(one)]
    segs, i0, o0, cnt = [], [], [], []
    for a, b in zip(cuts[:-1], cuts[1:]):
        k0 = max(0, a * down // up - hist)                      # exactly ceil(half / up) samples of history
        k1 = min(len(x), ((b - 1) * down + half) // up + 1)     # up to the last sample the piece's last output reads
        segs.append(x[k0:k1]); i0.append(k0); o0.append(a); cnt.append(b - a)
    np.testing.assert_array_equal(np.concatenate(r.ranges(segs, i0, o0, cnt)), one)
    for s, a, b, n in zip(segs, i0, o0, cnt):                   # and each piece in a call of its own
        np.testing.assert_array_equal(r.range(s, a, b, n), one[b:b + n])


@pytest.mark.parametrize("rate", RATES)
def test_stream_packets_are_the_one_shot(rs, batch, rate):
    from wwhip.resample import StreamResampler, determined
    c = _cases(rate)
    x, one = c["i16"][7], batch[rate]["i16"][7]                 # 16,001 samples
    up, down, half = c["up"], c["down"], c["half"]
    st = StreamResampler(rate, 16000)
    rng = np.random.default_rng(3)
    # a run of single samples across the input position at which the first output of the second tile is determined
    edge_out = 1792 if up == 1 else 256
    edge_in = (edge_out * down + half) // up
    sizes, pos = [0], 0
    while pos < len(x):
        if edge_in - 20 <= pos < edge_in + 20:
            k = 1
        else:
            k = int(rng.choice([0, 1, int(rng.integers(1, 5001))], p=[0.1, 0.1, 0.8]))
            if pos < edge_in - 20:
                k = min(k, edge_in - 20 - pos)
        sizes.append(k)
        pos += k
    sizes.append(0)
    assert 0 in sizes and sizes.count(1) >= 40
    got, pos = [], 0
    for k in sizes:
        got.append(st.push(x[pos:pos + k]))
        pos = min(pos + k, len(x))
        assert st.n_out == determined(pos, up, down, half)
    got.append(st.flush())
    np.testing.assert_array_equal(np.concatenate(got), one)
    st.close()


@pytest.mark.parametrize("rate", (48000, 44100, 8000))
def test_int16_output_is_the_rounded_float_output(rs, batch, rate):
    c = _cases(rate)
    for x, y in zip(c["i16"], batch[rate]["i16"]):
        want = np.clip(np.rint(y * np.float32(32768.0)), -32768, 32767).astype(np.int16)
        np.testing.assert_array_equal(rs[rate](x, np.int16), want)
    sq = batch[rate]["i16"][9]
    assert np.abs(sq).max() > 1.0                               # the full-scale square wave overshoots: the clip is exercised


@pytest.mark.parametrize("rate", (48000, 44100))
def test_tones_through_the_kernel(rs, rate):
    up, down, half, _ = R64.design(rate)
    x = R64.tones(rate, rate // 4, 8000.0).astype(np.float32)
    y = rs[rate](x)
    want = R64.tones(16000, len(y), 8000.0)
    A = R64.bound_sum(x, rate)
    edge = -(-half // down) + 1
    err = np.abs(y.astype(np.float64) - want)[edge:len(y) - edge]
    print(f"{rate}: tone error through the kernel = {err.max():.2e}")
    assert (err <= 1e-7 + (R64.tpp(up, half) + 2) * U * A[edge:len(y) - edge]).all()


@pytest.mark.parametrize("rate", (48000, 44100))
def test_into_the_front_end(rs, assets, rate):
    from wwhip.models import engine_for
    eng = engine_for(os.path.join(assets, "CRNN_softmax"))
    x = _pcm(np.random.default_rng(9), 3 * rate + 123, rate)
    got = eng.logmel([rs[rate](x)])[0]
    want = eng.logmel([R64.resample(x, rate).astype(np.float32)])[0]
    err = float(np.abs(got - want).max())
    print(f"{rate}: log-mel of the kernel's samples vs of the float64 samples: {err:.2e}")
    assert got.shape == want.shape and got.shape[0] > 290 and err <= 1e-4


def _write_wav(path, pcm, rate, channels=1):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(channels)
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(np.ascontiguousarray(pcm, np.int16).tobytes())


def test_into_the_evaluator(tmp_path, assets):
    from test_gpu_dropin import TOL
    from wwhip import resample as RS
    from wwhip.evaluate import get_posterior
    from wwhip.io import WavInput
    rng = np.random.default_rng(21)
    files, ref = [], {}
    for i, (n, ch) in enumerate(((2 * 48000 + 11, 1), (3 * 48000 - 7, 2), (120000, 1))):
        pcm = np.stack([_pcm(rng, n, 48000) for _ in range(ch)], axis=1)
        p = str(tmp_path / f"c{i}.wav")
        _write_wav(p, pcm, 48000, ch)
        files.append(p)
        mono = pcm[:, 0].astype(np.float64) / 32768.0 if ch == 1 else (pcm.astype(np.float32).mean(axis=1) / np.float32(32768.0)).astype(np.float64)
        ref[p] = R64.resample(mono, 48000).astype(np.float32)
    mdir = os.path.join(assets, "CRNN_softmax")
    got = np.array(get_posterior(mdir, "CRNN", "false_accepts", files, 20, 16000, loader=RS.load), np.float32)
    want = np.array(get_posterior(mdir, "CRNN", "false_accepts", files, 20, 16000, loader=lambda p: ref[p]), np.float32)
    err = float(np.abs(got - want).max())
    print(f"posteriors of 48 kHz wavs, kernel vs float64 resampling: {len(got)} windows, max difference {err:.2e}")
    assert len(got) == len(want) > 100 and err < TOL
    for p in files:
        assert RS.load(p).dtype == np.float32 and RS.load(p).shape == ref[p].shape
    with pytest.raises(ValueError):
        get_posterior(mdir, "CRNN", "false_accepts", files, 20, 16000)
    # the streaming input stage: converted once at open, delivered as 20 ms int16 frames
    x = np.frombuffer(wave.open(files[0], "rb").readframes(10 ** 9), np.int16)
    one = RS.Resampler(48000)(x, np.int16)
    assert len(one) == -(-len(x) // 3)
    wi = WavInput(files[0], resample=True)
    frames = [wi.read() for _ in range(-(-len(one) // 320))]
    assert all(f.dtype == np.int16 and f.shape == (320,) for f in frames)
    np.testing.assert_array_equal(np.concatenate(frames)[:len(one)], one)
    assert not np.concatenate(frames)[len(one):].any()
    with pytest.raises(ValueError):
        WavInput(files[0])


def test_refusals_and_degenerate_sizes_through_ctypes():
    from wwhip import _lib
    lib, ctx = _lib.load(), _lib.default_context()
    EINVAL, OK = _lib.WW_EINVAL, _lib.WW_OK

    def create(ri, ro, params=None):
        h = C.c_void_p()
        return lib.ww_resampler_create(ctx.handle, ri, ro, params, C.byref(h)), h

    def msg():
        return (lib.ww_last_error(ctx.handle) or b"").decode()

    for ri, ro in ((0, 16000), (-48000, 16000), (48000, 0)):
        rc, h = create(ri, ro)
        assert rc == EINVAL and not h.value and "positive" in msg()
    rc, h = create(44101, 16000)                                # ~3 M taps
    assert rc == EINVAL and not h.value and "WW_RESAMPLE_MAX_TAPS" in msg() and "1048576" in msg()
    assert lib.ww_resampler_create(ctx.handle, 48000, 16000, None, None) == EINVAL
    for a, b in [(a, b) for a in (8000, 11025, 16000, 22050, 24000, 32000, 44100, 48000, 88200, 96000, 176400, 192000) for b in (8000, 11025, 192000)]:
        rc, h = create(a, b)                                    # the standard rates against the extreme ones all fit
        assert rc == OK, (a, b, msg())
        assert lib.ww_resampler_destroy(h) == OK
    rc, r = create(48000, 16000)
    assert rc == OK
    info = _lib.ResampleInfo()
    assert lib.ww_resampler_info(r, C.byref(info)) == OK and (info.up, info.down, info.half, info.taps_per_output) == (1, 3, 102, 205)
    assert info.table_bytes == 205 * 4 and lib.ww_resampler_info(r, None) == EINVAL and lib.ww_resampler_info(None, C.byref(info)) == EINVAL

    x = _pcm(np.random.default_rng(4), 3000, 48000)
    want = np.empty(1000, np.float32)
    so, oo = np.array([0, 3000], np.int64), np.array([0, 1000], np.int64)
    rc2, fresh = create(48000, 16000)
    assert lib.ww_resample(fresh, _lib.ptr(x), 0, _lib.ptr(so), None, None, _lib.ptr(oo), 1, _lib.ptr(want), 1) == OK
    lib.ww_resampler_destroy(fresh)

    def call(in_=x, in_fmt=0, so_=so, i0=None, o0=None, oo_=oo, n=1, out_fmt=1, out_null=False):
        y = np.full(1000, -7.0, np.float32)
        rc = lib.ww_resample(r, None if in_ is None else _lib.ptr(in_), in_fmt, None if so_ is None else _lib.ptr(so_),
                             None if i0 is None else _lib.ptr(i0), None if o0 is None else _lib.ptr(o0), None if oo_ is None else _lib.ptr(oo_), n,
                             None if out_null else _lib.ptr(y), out_fmt)
        return rc, y

    def refused(**kw):
        rc, y = call(**kw)
        assert rc == EINVAL and msg() and (y == -7.0).all(), kw  # refused with a message, nothing written
        rc, y = call()                                           # and the object is as good as new
        assert rc == OK
        np.testing.assert_array_equal(y, want)

    refused(n=-1)
    refused(in_=None)
    refused(out_null=True)
    refused(so_=None)
    refused(oo_=None)
    refused(in_fmt=2)
    refused(out_fmt=-1)
    refused(so_=np.array([3000, 0], np.int64))                   # descending
    refused(oo_=np.array([1000, 0], np.int64))
    refused(so_=np.array([-1, 2999], np.int64))
    refused(oo_=np.array([0, 1001], np.int64))                   # one output beyond ceil(3000 / 3)
    refused(o0=np.array([1], np.int64))                          # the same range, shifted beyond the end
    refused(i0=np.array([-1], np.int64))
    refused(o0=np.array([-1], np.int64))
    assert lib.ww_resample(None, _lib.ptr(x), 0, _lib.ptr(so), None, None, _lib.ptr(oo), 1, _lib.ptr(want), 1) == EINVAL
    # n = 0 and empty segments: WW_OK, nothing written
    rc, y = call(n=0)
    assert rc == OK and (y == -7.0).all()
    rc, y = call(n=0, in_=None, so_=None, oo_=None, out_null=True)
    assert rc == OK
    rc, y = call(so_=np.array([5, 5], np.int64), oo_=np.array([9, 9], np.int64))
    assert rc == OK and (y == -7.0).all()
    rc, y = call(so_=np.array([0, 0, 3000, 3000], np.int64), oo_=np.array([0, 0, 1000, 1000], np.int64), n=3)   # empty, whole, empty
    assert rc == OK
    np.testing.assert_array_equal(y, want)
    rc, y = call(so_=np.array([0, 3000], np.int64), oo_=np.array([100, 100], np.int64))                        # samples, no outputs
    assert rc == OK and (y == -7.0).all()
    rc, y = call(so_=np.array([0, 300], np.int64), oo_=np.array([200, 300], np.int64))                         # the untouched rest keeps its sentinel
    assert rc == OK and (y[:200] == -7.0).all() and (y[300:] == -7.0).all() and not (y[200:300] == -7.0).any()
    assert lib.ww_resampler_destroy(r) == OK and lib.ww_resampler_destroy(None) == OK
