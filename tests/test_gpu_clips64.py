"""The clip path (``ww_clips_forward_dev``: PCM -> log-mel -> one zero-padded window per clip -> encode + detect) against float64
in logit space, and against the library's own two-step path bit for bit, at the clip lengths and front-end settings where its
own logic has edges: the equal-clips row -> clip lookup of logmel_rows_kernel (magic multiply from four frames on, plain divide
below, 64-bit form under generic staging or >= 0x7fff0000 samples) and the window hand-over (no frame at all, exactly ``window``
frames, more than ``window``).  Geometries, clip sets and the reference: tests/clips64.py, pinned on the CPU by
tests/test_clips64.py.

Every clip call writes into an output tensor pre-filled with -1 and the result is checked finite.  Each float64 case prints the tau
it needed (``pytest -s``); every tau below is about 4x the worst measured on an MI355X, quoted in the test's docstring."""
import ctypes as C
import os

import numpy as np
import pytest

import clips64 as K
from oracle import ref64 as R

pytestmark = pytest.mark.gpu

TOL_POST = 1e-4          # the absolute rule of tests/test_gpu_parity.py, kept
TAU_STREAM = 3e-4        # tests/test_gpu_ref64.py: the same composition on the streaming path; TAU_CLIP must not exceed it
TAU_CLIP = 1.6e-4        # fp32 posteriors, precise front end (measured 4.0e-5: CRNN, geometry n)
TAU_CLIP_BF16 = 2.4e-4   # precision="bf16x3" (measured 5.9e-5: CRNN, geometry i-24001)
TAU_CLIP_FAST = 2.9e-4   # fp32 models behind the fp32-FFT front end, precise = 0 (measured 7.3e-5: CRNN, o-993); the contract
                         # there is TOL_POST (test_fp32_frontend_mode_meets_posterior_tolerance), the logit tau is on record
assert TAU_CLIP <= TAU_STREAM

ENGINES = [("CRNN", "fp32"), ("Wavenet", "fp32"), ("CRNN_softmax", "fp32"), ("CRNN", "bf16x3"), ("Wavenet", "bf16x3"),
           ("CRNN_old", "fp32")]
SPOT = ["e", "h", "i-24001"]   # the geometries of the models that ride along

# (model, precision, geometry) of the float64 cases; the bit-equality cases add CRNN_old (generic kernels)
CASES64 = ([(m, "fp32", g) for m in ("CRNN", "Wavenet") for g in K.GEOMETRY_IDS]
           + [(m, p, g) for m, p in (("CRNN_softmax", "fp32"), ("CRNN", "bf16x3"), ("Wavenet", "bf16x3")) for g in SPOT])
CASES_EQ = CASES64 + [("CRNN_old", "fp32", g) for g in ("e", "h")]


def _id(case):
    return "-".join(case)


@pytest.fixture(scope="module")
def engines(assets):
    from wwhip.engine import Engine
    out = {(m, p): Engine(os.path.join(assets, m), precision=p) for m, p in ENGINES}
    yield out
    for e in out.values():
        e.close()


@pytest.fixture(scope="module")
def refs(assets, engines):
    """Clip sets and float64 posteriors, one evaluation per (model, samples, front end) for the whole module."""
    from oracle.cpu import CpuOracle
    names = sorted({m for m, _ in ENGINES})
    return K.ClipRefs({m: CpuOracle(engines[(m, "fp32")].blob) for m in names}, {m: R.Ref64(os.path.join(assets, m)) for m in names})


def _fp(geo):
    from wwhip.engine import frontend_params
    return frontend_params(*geo[1:])


def _clips_forward(e, clips, geo):
    """``clips_forward_dev`` on the clips ``[B, samples]`` (a host array or a CUDA tensor): detect rows ``[B, n_out]``."""
    import torch
    d = clips if isinstance(clips, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(clips, np.int16)).cuda()
    assert d.is_contiguous() and d.dtype == torch.int16 and d.shape[1] == geo[0]
    B = d.shape[0]
    out = torch.full((B, e.n_out), -1.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    e.clips_forward_dev(d.data_ptr(), B, geo[0], out.data_ptr(), _fp(geo))
    e.ctx.synchronize()
    got = out.cpu().numpy()
    assert np.isfinite(got).all() and (got >= 0.0).all() and (got <= 1.0).all(), "rows left unwritten or not posteriors"
    return got


def _two_step(e, clips, geo):
    """The same clips through ``Engine.logmel`` (ww_logmel: offset tables) and ``Engine.forward`` on the padded windows."""
    mels = e.logmel(list(clips), _fp(geo))
    nf = K.num_frames(geo[0], geo[4])
    assert all(m.shape == (nf, 40) for m in mels)
    return e.forward(K.pad_windows(mels, e.window))


def _post(case, got, want64, tau):
    got = np.asarray(got, np.float64).reshape(np.shape(want64))
    print(f"\nREF64 {case}: posterior needs tau {R.needed_tau(got, want64):.2e} (tau {tau:g}), "
          f"max|dp| {np.abs(got - want64).max():.2e}", end="")
    ratio = R.check_posteriors(got, want64, tau)
    assert np.abs(got - want64).max() < TOL_POST, case
    return ratio


# ---------------------------------------------------------------- a. float64, logit space
@pytest.mark.parametrize("case", CASES64, ids=_id)
def test_clips_vs_float64(engines, refs, case):
    """The whole clip set (16 - 24 clips) of a geometry in one call against Ref64.logmel -> window -> Ref64.forward.
    Measured needed tau, worst geometry of each group - fp32, precise front end: CRNN 4.0e-5 (n; 2.8e-5 .. 3.4e-5 at every
    other geometry of 46 frames or more, 7.8e-7 .. 8.9e-6 up to 20 frames), Wavenet 5.3e-6 (l), CRNN_softmax 1.4e-5 (h); bf16x3: CRNN
    5.9e-5 (i-24001), Wavenet 4.7e-5 (e, h); precise = 0: CRNN 7.3e-5 (o-993), Wavenet 2.5e-5 (o-993), max|dp| 5.8e-6 (CRNN,
    o-24001) against the 1e-4 contract.  The CRNN's tau is its sensitivity to fp32 log-mel rows (tests/test_gpu_ref64.py,
    test_stream_bank_vs_float64: 6.2e-5 on the streaming path), not a front-end error; no geometry stands out."""
    name, precision, gid = case
    e = engines[(name, precision)]
    geo = K.geometry(gid, e.window)
    got = _clips_forward(e, refs.clips(name, gid), geo)
    tau = TAU_CLIP_BF16 if precision == "bf16x3" else TAU_CLIP if geo[5] else TAU_CLIP_FAST
    _post(f"{name} {precision} clips {gid} ({geo[0]} samples, {K.num_frames(geo[0], geo[4])} frames)", got, refs.want64(name, gid), tau)


# ---------------------------------------------------------------- b. bit-equality with the two-step path
@pytest.mark.parametrize("case", CASES_EQ, ids=_id)
def test_clips_equal_logmel_then_forward(engines, refs, case):
    """clips_forward_dev on B clips equals Engine.forward on the windows built from Engine.logmel of the same B clips, bit for
    bit, for B = 1, 2, 7 and the whole set: the equal-clips arithmetic against ww_logmel's offset tables, and the hand-over
    (hop = nf, valid = min(nf, T), nothing written at nf = 0) against explicit zero-padded windows.  Both sides run the same
    kernels on the same rows at every geometry, so nothing is held to a tolerance here."""
    name, precision, gid = case
    e = engines[(name, precision)]
    geo = K.geometry(gid, e.window)
    clips = refs.clips(name, gid)
    for B in (1, 2, 7, len(clips)):
        np.testing.assert_array_equal(_clips_forward(e, clips[:B], geo), _two_step(e, clips[:B], geo), err_msg=f"{_id(case)} B={B}")


# ---------------------------------------------------------------- c. batch invariance
@pytest.mark.parametrize("gid", ["c", "f", "h", "i-24001", "i-993"])
@pytest.mark.parametrize("name", ["CRNN", "Wavenet"])
def test_clips_batch_invariance(engines, refs, name, gid):
    """A clip alone, the set permuted and the set in chunks of 5 give the bits of the whole set."""
    e = engines[(name, "fp32")]
    geo = K.geometry(gid, e.window)
    clips = refs.clips(name, gid)
    n = len(clips)
    whole = _clips_forward(e, clips, geo)
    for i in (0, n // 2, n - 1):
        np.testing.assert_array_equal(_clips_forward(e, clips[i:i + 1], geo), whole[i:i + 1])
    perm = np.random.default_rng(97).permutation(n)
    assert (perm != np.arange(n)).any()
    np.testing.assert_array_equal(_clips_forward(e, clips[perm], geo), whole[perm])
    chunks = np.concatenate([_clips_forward(e, clips[i:i + 5], geo) for i in range(0, n, 5)])
    np.testing.assert_array_equal(chunks, whole)


# ---------------------------------------------------------------- d, e. the largest call: 65,535 clips
@pytest.fixture()
def own_crnn(assets):
    """A CRNN on a context of its own: what the large calls make the context's arena grow to goes away with it, and the
    offset-table cache starts empty."""
    from wwhip import _lib
    from wwhip.engine import Engine
    ctx = _lib.Context(0)
    e = Engine(os.path.join(assets, "CRNN"), ctx=ctx)
    yield e
    e.close()
    ctx.close()


def test_magic_multiply_at_high_row_indices(engines, refs, own_crnn):
    """Geometry c (993 samples, 4 frames: the smallest clip on the magic multiply) at 65,535 clips tiled from 16: mel rows up to
    262,139 through __umulhi(row, magic) >> shift.  Row i has the bits of row i mod 16 of the 16-clip call (the large call runs
    the CRNN's front + tail kernels, the small one the fused kernel: the project holds those to the same bits)."""
    geo = K.geometry("c", 151)
    clips = refs.clips("CRNN", "c")
    small16 = clips[clips.any(axis=1)][:16]          # (the stream's silent stretches give all-zero clips, which share a row)
    assert len(small16) == 16
    small = _clips_forward(engines[("CRNN", "fp32")], small16, geo)
    assert len({r.tobytes() for r in small}) == 16   # sixteen distinct rows: a clip read from the wrong place shows
    n = 65535
    big = _clips_forward(own_crnn, np.tile(small16, (4096, 1))[:n], geo)
    np.testing.assert_array_equal(big, small[np.arange(n) % 16])


def test_sample_indices_past_2_to_31(engines, refs, own_crnn):
    """65,535 clips of 32,784 samples (202 frames) = 2,148,499,440 samples >= 0x7fff0000: the front end's [simple, !small]
    instance, whose sample indices are 64-bit and pass 2^31.  The PCM is tiled on the device from 16 distinct clips; needs about
    7 GB of HBM (4.3 GB of PCM, 2.1 GB of mel workspace).  Every row has the bits of row i mod 16 of the 16-clip call."""
    import torch
    n, samples = 65535, 32784
    assert n * samples >= 0x7fff0000
    geo = (samples,) + K.DEFAULT + (True,)
    small16 = K.clip_set(refs.oracles["CRNN"], samples)[:16]
    assert len(small16) == 16
    small = _clips_forward(engines[("CRNN", "fp32")], small16, geo)
    assert len({r.tobytes() for r in small}) == 16
    d = torch.from_numpy(small16).cuda().repeat(4096, 1)[:n]
    try:
        big = _clips_forward(own_crnn, d, geo)
    finally:
        del d
        torch.cuda.empty_cache()
    np.testing.assert_array_equal(big, small[np.arange(n) % 16])


# ---------------------------------------------------------------- f. the offset-table cache
def test_offset_table_cache_eviction(engines, refs, own_crnn):
    """ww_clips_forward_dev keeps the offset tables of eight (n_clips, samples, hop) geometries per context.  Ten geometries in
    order, twice, then the first again: from the ninth call on every call evicts the oldest entry and builds its own anew.
    Every call's output equals the same geometry's first output, which equals the module engine's (another context)."""
    geos = [(4, 400, 160), (5, 832, 160), (6, 993, 160), (3, 3553, 160), (7, 993, 160), (4, 700, 1), (3, 12001, 80),
            (2, 24001, 200), (2, 24001, 512), (5, 832, 80)]
    assert len(set(geos)) == 10
    ora = refs.oracles["CRNN"]
    first = {}
    for k in list(range(10)) * 2 + [0]:
        n, samples, hop = geos[k]
        geo = (samples, 32767.0, True, 0.0, hop, True)
        clips = K.clip_set(ora, samples)[:n]
        got = _clips_forward(own_crnn, clips, geo)
        if k not in first:
            first[k] = got
            np.testing.assert_array_equal(got, _clips_forward(engines[("CRNN", "fp32")], clips, geo))
        np.testing.assert_array_equal(got, first[k], err_msg=f"geometry {geos[k]}")


# ---------------------------------------------------------------- g. refusals
def test_refusals_and_degenerate_sizes_through_ctypes(engines, refs):
    import torch
    from wwhip import _lib
    from wwhip.engine import frontend_params
    e = engines[("CRNN", "fp32")]
    lib, ctx = _lib.load(), e.ctx
    EINVAL, OK = _lib.WW_EINVAL, _lib.WW_OK
    n, samples = 6, 993
    pcm = refs.clips("CRNN", "c")[:n]
    d = torch.from_numpy(np.concatenate([pcm.ravel(), np.zeros(8, np.int16)])).cuda()   # (room behind for the shifted pointer)
    want = _clips_forward(e, pcm, K.geometry("c", e.window))

    def msg():
        return (lib.ww_last_error(ctx.handle) or b"").decode()

    def call(n_clips=n, n_samples=samples, off=0, fp=frontend_params(), null_pcm=False, null_out=False, null_fp=False):
        out = torch.full((n, e.n_out), -1.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        rc = lib.ww_clips_forward_dev(ctx.handle, e.handle, None if null_pcm else C.c_void_p(d.data_ptr() + off), n_clips, n_samples,
                                      None if null_fp else C.byref(fp), None if null_out else C.c_void_p(out.data_ptr()))
        ctx.synchronize()
        return rc, out.cpu().numpy()

    def refused(**kw):
        rc, y = call(**kw)
        assert rc == EINVAL and msg() and (y == -1.0).all(), kw   # refused with a message, nothing written
        rc, y = call()                                             # and the next valid call gives the bits it gave before
        assert rc == OK
        np.testing.assert_array_equal(y, want)

    refused(n_clips=65536)
    refused(n_clips=-1)
    refused(n_samples=-1)
    refused(off=2)                                   # d_pcm 2 bytes off 16-byte alignment
    refused(fp=frontend_params(hop=0))
    refused(fp=frontend_params(hop=513))
    refused(fp=frontend_params(pcm_divisor=0.0))
    refused(null_out=True)
    refused(null_pcm=True)
    refused(null_fp=True)
    rc, y = call(n_clips=0)
    assert rc == OK and (y == -1.0).all()
    rc, y = call()
    assert rc == OK
    np.testing.assert_array_equal(y, want)
