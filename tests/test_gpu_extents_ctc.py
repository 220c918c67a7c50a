"""The CTC lattice calls, the stream ticks and the resampler read and write only what their contract names (include/wwhip.h), on
the MI355X.  Sections E and F of tests/test_gpu_extents.py's list; the harness is tests/extents.py, and section E's layouts and
assertions are tests/extents_ctc.py's, which tests/test_extents.py runs over the host functions of csrc/ctc_*.h first.

  E  lattice calls   ww_ctc_{score,align,occupancy}_dev at P = 4, 8, 16, 32 (Umax = 1, 3, 7, 9; K = 3 targets of mixed lengths), n = 45
                     sequences (135 pairs: a partial last workgroup of 7 live segments at every P), T = 1, 2, 9, 10, 19, 64, L = 2, 4, 8,
                     both modes; ww_ctc_beam_dev at W = 1, 8, 64 and top_paths = 1, min(W, 8) (T <= 19: the call refuses more);
                     ww_ctc_greedy_dev; one case each of ww_ctc_{score,align,beam,occupancy}_windows_dev
  F  ticks           ww_stream_step, ww_stream_step_ctc, _ctc_score, _ctc_align, _ctc_beam with every host array between guards
     resampler       ww_resample_dev on a ragged call, int16 / float32 / mu-law, 48 kHz -> 16 kHz and 8 kHz -> 16 kHz

E, per (call, P, T, L, mode).  Guards: ``d_steps`` between guards of NaN, 1e30, 0.0 (64 sequences wide) - the three runs give the
same bits; every output (``d_score``; ``d_value``, ``d_span``; ``d_occ``, ``d_cls`` given and NULL; the beam's three) between
sentinel guards that keep every byte.  Poisoned sequences: sequences 0 and n - 1, the sequences whose pairs own the last segment of
a 16-lane row, of a wave and of a workgroup and the first segment of the next, and one with a clean segment right below it
(``extents_ctc.check_edges`` asserts that the set is that) hold NaN, then 1e30, then 0.0 in every element; every other sequence
keeps the 0.0 guard run's bits.  With sequence n - 1 poisoned the grid's dead segments repeat poisoned work: the back guards and
sequence n - 2 decide that they store nothing.  The 0.0 run is the host function's (``ww_ctc_*_rows``), bit for bit - the contract
of tests/test_gpu_ctc_*.py; no tolerance is introduced here.

F.  Every host array of a tick is a ``Guarded(device=False)``; the output guards are intact after every one of 25 ticks, and at
S = 3 stream 1's outputs over all ticks are the same bits whether streams 0 and 2 and the frames' guards hold a full-scale square or
zeros.  The resampler's input guards hold a square, then zeros (float32: NaN, 1e30, 0.0), its output lies between sentinel guards
wider than an output tile, all runs have the same bits, and the 0.0 run is within tests/test_gpu_resample.py's derived bound
``(tpp + 2) 2^-24 A[m]`` of float64.

No address handed to the library lies outside an allocation of the test's, guards included; nothing here is expected to fault.

Measured on an MI355X (``pytest -s``; T = 19, L = 4).  Every case passed as the kernels stood: no leak between pairs, no store by a
dead segment, no fix needed.  The cases can fail: a build of the library, made aside and not kept, whose score and occupancy
kernels multiply what the shift by 2 brought by a 0 mask where they select, failed ``test_lattice_calls`` under the NaN poison at
P = 4 and P = 8 (``score P=8 T=9 L=2 exact``: 3 of 120 clean scores NaN) and nowhere else - at P = 16 a segment is a whole DPP row,
whose shifts bring 0 across its edge, and at P = 32 a segment's 13 idle lanes keep a shift by 2 inside it.  A poisoned sequence's own rows: the score and the occupancy's ``value`` are NaN under the NaN poison and
Inf under 1e30 at every P and in both modes; the alignment's ``value`` is NaN / Inf in exact mode, and in prefix mode under the NaN
poison it is NaN for U = 1 and 0.0 (no path, spans -1) for longer targets - ``q > Q`` is false for a NaN, the comparison launders
it; the beam's first path is the empty string (length 0) with probability NaN / Inf at every width.  The ticks deliver 47 windows
in 25 ticks in every form.  The resampler's 0.0 runs use 0.046 / 0.041 / 0.041 of the bound at 48 kHz -> 16 kHz (int16 / float32 /
mu-law) and 0.090 / 0.099 / 0.100 at 8 kHz -> 16 kHz."""
import numpy as np
import pytest

import ctc64
import extents as X
import extents_ctc as EC
import geometry64 as G
import resample64 as R64

pytestmark = pytest.mark.gpu

SENT = X.SENTINEL
MEL_GUARD_ROWS = 256       # tests/test_gpu_extents.py: wider than any window


class Lab:
    """The module's engines (one synthetic CTC model per L, the shipped CRNN), each made once."""

    def __init__(self, assets):
        self.assets, self.engines = assets, {}

    def ctc(self, L):
        from wwhip.engine import Engine
        if L not in self.engines:
            self.engines[L] = Engine(f"synthetic-ctc-{L}", bundle=ctc64.reference(L)[0])
        return self.engines[L]

    def crnn(self):
        import os
        from wwhip.engine import Engine
        if "crnn" not in self.engines:
            self.engines["crnn"] = Engine(os.path.join(self.assets, "CRNN"))
        return self.engines["crnn"]

    def close(self):
        for e in self.engines.values():
            e.close()


@pytest.fixture(scope="module")
def lab(assets):
    out = Lab(assets)
    yield out
    out.close()


@pytest.fixture(scope="module")
def host():
    return EC.Backend()


def _same(got: dict, want: dict, what: str) -> None:
    assert got.keys() == want.keys(), (what, sorted(got), sorted(want))
    for k in want:
        X.assert_same_bits(got[k], want[k], f"{what}: {k} against the host function")


# ==================================================================================================== E. the lattice calls
@pytest.mark.parametrize("umax", list(EC.SEGMENT))
@pytest.mark.parametrize("name", ["score", "align", "occupancy"])
def test_lattice_calls(lab, host, name, umax):
    """Per T, L and mode: the guard runs, the poisoned-sequence runs, and the 0.0 run against ``ww_ctc_{name}_rows``.  The occupancy
    in exact mode runs with ``d_cls`` NULL and given (prefix mode refuses a ``cls``); ``value`` and ``occ`` do not depend on it."""
    show = []
    for L in ctc64.LS:
        dev = EC.Backend(lab.ctc(L))
        for T in EC.TS:
            y, targets = EC.lattice_inputs(umax, T, L)
            for mode in EC.MODES:
                say = show if (T, L) == (19, 4) else None
                base = EC.lattice_case(dev, name, umax, T, L, mode, show=say)
                _same(base, EC.lattice_run(host, name, y, targets, mode, "zero"), f"{name} P={EC.SEGMENT[umax]} T={T} L={L} {mode}")
                if name == "occupancy" and mode == "exact":
                    both = EC.lattice_case(dev, name, umax, T, L, mode, want_cls=True, show=say)
                    _same(both, EC.lattice_run(host, name, y, targets, mode, "zero", want_cls=True), f"occupancy with cls P={EC.SEGMENT[umax]} T={T} L={L}")
                    for k in base:
                        X.assert_same_bits(both[k], base[k], f"occupancy T={T} L={L}: {k} with and without cls")
    print("".join(f"\nEXTENTS E {line}" for line in show), end="")


@pytest.mark.parametrize("W", [1, 8, 64])
def test_beam_call(lab, host, W):
    """``ww_ctc_beam_dev`` (a wave per sequence, four to a workgroup: sequences 0, 3, 4 and 44 poisoned; the last workgroup has one live
    wave and three that repeat sequence 44) at T = 1, 2, 9, 10, 19 and ``top_paths`` = 1 and min(W, 8), the most the call accepts."""
    show = []
    for L in ctc64.LS:
        dev = EC.Backend(lab.ctc(L))
        for T in EC.BEAM_TS:
            y, M = EC.beam_inputs(T, L)
            for P in sorted({1, min(W, 8)}):
                base = EC.beam_case(dev, T, L, W, P, show=show if (T, L) == (19, 4) else None)
                _same(base, EC.beam_run(host, y, W, P, M, "zero"), f"beam T={T} L={L} W={W} top_paths={P}")
    print("".join(f"\nEXTENTS E {line}" for line in show), end="")


def test_greedy_call(lab, host):
    """``ww_ctc_greedy_dev`` (a thread per sequence, 64 to a workgroup: n = 70, sequences 0, 63, 64 and 69 poisoned) against
    ``wwhip.ctc.greedy_decode``, the numpy statement of csrc/ctc_decode.h."""
    for L in ctc64.LS:
        dev = EC.Backend(lab.ctc(L))
        for T in EC.TS:
            _same(EC.greedy_case(dev, T, L), EC.greedy_case(host, T, L), f"greedy T={T} L={L}")


# ---- the model forms: one case each ---------------------------------------------------------------------------------------------------
WIN_N, WIN_L, WIN_M = 20, 4, 2
WIN_TAIL_PAIR = (18, 19)     # window 18 (full) and window 19 (100 rows) both end on the body's last row
WIN_TARGETS = [(1, 2), (0,), (2, 2, 1)]
WIN_BEAM = (8, 3, 5)         # beam_width, top_paths, max_labels


class WindowList:
    """20 windows in one mel body as section A lays them out (``extents.window_layout``): 3 to 11 unnamed rows in front of each,
    ``valid`` = T but for windows 3 (0 rows), 7 (1), 11 (T - 1) and 19 (100), windows 18 and 19 ending on the body's last row."""

    def __init__(self, T, F, seed=4800):
        self.T, self.F = T, F
        self.valid = np.full(WIN_N, T, np.int32)
        self.valid[[3, 7, 11, 19]] = [0, 1, T - 1, 100]
        gaps = [3 + (5 * w) % 9 for w in range(WIN_N)]
        self.row, self.rows, self.named = X.window_layout(self.valid, gaps, T, tail_pair=WIN_TAIL_PAIR)
        content = G.windows(seed, WIN_N, T, F)
        self.body = np.zeros((self.rows, F), np.float32)
        for w in range(WIN_N):
            if w != WIN_TAIL_PAIR[1]:
                self.body[self.row[w]:self.row[w] + self.valid[w]] = content[w, :self.valid[w]]
        assert self.row[18] + T == self.rows == self.row[19] + 100 and not self.named.all() and 100 < T


def _window_spec(name, n, L):
    K = len(WIN_TARGETS)
    decode = {"labels": ((n, WIN_M), np.int32), "lengths": ((n,), np.int32)}
    if name == "score":
        return {"score": ((K, n), np.float32), **decode}
    if name == "align":
        return {"value": ((K, n), np.float32), "span": ((K, n, EC.NU, 2), np.int8), **decode}
    if name == "occupancy":
        return {"value": ((K, n), np.float32), "occ": ((K, n, 19, EC.NU), np.float32), "cls": ((K, n, 19, L), np.float32), **decode}
    W, P, M = WIN_BEAM
    return {"labels": ((n, P, M), np.int32), "lengths": ((n, P), np.int32), "prob": ((n, P), np.float32)}


@pytest.mark.parametrize("name", ["score", "align", "occupancy", "beam"])
def test_windows_dev_forms(lab, name):
    """``ww_ctc_{name}_windows_dev``: NaN, 1e30 and 0.0 in every unnamed mel row and in the mel guards give the 0.0 run's bits in
    every output, the decode's ``d_labels`` / ``d_lengths`` included, and every output guard is intact."""
    import torch
    e = lab.ctc(WIN_L)
    lay = WindowList(e.window, e.n_mel)
    mode = "prefix" if name == "score" else "exact"

    def run(poison):
        mel = X.Guarded(X.poison_rows(lay.body, lay.named, poison), poison, width=MEL_GUARD_ROWS * lay.F, device=True)
        d_row, d_valid = torch.from_numpy(np.array(lay.row)).cuda(), torch.from_numpy(np.array(lay.valid)).cuda()
        o = X.guarded_outputs(_window_spec(name, WIN_N, WIN_L), device=True)
        lead = (mel.ptr, lay.rows, d_row.data_ptr(), d_valid.data_ptr(), WIN_N)
        torch.cuda.synchronize()
        if name == "score":
            e.ctc_score_windows_dev(*lead, WIN_TARGETS, mode, o["score"].ptr, WIN_M, o["labels"].ptr, o["lengths"].ptr)
        elif name == "align":
            e.ctc_align_windows_dev(*lead, WIN_TARGETS, mode, o["value"].ptr, o["span"].ptr, WIN_M, o["labels"].ptr, o["lengths"].ptr)
        elif name == "occupancy":
            e.ctc_occupancy_windows_dev(*lead, WIN_TARGETS, mode, o["value"].ptr, o["occ"].ptr, o["cls"].ptr, WIN_M, o["labels"].ptr, o["lengths"].ptr)
        else:
            e.ctc_beam_windows_dev(*lead, *WIN_BEAM, o["labels"].ptr, o["lengths"].ptr, o["prob"].ptr)
        e.ctx.synchronize()
        mel.check_guards(f"{name}_windows_dev ({poison}): mel")
        return X.read_outputs(o, f"{name}_windows_dev ({poison})")
    base = X.poison_runs(run, what=f"{name}_windows_dev")
    main = base["prob" if name == "beam" else "score" if name == "score" else "value"]
    assert np.isfinite(main).all() and main.min() >= 0.0 and main.max() <= 1.0 and (main > 0).any()
    assert (base["lengths"] >= 0).all() and (base["lengths"] <= 19).all()
    print(f"\nEXTENTS E {name}_windows_dev: {np.array2string(main.reshape(-1)[:4], precision=6)}", end="")


# ==================================================================================================== F. ticks
TICKS, TICK_L, TICK_M = 25, 4, 3
TICK_TARGETS = [(1, 2), (0,), (2, 2, 1)]
TICK_BEAM = (8, 3, 5)
TICK_CALLS = ["step", "step_ctc", "step_ctc_score", "step_ctc_align", "step_ctc_beam"]


def _tick_pcm(seed, ticks=TICKS):
    """``[ticks, 320]`` int16: noise and a chirp, a few thousand of amplitude (tests/test_gpu_extents.py: ``_pcm``)."""
    n = ticks * 320
    rng = np.random.default_rng(seed)
    t = np.arange(n) / 16000.0
    return np.clip(np.rint(rng.normal(0, 1500, n) + 4000.0 * np.sin(2 * np.pi * (300.0 + 700.0 * t) * t)), -32768, 32767).astype(np.int16).reshape(ticks, 320)


def _tick_spec(call, S):
    K, (W, P, BM) = len(TICK_TARGETS), TICK_BEAM
    if call == "step":
        return {"post": ((S, 2), np.float32), "n_post": ((S,), np.int32)}
    spec = {"labels": ((S, 2, TICK_M), np.int32), "lengths": ((S, 2), np.int32), "steps": ((S, 2, 19, TICK_L), np.float32)}
    if call in ("step_ctc_score", "step_ctc_align"):
        spec["scores"] = ((S, 2, K), np.float32)
    if call == "step_ctc_align":
        spec.update(align_value=((S, 2, K), np.float32), align_span=((S, 2, K, EC.NU, 2), np.int8))
    if call == "step_ctc_beam":
        spec.update(beam_labels=((S, 2, P, BM), np.int32), beam_lengths=((S, 2, P), np.int32), beam_probs=((S, 2, P), np.float32))
    spec["n_post"] = ((S,), np.int32)
    return spec


def _bank(lab, call, S):
    from wwhip.engine import CtcStreamBank, StreamBank
    if call == "step":
        return StreamBank(lab.crnn(), S)
    kw = {}
    if call in ("step_ctc_score", "step_ctc_align"):
        kw = dict(targets=TICK_TARGETS, mode="prefix", align=call == "step_ctc_align")
    return CtcStreamBank(lab.ctc(TICK_L), S, max_labels=TICK_M, want_steps=True, **kw)


def _tick(bank, call, frames, flags, o):
    from wwhip import _lib
    lib, h, f, s = bank._lib, bank._h, frames.ptr, _lib.ptr(flags)
    if call == "step":
        rc = lib.ww_stream_step(h, f, s, o["post"].ptr, o["n_post"].ptr)
    elif call == "step_ctc":
        rc = lib.ww_stream_step_ctc(h, f, s, TICK_M, o["labels"].ptr, o["lengths"].ptr, o["steps"].ptr, o["n_post"].ptr)
    elif call == "step_ctc_score":
        rc = lib.ww_stream_step_ctc_score(h, f, s, TICK_M, o["labels"].ptr, o["lengths"].ptr, o["steps"].ptr, o["scores"].ptr, o["n_post"].ptr)
    elif call == "step_ctc_align":
        rc = lib.ww_stream_step_ctc_align(h, f, s, TICK_M, o["labels"].ptr, o["lengths"].ptr, o["steps"].ptr, o["scores"].ptr, o["align_value"].ptr,
                                          o["align_span"].ptr, o["n_post"].ptr)
    else:
        rc = lib.ww_stream_step_ctc_beam(h, f, s, TICK_M, o["labels"].ptr, o["lengths"].ptr, o["steps"].ptr, *TICK_BEAM, o["beam_labels"].ptr,
                                         o["beam_lengths"].ptr, o["beam_probs"].ptr, o["n_post"].ptr)
    _lib.raise_for(rc, bank.engine.ctx.handle)


def _tick_run(lab, call, S, me, fill, others):
    """25 ticks of a fresh bank: stream ``me`` gets the test signal, the other streams ``others`` ("zero" / "square"), the frames'
    guards hold ``fill``.  Every output starts each tick as the sentinel (the library leaves entries at or past ``n_post[s]`` as they
    were) and every guard is checked after each tick.  -> stream ``me``'s rows of every output, ``[TICKS, ...]``."""
    x = _tick_pcm(4900)
    frames = X.Guarded(np.zeros((S, 320), np.int16), fill, width=640)
    o = X.guarded_outputs(_tick_spec(call, S))
    flags = np.ones(S, np.uint8)
    got = {k: [] for k in o}
    bank = _bank(lab, call, S)
    try:
        for t in range(TICKS):
            frames.body[...] = X.fill_of(others, np.int16, 320)[None]
            frames.body[me] = x[t]
            for g in o.values():
                g.body[...] = SENT
            _tick(bank, call, frames, flags, o)
            frames.check_guards(f"{call} S={S} tick {t}: frames")
            for k, v in X.read_outputs(o, f"{call} S={S} tick {t} ({fill} guards, {others} neighbours)").items():
                got[k].append(v[me])
    finally:
        bank.close()
    return {k: np.array(v) for k, v in got.items()}


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("call", TICK_CALLS)
def test_ticks(lab, call, S):
    """The host-pointer ticks: every caller array between guards, 25 ticks.  S = 1: the frames' guards hold a square, then zeros.
    S = 3: stream 1 between streams 0 and 2, which hold what the guards hold."""
    me = 0 if S == 1 else 1
    base = _tick_run(lab, call, S, me, "zero", "zero")
    got = _tick_run(lab, call, S, me, "square", "square")
    for k in base:
        X.assert_same_bits(got[k], base[k], f"{call} S={S}: stream {me}'s {k} over {TICKS} ticks, a square against zeros around it")
    n = base["n_post"]
    assert n.min() >= 0 and n.max() <= 2 and n.sum() >= TICKS
    if call != "step":               # a CTC tick leaves the entries at or past n_post[s] as they were (include/wwhip.h)
        for k, v in base.items():
            for t in range(TICKS):
                assert k == "n_post" or (X.bits(v[t, n[t]:]) == X.bits(np.full_like(v[t, n[t]:], SENT))).all(), (call, k, t)
    print(f"\nEXTENTS F {call} S={S}: {int(n.sum())} windows in {TICKS} ticks", end="")


# ==================================================================================================== F. the resampler
RS_LENGTHS = [1500, 0, 17, 2999, 801]     # one empty segment, one shorter than either filter (205 and 137 taps)
U24 = 2.0 ** -24


def _rs_input(fmt, rate):
    rng = np.random.default_rng(5000 + rate)
    n = sum(RS_LENGTHS)
    if fmt == "mulaw":
        return rng.integers(0, 256, n).astype(np.uint8)
    t = np.arange(n) / float(rate)
    pcm = np.clip(np.rint(rng.normal(0, 2000, n) + 8000.0 * np.sin(2 * np.pi * 440.0 * t)), -32768, 32767).astype(np.int16)
    return pcm if fmt == "i16" else (pcm.astype(np.float32) / np.float32(32768.0)) * np.float32(0.999)


@pytest.mark.parametrize("fmt", ["i16", "f32", "mulaw"])
@pytest.mark.parametrize("rate", [48000, 8000])
def test_resample_dev(rate, fmt):
    import torch
    from wwhip import g711
    from wwhip.resample import Resampler
    rs = Resampler(rate, 16000)
    try:
        up, down, half, _ = R64.design(rate)
        assert (rs.up, rs.down, rs.half) == (up, down, half) and (up > down) == (rate < 16000) and 17 < 2 * half // up
        x = _rs_input(fmt, rate)
        so = np.concatenate([[0], np.cumsum(RS_LENGTHS)]).astype(np.int64)
        counts = [R64.out_len(n, up, down) for n in RS_LENGTHS]
        oo = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        tile = max(R64.tile_outputs(up, down, half, c) for c in counts if c)
        in_dtype, law = {"i16": (np.int16, None), "f32": (np.float32, None), "mulaw": (np.uint8, "mulaw")}[fmt]

        def run(poison):
            d_in = X.Guarded(x, poison, width=4096, device=True)
            o = X.Guarded(np.full(int(oo[-1]), SENT, np.float32), SENT, width=tile + 1, device=True)
            assert o.width > tile
            torch.cuda.synchronize()
            rs.resample_dev(d_in.ptr, in_dtype, so, oo, o.ptr, np.float32, law=law)
            rs.ctx.synchronize()
            d_in.check_guards(f"resample_dev {rate} {fmt} ({poison}): input")
            o.check_guards(f"resample_dev {rate} {fmt} ({poison}): output")
            return {"y": o.read()}
        y = X.poison_runs(run, poisons=tuple(X.POISONS) if fmt == "f32" else X.PCM_POISONS, what=f"resample_dev {rate} {fmt}")["y"]
        tpp, worst = R64.tpp(up, half), 0.0
        for u, n in enumerate(RS_LENGTHS):
            seg = x[so[u]:so[u + 1]]
            seg = g711.decode(seg, "mulaw") if fmt == "mulaw" else seg
            got = y[oo[u]:oo[u + 1]].astype(np.float64)
            assert got.shape == (counts[u],)
            if not n:
                continue
            bound = (tpp + 2) * U24 * R64.bound_sum(seg, rate)
            err = np.abs(got - R64.resample(seg, rate))
            worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max()))
            assert (err <= bound).all(), (rate, fmt, u, worst)
        print(f"\nEXTENTS F resample_dev {rate} {fmt}: the zero run uses {worst:.3f} of (tpp + 2) 2^-24 A", end="")
    finally:
        rs.close()
