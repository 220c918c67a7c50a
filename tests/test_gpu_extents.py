"""Device calls read and write only the rows their contract names (include/wwhip.h), on the MI355X.

Every buffer a call gets is a ``extents.Guarded``: the body the call is told about between two guards the test owns.  Input guards
and every input row the call does not name hold a poison - NaN, 1e30, 0.0 in turn (int16 PCM: a full-scale square, zeros) - and the
runs must give the 0.0 run's BITS (integer views, no tolerance); output guards hold -7 and must keep every byte.  The 0.0 run is
held to float64 with the project's bounds (``TAU``, ``TAU_BF16``: tests/test_gpu_ref64.py, copied by name as
tests/test_gpu_geometry64.py does), the needed value printed (``pytest -s``).  A window or segment whose OWN rows are NaN must leave
every other output row's bits alone; what its own row holds is printed, not asserted (the reference does not define it).

  A  window lists     ww_forward_windows_dev, ww_set_forward_windows_dev, ww_ctc_forward_windows_dev; Engine.forward / detect
  B  sliding forms    ww_forward_segments_dev, ww_set_forward_segments_dev; Engine.slide_forward, ww_ctc_slide_forward
  C  clips, front end ww_clips_forward_dev, ww_logmel_dev
  D  evaluator tail   ww_far_frr_dev (with d_smoothed), ww_posterior_pick_dev, ww_posterior_events_dev
  E, F                the CTC lattice calls; the host-pointer ticks and ww_resample_dev: tests/test_gpu_extents_ctc.py

No address handed to the library lies outside an allocation of the test's, guards included; nothing here is expected to fault.
tests/test_extents.py shows on NumPy stand-ins that this harness rejects the mistakes it is there for.

Measured on an MI355X.  The 0.0 runs need tau 3.0e-6 (A: the shipped CRNN in every form and its set; generic 9.9e-7, Wavenet 2.5e-6,
CTC 1.4e-6), 4.3e-5 / 8.2e-5 (split-bf16 CRNN / Wavenet, held to 6.5e-4) and 3.7e-6 / 2.0e-6 (B: CRNN rows form / Wavenet).  A window
whose own rows are NaN comes out FINITE from every model but the CTC one (the ReLUs return 0 for a NaN): the shipped CRNN gives
[0.509052 0.490948] in every form, the Wavenet [0.842521 0.157479], the CTC head NaN.  Before crnn_rows_kernel cleared the operands
under its edge positions' zeroed taps, B failed for the CRNN and its set under the NaN poison alone (hop 1: 46 of 89 windows differed)
and a NaN in row 0 of ``slide_forward``'s sequence moved windows 1..6 in the rows form."""
import ctypes as C
import os

import numpy as np
import pytest

import ctc64
import extents as X
import geometry64 as G
import sweep64 as S
from oracle import ref64 as R

pytestmark = pytest.mark.gpu

TAU = 4e-5          # tests/test_gpu_ref64.py (tests/test_gpu_geometry64.py: TAU)
TAU_BF16 = 6.5e-4   # tests/test_gpu_ref64.py (tests/test_gpu_geometry64.py: TAU_BF16)
FORMS = {"fused": {"crnn_split_at": 0}, "front + vector tail": {"crnn_split_at": 1, "crnn_tail_mfma": 0},
         "front + matrix tail": {"crnn_split_at": 1, "crnn_tail_mfma": 2}}   # tests/test_gpu_geometry64.py: FORMS
CRNNS = ["CRNN_nosilence", "CRNN_softmax"]
WAVES = ["Wavenet", "Wavenet_alt"]
GENERIC = "c-t150"         # one generic-conv row of geometry64.GEOMETRIES whose window holds the 100-row case
CTC_L = 2
MEL_GUARD_ROWS = 256       # wider than crnn_rows_kernel's staged 15 * 8 + 20 rows and than any window
SENT = X.SENTINEL


class Lab:
    """The module's engines, sets and float64 readings, each made once; references are memoised by model and window bytes."""

    def __init__(self, assets):
        self.assets, self.engines, self.sets, self.readers, self.memo = assets, {}, {}, {}, {}

    def engine(self, name, precision="fp32"):
        from wwhip.engine import Engine
        key = (name, precision)
        if key not in self.engines:
            if name == GENERIC:
                e = G.engine_for(G.GEOMETRIES[name].bundle())
            elif name == "ctc":
                e = Engine(f"synthetic-ctc-{CTC_L}", bundle=ctc64.reference(CTC_L)[0])
            else:
                e = Engine(os.path.join(self.assets, name), precision=precision)
            self.engines[key] = e
        return self.engines[key]

    def model_set(self, names):
        from wwhip.engine import ModelSet
        key = tuple(names)
        if key not in self.sets:
            self.sets[key] = ModelSet([self.engine(m) for m in names])
        return self.sets[key]

    def _reader(self, name):
        if name not in self.readers:
            if name == GENERIC:
                ref = G.reference(G.GEOMETRIES[name].bundle())
                self.readers[name] = lambda w: ref.forward(w)[0]
            elif name == "ctc":
                ref = ctc64.Ctc64(ctc64.reference(CTC_L)[0].crnn)
                self.readers[name] = lambda w: ref.sequence(w)[0]
            else:
                ref = R.Ref64(os.path.join(self.assets, name))
                self.readers[name] = lambda w: ref.forward(w)[0]
        return self.readers[name]

    def ref64(self, name, wins):
        """The float64 outputs of ``wins [n, T, F]`` by model ``name``, each distinct window evaluated once per module."""
        wins = np.ascontiguousarray(wins, np.float32)
        keys = [(name, w.tobytes()) for w in wins]
        new = [i for i, k in enumerate(keys) if k not in self.memo]
        if new:
            out = self._reader(name)(wins[new])
            for j, i in enumerate(new):
                self.memo[keys[i]] = out[j]
        return np.array([self.memo[k] for k in keys])

    def close(self):
        for s in self.sets.values():
            s.close()
        for e in self.engines.values():
            e.close()


@pytest.fixture(scope="module")
def lab(assets):
    out = Lab(assets)
    yield out
    out.close()


def _held(what, got, want64, tau):
    got = np.asarray(got, np.float64).reshape(np.shape(want64))
    assert np.isfinite(got).all() and got.min() >= 0.0 and got.max() <= 1.0, what
    print(f"\nEXTENTS {what}: the 0.0 run needs tau {R.needed_tau(got, want64):.2e} (held to {tau:g}), max|dp| "
          f"{np.abs(got - want64).max():.2e}", end="")
    R.check_posteriors(got, want64, tau)


def _out_guard(shape):
    """Two rows of the output, at least 256 elements: a row or a plane written behind the extent lands here."""
    return max(256, 2 * int(np.prod(shape[1:], dtype=np.int64)))


def _outputs(spec):
    """``{name: (shape, dtype)}`` -> guarded device buffers full of the sentinel."""
    return {k: X.Guarded(np.full(shape, SENT, dtype), SENT, width=_out_guard(shape), device=True) for k, (shape, dtype) in spec.items()}


def _finish(ctx, mel, outs, what):
    ctx.synchronize()
    mel.check_guards(f"{what}: input")
    for k, g in outs.items():
        g.check_guards(f"{what}: {k}")
    return {k: g.read() for k, g in outs.items()}


# ==================================================================================================== A. window lists
N_WIN = 35                  # two 16-window groups of the matrix tail and a remainder of 3; the Wavenet's twelve-wave form
TAIL_PAIR = (20, 21)        # window 20 (full) and window 21 (100 rows) both end on the body's last row
ISOLATE = (0, 15, 16, 34)


class Windows:
    """35 windows in one mel body: disjoint row ranges with 3 to 11 unnamed rows in front of each (and the front guard in front of
    the first); ``valid`` = T but for windows 3 (0 rows), 17 (1), 21 (100) and 30 (T - 1).  Windows 20 and 21 end on the last row -
    the one pair that shares rows, as two windows that end on one row must."""

    def __init__(self, T, F, seed=4100):
        self.T, self.F = T, F
        self.valid = np.full(N_WIN, T, np.int32)
        self.valid[[3, 17, 21, 30]] = [0, 1, 100, T - 1]
        assert 100 < T
        gaps = [3 + (5 * w) % 9 for w in range(N_WIN)]
        self.row, self.rows, self.named = X.window_layout(self.valid, gaps, T, tail_pair=TAIL_PAIR)
        content = G.windows(seed, N_WIN, T, F)
        self.body = np.zeros((self.rows, F), np.float32)
        for w in range(N_WIN):
            if w != TAIL_PAIR[1]:
                self.body[self.row[w]:self.row[w] + self.valid[w]] = content[w, :self.valid[w]]
        self.cut = np.zeros((N_WIN, T, F), np.float32)     # the explicit zero-padded windows
        for w in range(N_WIN):
            self.cut[w, :self.valid[w]] = self.body[self.row[w]:self.row[w] + self.valid[w]]
        assert self.row[20] + T == self.rows == self.row[21] + 100
        for a in (self.body, self.cut, self.row, self.valid, self.named):
            a.setflags(write=False)


_layouts = {}


def _windows_of(T, F):
    if (T, F) not in _layouts:
        _layouts[T, F] = Windows(T, F)
    return _layouts[T, F]


class WindowCase:
    """One engine (or set) and dispatch form of section A: what to call, what it writes, which model reads window w in float64."""

    def __init__(self, lab, name):
        self.name, self.opts, self.tau, self.kind = name, {}, TAU, "engine"
        if name in FORMS:
            self.e, self.opts, self.models = lab.engine(CRNNS[0]), FORMS[name], [CRNNS[0]]
        elif name == "generic":
            self.e, self.models = lab.engine(GENERIC), [GENERIC]
        elif name == "wavenet":
            self.e, self.models = lab.engine(WAVES[0]), [WAVES[0]]
        elif name == "crnn bf16x3":
            self.e, self.models, self.tau = lab.engine(CRNNS[0], "bf16x3"), [CRNNS[0]], TAU_BF16
        elif name == "wavenet bf16x3":
            self.e, self.models, self.tau = lab.engine(WAVES[0], "bf16x3"), [WAVES[0]], TAU_BF16
        elif name in ("crnn set", "wavenet set"):
            self.models = CRNNS if name == "crnn set" else WAVES
            self.e, self.kind = lab.model_set(self.models), "set"
        elif name == "ctc":
            self.e, self.models, self.kind = lab.engine("ctc"), ["ctc"], "ctc"
        else:
            raise KeyError(name)
        self.ids = np.arange(N_WIN, dtype=np.int32) % len(self.models)
        self.lay = _windows_of(self.e.window, self.e.n_mel)
        self.main = "steps" if self.kind == "ctc" else "out"

    def spec(self, n):
        e = self.e
        if self.kind == "ctc":
            return {"labels": ((n, 19), np.int32), "lengths": ((n,), np.int32), "steps": ((n, 19, e.n_out), np.float32),
                    "enc": ((n, 19, 64), np.float32)}
        spec = {"out": ((n, e.n_out), np.float32)}
        if self.kind == "set":
            spec["enc"] = ((n,) + tuple(e.enc_shape), np.float32)
        return spec

    def call(self, d_mel, rows, d_row, d_valid, n, outs):
        e = self.e
        if self.kind == "ctc":
            e.ctc_forward_windows_dev(d_mel, rows, d_row, d_valid, n, 19, outs["labels"].ptr, outs["lengths"].ptr, outs["steps"].ptr,
                                      outs["enc"].ptr)
        elif self.kind == "set":
            e.forward_windows_dev(d_mel, rows, d_row, d_valid, self.ids[:n], n, outs["out"].ptr, outs["enc"].ptr)
        else:
            with e.options(**self.opts):
                e.forward_windows_dev(d_mel, rows, d_row, d_valid, n, outs["out"].ptr)

    def want64(self, lab):
        got = [None] * N_WIN
        for m, name in enumerate(self.models):
            idx = np.flatnonzero(self.ids == m)
            for i, v in zip(idx, lab.ref64(name, self.lay.cut[idx])):
                got[i] = v
        return np.array(got)

    def run(self, poison, nan_window=None):
        import torch
        lay = self.lay
        body = X.poison_rows(lay.body, lay.named, poison)
        if nan_window is not None:
            body[lay.row[nan_window]:lay.row[nan_window] + lay.valid[nan_window]] = np.nan
        mel = X.Guarded(body, poison, width=MEL_GUARD_ROWS * lay.F, device=True)
        d_row, d_valid = torch.from_numpy(np.array(lay.row)).cuda(), torch.from_numpy(np.array(lay.valid)).cuda()
        outs = _outputs(self.spec(N_WIN))
        torch.cuda.synchronize()
        self.call(mel.ptr, lay.rows, d_row.data_ptr(), d_valid.data_ptr(), N_WIN, outs)
        return _finish(self.e.ctx, mel, outs, f"{self.name} ({poison}{'' if nan_window is None else f', window {nan_window} NaN'})")


WINDOW_CASES = list(FORMS) + ["generic", "wavenet", "crnn bf16x3", "wavenet bf16x3", "crnn set", "wavenet set", "ctc"]


@pytest.mark.parametrize("name", WINDOW_CASES)
def test_window_lists(lab, name):
    """(1) NaN and 1e30 in every unnamed row and in the guards give the bits of the 0.0 run; (2) the 0.0 run against float64 on the
    explicit zero-padded windows; (3) every output guard intact (the set form's ``d_enc`` and the CTC form's four outputs included);
    isolation: window k's own rows NaN, k in {0, 15, 16, 34} - every other row of every output keeps its bits."""
    case = WindowCase(lab, name)
    base = X.poison_runs(case.run, what=name)
    _held(f"A {name}, {N_WIN} windows", base[case.main].reshape(-1, case.e.n_out), case.want64(lab).reshape(-1, case.e.n_out), case.tau)
    others = np.ones(N_WIN, bool)
    for k in ISOLATE:
        got = case.run("zero", nan_window=k)
        others[:] = True
        others[k] = False
        for key in base:
            X.assert_same_bits(got[key][others], base[key][others], f"{name}: {key}, rows other than window {k}, whose own rows are NaN")
        print(f"\nEXTENTS A {name}: window {k} all NaN -> its own row {np.array2string(got[case.main][k].reshape(-1)[:4], precision=6)}", end="")


@pytest.mark.parametrize("name", list(FORMS) + ["generic", "wavenet", "crnn bf16x3", "wavenet bf16x3", "ctc"])
def test_host_forms_isolate_a_nan_window(lab, name):
    """``Engine.forward`` with window k NaN and ``Engine.detect`` with encoder row k NaN, at batch sizes 3 and 35 (``ctc_forward`` for
    the CTC model): every other row has the bits of the clean batch."""
    case = WindowCase(lab, name)
    e, cut = case.e, case.lay.cut
    for B, ks in ((3, (0, 2)), (N_WIN, ISOLATE)):
        wins = np.array(cut[:B])
        with e.options(**case.opts):
            if case.kind == "ctc":
                clean = e.ctc_forward(wins, 19, want=("labels", "steps", "enc"))
                clean = {"labels": clean.labels, "lengths": clean.lengths, "steps": clean.steps, "enc": clean.enc}
            else:
                post, enc = e.forward(wins, want_enc=True)
                clean = {"out": post, "enc": enc, "detect": e.detect(enc)}
            for k in ks:
                w = wins.copy()
                w[k] = np.nan
                others = np.arange(B) != k
                if case.kind == "ctc":
                    r = e.ctc_forward(w, 19, want=("labels", "steps", "enc"))
                    got = {"labels": r.labels, "lengths": r.lengths, "steps": r.steps, "enc": r.enc}
                else:
                    post, enc = e.forward(w, want_enc=True)
                    bad = clean["enc"].copy()
                    bad[k] = np.nan
                    got = {"out": post, "enc": enc, "detect": e.detect(bad)}
                for key in clean:
                    X.assert_same_bits(got[key][others], clean[key][others], f"{name} host, batch {B}: {key}, rows other than {k}")
                print(f"\nEXTENTS A {name} host, batch {B}: window {k} all NaN -> {np.array2string(got[case.main][k].reshape(-1)[:4], precision=6)}"
                      + ("" if case.kind == "ctc" else f", detect of a NaN encoder row -> {np.array2string(got['detect'][k], precision=6)}"), end="")


# ==================================================================================================== B. sliding forms
SEG_NW = [1, 15, 16, 17, 0, 40]      # last tiles of 1, 15, 16, 1 and 8 positions
SEG_GAP = [0, 5, 3, 0, 7, 1]         # unnamed rows behind each segment: segment 1 follows segment 0 at once
HOPS = [1, 2, 3, 8]                  # g = gcd(hop, 8) = 1, 2, 1, 8
SET_MEMBERS = [1, 0, 1]


class Segments:
    """Six mel sequences in one body (``SEG_NW`` windows each under ``hop``; an empty sequence has no rows), ``SEG_GAP`` unnamed rows
    behind each."""

    def __init__(self, T, F, hop, seed=4200):
        self.T, self.F, self.hop = T, F, hop
        self.nw = np.array(SEG_NW, np.int32)
        self.len = [T + (n - 1) * hop if n else 0 for n in SEG_NW]
        self.row0 = np.zeros(len(SEG_NW), np.int64)
        at = 0
        for s, (n, gap) in enumerate(zip(self.len, SEG_GAP)):
            self.row0[s] = at
            at += n + gap
        self.rows = at
        self.named = np.zeros(at, bool)
        self.body = np.zeros((at, F), np.float32)
        for s, n in enumerate(self.len):
            if n:
                self.named[self.row0[s]:self.row0[s] + n] = True
                self.body[self.row0[s]:self.row0[s] + n] = G.windows(seed + 10 * hop + s, 1, n, F)[0]
        self.off = np.concatenate([[0], np.cumsum(self.nw)]).astype(np.int64)   # first output row of each segment
        self.W = int(self.off[-1])

    def seq(self, s):
        return self.body[self.row0[s]:self.row0[s] + self.len[s]]

    def windows(self, s):
        return np.ascontiguousarray(np.lib.stride_tricks.sliding_window_view(self.seq(s), (self.T, self.F))[::self.hop, 0])


class SlideCase:
    def __init__(self, lab, name):
        self.name, self.opts = name, {}
        if name in ("crnn", "crnn matrix tail"):    # the rows form with gru_tail_kernel (the default below 9,216 windows) / gru_tail16_kernel
            self.e, self.members, self.kind = lab.engine(CRNNS[0]), [CRNNS[0]], "engine"
            self.opts = {"crnn_tail_mfma": 2} if name == "crnn matrix tail" else {}
        elif name == "wavenet":
            self.e, self.members, self.kind = lab.engine(WAVES[0]), [WAVES[0]], "engine"
        else:
            self.e, self.members, self.kind = lab.model_set(CRNNS), [CRNNS[m] for m in SET_MEMBERS], "set"

    def run(self, seg, poison, nan_seg=None, only=None):
        """The six segments in one call, or (``only``) one segment alone in a body of its own rows between zero guards."""
        import torch
        e = self.e
        if only is None:
            body, row0, nw = X.poison_rows(seg.body, seg.named, poison), seg.row0, seg.nw
            if nan_seg is not None:
                body[seg.row0[nan_seg]:seg.row0[nan_seg] + seg.len[nan_seg]] = np.nan
        else:
            body, row0, nw = np.array(seg.seq(only)), np.zeros(1, np.int64), seg.nw[only:only + 1]
        W, slots = int(nw.sum()), len(self.members)
        mel = X.Guarded(body, poison, width=MEL_GUARD_ROWS * seg.F, device=True)
        outs = _outputs({"out": ((slots, W, e.n_out), np.float32)})
        torch.cuda.synchronize()
        if self.kind == "set":
            e.set_option("crnn_slide_min", 1)
            try:
                e.forward_segments_dev(mel.ptr, len(body), row0, nw, seg.hop, outs["out"].ptr, members=SET_MEMBERS)
            finally:
                e.set_option("crnn_slide_min", 64)
        else:
            with e.options(**self.opts):
                e.forward_segments_dev(mel.ptr, len(body), row0, nw, seg.hop, outs["out"].ptr)
        return _finish(e.ctx, mel, outs, f"{self.name} hop {seg.hop} ({poison}, nan_seg {nan_seg}, only {only})")


@pytest.mark.parametrize("hop", HOPS)
@pytest.mark.parametrize("name", ["crnn", "crnn matrix tail", "crnn set", "wavenet"])
def test_sliding_segments(lab, name, hop):
    """(1) the three poisons in the gaps and the guards: the same bits; (2) each segment's rows are the bits of a call on that segment
    alone (a zero-row gap's over-read lands in the neighbour's finite rows: only this shows it); (3) the first and the last segment
    against float64; (4) guards intact - ``d_out`` is ``[slots][W][n_out]``, so the back guard is the row behind the last plane;
    isolation: segment 3 all NaN, every other segment keeps its bits."""
    case = SlideCase(lab, name)
    seg = Segments(case.e.window, case.e.n_mel, hop)
    base = X.poison_runs(lambda p: case.run(seg, p), what=f"{name} hop {hop}")["out"]
    assert base.shape == (len(case.members), seg.W, case.e.n_out)
    for s, n in enumerate(SEG_NW):
        if n:
            alone = case.run(seg, "zero", only=s)["out"]
            X.assert_same_bits(base[:, seg.off[s]:seg.off[s + 1]], alone, f"{name} hop {hop}: segment {s} in the call against the segment alone")
    if name == "crnn set":
        X.assert_same_bits(base[0], base[2], f"{name} hop {hop}: the two slots of member {SET_MEMBERS[0]}")
    for s in (0, len(SEG_NW) - 1):
        wins = seg.windows(s)
        for k, member in enumerate(case.members):
            if k == 2:
                continue
            _held(f"B {name} hop {hop}, segment {s} ({SEG_NW[s]} windows), {member}", base[k, seg.off[s]:seg.off[s + 1]],
                  lab.ref64(member, wins), TAU)
    got = case.run(seg, "zero", nan_seg=3)["out"]
    keep = np.ones(seg.W, bool)
    keep[seg.off[3]:seg.off[4]] = False
    X.assert_same_bits(got[:, keep], base[:, keep], f"{name} hop {hop}: rows of the segments other than 3, whose rows are NaN")
    print(f"\nEXTENTS B {name} hop {hop}: segment 3 all NaN -> its first row {np.array2string(got[0, seg.off[3]], precision=6)}", end="")


@pytest.mark.parametrize("name", ["crnn fused", "crnn rows", "wavenet", "ctc"])
def test_host_sliding_forms_isolate_nan_rows(lab, name):
    """``Engine.slide_forward`` (the CRNN below its rows-form threshold and with the rows form from one window on; the Wavenet) and
    ``ww_ctc_slide_forward`` over 40 windows at hops 1, 2, 3 and 8: NaN in the first ``hop`` rows (named by window 0 alone), then in
    the last ``hop`` rows (named by window 39 alone) - every other window has the clean run's bits."""
    e = lab.engine({"crnn fused": CRNNS[0], "crnn rows": CRNNS[0], "wavenet": WAVES[0], "ctc": "ctc"}[name])
    opts = {"crnn rows": {"crnn_slide_min": 1}, "crnn fused": {"crnn_slide_min": 0}}.get(name, {})
    T, nw = e.window, 40

    def slide(mel, hop):
        if name == "ctc":
            r = e.ctc_slide_forward(mel, hop, 19, want=("labels", "steps"))
            return {"labels": r.labels, "lengths": r.lengths, "steps": r.steps}
        with e.options(**opts):
            return {"out": e.slide_forward(mel, hop)}
    for hop in HOPS:
        mel = np.array(Segments(T, e.n_mel, hop).seq(5))
        clean = slide(mel, hop)
        for where, rows, k in (("first", slice(0, hop), 0), ("last", slice(len(mel) - hop, len(mel)), nw - 1)):
            bad = mel.copy()
            bad[rows] = np.nan
            got = slide(bad, hop)
            others = np.arange(nw) != k
            for key in clean:
                assert len(clean[key]) == nw
                X.assert_same_bits(got[key][others], clean[key][others], f"{name} hop {hop}: {key}, the {where} {hop} rows NaN")
            main = got["steps" if name == "ctc" else "out"][k].reshape(-1)[:4]
            print(f"\nEXTENTS B {name} host hop {hop}: the {where} {hop} rows NaN -> window {k}: {np.array2string(main, precision=6)}", end="")


# ==================================================================================================== C. clip path and front end
CLIP_SAMPLES = [511, 512, 2000, 24000, 24159]   # no frame, one frame, fewer frames than a window, 147 frames, one hop short of 149
N_CLIPS = 5
UTT_LENGTHS = [0, 511, 512, 673, 8000, 3333]
PCM_GUARD = 4096


def _pcm(seed, n):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / 16000.0
    return np.clip(np.rint(rng.normal(0, 1500, n) + 4000.0 * np.sin(2 * np.pi * (300.0 + 700.0 * t) * t)), -32768, 32767).astype(np.int16)


@pytest.mark.parametrize("samples", CLIP_SAMPLES)
@pytest.mark.parametrize("model", [CRNNS[0], WAVES[0]])
def test_clip_path(lab, model, samples):
    """Five clips per call behind and in front of a full-scale square (then zeros): the same bits, posteriors, and guards intact."""
    import torch
    e = lab.engine(model)
    pcm = _pcm(4300 + samples, N_CLIPS * samples).reshape(N_CLIPS, samples)

    def run(poison):
        d_pcm = X.Guarded(pcm, poison, width=PCM_GUARD, device=True)
        assert d_pcm.ptr % 16 == 0
        outs = _outputs({"out": ((N_CLIPS, e.n_out), np.float32)})
        torch.cuda.synchronize()
        e.clips_forward_dev(d_pcm.ptr, N_CLIPS, samples, outs["out"].ptr)
        return _finish(e.ctx, d_pcm, outs, f"clips {model} {samples} ({poison})")
    out = X.poison_runs(run, poisons=X.PCM_POISONS, what=f"clips {model} {samples}")["out"]
    assert np.isfinite(out).all() and out.min() >= 0.0 and out.max() <= 1.0
    if samples < 512:
        assert (out == out[0]).all()      # no frame: every clip is the all-zero window
    print(f"\nEXTENTS C clips {model}, {samples} samples: posteriors {np.array2string(out[:, e.posterior_index], precision=6)}", end="")


@pytest.mark.parametrize("hop", [160, 1])
def test_front_end(lab, hop):
    """A ragged batch of six utterances (0, 511, 512, 673, 8,000 and 3,333 samples; contiguous ``frame_offs`` as the host form writes
    them) between PCM guards: a square and zeros give the same rows, which are ``Engine.logmel``'s bit for bit; guards intact."""
    import torch
    from wwhip.engine import frontend_params
    e = lab.engine(CRNNS[0])
    fp = frontend_params(hop=hop)
    utts = [_pcm(4400 + i, n) for i, n in enumerate(UTT_LENGTHS)]
    soffs = np.concatenate([[0], np.cumsum(UTT_LENGTHS)]).astype(np.int64)
    frames = [e.num_frames(n, hop) for n in UTT_LENGTHS]
    assert frames[:3] == [0, 0, 1] and frames[3] == (673 - 512) // hop + 1
    foffs = np.concatenate([[0], np.cumsum(frames)]).astype(np.int64)
    total = int(foffs[-1])
    want = e.logmel(utts, fp)

    def run(poison):
        d_pcm = X.Guarded(np.concatenate(utts), poison, width=PCM_GUARD, device=True)
        d_soffs, d_foffs = torch.from_numpy(soffs).cuda(), torch.from_numpy(foffs).cuda()
        outs = _outputs({"mel": ((total, e.n_mel), np.float32)})
        torch.cuda.synchronize()
        e.logmel_dev(d_pcm.ptr, d_soffs.data_ptr(), d_foffs.data_ptr(), len(utts), total, max(frames), outs["mel"].ptr, fp)
        return _finish(e.ctx, d_pcm, outs, f"logmel_dev hop {hop} ({poison})")
    mel = X.poison_runs(run, poisons=X.PCM_POISONS, what=f"logmel_dev hop {hop}")["mel"]
    for u, w in enumerate(want):
        assert len(w) == frames[u]
        X.assert_same_bits(mel[foffs[u]:foffs[u + 1]], w, f"logmel_dev hop {hop}: utterance {u} against Engine.logmel")


# ==================================================================================================== D. evaluator tail
N_NEG, N_POS = 1000, 300
TAIL_POISONS = ("nan", "1e30", "zero")   # (1e30 beside the NaN: a NaN is above no threshold, so a leaked one would not move a count)


def _far_frr_dev(e, d_pos, n_pos, d_neg, n_neg, thr, win, d_sm):
    from wwhip import _lib
    frr, fa, cnt = np.full(thr.size, SENT), np.full(thr.size, SENT), np.full(thr.size, -7, np.int64)
    rc = _lib.load().ww_far_frr_dev(e.ctx.handle, C.c_void_p(d_pos), n_pos, C.c_void_p(d_neg), n_neg, int(win), _lib.ptr(thr), thr.size,
                                    float(n_pos), 1.0, _lib.ptr(frr), _lib.ptr(fa), _lib.ptr(cnt), C.c_void_p(d_sm))
    _lib.raise_for(rc, e.ctx.handle)
    return frr, fa, cnt


@pytest.mark.parametrize("win", [1, 30, 31])
def test_far_frr_dev(lab, win):
    """1,000 negatives and 300 positives (several 256-thread blocks with a ragged end) between guards: the same counters and the same
    smoothed bits under every poison, the guards of ``d_smoothed`` intact, and the counters equal to sweep64's float64 statement."""
    import torch
    e = lab.engine(CRNNS[0])
    neg, pos = S.noise(4500 + win, N_NEG), np.random.default_rng(4501).uniform(0.2, 1.0, N_POS).astype(np.float32)
    thr = np.ascontiguousarray(S.DEFAULT_THR)

    def run(poison):
        d_neg, d_pos = X.Guarded(neg, poison, width=256, device=True), X.Guarded(pos, poison, width=256, device=True)
        outs = _outputs({"smoothed": ((N_NEG,), np.float64)})
        torch.cuda.synchronize()
        frr, fa, cnt = _far_frr_dev(e, d_pos.ptr, N_POS, d_neg.ptr, N_NEG, thr, win, outs["smoothed"].ptr)
        d_pos.check_guards("positives")
        got = _finish(e.ctx, d_neg, outs, f"far_frr_dev win {win} ({poison})")
        got.update(frr=frr, fa=fa, cnt=cnt)
        return got
    base = X.poison_runs(run, poisons=TAIL_POISONS, what=f"far_frr_dev win {win}")
    sm64 = S.smooth(neg, win)
    assert np.all(np.abs(base["smoothed"] - sm64) <= S.smooth_bound(neg, win))
    have, need = S.margin_holds(neg, win, thr)
    assert have > need, "the input leaves float64 no margin at a threshold: choose another seed"
    np.testing.assert_array_equal(base["cnt"], S.counts(sm64, thr))
    np.testing.assert_array_equal(base["cnt"], S.counts(base["smoothed"], thr))
    np.testing.assert_array_equal(base["fa"], base["cnt"] / 1.0)
    accepted = np.rint(N_POS - base["frr"] * N_POS).astype(np.int64)
    np.testing.assert_array_equal(accepted, S.accepts(pos, thr))


def test_posterior_pick_dev(lab):
    """1,000 detect rows of two columns: every row (no table), then the maximum of 7 ragged runs (one empty, one that ends at n, none
    that covers rows 0..4).  The column that is not picked, the rows no run names and the guards hold the poison."""
    import torch
    e = lab.engine(CRNNS[0])
    n, pidx = 1000, e.posterior_index
    assert e.n_out == 2
    rows = np.random.default_rng(4600).uniform(0, 1, (n, 2)).astype(np.float32)
    offs = np.array([5, 6, 130, 130, 257, 512, 513, n], np.int64)
    in_run = np.zeros(n, bool)
    in_run[5:] = True

    def run(poison, table):
        body = np.array(rows)
        body[:, 1 - pidx] = X.fill_of(poison, np.float32, 1)[0]
        if table:
            body = X.poison_rows(body, in_run, poison)
        d_rows = X.Guarded(body, poison, width=256, device=True)
        d_offs = torch.from_numpy(offs).cuda()
        outs = _outputs({"picked": ((offs.size - 1 if table else n,), np.float32)})
        torch.cuda.synchronize()
        if table:
            e.posterior_pick_dev(d_rows.ptr, n, outs["picked"].ptr, d_offs.data_ptr(), offs.size - 1)
        else:
            e.posterior_pick_dev(d_rows.ptr, n, outs["picked"].ptr)
        return _finish(e.ctx, d_rows, outs, f"posterior_pick_dev (table {table}, {poison})")
    for table in (False, True):
        got = X.poison_runs(lambda p: run(p, table), poisons=TAIL_POISONS, what=f"pick, table {table}")["picked"]
        X.assert_same_bits(got, S.pick(rows, 2, pidx, offs if table else None), f"pick, table {table}, against sweep64.pick")


@pytest.mark.parametrize("win", [1, 30, 31])
def test_posterior_events_dev(lab, win):
    """Two planes of 1,000 rows, three segments over rows 17..976: the rows of both planes that no segment names, and the guards, hold
    the poison ("rows outside every segment belong to no event") - the same events, totals and plane counts under every poison."""
    import torch
    e = lab.engine(CRNNS[0])
    n = 1000
    post = np.stack([S.noise(4700 + win, n), S.noise(4710 + win, n)])
    offs = np.array([17, 301, 640, 977], np.int64)
    named = np.zeros(n, bool)
    named[17:977] = True
    thr = np.array([0.45, 0.5]) if win > 1 else np.array([0.7, 0.8])

    def run(poison):
        body = np.array(post)
        body[:, ~named] = X.fill_of(poison, np.float32, 1)[0]
        d_post = X.Guarded(body, poison, width=256, device=True)
        torch.cuda.synchronize()
        ev, counts, total = e.posterior_events_dev(d_post.ptr, n, thr, offs, window=win, planes=2, want_counts=True)
        d_post.check_guards(f"events win {win} ({poison})")
        return {"events": ev, "counts": counts, "total": np.int64(total)}
    base = X.poison_runs(run, poisons=TAIL_POISONS, what=f"posterior_events_dev win {win}")
    ev = base["events"]
    assert len(ev) == base["total"] == base["counts"].sum() and base["counts"].min() >= 3
    seg_len = np.diff(offs)
    assert (ev["start"] >= 0).all() and (ev["end"] <= seg_len[ev["seg"]]).all() and (ev["start"] < ev["end"]).all()
    print(f"\nEXTENTS D events win {win}: {base['counts'].tolist()} events per plane", end="")
