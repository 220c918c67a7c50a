"""Section E of the extents tests: the CTC lattice calls between guards, stated once for the host functions of csrc/ctc_*.h
(tests/test_extents.py, no GPU) and for the device kernels (tests/test_gpu_extents_ctc.py).  The layouts, the poisoned-sequence sets
and every assertion are the same code for both: a ``Backend`` only says which entry point gets the addresses.

The calls take ``steps [n][T][L]`` and read all of it, so there are two kinds of run (tests/extents.py):

  guards      the body is the table; the guards around it hold NaN, 1e30, 0.0 in turn and the three runs give the same bits; every
              output lies between sentinel guards that keep every byte.
  poisoned    some SEQUENCES of the body hold the poison in every element; every other sequence's outputs carry the bits of the
              0.0 guard run.  What a poisoned sequence's own rows hold is reported, not asserted.

The kernels' geometry, restated from csrc/ctc_score.hip (the align and occupancy kernels share it): a (sequence, target) pair owns
``P`` adjacent lanes, ``P`` = 2 Umax + 1 rounded up to 4, 8, 16, 32; pairs in sequence-major order, 256 / P to a workgroup of four
waves; DPP row shifts stay inside 16 lanes.  ``edge_sequences`` names the sequences whose pairs sit on those edges.  The beam kernel
(csrc/ctc_beam.hip) is a wave per sequence, four to a workgroup; the greedy decode a thread per sequence, 64 to a workgroup."""
import numpy as np

import extents as X

N_SEQ, K = 45, 3
# Umax -> the K lengths: but for Umax = 1 one is shorter than Umax (idle lanes beside a live neighbour).  The LAST target is the longest:
# where 2 Umax + 1 = P - 1 (P = 4, 8, 16) its lane P - 2 is live, the one lane a shift by 2 carries into the NEXT sequence's first
# segment - and the one lane of a sequence's last segment that a shift down from the next sequence reaches.
TARGET_LENS = {1: (1, 1, 1), 3: (2, 1, 3), 7: (4, 1, 7), 9: (6, 1, 9)}
SEGMENT = {1: 4, 3: 8, 7: 16, 9: 32}                                        # Umax -> P (tests/test_gpu_ctc_score.py: test_every_kernel_shape's map)
TS = (1, 2, 9, 10, 19, 64)     # no loop, one step, one prefetch group of 8, one step into the second, the standard geometry, the LDS ceiling
BEAM_TS = (1, 2, 9, 10, 19)    # the beam calls refuse T > WW_CTC_BEAM_MAX_T = 19
MODES = ("exact", "prefix")
NU = 9                         # WW_CTC_SCORE_MAX_TARGET
AHEAD = 8                      # the kernels' prefetch group (CS_AHEAD, CA_AHEAD, CO_AHEAD)
BEAM_WAVES = 4                 # csrc/ctc_beam.hip: CB_WAVES
GREEDY_N, GREEDY_BLOCK = 70, 64
SEQ_AXIS = {"score": 1, "value": 1, "span": 1, "occ": 1, "cls": 1, "labels": 0, "lengths": 0, "prob": 0}


def segment_width(umax: int) -> int:
    s = 2 * umax + 1
    return 4 if s <= 4 else 8 if s <= 8 else 16 if s <= 16 else 32


def tables(seed: int, n: int, T: int, L: int) -> np.ndarray:
    """Posteriors with a peak per row (a Dirichlet of small concentration), a third of the sequences on a grid of sixteenths - exact
    zeros, which a NaN times a zero mask would not survive (tests/test_gpu_ctc_score.py: ``_tables``)."""
    y = np.random.default_rng(seed).dirichlet(np.full(L, 0.3), (n, T)).astype(np.float32)
    y[::3] = np.round(y[::3] * 16) / np.float32(16)
    y.setflags(write=False)
    return y


def targets_of(umax: int, L: int):
    """K = 3 targets of ``TARGET_LENS[umax]`` labels in [0, L - 2] (L = 2 has the one label 0: every target is a run of repeats)."""
    rng = np.random.default_rng(100 * umax + L)
    return [tuple(int(c) for c in rng.integers(0, L - 1, U)) for U in TARGET_LENS[umax]]


def edge_sequences(P: int, k: int = K, n: int = N_SEQ) -> dict:
    """``{what: sequence}``: sequences 0 and n - 1, and the sequences whose pairs own the segment that holds the last lane of the
    first 16-lane row, wave and workgroup of the grid, and the segment that holds the lane behind it."""
    out = {"the first sequence": 0, "the last sequence": n - 1}
    for name, lane in (("16-lane row", 16), ("wave", 64), ("workgroup", 256)):
        out[f"the last segment of a {name}"] = ((lane - 1) // P) // k
        out[f"the first segment of the next {name}"] = (lane // P) // k
    # The backward pass of the occupancy kernel shifts the other way (row_shl, __shfl_down): it would leak from a pair into the pair
    # BELOW it.  The sets above do not always leave a clean pair right below a poisoned one inside the reach of a shift (a 16-lane
    # row for DPP, a wave for the shuffles of P = 32), so one more sequence is poisoned: the first whose first segment does not open
    # such a unit and whose neighbours on both sides are clean.
    unit, taken = (16 if P < 16 else 64), set(out.values())
    out["a sequence with a clean segment right below it"] = next(i for i in range(1, n - 1) if not {i - 1, i, i + 1} & taken and (i * k * P) % unit)
    return out


def check_edges(P: int, k: int = K, n: int = N_SEQ) -> list:
    """Asserts that ``edge_sequences`` is what it claims and that the grid has the shape the cases are about; returns the sorted
    poisoned set."""
    total, per = n * k, 256 // P
    assert total == 135 and total % per == 7 and -(-total // per) >= 3      # a partial last workgroup of 7 live segments
    edges = edge_sequences(P, k, n)
    poisoned = sorted(set(edges.values()))
    for name, lane in (("16-lane row", 16), ("wave", 64), ("workgroup", 256)):
        a, b = (lane - 1) // P, lane // P
        if P <= lane:                # segment a ends on the edge's last lane, segment b begins on the lane behind it
            assert (a + 1) * P == lane == b * P and b == a + 1, (P, name)
        else:                        # P = 32 against a 16-lane row: one segment lies across the edge
            assert a == b and a * P < lane < (a + 1) * P, (P, name)
        assert edges[f"the last segment of a {name}"] == a // k and edges[f"the first segment of the next {name}"] == b // k
        assert a // k in poisoned and b // k in poisoned and b < total
    seq = lambda pair: pair // k
    wave = lambda pair: pair * P // 64
    up = [j for j in range(total - 1) if seq(j) in poisoned and seq(j + 1) not in poisoned and wave(j) == wave(j + 1)]
    down = [j for j in range(total - 1) if seq(j) not in poisoned and seq(j + 1) in poisoned and wave(j) == wave(j + 1)]
    assert up and down               # a clean pair right above and right below a poisoned one, in one wave: where a shift would leak
    if P < 16:                       # and in one 16-lane row, where a DPP shift reaches
        assert [j for j in up if j * P // 16 == (j + 1) * P // 16] and [j for j in down if j * P // 16 == (j + 1) * P // 16]
    assert n - 2 not in poisoned and n - 1 in poisoned    # the grid's dead segments repeat poisoned work; sequence n - 2 decides it
    assert len(poisoned) < n // 2
    return poisoned


class Backend:
    """``device=False``: the host functions ``ww_ctc_*_rows`` over ``Guarded(device=False)`` buffers; ``device=True``: ``ww_ctc_*_dev``
    on the context of ``engine`` over device buffers."""

    def __init__(self, engine=None):
        from wwhip import _lib
        self._lib, self.lib = _lib, _lib.load()
        self.device = engine is not None
        self.handle = engine.ctx.handle if self.device else None
        self.engine = engine

    def sync(self):
        """Both ways: the buffers are uploaded on torch's stream, the library enqueues on its context's."""
        if self.device:
            import torch
            torch.cuda.synchronize()
            self.engine.ctx.synchronize()

    def lattice(self, name, steps_ptr, n, T, L, targets, mode, outs):
        from wwhip import ctc
        tab, lens = ctc.pack_targets(targets, L)
        p = self._lib.ptr
        tail = {"score": ("score",), "align": ("value", "span"), "occupancy": ("value", "occ", "cls")}[name]
        args = [outs[k].ptr if k in outs else None for k in tail]
        fn = getattr(self.lib, f"ww_ctc_{name}_dev" if self.device else f"ww_ctc_{name}_rows")
        lead = (self.handle,) if self.device else ()
        self._lib.raise_for(fn(*lead, steps_ptr, n, T, L, p(tab), p(lens), len(lens), ctc.score_mode(mode), *args), self.handle)

    def beam(self, steps_ptr, n, T, L, W, P, M, outs):
        fn = self.lib.ww_ctc_beam_dev if self.device else self.lib.ww_ctc_beam_rows
        lead = (self.handle,) if self.device else ()
        self._lib.raise_for(fn(*lead, steps_ptr, n, T, L, W, P, M, outs["labels"].ptr, outs["lengths"].ptr, outs["prob"].ptr), self.handle)

    def greedy(self, steps, n, T, L, M, outs):
        """The device call, or on the host ``wwhip.ctc.greedy_decode`` (the numpy statement of csrc/ctc_decode.h; the library has no
        host entry point for the decode alone) written through the guarded bodies."""
        if self.device:
            self._lib.raise_for(self.lib.ww_ctc_greedy_dev(self.handle, steps.ptr, n, T, L, M, outs["labels"].ptr, outs["lengths"].ptr), self.handle)
            return
        from wwhip import ctc
        labels, lengths = ctc.greedy_decode(steps.body.reshape(n, T, L), M)
        outs["labels"].body[...] = labels
        outs["lengths"].body[...] = lengths


def steps_guard(T: int, L: int) -> int:
    """The width of ``d_steps``' guards: 64 sequences - a whole number of them, and wider than a prefetch group's reach."""
    assert 64 * T * L >= AHEAD * L
    return 64 * T * L


def lattice_spec(name, n, T, L, want_cls):
    if name == "score":
        return {"score": ((K, n), np.float32)}
    if name == "align":
        return {"value": ((K, n), np.float32), "span": ((K, n, NU, 2), np.int8)}
    spec = {"value": ((K, n), np.float32), "occ": ((K, n, T, NU), np.float32)}
    if want_cls:
        spec["cls"] = ((K, n, T, L), np.float32)
    return spec


def lattice_run(be: Backend, name, y, targets, mode, fill, poisoned=None, want_cls=False) -> dict:
    """One call: the table ``y`` (the sequences in ``poisoned`` holding ``fill`` in every element) between guards of ``fill``, every
    output between sentinel guards; all guards checked."""
    n, T, L = y.shape
    body = y if poisoned is None else X.poison_sequences(y, poisoned, fill)
    steps = X.Guarded(body, fill, width=steps_guard(T, L), device=be.device)
    outs = X.guarded_outputs(lattice_spec(name, n, T, L, want_cls), be.device)   # (the outputs are [K][n]...: a guard is two whole planes)
    what = f"{name} T={T} L={L} {mode} ({fill}{'' if poisoned is None else f', sequences {list(poisoned)} poisoned'}{', cls' if want_cls else ''})"
    be.sync()
    be.lattice(name, steps.ptr, n, T, L, targets, mode, outs)
    be.sync()
    steps.check_guards(f"{what}: steps")
    return X.read_outputs(outs, what)


def lattice_inputs(umax, T, L):
    """``(steps [45, T, L], targets)`` of a case."""
    return tables(7000 + 10 * T + L, N_SEQ, T, L), targets_of(umax, L)


def lattice_case(be: Backend, name, umax, T, L, mode, want_cls=False, show=None) -> dict:
    """Every run of one (call, P, T, L, mode): the three guard poisons give the 0.0 run's bits, and with the edge sequences poisoned
    (NaN, 1e30, and 0.0 as a finite change) every other sequence keeps them.  Returns the 0.0 run."""
    P = SEGMENT[umax]
    assert segment_width(umax) == P and max(TARGET_LENS[umax]) == umax == TARGET_LENS[umax][-1] and (umax == 1 or min(TARGET_LENS[umax]) < umax)
    poisoned = check_edges(P)
    y, targets = lattice_inputs(umax, T, L)
    what = f"{name} P={P} T={T} L={L} {mode}{' cls' if want_cls else ''}"
    base = X.poison_runs(lambda p: lattice_run(be, name, y, targets, mode, p, None, want_cls), what=what)
    for p in X.POISONS:
        got = lattice_run(be, name, y, targets, mode, p, poisoned, want_cls)
        own = [] if show is not None and p != "zero" else None
        X.assert_others_same_bits(got, base, poisoned, SEQ_AXIS, f"{what}, {p} in sequences {poisoned}", own)
        if own:
            main = dict(own)["score" if name == "score" else "value"]
            show.append(f"{what}: poisoned sequences' own {'score' if name == 'score' else 'value'} under {p}: {np.unique(main.astype(np.float64)).tolist()[:4]}")
    return base


# ---- the beam and the greedy decode ----------------------------------------------------------------------------------------------------
def beam_edges(n: int = N_SEQ) -> list:
    """A wave per sequence, four to a workgroup: sequences 0 and n - 1, the last wave of workgroup 0 and the first of workgroup 1.
    n = 45 leaves the last workgroup one live wave and three that repeat sequence n - 1."""
    assert n % BEAM_WAVES == 1 and n // BEAM_WAVES >= 2
    poisoned = sorted({0, BEAM_WAVES - 1, BEAM_WAVES, n - 1})
    assert (BEAM_WAVES - 1) // BEAM_WAVES == 0 and BEAM_WAVES // BEAM_WAVES == 1 and n - 2 not in poisoned and 1 not in poisoned
    return poisoned


def beam_run(be: Backend, y, W, P, M, fill, poisoned=None) -> dict:
    n, T, L = y.shape
    body = y if poisoned is None else X.poison_sequences(y, poisoned, fill)
    steps = X.Guarded(body, fill, width=steps_guard(T, L), device=be.device)
    outs = X.guarded_outputs({"labels": ((n, P, M), np.int32), "lengths": ((n, P), np.int32), "prob": ((n, P), np.float32)}, be.device)
    what = f"beam T={T} L={L} W={W} P={P} ({fill}{'' if poisoned is None else f', sequences {list(poisoned)} poisoned'})"
    be.sync()
    be.beam(steps.ptr, n, T, L, W, P, M, outs)
    be.sync()
    steps.check_guards(f"{what}: steps")
    return X.read_outputs(outs, what)


def beam_inputs(T, L):
    """``(steps [45, T, L], max_labels)`` of a case."""
    return tables(7500 + 10 * T + L, N_SEQ, T, L), min(T, 5)


def beam_case(be: Backend, T, L, W, P, show=None) -> dict:
    poisoned = beam_edges()
    y, M = beam_inputs(T, L)
    what = f"beam T={T} L={L} W={W} top_paths={P}"
    base = X.poison_runs(lambda p: beam_run(be, y, W, P, M, p), what=what)
    for p in X.POISONS:
        got = beam_run(be, y, W, P, M, p, poisoned)
        own = [] if show is not None and p != "zero" else None
        X.assert_others_same_bits(got, base, poisoned, SEQ_AXIS, f"{what}, {p} in sequences {poisoned}", own)
        if own:
            d = dict(own)
            show.append(f"{what}: poisoned sequences' own first path under {p}: lengths {np.unique(d['lengths'][:, 0]).tolist()}, "
                        f"prob {np.unique(d['prob'][:, 0].astype(np.float64)).tolist()[:4]}")
    return base


def greedy_edges(n: int = GREEDY_N) -> list:
    assert GREEDY_BLOCK < n < 2 * GREEDY_BLOCK
    return sorted({0, GREEDY_BLOCK - 1, GREEDY_BLOCK, n - 1})


def greedy_run(be: Backend, y, M, fill, poisoned=None) -> dict:
    n, T, L = y.shape
    body = y if poisoned is None else X.poison_sequences(y, poisoned, fill)
    steps = X.Guarded(body, fill, width=steps_guard(T, L), device=be.device)
    outs = X.guarded_outputs({"labels": ((n, M), np.int32), "lengths": ((n,), np.int32)}, be.device)
    what = f"greedy T={T} L={L} ({fill}{'' if poisoned is None else f', sequences {list(poisoned)} poisoned'})"
    be.sync()
    be.greedy(steps, n, T, L, M, outs)
    be.sync()
    steps.check_guards(f"{what}: steps")
    return X.read_outputs(outs, what)


def greedy_inputs(T, L):
    return tables(7600 + 10 * T + L, GREEDY_N, T, L), min(T, 3)


def greedy_case(be: Backend, T, L) -> dict:
    poisoned = greedy_edges()
    y, M = greedy_inputs(T, L)
    what = f"greedy T={T} L={L}"
    base = X.poison_runs(lambda p: greedy_run(be, y, M, p), what=what)
    for p in X.POISONS:
        X.assert_others_same_bits(greedy_run(be, y, M, p, poisoned), base, poisoned, SEQ_AXIS, f"{what}, {p} in sequences {poisoned}")
    return base
