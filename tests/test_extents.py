"""tests/extents.py can fail: NumPy stand-ins of a zero-padded window op and of a per-segment smoothing, clean and with the four
mistakes the GPU test (tests/test_gpu_extents.py) is there to notice.  No GPU.

The window op is the shape of the library's CRNN front: window ``w`` is ``valid[w]`` rows of a mel buffer from row ``win_row[w]``,
zero padded to ``T`` rows; a conv over time (``KT`` rows, stride 1), a ReLU, a mean and a sigmoid give one value per window.  The
stand-ins index the ALLOCATION of a ``Guarded`` (guards included), as a kernel indexes memory: a mistaken index lands in a guard, not
in a Python exception.  The ReLU comes in the two forms hardware offers - one that propagates a NaN (``np.maximum``) and the
``v_max_f32`` form that returns the other operand (``np.fmax``) - because the second launders a NaN poison into the baseline's 0.

Further down: a stand-in of the segmented CTC lattice (pairs packed P lanes apart, neighbours by a shift of the whole vector) in three
variants - edge lanes that select 0 (passes), that multiply by a 0 mask (fails under the NaN alone), and a tail segment that stores
(trips the output guard) - and the library's host functions ``ww_ctc_{score,align,beam,occupancy}_rows`` through every layout and
assertion that tests/test_gpu_extents_ctc.py makes of the device kernels (tests/extents_ctc.py states them once for both)."""
import numpy as np
import pytest

import ctc64
import events64 as E
import extents as X
import extents_ctc as EC

T, F, KT = 24, 8, 4
VALID = [T, 0, T, 1, 9, T - 1, T, 9]
GAPS = [0, 4, 3, 11, 5, 7, 3, 0]          # in front of each window; window 7 is laid inside window 6: both end on the last row
RNG = np.random.default_rng(41)
W = RNG.normal(0, 0.4, (KT, F)).astype(np.float32)
B = np.float32(0.3)
CONTENT = RNG.uniform(0.0, 6.5, (len(VALID), T, F)).astype(np.float32)


def window_op(mel: X.Guarded, mel_rows, win_row, valid, out: X.Guarded, n, relu, mutant=None, clamp_input=False):
    """``out[w] = sigmoid(mean(relu(conv(window w))))`` for ``w < n``.  ``mutant``: ``"mask"`` pads by ``window * mask`` instead of
    selecting, ``"field"`` lets the staged rows reach one row past ``valid``, ``"store"`` writes one row past ``n``.  ``clamp_input``:
    the staged values pass ``fmax(x, 0)`` first (a no-op on log-mel, which is not negative)."""
    m, o = mel.buf, out.buf                       # flat allocations; the body starts at .width
    for w in range(n + (mutant == "store")):
        ww = min(w, n - 1)
        row, v = int(win_row[ww]), max(0, min(int(valid[ww]), T, mel_rows - int(win_row[ww])))
        img = np.zeros((T, F), np.float32)
        if mutant == "mask":
            base = mel.width + row * F
            raw = m[base:base + T * F].reshape(T, F)          # (the guard is wider than a window: inside the allocation)
            img = raw * (np.arange(T) < v)[:, None].astype(np.float32)
        else:
            take = min(T, v + (mutant == "field"))
            base = mel.width + row * F
            img[:take] = m[base:base + take * F].reshape(take, F)
        if clamp_input:
            img = np.fmax(img, np.float32(0))
        with np.errstate(over="ignore", invalid="ignore"):
            pre = np.array([np.float32((img[t:t + KT] * W).sum(dtype=np.float32) + B) for t in range(T - KT + 1)], np.float32)
            y = np.float32(relu(pre, np.float32(0)).mean(dtype=np.float32))
            o[out.width + w] = np.float32(1) / (np.float32(1) + np.exp(-y * np.float32(0.25)))


def run_windows(poison, relu, mutant=None, clamp_input=False):
    row, rows, named = X.window_layout(VALID, GAPS, T, tail_pair=(6, 7))
    body = np.zeros((rows, F), np.float32)
    for w in (0, 1, 2, 3, 4, 5, 6):               # (window 7 names the last 9 rows of window 6)
        body[row[w]:row[w] + VALID[w]] = CONTENT[w, :VALID[w]]
    mel = X.Guarded(X.poison_rows(body, named, poison), poison, width=(T + 1) * F)
    out = X.Guarded(np.full(len(VALID), X.SENTINEL, np.float32), X.SENTINEL)
    window_op(mel, rows, row, VALID, out, len(VALID), relu, mutant, clamp_input)
    mel.check_guards(f"mel ({poison})")
    out.check_guards(f"out ({poison}, {mutant})")
    return {"out": out.read()}


def test_layout_is_what_the_gpu_test_states():
    row, rows, named = X.window_layout(VALID, GAPS, T, tail_pair=(6, 7))
    assert row[6] + T == rows and row[7] + 9 == rows              # a full and a partial window end on the last row
    spans = sorted((int(row[w]), int(row[w]) + VALID[w]) for w in range(7) if VALID[w])
    assert all(a[1] < b[0] for a, b in zip(spans, spans[1:]))    # disjoint, at least one unnamed row between them
    assert int(named.sum()) == sum(VALID[:7]) and not named[row[3] + 1] and not named[row[1]]
    g = X.Guarded(np.zeros((3, 5), np.float32), "nan", width=1)
    assert g.width == 64 and g.ptr % 256 == g.buf.ctypes.data % 256 and np.isnan(g.buf[:64]).all() and np.isnan(g.buf[-64:]).all()
    assert X.Guarded(np.zeros(7, np.int16), "square", width=1).width == 128
    assert X.same_bits(np.float32([np.nan, 0.0]), np.float32([np.nan, 0.0])) and not X.same_bits(np.float32([0.0]), np.float32([-0.0]))


@pytest.mark.parametrize("relu", [np.maximum, np.fmax], ids=["nan-propagating relu", "v_max relu"])
def test_clean_window_op_passes_every_poison(relu):
    base = X.poison_runs(lambda p: run_windows(p, relu), what="clean")
    out = base["out"]
    assert np.isfinite(out).all() and len(set(out.tolist())) >= 6
    # the reference of the op on explicit zero-padded windows: the same arithmetic on a buffer without neighbours
    for w, v in enumerate(VALID):
        cut = np.zeros((T, F), np.float32)
        cut[:v] = CONTENT[6 if w == 7 else w, (T - 9 if w == 7 else 0):][:v]
        mel, o = X.Guarded(cut, 0.0, width=(T + 1) * F), X.Guarded(np.zeros(1, np.float32), 0.0)
        window_op(mel, T, [0], [T], o, 1, relu)
        assert X.same_bits(o.read()[0], out[w]), w


@pytest.mark.parametrize("relu", [np.maximum, np.fmax], ids=["nan-propagating relu", "v_max relu"])
@pytest.mark.parametrize("mutant", ["mask", "field", "store"])
def test_window_mutants_are_rejected(mutant, relu):
    with pytest.raises(AssertionError, match="guard" if mutant == "store" else "poison"):
        X.poison_runs(lambda p: run_windows(p, relu, mutant), what=mutant)


def test_each_poison_alone_misses_a_mutant():
    """``window * mask``: 1e30 * 0 is 0, only the NaN shows it.  A field one row past ``valid`` whose values pass a ``v_max`` ReLU on
    the way in: the NaN comes out as the baseline's 0 and only 1e30 shows it.  The three poisons together reject both."""
    X.poison_runs(lambda p: run_windows(p, np.maximum, "mask"), poisons=("1e30", "zero"), what="mask")
    with pytest.raises(AssertionError, match="nan poison"):
        X.poison_runs(lambda p: run_windows(p, np.maximum, "mask"), poisons=("nan", "zero"), what="mask")
    X.poison_runs(lambda p: run_windows(p, np.fmax, "field", clamp_input=True), poisons=("nan", "zero"), what="laundered")
    with pytest.raises(AssertionError, match="1e30 poison"):
        X.poison_runs(lambda p: run_windows(p, np.fmax, "field", clamp_input=True), poisons=("1e30", "zero"), what="laundered")
    with pytest.raises(AssertionError, match="1e30 poison"):
        X.poison_runs(lambda p: run_windows(p, np.fmax, "field", clamp_input=True), what="laundered")


# ---------------------------------------------------------------------------------------------------- smoothing over segments
N, WIN = 200, 7
POST = np.random.default_rng(43).uniform(0, 1, N).astype(np.float32)


def smooth_op(post: X.Guarded, offs, win, out: X.Guarded, mutant=False):
    """``out[i]`` = the ascending fp64 chain of include/wwhip.h over the window clipped to row i's segment; rows outside every segment
    are not written.  ``mutant``: the clip's lower end is one element too low."""
    p, o = post.buf, out.buf
    for a, b in zip(offs[:-1], offs[1:]):
        for i in range(a, b):
            hi = i + (win - 1) // 2
            lo = hi - (win - 1)
            acc = 0.0
            for j in range(max(lo, a - (1 if mutant else 0)), min(hi, b - 1) + 1):
                acc += float(p[post.width + j]) * (1.0 / win)
            o[out.width + i] = acc


SEGS = np.array([3, 40, 40, 97, 100, 130], np.int64)          # five segments back to back, one empty; rows 0..2 and 130..199 are in none
IN_SEG = np.zeros(N, bool)
IN_SEG[3:130] = True


def run_smooth(poison, mutant=False):
    post = X.Guarded(X.poison_rows(POST, IN_SEG, poison), poison)
    out = X.Guarded(np.full(N, X.SENTINEL, np.float64), X.SENTINEL)
    smooth_op(post, SEGS, WIN, out, mutant)
    post.check_guards("post")
    out.check_guards("smoothed")
    return {"smoothed": out.read()}


def test_clean_smoothing_passes_and_is_the_float64_statement():
    sm = X.poison_runs(lambda p: run_smooth(p), poisons=("nan", "zero"), what="smoothing")["smoothed"]
    assert (sm[~IN_SEG] == X.SENTINEL).all()
    for a, b in zip(SEGS[:-1], SEGS[1:]):
        np.testing.assert_allclose(sm[a:b], E.smooth(POST[a:b], WIN), rtol=0, atol=1e-15)


def test_smoothing_that_reads_one_element_before_its_segment_is_rejected():
    with pytest.raises(AssertionError, match="nan poison"):
        X.poison_runs(lambda p: run_smooth(p, mutant=True), poisons=("nan", "zero"), what="smoothing")


# ---------------------------------------------------------------------------------------------------- the segmented CTC lattice
# The shape of ctc_score_kernel (csrc/ctc_score.hip): the forward recursion of every (sequence, target) pair in ONE flat vector of
# lanes, pair j in lanes [j P, (j + 1) P), a(s - 1) and a(s - 2) fetched by a shift of the WHOLE vector - so what lane 0 and lane 1 of
# a segment receive is the neighbour pair's.  The grid is rounded up to whole workgroups of 256 / P segments; a segment past the last
# pair repeats the last pair's work.  Scores go to ``out[pair]`` (the bank's [windows][K] layout).
LAT_P, LAT_UMAX = 4, 1       # 2 U + 1 = P - 1: lane P - 2 of a segment is live, and a shift by 2 brings it to the next segment's lane 0


def lattice_op(steps: X.Guarded, n, T, L, targets, out: X.Guarded, variant=None, P=LAT_P):
    """``variant``: ``None`` - the edge lanes SELECT 0; ``"mask"`` - they multiply what the shift brought by a 0 mask; ``"tail"`` - a
    segment past the last pair stores its repeat."""
    k_n = len(targets)
    total, per = n * k_n, 256 // P
    segs = -(-total // per) * per
    lane = np.arange(segs * P)
    s, raw = lane % P, lane // P
    pair = np.minimum(raw, total - 1)
    i, k = pair // k_n, pair % k_n
    tab = np.array([list(c) + [0] * (EC.NU - len(c)) for c in targets])
    U = np.array([len(c) for c in targets])[k]
    on, odd, u = s < 2 * U + 1, (s % 2 == 1), np.minimum(np.maximum(s - 1, 0) // 2, EC.NU - 1)
    cls = np.where(on & odd, tab[k, u], L - 1)
    skip = on & odd & (u >= 1) & (tab[k, u] != tab[k, np.maximum(u - 1, 0)])
    dt = out.dtype                                # the arithmetic's type: float32 as the kernel's, or float64 (below)
    m, o, zero = steps.buf.astype(dt), out.buf, dt.type(0)
    col = steps.width + i * T * L + cls

    def shr(v, d):
        return np.concatenate([np.zeros(d, dt), v[:-d]])
    a = np.where(on & (s <= 1), m[col], zero)
    with np.errstate(over="ignore", invalid="ignore"):
        for t in range(1, T):
            y, a1, a2 = m[col + t * L], shr(a, 1), shr(a, 2)
            if variant == "mask":
                a1, a2 = a1 * (s >= 1).astype(dt), a2 * skip.astype(dt)
            else:
                a1, a2 = np.where(s >= 1, a1, zero), np.where(skip, a2, zero)
            a = np.where(on, ((a + a1) + a2) * y, zero)
        exact = a + shr(a, 1)
    store = (s == 2 * U) & ((raw < total) | (variant == "tail"))
    o[out.width + raw[store]] = exact[store]


def run_lattice(poison, variant=None, poisoned=None, T=4, L=4, dtype=np.float32, umax=LAT_UMAX):
    n, targets = EC.N_SEQ, EC.targets_of(umax, L)
    y = EC.tables(45, n, T, L)
    body = y if poisoned is None else X.poison_sequences(y, poisoned, poison)
    steps = X.Guarded(body, poison, width=EC.steps_guard(T, L))
    outs = X.guarded_outputs({"score": ((n, EC.K), dtype)})
    lattice_op(steps, n, T, L, targets, outs["score"], variant, EC.SEGMENT[umax])
    steps.check_guards(f"steps ({poison})")
    return X.read_outputs(outs, f"lattice stand-in ({poison}, {variant})")


def lattice_standin_case(variant, poisons, T=4, dtype=np.float32, umax=LAT_UMAX):
    poisoned = EC.check_edges(EC.SEGMENT[umax])
    base = X.poison_runs(lambda p: run_lattice(p, variant, None, T, dtype=dtype, umax=umax), what=f"stand-in {variant}")
    for p in poisons:
        X.assert_others_same_bits(run_lattice(p, variant, poisoned, T, dtype=dtype, umax=umax), base, poisoned, {"score": 0},
                                  f"stand-in {variant}, {p} poison")
    return base


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("T", [1, 2, 4, 9, 19])
def test_lattice_standin_that_selects_passes_and_is_the_statement(T, dtype):
    from wwhip import ctc
    got = lattice_standin_case(None, tuple(X.POISONS), T, dtype)["score"]
    want = ctc.score(EC.tables(45, EC.N_SEQ, T, 4), EC.targets_of(LAT_UMAX, 4), "exact", dtype)
    X.assert_same_bits(got, np.ascontiguousarray(want.T), f"the stand-in against wwhip.ctc.score in {np.dtype(dtype)}, T = {T}")
    assert T < 2 or (got > 0).sum() > got.size // 2


def test_lattice_standin_that_masks_fails_under_the_nan_alone():
    """Lane 0 of a segment multiplies the neighbour's a(2U) by a 0 mask: 0 * NaN is NaN, 0 * 1e30 is 0.  The neighbour's a(2U) is
    not 0 from step 1 on, leaks into lane 0 at step 2 and reaches the score's lanes at step 3: T = 4.  In float32 a sequence of 1e30
    has overflowed by then (1e30 * 1e30), and 0 * Inf is NaN too - there both poisons show the mistake; the arithmetic in float64,
    where 1e30^4 is finite, shows what the 1e30 poison alone is worth against this mistake: nothing."""
    lattice_standin_case("mask", ("1e30", "zero"), dtype=np.float64)
    with pytest.raises(AssertionError, match="nan poison"):
        lattice_standin_case("mask", ("nan",), dtype=np.float64)
    lattice_standin_case("mask", tuple(X.POISONS), T=3)      # (one step too few for the leak to reach a score)
    for p in ("nan", "1e30"):
        with pytest.raises(AssertionError, match=f"{p} poison"):
            lattice_standin_case("mask", (p,))


@pytest.mark.parametrize("umax", list(EC.SEGMENT))
def test_lattice_standin_at_every_segment_width(umax):
    """The stand-in at the widths and target lengths of section E, T = 19: the select passes and is the float32 statement; the 0 mask
    is rejected wherever a shift can reach across two pairs at all - P = 4, 8, 16, where the longest target fills P - 1 lanes and is
    the sequence's last.  At P = 32 the 13 idle lanes of a segment keep a shift by 2 to itself, and the mask goes unnoticed."""
    from wwhip import ctc
    got = lattice_standin_case(None, tuple(X.POISONS), 19, umax=umax)["score"]
    want = ctc.score(EC.tables(45, EC.N_SEQ, 19, 4), EC.targets_of(umax, 4), "exact", np.float32)
    X.assert_same_bits(got, np.ascontiguousarray(want.T), f"the stand-in against wwhip.ctc.score in float32, Umax = {umax}")
    if EC.SEGMENT[umax] < 32:
        with pytest.raises(AssertionError, match="nan poison"):
            lattice_standin_case("mask", ("nan",), 19, umax=umax)
    else:
        lattice_standin_case("mask", tuple(X.POISONS), 19, umax=umax)


def test_lattice_standin_whose_tail_segments_store_trips_the_output_guard():
    """The repeat carries the last pair's value: in the body nothing would show.  Only the guard behind ``out`` does."""
    with pytest.raises(AssertionError, match="back guard"):
        run_lattice("zero", "tail")


# ---------------------------------------------------------------------------------------------------- the host twins, section E's cases
@pytest.fixture(scope="module")
def host():
    return EC.Backend()


@pytest.mark.parametrize("umax", list(EC.SEGMENT))
@pytest.mark.parametrize("name", ["score", "align", "occupancy"])
def test_host_lattice_functions_pass_section_e(host, name, umax):
    """``ww_ctc_{score,align,occupancy}_rows`` through every layout and assertion the device kernels get
    (tests/test_gpu_extents_ctc.py): the cases are well formed, and the reference itself keeps every sequence to itself."""
    for T in EC.TS:
        for L in ctc64.LS:
            for mode in EC.MODES:
                base = EC.lattice_case(host, name, umax, T, L, mode)
                assert np.isfinite(base["score" if name == "score" else "value"]).all()
                if name == "occupancy" and mode == "exact":
                    both = EC.lattice_case(host, name, umax, T, L, mode, want_cls=True)
                    for k in base:
                        X.assert_same_bits(both[k], base[k], f"occupancy {k} with and without cls")
    live = EC.lattice_case(host, name, umax, 19, 4, "prefix")["score" if name == "score" else "value"]
    assert (live > 0).sum() > live.size // 2     # (the cases are not all-zero scores)


@pytest.mark.parametrize("W", [1, 8, 64])
def test_host_beam_function_passes_section_e(host, W):
    for T in EC.BEAM_TS:
        for L in ctc64.LS:
            for P in sorted({1, min(W, 8)}):     # top_paths is at most min(beam_width, WW_CTC_BEAM_MAX_PATHS = 8)
                base = EC.beam_case(host, T, L, W, P)
                assert (base["lengths"][:, 0] >= 0).all() and (base["prob"][:, 0] > 0).all()


def test_greedy_statement_passes_section_e(host):
    for T in EC.TS:
        for L in ctc64.LS:
            base = EC.greedy_case(host, T, L)
            assert (base["lengths"] >= 0).all() and (base["lengths"] <= T).all()
