"""tests/extents.py can fail: NumPy stand-ins of a zero-padded window op and of a per-segment smoothing, clean and with the four
mistakes the GPU test (tests/test_gpu_extents.py) is there to notice.  No GPU.

The window op is the shape of the library's CRNN front: window ``w`` is ``valid[w]`` rows of a mel buffer from row ``win_row[w]``,
zero padded to ``T`` rows; a conv over time (``KT`` rows, stride 1), a ReLU, a mean and a sigmoid give one value per window.  The
stand-ins index the ALLOCATION of a ``Guarded`` (guards included), as a kernel indexes memory: a mistaken index lands in a guard, not
in a Python exception.  The ReLU comes in the two forms hardware offers - one that propagates a NaN (``np.maximum``) and the
``v_max_f32`` form that returns the other operand (``np.fmax``) - because the second launders a NaN poison into the baseline's 0."""
import numpy as np
import pytest

import events64 as E
import extents as X

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
