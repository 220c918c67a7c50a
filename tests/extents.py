"""The extent of a call: which rows it may let into its result and which bytes it may write.  The harness of
tests/test_extents.py (NumPy stand-ins: the harness must be able to fail), tests/test_gpu_extents.py and
tests/test_gpu_extents_ctc.py (the library's device calls).

A buffer handed to a call is a ``Guarded``: ONE allocation laid out as ``[front guard | body | back guard]``, of which the call gets
the body's address and the body's extent.  Every address a test hands over therefore lies inside memory the test owns, and so does an
over-read or over-write of up to a guard's width; nothing here provokes a fault.

  inputs   the guards and every body row the call does not name hold a POISON, and the call runs once per poison: ``nan``, ``1e30``
           and ``zero``.  The ``zero`` run is the baseline; the other two must give ITS BITS (``same_bits`` - integer views, no
           tolerance).  Two poisons because one can be laundered: a ReLU written as ``max(x, 0)`` the way ``v_max_f32`` evaluates it
           returns the other operand for a NaN, so a NaN that leaks into a pre-activation comes out as 0 - exactly what the baseline
           holds; 1e30 survives the ReLU.  The other way round, a kernel that zeroes a pad by multiplying with a 0 mask, or loads a
           spare row against zero weights, shows under the NaN alone: 0 * NaN is NaN, 0 * 1e30 is 0.  (tests/test_extents.py pins
           both cases.)
           int16 PCM has no NaN: its poisons are a full-scale +-32767 square wave and zeros.
           A call whose every row is named (the CTC lattice calls read all of ``steps [n][T][L]``) gets a second kind of run: some
           SEQUENCES of the body hold the poison (``poison_sequences``) and every other sequence's outputs must carry the clean
           run's bits (``assert_others_same_bits``); what the poisoned sequences' own rows hold is reported, not asserted.
  outputs  the guards hold a sentinel (-7) and ``check_guards`` asserts that every guard byte is what it was.

What the poison runs do NOT show: an over-read whose value is discarded (loaded and never used, or used only in lanes whose results
are dropped).  That is legal as long as the address lies in the caller's buffer, and only the address arithmetic can say so."""
import numpy as np

SENTINEL = -7.0
POISONS = {"nan": float("nan"), "1e30": 1e30, "zero": 0.0}   # "zero" last: callers index by name, the order is the run order
PCM_POISONS = ("square", "zero")
_UINT = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}


def bits(a):
    """``a`` as unsigned integers of its item size (float32 -> uint32, as tests/test_gpu_stream_rate.py's ``_bits``); a structured
    array as bytes."""
    a = np.ascontiguousarray(a)
    if a.dtype.fields is not None or a.dtype.itemsize not in _UINT:
        return a.reshape(-1).view(np.uint8)
    return a.view(_UINT[a.dtype.itemsize])


def same_bits(a, b) -> bool:
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and bool(np.array_equal(bits(a), bits(b)))


def assert_same_bits(got, want, what: str) -> None:
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    x, y = bits(got).reshape(-1), bits(want).reshape(-1)
    if not np.array_equal(x, y):
        bad = np.flatnonzero(x != y) // (x.size // max(got.size, 1))
        at = np.unravel_index(int(bad[0]), got.shape) if got.ndim else ()
        raise AssertionError(f"{what}: {len(np.unique(bad))} of {got.size} elements differ, the first at {tuple(int(i) for i in at)}: "
                             f"got {got[at]!r}, want {want[at]!r}")


def pcm_square(n: int, half_period: int = 40) -> np.ndarray:
    """``n`` int16 samples of a full-scale square wave (+32767 / -32767, 200 Hz at 16 kHz): energy in every band of the front end."""
    return np.where((np.arange(n) // half_period) % 2 == 0, 32767, -32767).astype(np.int16)


def fill_of(poison, dtype, n: int) -> np.ndarray:
    """``n`` guard elements of ``dtype`` for a poison's name (``POISONS`` / ``PCM_POISONS``) or a number (the sentinel)."""
    if isinstance(poison, str):
        if poison == "square":
            return pcm_square(n).astype(dtype)
        poison = POISONS[poison]
    return np.full(n, poison, dtype)


def guard_width(min_elems: int, dtype) -> int:
    """The smallest width >= ``min_elems`` that is a multiple of 64 elements AND of 256 bytes: the body keeps the allocation's
    alignment."""
    unit = max(64, 256 // np.dtype(dtype).itemsize)
    return max(1, -(-int(min_elems) // unit)) * unit


class Guarded:
    """``[front guard | body | back guard]`` in one allocation: a NumPy array (``device=False``) or a torch tensor on the GPU.

    ``body``   the initial body (any shape; copied); ``fill`` what the guards hold: a poison's name or a number;
    ``width``  the least guard width in elements (rounded up by ``guard_width``).
    ``ptr``    the body's address: what the call gets.  ``body`` / ``read()``: the live body / a host copy of it.
    ``check_guards(what)``: every guard byte is what the constructor wrote."""

    def __init__(self, body, fill, width: int = 64, device: bool = False):
        body = np.ascontiguousarray(body)
        self.shape, self.dtype, self.n = body.shape, body.dtype, body.size
        self.width = guard_width(width, body.dtype)
        self._front = fill_of(fill, body.dtype, self.width)
        self._back = self._front.copy()
        host = np.concatenate([self._front, body.reshape(-1), self._back])
        assert host.size == self.n + 2 * self.width and (self.width * body.dtype.itemsize) % 256 == 0
        self.device = bool(device)
        if device:
            import torch
            self.buf = torch.from_numpy(host).cuda()
            assert self.buf.data_ptr() % 256 == 0
            self.ptr = self.buf.data_ptr() + self.width * body.dtype.itemsize
        else:
            self.buf = host
            self.ptr = host.ctypes.data + self.width * body.dtype.itemsize

    @property
    def body(self):
        """The live body (a view of the allocation) in the body's shape."""
        return self.buf[self.width:self.width + self.n].reshape(self.shape)

    def _host(self) -> np.ndarray:
        return self.buf.cpu().numpy() if self.device else self.buf

    def read(self) -> np.ndarray:
        return self._host()[self.width:self.width + self.n].reshape(self.shape).copy()

    def check_guards(self, what: str) -> None:
        h = self._host()
        for name, got, want in (("front", h[:self.width], self._front), ("back", h[self.width + self.n:], self._back)):
            x, y = bits(got), bits(want)
            if not np.array_equal(x, y):
                bad = np.flatnonzero(x != y)
                raise AssertionError(f"{what}: {len(bad)} elements of the {name} guard were written, the first at guard element "
                                     f"{int(bad[0])} (now {got[bad[0]]!r})")


def poison_rows(rows: np.ndarray, named: np.ndarray, poison) -> np.ndarray:
    """A copy of ``rows`` (first axis: rows) whose rows outside the boolean mask ``named`` hold the poison."""
    out = np.array(rows, copy=True)
    out[~np.asarray(named, bool)] = fill_of(poison, out.dtype, 1)[0]
    return out


def poison_runs(run, poisons=tuple(POISONS), what: str = ""):
    """``run(poison)`` once per poison; it returns a dict of host arrays (and has checked its own guards).  Every run must give the
    bits of the LAST poison's run (the baseline: ``zero``), which is returned."""
    got = {p: run(p) for p in poisons}
    base = got[poisons[-1]]
    for p in poisons[:-1]:
        assert got[p].keys() == base.keys()
        for k in base:
            assert_same_bits(got[p][k], base[k], f"{what}: {k} under the {p} poison against the {poisons[-1]} baseline")
    return base


def poison_sequences(steps: np.ndarray, which, poison) -> np.ndarray:
    """A copy of ``steps`` (first axis: sequences) in which the sequences in ``which`` hold the poison in EVERY element.  For calls
    whose every row is named (the CTC lattice calls take ``steps [n][T][L]`` and read all of it): the guards' poison says nothing
    about a leak between two sequences of the body, a poisoned sequence beside a clean one does."""
    out = np.array(steps, copy=True)
    which = sorted(int(i) for i in which)
    assert which and 0 <= which[0] and which[-1] < len(out), (which, len(out))
    out[which] = fill_of(poison, out.dtype, 1)[0]
    return out


def assert_others_same_bits(got: dict, base: dict, which, axes: dict, what: str, show=None) -> None:
    """The comparison of a poisoned-sequence run: every output of ``got`` carries the bits of ``base`` on every index of its sequence
    axis (``axes[name]``) that is NOT in ``which``.  The poisoned sequences' own rows are not asserted - the reference does not define
    them; ``show`` (a list) receives ``(name, own rows)`` for the caller to print."""
    assert got.keys() == base.keys(), (what, sorted(got), sorted(base))
    for k in base:
        n = base[k].shape[axes[k]]
        keep = np.ones(n, bool)
        keep[sorted(int(i) for i in which)] = False
        assert keep.any()
        a, b = np.compress(keep, got[k], axis=axes[k]), np.compress(keep, base[k], axis=axes[k])
        assert_same_bits(a, b, f"{what}: {k}, the sequences other than the poisoned {sorted(int(i) for i in which)}")
        if show is not None:
            show.append((k, np.compress(~keep, got[k], axis=axes[k])))


def guarded_outputs(spec: dict, device: bool = False, rows: int = 2) -> dict:
    """``{name: (shape, dtype)}`` -> ``{name: Guarded}``, each body and each guard full of the sentinel in the output's own dtype
    (float32 value / occ / cls / prob, int8 span, int32 labels / lengths: -7 is a value of all of them).  A guard is ``rows`` rows of
    the output (everything behind its first axis), at least 256 elements: a row or a plane stored behind the extent lands in it."""
    out = {}
    for name, (shape, dtype) in spec.items():
        width = max(256, int(rows) * int(np.prod(shape[1:], dtype=np.int64)))
        out[name] = Guarded(np.full(shape, SENTINEL, dtype), SENTINEL, width=width, device=device)
    return out


def read_outputs(outs: dict, what: str) -> dict:
    """Every output's guards checked, then ``{name: host copy of the body}``."""
    for name, g in outs.items():
        g.check_guards(f"{what}: {name}")
    return {name: g.read() for name, g in outs.items()}


def window_layout(valid, gaps, T: int, tail_pair=None):
    """Rows for a list of windows in one mel body.  Window ``w`` names ``valid[w]`` rows; the windows lie in list order, ``gaps[w]``
    unnamed rows in front of window ``w``, and nothing behind the last one: it ends on the body's last row.  ``tail_pair = (a, b)``:
    window ``a`` is laid out behind all others, and window ``b`` (a partial one) ends on the body's last row too, inside the rows of
    window ``a`` - the one pair of windows that shares rows (two windows that end on the same row cannot be disjoint).  Returns
    ``(win_row int64[n], body_rows, named bool[rows])``."""
    n = len(valid)
    row = np.zeros(n, np.int64)
    order = list(range(n))
    if tail_pair is not None:
        a, b = tail_pair
        assert valid[b] <= valid[a]
        order = [w for w in order if w not in (a, b)] + [a]
    at = 0
    for w in order:
        at += int(gaps[w])
        row[w] = at
        at += min(int(valid[w]), T)
    if tail_pair is not None:
        row[b] = at - int(valid[b])
    named = np.zeros(at, bool)
    for w in range(n):
        named[row[w]:row[w] + min(int(valid[w]), T)] = True
    return row, at, named
