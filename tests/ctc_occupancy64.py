"""What the forward-backward occupancy tests share (host only): path enumeration of ``occ`` and ``cls`` in both modes, the seeded
tables of the native check and the device test, and the derived bounds.

Bounds.  ``csrc/ctc_occupancy.h`` computes ``g = (a b) / Z`` from sums of non-negative products, so roundings only accumulate as
relative errors (``u = 2^-24`` each).  Counting what the header writes, on the SAME float32 posteriors:

- ``a_t(s)`` passes through 3 roundings a step (two additions, one product): ``3 t``.
- ``b_t(s)`` likewise, a product and two additions a step from ``T - 1`` down: ``3 (T - 1 - t)``.
- ``Z``, exact mode: ``3 (T - 1)`` and the join, ``3 T - 2``.  Prefix mode: ``e_t`` carries ``3 (t - 1) + 2`` and then ``T - t``
  additions of the running sum, ``2 t + T - 1 <= 3 T - 3``.
- the product ``a b`` and the division: 2.

That is ``3 (T - 1) + (3 T - 2) + 2 = 6 T - 3`` roundings for an ``occ`` entry (the completion column ``e_t / Z`` has fewer); the
bound used is the issue's ``(6 T + 4) u g64``, whose 7 spare roundings cover the second-order terms of ``(1 + u)^(6T)`` many times
over.  A ``cls`` entry adds at most ``U`` additions of ``g`` (the blank has ``U + 1`` states): ``2 U`` more, as allowed.

Under ``FLT_MIN``.  A product that lands under ``FLT_MIN`` is rounded to the denormal grid (``2^-150`` off at most) or, where the
hardware flushes, lost (``2^-126`` at most); an addition there is exact.  Such an error enters at one (state, step) node and reaches a
later value scaled by a sum of path products from that node, which is at most 1 (distinct lattice paths are distinct class
sequences).  So ``a_t(s)`` and ``b_t(s)`` are each off by ``(2U + 1) T 2^-126`` at most, the product ``a b`` (both factors at most 1)
by ``(2U + 1) (T - 1) 2^-126`` and its own ``2^-126``, ``Z`` by ``(2U + 1) T 2^-126``.  Through the quotient, with ``g <= 1``:
``|dg| <= (|d(ab)| + g |dZ|) / Z <= 2 (2U + 1) T 2^-126 / Z64``, and the division's own result may round under ``FLT_MIN``:
``+ 2^-149``.  The constant arrived at is therefore ``2 (2U + 1) T``, twice the form the issue sketches (it counts one of the two
directions).  A ``cls`` entry sums up to ``U + 1`` of them.  Where ``Z64`` itself is within a few hundred ``FLT_MIN`` the term
exceeds 1 and the bound says nothing, as it should: the linear domain has run out.

Against the float64 MODEL the posteriors themselves move, each within a relative ``tau + 2^-21`` (``ctc_score64``'s docstring).  ``g``
is a ratio of two sums of positive path products, each product of ``T`` posteriors and so within ``T (tau + 2^-21)`` relative; the
ratio moves by at most twice that, ``2.02 T (tau + 2^-21)`` with 1 % for the second order, on top of the arithmetic bound."""
from __future__ import annotations

import itertools

import numpy as np

import ctc64

MODES = ("exact", "prefix")
NU = 9  # WW_CTC_SCORE_MAX_TARGET: the columns of occ


def enumerate_occupancy(y, c):
    """One ``[T, L]`` table by enumeration of all ``L^T`` paths, in float64 (T <= 6, L <= 4): ``dict(exact=(Z, occ [T, 9],
    cls [T, L]), prefix=(Z, occ [T, 9], None))``, the occupancies already divided by ``Z`` (all 0 where ``Z == 0``).

    Exact: the paths whose collapse is ``c``; a path is on label ``u`` at the steps of its ``u``-th emitted run.  Prefix: the paths
    whose collapse starts with ``c``; up to the step that completes ``c`` they are on their labels as before, that step counts for
    column ``U - 1`` alone, and what follows is free: it belongs to nothing and its posteriors do not enter the product (the
    statement's rule, which is the probability itself where the rows sum to 1)."""
    y = np.asarray(y, np.float64)
    T, L = y.shape
    c, U = list(c), len(c)
    Ze = Zp = 0.0
    occ_e, cls_e, occ_p = np.zeros((T, NU)), np.zeros((T, L)), np.zeros((T, NU))
    for path in itertools.product(range(L), repeat=T):
        out, where, prev = [], [], -1   # the collapse, and per step the index of the label the path is on (-1: a blank)
        for k in path:
            if k != L - 1 and k != prev:
                out.append(k)
            where.append(len(out) - 1 if k != L - 1 else -1)
            prev = k
        if out[:U] != c:
            continue
        p = float(np.prod([y[t, path[t]] for t in range(T)]))
        done = next(t for t in range(T) if where[t] == U - 1)   # the step that completes c
        if not any(path[done + 1:]):   # what follows is free: a completing prefix counts once, with the product up to `done`
            q = float(np.prod([y[t, path[t]] for t in range(done + 1)]))
            Zp += q
            occ_p[done, U - 1] += q
            for t in range(done):
                if where[t] >= 0:
                    occ_p[t, where[t]] += q
        if len(out) == U:
            Ze += p
            for t in range(T):
                cls_e[t, path[t]] += p
                if where[t] >= 0:
                    occ_e[t, where[t]] += p
    if Ze > 0:
        occ_e, cls_e = occ_e / Ze, cls_e / Ze
    if Zp > 0:
        occ_p = occ_p / Zp
    return dict(exact=(Ze, occ_e, cls_e), prefix=(Zp, occ_p, None))


def arithmetic_bound(g64, Z64, steps: int, U: int, classes: bool = False):
    """The bound on ``|float32 g - float64 g|`` over the same float32 posteriors; ``g64 [..., T, *]`` with ``Z64 [...]`` (the module's
    docstring).  ``classes``: a ``cls`` entry."""
    g = np.asarray(g64, np.float64)
    Z = np.asarray(Z64, np.float64)[..., None, None]
    rel = (6 * steps + 4 + (2 * U if classes else 0)) * 2.0 ** -24
    with np.errstate(divide="ignore"):
        absolute = 2 * (2 * U + 1) * steps * 2.0 ** -126 / Z + 2.0 ** -149
    return rel * g + (U + 1 if classes else 1) * np.where(Z > 0, absolute, 0.0)


def model_bound(g64, Z64, U: int, classes: bool = False, tau: float = ctc64.TAU):
    """The bound on ``|the library's g - the float64 model's g|`` at the models' T = 19: the ratio of two sums of path products whose
    posteriors move by ``tau + 2^-21`` each, then the arithmetic."""
    g = np.asarray(g64, np.float64)
    return g * (2.02 * ctc64.STEPS * (tau + 2.0 ** -21)) + arithmetic_bound(g, Z64, ctc64.STEPS, U, classes)


def small_tables(seed: int = 7, n: int = 320):
    """``[(steps [T, L] float64, target)]`` small enough to enumerate (T <= 6, L <= 4, U <= 3): a third on a grid of eighths (exact
    zeros), every fourth target one label repeated."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        T, L, U = int(rng.integers(1, 7)), int(rng.integers(2, 5)), int(rng.integers(1, 4))
        y = rng.dirichlet(np.full(L, 0.6), T)
        if i % 3 == 0:
            y = np.round(y * 8) / 8
        c = rng.integers(0, L - 1, U)
        if i % 4 == 0:
            c[:] = c[0]
        out.append((y, tuple(int(v) for v in c)))
    return out


def random_tables(seed: int = 20263, n: int = 1500):
    """``[(steps [T, L] float32, target)]`` for the native check and the device test: the first tables walk the (T, U) corners, every
    other table is small enough to be enumerated (T <= 6, L <= 4, U <= 2); a third lie on a grid of sixteenths (exact zeros), a third
    carry a blank that wins often; every fourth target is one label repeated."""
    rng = np.random.default_rng(seed)
    corners = [(T, U) for T in (1, 2, 3, 16, 17, 18, 19, 33, 63, 64) for U in (1, 2, 8, 9)]
    out = []
    for i in range(n):
        if i < len(corners):
            (T, U), L = corners[i], int(rng.integers(2, 13))
        elif i % 2:
            T, U, L = int(rng.integers(1, 7)), int(rng.integers(1, 3)), int(rng.integers(2, 5))
        else:
            T, U, L = int(rng.integers(1, 65)), int(rng.integers(1, 10)), int(rng.integers(2, 13))
        s = rng.dirichlet(np.full(L, 0.4), T).astype(np.float32)
        if i % 3 == 0:
            s = np.round(s * 16) / np.float32(16)
        elif i % 3 == 1:
            s[:, L - 1] += np.float32(0.5)
        c = rng.integers(0, L - 1, U)
        if i % 4 == 0:
            c[:] = c[0]
        elif i % 4 == 1 and U >= 2:
            c[1] = c[0]
        out.append((np.ascontiguousarray(s, np.float32), tuple(int(v) for v in c)))
    return out
