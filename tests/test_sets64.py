"""The yardsticks of tests/test_gpu_set_geometry64.py, pinned on the CPU (no GPU, no HIP library).

A set test that compared a member's rows only with the library's own single-model path could not see a launch that ran the right
kernel on the wrong member's weights on BOTH sides, and a float64 comparison sees a wrong member only if the members' float64
readings differ by far more than the bound.  So for every family of ``tests/sets64.py`` and every pair of its members the float64
posteriors in the engine's posterior column differ by more than 100 TAU (4e-3) on at least 90 % of the test windows; ``w-t100-odd``
(softmax of one value: identically 1) is told apart by its float64 logits and encodings, relative to TAU_E.  The standard-conv row
with a head of one sigmoid unit, which ``geometry64.GEOMETRIES`` does not have, is tied to the packer and the C oracle here as
tests/test_host_logic.py and tests/test_geometry64.py tie the table's rows; and the thresholds of the trigger test are shown to
come from the float64 posteriors alone."""
import itertools

import numpy as np
import pytest

import geometry64 as G
import sets64 as S64
from test_geometry64 import TOL_ORACLE
from test_gpu_geometry64 import TAU, TAU_E, TAU_STREAM
from test_host_logic import _geom_words, pack_check  # noqa: F401  (pack_check: the fixture that builds tests/native/model_pack_check.cpp)

SHARE = 0.9


@pytest.mark.parametrize("name", list(S64.ROWS))
def test_members_are_one_geometry_and_one_filter(name):
    """Three members, member 0 the row itself, the seeds sets64 names; equal geometry words and equal filter bytes; different
    weights in blobs of one size."""
    from wwhip import weights as W
    f = S64.family(name)
    assert len(f.bundles) == S64.K and [r.args["seed"] - f.g.args["seed"] for r in f.rows] == list(S64.SEED_OVERRIDES.get(name, (0, 1000, 2000)))
    assert W.pack_blob(f.bundles[0]) == W.pack_blob(f.g.bundle())
    geoms = [G.expected_geometry(b) for b in f.bundles]
    assert geoms[0] == geoms[1] == geoms[2]
    for b in f.bundles[1:]:
        for a in ("weight", "bias"):
            assert getattr(b.filt, a).tobytes() == getattr(f.bundles[0].filt, a).tobytes()
    blobs = [G.blob_of(b) for b in f.bundles]
    assert len(set(blobs)) == S64.K and len({len(b) for b in blobs}) == 1
    assert f.wins.shape == (S64.N_WINDOWS, f.T, f.n_mel) and f.col == (0 if f.n_out == 1 else 1)


@pytest.mark.parametrize("name", list(S64.ROWS))
def test_float64_tells_the_members_apart(name):
    """Every pair of members, on the family's test windows, in float64: |p_a - p_b| in the posterior column above 100 TAU on at
    least 90 % of the windows.  w-t100-odd: max|dz| / max(1, |z|) and max|de| / max(1, max|e|) above 100 TAU_E instead.
    Measured: the share is 100 % for every pair but w-t16's members 1, 2 and w-t183's members 0, 2 (95 %: one window of 20 at 2e-3);
    the smallest median difference is 7.3e-2 (c-std-n1-sigmoid, members 1, 2; w-max 7.8e-2).  w-t183 and w-max run other member seeds than
    seed + 1000, seed + 2000 (sets64.SEED_OVERRIDES says why)."""
    f = S64.family(name)
    for a, b in itertools.combinations(range(S64.K), 2):
        if name == S64.LOGIT_FAMILY:
            assert all((p == 1.0).all() for p in f.post64)
            za, zb = f.logits64(a, f.wins), f.logits64(b, f.wins)
            dz = np.abs(za - zb).max(axis=-1) / np.maximum(1.0, np.maximum(np.abs(za), np.abs(zb)).max(axis=-1))
            ea, eb = f.enc64[a].reshape(len(f.wins), -1), f.enc64[b].reshape(len(f.wins), -1)
            de = np.abs(ea - eb).max(axis=1) / np.maximum(1.0, np.maximum(np.abs(ea), np.abs(eb)).max(axis=1))
            print(f"\nSETS64 {name} members {a}, {b}: median dz {np.median(dz):.2e}, de {np.median(de):.2e}; shares above 100 tau_e "
                  f"{float((dz > 100 * TAU_E).mean()):.0%}, {float((de > 100 * TAU_E).mean()):.0%}", end="")
            assert (dz > 100 * TAU_E).mean() >= SHARE and (de > 100 * TAU_E).mean() >= SHARE
        else:
            d = np.abs(f.post64[a][:, f.col] - f.post64[b][:, f.col])
            print(f"\nSETS64 {name} members {a}, {b}: |dp| median {np.median(d):.2e}, min {d.min():.2e}; share above 100 tau "
                  f"{float((d > 100 * TAU).mean()):.0%}", end="")
            assert (d > 100 * TAU).mean() >= SHARE, (name, a, b)
    for k in range(S64.K):   # and the windows stay useful for every member (tests/test_geometry64.py's condition)
        assert np.isfinite(f.post64[k]).all() and np.isfinite(f.enc64[k]).all()
        if name != S64.LOGIT_FAMILY:
            p = f.post64[k][:, f.col]
            assert (np.minimum(p, 1.0 - p) >= 1e-3).mean() >= SHARE, (name, k)


@pytest.mark.parametrize("name", [n for n, g in S64.ROWS.items() if g.n_out > 1])
def test_float64_tells_the_posterior_column_from_column_0(name):
    """A bank or a trigger that picked its column for another head width (``NOUT == 1 ? 0 : 1``) would read column 0 of these
    heads: for every member, column 0 differs from column ``posterior_index`` by more than 100 TAU on at least 90 % of the test
    windows in float64.  Measured: 100 % everywhere but c-std-n8's member 2 (90 %), c-std-n3-sigmoid's member 1 and w-t1's member 1
    (95 %); the smallest median difference is 1.7e-2 (w-max, member 0)."""
    f = S64.family(name)
    assert f.col == 1
    for k in range(S64.K):
        d = np.abs(f.post64[k][:, 0] - f.post64[k][:, 1])
        print(f"\nSETS64 {name} member {k}: |p[0] - p[1]| median {np.median(d):.2e}, min {d.min():.2e}; share above 100 tau "
              f"{float((d > 100 * TAU).mean()):.0%}", end="")
        assert (d > 100 * TAU).mean() >= SHARE, (name, k)


def test_the_one_unit_standard_row_loads(pack_check):  # noqa: F811
    """``c-std-n1-sigmoid`` (defined in sets64.py, not in GEOMETRIES): every member's blob packs with status 0, the packer prints
    the geometry words ``expected_geometry`` predicts, with ``generic`` = 0 (the standard kernels) and NOUT 1 / HEAD sigmoid; and
    Crnn64 is within tests/test_geometry64.py's bound (1e-4 absolute) of the fp32 C oracle, posteriors and encodings.
    Measured: oracle - float64 posterior 1.2e-7, encoding 3.5e-7."""
    from oracle.cpu import CpuOracle
    f = S64.family("c-std-n1-sigmoid")
    assert f.g.standard and G.oracle_takes(f.g) and f.g.name not in G.GEOMETRIES
    for k, b in enumerate(f.bundles):
        (status, msg, arrays, other), = pack_check(G.blob_of(b))
        assert status == 0 and arrays, (k, status, msg)
        want = G.expected_geometry(b)
        got = _geom_words(other, "crnn")
        assert {key: got[key] for key in want} == want, (k, got, want)
        assert (got["generic"], got["NOUT"], got["HEAD"]) == (0, 1, G.SIG)
        info = _geom_words(other, "info")
        assert (info["window"], info["n_mel"], info["n_out"]) == (151, 40, 1)
        out, enc = CpuOracle(G.blob_of(b)).forward(f.wins, want_enc=True)
        dp, de = np.abs(out - f.post64[k]).max(), np.abs(enc.reshape(f.enc64[k].shape) - f.enc64[k]).max()
        print(f"\nSETS64 c-std-n1-sigmoid member {k}: oracle - float64 posterior {dp:.2e}, encoding {de:.2e}", end="")
        assert dp < TOL_ORACLE and de < TOL_ORACLE


@pytest.mark.parametrize("name", S64.TRIGGER_FAMILIES)
def test_trigger_thresholds_come_from_float64(name):
    """The thresholds of the trigger test: from the float64 posteriors of the bank script alone (``sets64.trigger_thresholds``), no
    float64 posterior within 100 TAU_STREAM (3e-2) of its member's threshold, and on some tick at least one and fewer than all
    member slots fire."""
    f = S64.family(name)
    p = f.trigger_post64()
    rows = (S64.TRIGGER_TICKS * 320 - 512) // 160 + 1
    assert p.shape == (S64.K, S64.TRIGGER_STREAMS, rows) and np.isfinite(p).all()
    thr = S64.trigger_thresholds(p, 100 * TAU_STREAM)
    assert len(thr) == S64.K
    for k in range(S64.K):
        assert np.abs(p[k] - thr[k]).min() > 100 * TAU_STREAM, (name, k)
    over = p > np.array(thr)[:, None, None]
    n_over = over.sum(axis=0)   # [S, rows]: the slots over their threshold on a row
    print(f"\nSETS64 {name} thresholds {[round(t, 4) for t in thr]}: {int((n_over > 0).sum())} of {n_over.size} rows fire, "
          f"{int(((n_over > 0) & (n_over < S64.K)).sum())} with fewer than all slots", end="")
    assert ((n_over > 0) & (n_over < S64.K)).any(), name
    n_post = np.zeros((S64.TRIGGER_TICKS, S64.TRIGGER_STREAMS), int)
    have = 0
    for t in range(S64.TRIGGER_TICKS):
        now = max(0, ((t + 1) * 320 - 512) // 160 + 1)
        n_post[t], have = now - have, now
    events = S64.trigger_expectation(p, thr, n_post)
    assert any(fired for fired, _, _ in events) and any(0 < bin(m).count("1") < S64.K for _, _, ms in events for m in ms)
