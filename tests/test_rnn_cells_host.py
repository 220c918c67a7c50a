"""CRNNs of either recurrent cell without a GPU: the Keras reader (``weights.load_keras_pair`` / ``crnn_from_keras``), the blob format
(the optional ``crnn.cell`` section, an LSTM's missing ``bh``), and the packer's side of it (csrc/model_pack.h) as a stand-alone
program under Address + UB sanitizer (tests/native/rnn_pack_check.cpp, run as a child process: nothing is loaded into this
interpreter)."""
import dataclasses
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CSRC = os.path.join(_ROOT, "wakeword-detection_amd", "csrc")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import geometry64 as G  # noqa: E402
import rnn64 as R  # noqa: E402
from wwhip import weights as W  # noqa: E402

KERAS_PAIRS = [("", "CRNN_softmax"), ("nosilence", "CRNN_nosilence"), ("nosilence_enhanced", "CRNN_nosilence_enhanced")]   # tests/test_h5min.py
WW_EBLOB = -2
INT_MAX = 2 ** 31 - 1
SMALL = dict(T=20, n_mel=40, C=3, KF=8, KT=4, SF=8, ST=2, same=False)   # 9 steps of 15 features: small blobs


def _fields(obj):
    for f in dataclasses.fields(obj):
        v = getattr(obj, f.name)
        if isinstance(v, tuple) and v and dataclasses.is_dataclass(v[0]):
            for i, d in enumerate(v):
                for name, x in _fields(d):
                    yield f"{f.name}[{i}].{name}", x
        else:
            yield f.name, v


def _same_params(a, b):
    for (na, va), (nb, vb) in zip(_fields(a), _fields(b)):
        assert na == nb
        if isinstance(va, np.ndarray):
            assert va.dtype == vb.dtype == np.float32 and va.shape == vb.shape and va.tobytes() == vb.tobytes(), na
        else:
            assert va == vb, (na, va, vb)


# ---- the Keras reader ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sub,asset", KERAS_PAIRS)
def test_keras_pair_is_its_tflite_twin(golden, assets, sub, asset):
    twin = W.load_model_dir(os.path.join(assets, asset))
    kd = os.path.join(golden, "keras_h5", sub)
    got = W.load_keras_pair(os.path.join(kd, "encode.h5"), os.path.join(kd, "detect.h5"), twin.filt)
    _same_params(got.crnn, twin.crnn)
    assert got.crnn.cell == W.CELL_GRU and got.crnn.units == 32 and got.crnn.head_units == 64
    blob = W.pack_blob(got)
    assert blob == W.pack_blob(twin)
    assert "crnn.cell" not in W.unpack_blob(blob)


def _lstm_config(golden, H, F, n_out, rng):
    """The shipped encoder / detector configs rewritten for LSTM cells of H units and a head of F, with weights to match."""
    kd = os.path.join(golden, "keras_h5")
    (ecfg, ew), (dcfg, dw) = W.read_keras_h5(os.path.join(kd, "encode.h5")), W.read_keras_h5(os.path.join(kd, "detect.h5"))
    ecfg, dcfg = json.loads(json.dumps(ecfg)), json.loads(json.dumps(dcfg))
    new_w = {k: v for k, v in ew.items() if k.startswith("conv2d/")}
    n = lambda *s: (0.1 * rng.normal(size=s)).astype(np.float32)
    for L, n_in in zip(ecfg["config"]["layers"][4:], (640, 2 * H)):
        inner = L["config"]["layer"]
        inner["class_name"] = "LSTM"
        inner["config"]["units"] = H
        inner["config"].pop("reset_after")
        for d in ("forward", "backward"):
            pre = f"{L['config']['name']}/{d}_lstm/lstm_cell"
            new_w[pre + "/kernel:0"], new_w[pre + "/recurrent_kernel:0"], new_w[pre + "/bias:0"] = n(n_in, 4 * H), n(H, 4 * H), n(4 * H)
    dl = [L for L in dcfg["config"]["layers"] if L["class_name"] == "Dense"]
    dl[0]["config"]["units"], dl[1]["config"]["units"] = F, n_out
    new_d = {"dense/kernel:0": n(2 * H, F), "dense/bias:0": n(F), "dense_1/kernel:0": n(F, n_out), "dense_1/bias:0": n(n_out)}
    return (ecfg, new_w), (dcfg, new_d)


def test_config_half_reads_a_hand_built_lstm(golden):
    rng = np.random.default_rng(3)
    (ecfg, ew), (dcfg, dw) = _lstm_config(golden, 48, 40, 2, rng)
    got = W.crnn_from_keras_config((ecfg, ew), (dcfg, dw))
    rnn = [tuple(tuple(ew[f"{layer}/{d}_lstm/lstm_cell/{k}:0"] for k in ("kernel", "recurrent_kernel", "bias")) for d in ("forward", "backward"))
           for layer in ("bidirectional", "bidirectional_1")]
    want = W.crnn_from_keras(40, 151, (ew["conv2d/kernel:0"], ew["conv2d/bias:0"]), rnn[0], rnn[1], (dw["dense/kernel:0"], dw["dense/bias:0"]),
                             (dw["dense_1/kernel:0"], dw["dense_1/bias:0"]), cell=W.CELL_LSTM, strides=(2, 8), padding="same", head_kind=W.HEAD_SOFTMAX)
    _same_params(got, want)
    assert (got.cell, got.units, got.head_units, got.n_out, got.out_t, got.pad_t) == (W.CELL_LSTM, 48, 40, 2, 19, (6, 7))
    g = got.gru2[1]
    assert g.b_h is None and g.w_x.shape == (192, 96) and g.w_h.shape == (192, 48) and g.b_x.shape == (192,)
    np.testing.assert_array_equal(g.w_x, rnn[1][1][0].T)
    np.testing.assert_array_equal(got.head_w1, dw["dense/kernel:0"].T)


@pytest.mark.parametrize("what", ["SimpleRNN", "reset_after", "return_sequences", "units", "activation", "three dense", "merge_mode"])
def test_config_half_refuses_anything_else(golden, what):
    (ecfg, ew), (dcfg, dw) = _lstm_config(golden, 32, 64, 2, np.random.default_rng(4))
    layers = ecfg["config"]["layers"]
    if what == "SimpleRNN":
        layers[4]["config"]["layer"]["class_name"] = "SimpleRNN"
    elif what == "reset_after":
        layers[4]["config"]["layer"]["class_name"] = layers[5]["config"]["layer"]["class_name"] = "GRU"
        layers[4]["config"]["layer"]["config"]["reset_after"] = layers[5]["config"]["layer"]["config"]["reset_after"] = False
    elif what == "return_sequences":
        layers[5]["config"]["layer"]["config"]["return_sequences"] = True
    elif what == "units":
        layers[5]["config"]["layer"]["config"]["units"] = 16
    elif what == "activation":
        layers[4]["config"]["layer"]["config"]["recurrent_activation"] = "hard_sigmoid"
    elif what == "three dense":
        dcfg["config"]["layers"].append(dcfg["config"]["layers"][-1])
    elif what == "merge_mode":
        layers[4]["config"]["merge_mode"] = "sum"
    with pytest.raises(W.GraphPatternError):
        W.crnn_from_keras_config((ecfg, ew), (dcfg, dw))


# ---- the blob --------------------------------------------------------------------------------------------------------------------------
def test_shipped_combination_keeps_its_sections(assets):
    for name in ("CRNN", "CRNN_softmax", "CRNN_nosilence"):
        sec = W.unpack_blob(W.pack_blob(W.load_model_dir(os.path.join(assets, name))))
        assert "crnn.cell" not in sec and len(sec["crnn.meta"]) == 14 and "crnn.g2b.bh" in sec
    for name in G.CRNN_ROWS:
        assert "crnn.cell" not in W.unpack_blob(W.pack_blob(G.GEOMETRIES[name].bundle()))


@pytest.mark.parametrize("cell,H,F", [(R.LSTM, 48, 64), (R.LSTM, 32, 64), (R.GRU, 32, 40), (R.GRU, 16, 1), (R.GRU, 64, 64)])
def test_blob_round_trip(cell, H, F):
    b = R.synthetic_rnn(seed=5, cell=cell, H=H, F=F, **SMALL, n_out=2, head=1)
    sec = W.unpack_blob(W.pack_blob(b))
    p = b.crnn
    assert len(sec["crnn.meta"]) == 14 and sec["crnn.meta"][11] == H
    assert sec["crnn.cell"].dtype == np.int32 and list(sec["crnn.cell"]) == [cell, F]
    for li, layer in ((1, p.gru1), (2, p.gru2)):
        for dn, g in zip("fb", layer):
            for key, arr in (("wx", g.w_x), ("bx", g.b_x), ("wh", g.w_h), ("bh", g.b_h)):
                name = f"crnn.g{li}{dn}.{key}"
                if arr is None:
                    assert cell == R.LSTM and key == "bh" and name not in sec
                else:
                    np.testing.assert_array_equal(sec[name], arr.ravel())
    np.testing.assert_array_equal(sec["crnn.head_w1"], p.head_w1.ravel())
    assert sec["crnn.head_w1"].size == F * 2 * H and sec["crnn.head_w2"].size == 2 * F


# ---- csrc/model_pack.h under the sanitizers ----------------------------------------------------------------------------------------------
def _no_sanitizer_runtime(output):
    """Did a -fsanitize build fail because this clang ships no runtime for it?  (tests/test_stream_rates_host.py's rule.)"""
    return re.search(r"libclang_rt\.|unsupported (option|argument)[^\n]*-fsanitize", output) is not None


@pytest.fixture(scope="module")
def pack_check(tmp_path_factory):
    cxx = "/opt/rocm/lib/llvm/bin/clang++"
    if not os.path.exists(cxx):
        cxx = shutil.which("clang++")
    if cxx is None:
        pytest.skip("no clang++ in this image")
    d = tmp_path_factory.mktemp("rnn_pack")
    exe = d / "rnn_pack_check"
    b = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-I" + _CSRC,
                        os.path.join(_ROOT, "tests", "native", "rnn_pack_check.cpp"), "-o", str(exe)], capture_output=True, text=True)
    if b.returncode != 0 and _no_sanitizer_runtime(b.stderr + b.stdout):
        pytest.skip("this clang has no sanitizer runtime: " + b.stderr[-300:])
    assert b.returncode == 0, b.stderr[-2000:]
    count = [0]

    def run(blob, cases=None):
        """[(status, text, {word: value} | None)] per case."""
        count[0] += 1
        f = d / f"blob{count[0]}.bin"
        f.write_bytes(blob)
        args = [str(exe), str(f)]
        if cases is not None:
            cf = d / f"cases{count[0]}.txt"
            cf.write_text("".join(c + "\n" for c in cases))
            args.append(str(cf))
        r = subprocess.run(args, capture_output=True, text=True, timeout=300,
                           env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1"))
        assert r.returncode == 0 and not r.stderr.strip(), (r.returncode, r.stdout[-300:], r.stderr[-3000:])
        n = 1 if cases is None else len(cases)
        lines = r.stdout.strip().splitlines()
        assert lines[-1] == f"ok {n}", lines[-1]
        out = []
        for ln in lines[:-1]:
            if ln.startswith("status "):
                _, rc, *text = ln.split(" ", 2)
                out.append([int(rc), text[0] if text else "", None])
            elif ln.startswith("rnn "):
                out[-1][2] = dict(w.split("=") for w in ln.split()[1:])
        assert len(out) == n
        return out
    return run


def _section(blob, name):
    """(index, offset, count) of a section of the blob."""
    n = int(np.frombuffer(blob, np.uint32, 1, 12)[0])
    for i in range(n):
        e = 16 + 32 * i
        if bytes(blob[e:e + 24]).rstrip(b"\0") == name.encode():
            off, cnt = (int(x) for x in np.frombuffer(blob, np.uint32, 2, e + 24))
            return i, off, cnt
    raise KeyError(name)


@pytest.mark.parametrize("cell", [R.GRU, R.LSTM])
@pytest.mark.parametrize("H", [16, 32, 48, 64])
def test_packer_accepts_every_cell_and_width(pack_check, cell, H):
    for F in (1, 40, 64):
        b = R.synthetic_rnn(seed=6, cell=cell, H=H, F=F, **SMALL, n_out=3, head=1)
        (rc, text, g), = pack_check(W.pack_blob(b))
        assert rc == 0, text
        assert g == dict(CELL=str(cell), H=str(H), F=str(F), SEQP=str(-(-2 * H // 64) * 64), FEATP="64", generic="1", enc_width=str(2 * H),
                         wx2="ok", wx1p="ok", bh="ok", w1="ok", conv="ok"), g


def test_generic_follows_conv_and_cell(pack_check):
    """At the standard conv only (GRU, 32, 64) keeps the kernels built for it; at another conv nothing does."""
    std = dict(T=151, n_mel=40, C=32, KF=5, KT=20, SF=2, ST=8, same=True)
    for cell, H, F, want in ((R.GRU, 32, 64, "0"), (R.GRU, 32, 63, "1"), (R.LSTM, 32, 64, "1"), (R.GRU, 48, 64, "1")):
        (rc, text, g), = pack_check(W.pack_blob(R.synthetic_rnn(seed=7, cell=cell, H=H, F=F, **std, n_out=2, head=1)))
        assert rc == 0 and g["generic"] == want and g["FEATP"] == "640" and g["wx2"] == g["w1"] == g["conv"] == "ok", (cell, H, F, text, g)
    (rc, text, g), = pack_check(W.pack_blob(G.GEOMETRIES["c-t150"].bundle()))
    assert rc == 0 and (g["generic"], g["CELL"], g["H"], g["F"], g["SEQP"]) == ("1", "0", "32", "64", "64")


def test_packer_refuses_by_rule(pack_check):
    lstm = R.synthetic_rnn(seed=8, cell=R.LSTM, H=32, F=40, **SMALL, n_out=2, head=1)
    gru = R.synthetic_rnn(seed=9, cell=R.GRU, H=48, F=64, **SMALL, n_out=2, head=1)
    blob = W.pack_blob(lstm)
    _, cell_off, cnt = _section(blob, "crnn.cell")
    _, meta_off, _ = _section(blob, "crnn.meta")
    assert cnt == 2
    cases = [(f"u32@{cell_off}=2", "cell"), (f"u32@{cell_off}={INT_MAX}", "cell"), (f"u32@{cell_off}={2 ** 32 - 1}", "cell"),
             (f"u32@{meta_off + 44}=24", "H = 24"), (f"u32@{meta_off + 44}=0", "H = 0"), (f"u32@{meta_off + 44}={INT_MAX}", "H = "),
             (f"u32@{meta_off + 44}=80", "H = 80"),
             (f"u32@{cell_off + 4}=0", "F = 0"), (f"u32@{cell_off + 4}=65", "F = 65"), (f"u32@{cell_off + 4}={INT_MAX}", "F = "),
             (f"u32@{cell_off + 4}={2 ** 32 - 1}", "F = -1"),
             (f"u32@{16 + 32 * _section(blob, 'crnn.cell')[0] + 28}=3", "crnn.cell")]
    for (rc, text, g), (case, word) in zip(pack_check(blob, [c for c, _ in cases]), cases):
        assert rc == WW_EBLOB and g is None and word in text, (case, rc, text)
    # an LSTM blob that carries bh; a GRU blob that lacks it
    with_bh = dataclasses.replace(lstm.crnn, gru2=tuple(dataclasses.replace(g, b_h=np.zeros(128, np.float32)) for g in lstm.crnn.gru2))
    (rc, text, _), = pack_check(W.pack_blob(dataclasses.replace(lstm, crnn=with_bh)))
    assert rc == WW_EBLOB and "LSTM" in text and "crnn.g2f.bh" in text
    no_bh = dataclasses.replace(gru.crnn, gru1=(gru.crnn.gru1[0], dataclasses.replace(gru.crnn.gru1[1], b_h=None)))
    (rc, text, _), = pack_check(W.pack_blob(dataclasses.replace(gru, crnn=no_bh)))
    assert rc == WW_EBLOB and "GRU" in text and "crnn.g1b.bh" in text
    # a CTC head on anything but GRU / 32
    std = dict(T=151, n_mel=40, C=32, KF=5, KT=20, SF=2, ST=8, same=True)
    for cell, H in ((R.LSTM, 32), (R.GRU, 48), (R.GRU, 16)):
        base = R.synthetic_rnn(seed=10, cell=cell, H=H, F=2 * H if H <= 32 else 64, **std, n_out=2, head=1)
        rng = np.random.default_rng(1)
        ctc = W.crnn_ctc_params(base.crnn, rng.normal(size=(4, 2 * H)), rng.normal(size=4))
        (rc, text, _), = pack_check(W.pack_blob(dataclasses.replace(base, crnn=ctc)))
        assert rc == WW_EBLOB and "CTC" in text and "GRU of 32" in text, (cell, H, text)
    # ... and the one it takes still loads
    base = R.synthetic_rnn(seed=11, cell=R.GRU, H=32, F=64, **std, n_out=2, head=1)
    ctc = W.crnn_ctc_params(base.crnn, np.ones((4, 64)), np.zeros(4))
    (rc, text, g), = pack_check(W.pack_blob(dataclasses.replace(base, crnn=ctc)))
    assert rc == 0 and g["generic"] == "0", text


def test_mangled_lstm_blobs_end_with_a_status(pack_check):
    """Truncated at every section boundary and inside the table, sections swapped pairwise, every meta word at INT_MAX: a status each
    time, nothing for the sanitizers to report (pack_check asserts an empty stderr)."""
    blob = W.pack_blob(R.synthetic_rnn(seed=12, cell=R.LSTM, H=48, F=40, **SMALL, n_out=2, head=1))
    n = int(np.frombuffer(blob, np.uint32, 1, 12)[0])
    offs = sorted({int(np.frombuffer(blob, np.uint32, 1, 16 + 32 * i + 24)[0]) for i in range(n)})
    cuts = sorted({0, 1, 15, 16, 17, 16 + 32 * n - 1, 16 + 32 * n, len(blob) - 1, len(blob) - 4, len(blob) - 16} | set(offs) |
                  {o + 4 for o in offs} | {o - 1 for o in offs})
    cases = [f"len={c}" for c in cuts if 0 <= c < len(blob)]
    _, meta_off, _ = _section(blob, "crnn.meta")
    cell_i, cell_off, _ = _section(blob, "crnn.cell")
    cases += [f"u32@{meta_off + 4 * k}={INT_MAX}" for k in range(14)] + [f"u32@{meta_off + 4 * k}={2 ** 31}" for k in range(14)]
    cases += [f"u32@{cell_off + 4 * k}={INT_MAX}" for k in range(2)]
    cases += [f"swap@{i},{j}" for i in range(n) for j in range(i + 1, n) if (i + j) % 3 == 0 or cell_i in (i, j)]
    cases += [f"name@{cell_i}=crnn.g1f.bh", f"name@{_section(blob, 'crnn.g1f.bx')[0]}=crnn.g1f.bh", f"u32@{16 + 32 * cell_i + 24}={len(blob) - 4}"]
    got = pack_check(blob, [""] + cases)
    assert got[0][0] == 0 and got[0][2]["CELL"] == "1"
    statuses = [rc for rc, _, _ in got[1:]]
    assert all(rc in (0, WW_EBLOB) for rc in statuses), sorted(set(statuses))
    assert statuses.count(WW_EBLOB) > len(statuses) // 2
    end = max(int(o) + 4 * int(c) for o, c in (np.frombuffer(blob, np.uint32, 2, 16 + 32 * i + 24) for i in range(n)))   # (then padding)
    for (rc, text, g), case in zip(got[1:], cases):
        if (case.startswith("len=") and int(case[4:]) < end) or case.endswith((f"={INT_MAX}", f"={2 ** 31}")):
            assert rc == WW_EBLOB and text, case
        if case.startswith("len=") and int(case[4:]) >= end:
            assert rc == 0, case
