#!/usr/bin/env python3
"""rnn_layer_kernel<CELL, H> on the MI355X: what each instantiation costs, and that the shipped cell's bits did not move.

    python tools/rnn_cells.py [--out FILE] [--reps 7]     per-kernel HIP-event times (the library's profile: ww_profile_enable) of the
                                                         eight (cell, H) instantiations at 256 and 4,096 windows x 19 steps;
                                                         gru_generic_kernel on the same windows in the same process, the two sides
                                                         alternated; the whole forward (forward_windows_dev between two events) per model
    python tools/rnn_cells.py --digest [--out FILE]      sha256 of Engine.forward's posteriors and encodings for geometry64's
                                                         GENERIC_ROWS and the shipped CRNNs at their 70 windows: run it on two
                                                         commits, the two lists must be equal

The timed models are tests/rnn64.py's builders at the standard conv (19 steps of 640 features); (GRU, 32) runs under a 40-wide head,
which is what sends it to rnn_layer_kernel; gru_generic_kernel's model is the same GRU of 32 units under the 64-wide head behind a
conv with KT = 19 instead of 20 (not the standard geometry, still 19 steps of 640 features, the same windows)."""
import argparse
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "wakeword-detection_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

STD = dict(T=151, n_mel=40, C=32, KF=5, KT=20, SF=2, ST=8, same=True)


def engine_of(bundle):
    from wwhip.engine import Engine
    return Engine("synthetic", bundle=bundle)


def digest(out):
    import geometry64 as G
    from wwhip import weights as W
    from wwhip.engine import Engine
    assets = os.path.join(ROOT, "wakeword-detection_amd", "assets", "tf_lite_models")
    lines = []
    for name in G.GENERIC_ROWS:
        e = engine_of(G.GEOMETRIES[name].bundle())
        post, enc = e.forward(G.row_windows(name), want_enc=True)
        lines.append(f"digest {name} post {hashlib.sha256(np.ascontiguousarray(post).tobytes()).hexdigest()} "
                     f"enc {hashlib.sha256(np.ascontiguousarray(enc).tobytes()).hexdigest()}")
        e.close()
    wins = G.windows(990, 70, 151, 40)
    for name in sorted(os.listdir(assets)):
        d = os.path.join(assets, name)
        if not os.path.isfile(os.path.join(d, "encode.tflite")) or W.load_model_dir(d).kind != W.KIND_CRNN:
            continue
        for precision in ("fp32", "bf16x3"):
            e = Engine(d, precision=precision)
            if e.window == 151:
                post, enc = e.forward(wins, want_enc=True)
                lines.append(f"digest {name} {precision} post {hashlib.sha256(np.ascontiguousarray(post).tobytes()).hexdigest()} "
                             f"enc {hashlib.sha256(np.ascontiguousarray(enc).tobytes()).hexdigest()}")
            e.close()
    emit(lines, out)


def emit(lines, out):
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "a") as f:
            f.write(text)


def profile_once(e, d_mel, d_row, d_valid, nw, d_out, T):
    e.ctx.synchronize()
    e.ctx.profile(True)
    try:
        e.ctx.profile_read()
        e.forward_windows_dev(d_mel.data_ptr(), nw * T, d_row.data_ptr(), d_valid.data_ptr(), nw, d_out.data_ptr())
        return {k: v["total_ms"] * 1e3 for k, v in e.ctx.profile_read().items()}
    finally:
        e.ctx.profile(False)


def whole_once(e, d_mel, d_row, d_valid, nw, d_out, T):
    e.ctx.synchronize()
    e.ctx.timer_start()
    e.forward_windows_dev(d_mel.data_ptr(), nw * T, d_row.data_ptr(), d_valid.data_ptr(), nw, d_out.data_ptr())
    return e.ctx.timer_stop() * 1e3


def measure(out, reps):
    import torch
    import geometry64 as G
    import rnn64 as R
    models = []
    for cell in (R.GRU, R.LSTM):
        for H in (16, 32, 48, 64):
            F = 40 if (cell, H) == (R.GRU, 32) else 64
            models.append((f"{'gru' if cell == R.GRU else 'lstm'}{H}", engine_of(R.synthetic_rnn(seed=500 + H + cell, cell=cell, H=H, F=F, **STD, n_out=2, head=1))))
    base = engine_of(G.synthetic_crnn(seed=599, **dict(STD, KT=19), n_out=2, head=1))
    lines = [f"# tools/rnn_cells.py, {reps} repetitions per figure (median), microseconds; {torch.cuda.get_device_name(0)}"]
    T = 151
    for nw in (256, 4096):
        wins = G.windows(991, 64, T, 40)
        d_mel = torch.from_numpy(np.ascontiguousarray(wins[np.arange(nw) % 64]).reshape(-1, 40)).cuda()
        d_row = torch.arange(nw, dtype=torch.int64, device="cuda") * T
        d_valid = torch.full((nw,), T, dtype=torch.int32, device="cuda")
        args = lambda e: (e, d_mel, d_row, d_valid, nw, torch.empty((nw, e.n_out), dtype=torch.float32, device="cuda"), T)
        for name, e in models:
            a, b = args(e), args(base)
            profile_once(*a), profile_once(*b)   # warm-up, workspace growth
            mine, theirs, whole, whole_b = [], [], [], []
            for rep in range(reps):
                for side in ((0, 1) if rep % 2 == 0 else (1, 0)):   # the two sides alternated
                    (mine if side == 0 else theirs).append(profile_once(*(a if side == 0 else b)))
                for side in ((0, 1) if rep % 2 == 0 else (1, 0)):
                    (whole if side == 0 else whole_b).append(whole_once(*(a if side == 0 else b)))
            med = lambda rows, k: float(np.median([r[k] for r in rows]))
            lines.append(f"{nw:5d} windows  {name:7s} rnn_layer_kernel<seq> {med(mine, 'rnn_layer_kernel<seq>'):8.1f}  <last> {med(mine, 'rnn_layer_kernel<last>'):8.1f}  "
                         f"gemm1 {med(mine, 'gemm_nt_kernel<gru1,generic>'):8.1f}  gemm2 {med(mine, 'gemm_nt_kernel<gru2,generic>'):8.1f}  "
                         f"conv {med(mine, 'conv_generic_kernel'):8.1f}  head {med(mine, 'crnn_head_kernel'):6.1f}  forward {float(np.median(whole)):9.1f}   |   "
                         f"gru_generic_kernel<seq> {med(theirs, 'gru_generic_kernel<seq>'):8.1f}  <last> {med(theirs, 'gru_generic_kernel<last>'):8.1f}  "
                         f"forward {float(np.median(whole_b)):9.1f}")
    emit(lines, out)
    for _, e in models:
        e.close()
    base.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--digest", action="store_true")
    ap.add_argument("--out", default=None, help="append the lines to this file as well")
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    from wwhip import _build
    assert os.path.isfile(_build.LIB_PATH), "build the library first (python __graft_entry__.py)"
    digest(a.out) if a.digest else measure(a.out, a.reps)


if __name__ == "__main__":
    main()
