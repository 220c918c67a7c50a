#!/usr/bin/env python3
"""What the CTC tail costs beside the vector tail (development tool; tools/kbench.py's method).

Two sides on the same resident windows, alternated within one process for several rounds:
  ctc      ``ctc_forward_windows_dev`` of a synthetic 4-class CTC model (front + gru_tail_ctc_kernel; labels and lengths only)
  softmax  ``forward_windows_dev`` of the shipped CRNN_softmax forced into front + vector tail (``crnn_split_at=1,
           crnn_tail_mfma=0``): the same work minus 18 head rows and the decode
Per side and size: p50 / p90 of the per-call time (context timer around ``calls`` back-to-back calls, one sample per round), then
the per-kernel split under ``ww_profile``.  Usage: python tools/ctc_bench.py [rounds] [calls] > profiles/ctc/measured.txt"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "wakeword-detection_amd"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from wwhip import _lib  # noqa: E402
from wwhip.engine import Engine  # noqa: E402

import ctc64  # noqa: E402

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 9
calls = int(sys.argv[2]) if len(sys.argv) > 2 else 200
ctx = _lib.Context(0)
ctc = Engine("synthetic-ctc-4", ctx=ctx, bundle=ctc64.model(4))
smx = Engine(os.path.join(ROOT, "wakeword-detection_amd/assets/tf_lite_models/CRNN_softmax"), ctx=ctx)
smx.set_option("crnn_split_at", 1)
smx.set_option("crnn_tail_mfma", 0)

for n in (256, 4096):
    wins = ctc64.G.windows(7, min(n, 512), 151, 40)
    d_mel = torch.from_numpy(np.ascontiguousarray(wins).reshape(-1, 40)).cuda()
    d_row = (torch.arange(n, dtype=torch.int64, device="cuda") % len(wins)) * 151
    d_valid = torch.full((n,), 151, dtype=torch.int32, device="cuda")
    d_lab = torch.empty((n, 2), dtype=torch.int32, device="cuda")
    d_len = torch.empty(n, dtype=torch.int32, device="cuda")
    d_out = torch.empty((n, smx.n_out), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    sides = {
        "ctc": lambda: ctc.ctc_forward_windows_dev(d_mel.data_ptr(), d_mel.shape[0], d_row.data_ptr(), d_valid.data_ptr(), n, 2,
                                                   d_lab.data_ptr(), d_len.data_ptr()),
        "softmax": lambda: smx.forward_windows_dev(d_mel.data_ptr(), d_mel.shape[0], d_row.data_ptr(), d_valid.data_ptr(), n, d_out.data_ptr()),
    }
    for fn in sides.values():
        for _ in range(5):
            fn()
    ctx.synchronize()
    times = {k: [] for k in sides}
    for _ in range(rounds):
        for k, fn in sides.items():
            ctx.timer_start()
            for _ in range(calls):
                fn()
            times[k].append(ctx.timer_stop() / calls * 1e3)
    for k, t in times.items():
        print(f"{n} windows, {k}: p50 {np.percentile(t, 50):.1f} us, p90 {np.percentile(t, 90):.1f} us per call "
              f"({rounds} rounds of {calls} calls, sides alternated)")
    for k, fn in sides.items():
        ctx.profile(True)
        for _ in range(calls):
            fn()
        p = ctx.profile_read()
        ctx.profile(False)
        print(f"{n} windows, {k}, per kernel (us):", {name: round(v["total_ms"] / v["calls"] * 1e3, 1) for name, v in p.items()})
ctc.close()
smx.close()
