#!/usr/bin/env python3
"""What the CTC tail costs beside the vector tail (development tool; tools/kbench.py's method).

Two sides on the same resident windows, alternated within one process for several rounds:
  ctc      ``ctc_forward_windows_dev`` of a synthetic 4-class CTC model (front + gru_tail_ctc_kernel; labels and lengths only)
  softmax  ``forward_windows_dev`` of the shipped CRNN_softmax forced into front + vector tail (``crnn_split_at=1,
           crnn_tail_mfma=0``): the same work minus 18 head rows and the decode
Per side and size: p50 / p90 of the per-call time (context timer around ``calls`` back-to-back calls, one sample per round), then
the per-kernel split under ``ww_profile``.  Usage: python tools/ctc_bench.py [rounds] [calls] > profiles/ctc/measured.txt

``stream``: what a CTC stream bank's tick costs (``wwhip.engine.CtcStreamBank``, S = 128, L = 4), per form, beside the shipped
``CRNN_softmax`` ``StreamBank`` tick on the same frames - one process, the sides alternated over several rounds, per side the p50 /
p99 of the host's time per ``step`` (``time.perf_counter`` around the call: what the 20 ms loop pays), and the mean host timeline.
Usage: python tools/ctc_bench.py stream [rounds] [ticks] > profiles/ctc/stream_measured.txt

``score``: what the forward-algorithm score costs.  ``ctc_score_windows_dev`` (front + CTC tail + ctc_score_kernel, K = 1 and K = 3
targets) beside ``ctc_forward_windows_dev`` on 256 and 4,096 resident windows, the sides alternated as above, then the per-kernel
split; and the S = 128 ``CtcStreamBank`` tick with targets beside the same bank without them (``want_steps`` on both sides: a
scoring bank keeps its posteriors), host time per ``step``.
Usage: python tools/ctc_bench.py score [rounds] [calls] [ticks] > profiles/ctc/score_measured.txt

``align``: what the Viterbi alignment costs.  ``ctc_align_windows_dev`` (front + CTC tail + ctc_align_kernel, K = 1 and K = 3) beside
``ctc_score_windows_dev`` (the same model launches + ctc_score_kernel) and ``ctc_forward_windows_dev`` on 256 and 4,096 resident
windows, the sides alternated, then the per-kernel split; and the S = 128 ``CtcStreamBank`` tick with scores and alignment beside the
same bank with scores alone, host time per ``step``.
Usage: python tools/ctc_bench.py align [rounds] [calls] [ticks] > profiles/ctc/align_measured.txt

``beam``: what the prefix beam search costs.  ``ctc_beam_windows_dev`` (front + CTC tail + ctc_beam_kernel, W = 8 and W = 64, four
paths) beside ``ctc_score_windows_dev`` and ``ctc_forward_windows_dev`` on 256 and 4,096 resident windows, and ``ctc_beam_dev`` alone
on the same posteriors, the sides alternated, then the per-kernel split; ``ww_ctc_beam_rows`` on the host for the same 4,096
sequences; and the S = 128 ``CtcStreamBank`` tick with posteriors, with and without the beam, host time per ``step``.
Usage: python tools/ctc_bench.py beam [rounds] [calls] [ticks] > profiles/ctc/beam_measured.txt

``occupancy``: what the forward-backward occupancy costs.  ``ctc_occupancy_dev`` (ctc_occupancy_kernel alone, two targets, exact mode,
with and without ``cls``) beside ``ctc_score_dev`` and ``ctc_align_dev`` on the same 256 and 4,096 resident posteriors of the L = 4
model, and the three ``_windows_dev`` forms (the model launches in front), the sides alternated, then the per-kernel split.
Usage: python tools/ctc_bench.py occupancy [rounds] [calls] > profiles/ctc/occupancy_measured.txt"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "wakeword-detection_amd"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from wwhip import _lib  # noqa: E402
from wwhip.engine import Engine  # noqa: E402

import ctc64  # noqa: E402



def windows_mode(rounds: int, calls: int) -> None:
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


def stream_mode(rounds: int, ticks: int, S: int = 128) -> None:
    import time
    from wwhip.engine import CtcStreamBank, StreamBank
    ctx = _lib.Context(0)
    ctc = Engine("synthetic-ctc-4", ctx=ctx, bundle=ctc64.model(4))
    smx = Engine(os.path.join(ROOT, "wakeword-detection_amd/assets/tf_lite_models/CRNN_softmax"), ctx=ctx)
    banks = {"ctc, one launch (default)": CtcStreamBank(ctc, S), "ctc, two launches": CtcStreamBank(ctc, S, two_launch=True),
             "ctc, full_recompute": CtcStreamBank(ctc, S, full_recompute=True), "ctc, one launch, want_steps": CtcStreamBank(ctc, S, want_steps=True),
             "CRNN_softmax StreamBank (yardstick)": StreamBank(smx, S)}
    rng = np.random.default_rng(3)
    frames = np.clip(rng.normal(0, 2500, (ticks, S, 320)), -32768, 32767).astype(np.int16)
    speech = np.ones(S, np.uint8)
    for b in banks.values():   # past the 151-row fill, every later tick two windows per stream
        for t in range(100):
            b.step(frames[t % ticks], speech)
        b.timeline(reset=True)
    times = {k: [] for k in banks}
    for _ in range(rounds):
        for k, b in banks.items():
            for t in range(ticks):
                t0 = time.perf_counter()
                b.step(frames[t], speech)
                times[k].append((time.perf_counter() - t0) * 1e6)
    print(f"S = {S} streams, L = 4, 2 windows per stream and tick; {rounds} rounds of {ticks} ticks per side, sides alternated; host time per step()")
    for k, t in times.items():
        tl = banks[k].timeline()
        print(f"{k}: p50 {np.percentile(t, 50):.1f} us, p99 {np.percentile(t, 99):.1f} us, min {min(t):.1f} us per tick; "
              f"timeline (mean us): " + ", ".join(f"{n} {tl[n]:.1f}" for n in StreamBank.TIMELINE_PHASES))
    for b in banks.values():
        b.close()
    ctc.close()
    smx.close()


def score_mode(rounds: int, calls: int, ticks: int, S: int = 128) -> None:
    import time
    from wwhip.engine import CtcStreamBank
    ctx = _lib.Context(0)
    ctc = Engine("synthetic-ctc-4", ctx=ctx, bundle=ctc64.model(4))
    one, three = [(1, 2)], [(1, 2), (0,), (1, 1)]
    for n in (256, 4096):
        wins = ctc64.G.windows(7, min(n, 512), 151, 40)
        d_mel = torch.from_numpy(np.ascontiguousarray(wins).reshape(-1, 40)).cuda()
        d_row = (torch.arange(n, dtype=torch.int64, device="cuda") % len(wins)) * 151
        d_valid = torch.full((n,), 151, dtype=torch.int32, device="cuda")
        d_lab = torch.empty((n, 2), dtype=torch.int32, device="cuda")
        d_len = torch.empty(n, dtype=torch.int32, device="cuda")
        d_score = torch.empty((3, n), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        a = (d_mel.data_ptr(), d_mel.shape[0], d_row.data_ptr(), d_valid.data_ptr(), n)
        sides = {
            "ctc_forward (labels)": lambda: ctc.ctc_forward_windows_dev(*a, 2, d_lab.data_ptr(), d_len.data_ptr()),
            "ctc_score K=1 (scores)": lambda: ctc.ctc_score_windows_dev(*a, one, "exact", d_score.data_ptr()),
            "ctc_score K=3 prefix (scores + labels)": lambda: ctc.ctc_score_windows_dev(*a, three, "prefix", d_score.data_ptr(), 2, d_lab.data_ptr(), d_len.data_ptr()),
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
    banks = {"steps, one launch": CtcStreamBank(ctc, S, want_steps=True),
             "steps + scores K=1, one launch": CtcStreamBank(ctc, S, want_steps=True, targets=one),
             "steps + scores K=3, one launch": CtcStreamBank(ctc, S, want_steps=True, targets=three, mode="prefix"),
             "steps, two launches": CtcStreamBank(ctc, S, want_steps=True, two_launch=True),
             "steps + scores K=1, two launches": CtcStreamBank(ctc, S, want_steps=True, two_launch=True, targets=one),
             "labels only, one launch (polled; for scale)": CtcStreamBank(ctc, S)}
    rng = np.random.default_rng(3)
    frames = np.clip(rng.normal(0, 2500, (ticks, S, 320)), -32768, 32767).astype(np.int16)
    speech = np.ones(S, np.uint8)
    for b in banks.values():   # past the 151-row fill, every later tick two windows per stream
        for t in range(100):
            b.step(frames[t % ticks], speech)
    times = {k: [] for k in banks}
    for _ in range(rounds):
        for k, b in banks.items():
            for t in range(ticks):
                t0 = time.perf_counter()
                b.step(frames[t], speech)
                times[k].append((time.perf_counter() - t0) * 1e6)
    print(f"S = {S} streams, L = 4, 2 windows per stream and tick; {rounds} rounds of {ticks} ticks per side, sides alternated; host time per step()")
    for k, t in times.items():
        print(f"{k}: p50 {np.percentile(t, 50):.1f} us, p99 {np.percentile(t, 99):.1f} us, min {min(t):.1f} us per tick")
    for b in banks.values():
        b.close()
    ctc.close()


def align_mode(rounds: int, calls: int, ticks: int, S: int = 128) -> None:
    import time
    from wwhip.engine import CtcStreamBank
    ctx = _lib.Context(0)
    ctc = Engine("synthetic-ctc-4", ctx=ctx, bundle=ctc64.model(4))
    one, three = [(1, 2)], [(1, 2), (0,), (1, 1)]
    for n in (256, 4096):
        wins = ctc64.G.windows(7, min(n, 512), 151, 40)
        d_mel = torch.from_numpy(np.ascontiguousarray(wins).reshape(-1, 40)).cuda()
        d_row = (torch.arange(n, dtype=torch.int64, device="cuda") % len(wins)) * 151
        d_valid = torch.full((n,), 151, dtype=torch.int32, device="cuda")
        d_lab = torch.empty((n, 2), dtype=torch.int32, device="cuda")
        d_len = torch.empty(n, dtype=torch.int32, device="cuda")
        d_score = torch.empty((3, n), dtype=torch.float32, device="cuda")
        d_span = torch.empty((3, n, 9, 2), dtype=torch.int8, device="cuda")
        torch.cuda.synchronize()
        a = (d_mel.data_ptr(), d_mel.shape[0], d_row.data_ptr(), d_valid.data_ptr(), n)
        sides = {
            "ctc_forward (labels)": lambda: ctc.ctc_forward_windows_dev(*a, 2, d_lab.data_ptr(), d_len.data_ptr()),
            "ctc_score K=1 exact": lambda: ctc.ctc_score_windows_dev(*a, one, "exact", d_score.data_ptr()),
            "ctc_align K=1 exact": lambda: ctc.ctc_align_windows_dev(*a, one, "exact", d_score.data_ptr(), d_span.data_ptr()),
            "ctc_score K=3 prefix": lambda: ctc.ctc_score_windows_dev(*a, three, "prefix", d_score.data_ptr()),
            "ctc_align K=3 prefix": lambda: ctc.ctc_align_windows_dev(*a, three, "prefix", d_score.data_ptr(), d_span.data_ptr()),
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
    banks = {"steps + scores K=1, one launch": CtcStreamBank(ctc, S, want_steps=True, targets=one),
             "steps + scores + alignment K=1, one launch": CtcStreamBank(ctc, S, want_steps=True, targets=one, align=True),
             "steps + scores K=3 prefix, one launch": CtcStreamBank(ctc, S, want_steps=True, targets=three, mode="prefix"),
             "steps + scores + alignment K=3 prefix, one launch": CtcStreamBank(ctc, S, want_steps=True, targets=three, mode="prefix", align=True)}
    rng = np.random.default_rng(3)
    frames = np.clip(rng.normal(0, 2500, (ticks, S, 320)), -32768, 32767).astype(np.int16)
    speech = np.ones(S, np.uint8)
    for b in banks.values():   # past the 151-row fill, every later tick two windows per stream
        for t in range(100):
            b.step(frames[t % ticks], speech)
    times = {k: [] for k in banks}
    for _ in range(rounds):
        for k, b in banks.items():
            for t in range(ticks):
                t0 = time.perf_counter()
                b.step(frames[t], speech)
                times[k].append((time.perf_counter() - t0) * 1e6)
    print(f"S = {S} streams, L = 4, 2 windows per stream and tick; {rounds} rounds of {ticks} ticks per side, sides alternated; host time per step()")
    for k, t in times.items():
        print(f"{k}: p50 {np.percentile(t, 50):.1f} us, p99 {np.percentile(t, 99):.1f} us, min {min(t):.1f} us per tick")
    for b in banks.values():
        b.close()
    ctc.close()


def beam_mode(rounds: int, calls: int, ticks: int, S: int = 128) -> None:
    import time
    from wwhip import ctc as C
    from wwhip.engine import CtcStreamBank
    ctx = _lib.Context(0)
    ctc = Engine("synthetic-ctc-4", ctx=ctx, bundle=ctc64.model(4))
    one = [(1, 2)]
    for n in (256, 4096):
        wins = ctc64.G.windows(7, min(n, 512), 151, 40)
        d_mel = torch.from_numpy(np.ascontiguousarray(wins).reshape(-1, 40)).cuda()
        d_row = (torch.arange(n, dtype=torch.int64, device="cuda") % len(wins)) * 151
        d_valid = torch.full((n,), 151, dtype=torch.int32, device="cuda")
        d_lab = torch.empty((n, 4, 19), dtype=torch.int32, device="cuda")
        d_len = torch.empty((n, 4), dtype=torch.int32, device="cuda")
        d_prob = torch.empty((n, 4), dtype=torch.float32, device="cuda")
        d_score = torch.empty((1, n), dtype=torch.float32, device="cuda")
        d_steps = torch.empty((n, 19, 4), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        a = (d_mel.data_ptr(), d_mel.shape[0], d_row.data_ptr(), d_valid.data_ptr(), n)
        o = (d_lab.data_ptr(), d_len.data_ptr(), d_prob.data_ptr())
        ctc.ctc_forward_windows_dev(*a, 2, d_lab.data_ptr(), d_len.data_ptr(), d_steps.data_ptr())
        ctx.synchronize()
        sides = {
            "ctc_forward (labels)": lambda: ctc.ctc_forward_windows_dev(*a, 2, d_lab.data_ptr(), d_len.data_ptr()),
            "ctc_score K=1 exact": lambda: ctc.ctc_score_windows_dev(*a, one, "exact", d_score.data_ptr()),
            "ctc_beam W=8 P=4": lambda: ctc.ctc_beam_windows_dev(*a, 8, 4, 19, *o),
            "ctc_beam W=64 P=4": lambda: ctc.ctc_beam_windows_dev(*a, 64, 4, 19, *o),
            "ctc_beam_dev alone W=8 P=4": lambda: ctc.ctc_beam_dev(d_steps.data_ptr(), n, 19, 4, 8, 4, 19, *o),
            "ctc_beam_dev alone W=64 P=4": lambda: ctc.ctc_beam_dev(d_steps.data_ptr(), n, 19, 4, 64, 4, 19, *o),
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
        if n == 4096:   # the host function on the same sequences (one thread)
            steps = d_steps.cpu().numpy()
            for W in (8, 64):
                t = []
                for _ in range(3):
                    t0 = time.perf_counter()
                    C.beam_rows(steps, W, 4, 19)
                    t.append((time.perf_counter() - t0) * 1e6)
                print(f"{n} sequences, ww_ctc_beam_rows on the host W={W} P=4: best of 3 {min(t):.0f} us")
    banks = {"steps, one launch": CtcStreamBank(ctc, S, want_steps=True),
             "steps + beam W=8 P=4, one launch": CtcStreamBank(ctc, S, want_steps=True, beam_width=8, top_paths=4),
             "steps + beam W=64 P=4, one launch": CtcStreamBank(ctc, S, want_steps=True, beam_width=64, top_paths=4),
             "steps + scores K=1, one launch": CtcStreamBank(ctc, S, want_steps=True, targets=one)}
    rng = np.random.default_rng(3)
    frames = np.clip(rng.normal(0, 2500, (ticks, S, 320)), -32768, 32767).astype(np.int16)
    speech = np.ones(S, np.uint8)
    for b in banks.values():   # past the 151-row fill, every later tick two windows per stream
        for t in range(100):
            b.step(frames[t % ticks], speech)
    times = {k: [] for k in banks}
    for _ in range(rounds):
        for k, b in banks.items():
            for t in range(ticks):
                t0 = time.perf_counter()
                b.step(frames[t], speech)
                times[k].append((time.perf_counter() - t0) * 1e6)
    print(f"S = {S} streams, L = 4, 2 windows per stream and tick; {rounds} rounds of {ticks} ticks per side, sides alternated; host time per step()")
    for k, t in times.items():
        print(f"{k}: p50 {np.percentile(t, 50):.1f} us, p99 {np.percentile(t, 99):.1f} us, min {min(t):.1f} us per tick")
    for b in banks.values():
        b.close()
    ctc.close()


def occupancy_mode(rounds: int, calls: int) -> None:
    ctx = _lib.Context(0)
    ctc = Engine("synthetic-ctc-4", ctx=ctx, bundle=ctc64.model(4))
    two = [(1, 2), (1, 1)]
    for n in (256, 4096):
        wins = ctc64.G.windows(7, min(n, 512), 151, 40)
        d_mel = torch.from_numpy(np.ascontiguousarray(wins).reshape(-1, 40)).cuda()
        d_row = (torch.arange(n, dtype=torch.int64, device="cuda") % len(wins)) * 151
        d_valid = torch.full((n,), 151, dtype=torch.int32, device="cuda")
        d_lab = torch.empty((n, 2), dtype=torch.int32, device="cuda")
        d_len = torch.empty(n, dtype=torch.int32, device="cuda")
        d_steps = torch.empty((n, 19, 4), dtype=torch.float32, device="cuda")
        d_score = torch.empty((2, n), dtype=torch.float32, device="cuda")
        d_span = torch.empty((2, n, 9, 2), dtype=torch.int8, device="cuda")
        d_occ = torch.empty((2, n, 19, 9), dtype=torch.float32, device="cuda")
        d_cls = torch.empty((2, n, 19, 4), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        a = (d_mel.data_ptr(), d_mel.shape[0], d_row.data_ptr(), d_valid.data_ptr(), n)
        ctc.ctc_forward_windows_dev(*a, 2, d_lab.data_ptr(), d_len.data_ptr(), d_steps.data_ptr())
        ctx.synchronize()
        s = (d_steps.data_ptr(), n, 19, 4, two, "exact")
        sides = {
            "ctc_score_dev alone K=2 exact": lambda: ctc.ctc_score_dev(*s, d_score.data_ptr()),
            "ctc_align_dev alone K=2 exact": lambda: ctc.ctc_align_dev(*s, d_score.data_ptr(), d_span.data_ptr()),
            "ctc_occupancy_dev alone K=2 exact": lambda: ctc.ctc_occupancy_dev(*s, d_score.data_ptr(), d_occ.data_ptr()),
            "ctc_occupancy_dev alone K=2 exact + cls": lambda: ctc.ctc_occupancy_dev(*s, d_score.data_ptr(), d_occ.data_ptr(), d_cls.data_ptr()),
            "ctc_score_windows_dev K=2 exact": lambda: ctc.ctc_score_windows_dev(*a, two, "exact", d_score.data_ptr()),
            "ctc_align_windows_dev K=2 exact": lambda: ctc.ctc_align_windows_dev(*a, two, "exact", d_score.data_ptr(), d_span.data_ptr()),
            "ctc_occupancy_windows_dev K=2 exact": lambda: ctc.ctc_occupancy_windows_dev(*a, two, "exact", d_score.data_ptr(), d_occ.data_ptr()),
            "ctc_occupancy_windows_dev K=2 exact + cls": lambda: ctc.ctc_occupancy_windows_dev(*a, two, "exact", d_score.data_ptr(), d_occ.data_ptr(),
                                                                                               d_cls.data_ptr()),
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


if __name__ == "__main__":
    args = sys.argv[1:]
    if args and args[0] == "occupancy":
        occupancy_mode(int(args[1]) if len(args) > 1 else 9, int(args[2]) if len(args) > 2 else 200)
    elif args and args[0] == "beam":
        beam_mode(int(args[1]) if len(args) > 1 else 9, int(args[2]) if len(args) > 2 else 200, int(args[3]) if len(args) > 3 else 300)
    elif args and args[0] == "align":
        align_mode(int(args[1]) if len(args) > 1 else 9, int(args[2]) if len(args) > 2 else 200, int(args[3]) if len(args) > 3 else 300)
    elif args and args[0] == "score":
        score_mode(int(args[1]) if len(args) > 1 else 9, int(args[2]) if len(args) > 2 else 200, int(args[3]) if len(args) > 3 else 300)
    elif args and args[0] == "stream":
        stream_mode(int(args[1]) if len(args) > 1 else 7, int(args[2]) if len(args) > 2 else 300)
    else:
        windows_mode(int(args[0]) if len(args) > 0 else 9, int(args[1]) if len(args) > 1 else 200)
