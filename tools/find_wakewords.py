#!/usr/bin/env python3
"""Scan recordings for wake words (wwhip.evaluate.find_wakewords), and what the detection-event call costs.

  find_wakewords.py [scan] --models DIR [DIR ...] --threshold T[,T...] [--hop 2] [--window 30] [--resample] [--no-pad] a.wav [b.wav ...]
        every model directory (several: one wwhip.ModelSet - same geometry, one front-end pass) over every wav; one line per detection:
        file, wake word, the windows [start, end), start / end / peak in seconds from the file's first sample, the peak's smoothed
        posterior.  One threshold serves all models, or one per model (comma-separated).  --resample: files at another rate (or G.711) are converted on
        the GPU instead of refused.
  find_wakewords.py measure [out=profiles/events/measured.txt] [reps=30] [n=414000]
        on an MI355X: posterior_events_dev on a resident [K][n] plane (414,000 rows = 2.3 h at hop 2), K = 1 and 3, at three event
        densities - none, about 100, n / 4 - against what the library offered before: the device-to-host copy of those posteriors,
        far_frr(..., want_smoothed) per plane and the run rule in numpy.  The two sides alternate inside the process after a warm-up;
        host clock around calls that end in a device synchronise; p50 / p99 ms.  Both sides' events are compared before anything is
        timed.  The table is printed and written to `out`.
"""
import argparse
import os
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [HERE, os.path.join(HERE, "wakeword-detection_amd")]

import numpy as np  # noqa: E402


def scan(argv):
    ap = argparse.ArgumentParser(prog="find_wakewords.py", description="which wake word fires where, in which recording")
    ap.add_argument("wavs", nargs="+")
    ap.add_argument("--models", nargs="+", required=True, help="model directories (filter / encode / detect .tflite)")
    ap.add_argument("--threshold", required=True, type=lambda t: [float(x) for x in t.split(",")], help="one for all models, or one per model: T,T,...")
    ap.add_argument("--hop", type=int, default=2, help="rows between sliding windows (default 2)")
    ap.add_argument("--window", type=int, default=30, help="taps of the smoothing mean (default 30; 0: none)")
    ap.add_argument("--resample", action="store_true")
    ap.add_argument("--no-pad", action="store_true", help="do not pad each file with 0.5 s of zeros on both sides")
    a = ap.parse_args(argv)
    from wwhip.engine import Engine, ModelSet
    from wwhip.evaluate import find_wakewords, read_wav_pcm
    if len(a.threshold) not in (1, len(a.models)):
        ap.error(f"--threshold: one value, or one per model ({len(a.models)})")
    clips = []
    for path in a.wavs:
        c = read_wav_pcm(path, resample=a.resample)
        if c.dtype != np.int16:
            c = np.clip(np.rint(c * 32768.0), -32768, 32767).astype(np.int16)
        clips.append(c)
    runner = Engine(a.models[0]) if len(a.models) == 1 else ModelSet(a.models)
    thr = a.threshold[0] if len(a.threshold) == 1 else a.threshold
    found = find_wakewords(runner, clips, thr, hop=a.hop, windowsize=a.window, pad=not a.no_pad)
    for d in found:
        print(f"{a.wavs[d.clip]}\t{d.name}\twindows [{d.start}, {d.end})\t{d.start_s:.3f} s .. {d.end_s:.3f} s\tpeak {d.peak_s:.3f} s\t{d.peak_value:.6f}")
    print(f"{len(found)} detection(s) in {len(clips)} file(s)", file=sys.stderr)
    runner.close()


# ---------------------------------------------------------------------------------------------------------------- measure
def _numpy_rule(sm, thr, plane):
    """The run rule on one plane's smoothed values, vectorised: an EVENT_DTYPE array (one segment)."""
    from wwhip import _lib
    above = sm > thr
    edge = np.diff(np.concatenate(([0], above.view(np.int8), [0])))
    starts, ends = np.flatnonzero(edge == 1), np.flatnonzero(edge == -1)
    ev = np.zeros(starts.size, _lib.EVENT_DTYPE)
    if starts.size:
        cuts = np.stack([starts, ends], 1).ravel()
        cuts_in = np.minimum(cuts, sm.size - 1)  # (reduceat wants indices inside the array; an end at n is the last run's)
        best = np.maximum.reduceat(sm, cuts_in)[::2]
        if ends[-1] == sm.size:  # the last run reaches the end: its maximum runs to the last row
            best[-1] = sm[starts[-1]:].max()
        run = np.repeat(np.arange(starts.size), ends - starts)
        rows = np.flatnonzero(above)
        hit = rows[sm[rows] == best[run]]
        first = np.full(starts.size, sm.size, np.int64)
        np.minimum.at(first, run[sm[rows] == best[run]], hit)
        ev["plane"], ev["start"], ev["end"], ev["peak"], ev["peak_value"] = plane, starts, ends, first, best
    return ev


def _planes(kind, K, n, rng):
    """[K][n] float32 posteriors and the threshold of one density."""
    if kind == "none":
        return rng.uniform(0, 0.4, (K, n)).astype(np.float32), 0.5
    if kind == "100":
        p = rng.uniform(0, 0.2, (K, n)).astype(np.float32)
        per = 100 // K + 1
        for k in range(K):
            for a in rng.choice(np.arange(100, n - 200, 200), per, replace=False):
                p[k, a:a + 60] = rng.uniform(0.85, 1.0, 60)
        return p, 0.5
    # n / 4: one row in four is 1 - a 30-tap mean sees 7 or 8 of them, in turn two rows each
    p = np.zeros((K, n), np.float32)
    p[:, ::4] = 1.0
    return p, 7.5 / 30


def measure(argv):
    import torch
    from wwhip import _lib
    from wwhip.engine import Engine
    kv = dict(x.split("=", 1) for x in argv)
    out, reps, n = kv.get("out", os.path.join(HERE, "profiles", "events", "measured.txt")), int(kv.get("reps", 30)), int(kv.get("n", 414000))
    assert torch.cuda.is_available(), "measure needs the MI355X"
    eng = Engine(os.path.join(HERE, "wakeword-detection_amd", "assets", "tf_lite_models", "CRNN"))
    rng = np.random.default_rng(1)
    lines = [f"posterior_events_dev on a resident [K][{n}] float32 plane, window 30, one segment; {reps} alternating repeats after 3 warm-up rounds;",
             "host clock around calls that end in a device synchronise; ms.",
             "A = posterior_events_dev (five launches; thresholds up, plane totals and events down)",
             "B = the posteriors to the host, Engine.far_frr(..., want_smoothed) per plane (upload, smooth, sweep, smoothed values down), the run rule in numpy",
             "",
             f"{'K':>2} {'density':>8} {'events':>8} | {'A p50':>8} {'A p99':>8} | {'B p50':>8} {'B p99':>8} | {'B d2h':>7} {'B far_frr':>9} {'B numpy':>8} | B p50 / A p50"]
    for K in (1, 3):
        for kind in ("none", "100", "n/4"):
            p, thr = _planes(kind, K, n, rng)
            d = torch.from_numpy(p).cuda()
            torch.cuda.synchronize()

            def side_a():
                return eng.posterior_events_dev(d.data_ptr(), n, thr, None, 30, planes=K, cap=K * n)

            def side_b(parts=None):
                t0 = time.perf_counter()
                host = d.cpu().numpy()
                t1 = time.perf_counter()
                sms = [eng.far_frr(np.zeros(0, np.float32), host[k], np.array([thr]), 1.0, 1.0, window=30, want_smoothed=True)[3] for k in range(K)]
                t2 = time.perf_counter()
                ev = np.concatenate([_numpy_rule(sms[k], thr, k) for k in range(K)])
                if parts is not None:
                    parts.append((t1 - t0, t2 - t1, time.perf_counter() - t2))
                return ev

            a, b = side_a(), side_b()
            assert a.tobytes() == b.tobytes(), (K, kind, len(a), len(b))
            for _ in range(3):
                side_a(), side_b()
            ta, tb, parts = [], [], []
            for _ in range(reps):
                t0 = time.perf_counter()
                side_a()
                t1 = time.perf_counter()
                side_b(parts)
                t2 = time.perf_counter()
                ta.append((t1 - t0) * 1e3)
                tb.append((t2 - t1) * 1e3)
            q = lambda v, f: float(np.percentile(v, f))
            part = np.median(np.array(parts), axis=0) * 1e3
            lines.append(f"{K:>2} {kind:>8} {len(a):>8} | {q(ta, 50):>8.3f} {q(ta, 99):>8.3f} | {q(tb, 50):>8.3f} {q(tb, 99):>8.3f} | "
                         f"{part[0]:>7.3f} {part[1]:>9.3f} {part[2]:>8.3f} | {q(tb, 50) / q(ta, 50):.1f}x")
    # where A's time goes on the device (the context's event pairs; a run of its own, not part of the timings above)
    p, thr = _planes("100", 3, n, rng)
    d = torch.from_numpy(p).cuda()
    torch.cuda.synchronize()
    eng.ctx.profile_read()
    eng.ctx.profile(True)
    for _ in range(10):
        eng.posterior_events_dev(d.data_ptr(), n, thr, None, 30, planes=3, cap=3 * n)
    eng.ctx.profile(False)
    prof = eng.ctx.profile_read()
    lines += ["", "device time per call of A by kernel, K = 3, about 100 events (event pairs around each launch, mean of 10 calls, us):",
              "  " + ", ".join(f"{k} {v['total_ms'] / v['calls'] * 1e3:.1f}" for k, v in sorted(prof.items()))]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write(text)
    eng.close()


if __name__ == "__main__":
    args = sys.argv[1:]
    if args and args[0] == "measure":
        measure(args[1:])
    else:
        scan(args[1:] if args and args[0] == "scan" else args)
