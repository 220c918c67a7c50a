#!/usr/bin/env python3
"""Stream banks at another rate than 16 kHz: what a tick and a feed cost (profiles/stream_rate/measured.txt).

  tick   S streams, is_speech = 1, 20 ms per tick at --rate through StreamBank(sample_rate=rate): p50 / p99 of the per-tick latency
         (tick submitted on the host -> posteriors visible on the host).  --rate 16000 is the plain bank (tools/stream_latency.py's
         number for one model).
  push   what a caller had to do without a rate bank: S StreamResampler objects in front of a 16 kHz bank - per tick S push() calls
         (each its own upload, launch, synchronise and download), the 16 kHz samples queued per stream, a tick of the 16 kHz bank
         once every stream holds 320.  The same p50 / p99, the pushes included.
  feed   a causal Wavenet bank fed S streams x --seconds in ONE call at --rate (16000: the plain bank's feed): milliseconds per call.
  mixed  per-stream rates (profiles/stream_rate/mixed_measured.txt), four sides alternated within this process over
         --rounds rounds of --ticks ticks each, p50 / p99 per side and round:
           a  ONE bank of S streams, half at 8000 and half at 48000 (StreamBank(sample_rate=[...]))
           b  what it takes without: a bank of S / 2 streams at 8000 and one of S / 2 at 48000, ticked one after the other
           c  a bank with per-stream rates whose S streams are all at 48000
           d  the single-rate bank of S streams at 48000 (c - d: the price of the per-stream descriptor)
  g711   G.711 input (profiles/stream_rate/g711_measured.txt), three sides alternated within this process over --rounds
         rounds of --ticks ticks each, S streams at 8000 Hz, p50 / p99 per side and round:
           a  the uniform mu-law bank (StreamBank(sample_rate=8000, sample_format="mulaw")) given the bytes
           b  the uniform int16 bank at 8000 given frames that were decoded beforehand (the decode is not timed)
           c  the bank of b with the host decode a caller needed without a: table[frames] in numpy inside the timed region
         and a catch-up: S streams x --seconds of mu-law in ONE feed of a causal Wavenet bank through ww_stream_feed_bytes against
         the host decode (table[packet] per stream) plus ww_stream_feed of the int16 bank, milliseconds per call.

One JSON line.  The single-rate modes use nothing this tool's commit added, so the file also runs on its parent."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "wakeword-detection_amd")]
import numpy as np  # noqa: E402
from wwhip.engine import Engine, StreamBank  # noqa: E402

ASSETS = os.path.join(ROOT, "wakeword-detection_amd/assets/tf_lite_models")


def _pct(lat):
    return {"p50_us": float(np.percentile(lat, 50) * 1e6), "p99_us": float(np.percentile(lat, 99) * 1e6), "mean_us": float(lat.mean() * 1e6)}


def tick(args):
    eng = Engine(os.path.join(ASSETS, args.model))
    kw = {} if args.rate == 16000 else {"sample_rate": args.rate}
    bank = StreamBank(eng, args.streams, **kw)
    F = args.rate // 50
    rng = np.random.default_rng(0)
    frames = np.clip(rng.normal(0, 2500, (64, args.streams, F)), -32768, 32767).astype(np.int16)
    speech = np.ones(args.streams, np.uint8)
    for t in range(100):
        bank.step(frames[t % 64], speech)
    lat = np.empty(args.ticks)
    n_post = 0
    for t in range(args.ticks):
        t0 = time.perf_counter()
        p, n = bank.step(frames[t % 64], speech)
        lat[t] = time.perf_counter() - t0
        n_post += int(n.sum())
    out = dict(mode="tick", model=args.model, rate=args.rate, streams=args.streams, ticks=args.ticks, posteriors_per_tick=n_post / args.ticks, **_pct(lat))
    if hasattr(bank, "timeline"):
        out["host_phases_us"] = {k: round(v, 2) for k, v in bank.timeline().items()}
    bank.close()
    eng.close()
    return out


def push(args):
    from wwhip.resample import StreamResampler
    eng = Engine(os.path.join(ASSETS, args.model))
    S, F = args.streams, args.rate // 50
    bank = StreamBank(eng, S)
    rs = [StreamResampler(args.rate, 16000, eng.ctx, dtype=np.int16) for _ in range(S)]
    rng = np.random.default_rng(0)
    frames = np.clip(rng.normal(0, 2500, (64, S, F)), -32768, 32767).astype(np.int16)
    speech = np.ones(S, np.uint8)
    queue = np.zeros((S, 4096), np.int16)
    held = np.zeros(S, int)
    block = np.zeros((S, 320), np.int16)

    def one(t):
        for s in range(S):
            y = rs[s].push(frames[t % 64, s])
            queue[s, held[s]:held[s] + len(y)] = y
            held[s] += len(y)
        if held.min() < 320:
            return 0
        block[:] = queue[:, :320]
        queue[:, :-320] = queue[:, 320:]
        held[:] -= 320
        return int(bank.step(block, speech)[1].sum())
    for t in range(20):
        one(t)
    lat = np.empty(args.ticks)
    n_post = 0
    for t in range(args.ticks):
        t0 = time.perf_counter()
        n_post += one(t)
        lat[t] = time.perf_counter() - t0
    bank.close()
    for r in rs:
        r.close()
    eng.close()
    return dict(mode="push", model=args.model, rate=args.rate, streams=S, ticks=args.ticks, posteriors_per_tick=n_post / args.ticks, **_pct(lat))


def feed(args):
    eng = Engine(os.path.join(ASSETS, "Wavenet"))
    kw = {} if args.rate == 16000 else {"sample_rate": args.rate}
    S, n = args.streams, int(args.rate * args.seconds)
    rng = np.random.default_rng(0)
    pk = [np.clip(rng.normal(0, 2500, n), -32768, 32767).astype(np.int16) for _ in range(S)]
    ms = []
    rows = 0
    bank = StreamBank(eng, S, causal=True, **kw)
    for rep in range(args.repeats + 1):  # (the first call sizes the scratch: not counted)
        bank.reset()
        t0 = time.perf_counter()
        posts, _ = bank.feed(list(range(S)), pk)
        ms.append((time.perf_counter() - t0) * 1e3)
        rows = sum(len(p) for p in posts)
    bank.close()
    eng.close()
    return dict(mode="feed", rate=args.rate, streams=S, seconds=args.seconds, rows=rows, ms_per_call=[round(v, 2) for v in ms[1:]],
                median_ms=float(np.median(ms[1:])))


def mixed(args):
    eng = Engine(os.path.join(ASSETS, args.model))
    S, H = args.streams, args.streams // 2
    rng = np.random.default_rng(0)

    def noise(*shape):
        return np.clip(rng.normal(0, 2500, shape), -32768, 32767).astype(np.int16)
    f8, f48, f48all = noise(64, H, 160), noise(64, H, 960), noise(64, S, 960)
    flat = [np.concatenate((f8[t].ravel(), f48[t].ravel())) for t in range(64)]  # streams 0 .. H - 1 at 8000, the rest at 48000
    sp_s, sp_h = np.ones(S, np.uint8), np.ones(H, np.uint8)
    a = StreamBank(eng, S, sample_rate=[8000] * H + [48000] * (S - H))
    b8, b48 = StreamBank(eng, H, sample_rate=8000), StreamBank(eng, S - H, sample_rate=48000)
    c = StreamBank(eng, S, sample_rate=[48000] * S)
    d = StreamBank(eng, S, sample_rate=48000)

    def tick_b(t):
        n = b8.step(f8[t], sp_h)[1].sum()
        return n + b48.step(f48[t], sp_h)[1].sum()
    sides = {"a": lambda t: a.step(flat[t], sp_s)[1].sum(), "b": tick_b, "c": lambda t: c.step(f48all[t].ravel(), sp_s)[1].sum(),
             "d": lambda t: d.step(f48all[t], sp_s)[1].sum()}
    for fn in sides.values():
        for t in range(100):
            fn(t % 64)
    rounds = {k: [] for k in sides}
    posts = {k: 0 for k in sides}
    for r in range(args.rounds):
        for k, fn in sides.items():
            lat = np.empty(args.ticks)
            for t in range(args.ticks):
                t0 = time.perf_counter()
                posts[k] += int(fn(t % 64))
                lat[t] = time.perf_counter() - t0
            rounds[k].append({q: round(v, 2) for q, v in _pct(lat).items()})
    for bank in (a, b8, b48, c, d):
        bank.close()
    eng.close()
    p50 = {k: [r["p50_us"] for r in v] for k, v in rounds.items()}
    return dict(mode="mixed", model=args.model, streams=S, ticks=args.ticks, rounds=rounds,
                posteriors_per_tick={k: v / (args.ticks * args.rounds) for k, v in posts.items()},
                p50_range_us={k: [min(v), max(v)] for k, v in p50.items()},
                a_below_b_beyond_spread=max(p50["a"]) < min(p50["b"]),
                c_minus_d_p50_us=[round(x - y, 2) for x, y in zip(p50["c"], p50["d"])])


def g711(args):
    from wwhip import g711 as g
    eng = Engine(os.path.join(ASSETS, args.model))
    S, F = args.streams, 160
    rng = np.random.default_rng(0)
    table = g.table("mulaw")
    codes = rng.integers(0, 256, (64, S, F), dtype=np.uint8)
    decoded = table[codes]
    sp = np.ones(S, np.uint8)
    a = StreamBank(eng, S, sample_rate=8000, sample_format="mulaw")
    b = StreamBank(eng, S, sample_rate=8000)
    sides = {"a": lambda t: a.step(codes[t], sp)[1].sum(), "b": lambda t: b.step(decoded[t], sp)[1].sum(),
             "c": lambda t: b.step(table[codes[t]], sp)[1].sum()}
    for fn in sides.values():
        for t in range(100):
            fn(t % 64)
    rounds = {k: [] for k in sides}
    posts = {k: 0 for k in sides}
    for r in range(args.rounds):
        for k, fn in sides.items():
            lat = np.empty(args.ticks)
            for t in range(args.ticks):
                t0 = time.perf_counter()
                posts[k] += int(fn(t % 64))
                lat[t] = time.perf_counter() - t0
            rounds[k].append({q: round(v, 2) for q, v in _pct(lat).items()})
    a.close()
    b.close()
    eng.close()
    # the catch-up feed
    wave = Engine(os.path.join(ASSETS, "Wavenet"))
    n = int(8000 * args.seconds)
    pk = [rng.integers(0, 256, n, dtype=np.uint8) for _ in range(S)]
    fa = StreamBank(wave, S, causal=True, sample_rate=8000, sample_format="mulaw")
    fb = StreamBank(wave, S, causal=True, sample_rate=8000)
    ids = list(range(S))
    ms = {"feed_bytes": [], "decode_then_feed": [], "decode_alone": []}
    rows = {}
    for rep_ in range(args.repeats + 1):  # (the first call sizes the scratch: not counted)
        fa.reset()
        t0 = time.perf_counter()
        posts_a, _ = fa.feed(ids, pk)
        ms["feed_bytes"].append((time.perf_counter() - t0) * 1e3)
        fb.reset()
        t0 = time.perf_counter()
        dec = [table[p] for p in pk]
        t1 = time.perf_counter()
        posts_b, _ = fb.feed(ids, dec)
        ms["decode_then_feed"].append((time.perf_counter() - t0) * 1e3)
        ms["decode_alone"].append((t1 - t0) * 1e3)
        rows = {"feed_bytes": sum(len(p) for p in posts_a), "decode_then_feed": sum(len(p) for p in posts_b)}
    same = all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(posts_a, posts_b))
    fa.close()
    fb.close()
    wave.close()
    p50 = {k: [r["p50_us"] for r in v] for k, v in rounds.items()}
    return dict(mode="g711", model=args.model, streams=S, ticks=args.ticks, rounds=rounds,
                posteriors_per_tick={k: v / (args.ticks * args.rounds) for k, v in posts.items()},
                p50_range_us={k: [min(v), max(v)] for k, v in p50.items()},
                a_minus_b_p50_us=[round(x - y, 2) for x, y in zip(p50["a"], p50["b"])],
                c_minus_a_p50_us=[round(x - y, 2) for x, y in zip(p50["c"], p50["a"])],
                feed=dict(seconds=args.seconds, rows=rows, same_bits=bool(same), ms_per_call={k: [round(v, 2) for v in x[1:]] for k, x in ms.items()},
                          median_ms={k: float(np.median(x[1:])) for k, x in ms.items()}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mode", choices=["tick", "push", "feed", "mixed", "g711"])
    ap.add_argument("--rate", type=int, default=48000, help="the streams' sample rate (a multiple of 50; 16000 = a plain bank)")
    ap.add_argument("--streams", type=int, default=128)
    ap.add_argument("--ticks", type=int, default=3000)
    ap.add_argument("--model", default="CRNN", choices=["CRNN", "Wavenet"])
    ap.add_argument("--seconds", type=float, default=10.0, help="feed: audio per stream and call")
    ap.add_argument("--repeats", type=int, default=3, help="feed: timed calls")
    ap.add_argument("--rounds", type=int, default=3, help="mixed: rounds the sides alternate over")
    a = ap.parse_args()
    print(json.dumps({"tick": tick, "push": push, "feed": feed, "mixed": mixed, "g711": g711}[a.mode](a)))
