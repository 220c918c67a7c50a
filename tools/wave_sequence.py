#!/usr/bin/env python3
"""The fp32 Wavenet's sequence form, measured (profiles/EXPERIMENTS.md).

  throughput  the hey-snips-size stand-in of tools/eval_at_scale.py joined into one stream, mel resident on the device: the
              sequence form (ww_wave_sequence_dev: post_frames of every row) against the window form at hop 2
              (ww_forward_segments_dev), alternated in one process; time per 10 ms frame of audio and the sequence kernel's
              achieved FLOP/s at 113.5 kFLOP per row.  --once: one untimed call of the sequence form (for a kernel trace).
  latency     StreamBank.step p50 / p99 at S streams: the causal bank against the window bank, alternated in blocks of ticks.
  distance    on the clips of tools/eval_testset.py: how far post_frames lies from the window form's posterior at the same end
              row, in logit units (the two readings differ by their left context; this is a description, not a check).

  feed        StreamBank.feed measured: catch-up (S streams x N seconds in ONE feed against the tick loop over the same audio on a
              twin bank, alternated), lock step (a feed of 320 samples per stream against step, polled and sync_wait, p50 / p99,
              alternated in blocks) and one stream's hour in one packet against Engine.logmel + sequence_forward, with the library's
              per-kernel times.  --part catchup | lockstep | hour | once (one untimed 1 h feed, for a kernel trace) | all.

  set         a model set's sequence form: ONE ww_set_wave_sequence_all_dev call for K slots (the two shipped Wavenets, repeated)
              against K ww_wave_sequence_dev calls of the members' engines over the same resident mel, post_frames of every row,
              alternated; at two shapes - --seqs sequences of --rows rows (clips) and one sequence of --long-rows rows (a recording) -
              and K = 1, 2, 4, 8.  The outputs of the two sides are compared bit for bit.

usage: wave_sequence.py set [--seqs 256] [--rows 300] [--long-rows 360000] [--reps 9] |
       wave_sequence.py feed [--part all] [--streams 128] [--seconds 10] [--reps 5] [--ticks 4000] |
       wave_sequence.py throughput [--model Wavenet] [--reps 5] [--once] | latency [--streams 128] [--ticks 4000] |
       distance [--clips 256]"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "wakeword-detection_amd")]
import numpy as np

FLOP_PER_ROW = 20.66e6 / 182  # the network's work per frame: one window's 20.66 MFLOP over its 182 rows


def _engine(model):
    from wwhip.engine import Engine
    return Engine(os.path.join(ROOT, "wakeword-detection_amd/assets/tf_lite_models", model))


def _spread(v):
    v = np.asarray(v, float)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()), "n": int(v.size)}


def throughput(args):
    import torch
    from wwhip.evaluate import synth_testset_scaled
    eng = _engine(args.model)
    clips, _ = synth_testset_scaled(args.wake, args.wake)
    pcm = np.concatenate(clips)
    hours = len(pcm) / 16000 / 3600
    mel = eng.logmel([pcm])[0]
    rows, T, NO = len(mel), eng.window, eng.n_out
    d_mel = torch.from_numpy(mel).cuda()
    nw = (rows - T) // 2 + 1
    d_pf = torch.empty((rows, NO), dtype=torch.float32, device="cuda")
    d_win = torch.empty((nw, NO), dtype=torch.float32, device="cuda")
    offs = np.array([0, rows], np.int64)
    seq = lambda: eng.wave_sequence_dev(d_mel.data_ptr(), rows, offs, d_post_frames_ptr=d_pf.data_ptr())
    win = lambda: eng.forward_segments_dev(d_mel.data_ptr(), rows, np.array([0], np.int64), np.array([nw], np.int32), 2, d_win.data_ptr())
    torch.cuda.synchronize()
    if args.once:
        seq(); eng.ctx.synchronize()
        print(json.dumps({"rows": rows, "once": True}))
        return

    def timed(f):
        eng.ctx.synchronize()
        t0 = time.perf_counter(); f(); eng.ctx.synchronize()
        return time.perf_counter() - t0
    for f in (seq, win, seq, win):  # warm-up: code objects, the context's workspace at its final size
        timed(f)
    t_seq, t_win = [], []
    for _ in range(args.reps):      # the two sides alternated
        t_seq.append(timed(seq)); t_win.append(timed(win))
    eng.ctx.profile(True); seq(); prof = eng.ctx.profile_read(); eng.ctx.profile(False)
    k_ms = prof["wavenet_seq_kernel"]["total_ms"]
    # the same end rows: window w ends at row 2 w + T - 1
    pf, pw = d_pf.cpu().numpy(), d_win.cpu().numpy()
    frames = len(pcm) / 160
    out = {"model": args.model, "audio_hours": round(hours, 3), "mel_rows": rows, "windows_hop2": nw,
           "sequence_s": _spread(t_seq), "window_hop2_s": _spread(t_win),
           "sequence_ns_per_10ms_frame": float(np.median(t_seq)) / frames * 1e9, "window_hop2_ns_per_10ms_frame": float(np.median(t_win)) / frames * 1e9,
           "speedup_median": float(np.median(t_win) / np.median(t_seq)),
           "kernels_ms_one_call": {k: round(v["total_ms"], 3) for k, v in prof.items()},
           "wavenet_seq_kernel_TFLOPs": rows * FLOP_PER_ROW / (k_ms * 1e-3) / 1e12,
           "max_abs_dp_same_end_row": float(np.abs(pf[T - 1::2][:nw] - pw).max()),
           "checksum_sequence": float(pf.sum(dtype=np.float64)), "checksum_window": float(pw.sum(dtype=np.float64))}
    print(json.dumps(out))


def latency(args):
    from wwhip.engine import StreamBank
    eng = _engine(args.model)
    S = args.streams
    rng = np.random.default_rng(0)
    frames = np.clip(rng.normal(0, 2500, (64, S, 320)), -32768, 32767).astype(np.int16)
    speech = np.ones(S, np.uint8)
    banks = {"causal": StreamBank(eng, S, causal=True), "window": StreamBank(eng, S)}
    lat = {k: [] for k in banks}
    for k, b in banks.items():
        for t in range(300):
            b.step(frames[t % 64], speech)
    block = 500
    for t0 in range(0, args.ticks, block):  # alternated in blocks of ticks
        for k, b in banks.items():
            for t in range(t0, min(t0 + block, args.ticks)):
                a = time.perf_counter(); b.step(frames[t % 64], speech); lat[k].append(time.perf_counter() - a)
    out = {"model": args.model, "streams": S, "ticks": args.ticks}
    for k in banks:
        v = np.array(lat[k]) * 1e6
        halves = [float(np.percentile(h, 50)) for h in np.array_split(v, 4)]
        out[k] = {"p50_us": float(np.percentile(v, 50)), "p99_us": float(np.percentile(v, 99)), "mean_us": float(v.mean()),
                  "p50_us_by_quarter": halves}
        banks[k].close()
    print(json.dumps(out))


def feed(args):
    from wwhip.engine import StreamBank
    eng = _engine(args.model)
    rng = np.random.default_rng(0)
    out = {"model": args.model}
    noise = lambda *shape: np.clip(rng.normal(0, 2500, shape), -32768, 32767).astype(np.int16)

    def clock(f):
        a = time.perf_counter(); f(); return time.perf_counter() - a   # (step and feed both return after a synchronise / their posteriors)

    if args.part in ("catchup", "all"):
        for S, seconds in ((args.streams, args.seconds), (1024, 1)):
            ticks = seconds * 50
            pcm = noise(S, ticks * 320)
            ids, speech = list(range(S)), np.ones(S, np.uint8)
            fed, ticked = StreamBank(eng, S, causal=True), StreamBank(eng, S, causal=True)
            packets = [pcm[s] for s in range(S)]

            def tick_loop():
                for t in range(ticks):
                    ticked.step(pcm[:, t * 320:(t + 1) * 320], speech)
            t_feed, t_tick = [], []
            for r in range(args.reps + 1):   # alternated; the first pair is the warm-up (code objects, the call's scratch at its size)
                a, b = clock(lambda: fed.feed(ids, packets)), clock(tick_loop)
                if r:
                    t_feed.append(a); t_tick.append(b)
            eng.ctx.profile(True); fed.feed(ids, packets); prof = eng.ctx.profile_read(); eng.ctx.profile(False)
            out[f"catchup_{S}x{seconds}s"] = {"feed_ms": _spread(np.array(t_feed) * 1e3), "tick_loop_ms": _spread(np.array(t_tick) * 1e3), "ticks": ticks,
                                             "speedup_median": float(np.median(t_tick) / np.median(t_feed)),
                                             "spreads_overlap": bool(max(t_feed) >= min(t_tick)),
                                             "feed_kernels_ms_one_call": {k: round(v["total_ms"], 3) for k, v in prof.items()}}
            fed.close(); ticked.close()
    if args.part in ("lockstep", "all"):
        S = args.streams
        frames = noise(64, S, 320)
        ids, speech = list(range(S)), np.ones(S, np.uint8)
        banks = {"feed": StreamBank(eng, S, causal=True), "step_polled": StreamBank(eng, S, causal=True), "step_sync_wait": StreamBank(eng, S, causal=True, sync_wait=True)}
        call = {k: ((lambda f, b=b: b.feed(ids, list(f))) if k == "feed" else (lambda f, b=b: b.step(f, speech))) for k, b in banks.items()}
        lat = {k: [] for k in banks}
        for k in banks:
            for t in range(300):
                call[k](frames[t % 64])
        block = 500
        for t0 in range(0, args.ticks, block):
            for k in banks:
                for t in range(t0, min(t0 + block, args.ticks)):
                    f = frames[t % 64]
                    a = time.perf_counter(); call[k](f); lat[k].append(time.perf_counter() - a)
        ls = {"streams": S, "calls": args.ticks}
        for k, b in banks.items():
            v = np.array(lat[k]) * 1e6
            ls[k] = {"p50_us": float(np.percentile(v, 50)), "p99_us": float(np.percentile(v, 99)), "mean_us": float(v.mean()),
                     "p50_us_by_quarter": [float(np.percentile(h, 50)) for h in np.array_split(v, 4)]}
            b.close()
        out["lockstep"] = ls
    if args.part in ("hour", "once", "all"):
        pcm = noise(3600 * 16000)
        bank = StreamBank(eng, 1, causal=True)
        if args.part == "once":
            bank.feed([0], [pcm]); bank.close()
            print(json.dumps({"once": True, "samples": len(pcm)}))
            return
        two = lambda: eng.sequence_forward(eng.logmel([pcm]), pool=eng.window, want=("post_frames",))
        one = lambda: (bank.reset(), bank.feed([0], [pcm]))
        t_one, t_two = [], []
        for r in range(args.reps + 1):
            a, b = clock(one), clock(two)
            if r:
                t_one.append(a); t_two.append(b)
        bank.reset()
        eng.ctx.profile(True); p, _ = bank.feed([0], [pcm]); prof = eng.ctx.profile_read(); eng.ctx.profile(False)
        eng.ctx.profile(True); two(); prof2 = eng.ctx.profile_read(); eng.ctx.profile(False)
        out["hour"] = {"rows": int(len(p[0])), "feed_ms": _spread(np.array(t_one) * 1e3), "logmel_plus_sequence_ms": _spread(np.array(t_two) * 1e3),
                       "feed_kernels_ms": {k: round(v["total_ms"], 3) for k, v in prof.items()},
                       "logmel_plus_sequence_kernels_ms": {k: round(v["total_ms"], 3) for k, v in prof2.items()}}
        bank.close()
    print(json.dumps(out))


def set_form(args):
    import torch
    from wwhip.engine import ModelSet
    names = ["Wavenet", "Wavenet_alt"]
    engines = [_engine(n) for n in names]
    ms = ModelSet(engines)
    NO = ms.n_out
    rng = np.random.default_rng(0)
    out = {"members": names, "reps": args.reps, "shapes": []}

    def timed(f):
        ms.ctx.synchronize()
        t0 = time.perf_counter(); f(); ms.ctx.synchronize()
        return time.perf_counter() - t0
    for label, n_seq, rows_each in (("clips", args.seqs, args.rows), ("recording", 1, args.long_rows)):
        rows = n_seq * rows_each
        d_mel = torch.from_numpy(rng.uniform(0.0, 6.0, (rows, 40)).astype(np.float32)).cuda()
        offs = np.arange(n_seq + 1, dtype=np.int64) * rows_each
        shape = {"shape": label, "sequences": n_seq, "rows_each": rows_each, "by_slots": []}
        for K in (1, 2, 4, 8):
            slots = [k % len(engines) for k in range(K)]
            d_one = torch.empty((K, rows, NO), dtype=torch.float32, device="cuda")
            d_many = torch.empty((K, rows, NO), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            one = lambda: ms.wave_sequence_all_dev(d_mel.data_ptr(), rows, offs, slots, d_post_frames_ptr=d_one.data_ptr())

            def many():
                for k, m in enumerate(slots):
                    engines[m].wave_sequence_dev(d_mel.data_ptr(), rows, offs, d_post_frames_ptr=d_many[k].data_ptr())
            for f in (one, many, one, many):  # warm-up: code objects, the context's workspace at its final size
                timed(f)
            t_one, t_many = [], []
            for _ in range(args.reps):        # the two sides alternated
                t_one.append(timed(one)); t_many.append(timed(many))
            ms.ctx.profile(True); one(); prof = ms.ctx.profile_read(); ms.ctx.profile(False)
            shape["by_slots"].append({"slots": K, "one_call_ms": _spread(np.array(t_one) * 1e3), "k_calls_ms": _spread(np.array(t_many) * 1e3),
                                      "k_calls_over_one_call_median": float(np.median(t_many) / np.median(t_one)),
                                      "spreads_overlap": bool(max(t_one) >= min(t_many) and max(t_many) >= min(t_one)),
                                      "one_call_kernels_ms": {k: round(v["total_ms"], 3) for k, v in prof.items()},
                                      "one_call_kernel_scopes": {k: int(v["calls"]) for k, v in prof.items()},
                                      "same_bits": bool(torch.equal(d_one, d_many))})
        out["shapes"].append(shape)
    ms.close()
    print(json.dumps(out))


def distance(args):
    from wwhip.evaluate import synth_testset
    eng = _engine(args.model)
    clips, _ = synth_testset(args.clips)
    mels = [m for m in eng.logmel(clips) if len(m) >= eng.window]
    T, c = eng.window, eng.posterior_index
    pf = eng.sequence_forward(mels, want=("post_frames",))["post_frames"]
    d = []
    lg = lambda p: np.log(np.clip(p, 1e-30, None)) - np.log(np.clip(1 - p, 1e-30, None))
    for m, f in zip(mels, pf):
        w = eng.slide_forward(m, 1)
        d.append(np.abs(lg(f[T - 1:, c].astype(np.float64)) - lg(w[:, c].astype(np.float64))))
    d = np.concatenate(d)
    first = np.array([abs(lg(float(f[T - 1, c])) - lg(float(eng.slide_forward(m[:T], 1)[0, c]))) for m, f in zip(mels[:8], pf[:8])])
    print(json.dumps({"model": args.model, "clips": len(mels), "end_rows": int(d.size), "logit_distance_median": float(np.median(d)),
                      "logit_distance_p99": float(np.percentile(d, 99)), "logit_distance_max": float(d.max()),
                      "at_row_T_minus_1_max": float(first.max())}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["throughput", "latency", "distance", "feed", "set"])
    ap.add_argument("--model", default="Wavenet")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--wake", type=int, default=2529)
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--streams", type=int, default=128)
    ap.add_argument("--ticks", type=int, default=4000)
    ap.add_argument("--clips", type=int, default=256)
    ap.add_argument("--seconds", type=int, default=10)
    ap.add_argument("--seqs", type=int, default=256)
    ap.add_argument("--rows", type=int, default=300)
    ap.add_argument("--long-rows", type=int, default=360000)
    ap.add_argument("--part", default="all", choices=["all", "catchup", "lockstep", "hour", "once"])
    a = ap.parse_args()
    {"throughput": throughput, "latency": latency, "distance": distance, "feed": feed, "set": set_form}[a.what](a)
