#!/usr/bin/env python3
"""wwdetect/CRNN/evaluate.py for a CTC-trained CRNN (its ``eval_CTC`` branch) on the HIP path: every record of
``<data_dir>/test.h5`` is one window - truncated to 151 frames and zero-padded on the device -, the window's 19 rows of label
posteriors are greedy-CTC-decoded there, and a clip counts as a wake word iff its first two labels read [HEY][SNIPS].

    python tools/evaluate_ctc.py --data_dir <dir with test.h5> --model_dir <a CRNN model directory> --ctc_head head.npz

No converted CTC model exists to read, so the model is given in two parts: ``--model_dir`` is a directory of the
standard CRNN geometry (filter / encode / detect ``.tflite``: its filter, conv and two BiGRU layers are used, its detect head is
not), ``--ctc_head`` an ``.npz`` with ``w [L, 64]`` and ``b [L]`` of the TimeDistributed dense layer (Keras stores the kernel as
``[64, L]``: pass ``--keras_kernel`` to have it transposed).  The H5 file is read by h5py where installed, by ``wwhip.h5min``
otherwise."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "wakeword-detection_amd")]

import numpy as np  # noqa: E402

from wwhip import weights as W  # noqa: E402
from wwhip.engine import Engine  # noqa: E402
from wwhip.evaluate import evaluate_ctc, open_h5  # noqa: E402


def ctc_bundle(model_dir: str, head_path: str, keras_kernel: bool = False):
    base = W.load_model_dir(model_dir)
    if base.kind != W.KIND_CRNN:
        raise ValueError(f"{model_dir} is not a CRNN")
    with np.load(head_path) as z:
        w, b = np.asarray(z["w"], np.float32), np.asarray(z["b"], np.float32)
    base.crnn = W.crnn_ctc_params(base.crnn, w.T if keras_kernel else w, b)
    return base


def read_records(path: str):
    """``(features, is_hotword, keys)`` of a DatasetFilter feature file, in the file's name order."""
    feats, labels, keys = [], [], []
    with open_h5(path) as h5:
        for key in h5.keys():
            keys.append(key)
            labels.append(int(h5[key].attrs["is_hotword"]))
            feats.append(np.asarray(h5[key][()], np.float32))
    return feats, labels, keys


def parse_args():
    p = argparse.ArgumentParser(description="Evaluates a CTC-trained CRNN model.")
    p.add_argument("--data_dir", type=str, default="data_speech_isolated/silero", help="Directory where test data is stored.")
    p.add_argument("--model_dir", type=str, default=os.path.join(ROOT, "wakeword-detection_amd/assets/tf_lite_models/CRNN"))
    p.add_argument("--ctc_head", type=str, required=True, help=".npz with w [L, 64] and b [L] (the blank is the last class)")
    p.add_argument("--keras_kernel", action="store_true", help="w is stored as Keras keeps it, [64, L]")
    p.add_argument("--testset", type=str, default="test.h5")
    p.add_argument("--thresholds", type=int, default=0, metavar="N",
                   help="also score every clip with the CTC forward algorithm (P(decode == [HEY][SNIPS])) and print the FAR/FRR sweep over N "
                        "thresholds evenly spaced in (0, 1)")
    p.add_argument("--score_mode", type=str, default="exact", choices=("exact", "prefix"), help="exact: the decode IS the target; prefix: starts with it")
    p.add_argument("--align", action="store_true",
                   help="also print, per clip, where the best [HEY][SNIPS] path (Viterbi, --score_mode) lies: each label's seconds into the clip")
    p.add_argument("--beam", type=int, default=0, metavar="W",
                   help="apply the [HEY][SNIPS] rule to the most probable label string found by prefix beam search of width W (1..64) instead "
                        "of the greedy decode: eval_CTC with greedy=False")
    return p.parse_args()


def main(args):
    feats, labels, keys = read_records(os.path.join(args.data_dir, args.testset))
    eng = Engine(args.model_dir, bundle=ctc_bundle(args.model_dir, args.ctc_head, args.keras_kernel))
    thr = np.linspace(0.0, 1.0, args.thresholds + 2)[1:-1] if args.thresholds > 0 else None
    stats = evaluate_ctc(eng, feats, labels, thresholds=thr, mode=args.score_mode, align=args.align, beam_width=args.beam or None)
    eng.close()
    if args.beam:
        print(f"beam search, width {args.beam}: top string's probability median {np.median(stats['beam_probs']) if len(feats) else float('nan'):.3g}")
    print("False accept files:", [k for k, p, t in zip(keys, stats["predicted"], labels) if p and not t])
    print("False reject files:", [k for k, p, t in zip(keys, stats["predicted"], labels) if t and not p])
    for name in ("tp", "fp", "tn", "fn", "precision", "recall"):
        print(f"{name}: {float(stats[name])}")
    print(f"balanced accuracy: {stats['balanced accuracy']}")
    if thr is not None:
        print(f"score ({args.score_mode}): wake-word clips median {np.median(stats['scores'][np.asarray(labels, bool)]) if any(labels) else float('nan'):.3g}, "
              f"others median {np.median(stats['scores'][~np.asarray(labels, bool)]) if not all(labels) else float('nan'):.3g}")
        print("threshold  FRR  FA/h  FA")
        for t, frr, fa, cnt in zip(stats["thresholds"], stats["frr"], stats["fa_per_hour"], stats["fa_count"]):
            print(f"{t:.4f}  {frr:.4f}  {fa:.3f}  {int(cnt)}")
    if args.align:
        print(f"clip  path probability ({args.score_mode})  [HEY] s  [SNIPS] s")
        for key, val, sec in zip(keys, stats["align_value"], stats["span_seconds"]):
            print(f"{key}  {val:.3g}  " + "  ".join("-" if np.isnan(a) else f"{a:.2f}-{b:.2f}" for a, b in sec))
    return stats


if __name__ == "__main__":
    main(parse_args())
