#!/usr/bin/env python
"""FastSpeech2 with given targets against plain inference at the benchmark's shape: 32 utterances x 128 tokens -> 640
frames each (5 frames per token), LJSpeech configuration.  ``teacher_forced_batch`` (given durations, pitch, energy) and
``inference_batch`` (a model whose duration predictor answers 5 for every token) run in one process on one device; each
figure is the median over ``--steps`` calls after ``--warmup``, timed with a device synchronise around the call.
Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--tokens", type=int, default=128)
    ap.add_argument("--frames-per-token", type=int, default=5)
    args = ap.parse_args(argv)
    import torch
    from parakeet_amd import synthetic as syn
    from parakeet_amd.fastspeech2 import FastSpeech2
    cfg = dict(syn.FS2_LJSPEECH)
    model = FastSpeech2(80, 80, **cfg)
    model.set_state_dict(syn.fastspeech2_state(80, 80, cfg, seed=1, fixed_duration=args.frames_per_token))
    model.eval()
    B, T = args.batch, args.tokens
    texts = [syn.phoneme_ids(T, 80, seed=100 + b) for b in range(B)]
    pred = model.predict_batch(texts)
    assert all(int(d.sum()) == T * args.frames_per_token for d, _, _ in pred)
    ds, ps, es = [p[0] for p in pred], [p[1] for p in pred], [p[2] for p in pred]

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.steps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ms)), float(np.min(ms))

    plain = timed(lambda: model.inference_batch(texts))
    forced = timed(lambda: model.teacher_forced_batch(texts, ds, ps, es))
    forced_before = timed(lambda: model.teacher_forced_batch(texts, ds, ps, es, return_before=True))
    print(json.dumps(dict(shape=f"{B}x{T}->{T * args.frames_per_token}", steps=args.steps,
                          inference_batch_ms=round(plain[0], 4), inference_batch_min_ms=round(plain[1], 4),
                          teacher_forced_batch_ms=round(forced[0], 4), teacher_forced_batch_min_ms=round(forced[1], 4),
                          teacher_forced_batch_with_before_ms=round(forced_before[0], 4),
                          ratio=round(forced[0] / plain[0], 4))))


if __name__ == "__main__":
    main()
