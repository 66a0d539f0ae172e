#!/usr/bin/env python
"""Tacotron2 teacher forcing (pk_taco_teacher) against the free-running decode of the same batch, one JSON line each.

Workload: 32 utterances x 128 tokens x 640 frames, synthetic.TACOTRON2_LJSPEECH, seeded weights / ids / teacher frames, one
dropout seed per utterance.  ``teacher``: teacher_forced_batch on 640 given frames per utterance.  ``infer``: infer_batch with
a stop head biased off and max_decoder_steps = 640, i.e. exactly 640 steps.  Each figure is the median device-event time of
one whole call (encoder, decoder loop, read with the postnet), 2 warm-ups, >= 5 timed.

  python tools/bench_taco_teacher.py [--which both|teacher|infer] [--tree DIR] [--iters 7] [--out FILE]

``--tree``: import parakeet_amd from another checkout of the project (the parent commit, built), to time its infer_batch on
the same box.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch


def timed(fn, warm, iters):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), [round(t, 3) for t in ts]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--which", default="both", choices=("both", "teacher", "infer"))
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--utts", type=int, default=32)
    ap.add_argument("--tokens", type=int, default=128)
    ap.add_argument("--frames", type=int, default=640)
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--out", default=None, help="append the lines to this file")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    from parakeet_amd import build as pk_build
    from parakeet_amd import synthetic as syn
    from parakeet_amd.runtime import Context
    from parakeet_amd.tacotron2 import Tacotron2
    Context.get()
    cfg = dict(syn.TACOTRON2_LJSPEECH)
    m = Tacotron2(**cfg)
    m.set_state_dict(syn.tacotron2_state(cfg, seed=5, stop_bias=-30.0))       # sigmoid(stop_logit) > 0.5 never fires
    m.eval()
    rng = np.random.default_rng(7)
    texts = [rng.integers(1, cfg["vocab_size"], size=args.tokens) for _ in range(args.utts)]
    mels = [(0.5 * rng.standard_normal((args.frames, 80))).astype(np.float32) for _ in range(args.utts)]
    seeds = list(range(args.utts))
    base = {"utts": args.utts, "tokens": args.tokens, "frames": args.frames, "device": torch.cuda.get_device_name(0),
            "host": os.uname().nodename, "tree": os.path.abspath(args.tree), "source_hash": pk_build.source_hash()[:16]}
    lines = []
    if args.which in ("both", "teacher"):
        dev = [torch.as_tensor(x).cuda() for x in mels]
        for name, arg in (("teacher_host_mels", mels), ("teacher_device_mels", dev)):
            got = []

            def tf():
                got[:] = [int(o["mel_output"].shape[0]) for o in m.teacher_forced_batch(texts, arg, seeds=seeds)]
            ms, raw = timed(tf, 2, args.iters)
            assert got == [args.frames] * args.utts
            lines.append(dict(base, variant=name, ms=round(ms, 3), us_per_step=round(ms * 1e3 / args.frames, 1), raw_ms=raw))
            print(json.dumps(lines[-1]), flush=True)
    if args.which in ("both", "infer"):
        got = []

        def ar():
            got[:] = [int(o["mel_output"].shape[0]) for o in m.infer_batch(texts, max_decoder_steps=args.frames, seeds=seeds)]
        ms, raw = timed(ar, 2, args.iters)
        assert got == [args.frames] * args.utts, got
        lines.append(dict(base, variant="infer_batch", ms=round(ms, 3), us_per_step=round(ms * 1e3 / args.frames, 1), raw_ms=raw))
        print(json.dumps(lines[-1]), flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write("".join(json.dumps(x) + "\n" for x in lines))


if __name__ == "__main__":
    main()
