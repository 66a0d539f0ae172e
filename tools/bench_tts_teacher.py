#!/usr/bin/env python
"""TransformerTTS teacher forcing (pk_tts_teacher) against the AR decode of the same batch, one JSON line per variant.

Workload: 32 utterances x 128 tokens x 640 teacher frames, synthetic.TRANSFORMER_TTS_LJSPEECH (6 + 6 layers, adim 512,
8 x 64 heads, dunits 1024), seeded weights / ids / spectrograms.  Variants: teacher forcing at the default math (f16x3) and
at f32, each with and without the attention weights; then the AR decode (inference_batch, stop head biased off, maxlen 640
steps) of the same texts.  Reports the median device-event time of one call (2 warm-ups, >= 5 timed; the AR decode 1 + 3),
the FLOP count of the teacher pass from the shapes (every GEMM 2 M N K, the causal self-attention 2 x 2 L^2 A / 2 per
utterance and layer, the encoder-decoder attention 2 x 2 L T A) and its rate, and the speed-up over the AR decode.

  python tools/bench_tts_teacher.py [--utts 32] [--tokens 128] [--frames 640] [--iters 5] [--out FILE] [--skip-ar]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from parakeet_amd import synthetic as syn  # noqa: E402
from parakeet_amd.runtime import Context  # noqa: E402
from parakeet_amd.transformer_tts import TransformerTTS  # noqa: E402


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
    return float(np.median(ts))


def teacher_flops(cfg, B, T, L):
    """FLOPs of one teacher-forced batch from the shapes (T tokens + <eos>, L decoder rows per utterance)."""
    A, E, D, U, O = cfg["adim"], cfg["eunits"], cfg["dunits"], cfg["dprenet_units"], 80
    Te = T + 1
    enc_rows, dec_rows = B * Te, B * L
    f = 0.0
    f += cfg["elayers"] * enc_rows * 2 * (3 * A * A + A * A + 2 * A * E)            # encoder GEMMs (k = 1 convs)
    f += cfg["elayers"] * B * 2 * 2 * Te * Te * A                                     # encoder attention
    f += cfg["dlayers"] * enc_rows * 2 * (2 * A * A)                                  # memory k | v
    f += dec_rows * 2 * (O * U + U * U + U * A)                                        # prenet + input Linear
    f += cfg["dlayers"] * dec_rows * 2 * (3 * A * A + 3 * A * A + 2 * A * D)          # q|k|v, out, src_q, src_out, FFN
    f += cfg["dlayers"] * B * 2 * 2 * L * L * A / 2                                   # causal self-attention
    f += cfg["dlayers"] * B * 2 * 2 * L * Te * A                                      # encoder-decoder attention
    f += dec_rows * 2 * A * O                                                          # feat_out
    return f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=32)
    ap.add_argument("--tokens", type=int, default=128)
    ap.add_argument("--frames", type=int, default=640)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    ap.add_argument("--skip-ar", action="store_true", help="teacher variants only (kernel traces of the teacher pass)")
    args = ap.parse_args()
    Context.get()
    cfg = dict(syn.TRANSFORMER_TTS_LJSPEECH)
    idim = 80
    state = syn.transformer_tts_state(idim, 80, cfg, seed=5, stop_bias=-30.0)
    m = TransformerTTS(idim=idim, odim=80, **cfg)
    m.set_state_dict(state)
    m.eval()
    texts = [syn.phoneme_ids(args.tokens, idim=idim, seed=100 + b) for b in range(args.utts)]
    rng = np.random.default_rng(7)
    speech = [rng.standard_normal((args.frames, 80)).astype(np.float32) for _ in range(args.utts)]
    seeds = list(range(args.utts))
    flops = teacher_flops(cfg, args.utts, args.tokens, args.frames)
    lines = []
    for math in ("f16x3", "f32"):
        m.set_math(math)
        for att in (False, True):
            ms = timed(lambda: m.teacher_forced_batch(texts, speech, seeds, return_att=att), 2, args.iters)
            lines.append({"variant": "teacher", "math": math, "att": att, "utts": args.utts, "tokens": args.tokens,
                          "frames": args.frames, "ms": round(ms, 3), "tflop": round(flops / 1e12, 4),
                          "tflops_per_s": round(flops / (ms * 1e-3) / 1e12, 1)})
            print(json.dumps(lines[-1]), flush=True)
    if args.skip_ar:
        return
    m.set_math("f16x3")
    ratio = (args.frames + 0.5) / (args.tokens + 1)                    # maxlen = int((T + 1) * ratio) = frames steps
    frames_ar = []

    def ar():
        outs = m.inference_batch(texts, maxlenratio=ratio, seeds=seeds, return_att=False)
        frames_ar[:] = [int(o[0].shape[0]) for o in outs]
    ms_ar = timed(ar, 1, 3)
    assert frames_ar == [args.frames] * args.utts, frames_ar
    lines.append({"variant": "ar_decode", "math": "f16x3", "att": False, "utts": args.utts, "tokens": args.tokens,
                  "frames": args.frames, "ms": round(ms_ar, 3), "us_per_step": round(ms_ar * 1e3 / args.frames, 1)})
    print(json.dumps(lines[-1]), flush=True)
    for x in lines[:-1]:
        x["speedup_vs_ar"] = round(ms_ar / x["ms"], 1)
    summary = {"summary": "teacher f16x3 without att vs AR decode", "teacher_ms": lines[0]["ms"], "ar_ms": round(ms_ar, 3),
               "speedup": lines[0]["speedup_vs_ar"]}
    print(json.dumps(summary), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("".join(json.dumps(x) + "\n" for x in lines + [summary]))


if __name__ == "__main__":
    main()
