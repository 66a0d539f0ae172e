#!/usr/bin/env python
"""SpeedySpeech with given durations beside free-running inference at the same durations, and the masked-L1 + SSIM pass on the
resulting pair; one JSON line each.

Workload: 32 utterances x 128 tokens, every duration 5 -> 640 frames each, baker configuration, synthetic state.
``teacher_forced_batch`` runs the kernels of ``inference_batch`` without the host wait for the frame counts; the two are
timed alternately (20 rounds of one call each, after 5 warm-ups) so that drift of the machine hits both.  ``inference_batch``
is given the same lengths by a duration head whose weights are zero and whose bias is ln 5.  ``pk_mel_loss_run`` reads the
32 x 640 x 80 pair (13.1 MB) once; its time stands beside that of an empty pair (B = 1, one row: launches, table upload and
nothing else), the call's floor.  Each figure is the median device-event time of one whole call.

  python tools/bench_speedyspeech_forward.py [--utts 32] [--tokens 128] [--duration 5] [--iters 20] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=32)
    ap.add_argument("--tokens", type=int, default=128)
    ap.add_argument("--duration", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None, help="append the lines to this file")
    args = ap.parse_args()
    from parakeet_amd import build as pk_build
    from parakeet_amd import synthetic as syn
    from parakeet_amd.losses import mel_loss_sums
    from parakeet_amd.speedyspeech import SpeedySpeech
    B, T, d = args.utts, args.tokens, args.duration
    state = syn.speedyspeech_state(seed=303)
    state["duration_predictor.layers.3.weight"] = np.zeros_like(state["duration_predictor.layers.3.weight"])
    state["duration_predictor.layers.3.bias"] = np.full_like(state["duration_predictor.layers.3.bias"], np.log(d))
    m = SpeedySpeech(vocab_size=70, tone_size=7, **syn.SPEEDYSPEECH_BAKER)
    m.set_state_dict(state)
    m.eval()
    rng = np.random.default_rng(5)
    texts = [rng.integers(1, 70, T) for _ in range(B)]
    tones = [rng.integers(1, 7, T) for _ in range(B)]
    durs = [np.full(T, d, np.int64) for _ in range(B)]
    free = m.inference_batch(texts, tones)
    forced = m.teacher_forced_batch(texts, durs, tones)
    assert all(f.shape == (T * d, m.odim) for f in free)
    same = all(torch.equal(a, b) for a, b in zip(free, forced))
    base = {"utts": B, "tokens": T, "frames": T * d, "device": torch.cuda.get_device_name(0), "host": os.uname().nodename,
            "source_hash": pk_build.source_hash()[:16]}
    fns = {"teacher_forced_batch": lambda: m.teacher_forced_batch(texts, durs, tones),
           "inference_batch": lambda: m.inference_batch(texts, tones)}
    for _ in range(5):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    raw = {k: [] for k in fns}
    for _ in range(args.iters):
        for k, fn in fns.items():
            raw[k].append(event_ms(fn))
    lines = [dict(base, name=k, ms=round(float(np.median(v)), 3), raw_ms=[round(t, 3) for t in v],
                  bit_identical_outputs=same) for k, v in raw.items()]
    pred = torch.cat(forced)
    target = pred + 0.1 * torch.randn_like(pred)
    lens = [T * d] * B
    one = torch.zeros(1, m.odim, device=pred.device)
    lf = {"mel_loss_32x640x80": lambda: mel_loss_sums(pred, target, lens), "mel_loss_floor_1x1x80": lambda: mel_loss_sums(one, one, [1])}
    for _ in range(5):
        for fn in lf.values():
            fn()
    torch.cuda.synchronize()
    raw = {k: [] for k in lf}
    for _ in range(args.iters):
        for k, fn in lf.items():
            raw[k].append(event_ms(fn))
    nbytes = 2.0 * pred.numel() * 4
    ctx = m._ctx
    ctx.prof_enable(True)
    ctx.prof_reset()
    for _ in range(args.iters):
        mel_loss_sums(pred, target, lens)
    ctx.sync()
    prof = ctx.prof_dump()
    ctx.prof_enable(False)
    kern = {k: round(ms / n * 1e3, 2) for k, (n, ms) in prof.items() if k.startswith("mel_loss")}
    for k, v in raw.items():
        ms = float(np.median(v))
        ln = dict(base, name=k, ms=round(ms, 4), raw_ms=[round(t, 4) for t in v])
        if k == "mel_loss_32x640x80":
            ln.update(read_bytes=nbytes, kernel_us=kern, tile_kernel_gbs=round(nbytes / (kern["mel_loss_tile"] * 1e-6) * 1e-9, 1))
        lines.append(ln)
    for ln in lines:
        print(json.dumps(ln))
    if args.out:
        with open(args.out, "a") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
