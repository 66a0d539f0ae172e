#!/usr/bin/env python
"""Parallel WaveGAN throughput at several generator shapes, one JSON line per shape.

Workload: 32 utterances x 640 frames (seeded synthetic weights, mels and noise) through PWGGenerator.infer_packed at the
default math (f16x3), for the tuned default shape, the default shape on the shape-generic kernels (option
"generic_kernel"), and configurations A (32/64/32), B (128/256/128) and C (64/128/64, aux 64, kernel 5, hop 300) of
tests/golden/pwg_sizes.npz.  Reports the median device-event time of one call (2 warm-ups, >= 5 timed), M samples/s,
the mean time per residual-block launch from the engine profiler, and roofline.frac of the generic layer kernel: its
minimum HBM traffic per sample and layer (x read + x written + skip read + skip written, fp32: 4 (2 R + 2 SK) bytes,
1 024 B at 64 / 64) over the launch time, against the 8 TB/s peak.

  python tools/bench_pwg_sizes.py [--utts 32] [--frames 640] [--iters 5]
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
from parakeet_amd.parallel_wavegan import PWGGenerator  # noqa: E402
from parakeet_amd.runtime import Context  # noqa: E402

HBM_PEAK = 8.0e12


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


def run(label, cfg, generic, args):
    ctx = Context.get()
    gen = PWGGenerator(**cfg)
    gen.set_state_dict(syn.pwg_state(cfg, seed=5))
    gen.eval()
    if generic:
        gen.set_option("generic_kernel", 1)
    hop = gen.upsample_factor
    frames = np.full(args.utts, args.frames, np.int32)
    samples = int(frames.sum()) * hop
    g = torch.Generator(device="cuda").manual_seed(1)
    mel = torch.randn(int(frames.sum()), cfg["aux_channels"], device="cuda", generator=g)
    noise = torch.randn(samples, device="cuda", generator=g)
    fn = lambda: gen.infer_packed(mel, frames, noise=noise)  # noqa: E731
    ms = timed(fn, 2, args.iters)
    ctx.prof_enable(True)
    ctx.prof_reset()
    fn()
    ctx.sync()
    prof = ctx.prof_dump()
    ctx.prof_enable(False)
    name = "pwg_block_gen" if generic else "pwg_layer_h3"
    n, t = prof.get(name, (0, 0.0))
    per_launch = t / max(n, 1)
    R, SK = cfg["residual_channels"], cfg["skip_channels"]
    bytes_layer = 4 * (2 * R + 2 * SK) * samples
    out = {"shape": label, "generic": bool(generic), "channels": [R, cfg["gate_channels"], SK],
           "aux": cfg["aux_channels"], "kernel_size": cfg["kernel_size"], "layers": cfg["layers"], "hop": hop,
           "samples": samples, "ms": round(ms, 3), "msamples_per_s": round(samples / ms / 1e3, 2),
           "layer_kernel": name, "layer_launches": n, "ms_per_layer_launch": round(per_launch, 4),
           "layer_share": round(t / ms, 3) if ms else None,
           "roofline": {"bytes_per_sample_layer": 4 * (2 * R + 2 * SK),
                        "frac": round(bytes_layer / (per_launch * 1e-3) / HBM_PEAK, 3) if per_launch else None}}
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=32)
    ap.add_argument("--frames", type=int, default=640)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    args = ap.parse_args()
    lines = [run("default", dict(syn.PWG_LJSPEECH), False, args),
             run("default", dict(syn.PWG_LJSPEECH), True, args)]
    for name in ("A", "B", "C"):
        lines.append(run(name, syn.pwg_size_config(name), True, args))
    if args.out:
        with open(args.out, "w") as f:
            f.write("".join(json.dumps(x) + "\n" for x in lines))


if __name__ == "__main__":
    main()
