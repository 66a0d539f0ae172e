#!/usr/bin/env python
"""The HiFi-GAN generator on the engine (pk_hfg_infer, csrc/hifigan.hip) beside the same stack as a chain of
torch.nn.functional.conv1d / conv_transpose1d / leaky_relu calls in fp32 on the same GPU; one JSON line each.

Workloads: HiFi-GAN V1 (channels 512, scales 8 8 2 2, hop 256) and the hop-300 variant (scales 5 5 4 3) at channels 512,
32 utterances x 640 frames of seeded mel, dense seeded weights (synthetic.hifigan_state).  Both maths.  Each figure is the
median device-event time of one whole call after the warm-ups.  FLOP are counted from the shapes: 2 * k * C_in * C_out per
output position of a convolution, 2 * 2 * C_in * C_out per output position of a transposed one (two taps reach an output).

  python tools/bench_hifigan.py [--utts 32] [--frames 640] [--iters 10] [--warmup 3] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FP16_MFMA_PEAK, FP32_MFMA_PEAK = 2.5e15, 157.3e12
PWG_MS_SAME_AUDIO = 40.2                             # README: Parallel WaveGAN, 32 x 640 frames at hop 256 (context only)


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


def flop_per_frame(cfg):
    """FLOP of one mel frame through the stack, from the shapes."""
    ch, k = cfg["channels"], cfg["kernel_size"]
    f = 2.0 * k * cfg["in_channels"] * ch
    rate = 1
    for i, s in enumerate(cfg["upsample_scales"]):
        cin, c = ch >> i, ch >> (i + 1)
        rate *= s
        f += 2.0 * 2 * cin * c * rate
        for kj, ds in zip(cfg["resblock_kernel_sizes"], cfg["resblock_dilations"]):
            f += 2.0 * kj * c * c * rate * len(ds) * (2 if cfg["use_additional_convs"] else 1)
    return f + 2.0 * k * (ch >> len(cfg["upsample_scales"])) * rate


def torch_chain(cfg, state):
    import torch.nn.functional as F
    W = {k_: torch.from_numpy(v).cuda() for k_, v in state.items()}
    k, slope, nb = cfg["kernel_size"], cfg["nonlinear_activation_params"]["negative_slope"], len(cfg["resblock_kernel_sizes"])

    def run(c):   # (B, C_in, T')
        x = F.conv1d(c, W["input_conv.weight"], W["input_conv.bias"], padding=(k - 1) // 2)
        for i, s in enumerate(cfg["upsample_scales"]):
            x = F.conv_transpose1d(F.leaky_relu(x, slope), W[f"upsamples.{i}.1.weight"], W[f"upsamples.{i}.1.bias"], stride=s,
                                   padding=s // 2 + s % 2, output_padding=s % 2)
            tot = None
            for j, (kj, ds) in enumerate(zip(cfg["resblock_kernel_sizes"], cfg["resblock_dilations"])):
                y = x
                for n, d in enumerate(ds):
                    p = f"blocks.{i * nb + j}"
                    t = F.conv1d(F.leaky_relu(y, slope), W[f"{p}.convs1.{n}.1.weight"], W[f"{p}.convs1.{n}.1.bias"],
                                 padding=(kj - 1) // 2 * d, dilation=d)
                    if cfg["use_additional_convs"]:
                        t = F.conv1d(F.leaky_relu(t, slope), W[f"{p}.convs2.{n}.1.weight"], W[f"{p}.convs2.{n}.1.bias"],
                                     padding=(kj - 1) // 2)
                    y = t + y
                tot = y if tot is None else tot + y
            x = tot / nb
        return torch.tanh(F.conv1d(F.leaky_relu(x, 0.01), W["output_conv.1.weight"], W["output_conv.1.bias"], padding=(k - 1) // 2))
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=32)
    ap.add_argument("--frames", type=int, default=640)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="append the lines to this file")
    args = ap.parse_args()
    from parakeet_amd import build as pk_build
    from parakeet_amd import synthetic as syn
    from parakeet_amd.hifigan import HiFiGANGenerator
    B, T = args.utts, args.frames
    lines = []
    for name, scales in (("V1", (8, 8, 2, 2)), ("CS512", (5, 5, 4, 3))):
        cfg = dict(syn.HIFIGAN_V1, upsample_scales=scales, upsample_kernel_sizes=tuple(2 * s for s in scales))
        state = syn.hifigan_state(cfg, seed=31)
        hop = int(np.prod(scales))
        mel = torch.from_numpy(np.random.default_rng(7).standard_normal((B * T, 80)).astype(np.float32)).cuda()
        flop = flop_per_frame(cfg) * B * T
        base = dict(workload=f"{name}: {B} x {T} frames, hop {hop}, channels 512", samples=B * T * hop, flop=flop,
                    source_hash=pk_build.file_hash("hifigan.hip")[:16])
        chain = torch_chain(cfg, state)
        c = mel.reshape(B, T, 80).transpose(1, 2).contiguous()
        with torch.no_grad():
            ref = chain(c).reshape(-1)
            t_ref, ts = timed(lambda: chain(c), args.warmup, args.iters)
        lines.append(dict(base, what="torch.nn.functional chain, fp32", ms=round(t_ref, 3), all_ms=ts,
                          tflops=round(flop / t_ref * 1e-9, 2)))
        g = HiFiGANGenerator(**cfg)
        g.set_state_dict(state)
        g.eval()
        frames = [T] * B
        for math in ("f16x3", "f32"):
            g.set_math(math)
            wav = g.infer_packed(mel, frames)
            rel = float((wav - ref).abs().max() / ref.abs().max())
            ms, ts = timed(lambda: g.infer_packed(mel, frames), args.warmup, args.iters)
            peak = FP16_MFMA_PEAK if math == "f16x3" else FP32_MFMA_PEAK
            products = 3.0 if math == "f16x3" else 1.0
            lines.append(dict(base, what="pk_hfg_infer", math=math, ms=round(ms, 3), all_ms=ts, tflops=round(flop / ms * 1e-9, 2),
                              matrix_pipe_fraction=round(products * flop / (ms * 1e-3) / peak, 4), torch_over_engine=round(t_ref / ms, 3),
                              msamples_per_s=round(B * T * hop / ms * 1e-3, 2), wav_rel_diff_to_torch_fp32=rel,
                              pwg_ms_same_audio=PWG_MS_SAME_AUDIO if hop == 256 else None))
        del g, chain, ref
        torch.cuda.empty_cache()
    for l in lines:
        print(json.dumps(l), flush=True)
    if args.out:
        with open(args.out, "at") as f:
            for l in lines:
                f.write(json.dumps(l) + "\n")


if __name__ == "__main__":
    main()
