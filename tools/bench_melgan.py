#!/usr/bin/env python
"""The MelGAN and multi-band MelGAN generators on the engine (pk_mgan_infer, csrc/melgan.hip, csrc/pqmf.hip) beside the same
stack as a chain of torch.nn.functional pad(reflect) / conv1d / conv_transpose1d / leaky_relu calls in fp32 on the same GPU;
one JSON line each.

Workloads, 32 utterances x 640 frames of seeded mel each, dense seeded weights (synthetic.melgan_state), hop 256:
  MelGAN             channels 512, scales 8 8 2 2, 3 stacks
  multi-band MelGAN  channels 384, scales 8 4 2, 4 stacks, 4 sub-bands merged by the PQMF bank (62 taps); the torch side
                     synthesises with conv_transpose1d of the engine's own synthesis filters
Both maths.  Each figure is the median device-event time of one whole call after the warm-ups; all repeats are kept.  FLOP
are counted from the shapes: 2 * k * C_in * C_out per output position of a convolution, 2 * 2 * C_in * C_out per output
position of a transposed one (two taps reach an output), 2 * (taps + 1) per sample of the bank.

  python tools/bench_melgan.py [--utts 32] [--frames 640] [--iters 10] [--warmup 3] [--out profiles/melgan_bench.jsonl]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FP16_MFMA_PEAK, FP32_MFMA_PEAK = 2.5e15, 157.3e12
PWG_MS_SAME_AUDIO = 40.2                             # README: Parallel WaveGAN, 32 x 640 frames at hop 256 (context only)
HIFIGAN_V1_MS_SAME_AUDIO = {"f16x3": 116.3, "f32": 188.2}   # profiles/hifigan_bench.jsonl (context only)


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


def flop_per_frame(cfg, taps=None):
    """FLOP of one mel frame through the stack (and the bank), from the shapes."""
    ch, k, S, sk = cfg["channels"], cfg["kernel_size"], cfg["stacks"], cfg["stack_kernel_size"]
    f = 2.0 * k * cfg["in_channels"] * ch
    rate = 1
    for i, s in enumerate(cfg["upsample_scales"]):
        cin, c = ch >> i, ch >> (i + 1)
        rate *= s
        f += 2.0 * 2 * cin * c * rate + S * 2.0 * (sk + 2) * c * c * rate
    f += 2.0 * k * (ch >> len(cfg["upsample_scales"])) * cfg["out_channels"] * rate
    if taps is not None:
        f += 2.0 * (taps + 1) * rate * cfg["out_channels"]
    return f


def torch_chain(cfg, state, syn_filter=None):
    import torch.nn.functional as F
    W = {k_: torch.from_numpy(v).cuda() for k_, v in state.items()}
    k, sk, S = cfg["kernel_size"], cfg["stack_kernel_size"], cfg["stacks"]
    slope, n = cfg["nonlinear_activation_params"]["negative_slope"], len(cfg["upsample_scales"])
    K = cfg["out_channels"]
    if syn_filter is not None:   # zeros inserted, scaled by K, correlated: conv_transpose1d of the flipped filters, cropped
        taps = syn_filter.shape[1] - 1
        wt = (K * torch.from_numpy(syn_filter[:, ::-1].copy())).cuda()[:, None, :]          # (K, 1, taps + 1)

    def conv(x, name, pad=0, d=1):
        if pad:
            x = F.pad(x, (pad, pad), mode="reflect")
        return F.conv1d(x, W[name + ".weight"], W[name + ".bias"], dilation=d)

    def run(c):   # (B, C_in, T')
        x = conv(c, "melgan.1", (k - 1) // 2)
        for i, s in enumerate(cfg["upsample_scales"]):
            q = 2 + i * (2 + S)
            x = F.conv_transpose1d(F.leaky_relu(x, slope), W[f"melgan.{q + 1}.weight"], W[f"melgan.{q + 1}.bias"], stride=s,
                                   padding=s // 2 + s % 2, output_padding=s % 2)
            for j in range(S):
                p, d = f"melgan.{q + 2 + j}", sk ** j
                t = conv(F.leaky_relu(x, slope), p + ".stack.2", (sk - 1) // 2 * d, d)
                x = conv(F.leaky_relu(t, slope), p + ".stack.4") + conv(x, p + ".skip_layer")
        y = torch.tanh(conv(F.leaky_relu(x, slope), f"melgan.{2 + n * (2 + S) + 2}", (k - 1) // 2))
        if syn_filter is None:
            return y
        full = F.conv_transpose1d(y, wt, stride=K)                                          # (B, 1, (M - 1) K + taps + 1)
        return full[:, :, taps // 2:taps // 2 + y.shape[2] * K]
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
    from parakeet_amd.melgan import PQMF, MelGANGenerator
    B, T = args.utts, args.frames
    lines = []
    for name, cfg in (("MelGAN", syn.MELGAN), ("multi-band MelGAN", syn.MB_MELGAN)):
        state = syn.melgan_state(cfg, seed=31)
        q = PQMF() if cfg["out_channels"] > 1 else None
        hop = int(np.prod(cfg["upsample_scales"])) * cfg["out_channels"]
        mel = torch.from_numpy(np.random.default_rng(7).standard_normal((B * T, 80)).astype(np.float32)).cuda()
        flop = flop_per_frame(cfg, q.taps if q else None) * B * T
        base = dict(workload=f"{name}: {B} x {T} frames, hop {hop}, channels {cfg['channels']}", samples=B * T * hop, flop=flop,
                    source_hash=pk_build.file_hash("melgan.hip")[:16], conv_hash=pk_build.file_hash("pk_hfg_conv.h")[:16])
        chain = torch_chain(cfg, state, q.filters()[1] if q else None)
        c = mel.reshape(B, T, 80).transpose(1, 2).contiguous()
        with torch.no_grad():
            ref = chain(c).reshape(-1)
            t_ref, ts = timed(lambda: chain(c), args.warmup, args.iters)
        lines.append(dict(base, what="torch.nn.functional chain, fp32", ms=round(t_ref, 3), all_ms=ts,
                          tflops=round(flop / t_ref * 1e-9, 2)))
        g = MelGANGenerator(**cfg)
        g.set_state_dict(state)
        g.set_pqmf(q)
        g.eval()
        frames = [T] * B
        for math in ("f16x3", "f32"):
            g.set_math(math)
            wav = g.infer_packed(mel, frames)
            assert wav.shape == ref.shape
            rel = float((wav - ref).abs().max() / ref.abs().max())
            ms, ts = timed(lambda: g.infer_packed(mel, frames), args.warmup, args.iters)
            peak = FP16_MFMA_PEAK if math == "f16x3" else FP32_MFMA_PEAK
            products = 3.0 if math == "f16x3" else 1.0
            lines.append(dict(base, what="pk_mgan_infer", math=math, ms=round(ms, 3), all_ms=ts, tflops=round(flop / ms * 1e-9, 2),
                              matrix_pipe_fraction=round(products * flop / (ms * 1e-3) / peak, 4), torch_over_engine=round(t_ref / ms, 3),
                              msamples_per_s=round(B * T * hop / ms * 1e-3, 2), wav_rel_diff_to_torch_fp32=rel,
                              pwg_ms_same_audio=PWG_MS_SAME_AUDIO, hifigan_v1_ms_same_audio=HIFIGAN_V1_MS_SAME_AUDIO[math]))
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
