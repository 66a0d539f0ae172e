#!/usr/bin/env python
"""The per-utterance sums of csrc/seq_loss.hip beside the torch composition a user would write without them; one JSON line
per variant.

  guided   ``guided_attention_sums`` on 32 utterances x 4 maps x 640 x 129 (42.3 MB read once) against: materialise the
           (32, 640, 129) guide and its mask from the lengths, multiply under the heads' broadcast, ``masked_select``, mean --
           all on the device.
  pair     ``pair_loss_sums`` on the 32 x 640 x 80 pair (13.1 MB) against ``masked_select`` of both operands under the frame
           mask, then the means of |p - t| and (p - t)^2.
  floor    both engine calls on B = 1 with one row: launches, the table upload and nothing else.

Each figure is the median device-event time of one whole call (20 rounds after 5 warm-ups, the variants alternating so that
drift of the machine hits all of them); the engine's own kernels are split out by the context profiler.

  python tools/bench_am_losses.py [--utts 32] [--maps 4] [--frames 640] [--tokens 129] [--iters 20] [--out FILE]
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
    ap.add_argument("--maps", type=int, default=4)
    ap.add_argument("--frames", type=int, default=640)
    ap.add_argument("--tokens", type=int, default=129)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None, help="append the lines to this file")
    args = ap.parse_args()
    from parakeet_amd import build as pk_build
    from parakeet_amd.losses import guided_attention_sums, pair_loss_sums
    from parakeet_amd.runtime import Context
    ctx = Context.get()
    dev = ctx.device
    B, G, S, T, W, sigma = args.utts, args.maps, args.frames, args.tokens, 80, 0.4
    g = torch.Generator(device="cpu").manual_seed(7)
    att = torch.softmax(torch.randn((B, G, S, T), generator=g), dim=-1).to(dev)
    olens = torch.full((B,), S, dtype=torch.int64, device=dev)
    ilens = torch.full((B,), T, dtype=torch.int64, device=dev)
    rows, cols = [S] * B, [T] * B
    offs = np.arange(B, dtype=np.int64) * (G * S * T)
    pred = torch.randn((B, S, W), generator=g).to(dev)
    target = (pred + 0.1 * torch.randn((B, S, W), generator=g).to(dev)).contiguous()
    lens = [S] * B

    def guided_engine():
        return guided_attention_sums(att, rows, cols, sigma, maps=G, offsets=offs, map_stride=S * T, row_stride=T)

    def guided_torch():
        s = torch.arange(S, device=dev, dtype=torch.float32)[None, :, None] / olens[:, None, None]
        t = torch.arange(T, device=dev, dtype=torch.float32)[None, None, :] / ilens[:, None, None]
        w = 1.0 - torch.exp(-((t - s) ** 2) / (2 * sigma ** 2))
        mask = (torch.arange(S, device=dev)[None, :, None] < olens[:, None, None]) \
            & (torch.arange(T, device=dev)[None, None, :] < ilens[:, None, None])
        losses = w.unsqueeze(1) * att
        return float(torch.mean(losses.masked_select(mask.unsqueeze(1).expand_as(losses))))

    def pair_engine():
        return pair_loss_sums(pred.reshape(-1, W), target.reshape(-1, W), lens)

    def pair_torch():
        mask = (torch.arange(S, device=dev)[None, :] < olens[:, None]).unsqueeze(-1).expand_as(pred)
        p, t = pred.masked_select(mask), target.masked_select(mask)
        return float(torch.mean(torch.abs(p - t))), float(torch.mean((p - t) ** 2))

    one_att, one_row = torch.ones(1, device=dev), torch.zeros((1, W), device=dev)
    fns = {"guided_engine": guided_engine, "guided_torch": guided_torch, "pair_engine": pair_engine, "pair_torch": pair_torch,
           "guided_floor_1x1x1": lambda: guided_attention_sums(one_att, [1], [1], sigma),
           "pair_floor_1x1x80": lambda: pair_loss_sums(one_row, one_row, [1])}
    # the two sides compute the same quantity
    se = guided_engine()
    assert abs(se[:, 0].sum() / (B * G * S * T) - guided_torch()) < 1e-6
    pe, pt = pair_engine(), pair_torch()
    assert abs(pe[:, 0].sum() / (B * S * W) - pt[0]) < 1e-4 * pt[0] and abs(pe[:, 1].sum() / (B * S * W) - pt[1]) < 1e-4 * pt[1]
    for _ in range(5):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    raw = {k: [] for k in fns}
    for _ in range(args.iters):
        for k, fn in fns.items():
            raw[k].append(event_ms(fn))
    ctx.prof_enable(True)
    ctx.prof_reset()
    for _ in range(args.iters):
        guided_engine()
        pair_engine()
    ctx.sync()
    prof = ctx.prof_dump()
    ctx.prof_enable(False)
    kern = {k: round(ms / n * 1e3, 2) for k, (n, ms) in prof.items()}
    nbytes = {"guided": 4.0 * att.numel(), "pair": 8.0 * pred.numel()}
    base = {"utts": B, "maps": G, "frames": S, "tokens": T, "width": W, "device": torch.cuda.get_device_name(0),
            "host": os.uname().nodename, "source_hash": pk_build.source_hash()[:16]}
    lines = []
    for k, v in raw.items():
        us = float(np.median(v)) * 1e3
        ln = dict(base, name=k, us=round(us, 2), raw_us=[round(t * 1e3, 2) for t in v])
        what = k.split("_")[0]
        if "floor" not in k:
            ln.update(read_bytes=nbytes[what], call_gbs=round(nbytes[what] / (us * 1e-6) * 1e-9, 1))
        if k == "guided_engine":
            ln.update(kernel_us={n: kern[n] for n in ("guided_attn_tile", "seq_loss_fold") if n in kern},
                      tile_kernel_gbs=round(nbytes[what] / (kern["guided_attn_tile"] * 1e-6) * 1e-9, 1))
        if k == "pair_engine":
            ln.update(kernel_us={n: kern[n] for n in ("pair_loss_tile", "seq_loss_fold") if n in kern},
                      tile_kernel_gbs=round(nbytes[what] / (kern["pair_loss_tile"] * 1e-6) * 1e-9, 1))
        lines.append(ln)
    for ln in lines:
        print(json.dumps(ln))
    if args.out:
        with open(args.out, "a") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
