#!/usr/bin/env python
"""The Parallel WaveGAN discriminator on the engine (pk_pwgd_run, one fused kernel) beside the same stack as a chain of
torch.nn.functional.conv1d / leaky_relu calls on the same GPU -- the reference's own sequence of ops; one JSON line each.

Workload: 32 utterances x 163 840 samples of seeded noise, the recipes' shape (10 layers, 64 channels, kernel 3, slope 0.2),
dense seeded weights.  Both maths, both output modes (logits and sums / sums only).  Each figure is the median device-event
time of one whole call, 3 warm-ups, >= 10 timed.  FLOP are counted from the shapes, 2 * K * C_out per conv and sample; the
fused kernel also recomputes the halo of every tile, (tile + 2 halo) / tile times the hidden layers' FLOP ("issued").

  python tools/bench_pwg_disc.py [--utts 32] [--samples 163840] [--iters 10] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


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
    ap.add_argument("--utts", type=int, default=32)
    ap.add_argument("--samples", type=int, default=163840)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None, help="append the lines to this file")
    args = ap.parse_args()
    import torch.nn.functional as F
    from parakeet_amd import build as pk_build
    from parakeet_amd import synthetic as syn
    from parakeet_amd.parallel_wavegan import PWGDiscriminator
    B, T = args.utts, args.samples
    cfg = dict(kernel_size=3, layers=10, conv_channels=64, dilation_factor=1, bias=True)
    state = syn.pwg_disc_state(cfg, seed=77)
    disc = PWGDiscriminator(**cfg)
    disc.set_state_dict(state)
    disc.eval()
    tile, halo = disc.tile_samples()
    x = torch.from_numpy((0.5 * np.random.default_rng(5).standard_normal((B, 1, T))).astype(np.float32)).cuda()
    rows = [x[b, 0] for b in range(B)]
    L, C, k = cfg["layers"], cfg["conv_channels"], cfg["kernel_size"]
    hidden = 2.0 * k * C * C * (L - 2)
    flop = (2.0 * k * C + hidden + 2.0 * k * C) * B * T
    issued = (2.0 * k * C + hidden) * B * T * (tile + 2 * halo) / tile + 2.0 * k * C * B * T
    ws = [torch.from_numpy(state[f"conv_layers.{2 * i}.weight"]).cuda() for i in range(L)]
    bs = [torch.from_numpy(state[f"conv_layers.{2 * i}.bias"]).cuda() for i in range(L)]
    dil = disc.dilations

    def chain(terms):
        h = x
        for i in range(L):
            h = F.conv1d(h, ws[i], bs[i], padding=(k - 1) // 2 * dil[i], dilation=dil[i])
            if i < L - 1:
                h = F.leaky_relu(h, 0.2)
        if terms:
            return torch.stack([((h - 1.0) ** 2).sum(dim=(1, 2)), (h ** 2).sum(dim=(1, 2))], 1)
        return h

    lines = []
    base = dict(workload=f"{B} x {T} samples, layers {L}, channels {C}, kernel {k}", tile=tile, halo=halo,
                flop=flop, flop_issued=issued, source_hash=pk_build.file_hash("pwg_disc.hip")[:16])
    with torch.no_grad():
        ref_sums = chain(True).double().cpu().numpy()
        for mode, terms in (("logits+sums", True), ("logits", False)):
            ms, ts = timed(lambda: chain(terms), 3, args.iters)
            lines.append(dict(base, what="torch conv1d / leaky_relu chain", output=mode, ms=round(ms, 3), all_ms=ts,
                              tflops=round(flop / ms * 1e-9, 2)))
    for math in ("f16x3", "f32"):
        disc.set_math(math)
        got, _ = disc.scores(rows)
        rel = float(np.max(np.abs(got - ref_sums) / np.abs(ref_sums)))
        for mode, fn in (("logits+sums", lambda: disc._run(rows, True, True)), ("sums", lambda: disc.scores(rows))):
            ms, ts = timed(fn, 3, args.iters)
            lines.append(dict(base, what="pk_pwgd_run", math=math, output=mode, ms=round(ms, 3), all_ms=ts,
                              tflops=round(flop / ms * 1e-9, 2), tflops_issued=round(issued / ms * 1e-9, 2),
                              sums_rel_diff_to_torch=rel))
    t_ref = next(l["ms"] for l in lines if l["what"].startswith("torch") and l["output"] == "logits+sums")
    for l in lines:
        if l["what"] == "pk_pwgd_run":
            l["torch_over_engine"] = round(t_ref / l["ms"], 3)
    for l in lines:
        print(json.dumps(l), flush=True)
    if args.out:
        with open(args.out, "at") as f:
            for l in lines:
                f.write(json.dumps(l) + "\n")


if __name__ == "__main__":
    main()
