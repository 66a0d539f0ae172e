#!/usr/bin/env python
"""Multi-resolution STFT distance on the engine (pk_stftd_run) beside (a) the same loss written with torch.stft (rocFFT)
and (b), for the two hop-aligned resolutions, the composition the engine offered before: parakeet_amd.audio.stft on each
signal plus torch reductions; one JSON line each.

Workload: 32 pairs x 163 840 samples of seeded noise-plus-tone signals at the reference's resolutions 1024 / 120 / 600,
2048 / 240 / 1200, 512 / 50 / 240.  Each figure is the median device-event time of one whole call, 3 warm-ups, >= 10 timed.
The dense-DFT formulation costs 2 * n_fft * (n_fft + 2) FLOP per frame; FLOP and byte counts are computed from the shapes.
The reduction reads 2 signals x frames x (n_fft + 4) floats of re, im per resolution and writes 3 floats per frame.

  python tools/bench_stft_loss.py [--utts 32] [--samples 163840] [--iters 10] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

RES = [(1024, 120, 600), (2048, 240, 1200), (512, 50, 240)]


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


def torch_sums(x, y, res, wins):
    """(B, T) each -> (R, 3) sums over the batch with torch.stft."""
    out = []
    for (n, hop, wl), w in zip(res, wins):
        def mag(v):
            z = torch.stft(v, n, hop_length=hop, win_length=wl, window=w, center=True, pad_mode="reflect",
                           return_complex=True)
            return torch.sqrt(torch.clamp_min(z.real ** 2 + z.imag ** 2, 1e-7))
        X, Y = mag(x), mag(y)
        out.append(torch.stack([((Y - X) ** 2).sum(), (Y ** 2).sum(), (torch.log(Y) - torch.log(X)).abs().sum()]))
    return torch.stack(out)


def composed_sums(stfts, x, y):
    """The route of parakeet_amd.audio.stft (hop % 4 == 0 only; its STFT objects built once) plus torch reductions."""
    out = []
    floor = float(np.sqrt(np.float32(1e-7)))
    for t in stfts:
        X = torch.clamp_min(t.magnitude(x).as_subclass(torch.Tensor), floor)
        Y = torch.clamp_min(t.magnitude(y).as_subclass(torch.Tensor), floor)
        out.append(torch.stack([((Y - X) ** 2).sum(), (Y ** 2).sum(), (torch.log(Y) - torch.log(X)).abs().sum()]))
    return torch.stack(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=32)
    ap.add_argument("--samples", type=int, default=163840)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--only", default=None, help="engine: time pk_stftd_run alone (for a kernel trace)")
    ap.add_argument("--out", default=None, help="append the lines to this file")
    args = ap.parse_args()
    from parakeet_amd import audio
    from parakeet_amd import build as pk_build
    from parakeet_amd.stft_loss import _DistEngine, losses_from_sums
    B, T = args.utts, args.samples
    rng = np.random.default_rng(5)
    t = np.arange(T, dtype=np.float64)
    y = np.stack([0.3 * np.sin(2 * np.pi * (0.01 + 0.001 * b) * t) + 0.05 * rng.standard_normal(T) for b in range(B)])
    x = y + 0.02 * rng.standard_normal(y.shape)
    x, y = torch.from_numpy(x.astype(np.float32)).cuda(), torch.from_numpy(y.astype(np.float32)).cuda()
    xs, ys = [x[b] for b in range(B)], [y[b] for b in range(B)]
    base = {"utts": B, "samples": T, "resolutions": RES, "device": torch.cuda.get_device_name(0),
            "host": os.uname().nodename, "source_hash": pk_build.source_hash()[:16]}
    frames = [1 + T // hop for _, hop, _ in RES]
    flop = sum(2.0 * n * (n + 2) * f * 2 * B for (n, _, _), f in zip(RES, frames))
    red_bytes = sum(4.0 * (2 * B * f * (n + 4) + 3 * B * f) for (n, _, _), f in zip(RES, frames))
    lines = []

    eng = _DistEngine([r[0] for r in RES], [r[1] for r in RES], [r[2] for r in RES])
    ms, raw = timed(lambda: eng.sums(xs, ys), 3, args.iters)
    lines.append(dict(base, name="engine_stftd_run", ms=round(ms, 3), raw_ms=raw, flop=flop, tflops=round(flop / ms * 1e-9, 2),
                      reduce_bytes=red_bytes))
    ctx = eng.ctx
    ctx.prof_enable(True)
    ctx.prof_reset()
    eng.sums(xs, ys)
    ctx.sync()
    prof = ctx.prof_dump()
    ctx.prof_enable(False)
    split = {k: round(v[1], 3) for k, v in prof.items() if k.startswith("stftd_")}
    lines.append(dict(base, name="engine_kernel_split_ms", **split,
                      reduce_gbs=round(red_bytes / max(split.get("stftd_reduce", 0.0), 1e-9) * 1e-6, 1)))
    if args.only != "engine":
        wins = [torch.hann_window(wl, periodic=True, device="cuda") for _, _, wl in RES]
        ms, raw = timed(lambda: torch_sums(x, y, RES, wins).cpu(), 3, args.iters)
        lines.append(dict(base, name="torch_stft_loss", ms=round(ms, 3), raw_ms=raw))
        # the two hop-aligned resolutions: the new path against the old composition
        eng2 = _DistEngine([r[0] for r in RES[:2]], [r[1] for r in RES[:2]], [r[2] for r in RES[:2]])
        ms, raw = timed(lambda: eng2.sums(xs, ys), 3, args.iters)
        lines.append(dict(base, name="engine_stftd_run_aligned_two", ms=round(ms, 3), raw_ms=raw))
        stfts = [audio.STFT(n, hop, wl, "hann", True, "reflect") for n, hop, wl in RES[:2]]
        ms, raw = timed(lambda: composed_sums(stfts, x, y).cpu(), 2, max(3, args.iters // 2))
        lines.append(dict(base, name="composed_audio_stft_aligned_two", ms=round(ms, 3), raw_ms=raw))
        # the three routes say the same
        e = eng.sums(xs, ys).sum(0)
        tq = torch_sums(x, y, RES, wins).double().cpu().numpy()
        n = np.array([B * f * (1 + r[0] // 2) for r, f in zip(RES, frames)], np.float64)
        le, lt = losses_from_sums(e, n), losses_from_sums(tq, n)
        lines.append(dict(base, name="losses", engine=[float(le[0].mean()), float(le[1].mean())],
                          torch=[float(lt[0].mean()), float(lt[1].mean())]))
    for ln in lines:
        print(json.dumps(ln))
    if args.out:
        with open(args.out, "a") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
