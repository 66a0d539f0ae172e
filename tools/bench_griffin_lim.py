#!/usr/bin/env python
"""Griffin-Lim on the engine (pk_gl_run) beside the same loop written with torch.stft / torch.istft (rocFFT), and one
pk_istft_run of the batch against its byte minimum; one JSON line each.

Workload: 32 utterances x 640 frames, n_fft 1024, hop 256, hann, center, 32 iterations, momentum 0.99, magnitudes of seeded
noise-plus-sines signals, the same initial phases on both sides.  Each figure is the median device-event time of one whole
call, 5 warm-ups, >= 20 timed.  The dense-DFT formulation costs 2 * n_fft * (n_fft + 2) FLOP per frame and direction (an FFT
is O(n log n)); the FLOP and byte counts below are computed from the shapes.

``--transform fft`` runs the engine's calls on the radix FFT (csrc/rfft.hip) instead of the dense products; its lines carry
no FLOP figure (the dense count does not apply) and the inverse moves no K-padded copy.  Run the two alternately in one
session to compare them.

  python tools/bench_griffin_lim.py [--utts 32] [--frames 640] [--iters 20] [--transform {dense,fft}] [--out FILE]
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


def torch_griffin_lim(S, angles, n_fft, hop, win, n_iter, momentum):
    """librosa.griffinlim with torch.stft / torch.istft: S, angles (B, n_bin, frames)."""
    def inv(X):
        return torch.istft(X, n_fft, hop_length=hop, win_length=n_fft, window=win, center=True)

    rebuilt = torch.zeros_like(angles)
    c = momentum / (1.0 + momentum)
    for _ in range(n_iter):
        prev = rebuilt
        rebuilt = torch.stft(inv(S * angles), n_fft, hop_length=hop, win_length=n_fft, window=win, center=True,
                             pad_mode="reflect", return_complex=True)
        angles = rebuilt - c * prev
        angles = angles / (angles.abs() + 1e-16)
    return inv(S * angles)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=32)
    ap.add_argument("--frames", type=int, default=640)
    ap.add_argument("--n-fft", type=int, default=1024)
    ap.add_argument("--hop", type=int, default=256)
    ap.add_argument("--n-iter", type=int, default=32)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--transform", choices=("dense", "fft"), default="dense")
    ap.add_argument("--out", default=None, help="append the lines to this file")
    args = ap.parse_args()
    from parakeet_amd import build as pk_build
    from parakeet_amd.audio import _Engine, _InvEngine
    N, hop, B, F = args.n_fft, args.hop, args.utts, args.frames
    nb = 1 + N // 2
    fwd = _Engine(N, hop, N, "hann", True, False, None, 0, transform=args.transform)
    inv = _InvEngine(N, hop, N, "hann", True, transform=args.transform)
    dense = args.transform == "dense"
    rng = np.random.default_rng(3)
    t = np.arange(hop * (F - 1), dtype=np.float64)
    wavs = [(0.3 * np.sin(2 * np.pi * (0.01 + 0.001 * b) * t) + 0.05 * rng.standard_normal(t.size)).astype(np.float32)
            for b in range(B)]
    mags = fwd.run(wavs, 1)                                               # (frames, n_bin) each, device
    ph = torch.from_numpy(rng.random((B, F, nb)).astype(np.float32)).cuda() * (2 * np.pi)
    ang = [torch.cat([torch.cos(p), torch.sin(p)], 1).contiguous() for p in ph]
    spec = fwd.run(wavs, 0)
    base = {"utts": B, "frames": F, "n_fft": N, "hop": hop, "n_iter": args.n_iter, "momentum": 0.99, "transform": args.transform,
            "device": torch.cuda.get_device_name(0), "host": os.uname().nodename, "source_hash": pk_build.source_hash()[:16]}
    rows = B * F
    flop_dir = 2.0 * N * (N + 2) * rows                                   # one dense transform of the batch
    lines = []

    ms, raw = timed(lambda: inv.griffin_lim(fwd, mags, args.n_iter, 0.99, None, ang), 5, args.iters)
    flop = flop_dir * (2 * args.n_iter + 1)
    lines.append(dict(base, name="engine_griffin_lim", ms=round(ms, 3), raw_ms=raw,
                      **(dict(flop=flop, tflops=round(flop / ms * 1e-9, 2)) if dense else {})))

    win = torch.hann_window(N, periodic=True, device="cuda")
    S = torch.stack([m.transpose(0, 1) for m in mags])
    A0 = torch.polar(torch.ones_like(ph), ph).transpose(1, 2).contiguous()
    ms, raw = timed(lambda: torch_griffin_lim(S, A0, N, hop, win, args.n_iter, 0.99), 5, args.iters)
    lines.append(dict(base, name="torch_stft_istft_griffin_lim", ms=round(ms, 3), raw_ms=raw))

    # one inverse of the batch; byte minimum: read spec, write and read the frame buffer, write wav
    ms, raw = timed(lambda: inv.run(spec), 5, args.iters)
    min_bytes = 4.0 * (rows * 2 * nb + 2 * rows * N + B * hop * (F - 1))
    moved = min_bytes + (4.0 * 2 * rows * (N + 16) if dense else 0.0)    # + the K-padded copy of spec: written, read
    lines.append(dict(base, name="engine_istft", ms=round(ms, 3), raw_ms=raw,
                      **(dict(flop=flop_dir, tflops=round(flop_dir / ms * 1e-9, 2)) if dense else {}),
                      min_bytes=min_bytes, moved_bytes=moved, min_bytes_gbs=round(min_bytes / ms * 1e-6, 1)))
    Xc = torch.stack([torch.complex(s[:, :nb], s[:, nb:]).transpose(0, 1) for s in spec])
    ms, raw = timed(lambda: torch.istft(Xc, N, hop_length=hop, win_length=N, window=win, center=True), 5, args.iters)
    lines.append(dict(base, name="torch_istft", ms=round(ms, 3), raw_ms=raw))

    # the two loops agree in what they reach (trajectories differ in the last bits; compare spectral convergence)
    y_e = torch.stack(inv.griffin_lim(fwd, mags, args.n_iter, 0.99, None, ang))
    y_t = torch_griffin_lim(S, A0, N, hop, win, args.n_iter, 0.99)

    def conv(y):
        m = torch.stft(y, N, hop_length=hop, win_length=N, window=win, center=True, pad_mode="reflect",
                       return_complex=True).abs()
        return float(torch.linalg.norm(m - S) / torch.linalg.norm(S))

    lines.append(dict(base, name="spectral_convergence", engine=round(conv(y_e), 4), torch=round(conv(y_t), 4)))
    for ln in lines:
        print(json.dumps(ln))
    if args.out:
        with open(args.out, "a") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
