#!/usr/bin/env python
"""The engine's resampler (pk_resample_run, csrc/resample.hip) beside scipy.signal.resample_poly on the host, the package's
only resampler before it (ge2e_audio.resample); one JSON line each.

Workload: 32 utterances x 7.43 s of seeded noise at 48 kHz -> 22.05 kHz (up 147, down 320), kaiser_best.  The engine figures
are the median device-event time of one whole call, 3 warm-ups, >= 10 timed: ``pk_resample_run`` on buffers that are already on
the device, and ``Resample.run_batch`` from host arrays (upload and packing included).  The host figure is the wall time of
``ge2e_audio.resample`` over the same 32 signals, one after the other and on a pool of --cpus processes.

Coefficient traffic: a work item loads T coefficients for its R outputs, 4 T / R bytes per output from the table (which stays
in L2), against the 8 bytes of input and output an output costs.

  python tools/bench_resample.py [--utts 32] [--seconds 7.43] [--iters 10] [--cpus 16] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

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


def _host_one(args):
    from parakeet_amd.ge2e_audio import resample
    x, a, b = args
    return resample(x, a, b).size


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=7.43)
    ap.add_argument("--orig-sr", type=int, default=48000)
    ap.add_argument("--target-sr", type=int, default=22050)
    ap.add_argument("--res-type", default="kaiser_best")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--cpus", type=int, default=16)
    ap.add_argument("--out", default=None, help="append the lines to this file")
    args = ap.parse_args()
    from parakeet_amd import _capi, build as pk_build
    from parakeet_amd.audio import Resample
    from parakeet_amd.runtime import dptr
    B, N = args.utts, int(round(args.seconds * args.orig_sr))
    rng = np.random.default_rng(5)
    xs = [(0.5 * rng.standard_normal(N)).astype(np.float32) for _ in range(B)]
    rs = Resample(args.orig_sr, args.target_sr, res_type=args.res_type)
    n_out = rs.output_length(N)
    tile, T = rs.tile_samples, rs.taps
    ctx = rs.ctx
    x = ctx.to_device(np.concatenate(xs))
    out = ctx.empty((B * n_out,))
    lens = np.full(B, N, dtype=np.int32)

    def run_device():
        _capi.check(ctx.lib.pk_resample_run(rs.h, dptr(x), lens.ctypes.data_as(C.POINTER(C.c_int32)), B, dptr(out), 0))

    base = dict(workload=f"{B} x {N} samples, {args.orig_sr} -> {args.target_sr} Hz, {args.res_type}", up=rs.up, down=rs.down,
                taps=T, tile=tile, outputs=B * n_out, source_hash=pk_build.file_hash("resample.hip")[:16])
    lines = []
    ms, ts = timed(run_device, 3, args.iters)
    fma = float(B) * n_out * T
    lines.append(dict(base, what="pk_resample_run, device buffers", ms=round(ms, 4), all_ms=ts,
                      gfma_per_s=round(fma / ms * 1e-6, 1), io_gb_per_s=round((B * N + B * n_out) * 4 / ms * 1e-6, 1)))
    ctx.prof_enable(True)
    ctx.prof_reset()
    for _ in range(args.iters):
        run_device()
    n, tot = ctx.prof_dump()["resample"]
    ctx.prof_enable(False)
    lines.append(dict(base, what="k_resample alone (the engine's per-kernel events)", launches=n, ms=round(tot / n, 4),
                      gfma_per_s=round(fma / (tot / n) * 1e-6, 1)))
    ms, ts = timed(lambda: rs.run_batch(xs), 3, args.iters)
    lines.append(dict(base, what="Resample.run_batch, host arrays", ms=round(ms, 3), all_ms=ts))
    t0 = time.perf_counter()
    for v in xs:
        _host_one((v, args.orig_sr, args.target_sr))
    lines.append(dict(base, what="ge2e_audio.resample (scipy), one process", ms=round((time.perf_counter() - t0) * 1e3, 1)))
    import multiprocessing as mp
    with mp.get_context("spawn").Pool(args.cpus) as pool:
        pool.map(_host_one, [(v[:100], args.orig_sr, args.target_sr) for v in xs[:args.cpus]])      # start the workers
        t0 = time.perf_counter()
        pool.map(_host_one, [(v, args.orig_sr, args.target_sr) for v in xs], chunksize=1)
        lines.append(dict(base, what=f"ge2e_audio.resample (scipy), {args.cpus} processes",
                          ms=round((time.perf_counter() - t0) * 1e3, 1)))
    for l in lines:
        print(json.dumps(l), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "at") as f:
            for l in lines:
                f.write(json.dumps(l) + "\n")


if __name__ == "__main__":
    main()
