#!/usr/bin/env python
"""STOI and ESTOI of 32 pairs of 7.43 s at 10 kHz (74 300 samples each, the harmonic test signal of tests/stoi_ref.py plus
noise at 5 dB; seeded), device-resident: ``pk_stoi_run`` timed by hipEvent (``torch.cuda.Event``) around the call, which uploads
its table of B entries and enqueues seven launches; the median and the minimum over ``--steps`` calls after ``--warmup``, and
from the engine's profiler the share of every launch.  Beside it, the float64 numpy restatement on the host for ONE pair.
Information only: no roofline fraction is given (the stages are small and launch-bound at this size).  Prints one JSON line and
appends it to profiles/stoi_bench.jsonl (or ``--out``)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--samples", type=int, default=74300)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stoi_bench.jsonl"))
    ap.add_argument("--no-record", action="store_true", help="do not append to the record file")
    args = ap.parse_args(argv)
    import ctypes as C
    import torch
    import stoi_ref as sr
    from parakeet_amd import metrics
    from parakeet_amd.runtime import Context, dptr
    ctx = Context.get()
    B, L = args.batch, args.samples
    xs = [sr.harmonic(L, b) for b in range(B)]
    ys = [sr.add_noise(x, 5, b) for b, x in enumerate(xs)]
    x, y = ctx.to_device(np.concatenate(xs)), ctx.to_device(np.concatenate(ys))
    offs = (np.arange(B + 1, dtype=np.int64) * L)
    res = torch.empty((B * 24,), dtype=torch.uint8, device=ctx.device)

    def run(ext):
        rc = ctx.lib.pk_stoi_run(ctx.handle, dptr(x), dptr(y), offs.ctypes.data_as(C.POINTER(C.c_int64)), B, ext, dptr(res))
        assert rc == 0, ctx.lib.pk_last_error()

    def timed(ext):
        for _ in range(args.warmup):
            run(ext)
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(ext)
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return float(np.median(ms)), float(np.min(ms))

    t0 = time.perf_counter()
    want = [sr.stoi(xs[0], ys[0], ext)["d"] for ext in (False, True)]
    ref_ms = (time.perf_counter() - t0) * 1e3 / 2
    got = [metrics.stoi_batch(xs[:1], ys[:1], sr.FS, ext)[0] for ext in (False, True)]
    assert max(abs(a - b) for a, b in zip(got, want)) < 1e-5, (got, want)
    t_s, t_e = timed(0), timed(1)
    ctx.prof_enable(True)
    ctx.prof_reset()
    run(1)
    ctx.sync()
    launches = {k: round(v[1], 4) for k, v in ctx.prof_dump().items() if k.startswith("stoi_")}
    ctx.prof_enable(False)
    rec = dict(shape=f"{B}x{L}", seconds_of_audio=round(B * L / sr.FS, 1), steps=args.steps,
               stoi_call_ms=round(t_s[0], 4), stoi_call_min_ms=round(t_s[1], 4), estoi_call_ms=round(t_e[0], 4),
               estoi_call_min_ms=round(t_e[1], 4), estoi_launch_ms=launches, numpy_one_pair_ms=round(ref_ms, 1),
               stoi_pair0=got[0], estoi_pair0=got[1])
    line = json.dumps(rec)
    print(line)
    if not args.no_record:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "at") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
