#!/usr/bin/env python
"""Feature statistics at a corpus pass: an LJSpeech-sized corpus (13 100 utterances, lengths drawn around 800 frames) of
D = 80 log-mel rows, and D = 1 (pitch, energy) at the same row count, device-resident, through ``pk_stats_update`` as ONE
ragged call.  Each figure is the median over ``--steps`` calls after ``--warmup``, timed on the host with a device synchronise
around the call (the call itself uploads the tile table and synchronises once for it).  The kernel reads its input once, so
the yardstick is a device-to-device copy of the same bytes measured in the same run (``copy_ms``; a copy also writes them, so
equal time means the kernel reads at half the copy's traffic).  ``kernels_ms`` is the engine's own event timing of the three
launches.  Prints one JSON line per dimension and appends it to profiles/stats_bench.jsonl."""
import argparse
import ctypes as C
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
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--utterances", type=int, default=13100)
    ap.add_argument("--frames", type=int, default=800, help="mean utterance length")
    ap.add_argument("--dims", type=int, nargs="+", default=[80, 1])
    ap.add_argument("--no-record", action="store_true", help="do not append to profiles/stats_bench.jsonl")
    args = ap.parse_args(argv)
    import torch
    from parakeet_amd import _capi
    from parakeet_amd.normalizer import FeatureStats, stats_tile_rows
    from parakeet_amd.runtime import Context, dptr, randn
    ctx = Context.get()
    rng = np.random.default_rng(0)
    lens = np.clip(rng.normal(args.frames, args.frames / 4, args.utterances), 16, None).astype(np.int64)
    rows = int(lens.sum())

    def timed(fn, before=None):
        ms = []
        for i in range(args.warmup + args.steps):
            if before:
                before()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if i >= args.warmup:
                ms.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ms)), float(np.min(ms))

    for D in args.dims:
        x = (randn(rows * D, seed=D) * 0.3 + 5.2).reshape(rows, D)
        y = torch.empty_like(x)
        fs = FeatureStats(D)
        eng = fs._engine()
        lp = lens.ctypes.data_as(C.POINTER(C.c_int64))

        def update():
            _capi.check(ctx.lib.pk_stats_update(eng.h, dptr(x), lp, len(lens), None, 0))

        call = timed(update, before=lambda: fs.reset())
        copy = timed(lambda: y.copy_(x))
        ctx.prof_enable(True)
        ctx.prof_reset()
        fs.reset()
        update()
        ctx.sync()
        prof = ctx.prof_dump()
        ctx.prof_enable(False)
        again = FeatureStats(D).partial_fit_batch([x[:int(lens[0])], x[int(lens[0]):]])     # another split: the bound, not the bytes
        assert fs.n_samples_seen_ == rows and np.allclose(fs.mean_, again.mean_, rtol=1e-12)
        gb = rows * D * 4 / 1e9
        rec = dict(dim=D, utterances=int(args.utterances), rows=rows, tile_rows=stats_tile_rows(D), input_gb=round(gb, 4),
                   steps=args.steps, update_call_ms=round(call[0], 4), update_call_min_ms=round(call[1], 4),
                   copy_ms=round(copy[0], 4), copy_min_ms=round(copy[1], 4),
                   read_gb_per_s_at_min=round(gb / (call[1] * 1e-3), 1), copy_gb_per_s_at_min=round(2 * gb / (copy[1] * 1e-3), 1),
                   kernels_ms={k: round(v[1], 4) for k, v in prof.items() if k.startswith("stats_")})
        line = json.dumps(rec)
        print(line)
        if not args.no_record:
            out = os.path.join(ROOT, "profiles", "stats_bench.jsonl")
            os.makedirs(os.path.dirname(out), exist_ok=True)
            with open(out, "at") as f:
                f.write(line + "\n")
        del x, y


if __name__ == "__main__":
    main()
