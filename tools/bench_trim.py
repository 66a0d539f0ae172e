#!/usr/bin/env python
"""Silence trimming at the benchmark's batch: 32 utterances x 7.43 s at 24 kHz (178 320 samples each, 23 MB).
``audio.trim_batch`` (frame 2048, hop 512, top_db 60) and ``audio.trim_long_silences_batch`` (30 ms windows, 8, 6, the energy
detector) from device-resident and from host inputs, in one process on one device; each figure is the median over ``--steps``
calls after ``--warmup``, timed on the host with a device synchronise around the call.  Kernel launches per call are read
from the engine's profiler.  The fp64 numpy restatement (tests/trim_ref.py) is timed on the host for ONE utterance.  Prints one
JSON line; nothing is asserted on time."""
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
    ap.add_argument("--samples", type=int, default=178320)
    args = ap.parse_args(argv)
    import torch
    import trim_ref as tr
    from parakeet_amd import audio
    from parakeet_amd.runtime import Context
    sr = 24000
    ctx = Context.get()
    w = tr.window_size(30, sr)
    base, _ = tr.burst_signal(gaps=(6, 9, 14, 25, 40), burst=20, sr=sr, w=w)
    host = [np.roll(np.tile(base, args.samples // base.size + 1)[:args.samples], 997 * b) for b in range(args.batch)]
    wavs = [ctx.to_device(x) for x in host]
    vad = dict(vad_window_length=30, vad_moving_average_width=8, vad_max_silence_length=6, sampling_rate=sr)

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.steps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        return round(float(np.median(ms)), 4), round(float(np.min(ms)), 4)

    def launches(fn):
        ctx.prof_enable(True)
        ctx.prof_reset()
        fn()
        ctx.sync()
        d = ctx.prof_dump()
        ctx.prof_enable(False)
        return {k: v[0] for k, v in d.items() if v[0]}

    trim_dev = timed(lambda: audio.trim_batch(wavs))
    trim_host = timed(lambda: audio.trim_batch(host))
    vad_dev = timed(lambda: audio.trim_long_silences_batch(wavs, **vad))
    vad_host = timed(lambda: audio.trim_long_silences_batch(host, **vad))
    peak = timed(lambda: audio.peak_normalize_batch(wavs))
    t0 = time.perf_counter()
    tr.trim_index(host[0])
    ref_trim = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    tr.trim_long_silences(host[0], tr.energy_flags(host[0], w)[1], w, 8, 6)
    ref_vad = (time.perf_counter() - t0) * 1e3
    kept = audio.trim_long_silences_batch(wavs, **vad)
    print(json.dumps(dict(shape=f"{args.batch}x{args.samples}@{sr}", bytes=4 * args.batch * args.samples, steps=args.steps,
                          tile_frames=audio.trim_tile_frames(2048, 512), frames=audio.trim_num_frames(args.samples, 2048, 512),
                          windows=args.samples // w, kept_samples_of_one=int(kept[0].numel()),
                          trim_batch_ms=trim_dev[0], trim_batch_min_ms=trim_dev[1], trim_batch_from_host_ms=trim_host[0],
                          trim_long_silences_batch_ms=vad_dev[0], trim_long_silences_batch_min_ms=vad_dev[1],
                          trim_long_silences_batch_from_host_ms=vad_host[0], peak_normalize_batch_ms=peak[0],
                          launches_trim_batch=launches(lambda: audio.trim_batch(wavs)),
                          launches_trim_long_silences_batch=launches(lambda: audio.trim_long_silences_batch(wavs, **vad)),
                          numpy_fp64_trim_one_utterance_ms=round(ref_trim, 2),
                          numpy_fp64_trim_long_silences_one_utterance_ms=round(ref_vad, 2))))


if __name__ == "__main__":
    main()
