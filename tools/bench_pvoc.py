#!/usr/bin/env python
"""The phase vocoder on 32 spectrograms of 321 frames x 1025 bins (163 840 samples each at n_fft 2048 / hop 512; seeded noise),
device-resident, at rate 0.8 (402 output frames): ``pk_pvoc_run`` timed by hipEvent (``torch.cuda.Event``) around the call,
which uploads its table of B entries and enqueues its one launch; the median and the minimum over ``--steps`` calls after
``--warmup``.  Beside it ``audio.time_stretch_batch`` on the waveforms (STFT, vocoder, ISTFT and the Python between them, by
wall clock with a device synchronisation) and the float64 numpy restatement for ONE utterance on the host.  Information only: no
threshold is set (the kernel is bound by the latency of a dependent float64 chain).  Prints one JSON line and
appends it to profiles/pvoc_bench.jsonl (or ``--out``)."""
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
    ap.add_argument("--samples", type=int, default=163840)
    ap.add_argument("--n-fft", type=int, default=2048)
    ap.add_argument("--rate", type=float, default=0.8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pvoc_bench.jsonl"))
    ap.add_argument("--no-record", action="store_true", help="do not append to the record file")
    args = ap.parse_args(argv)
    import ctypes as C
    import torch
    import pvoc_ref as R
    from parakeet_amd import audio
    from parakeet_amd.runtime import Context, dptr
    ctx = Context.get()
    B, L, n_fft, rate = args.batch, args.samples, args.n_fft, args.rate
    hop, nb = n_fft // 4, n_fft // 2 + 1
    F = 1 + L // hop
    T = audio.pvoc_num_frames(F, rate)
    rng = np.random.default_rng(0)
    spec0 = rng.standard_normal((F, 2 * nb)).astype(np.float32)
    x = ctx.to_device(np.concatenate([spec0] + [rng.standard_normal((F, 2 * nb)).astype(np.float32) for _ in range(B - 1)]))
    y = ctx.empty((B * T, 2 * nb))
    frames, rates = np.full(B, F, dtype=np.int32), np.full(B, rate, dtype=np.float64)
    fp, rp = frames.ctypes.data_as(C.POINTER(C.c_int32)), rates.ctypes.data_as(C.POINTER(C.c_double))

    def run():
        rc = ctx.lib.pk_pvoc_run(ctx.handle, dptr(x), fp, B, nb, rp, dptr(y))
        assert rc == 0, ctx.lib.pk_last_error()

    # the engine against the restatement on the first utterance before anything is timed
    t0 = time.perf_counter()
    want = R.phase_vocoder_rows(spec0, rate)
    numpy_ms = (time.perf_counter() - t0) * 1e3
    run()
    got = y[:T].cpu().numpy()
    assert (got.view(np.int32) == want.view(np.int32)).all()
    for _ in range(args.warmup):
        run()
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    wavs = [(0.1 * rng.standard_normal(L)).astype(np.float32) for _ in range(B)]
    dw = [ctx.to_device(w) for w in wavs]
    wall = []
    for i in range(3 + max(3, args.steps // 4)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        audio.time_stretch_batch(dw, rate, n_fft=n_fft)
        torch.cuda.synchronize()
        if i >= 3:
            wall.append((time.perf_counter() - t0) * 1e3)
    moved = B * nb * (F + T) * 8
    rec = dict(shape=f"{B}x{F}x{nb}", rate=rate, out_frames=T, steps=args.steps, pvoc_call_ms=round(float(np.median(ms)), 4),
               pvoc_call_min_ms=round(float(np.min(ms)), 4), bytes_in_plus_out=moved,
               gbytes_per_s=round(moved / (float(np.median(ms)) * 1e-3) / 1e9, 1),
               time_stretch_batch_wall_ms=round(float(np.median(wall)), 3), numpy_restatement_one_utt_ms=round(numpy_ms, 1))
    line = json.dumps(rec)
    print(line)
    if not args.no_record:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "at") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
