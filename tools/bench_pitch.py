#!/usr/bin/env python
"""The three frame-level features of FastSpeech2 at the benchmark's batch: 32 utterances x 163 840 samples at 22 050 Hz, hop 256
(641 frames each), pitch range 80 - 400 Hz.  ``Pitch.get_pitch_batch`` (estimator + continuous / log step), the estimator
alone, ``Energy.get_energy_batch`` and the log-mel of the same device-resident batch run in one process on one device; each
figure is the median over ``--steps`` calls after ``--warmup``, timed with a device synchronise around the call.  The fp64
numpy restatement of the estimator (tests/pitch_ref.py) is timed on the host for ONE utterance.  Prints one JSON line; the
fraction of the fp32 vector peak counts 3 flop (a subtract and an FMA) per (frame, lag, term) against 157.3 TFLOP/s, a peak
that needs packed fp32 instructions; the kernel is built without them (the library's op_sel rule), which halves it.

``--tracker viterbi`` adds a second line for the Viterbi tracker: ``track_viterbi`` (estimator, candidates,
path) and ``get_pitch_batch`` of a ``tracker="viterbi"`` handle, timed INTERLEAVED with the frame picker's calls -- one call of
each per round, medians over the rounds -- and the kernels' own times from the context's event profiler in a pass of its own."""
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
    ap.add_argument("--tracker", choices=("frame", "viterbi"), default="frame",
                    help="viterbi: a second JSON line for the Viterbi tracker, timed interleaved with the frame picker")
    args = ap.parse_args(argv)
    import torch
    import pitch_ref as pr
    from parakeet_amd.audio import Energy, LogMelFBank, Pitch
    from parakeet_amd.runtime import Context
    sr, hop = 22050, 256
    ctx = Context.get()
    sig = pr.make_signal(sr, 0)
    host = [np.roll(np.tile(sig, args.samples // sig.size + 1)[:args.samples], 997 * b) for b in range(args.batch)]
    wavs = [ctx.to_device(w) for w in host]
    pitch = Pitch(sr, hop, 80, 400)
    energy = Energy(sr, 1024, hop, 1024)
    mel = LogMelFBank(sr, 1024, hop, 1024, n_mels=80, fmin=0, fmax=8000)

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
        return float(np.median(ms)), float(np.min(ms))

    est = timed(lambda: pitch._run(wavs))
    full = timed(lambda: pitch.get_pitch_batch(wavs))
    from_host = timed(lambda: pitch.get_pitch_batch(host))
    en = timed(lambda: energy.get_energy_batch(wavs))
    lm = timed(lambda: mel.get_log_mel_fbank_batch(wavs))
    t0 = time.perf_counter()
    ref = pr.track(host[0], sr, hop, 80, 400)
    ref_ms = (time.perf_counter() - t0) * 1e3
    frames = pitch.frames(args.samples)
    pairs = args.batch * frames * pitch.tau_max * pitch.win_length
    peak = 157.3e12
    print(json.dumps(dict(shape=f"{args.batch}x{args.samples}@{sr}/{hop}", frames=frames, lags=pitch.tau_max, window=pitch.win_length,
                          tile_frames=pitch.tile_frames, steps=args.steps,
                          estimator_ms=round(est[0], 4), estimator_min_ms=round(est[1], 4),
                          get_pitch_batch_ms=round(full[0], 4), get_pitch_batch_min_ms=round(full[1], 4),
                          get_pitch_batch_from_host_ms=round(from_host[0], 4),
                          get_energy_batch_ms=round(en[0], 4), log_mel_batch_ms=round(lm[0], 4),
                          numpy_fp64_one_utterance_ms=round(ref_ms, 1), voiced_frames_of_one=int((ref["lag"] > 0).sum()),
                          pairs=pairs, fraction_of_fp32_vector_peak_at_min=round(3 * pairs / (est[1] * 1e-3) / peak, 4))))
    if args.tracker != "viterbi":
        return
    vit = Pitch(sr, hop, 80, 400, tracker="viterbi")
    calls = [lambda: pitch._run(wavs), lambda: vit.track_viterbi(wavs), lambda: pitch.get_pitch_batch(wavs),
             lambda: vit.get_pitch_batch(wavs)]
    for _ in range(args.warmup):
        for fn in calls:
            fn()
    torch.cuda.synchronize()
    ms = [[] for _ in calls]
    for _ in range(args.steps):                                       # one call of each per round
        for k, fn in enumerate(calls):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3)
    med = [round(float(np.median(m)), 4) for m in ms]
    ctx.prof_enable(True)
    ctx.prof_reset()
    for _ in range(args.steps):
        vit.track_viterbi(wavs)
    torch.cuda.synchronize()
    prof = ctx.prof_dump()
    ctx.prof_enable(False)
    kern = {name: round(total / n, 4) for name, (n, total) in prof.items() if name.startswith("pitch")}
    got = vit.track_viterbi(wavs[:1])[0][1].cpu().numpy()
    print(json.dumps(dict(shape=f"{args.batch}x{args.samples}@{sr}/{hop}", tracker="viterbi", frames=frames, steps=args.steps,
                          max_candidates=vit.max_candidates, interleaved=True, estimator_ms=med[0], track_viterbi_ms=med[1],
                          get_pitch_batch_frame_ms=med[2], get_pitch_batch_viterbi_ms=med[3], kernel_ms=kern,
                          voiced_frames_of_one=int((got > 0).sum()))))


if __name__ == "__main__":
    main()
