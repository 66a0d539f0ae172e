#!/usr/bin/env python
"""The K-weighting filter and gated loudness of 32 utterances of 163 840 samples at 22 050 Hz (7.43 s each; seeded noise under
a tone), device-resident: ``pk_iir_run`` and ``pk_loudness_run`` timed by hipEvent (``torch.cuda.Event``) around the call, which
uploads its table of B entries and enqueues its launches; the median and the minimum over ``--steps`` calls after ``--warmup``,
and from the engine's profiler the median of every launch alone (the local, carry and apply passes, the segment and gate
stages).  Beside it ``scipy.signal.sosfilt`` in float64 on the host for the same batch, with the number of cores the process
may use (scipy runs the recursion on one).  Information only: no threshold is set and no roofline fraction is given (the
passes are bound by the latency of the dependent float64 chain).  Prints one JSON line and appends it to
profiles/iir_bench.jsonl (or ``--out``)."""
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
    ap.add_argument("--sr", type=int, default=22050)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "iir_bench.jsonl"))
    ap.add_argument("--no-record", action="store_true", help="do not append to the record file")
    args = ap.parse_args(argv)
    import ctypes as C
    import scipy.signal
    import torch
    import iir_ref as R
    from parakeet_amd import audio, metrics
    from parakeet_amd.runtime import Context, dptr
    ctx = Context.get()
    B, L, sr = args.batch, args.samples, args.sr
    rng = np.random.default_rng(0)
    t = np.arange(L) / sr
    xs = [((0.05 + 0.01 * b) * (np.sin(2 * np.pi * (110.0 + 20 * b) * t) + 0.3 * rng.standard_normal(L))).astype(np.float32)
          for b in range(B)]
    sos = audio.k_weighting(sr)
    eng = audio._iir_engine(sos)
    x = ctx.to_device(np.concatenate(xs))
    y = ctx.empty((B * L,))
    lens = np.full(B, L, dtype=np.int32)
    lp = lens.ctypes.data_as(C.POINTER(C.c_int32))
    mean, rel = ctx.empty((B,), torch.float64), ctx.empty((B,), torch.float64)
    peak, counts = ctx.empty((B,)), ctx.empty((3 * B,), torch.int32)

    def run_filter():
        rc = ctx.lib.pk_iir_run(eng.h, dptr(x), lp, B, dptr(y))
        assert rc == 0, ctx.lib.pk_last_error()

    def run_loud():
        rc = ctx.lib.pk_loudness_run(eng.h, dptr(x), lp, B, sr, dptr(mean), dptr(rel), dptr(peak), dptr(counts))
        assert rc == 0, ctx.lib.pk_last_error()

    def timed(run):
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
        return float(np.median(ms)), float(np.min(ms))

    def launches(run, prefixes):
        ctx.prof_enable(True)
        seen = {}
        for _ in range(max(3, args.steps // 4)):
            ctx.prof_reset()
            run()
            ctx.sync()
            for k, v in ctx.prof_dump().items():
                if k.startswith(prefixes) and v[0] > 0:          # (names of earlier calls stay listed with no launches)
                    seen.setdefault(k, []).append(v[1])
        ctx.prof_enable(False)
        return {k: round(float(np.median(v)), 4) for k, v in seen.items()}

    # the engine against the restatement on the first utterance before anything is timed
    want = R.loudness(xs[0], sr)
    got = metrics.loudness_batch(xs[:1], sr, return_details=True)[0]
    assert got["mean_power"] == want["mean_power"] and got["gated"] == want["gated"], (got, want)
    t_f, t_l = timed(run_filter), timed(run_loud)
    l_f, l_l = launches(run_filter, ("iir_",)), launches(run_loud, ("iir_", "loud_"))
    host = np.stack(xs).astype(np.float64)
    t0 = time.perf_counter()
    ref = scipy.signal.sosfilt(sos, host, axis=-1)
    scipy_ms = (time.perf_counter() - t0) * 1e3
    run_filter()
    err = float(np.abs(y.cpu().numpy().reshape(B, L) - ref).max() / np.abs(ref).max())
    rec = dict(shape=f"{B}x{L}", sr=sr, sections=int(sos.shape[0]), seconds_of_audio=round(B * L / sr, 1), steps=args.steps,
               filter_call_ms=round(t_f[0], 4), filter_call_min_ms=round(t_f[1], 4), loudness_call_ms=round(t_l[0], 4),
               loudness_call_min_ms=round(t_l[1], 4), filter_launch_ms=l_f, loudness_launch_ms=l_l,
               scipy_sosfilt_f64_ms=round(scipy_ms, 1), host_cores=len(os.sched_getaffinity(0)),
               filter_vs_scipy_rel=err, lufs_utt0=got["lufs"])
    line = json.dumps(rec)
    print(line)
    if not args.no_record:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "at") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
