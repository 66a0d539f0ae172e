#!/usr/bin/env python
"""Monotonic alignment search at a corpus batch: 32 utterances x 640 decoder steps x 128 tokens, device-resident, in scores
mode (``pk_mas_run`` on given scores) and in attention mode (``logf(max(A, eps))`` formed in the kernel), plus the focus rate
of the same maps.  Each figure is the median over ``--steps`` calls after ``--warmup``, timed on the host with a device
synchronise around the call (the call itself uploads a table of B entries and synchronises once for it).  The fp64 numpy
restatement (tests/mas_ref.py) is timed on the host for ONE utterance.  The kernel is latency-bound -- S dependent steps, one
wave per utterance -- so no roofline fraction is given: the figure to read is the time per row.  Prints one JSON line and
appends it to profiles/mas_bench.jsonl."""
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
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rows", type=int, default=640)
    ap.add_argument("--tokens", type=int, default=128)
    ap.add_argument("--no-record", action="store_true", help="do not append to profiles/mas_bench.jsonl")
    args = ap.parse_args(argv)
    import torch
    import mas_ref as mr
    from parakeet_amd.alignment import durations_from_attention, focus_rate, monotonic_align
    from parakeet_amd.runtime import Context, dptr
    ctx = Context.get()
    B, S, T = args.batch, args.rows, args.tokens
    rng = np.random.default_rng(0)
    # attention of a teacher that mostly follows the diagonal: a bump around t = s T / S on a noise floor
    s_idx, t_idx = np.arange(S)[:, None], np.arange(T)[None, :]
    att = np.exp(-0.5 * ((t_idx - s_idx * (T / S)) / 1.5) ** 2)[None] + 0.05 * rng.random((B, S, T))
    att = (att / att.sum(axis=2, keepdims=True)).astype(np.float32)
    d_att = ctx.to_device(att)
    d_scores = torch.log(torch.clamp(d_att, min=1e-8))
    rows, cols = [S] * B, [T] * B

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

    # the kernel with its launch alone: the C call with outputs allocated once (no read-back of the durations)
    r32, c32 = np.full(B, S, np.int32), np.full(B, T, np.int32)
    offs = (np.arange(B, dtype=np.int64) * S * T)
    dur, score, status = ctx.empty((B * T,), dtype=torch.int32), ctx.empty((B,), dtype=torch.float64), ctx.empty((B,), dtype=torch.int32)
    i32p, i64p = C.POINTER(C.c_int32), C.POINTER(C.c_int64)

    def raw(src, mode):
        rc = ctx.lib.pk_mas_run(ctx.handle, dptr(src), offs.ctypes.data_as(i64p), T, r32.ctypes.data_as(i32p), c32.ctypes.data_as(i32p),
                                B, mode, 1e-8, dptr(dur), None, dptr(score), dptr(status), None)
        assert rc == 0, ctx.lib.pk_last_error()

    raw_scores = timed(lambda: raw(d_scores, 0))
    raw_att = timed(lambda: raw(d_att, 1))
    api_scores = timed(lambda: monotonic_align(d_scores, rows, cols))
    api_att = timed(lambda: durations_from_attention(d_att, rows, cols))
    focus = timed(lambda: focus_rate(d_att, rows, cols))
    t0 = time.perf_counter()
    ref = mr.mas(mr.attention_scores_f64(att[0]).astype(np.float32))
    ref_ms = (time.perf_counter() - t0) * 1e3
    got, _ = monotonic_align(mr.attention_scores_f64(att[0]).astype(np.float32))
    assert np.array_equal(got, ref["durations"])
    rec = dict(shape=f"{B}x{S}x{T}", steps=args.steps,
               mas_scores_call_ms=round(raw_scores[0], 4), mas_scores_call_min_ms=round(raw_scores[1], 4),
               mas_attention_call_ms=round(raw_att[0], 4), mas_attention_call_min_ms=round(raw_att[1], 4),
               ns_per_row_at_min=round(raw_scores[1] * 1e6 / S, 1),
               monotonic_align_ms=round(api_scores[0], 4), durations_from_attention_ms=round(api_att[0], 4),
               focus_rate_ms=round(focus[0], 4), numpy_fp64_one_utterance_ms=round(ref_ms, 2))
    line = json.dumps(rec)
    print(line)
    if not args.no_record:
        out = os.path.join(ROOT, "profiles", "mas_bench.jsonl")
        os.makedirs(os.path.dirname(out), exist_ok=True)
        with open(out, "at") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
