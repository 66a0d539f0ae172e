#!/usr/bin/env python
"""The edit distance at two batches, device-resident: 32 pairs of 640 x 600 ids (the shape tools/bench_dtw.py uses) and a
baker-sized corpus of 10 000 ragged pairs of 40 - 80 ids (30 symbols, a tenth of the ids edited; seeded).  Timed: ``pk_edit_run``
in mode 0 (distance) and mode 1 (distance, counts, ops) on both, and beside them from the same run ``pk_dtw_run`` in matrix
mode at 32 x (640 x 600) -- the float64 search of DESIGN.md 4.7b, not the code under test -- and the numpy restatement
(tests/edit_ref.py) on the host for one 640 x 600 pair and for 100 of the corpus pairs, scaled to the corpus.  Each device figure
is the median over ``--steps`` calls after ``--warmup``, timed on the host with a device synchronise around the call (a call
uploads its table of B entries).  The search is latency-bound -- N + M - 1 dependent anti-diagonals, one wave per pair -- so no
roofline fraction is given: the figure to read is the time per anti-diagonal.  Prints one JSON line and appends it to
profiles/edit_bench.jsonl (or ``--out``)."""
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
    ap.add_argument("--cols", type=int, default=600)
    ap.add_argument("--corpus", type=int, default=10000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "edit_bench.jsonl"))
    ap.add_argument("--no-record", action="store_true", help="do not append to the record file")
    args = ap.parse_args(argv)
    import torch
    import edit_ref as er
    from parakeet_amd.runtime import Context, dptr
    ctx = Context.get()
    i32p = C.POINTER(C.c_int32)
    rng = np.random.default_rng(0)

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

    def batch(refs, hyps):
        """-> run(mode), check(): the call on device-resident packed ids and its comparison with the restatement."""
        n, m = np.array([r.size for r in refs], np.int32), np.array([h.size for h in hyps], np.int32)
        B = int(n.size)
        tr, th = ctx.to_device(np.concatenate(refs), dtype=torch.int32), ctx.to_device(np.concatenate(hyps), dtype=torch.int32)
        dist, ln = ctx.empty((B,), dtype=torch.int32), ctx.empty((B,), dtype=torch.int32)
        counts, ops = ctx.empty((B, 4), dtype=torch.int32), ctx.empty((int((n + m).sum()),), dtype=torch.uint8)

        def run(mode):
            rc = ctx.lib.pk_edit_run(ctx.handle, dptr(tr), dptr(th), None, None, n.ctypes.data_as(i32p), m.ctypes.data_as(i32p), B,
                                     mode, dptr(dist), dptr(counts), dptr(ops), dptr(ln))
            assert rc == 0, ctx.lib.pk_last_error()

        def check(upto):
            run(1)
            d, c = dist.cpu().numpy(), counts.cpu().numpy()
            for b in range(upto):
                want = er.align(refs[b], hyps[b])
                assert d[b] == want["distance"] and np.array_equal(c[b], want["counts"]), b
        return run, check

    # 32 x (640 x 600): 30 symbols, the hypothesis the reference cut to M ids with a tenth of them edited
    B, N, M = args.batch, args.rows, args.cols
    refs = [rng.integers(0, 30, size=N).astype(np.int32) for _ in range(B)]
    hyps = [np.resize(er.plant(rng, np.resize(r, M), M // 10, 30)[0], M).astype(np.int32) for r in refs]
    run_big, check_big = batch(refs, hyps)
    check_big(2)
    t_big0, t_big1 = timed(lambda: run_big(0)), timed(lambda: run_big(1))
    t0 = time.perf_counter()
    er.align(refs[0], hyps[0])
    ref_big_ms = (time.perf_counter() - t0) * 1e3

    # the corpus: ragged 40 - 80 ids
    Bc = args.corpus
    crefs = [rng.integers(0, 30, size=int(rng.integers(40, 81))).astype(np.int32) for _ in range(Bc)]
    chyps = [er.plant(rng, r, max(1, r.size // 10), 30)[0] for r in crefs]
    run_c, check_c = batch(crefs, chyps)
    check_c(min(Bc, 20))
    t_c0, t_c1 = timed(lambda: run_c(0)), timed(lambda: run_c(1))
    t0 = time.perf_counter()
    for b in range(min(Bc, 100)):
        er.align(crefs[b], chyps[b])
    ref_corpus_ms = (time.perf_counter() - t0) * 1e3 * Bc / min(Bc, 100)

    # pk_dtw_run, matrix mode, at the first shape on this machine
    cost = ctx.to_device(rng.random(B * N * M).astype(np.float32))
    r32, c32 = np.full(B, N, np.int32), np.full(B, M, np.int32)
    ix, iy = ctx.empty((B * (N + M - 1),), dtype=torch.int32), ctx.empty((B * (N + M - 1),), dtype=torch.int32)
    pl, status, q = ctx.empty((B,), dtype=torch.int32), ctx.empty((B,), dtype=torch.int32), ctx.empty((B,), dtype=torch.float64)

    def dtw():
        rc = ctx.lib.pk_dtw_run(ctx.handle, 0, dptr(cost), None, None, None, 0, 0, 0, 0, 0, r32.ctypes.data_as(i32p),
                                c32.ctypes.data_as(i32p), B, dptr(ix), dptr(iy), dptr(pl), dptr(q), dptr(status))
        assert rc == 0, ctx.lib.pk_last_error()
    t_dtw = timed(dtw)

    rec = dict(shape=f"{B}x{N}x{M}", corpus=f"{Bc}x40-80", steps=args.steps,
               edit_distance_call_ms=round(t_big0[0], 4), edit_distance_call_min_ms=round(t_big0[1], 4),
               edit_align_call_ms=round(t_big1[0], 4), edit_align_call_min_ms=round(t_big1[1], 4),
               ns_per_antidiagonal_at_min=round(t_big1[1] * 1e6 / (N + M - 1), 1),
               dtw_matrix_call_ms=round(t_dtw[0], 4), dtw_matrix_call_min_ms=round(t_dtw[1], 4),
               corpus_distance_call_ms=round(t_c0[0], 4), corpus_distance_call_min_ms=round(t_c0[1], 4),
               corpus_align_call_ms=round(t_c1[0], 4), corpus_align_call_min_ms=round(t_c1[1], 4),
               numpy_one_pair_ms=round(ref_big_ms, 2), numpy_corpus_scaled_ms=round(ref_corpus_ms, 1))
    line = json.dumps(rec)
    print(line)
    if not args.no_record:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "at") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
