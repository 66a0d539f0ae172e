#!/usr/bin/env python
"""Dynamic time warping at a corpus batch: 32 pairs of 640 x 600 frames with 13 coefficients, device-resident.  Timed: ``pk_dtw_run``
in matrix mode (on given costs) and in feature mode (cost kernel, then the search), the cost kernel alone (``pk_dtw_cost``),
``path_stats`` along the paths, and ``metrics.mcd_batch`` from (frames, 80) log-mels (DCT product, search, sums, read-back).  Each
figure is the median over ``--steps`` calls after ``--warmup``, timed on the host with a device synchronise around the call
(a call uploads its table of B entries and synchronises once for it).  The fp64 numpy restatement (tests/dtw_ref.py) is timed
on the host for ONE pair.  The search is latency-bound -- N + M - 1 dependent anti-diagonals, one wave per pair -- so no
roofline fraction is given: the figure to read is the time per anti-diagonal.  Prints one JSON line and appends it to
profiles/dtw_bench.jsonl (or ``--out``)."""
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
    ap.add_argument("--n-coef", type=int, default=13)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dtw_bench.jsonl"))
    ap.add_argument("--no-record", action="store_true", help="do not append to the record file")
    args = ap.parse_args(argv)
    import torch
    import dtw_ref as dr
    from parakeet_amd import metrics
    from parakeet_amd.alignment import dtw_features, path_stats
    from parakeet_amd.runtime import Context, dptr
    ctx = Context.get()
    B, N, M, K = args.batch, args.rows, args.cols, args.n_coef
    rng = np.random.default_rng(0)
    # log-mels of a "recording" and of a "synthesis" that follows it at another tempo, with noise on top
    base = np.cumsum(rng.standard_normal((B, N, 80)) * 0.3, axis=1) - 3.0
    pick = np.minimum((np.arange(M) * (N / M)).astype(np.int64), N - 1)
    ref_mel = base.astype(np.float32)
    syn_mel = (base[:, pick] + 0.1 * rng.standard_normal((B, M, 80))).astype(np.float32)
    d_ref, d_syn = [ctx.to_device(m) for m in ref_mel], [ctx.to_device(m) for m in syn_mel]
    cr, cs = metrics.mel_cepstrum(d_ref, K), metrics.mel_cepstrum(d_syn, K)
    D = K + 1
    x, y = torch.cat(list(cr)).contiguous(), torch.cat(list(cs)).contiguous()
    r32, c32 = np.full(B, N, np.int32), np.full(B, M, np.int32)
    i32p = C.POINTER(C.c_int32)
    rp, cp = r32.ctypes.data_as(i32p), c32.ctypes.data_as(i32p)
    cost = ctx.empty((B * N * M,))
    ix, iy = ctx.empty((B * (N + M - 1),), dtype=torch.int32), ctx.empty((B * (N + M - 1),), dtype=torch.int32)
    ln, status = ctx.empty((B,), dtype=torch.int32), ctx.empty((B,), dtype=torch.int32)
    q = ctx.empty((B,), dtype=torch.float64)

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

    def cost_only():
        rc = ctx.lib.pk_dtw_cost(ctx.handle, dptr(x), dptr(y), None, None, 0, 0, D, 1, D, rp, cp, B, dptr(cost))
        assert rc == 0, ctx.lib.pk_last_error()

    def run(mode):
        rc = ctx.lib.pk_dtw_run(ctx.handle, mode, dptr(cost if mode == 0 else x), dptr(y), None, None, 0, 0, D, 1, D, rp, cp, B,
                                dptr(ix), dptr(iy), dptr(ln), dptr(q), dptr(status))
        assert rc == 0, ctx.lib.pk_last_error()

    t_cost = timed(cost_only)
    t_matrix = timed(lambda: run(0))
    t_feat = timed(lambda: run(1))
    paths = dtw_features(list(cr), list(cs), (1, D))
    t_stats = timed(lambda: path_stats(paths, list(cr), list(cs), (1, D)))
    t_mcd = timed(lambda: metrics.mcd_batch(d_ref, d_syn, K))
    c0, c1 = cr[0].cpu().numpy(), cs[0].cpu().numpy()
    t0 = time.perf_counter()
    ref = dr.dtw_features(c0, c1, 1, D)
    ref_ms = (time.perf_counter() - t0) * 1e3
    assert np.array_equal(paths[0].ix.cpu().numpy(), ref["ix"]) and paths[0].cost == ref["cost"]
    rec = dict(shape=f"{B}x{N}x{M}x{K}", steps=args.steps,
               dtw_matrix_call_ms=round(t_matrix[0], 4), dtw_matrix_call_min_ms=round(t_matrix[1], 4),
               dtw_features_call_ms=round(t_feat[0], 4), dtw_features_call_min_ms=round(t_feat[1], 4),
               cost_kernel_call_ms=round(t_cost[0], 4), cost_kernel_call_min_ms=round(t_cost[1], 4),
               ns_per_antidiagonal_at_min=round(t_matrix[1] * 1e6 / (N + M - 1), 1),
               path_stats_ms=round(t_stats[0], 4), mcd_batch_ms=round(t_mcd[0], 4),
               numpy_fp64_one_pair_ms=round(ref_ms, 2))
    line = json.dumps(rec)
    print(line)
    if not args.no_record:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "at") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
