#!/usr/bin/env python
"""The GE2E similarity matrix and loss on the engine (pk_spk_ge2e: three launches) beside the same chain as torch ops on the
same GPU -- mean, norm, matmul, bmm, the masked replace, cross-entropy: the reference's own sequence -- and a whole
``evaluate_batch`` from mel partials; one JSON line each.

(a) resident embeddings (N, M, C): ``loss_terms`` + fold (terms and loss wanted, no matrix stored) and the full set
    (matrix, p1, p2, terms, loss), each against the torch chain; shapes (64, 10, 256) and (512, 20, 256).
(b) ``evaluate_batch`` of N * M partials x 160 frames at the released model shape, split into embed_sequences (the LSTM),
    the loss kernels (profiler records of the ge2e_* launches), the device-to-host copy of the matrix and the host EER.
Each figure is the median device-event (for host work: wall-clock) time of one whole call, 5 warm-ups, >= 20 timed.

  python tools/bench_ge2e_loss.py [--iters 20] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))


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
    return float(np.median(ts)), [round(t, 4) for t in ts]


def wall(fn, warm, iters):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), [round(t, 4) for t in ts]


def torch_chain(e, w, b):
    """lstm_speaker_encoder.py:55-134 as torch ops (the scatter by its documented meaning: an indexed overwrite)"""
    import torch.nn.functional as F
    N, M, C = e.shape
    ci = e.mean(dim=1)
    ci = ci / torch.linalg.vector_norm(ci, dim=1, keepdim=True)
    ce = (e.sum(dim=1, keepdim=True) - e) / (M - 1)
    ce = ce / torch.linalg.vector_norm(ce, dim=2, keepdim=True)
    rows = e.reshape(-1, C)
    p1 = torch.matmul(rows, ci.t()).reshape(-1)
    p2 = torch.bmm(rows.reshape(-1, 1, C), ce.reshape(-1, C, 1)).reshape(-1)
    index = torch.arange(N * M, device=e.device).reshape(N, M) * N + torch.arange(N, device=e.device).unsqueeze(-1)
    index = index.reshape(-1)
    ones = torch.ones(N * M * N, device=e.device)
    mask = ones.clone()
    mask[index] = 0.0
    sc = ones.clone()
    sc[index] = p2
    p = p1 * mask + (1 - mask) * sc
    p = (p * w + b).reshape(N * M, N)
    target = torch.arange(N, device=e.device).unsqueeze(-1).expand(N, M).reshape(-1)
    return F.cross_entropy(p, target), p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None, help="append the lines to this file")
    args = ap.parse_args()
    import ge2e_loss_ref as ref
    from parakeet_amd import build as pk_build
    from parakeet_amd import synthetic as syn
    from parakeet_amd.lstm_speaker_encoder import LSTMSpeakerEncoder, equal_error_rate
    from parakeet_amd.runtime import Context
    cfg = syn.GE2E_RELEASED
    m = LSTMSpeakerEncoder(**cfg)
    m.set_state_dict(syn.ge2e_state(cfg, seed=11))
    m.eval()
    ctx = Context.get()
    lines = []
    src = pk_build.file_hash("spk_loss.hip")[:16]
    w = torch.tensor(10.0, device="cuda")
    b = torch.tensor(-5.0, device="cuda")
    for shape in ((64, 10, 256), (512, 20, 256)):
        N, M, C = shape
        e = torch.from_numpy(ref.embeddings(N, M, C, seed=9)).cuda()
        base = dict(bench="a: resident embeddings", shape=list(shape), flop_p1=2.0 * N * M * N * C, source_hash=src)
        with torch.no_grad():
            ms_t, ts_t = timed(lambda: torch_chain(e, w, b), 5, args.iters)
            loss_t, p_t = torch_chain(e, w, b)
        lines.append(dict(base, what="torch chain (mean, norm, matmul, bmm, masked replace, cross_entropy)", ms=round(ms_t, 4),
                          all_ms=ts_t))
        ms_l, ts_l = timed(lambda: m._ge2e(e, terms=True, loss=True), 5, args.iters)
        ms_f, ts_f = timed(lambda: m._ge2e(e, sim=True, p1=True, p2=True, terms=True, loss=True), 5, args.iters)
        o = m._ge2e(e, sim=True, loss=True)
        diff = float((o["sim"] - p_t).abs().max())
        ctx.prof_reset()
        ctx.prof_enable(True)
        for _ in range(args.iters):
            m._ge2e(e, terms=True, loss=True)
        ctx.sync()
        prof = {k: round(v[1] / v[0], 4) for k, v in ctx.prof_dump().items() if k.startswith("ge2e_")}
        ctx.prof_enable(False)
        lines.append(dict(base, what="pk_spk_ge2e: terms + loss", ms=round(ms_l, 4), all_ms=ts_l, kernel_ms=prof,
                          torch_over_engine=round(ms_t / ms_l, 3), loss=float(o["loss"][0]), loss_torch=float(loss_t),
                          p_max_diff_to_torch=diff))
        lines.append(dict(base, what="pk_spk_ge2e: p, p1, p2, terms, loss", ms=round(ms_f, 4), all_ms=ts_f,
                          torch_over_engine=round(ms_t / ms_f, 3)))
    # (b) evaluate_batch from partials at the released shape
    for N, M in ((64, 10),):
        x = torch.from_numpy(np.exp(np.random.default_rng(1).normal(-2.0, 2.0, size=(N * M, 160, cfg["n_mels"])))
                             .astype(np.float32)).cuda()
        ms_all, ts_all = wall(lambda: m.evaluate_batch(x, N), 3, args.iters)
        ms_emb, _ = timed(lambda: m.embed_sequences(x), 3, args.iters)
        emb = m.embed_sequences(x).reshape(N, M, -1)
        ms_loss, _ = timed(lambda: m._ge2e(emb, sim=True, loss=True), 3, args.iters)
        sim = m._ge2e(emb, sim=True)["sim"]
        ms_copy, _ = wall(lambda: sim.cpu(), 3, args.iters)
        labels, scores = ref.labels(N, M), sim.cpu().numpy()
        t = []
        for _ in range(args.iters):
            t0 = time.perf_counter()
            eer = equal_error_rate(labels, scores)
            t.append((time.perf_counter() - t0) * 1e3)
        out = m.evaluate_batch(x, N)
        lines.append(dict(bench="b: evaluate_batch", workload=f"{N * M} partials x 160 frames, released shape, N = {N}, M = {M}",
                          ms=round(ms_all, 3), all_ms=ts_all, embed_sequences_ms=round(ms_emb, 3), ge2e_kernels_ms=round(ms_loss, 4),
                          matrix_to_host_ms=round(ms_copy, 4), host_eer_ms=round(float(np.median(t)), 3),
                          loss=float(out["loss"]), eer=eer, source_hash=src))
    for l in lines:
        print(json.dumps(l), flush=True)
    if args.out:
        with open(args.out, "at") as f:
            for l in lines:
                f.write(json.dumps(l) + "\n")


if __name__ == "__main__":
    main()
