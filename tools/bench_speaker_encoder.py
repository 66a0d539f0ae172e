#!/usr/bin/env python
"""GE2E speaker encoder throughput: wav -> embeddings for a corpus batch, one JSON line.

Workload: 256 utterances with lengths U[2 s, 8 s] (seeded synthetic clips, 16 kHz) at examples/ge2e/inference.py's
settings (partial overlap 0.75), released model shape (40 mels, 3 x 256 LSTM, 256 out), default math.
Reports the median device-event time (5 warm-ups, >= 20 timed) of preprocess-free wav -> partials -> embeddings,
utterances/s and partials/s, the per-layer recurrence time from the engine profiler and its us per step, the FLOP share
of the matrix pipe's peak, the one-clip latency (4 s, notebook settings: overlap 0.5) and a torch-CPU restatement of the
model (LSTM, head, per-utterance mean; no front end) on 16 threads at the same batch, median of 3 runs after a warm-up.

  python tools/bench_speaker_encoder.py [--utts 256] [--iters 20] [--cpu-runs 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from parakeet_amd import ge2e_audio, synthetic as syn  # noqa: E402
from parakeet_amd.lstm_speaker_encoder import LSTMSpeakerEncoder  # noqa: E402
from parakeet_amd.runtime import Context  # noqa: E402
import ge2e_ref  # noqa: E402

PEAK_F16_TFLOPS = 2516.6   # MI355X dense fp16 matrix peak (256 CUs x 2.4 GHz x 4096 FLOP / clk)
PEAK_F32_TFLOPS = 157.3    # fp32 matrix peak


def model_flop(P, T, cfg):
    """Multiply-adds x 2 of the LSTM (input projection + recurrence, 4 gates) and the head, from shapes."""
    H, L, C, O = cfg["hidden_size"], cfg["num_layers"], cfg["n_mels"], cfg["output_size"]
    per_layer = [2 * T * 4 * H * ((C if l == 0 else H) + H) for l in range(L)]
    return P * (sum(per_layer) + 2 * H * O), [P * f for f in per_layer]


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
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=256)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--cpu-runs", type=int, default=3)
    args = ap.parse_args()
    cfg = syn.GE2E_RELEASED
    rng = np.random.default_rng(2021)
    secs = rng.uniform(2.0, 8.0, size=args.utts)
    clips = [ge2e_ref.synthetic_clip(s, seed=1000 + i) for i, s in enumerate(secs)]
    pre = ge2e_audio.ge2e_preprocessor(overlap=0.75)
    wavs = [pre.preprocess_wav(c) for c in clips]
    enc = LSTMSpeakerEncoder(**cfg)
    enc.set_state_dict(syn.ge2e_state(cfg, seed=7))
    enc.eval()

    def run():
        return enc.embed_utterances(pre.extract_mel_partials_batch(wavs))

    parts = pre.extract_mel_partials_batch(wavs)
    P = int(sum(p.shape[0] for p in parts))
    T = 160
    ms = timed(run, 5, args.iters)
    flop, per_layer_flop = model_flop(P, T, cfg)
    # recurrence per layer from the engine profiler (one profiled call)
    ctx = Context.get()
    ctx.prof_reset()
    ctx.prof_enable(True)
    run()
    torch.cuda.synchronize()
    prof = ctx.prof_dump()
    ctx.prof_enable(False)
    rec = {k: v[1] for k, v in prof.items() if k.startswith("spk_")}
    rec_layers = [rec.get(f"spk_lstm_rec_l{i}", 0.0) for i in range(2)] + [rec.get("spk_lstm_rec_l2+", 0.0)]
    enc_ms = sum(v for k, v in rec.items())
    # one clip, notebook settings
    pre1 = ge2e_audio.ge2e_preprocessor(overlap=0.5)
    w1 = pre1.preprocess_wav(ge2e_ref.synthetic_clip(4.0, seed=5))
    one_ms = timed(lambda: enc.embed_utterance(pre1.extract_mel_partials(w1)), 5, args.iters)
    # torch-CPU restatement (fp32 nn.LSTM + relu(linear) + normalize + per-utterance mean, normalize) on 16 threads at the
    # same partial batch: one warm-up, the median of --cpu-runs timed runs (the front end is not in it)
    torch.set_num_threads(16)
    lstm = torch.nn.LSTM(cfg["n_mels"], cfg["hidden_size"], cfg["num_layers"], batch_first=True)
    st = syn.ge2e_state(cfg, seed=7)
    W, bias = torch.from_numpy(st["linear.weight"]), torch.from_numpy(st["linear.bias"])
    cu = np.concatenate([[0], np.cumsum([int(p.shape[0]) for p in parts])])
    xs = torch.cat([p.cpu() for p in parts], 0)

    def cpu_run():
        _, (h, _) = lstm(xs)
        e = torch.nn.functional.normalize(torch.relu(h[-1] @ W + bias), dim=1)
        return torch.stack([torch.nn.functional.normalize(e[a:b].mean(0), dim=0) for a, b in zip(cu[:-1], cu[1:])])

    cpu_ts = []
    with torch.no_grad():
        for name, p in lstm.named_parameters():
            p.copy_(torch.from_numpy(st["lstm." + name]))
        cpu_run()
        for _ in range(args.cpu_runs):
            t0 = time.perf_counter()
            cpu_run()
            cpu_ts.append((time.perf_counter() - t0) * 1e3)
    cpu_ms = float(np.median(cpu_ts))
    out = {
        "metric": "ge2e_wav_to_embedding",
        "utterances": args.utts, "partials": P, "frames_per_partial": T,
        "median_ms": round(ms, 3),
        "utterances_per_s": round(args.utts / ms * 1e3, 1),
        "partials_per_s": round(P / ms * 1e3, 1),
        "engine_kernels_ms": round(enc_ms, 3),
        "rec_ms_per_layer": [round(v, 3) for v in rec_layers],
        "rec_us_per_step": [round(v * 1e3 / T, 2) for v in rec_layers],
        "model_gflop": round(flop / 1e9, 2),
        "mflop_per_partial": round(flop / P / 1e6, 1),
        "f16_pipe_peak_share": round(flop / (ms * 1e-3) / (PEAK_F16_TFLOPS * 1e12), 4),
        "one_clip_4s_ms": round(one_ms, 3),
        "cpu_torch16_ms": round(cpu_ms, 1),
        "cpu_torch16_runs_ms": [round(v, 1) for v in cpu_ts],
        "speedup_vs_cpu": round(cpu_ms / ms, 1),
        "profile_ms": {k: round(v, 3) for k, v in rec.items()},
    }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
