"""Score free-running synthesis against the recordings: mel-cepstral distortion and log-F0 RMSE along a dynamic-time-warping
path (parakeet_amd.metrics) -- the numbers for wavs whose lengths differ from the recordings', where the
teacher-forced criteria of the ``*_gta.py`` examples and the sample-aligned score_vocoder.py have nothing to say.

For every <utt_id>.wav in --gen-dir with a <utt_id>.wav in --ref-dir (PCM or float, any rate; a pair is scored at the
recording's rate, generated audio at another rate is resampled to it on the engine and the line says so) one tab-separated line

    utt_id  ref_frames  gen_frames  length_ratio  path_length  mcd_db  f0_rmse_cents  f0_rmse_nats  vuv_error  voiced_both

then the corpus means.  With --gen-mel-dir / --ref-mel-dir the pairs are <utt_id>.npy log-mels (frames, n_mels) in base 10 (what
``LogMelFBank`` and the ``*_gta.py`` examples write) and the f0 columns are missing.

These are this project's own definitions: the cepstra are the orthonormal DCT-II of the log-mel spectrum (NOT SPTK's
mel-cepstrum), the warping is unconstrained with a squared Euclidean local cost over c_1 ... c_n_coef, f0 is ``audio.Pitch``'s
(not pyworld's).  Nobody has compared these numbers with another toolkit's on speech.

    python examples/score_synthesis.py --gen-dir generated --ref-dir recordings [--config conf/default.yaml] [--n-coef 13]
    python examples/score_synthesis.py --gen-mel-dir gen_mels --ref-mel-dir ref_mels
"""
import argparse
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from parakeet_amd import metrics  # noqa: E402
from parakeet_amd.audio import LogMelFBank, Pitch, load_wav  # noqa: E402

WAV_COLUMNS = ("rows", "cols", "length_ratio", "length", "mcd", "f0_rmse_cents", "f0_rmse", "vuv_error", "voiced_both")
MEL_COLUMNS = ("rows", "cols", "length_ratio", "length", "mcd")
MEANS = ("length_ratio", "mcd", "f0_rmse_cents", "f0_rmse", "vuv_error")


def _fmt(v):
    return str(v) if isinstance(v, (int, np.integer)) else f"{v:.6f}"


def _ids(gen_dir, ref_dir, ext):
    ids = sorted(f[:-len(ext)] for f in os.listdir(gen_dir) if f.endswith(ext) and os.path.exists(os.path.join(ref_dir, f)))
    if not ids:
        raise SystemExit(f"no <utt_id>{ext} present in both directories")
    return ids


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--gen-dir", default=None, help="synthesised waveforms")
    ap.add_argument("--ref-dir", default=None, help="recordings")
    ap.add_argument("--gen-mel-dir", default=None, help="synthesised log-mels (.npy, base 10) instead of waveforms")
    ap.add_argument("--ref-mel-dir", default=None, help="reference log-mels (.npy, base 10)")
    ap.add_argument("--config", default=None, help="the recipe's yaml: fs, n_fft, n_shift, win_length, window, n_mels, fmin, fmax, "
                                                   "f0min, f0max (default: the project's 24 kHz / 2048 / 300 / 80 bands)")
    ap.add_argument("--n-coef", type=int, default=13, help="cepstral coefficients c_1 ... c_n (c_0 is excluded)")
    ap.add_argument("--batch", type=int, default=16, help="pairs per call")
    ap.add_argument("--f0min", type=float, default=None)
    ap.add_argument("--f0max", type=float, default=None)
    a = ap.parse_args(argv)
    wav_mode = a.gen_dir is not None or a.ref_dir is not None
    if wav_mode == (a.gen_mel_dir is not None or a.ref_mel_dir is not None) or \
            (wav_mode and None in (a.gen_dir, a.ref_dir)) or (not wav_mode and None in (a.gen_mel_dir, a.ref_mel_dir)):
        raise SystemExit("give --gen-dir and --ref-dir, or --gen-mel-dir and --ref-mel-dir")
    cfg = {}
    if a.config:
        import yaml
        with open(a.config) as f:
            cfg = yaml.safe_load(f)
    rows = []
    columns = WAV_COLUMNS if wav_mode else MEL_COLUMNS
    print("# utt_id\t" + "\t".join(columns))
    if wav_mode:
        ids = _ids(a.gen_dir, a.ref_dir, ".wav")
        extractors = {}
        for i in range(0, len(ids), a.batch):
            by_rate = {}
            for u in ids[i:i + a.batch]:
                y, sr = load_wav(os.path.join(a.ref_dir, u + ".wav"))
                x, sx = load_wav(os.path.join(a.gen_dir, u + ".wav"))
                note = ""
                if sx != sr:
                    note = f"\tresampled from {sx} Hz to {sr} Hz"
                    x = load_wav(os.path.join(a.gen_dir, u + ".wav"), sr=sr)[0]
                by_rate.setdefault(int(sr), []).append((u, y, x, note))
            for sr, items in by_rate.items():
                if sr not in extractors:
                    if cfg and int(cfg["fs"]) != sr:
                        raise SystemExit(f"{items[0][0]}: the recording is at {sr} Hz, the config's fs is {cfg['fs']}")
                    hop = int(cfg.get("n_shift", 300))
                    mel = LogMelFBank(sr=sr, n_fft=int(cfg.get("n_fft", 2048)), hop_length=hop, win_length=cfg.get("win_length"),
                                      window=cfg.get("window", "hann"), n_mels=int(cfg.get("n_mels", 80)), fmin=cfg.get("fmin", 80),
                                      fmax=cfg.get("fmax", 7600))
                    pitch = Pitch(sr=sr, hop_length=hop, f0min=a.f0min or cfg.get("f0min", 80), f0max=a.f0max or cfg.get("f0max", 400))
                    extractors[sr] = (mel, pitch)
                mel, pitch = extractors[sr]
                out = metrics.score_batch([it[1] for it in items], [it[2] for it in items], sr, mel=mel, pitch=pitch, n_coef=a.n_coef)
                for (u, _, _, note), r in zip(items, out):
                    rows.append(dict(r, utt_id=u, note=note))
        rows.sort(key=lambda r: r["utt_id"])
    else:
        ids = _ids(a.gen_mel_dir, a.ref_mel_dir, ".npy")
        for i in range(0, len(ids), a.batch):
            part = ids[i:i + a.batch]
            refs = [np.load(os.path.join(a.ref_mel_dir, u + ".npy")).astype(np.float32) for u in part]
            gens = [np.load(os.path.join(a.gen_mel_dir, u + ".npy")).astype(np.float32) for u in part]
            for u, r in zip(part, metrics.mcd_batch(refs, gens, a.n_coef, 10.0)):
                rows.append(dict(r, utt_id=u, note=""))
    for r in rows:
        print(r["utt_id"] + "\t" + "\t".join(_fmt(r[c]) for c in columns) + r["note"])
    means = []
    for c in columns:
        vals = [r[c] for r in rows if c in MEANS and not math.isnan(r[c])]
        means.append(_fmt(float(np.mean(vals))) if vals else "-")
    print("MEAN\t" + "\t".join(means) + f"\tover {len(rows)} utterances")
    return rows


if __name__ == "__main__":
    main()
