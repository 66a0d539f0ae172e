#!/usr/bin/env python
"""Mel spectrograms to WAV files with Griffin-Lim on the MI355X engine: a vocoder without weights, for listening to the
mels of an acoustic model when no neural vocoder of the matching feature domain is at hand (the reference's released
Tacotron2 and TransformerTTS v0.1 models list "Vocoder: Griffin-Lim", docs/src/released_models.md).

Reads every ``.npy`` of ``--input-dir`` -- (frames, n_mels) as ``examples/tacotron2_gta.py`` and
``examples/transformer_tts_gta.py`` write them, or (n_mels, frames) with ``--bins-first`` -- and writes ``<name>.wav`` to
``--output-dir``.  The mels are taken as natural-log magnitudes (``LogMagnitude``, the Tacotron2 / TransformerTTS / WaveFlow
domain) unless ``--linear``; the pipeline is exp, the pseudo-inverse of the mel filterbank, ``** power`` and fast Griffin-Lim
(``parakeet_amd.audio.GriffinLim``), one ragged batch per ``--batch-size`` files.  The STFT arguments default to the
Tacotron2 recipe's (examples/tacotron2/config.py).
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--input-dir", required=True)
    ap.add_argument("--output-dir", required=True)
    ap.add_argument("--sample-rate", type=int, default=22050)
    ap.add_argument("--n-fft", type=int, default=1024)
    ap.add_argument("--win-length", type=int, default=1024)
    ap.add_argument("--hop-length", type=int, default=256)
    ap.add_argument("--n-mels", type=int, default=80)
    ap.add_argument("--fmin", type=float, default=0)
    ap.add_argument("--fmax", type=float, default=8000)
    ap.add_argument("--n-iter", type=int, default=32)
    ap.add_argument("--momentum", type=float, default=0.99)
    ap.add_argument("--power", type=float, default=1.0, help="exponent on the linear magnitudes (above 1 sharpens harmonics)")
    ap.add_argument("--seed", type=int, default=0, help="seed of the initial phases; utterance i uses seed + i")
    ap.add_argument("--batch-size", type=int, default=32)
    ap.add_argument("--linear", action="store_true", help="the mels are linear magnitudes, not natural logs")
    ap.add_argument("--bins-first", action="store_true", help="the files hold (n_mels, frames)")
    ap.add_argument("--transform", choices=("dense", "fft"), default="dense",
                    help="fft: run the STFT and its inverse on the radix FFT (n_fft a power of two from 32 to 4096)")
    return ap.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    from parakeet_amd.audio import AudioProcessor, GriffinLim, LogMagnitude
    proc = AudioProcessor(args.sample_rate, args.n_fft, args.win_length, args.hop_length, n_mels=args.n_mels,
                          fmin=args.fmin, fmax=args.fmax, transform=args.transform)
    voc = GriffinLim(proc, None if args.linear else LogMagnitude(), n_iter=args.n_iter, momentum=args.momentum,
                     power=args.power)
    names = sorted(f for f in os.listdir(args.input_dir) if f.endswith(".npy"))
    if not names:
        raise SystemExit(f"no .npy file in {args.input_dir}")
    os.makedirs(args.output_dir, exist_ok=True)
    for i in range(0, len(names), args.batch_size):
        chunk = names[i:i + args.batch_size]
        mels = []
        for name in chunk:
            m = np.load(os.path.join(args.input_dir, name)).astype(np.float32)
            m = m if args.bins_first else m.T
            if m.ndim != 2 or m.shape[0] != args.n_mels:
                raise SystemExit(f"{name}: expected {args.n_mels} mel bins, got an array of shape {m.shape}")
            mels.append(m)
        wavs = voc.infer_batch(mels, seeds=[args.seed + i + j for j in range(len(chunk))])
        for name, wav in zip(chunk, wavs):
            out = os.path.join(args.output_dir, os.path.splitext(name)[0] + ".wav")
            proc.write_wav(out, wav)
            print(f"{out}: {wav.size / args.sample_rate:.2f} s")


if __name__ == "__main__":
    main()
