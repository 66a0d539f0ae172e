#!/usr/bin/env python
"""Copy synthesis with Parallel WaveGAN on the MI355X engine -- the counterpart of the reference's
examples/GANVocoder/parallelwave_gan/baker/synthesize_from_wav.py (same arguments; ``--device`` and ``--verbose`` are
accepted and ignored): every wav file of ``--input-dir`` is loaded at the model's rate, its log-mel spectrogram is
extracted, normalised with the vocoder's statistics and vocoded again; ``<output-dir>/gen_<name>`` is the result.

    wav (any rate, PCM or float) -> load_wav(sr=config.fs) -> LogMelFBank -> ZScore -> PWGGenerator -> gen_<name>

The reference loads with ``librosa.load(path, sr=config.fs)``; here a file at another rate goes through the engine's own
polyphase resampler (parakeet_amd.audio.Resample), which is not librosa's filter.  The files are taken in
sorted order and the whole directory runs as ONE ragged batch through each stage (the reference loops file by file).
``--output-sr`` delivers the result at another rate than the model's (resampled on the engine before it is encoded);
``--seed`` seeds the vocoder's noise stream.

``--config`` needs ``fs, n_fft, n_shift, win_length, window, n_mels, fmin, fmax`` and ``generator_params``
(examples/GANVocoder/parallelwave_gan/baker/conf/default.yaml).
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from parakeet_amd import checkpoint  # noqa: E402
from parakeet_amd.audio import LogMelFBank, load_wav, write_wav  # noqa: E402


def evaluate(args):
    """Returns {file name: (T,) float32 waveform at the model's rate} after writing the files."""
    config = checkpoint._config(args.config)
    pwg_inference = checkpoint.load_pwg(args.config, args.checkpoint, args.stat)
    print("model done!")
    fs = int(config["fs"])
    mel_extractor = LogMelFBank(sr=fs, n_fft=config["n_fft"], hop_length=config["n_shift"],
                                win_length=config.get("win_length"), window=config.get("window", "hann"),
                                n_mels=config["n_mels"], fmin=config.get("fmin"), fmax=config.get("fmax"))
    names = sorted(f for f in os.listdir(args.input_dir) if f.lower().endswith(".wav"))
    if not names:
        raise SystemExit(f"no .wav file in {args.input_dir}")
    t0 = time.time()
    wavs = [load_wav(os.path.join(args.input_dir, n), sr=fs)[0] for n in names]
    mels = mel_extractor.get_log_mel_fbank_batch(wavs)
    gen = pwg_inference.bind()
    gen.set_seed(getattr(args, "seed", 0) or 0)
    outs = [o.cpu().numpy()[:, 0] for o in gen.inference_batch(mels, normalize=True)]
    dt = time.time() - t0
    os.makedirs(args.output_dir, exist_ok=True)
    out_sr = int(getattr(args, "output_sr", None) or fs)
    for n, w in zip(names, outs):
        write_wav(os.path.join(args.output_dir, "gen_" + n), w, out_sr, source_samplerate=fs)
        print(f"{n} done!")
    total = sum(w.size for w in outs)
    print(f"{len(names)} utterances, {total} samples at {fs} Hz, time: {dt:.3f}s, RTF: {dt / (total / fs):.5f}.")
    return dict(zip(names, outs))


def main():
    parser = argparse.ArgumentParser(description="Synthesize with parallel wavegan.")
    parser.add_argument("--config", type=str, required=True, help="the recipe's yaml.")
    parser.add_argument("--checkpoint", type=str, required=True, help="snapshot to load.")
    parser.add_argument("--stat", type=str, required=True,
                        help="mean and standard deviation used to normalize spectrogram when training parallel wavegan.")
    parser.add_argument("--input-dir", type=str, required=True, help="input dir of wavs.")
    parser.add_argument("--output-dir", type=str, required=True, help="output dir.")
    parser.add_argument("--device", type=str, default="gpu", help="ignored: the engine is the GPU")
    parser.add_argument("--verbose", type=int, default=1, help="ignored")
    parser.add_argument("--output-sr", type=int, default=None, help="rate of the files written (default: the model's)")
    parser.add_argument("--seed", type=int, default=0, help="seed of the vocoder's noise")
    evaluate(parser.parse_args())


if __name__ == "__main__":
    main()
