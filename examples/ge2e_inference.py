#!/usr/bin/env python
"""GE2E utterance embeddings for a corpus on the MI355X engine -- the counterpart of the reference's
examples/ge2e/inference.py (same arguments; ``--device`` is accepted and ignored).

Every file matching ``--pattern`` under ``--input`` becomes ``<output>/<same relative path>.npy`` holding its (256,)
embedding, the conditions Tacotron2-aishell3 is trained on.  As in the reference (:81), the partials overlap by
``min_pad_coverage`` (0.75 with the released config), not by ``partial_overlap_ratio``.  The corpus goes through the
engine in batches of ``--batch`` utterances, each ONE ``embed_utterances`` call (the reference embeds file by file).

``--config`` is a YAML file with ``data`` / ``model`` sections overriding examples/ge2e/config.py's defaults; ``--opts``
takes ``KEY VALUE`` pairs such as ``data.n_mels 40``.  Files: PCM or float WAV; other rates are resampled with
scipy.signal.resample_poly on the host (``--resampler scipy``, the default) or by the engine's polyphase kernel
(``--resampler engine``); neither is librosa's resampler.  Silence trimming is skipped by default (no webrtcvad), as the reference
does without that package; ``--vad energy`` runs the reference's ``trim_long_silences`` on the engine behind this project's
energy detector (NOT webrtcvad: ``parakeet_amd.audio.trim_long_silences``).
"""
import argparse
import ast
import os
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from parakeet_amd import checkpoint  # noqa: E402
from parakeet_amd.ge2e_audio import SpeakerVerificationPreprocessor  # noqa: E402

DEFAULTS = {  # examples/ge2e/config.py
    "data": dict(audio_norm_target_dBFS=-30, sampling_rate=16000, vad_window_length=30, vad_moving_average_width=8,
                 vad_max_silence_length=6, mel_window_length=25, mel_window_step=10, n_mels=40, partial_n_frames=160,
                 min_pad_coverage=0.75, partial_overlap_ratio=0.5),
    "model": dict(num_layers=3, hidden_size=256, embedding_size=256),
}


def load_config(path, opts):
    cfg = {k: dict(v) for k, v in DEFAULTS.items()}
    if path:
        import yaml
        with open(path, "rt") as f:
            for sec, vals in (yaml.safe_load(f) or {}).items():
                cfg.setdefault(sec, {}).update(vals or {})
    opts = opts or []
    if len(opts) % 2:
        raise ValueError("--opts takes KEY VALUE pairs")
    for key, val in zip(opts[::2], opts[1::2]):
        sec, name = key.split(".", 1)
        try:
            val = ast.literal_eval(val)
        except (ValueError, SyntaxError):
            pass
        cfg.setdefault(sec, {})[name] = val
    return cfg


def main():
    ap = argparse.ArgumentParser(description="compute utterance embed.")
    ap.add_argument("--config", metavar="FILE", help="yaml overriding the default config")
    ap.add_argument("--input", type=str, required=True, help="path of the audio_file folder.")
    ap.add_argument("--pattern", type=str, default="*.wav", help="pattern to filter audio files.")
    ap.add_argument("--output", metavar="OUTPUT_DIR", required=True, help="where the .npy embeddings go.")
    ap.add_argument("--checkpoint_path", type=str, required=True, help="checkpoint path without .pdparams")
    ap.add_argument("--device", type=str, choices=["cpu", "gpu"], default="gpu", help="ignored: the engine is the GPU")
    ap.add_argument("--batch", type=int, default=1024, help="utterances per engine call")
    ap.add_argument("--resampler", choices=["scipy", "engine"], default="scipy", help="what resamples files at other rates")
    ap.add_argument("--vad", choices=["none", "energy"], default="none",
                    help="trim long silences before the partials are cut: 'energy' is the engine's energy detector, not webrtcvad")
    ap.add_argument("--opts", nargs=argparse.REMAINDER, help="KEY VALUE pairs overriding --config and the defaults")
    args = ap.parse_args()
    cfg = load_config(args.config, args.opts)
    c, m = cfg["data"], cfg["model"]
    model = checkpoint.load_ge2e(args.checkpoint_path, c["n_mels"], m["num_layers"], m["hidden_size"],
                                 m["embedding_size"])
    print(f"Loaded encoder {args.checkpoint_path}")
    processor = SpeakerVerificationPreprocessor(
        sampling_rate=c["sampling_rate"], audio_norm_target_dBFS=c["audio_norm_target_dBFS"],
        vad_window_length=c["vad_window_length"], vad_moving_average_width=c["vad_moving_average_width"],
        vad_max_silence_length=c["vad_max_silence_length"], mel_window_length=c["mel_window_length"],
        mel_window_step=c["mel_window_step"], n_mels=c["n_mels"], partial_n_frames=c["partial_n_frames"],
        min_pad_coverage=c["min_pad_coverage"], partial_overlap_ratio=c["min_pad_coverage"],   # sic: inference.py:81
        resampler=args.resampler, vad=None if args.vad == "none" else args.vad)
    input_dir = Path(args.input).expanduser()
    output_dir = Path(args.output).expanduser()
    ifpaths = sorted(input_dir.rglob(args.pattern))
    print(f"{len(ifpaths)} utterances in total")
    output_dir.mkdir(parents=True, exist_ok=True)
    for i in range(0, len(ifpaths), args.batch):
        chunk = ifpaths[i:i + args.batch]
        wavs = [processor.preprocess_wav(p) for p in chunk]
        embeds = model.embed_utterances(processor.extract_mel_partials_batch(wavs)).cpu().numpy()
        for p, e in zip(chunk, embeds):
            ofpath = (output_dir / p.relative_to(input_dir)).with_suffix(".npy")
            ofpath.parent.mkdir(parents=True, exist_ok=True)
            np.save(ofpath, e)
        print(f"{min(i + args.batch, len(ifpaths))} / {len(ifpaths)}")


if __name__ == "__main__":
    main()
