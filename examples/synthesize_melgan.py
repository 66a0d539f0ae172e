#!/usr/bin/env python
"""MelGAN / multi-band MelGAN synthesis on the MI355X engine: mel files -> wav, or text -> FastSpeech2 -> (MB-)MelGAN.

  synthesize_melgan.py vocoder --config C --checkpoint P [--stat S] --test-metadata M --output-dir D
      the arguments of synthesize_vocoder.py's parallel_wavegan: a jsonlines file of {"utt_id", "feats": path.npy} records,
      (T, n_mels) each.  Without --stat the features are taken as already normalised; with it they are raw log-mels and the
      vocoder's statistics are applied on the device.
  synthesize_melgan.py e2e --fastspeech2-config ... --melgan-config C --melgan-checkpoint P --melgan-stat S --text T ...
      the arguments of synthesize_e2e.py with --pwg-* renamed --melgan-*.

The checkpoint is a snapshot archive with a ``generator_params`` entry and the config a yaml with a ``generator_params``
section (and, for multi-band MelGAN, optionally ``pqmf_params``), as for Parallel WaveGAN.  With ``out_channels`` > 1 the
sub-bands are merged by the PQMF bank on the device; ``pqmf.*`` entries of the archive are ignored.  The parameter names the
engine expects and the layout (parakeet_amd/melgan.py) could not be checked against a released checkpoint; a checkpoint with
other names fails at the first synthesis with the name it misses.  All utterances are synthesised as ONE ragged batch; an
utterance shorter than the generator's ``min_frames`` (4 for the defaults) is refused.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from parakeet_amd import checkpoint  # noqa: E402
from parakeet_amd.audio import write_wav  # noqa: E402


def vocoder(args):
    stat = args.stat
    cfg = checkpoint._config(args.config)
    if stat is None:   # already normalised features: identity statistics
        import tempfile
        n = cfg["generator_params"].get("in_channels", 80)
        stat = os.path.join(tempfile.mkdtemp(), "identity.npy")
        np.save(stat, np.stack([np.zeros(n), np.ones(n)]).astype(np.float32))
    voc = checkpoint.load_melgan(args.config, args.checkpoint, stat)
    with open(args.test_metadata, "rt") as f:
        meta = [json.loads(line) for line in f if line.strip()]
    base = os.path.dirname(os.path.abspath(args.test_metadata))
    mels = [np.load(m["feats"] if os.path.isabs(m["feats"]) else os.path.join(base, m["feats"])).astype(np.float32) for m in meta]
    t0 = time.time()
    wavs = [w.numpy()[:, 0] for w in voc.inference_batch(mels)]
    dt = time.time() - t0
    os.makedirs(args.output_dir, exist_ok=True)
    n = 0
    for m, w in zip(meta, wavs):
        write_wav(os.path.join(args.output_dir, m["utt_id"] + ".wav"), w, cfg["fs"])
        n += w.size
    print(f"{len(meta)} utterances, {n} samples, time: {dt:.3f}s, Hz: {n / dt:.0f}, RTF: {cfg['fs'] / (n / dt):.5f}.")


def e2e(args):
    from parakeet_amd.frontend import English, phones_to_ids
    from parakeet_amd.frontend.phone_map import RECIPE_PUNC as PUNC
    from parakeet_amd.synthesize import Synthesizer
    am, phone_id_map = checkpoint.load_fastspeech2(args.fastspeech2_config, args.fastspeech2_checkpoint,
                                                   args.fastspeech2_stat, args.phones_dict)
    voc = checkpoint.load_melgan(args.melgan_config, args.melgan_checkpoint, args.melgan_stat)
    fs = checkpoint._config(args.fastspeech2_config)["fs"]
    frontend = None if args.phones_input else English(lexicon=args.lexicon)
    utt_ids, batch = [], []
    with open(args.text, "rt") as f:
        for line in f:
            parts = line.strip().split()
            if not parts:
                continue
            if frontend is None:
                ids = phones_to_ids(parts[1:], phone_id_map, PUNC, strip_start_end=False)
            else:
                ids = phones_to_ids(frontend.phoneticize(" ".join(parts[1:])), phone_id_map, PUNC)
                if frontend.backend.oov:
                    print(f"{parts[0]}: not in the lexicon, pronounced by rule: {frontend.backend.oov}", file=sys.stderr)
            utt_ids.append(parts[0])
            batch.append([int(i) for i in ids])
    os.makedirs(args.output_dir, exist_ok=True)
    t0 = time.perf_counter()
    wavs = Synthesizer(am, voc).synthesize_batch(batch)
    n = 0
    for utt_id, wav in zip(utt_ids, wavs):
        w = wav.numpy()
        n += w.shape[0]
        write_wav(os.path.join(args.output_dir, utt_id + ".wav"), w, fs)
        print(f"{utt_id} done!")
    dt = time.perf_counter() - t0
    print(f"{len(wavs)} utterances, {n / fs:.2f} s of audio in {dt:.3f} s ({n / fs / dt:.1f}x real time, incl. first-call setup)")


def main():
    ap = argparse.ArgumentParser(description="Synthesize with MelGAN / multi-band MelGAN from mel files, or from text through FastSpeech2.")
    sub = ap.add_subparsers(dest="mode", required=True)
    v = sub.add_parser("vocoder", help="mel spectrogram files -> wav")
    v.add_argument("--config", required=True)
    v.add_argument("--checkpoint", required=True)
    v.add_argument("--stat", default=None, help="the vocoder's statistics: the features are raw log-mels")
    v.add_argument("--test-metadata", required=True)
    v.add_argument("--output-dir", required=True)
    e = sub.add_parser("e2e", help="text -> FastSpeech2 -> (multi-band) MelGAN")
    e.add_argument("--fastspeech2-config", required=True)
    e.add_argument("--fastspeech2-checkpoint", required=True)
    e.add_argument("--fastspeech2-stat", required=True)
    e.add_argument("--melgan-config", required=True)
    e.add_argument("--melgan-checkpoint", required=True)
    e.add_argument("--melgan-stat", required=True)
    e.add_argument("--phones-dict", default="phone_id_map.txt")
    e.add_argument("--text", required=True, help="'utt_id sentence' per line")
    e.add_argument("--lexicon", default=None, help="CMUdict-format pronunciation lexicon for the English frontend")
    e.add_argument("--phones-input", action="store_true", help="--text holds 'utt_id PH1 PH2 ...' lines")
    e.add_argument("--output-dir", required=True)
    args = ap.parse_args()
    (vocoder if args.mode == "vocoder" else e2e)(args)


if __name__ == "__main__":
    main()
