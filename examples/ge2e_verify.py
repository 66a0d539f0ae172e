#!/usr/bin/env python
"""GE2E loss and equal error rate of a speaker encoder on held-out speakers, on the MI355X engine -- the numbers the
reference's trainer prints per batch (examples/ge2e/train.py:70-87: ``loss: {:>.6f} err: {:>.6f}``), without a trainer.

``--input`` is a directory of speaker sub-directories holding mel ``.npy`` files of shape (frames, n_mels) -- the layout
examples/ge2e/preprocess.py writes -- or ``.wav`` files, which go through the engine's front end (volume, power mel).
Batches are drawn as examples/ge2e/speaker_verification_dataset.py:75-105 draws them: N speakers from a shuffled cycle
over all speakers, M utterances of each from a shuffled cycle over the speaker's utterances, a random clip of
``partial_n_frames`` frames of each; seeded by ``--seed``.  Utterances shorter than a clip are left out.

By default a batch is scored as (N, M, embedding_size) (``evaluate_batch``).  ``--literal`` selects the reference's
``forward``, whose reshape makes the last axis N instead (parakeet/models/lstm_speaker_encoder.py:36).
"""
import argparse
import os
import random
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from parakeet_amd import checkpoint  # noqa: E402
from parakeet_amd.ge2e_audio import ge2e_preprocessor  # noqa: E402


def random_cycle(items, rng):
    """examples/ge2e/random_cycle.py: once in the given order, then reshuffled passes for ever"""
    saved = list(items)
    for it in saved:
        yield it
    while saved:
        rng.shuffle(saved)
        for it in saved:
            yield it


def main():
    ap = argparse.ArgumentParser(description="GE2E loss and EER of seeded N x M batches")
    ap.add_argument("--input", required=True, help="directory of speaker sub-directories of .npy mels or .wav files")
    ap.add_argument("--checkpoint_path", required=True, help="checkpoint path, with or without .pdparams")
    ap.add_argument("--speakers_per_batch", type=int, default=64)
    ap.add_argument("--utterances_per_speaker", type=int, default=10)
    ap.add_argument("--partial_n_frames", type=int, default=160)
    ap.add_argument("--batches", type=int, default=10)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--literal", action="store_true", help="the reference's forward(), reshape([N, -1, N]) included")
    args = ap.parse_args()
    N, M, F = args.speakers_per_batch, args.utterances_per_speaker, args.partial_n_frames
    model = checkpoint.load_ge2e(args.checkpoint_path)
    model.eval()
    pre = None
    mels = {}

    def mel_of(path):
        nonlocal pre
        if path not in mels:
            if path.suffix == ".npy":
                mels[path] = np.load(path).astype(np.float32)
            else:
                pre = pre or ge2e_preprocessor()
                mels[path] = pre.melspectrogram(pre.preprocess_wav(path)).cpu().numpy()
        return mels[path]

    root = Path(args.input).expanduser()
    speakers = {}
    for d in sorted(p for p in root.glob("*") if p.is_dir()):
        files = sorted(list(d.glob("*.npy")) + list(d.glob("*.wav")))
        files = [f for f in files if mel_of(f).shape[0] >= F]
        if files:
            speakers[d] = files
    if len(speakers) < 2:
        raise SystemExit(f"{root}: fewer than 2 speakers with an utterance of {F} frames")
    print(f"{len(speakers)} speakers, {sum(len(v) for v in speakers.values())} utterances")
    rng = random.Random(args.seed)
    speaker_gen = random_cycle(list(speakers), rng)
    utt_gen = {s: random_cycle(us, rng) for s, us in speakers.items()}
    losses, eers = [], []
    for i in range(args.batches):
        clips = []
        for s in [next(speaker_gen) for _ in range(N)]:
            for _ in range(M):
                mel = mel_of(next(utt_gen[s]))
                start = rng.randint(0, mel.shape[0] - F)
                clips.append(mel[start:start + F])
        batch = np.stack(clips)
        if args.literal:
            loss, eer = model(batch, N)
        else:
            out = model.evaluate_batch(batch, N)
            loss, eer = out["loss"], out["eer"]
        losses.append(float(loss))
        eers.append(eer)
        print("step: {}, loss: {:>.6f} err: {:>.6f}".format(i, losses[-1], eer))
    print("mean loss: {:>.6f} err: {:>.6f}".format(float(np.mean(losses)), float(np.mean(eers))))


if __name__ == "__main__":
    main()
