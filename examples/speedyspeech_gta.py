#!/usr/bin/env python
"""Ground-truth-aligned (GTA) mel spectrograms of a SpeedySpeech checkpoint on the MI355X engine: every utterance of a
normalised corpus goes through ``forward(text, tones, durations)`` with its own durations
(parakeet/models/speedyspeech/speedyspeech.py:166-184), each utterance as if it were alone, in length-sorted ragged batches of
one encode and one decode each (``SpeedySpeech.teacher_forced_batch``).  The result is what the hop-300 vocoder SpeedySpeech
is paired with is fine-tuned on to learn the acoustic model's errors.

Arguments: those of the reference's examples/speedyspeech/baker/synthesize.py (the ``--pwg-*`` ones are accepted and unused:
no waveform is made here).  ``--test-metadata`` is the ``metadata.jsonl`` its normalize.py writes, one JSON object per line:
``utt_id``, ``phones`` and ``tones`` (symbols, mapped through ``--phones-dict`` / ``--tones-dict``; or ids under ``text`` /
``tone_ids``), ``durations`` (frames per phone) and ``feats`` (path of the normalised (L, n_mels) .npy mel).  For each
utterance the script writes ``<utt_id>_gta.npy`` (sum(durations), n_mels), in the normalised space, or de-normalised with
``--denormalize``.  With ``--score`` it prints the four numbers of SpeedySpeechEvaluator.evaluate_core
(speedyspeech_updater.py:110-157: l1_loss, ssim_loss, duration_loss, loss) per utterance, each utterance scored as a batch of
one against its ``feats``, and their means over the corpus.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NAMES = ("l1_loss", "ssim_loss", "duration_loss", "loss")


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--speedyspeech-config", required=True)
    ap.add_argument("--speedyspeech-checkpoint", required=True)
    ap.add_argument("--speedyspeech-stat", required=True)
    ap.add_argument("--pwg-config", default=None, help="unused (no waveform is made)")
    ap.add_argument("--pwg-checkpoint", default=None, help="unused")
    ap.add_argument("--pwg-stat", default=None, help="unused")
    ap.add_argument("--phones-dict", required=True)
    ap.add_argument("--tones-dict", required=True)
    ap.add_argument("--test-metadata", required=True, help="metadata.jsonl of examples/speedyspeech/baker/normalize.py")
    ap.add_argument("--output-dir", required=True)
    ap.add_argument("--device", default="gpu")
    ap.add_argument("--verbose", type=int, default=1)
    ap.add_argument("--batch-size", type=int, default=32, help="utterances per teacher-forced pass")
    ap.add_argument("--denormalize", action="store_true", help="write log-mels (ZScore.inverse applied)")
    ap.add_argument("--score", action="store_true", help="print the evaluator's four numbers per utterance and over the corpus")
    return ap.parse_args(argv)


def read_metadata(path, phone_id_map, tone_id_map):
    """The jsonl file as a list of dicts(utt_id, text, tones, durations int64 (T,), feats path or None); relative paths are
    taken relative to the metadata file."""
    base = os.path.dirname(os.path.abspath(path))
    items = []
    with open(path, "rt", encoding="utf-8") as f:
        for line in f:
            line = line.strip()
            if not line:
                continue
            d = json.loads(line)
            text = d["text"] if "text" in d else [phone_id_map[p] for p in d["phones"]]
            tones = d["tone_ids"] if "tone_ids" in d else [tone_id_map[str(t)] for t in d["tones"]]
            feats = d.get("feats")
            if feats is not None and not os.path.isabs(str(feats)):
                feats = os.path.join(base, str(feats))
            items.append(dict(utt_id=str(d["utt_id"]), text=np.asarray(text, np.int64).reshape(-1),
                              tones=np.asarray(tones, np.int64).reshape(-1),
                              durations=np.asarray(d["durations"], np.int64).reshape(-1), feats=feats))
    return items


def main(argv=None):
    args = parse_args(argv)
    from parakeet_amd import checkpoint
    inf, phone_id_map, tone_id_map = checkpoint.load_speedyspeech(args.speedyspeech_config, args.speedyspeech_checkpoint,
                                                                  args.speedyspeech_stat, args.phones_dict, args.tones_dict)
    am = inf.bind()
    items = read_metadata(args.test_metadata, phone_id_map, tone_id_map)
    os.makedirs(args.output_dir, exist_ok=True)
    order = sorted(range(len(items)), key=lambda i: len(items[i]["text"]))     # batches of similar length
    bs, done = max(1, args.batch_size), 0
    totals = np.zeros(4)
    for i0 in range(0, len(order), bs):
        chunk = [items[i] for i in order[i0:i0 + bs]]
        texts, tones, durs = ([it[k] for it in chunk] for k in ("text", "tones", "durations"))
        mels = am.teacher_forced_batch(texts, durs, tones, denormalize=args.denormalize)
        for it, mel in zip(chunk, mels):
            np.save(os.path.join(args.output_dir, f"{it['utt_id']}_gta.npy"), mel.cpu().numpy())
        if args.score:
            for it in chunk:
                if it["feats"] is None:
                    raise ValueError(f"{it['utt_id']}: --score needs 'feats'")
            for it, s in zip(chunk, am.evaluate_per_utterance(texts, durs, [np.load(it["feats"]) for it in chunk], tones)):
                print(it["utt_id"], ", ".join(f"{k}: {s[k]:.6f}" for k in NAMES))
                totals += [s[k] for k in NAMES]
        done += len(chunk)
        if args.verbose:
            print(f"{done}/{len(items)} utterances")
    if args.score and items:
        print("corpus mean", ", ".join(f"{k}: {v:.6f}" for k, v in zip(NAMES, totals / len(items))))


if __name__ == "__main__":
    main()
