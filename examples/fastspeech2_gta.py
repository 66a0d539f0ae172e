#!/usr/bin/env python
"""Ground-truth-aligned (GTA) mel spectrograms of a FastSpeech2 checkpoint on the MI355X engine: every utterance of a
normalised corpus goes through ``_forward(..., ds, ps, es, is_inference=False)`` with its own durations, pitch and energy
(parakeet/models/fastspeech2/fastspeech2.py:433-442), in length-sorted ragged batches of one encode and one decode each
(``FastSpeech2.teacher_forced_batch``).  The result is what a vocoder is fine-tuned on to learn the acoustic model's errors.

Arguments: those of the reference's examples/fastspeech2/synthesize.py (the ``--pwg-*`` ones are accepted and unused: no
waveform is made here).  ``--test-metadata`` is the ``metadata.jsonl`` its normalize.py writes, one JSON object per line:
``utt_id``, ``text`` (phone ids; or ``phones``, mapped through ``--phones-dict``), ``durations`` (frames per phone),
``pitch`` and ``energy`` (paths of the normalised token-averaged (T, 1) .npy files) and, for a multi-speaker model,
``spk_id``.  For each utterance the script writes ``<utt_id>_gta.npy`` (r * sum(durations), n_mels), in the normalised
space, or de-normalised with ``--denormalize``.  With ``--score`` every line also needs ``feats`` (path of the normalised
(L, n_mels) .npy mel) and the script prints the five numbers of FastSpeech2Evaluator.evaluate_core
(fastspeech2_updater.py:123-163: l1_loss, duration_loss, pitch_loss, energy_loss, loss) per utterance, each utterance scored
as a batch of one against its ``feats``, and their means over the corpus.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NAMES = ("l1_loss", "duration_loss", "pitch_loss", "energy_loss", "loss")


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--fastspeech2-config", required=True)
    ap.add_argument("--fastspeech2-checkpoint", required=True)
    ap.add_argument("--fastspeech2-stat", required=True)
    ap.add_argument("--pwg-config", default=None, help="unused (no waveform is made)")
    ap.add_argument("--pwg-checkpoint", default=None, help="unused")
    ap.add_argument("--pwg-stat", default=None, help="unused")
    ap.add_argument("--phones-dict", default=None)
    ap.add_argument("--speaker-dict", default=None, help="speaker id map of a multi-speaker model")
    ap.add_argument("--test-metadata", required=True, help="metadata.jsonl of examples/fastspeech2/normalize.py")
    ap.add_argument("--output-dir", required=True)
    ap.add_argument("--device", default="gpu")
    ap.add_argument("--verbose", type=int, default=1)
    ap.add_argument("--batch-size", type=int, default=32, help="utterances per teacher-forced pass")
    ap.add_argument("--denormalize", action="store_true", help="write log-mels (ZScore.inverse applied)")
    ap.add_argument("--score", action="store_true", help="print the evaluator's five numbers per utterance and over the corpus")
    return ap.parse_args(argv)


def read_metadata(path, phone_id_map=None):
    """The jsonl file as a list of dicts(utt_id, text int64 (T,), durations int64 (T,), pitch, energy (paths), spk_id or
    None); relative paths are taken relative to the metadata file."""
    base = os.path.dirname(os.path.abspath(path))

    def resolve(p):
        p = str(p)
        return p if os.path.isabs(p) else os.path.join(base, p)
    items = []
    with open(path, "rt", encoding="utf-8") as f:
        for line in f:
            line = line.strip()
            if not line:
                continue
            d = json.loads(line)
            if "text" in d:
                text = np.asarray(d["text"], dtype=np.int64).reshape(-1)
            else:
                if phone_id_map is None:
                    raise ValueError(f"{d['utt_id']}: 'phones' need --phones-dict")
                text = np.asarray([phone_id_map[p] for p in d["phones"]], dtype=np.int64)
            items.append(dict(utt_id=str(d["utt_id"]), text=text,
                              durations=np.asarray(d["durations"], dtype=np.int64).reshape(-1),
                              pitch=resolve(d["pitch"]), energy=resolve(d["energy"]), spk_id=d.get("spk_id"),
                              feats=None if d.get("feats") is None else resolve(d["feats"])))
    return items


def main(argv=None):
    args = parse_args(argv)
    from parakeet_amd import checkpoint
    inf, phone_id_map = checkpoint.load_fastspeech2(args.fastspeech2_config, args.fastspeech2_checkpoint,
                                                    args.fastspeech2_stat, args.phones_dict,
                                                    speaker_dict=args.speaker_dict)
    am = inf.bind()
    items = read_metadata(args.test_metadata, phone_id_map)
    os.makedirs(args.output_dir, exist_ok=True)
    order = sorted(range(len(items)), key=lambda i: len(items[i]["text"]))     # batches of similar length
    bs, done = max(1, args.batch_size), 0
    totals = np.zeros(len(NAMES))
    for i0 in range(0, len(order), bs):
        chunk = [items[i] for i in order[i0:i0 + bs]]
        spk = None
        if args.speaker_dict is not None and all(it["spk_id"] is not None for it in chunk):
            spk = np.asarray([it["spk_id"] for it in chunk], dtype=np.int64)
        texts, durs = [it["text"] for it in chunk], [it["durations"] for it in chunk]
        pitch, energy = [np.load(it["pitch"]) for it in chunk], [np.load(it["energy"]) for it in chunk]
        mels = am.teacher_forced_batch(texts, durs, pitch, energy, spk_ids=spk, denormalize=args.denormalize)
        for it, mel in zip(chunk, mels):
            np.save(os.path.join(args.output_dir, f"{it['utt_id']}_gta.npy"), mel.cpu().numpy())
        if args.score:
            for it in chunk:
                if it["feats"] is None:
                    raise ValueError(f"{it['utt_id']}: --score needs 'feats'")
            scores = am.evaluate_per_utterance(texts, durs, pitch, energy, [np.load(it["feats"]) for it in chunk], spk_ids=spk)
            for it, sc in zip(chunk, scores):
                print(it["utt_id"], ", ".join(f"{k}: {sc[k]:.6f}" for k in NAMES))
                totals += [sc[k] for k in NAMES]
        done += len(chunk)
        if args.verbose:
            print(f"{done}/{len(items)} utterances")
    if args.score and items:
        print("corpus mean", ", ".join(f"{k}: {v:.6f}" for k, v in zip(NAMES, totals / len(items))))


if __name__ == "__main__":
    main()
