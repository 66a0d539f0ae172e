#!/usr/bin/env python
"""Token durations of a corpus from a teacher's attention on the MI355X engine: every utterance goes through the
teacher-forced decoder of a Tacotron2 or TransformerTTS checkpoint in ragged batches, and the monotonic alignment search of
DESIGN.md 4.7 (``parakeet_amd.alignment``) turns each attention map into integer durations -- monotonic, every token at least
one frame, summing to the mel length.  The result is the ``durations.txt`` that examples/fastspeech2_features.py reads with
``--durations``.  These are the teacher's attention boundaries, NOT the Montreal Forced Aligner's forced alignment, which the
reference's recipe uses and which is not a dependency; nobody has compared the two on speech.

``--metadata`` is the jsonl file of examples/tacotron2_gta.py, one JSON object per line: ``utt_id``, ``text`` (token ids, one
per entry of ``phones``), ``phones`` (the names written to durations.txt), optionally ``speaker`` (default ``--speaker``),
``tones``, ``global_condition``, and ``mel`` (``speech`` is accepted too): the path of the (L, d_mels) .npy in the model's own
mel domain.  Written under ``--output-dir``: ``durations.txt`` (``utt|speaker|ph d ph d ...``, d in frames) and
``alignment_report.jsonl`` with ``utt_id``, ``frames``, ``tokens``, ``score_per_frame`` (the path's mean log attention per
decoder step) and ``focus_rate`` (FastSpeech 3.3; with TransformerTTS also the ``layer`` and ``head`` used), so that badly
aligned utterances can be dropped.  An utterance with more tokens than decoder steps has no alignment: it is reported with
``"skipped"`` and left out of durations.txt.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--tacotron2-config", help="yaml with the model / data sections of examples/tacotron2/config.py")
    ap.add_argument("--tacotron2-checkpoint", help="checkpoint path without the .pdparams suffix")
    ap.add_argument("--transformer-tts-config")
    ap.add_argument("--transformer-tts-checkpoint")
    ap.add_argument("--transformer-tts-stat")
    ap.add_argument("--phones-dict", default=None, help="TransformerTTS: phone_id_map.txt")
    ap.add_argument("--metadata", required=True)
    ap.add_argument("--output-dir", required=True)
    ap.add_argument("--speaker", default="spk0", help="speaker name of items without one")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--batch-size", type=int, default=32, help="utterances per teacher-forced pass")
    ap.add_argument("--map", default="focus", help='TransformerTTS: "focus" (the largest focus rate) or "layer,head"')
    return ap.parse_args(argv)


def read_metadata(path, speaker="spk0"):
    """The jsonl file as a list of dicts: utt_id, text (int64), phones (list of str), speaker, tones (int64 or None), mel
    (path), global_condition (path or None)."""
    base = os.path.dirname(os.path.abspath(path))

    def full(p):
        return None if p is None else (str(p) if os.path.isabs(str(p)) else os.path.join(base, str(p)))
    items = []
    with open(path, "rt", encoding="utf-8") as f:
        for line in f:
            line = line.strip()
            if not line:
                continue
            d = json.loads(line)
            items.append(dict(utt_id=str(d["utt_id"]), text=np.asarray(d["text"], dtype=np.int64).reshape(-1),
                              phones=[str(p) for p in d["phones"]], speaker=str(d.get("speaker", speaker)),
                              tones=None if d.get("tones") is None else np.asarray(d["tones"], dtype=np.int64).reshape(-1),
                              mel=full(d["mel"] if "mel" in d else d["speech"]), global_condition=full(d.get("global_condition"))))
    return items


def _is_transformer(model):
    from parakeet_amd.transformer_tts import TransformerTTS
    return isinstance(model, TransformerTTS)


def run(model, items, output_dir, seed=0, batch_size=32, map="focus"):
    """Teacher forcing and the search over ``items`` in batches of ``batch_size``; writes durations.txt and
    alignment_report.jsonl under ``output_dir`` and returns the report as a list of dicts."""
    from parakeet_amd.alignment import write_durations
    os.makedirs(output_dir, exist_ok=True)
    tts = _is_transformer(model)
    r = int(model.reduction_factor) if tts else 1
    for it in items:
        if len(it["phones"]) != len(it["text"]):
            raise ValueError(f"{it['utt_id']}: {len(it['phones'])} phones for {len(it['text'])} token ids")
    n = max(1, batch_size)
    report, kept, durs = [], [], []
    for i0 in range(0, len(items), n):
        chunk, mels, seeds = [], [], []
        for k, it in enumerate(items[i0:i0 + n]):
            mel = np.load(it["mel"]).astype(np.float32)
            steps, cols = mel.shape[0] // r, len(it["text"]) + (1 if tts else 0)
            if cols > steps:
                report.append(dict(utt_id=it["utt_id"], frames=int(steps * r), tokens=len(it["text"]),
                                   skipped=f"{cols} attention columns for {steps} decoder steps"))
                continue
            chunk.append(it)
            mels.append(mel)
            seeds.append(seed + i0 + k)
        if chunk:
            texts = [it["text"] for it in chunk]
            if tts:
                d, score, focus = model.durations_batch(texts, mels, seeds=seeds, map=map, return_focus=True)
                extra = [dict(layer=l, head=h) for l, h in model.last_maps]
            else:
                gc = None
                if model.d_global_condition:
                    gc = np.stack([np.load(it["global_condition"]).astype(np.float32).reshape(-1) for it in chunk])
                d, score, focus = model.durations_batch(texts, mels, tones=[it["tones"] for it in chunk] if model.toned else None,
                                                        seeds=seeds, global_condition=gc, return_focus=True)
                extra = [{} for _ in chunk]
            for it, mel, db, sb, fb, ex in zip(chunk, mels, d, score, focus, extra):
                steps = mel.shape[0] // r
                assert int(db.sum()) == steps * r and len(db) == len(it["phones"]), it["utt_id"]
                report.append(dict(utt_id=it["utt_id"], frames=int(steps * r), tokens=len(it["text"]),
                                   score_per_frame=float(sb) / steps, focus_rate=float(fb), **ex))
                kept.append(it)
                durs.append(db)
        print(f"{min(i0 + n, len(items))}/{len(items)} utterances")
    write_durations(os.path.join(output_dir, "durations.txt"), [it["utt_id"] for it in kept], [it["speaker"] for it in kept],
                    [it["phones"] for it in kept], durs)
    with open(os.path.join(output_dir, "alignment_report.jsonl"), "wt", encoding="utf-8") as f:
        for rec in report:
            f.write(json.dumps(rec) + "\n")
    return report


def main(argv=None):
    args = parse_args(argv)
    from parakeet_amd import checkpoint
    if bool(args.tacotron2_config) == bool(args.transformer_tts_config):
        raise SystemExit("give either --tacotron2-config / --tacotron2-checkpoint or the three --transformer-tts-* arguments")
    if args.tacotron2_config:
        model = checkpoint.load_tacotron2(args.tacotron2_config, args.tacotron2_checkpoint)
    else:
        inf, _ = checkpoint.load_transformer_tts(args.transformer_tts_config, args.transformer_tts_checkpoint,
                                                 args.transformer_tts_stat, args.phones_dict)
        model = inf.acoustic_model
    which = args.map if args.map == "focus" else tuple(int(v) for v in args.map.split(","))
    run(model, read_metadata(args.metadata, args.speaker), args.output_dir, args.seed, args.batch_size, which)


if __name__ == "__main__":
    main()
