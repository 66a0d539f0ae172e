#!/usr/bin/env python
"""Normalise dumped raw features with statistics files -- the reference's examples/fastspeech2/normalize.py (:28-176):

    python examples/normalize.py --metadata dump/train/raw/metadata.jsonl --dumpdir dump/train/norm \
        --speech-stats dump/train/speech_stats.npy [--pitch-stats ...] [--energy-stats ...] \
        [--phones-dict phone_id_map.txt] [--speaker-dict speaker_id_map.txt]

Every record's ``speech`` (or ``feats``) array, and its ``pitch`` / ``energy`` arrays when their statistics are given, is
written as ``(x - mean) / scale`` in float32 under ``<dumpdir>/data_<kind>/<utt_id>_<kind>.npy``, and ``<dumpdir>/metadata.jsonl``
lists the records sorted by ``utt_id`` with absolute paths.  ``--pitch-stats`` and ``--energy-stats`` are optional, so the
script also serves the SpeedySpeech, TransformerTTS and vocoder recipes, which normalise ``speech`` / ``feats`` only.  With
``--phones-dict`` the record's ``phones`` become the ids ``text``, with ``--speaker-dict`` its ``speaker`` becomes ``spk_id``,
as in the reference.  The arithmetic is ``ZScore.forward``: a float32 subtraction and a float32 division, the bits of
``StandardScaler.transform`` on float32 input.
"""
import argparse
import json
import os
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _id_map(path):
    if path is None:
        return None
    with open(path, "rt", encoding="utf-8") as f:
        return {k: int(v) for k, v in (line.split() for line in f if line.strip())}


def normalize(args):
    from parakeet_amd.normalizer import ZScore
    dumpdir = Path(args.dumpdir).expanduser().resolve()
    dumpdir.mkdir(parents=True, exist_ok=True)
    meta_dir = Path(args.metadata).parent
    with open(args.metadata, "rt", encoding="utf-8") as f:
        metadata = [json.loads(line) for line in f if line.strip()]
    scalers = {kind: ZScore.from_stats(path) for kind, path in
               (("speech", args.speech_stats), ("pitch", args.pitch_stats), ("energy", args.energy_stats)) if path is not None}
    phones, speakers = _id_map(args.phones_dict), _id_map(args.speaker_dict)
    records = []
    for item in metadata:
        rec = dict(item)
        utt = item["utt_id"]
        for kind, z in scalers.items():
            keys = [k for k in (("speech", "feats") if kind == "speech" else (kind,)) if k in item]
            if not keys:
                if kind == "speech":
                    raise SystemExit(f"{utt}: the record has neither 'speech' nor 'feats'")
                raise SystemExit(f"{utt}: --{kind}-stats given, but the record has no '{kind}'")
            src = Path(item[keys[0]])
            x = np.load(src if src.is_absolute() else meta_dir / src, allow_pickle=False)
            y = np.asarray(z.forward(x.astype(np.float32)), dtype=np.float32)
            sub = dumpdir / f"data_{kind}"
            sub.mkdir(parents=True, exist_ok=True)
            dst = sub / f"{utt}_{kind}.npy"
            np.save(dst, y, allow_pickle=False)
            for k in keys:
                rec[k] = str(dst)
        if phones is not None:
            rec["text"] = [phones[p] for p in rec.pop("phones")]
        if speakers is not None:
            rec["spk_id"] = speakers[rec.pop("speaker")]
        records.append(rec)
    records.sort(key=lambda r: r["utt_id"])
    with open(dumpdir / "metadata.jsonl", "wt", encoding="utf-8") as f:
        for rec in records:
            f.write(json.dumps(rec) + "\n")
    if args.verbose > 0:
        print(f"{len(records)} records -> {dumpdir / 'metadata.jsonl'}")
    return records


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="Normalize dumped raw features.")
    ap.add_argument("--metadata", type=str, required=True, help="metadata.jsonl of the raw features")
    ap.add_argument("--dumpdir", type=str, required=True, help="directory to dump normalized feature files")
    ap.add_argument("--speech-stats", type=str, required=True, help="speech statistics file")
    ap.add_argument("--pitch-stats", type=str, default=None, help="pitch statistics file")
    ap.add_argument("--energy-stats", type=str, default=None, help="energy statistics file")
    ap.add_argument("--phones-dict", type=str, default=None, help="phone vocabulary file")
    ap.add_argument("--speaker-dict", type=str, default=None, help="speaker id map file")
    ap.add_argument("--verbose", type=int, default=1)
    return ap.parse_args(argv)


def main(argv=None):
    return normalize(parse_args(argv))


if __name__ == "__main__":
    main()
