#!/usr/bin/env python
"""Ground-truth-aligned (GTA) mel spectrograms of a Tacotron2 checkpoint on the MI355X engine: every utterance of a corpus
goes through Tacotron2.forward's teacher-forced decoder (parakeet/models/tacotron2.py:691-778, eval semantics), in ragged
batches of one lockstep pass each (``teacher_forced_batch``).

``--metadata`` is a jsonl file, one JSON object per line: ``utt_id``, ``text`` (phone ids), optionally ``tones`` (tone ids,
for a model with a tone embedding), ``mel`` (path of the (L, d_mels) .npy in the model's own mel domain, the one it was
trained on; relative paths are taken relative to the metadata file) and, for a model with ``d_global_condition``,
``global_condition`` (path of the (d_global_condition,) .npy, e.g. a GE2E speaker embedding).  For each utterance the script
writes ``<utt_id>_gta.npy`` (L, d_mels): mel_outputs_postnet, what a vocoder fine-tuned on GTA mels reads -- and, with
``--save-alignment``, ``<utt_id>_align.npy`` (L, T), the attention weights.  Prenet dropout stays on as in the reference;
``--seed`` + the utterance's index selects the engine's dropout stream.  With ``--score`` the script prints the numbers of
Tacotron2Loss (parakeet/models/tacotron2.py:886-982: mel_loss, post_mel_loss, loss and, with ``--guided-attention`` /
for a model with a stop token, guided_attn_loss / stop_loss) per utterance, each utterance scored as a batch of one against
its ``mel`` with the dropout stream of its GTA mel, and their means over the corpus.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--tacotron2-config", required=True, help="yaml with the model / data sections of examples/tacotron2/config.py")
    ap.add_argument("--tacotron2-checkpoint", required=True, help="checkpoint path without the .pdparams suffix")
    ap.add_argument("--metadata", required=True)
    ap.add_argument("--output-dir", required=True)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--batch-size", type=int, default=32, help="utterances per teacher-forced pass")
    ap.add_argument("--save-alignment", action="store_true", help="also write <utt_id>_align.npy")
    ap.add_argument("--score", action="store_true", help="print Tacotron2Loss's numbers per utterance and over the corpus")
    ap.add_argument("--guided-attention", action="store_true", help="--score: add the guided attention loss")
    ap.add_argument("--sigma", type=float, default=0.2, help="--score: sigma of the guided attention loss")
    return ap.parse_args(argv)


def read_metadata(path):
    """The jsonl file as a list of dicts: utt_id, text (int64), tones (int64 or None), mel (path), global_condition (path or
    None)."""
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
                              tones=None if d.get("tones") is None else np.asarray(d["tones"], dtype=np.int64).reshape(-1),
                              mel=full(d["mel"]), global_condition=full(d.get("global_condition"))))
    return items


def run(model, items, output_dir, seed=0, batch_size=32, save_alignment=False, score=False, guided_attention=False, sigma=0.2):
    os.makedirs(output_dir, exist_ok=True)
    n = max(1, batch_size)
    totals = {}
    for i0 in range(0, len(items), n):
        chunk = items[i0:i0 + n]
        mels = [np.load(it["mel"]).astype(np.float32) for it in chunk]
        tones = [it["tones"] for it in chunk] if model.toned else None
        gc = None
        if model.d_global_condition:
            gc = np.stack([np.load(it["global_condition"]).astype(np.float32).reshape(-1) for it in chunk])
        seeds = [seed + i0 + k for k in range(len(chunk))]
        outs = model.teacher_forced_batch([it["text"] for it in chunk], mels, tones=tones, seeds=seeds, global_condition=gc)
        for it, o in zip(chunk, outs):
            np.save(os.path.join(output_dir, f"{it['utt_id']}_gta.npy"), o["mel_outputs_postnet"].cpu().numpy())
            if save_alignment:
                np.save(os.path.join(output_dir, f"{it['utt_id']}_align.npy"), o["alignments"].cpu().numpy())
        if score:
            scores = model.evaluate_per_utterance([it["text"] for it in chunk], mels, tones=tones, seeds=seeds,
                                                  global_condition=gc, use_stop_token_loss=model.use_stop_token,
                                                  use_guided_attention_loss=guided_attention, sigma=sigma)
            for it, sc in zip(chunk, scores):
                print(it["utt_id"], ", ".join(f"{k}: {v:.6f}" for k, v in sc.items()))
                for k, v in sc.items():
                    totals[k] = totals.get(k, 0.0) + v
        print(f"{min(i0 + len(chunk), len(items))}/{len(items)} utterances")
    if score and items:
        print("corpus mean", ", ".join(f"{k}: {v / len(items):.6f}" for k, v in totals.items()))


def main(argv=None):
    args = parse_args(argv)
    from parakeet_amd import checkpoint
    model = checkpoint.load_tacotron2(args.tacotron2_config, args.tacotron2_checkpoint)
    run(model, read_metadata(args.metadata), args.output_dir, args.seed, args.batch_size, args.save_alignment, args.score,
        args.guided_attention, args.sigma)


if __name__ == "__main__":
    main()
