#!/usr/bin/env python
"""Ground-truth-aligned (GTA) mel spectrograms of a TransformerTTS checkpoint on the MI355X engine: every utterance of a
normalised corpus goes through TransformerTTS.inference(text, speech=mel, use_teacher_forcing=True)
(parakeet/models/transformer_tts/transformer_tts.py:567-579), in ragged batches of one parallel decoder pass each.

Arguments: the TransformerTTS half of examples/synthesize_ar.py plus ``--test-metadata``, the ``norm/metadata.jsonl``
written by the reference's examples/transformer_tts/normalize.py (one JSON object per line: ``utt_id``, ``text`` (phone
ids) and ``speech`` (path of the normalised (L, n_mels) .npy)).  For each utterance the script writes
``<utt_id>_gta.npy`` ((L // r) * r, n_mels) in the normalised space (the space a vocoder fine-tuned on GTA mels reads
after its own normalisation) and, with ``--save-attention``, ``<utt_id>_att.npy`` (dlayers, aheads, L // r, T + 1), the
encoder-decoder attention weights.  Prenet dropout stays on as in the reference; ``--seed`` + the utterance's index
selects the engine's dropout stream.  With ``--score`` the script prints the numbers of
TransformerTTSEvaluator.evaluate_core (transformer_tts_updater.py:222-322: bce_loss, l1_loss, l2_loss, enc_dec_attn_loss,
encoder_alpha, decoder_alpha, loss) per utterance, each utterance scored as a batch of one against its ``speech`` with the
dropout stream of its GTA mel, and their means over the corpus; ``--loss-type``, ``--bce-pos-weight``,
``--guided-attn-loss-sigma`` and ``--guided-attn-loss-lambda`` are the evaluator's options, ``--no-guided-attn-loss`` leaves
the attention term out (a model with reduction_factor > 1 needs it).
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--transformer-tts-config", required=True)
    ap.add_argument("--transformer-tts-checkpoint", required=True)
    ap.add_argument("--transformer-tts-stat", required=True)
    ap.add_argument("--phones-dict", default="phone_id_map.txt")
    ap.add_argument("--test-metadata", required=True, help="norm/metadata.jsonl of examples/transformer_tts/normalize.py")
    ap.add_argument("--output-dir", required=True)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--batch-size", type=int, default=32, help="utterances per teacher-forced pass")
    ap.add_argument("--save-attention", action="store_true", help="also write <utt_id>_att.npy")
    ap.add_argument("--score", action="store_true", help="print the evaluator's numbers per utterance and over the corpus")
    ap.add_argument("--loss-type", default="L1", choices=("L1", "L2", "L1+L2"))
    ap.add_argument("--bce-pos-weight", type=float, default=5.0)
    ap.add_argument("--no-guided-attn-loss", action="store_true")
    ap.add_argument("--guided-attn-loss-sigma", type=float, default=0.4)
    ap.add_argument("--guided-attn-loss-lambda", type=float, default=1.0)
    return ap.parse_args(argv)


def read_metadata(path):
    """The jsonl file as a list of (utt_id, phone ids (int64), speech path); relative speech paths are taken relative to
    the metadata file, as normalize.py writes them."""
    base = os.path.dirname(os.path.abspath(path))
    items = []
    with open(path, "rt", encoding="utf-8") as f:
        for line in f:
            line = line.strip()
            if not line:
                continue
            d = json.loads(line)
            sp = str(d["speech"])
            items.append((str(d["utt_id"]), np.asarray(d["text"], dtype=np.int64).reshape(-1),
                          sp if os.path.isabs(sp) else os.path.join(base, sp)))
    return items


def main(argv=None):
    args = parse_args(argv)
    from parakeet_amd import checkpoint
    inf, _ = checkpoint.load_transformer_tts(args.transformer_tts_config, args.transformer_tts_checkpoint,
                                             args.transformer_tts_stat, args.phones_dict)
    am = inf.acoustic_model
    items = read_metadata(args.test_metadata)
    os.makedirs(args.output_dir, exist_ok=True)
    totals = {}
    for i0 in range(0, len(items), max(1, args.batch_size)):
        chunk = items[i0:i0 + max(1, args.batch_size)]
        speech = [np.load(p).astype(np.float32) for _, _, p in chunk]
        seeds = [args.seed + i0 + k for k in range(len(chunk))]
        outs = am.teacher_forced_batch([t for _, t, _ in chunk], speech, seeds=seeds, return_att=args.save_attention)
        for (utt_id, _, _), (mel, att) in zip(chunk, outs):
            np.save(os.path.join(args.output_dir, f"{utt_id}_gta.npy"), mel.cpu().numpy())
            if att is not None:
                np.save(os.path.join(args.output_dir, f"{utt_id}_att.npy"), att.cpu().numpy())
        if args.score:
            scores = am.evaluate_per_utterance([t for _, t, _ in chunk], speech, seeds=seeds, bce_pos_weight=args.bce_pos_weight,
                                               loss_type=args.loss_type, use_guided_attn_loss=not args.no_guided_attn_loss,
                                               guided_attn_loss_sigma=args.guided_attn_loss_sigma,
                                               guided_attn_loss_lambda=args.guided_attn_loss_lambda)
            for (utt_id, _, _), sc in zip(chunk, scores):
                print(utt_id, ", ".join(f"{k}: {v:.6f}" for k, v in sc.items()))
                for k, v in sc.items():
                    totals[k] = totals.get(k, 0.0) + v
        print(f"{min(i0 + len(chunk), len(items))}/{len(items)} utterances")
    if args.score and items:
        print("corpus mean", ", ".join(f"{k}: {v / len(items):.6f}" for k, v in totals.items()))


if __name__ == "__main__":
    main()
