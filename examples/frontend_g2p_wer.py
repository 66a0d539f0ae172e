#!/usr/bin/env python
"""Phone error rate of the Mandarin frontend against a corpus's labels -- the counterpart of the reference's
examples/text_frontend/test_g2p.py with the same arguments, files and final line, the distances taken on the MI355X engine
as ONE batch (``parakeet_amd.utils.error_rate``) in place of a Python double loop per sentence.

``--input-dir`` holds ``text`` (``utt_id sentence`` per line, baker's prosody marks allowed) and ``text.ref`` (``utt_id phones``
per line).  ``--output-dir`` receives ``text.g2p`` and ``text.ref.clean``: the predicted and the labelled phones without
silence tokens, ``phones(baker_utt_id)`` per line (the form sclite reads).  The last line printed is
``The avg WER of g2p is: <sum of distances / sum of label lengths>``.

The frontend's dictionaries are the caller's: ``--lexicon`` is a pinyin lexicon file (``word syl [syl ...] [#pos]``; the
package's demonstration lexicon by default), which is what this recipe measures.  ``--confusions K`` adds the K most
frequent substituted, deleted and inserted phones, ``--per-utterance FILE`` one ``utt_id distance ref_len S D I`` line per
utterance."""
import argparse
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SILENCE_TOKENS = {"sp", "sil", "sp1", "spl"}


def text_cleaner(raw_text):
    """baker's transcript -> what the frontend reads: prosody marks #1 ... #4, quotes and brackets go; the ellipsis before a
    full stop goes; colons, semicolons, dashes, ellipses and the enumeration comma become commas."""
    text = re.sub("#[1-4]|“|”|（|）", "", raw_text)
    text = text.replace("…。", "。")
    return re.sub("：|；|——|……|、|…|—", "，", text)


def read_table(path):
    """``key rest of the line`` per line -> dict in file order."""
    out = {}
    with open(path, "rt", encoding="utf-8") as f:
        for line in f:
            parts = line.strip().split(" ")
            out[parts[0]] = " ".join(parts[1:])
    return out


def write_reports(args, utt_ids, ref_tokens, hyp_tokens, distances, ref_lens, alignments):
    """``--per-utterance`` and ``--confusions`` -> the confusion report's lines (printed), or None."""
    from parakeet_amd.alignment import confusions
    from parakeet_amd.utils.error_rate import format_confusions
    if args.per_utterance:
        with open(args.per_utterance, "wt", encoding="utf-8") as f:
            for u, d, n, al in zip(utt_ids, distances, ref_lens, alignments):
                c = al.counts
                f.write(f"{u} {int(d)} {int(n)} {c.substitutions} {c.deletions} {c.insertions}\n")
    if args.confusions:
        lines = format_confusions(confusions(alignments, ref_tokens, hyp_tokens), args.confusions)
        print("\n".join(lines))
        return lines
    return None


def main(argv=None):
    ap = argparse.ArgumentParser(description="g2p example.")
    ap.add_argument("--input-dir", default="data/g2p", type=str, help="directory to preprocessed test data.")
    ap.add_argument("--output-dir", default="exp/g2p", type=str, help="directory to save g2p results.")
    ap.add_argument("--lexicon", default=None, help="pinyin lexicon for the Mandarin frontend")
    ap.add_argument("--phones-dict", default=None)
    ap.add_argument("--tones-dict", default=None)
    ap.add_argument("--confusions", type=int, default=0, metavar="K", help="print the K most frequent substitutions, deletions and insertions")
    ap.add_argument("--per-utterance", default=None, metavar="FILE", help="write 'utt_id distance ref_len S D I' per utterance")
    args = ap.parse_args(argv)
    from parakeet_amd.frontend import Frontend
    from parakeet_amd.utils.error_rate import token_errors_batch
    if not os.path.isdir(args.input_dir):
        raise SystemExit(f"{args.input_dir} is not a directory")
    os.makedirs(args.output_dir, exist_ok=True)
    raw, ref = read_table(os.path.join(args.input_dir, "text")), read_table(os.path.join(args.input_dir, "text.ref"))
    frontend = Frontend(phone_vocab_path=args.phones_dict, tone_vocab_path=args.tones_dict, lexicon=args.lexicon)

    utt_ids, ref_tokens, hyp_tokens = [], [], []
    with open(os.path.join(args.output_dir, "text.g2p"), "wt", encoding="utf-8") as wf_g2p, \
            open(os.path.join(args.output_dir, "text.ref.clean"), "wt", encoding="utf-8") as wf_ref:
        for utt_id, raw_text in raw.items():
            if utt_id not in ref:
                continue
            g2p = [p for p in sum(frontend.get_phonemes(text_cleaner(raw_text)), []) if p not in SILENCE_TOKENS]
            gt = [p for p in ref[utt_id].split(" ") if p not in SILENCE_TOKENS]
            wf_ref.write(" ".join(gt) + "(baker_" + utt_id + ")" + "\n")
            wf_g2p.write(" ".join(g2p) + "(baker_" + utt_id + ")" + "\n")
            utt_ids.append(utt_id)
            ref_tokens.append([p for p in gt if p])                # (what word_errors keeps of the joined string)
            hyp_tokens.append([p for p in g2p if p])
    if frontend.missing:
        print("not in the lexicon:", " ".join(sorted(set(frontend.missing))), file=sys.stderr)
    need = bool(args.confusions or args.per_utterance)
    got = token_errors_batch(ref_tokens, hyp_tokens, return_alignments=need)   # the whole corpus as one batch
    distances, ref_lens = got[0].astype(float), got[1]
    report = write_reports(args, utt_ids, ref_tokens, hyp_tokens, distances, ref_lens, got[2]) if need else None
    avg_wer = float(sum(distances.tolist())) / int(sum(ref_lens.tolist()))
    print("The avg WER of g2p is:", avg_wer)
    return dict(rate=avg_wer, utt_ids=utt_ids, distances=distances, ref_lens=ref_lens, report=report)


if __name__ == "__main__":
    main()
