#!/usr/bin/env python
"""Character error rate of the Mandarin text normaliser against a corpus's normalised text -- the counterpart of the
reference's examples/text_frontend/test_textnorm.py with the same arguments, files and final line, the distances taken on
the MI355X engine as ONE batch (``parakeet_amd.utils.error_rate``).

``--input-dir`` holds ``text`` (``text_id raw sentence`` per line) and ``text.ref`` (``text_id normalised sentence``).
``--output-dir`` receives ``text.tn`` and ``text.ref.clean``: the normaliser's output and the label, Latin letters removed and a
space between the characters, ``c h a r s(text_id)`` per line.  The last line printed is
``The avg CER of text normalization is: <sum of distances / sum of label lengths>`` (the spaces between characters count, as
they do in the reference's ``char_errors``).

``--lexicon``, ``--phones-dict`` and ``--tones-dict`` are accepted as in the G2P recipe (the normaliser itself reads no
dictionary).  ``--confusions K`` adds the K most frequent substituted, deleted and inserted characters, ``--per-utterance
FILE`` one ``text_id distance ref_len S D I`` line per sentence."""
import argparse
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from frontend_g2p_wer import read_table, write_reports  # noqa: E402


def del_en_add_space(text):
    """Latin letters go, a space stands between the characters left: "你好aBC" -> "你 好"."""
    return " ".join(re.sub("[a-zA-Z]", "", text)).strip()


def main(argv=None):
    ap = argparse.ArgumentParser(description="text normalization example.")
    ap.add_argument("--input-dir", default="data/textnorm", type=str, help="directory to preprocessed test data.")
    ap.add_argument("--output-dir", default="exp/textnorm", type=str, help="directory to save textnorm results.")
    ap.add_argument("--lexicon", default=None, help="accepted for symmetry with the G2P recipe; the normaliser reads no dictionary")
    ap.add_argument("--phones-dict", default=None)
    ap.add_argument("--tones-dict", default=None)
    ap.add_argument("--confusions", type=int, default=0, metavar="K", help="print the K most frequent substitutions, deletions and insertions")
    ap.add_argument("--per-utterance", default=None, metavar="FILE", help="write 'text_id distance ref_len S D I' per sentence")
    args = ap.parse_args(argv)
    from parakeet_amd.frontend import TextNormalizer
    from parakeet_amd.utils.error_rate import split_chars, token_errors_batch
    if not os.path.isdir(args.input_dir):
        raise SystemExit(f"{args.input_dir} is not a directory")
    os.makedirs(args.output_dir, exist_ok=True)
    raw, ref = read_table(os.path.join(args.input_dir, "text")), read_table(os.path.join(args.input_dir, "text.ref"))
    normalizer = TextNormalizer()

    ids, ref_tokens, hyp_tokens = [], [], []
    with open(os.path.join(args.output_dir, "text.ref.clean"), "wt", encoding="utf-8") as wf_ref, \
            open(os.path.join(args.output_dir, "text.tn"), "wt", encoding="utf-8") as wf_tn:
        for text_id, raw_text in raw.items():
            if text_id not in ref:
                continue
            gt = del_en_add_space(ref[text_id])
            tn = del_en_add_space(normalizer.normalize_sentence(raw_text))
            wf_ref.write(gt + "(" + text_id + ")" + "\n")
            wf_tn.write(tn + "(" + text_id + ")" + "\n")
            ids.append(text_id)
            ref_tokens.append(split_chars(gt))                     # (what char_errors compares)
            hyp_tokens.append(split_chars(tn))
    need = bool(args.confusions or args.per_utterance)
    got = token_errors_batch(ref_tokens, hyp_tokens, return_alignments=need)   # the whole corpus as one batch
    distances, ref_lens = got[0].astype(float), got[1]
    report = write_reports(args, ids, ref_tokens, hyp_tokens, distances, ref_lens, got[2]) if need else None
    avg_cer = float(sum(distances.tolist())) / int(sum(ref_lens.tolist()))
    print("The avg CER of text normalization is:", avg_cer)
    return dict(rate=avg_cer, utt_ids=ids, distances=distances, ref_lens=ref_lens, report=report)


if __name__ == "__main__":
    main()
