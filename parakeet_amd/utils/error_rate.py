"""Error rates at word and character level with the interface of parakeet/utils/error_rate.py (``word_errors``,
``char_errors``, ``wer``, ``cer``: the same arguments, return values and ``ValueError`` texts), the Levenshtein distance taken
on the HIP engine (``parakeet_amd.alignment.edit_distance``, csrc/pk_edit.h) in place of that module's
Python double loop.  The string preparation is that module's: ``lower()`` under ``ignore_case``, ``filter(None,
split(delimiter))`` for words, the split-and-rejoin on ``' '`` for characters.

Beyond it: ``word_errors_batch`` / ``char_errors_batch`` score a corpus in one engine call, ``corpus_wer`` / ``corpus_cer``
are sum(distance) / sum(ref_len) (how the reference's G2P and text-normalisation recipes average), ``encode`` turns token
lists into the packed int32 ids the engine compares (host only)."""
import numpy as np

__all__ = ["word_errors", "char_errors", "wer", "cer", "word_errors_batch", "char_errors_batch", "corpus_wer", "corpus_cer",
           "encode", "split_words", "split_chars", "token_errors_batch", "format_confusions"]


def split_words(sentence, ignore_case=False, delimiter=" "):
    """The words ``word_errors`` compares."""
    if ignore_case:
        sentence = sentence.lower()
    return list(filter(None, sentence.split(delimiter)))


def split_chars(sentence, ignore_case=False, remove_space=False):
    """The characters ``char_errors`` compares: runs of spaces become one (or none), leading and trailing ones go."""
    if ignore_case:
        sentence = sentence.lower()
    return list(("" if remove_space else " ").join(filter(None, sentence.split(" "))))


def encode(ref_token_lists, hyp_token_lists):
    """Token lists -> ``(ref_ids, hyp_ids, ref_lens, hyp_lens)``: packed int32 ids (the pairs follow one another) and int32
    lengths.  One vocabulary per call: a single character is its code point, any other token (a word, a phone, any hashable)
    gets the next id below zero in order of first appearance, so that tokens are equal exactly when their ids are."""
    refs, hyps = [list(t) for t in ref_token_lists], [list(t) for t in hyp_token_lists]
    if len(refs) != len(hyps):
        raise ValueError(f"{len(refs)} references, {len(hyps)} hypotheses")
    vocab = {}

    def ids(tokens):
        out = np.empty(len(tokens), dtype=np.int32)
        for k, t in enumerate(tokens):
            if isinstance(t, str) and len(t) == 1:
                out[k] = ord(t)
            else:
                v = vocab.get(t)
                if v is None:
                    v = vocab[t] = -1 - len(vocab)
                out[k] = v
        return out
    r, h = [ids(t) for t in refs], [ids(t) for t in hyps]
    cat = lambda a: np.concatenate(a).astype(np.int32) if a else np.zeros(0, np.int32)  # noqa: E731
    return cat(r), cat(h), np.array([a.size for a in r], dtype=np.int32), np.array([a.size for a in h], dtype=np.int32)


def token_errors_batch(ref_token_lists, hyp_token_lists, return_alignments=False):
    """The distances of token lists (words, phones, characters: any hashable tokens) from one engine call, or several when
    the corpus exceeds the engine's batch -> ``(distances (B,) int64, ref_lens (B,) int64)`` and, with
    ``return_alignments``, the list of ``parakeet_amd.alignment.EditAlignment`` as a third item."""
    from ..alignment import EDIT_MAX_BATCH, edit_align, edit_distance
    refs, hyps = [list(t) for t in ref_token_lists], [list(t) for t in hyp_token_lists]
    if len(refs) != len(hyps):
        raise ValueError(f"{len(refs)} references, {len(hyps)} hypotheses")
    dist, als = [np.zeros(0, dtype=np.int64)], []
    for lo in range(0, len(refs), EDIT_MAX_BATCH):
        r, h, rl, hl = encode(refs[lo:lo + EDIT_MAX_BATCH], hyps[lo:lo + EDIT_MAX_BATCH])
        ro, ho = np.concatenate(([0], np.cumsum(rl))), np.concatenate(([0], np.cumsum(hl)))
        rs, hs = [r[ro[b]:ro[b + 1]] for b in range(rl.size)], [h[ho[b]:ho[b + 1]] for b in range(hl.size)]
        if return_alignments:
            got = edit_align(rs, hs)
            als += got
            dist.append(np.array([a.distance for a in got], dtype=np.int64))
        else:
            dist.append(np.asarray(edit_distance(rs, hs), dtype=np.int64))
    out = (np.concatenate(dist), np.array([len(r) for r in refs], dtype=np.int64))
    return out + (als,) if return_alignments else out


def _distances(ref_tokens, hyp_tokens):
    return token_errors_batch(ref_tokens, hyp_tokens)[0]


def word_errors_batch(references, hypotheses, ignore_case=False, delimiter=" "):
    """``word_errors`` of every pair from one engine call -> ``(distances (B,) float64, ref_lens (B,) int64)``."""
    refs = [split_words(s, ignore_case, delimiter) for s in references]
    hyps = [split_words(s, ignore_case, delimiter) for s in hypotheses]
    if len(refs) != len(hyps):
        raise ValueError(f"{len(refs)} references, {len(hyps)} hypotheses")
    return _distances(refs, hyps).astype(np.float64), np.array([len(r) for r in refs], dtype=np.int64)


def char_errors_batch(references, hypotheses, ignore_case=False, remove_space=False):
    """``char_errors`` of every pair from one engine call -> ``(distances (B,) float64, ref_lens (B,) int64)``."""
    refs = [split_chars(s, ignore_case, remove_space) for s in references]
    hyps = [split_chars(s, ignore_case, remove_space) for s in hypotheses]
    if len(refs) != len(hyps):
        raise ValueError(f"{len(refs)} references, {len(hyps)} hypotheses")
    return _distances(refs, hyps).astype(np.float64), np.array([len(r) for r in refs], dtype=np.int64)


def word_errors(reference, hypothesis, ignore_case=False, delimiter=" "):
    """Levenshtein distance in words and the number of words of the reference: ``(float, int)``."""
    d, n = word_errors_batch([reference], [hypothesis], ignore_case, delimiter)
    return float(d[0]), int(n[0])


def char_errors(reference, hypothesis, ignore_case=False, remove_space=False):
    """Levenshtein distance in characters and the length of the reference: ``(float, int)``."""
    d, n = char_errors_batch([reference], [hypothesis], ignore_case, remove_space)
    return float(d[0]), int(n[0])


def wer(reference, hypothesis, ignore_case=False, delimiter=" "):
    """Word error rate (Sw + Dw + Iw) / Nw; empty items of the split are dropped."""
    edit_distance, ref_len = word_errors(reference, hypothesis, ignore_case, delimiter)
    if ref_len == 0:
        raise ValueError("Reference's word number should be greater than 0.")
    return float(edit_distance) / ref_len


def cer(reference, hypothesis, ignore_case=False, remove_space=False):
    """Character error rate (Sc + Dc + Ic) / Nc; leading and trailing spaces go, runs of spaces count once."""
    edit_distance, ref_len = char_errors(reference, hypothesis, ignore_case, remove_space)
    if ref_len == 0:
        raise ValueError("Length of reference should be greater than 0.")
    return float(edit_distance) / ref_len


def _corpus(distances, ref_lens, what):
    total = int(np.sum(ref_lens))
    if total == 0:
        raise ValueError(what)
    return float(np.sum(distances)) / total


def format_confusions(conf, k):
    """The ``k`` most frequent substitutions, deletions and insertions of a ``parakeet_amd.alignment.Confusions`` as lines of
    text: ``count<TAB>ref -> hyp``, ``count<TAB>ref`` and ``count<TAB>hyp`` under a heading each (equal counts in the order
    the tokens sort)."""
    top = lambda c: sorted(c.items(), key=lambda kv: (-kv[1], str(kv[0])))[:k]   # noqa: E731
    lines = [f"substitutions ({sum(conf.substitutions.values())}):"]
    lines += [f"{n}\t{r} -> {h}" for (r, h), n in top(conf.substitutions)]
    lines += [f"deletions ({sum(conf.deletions.values())}):"] + [f"{n}\t{t}" for t, n in top(conf.deletions)]
    lines += [f"insertions ({sum(conf.insertions.values())}):"] + [f"{n}\t{t}" for t, n in top(conf.insertions)]
    return lines


def corpus_wer(references, hypotheses, ignore_case=False, delimiter=" "):
    """sum of the word distances / sum of the references' word counts over the corpus."""
    return _corpus(*word_errors_batch(references, hypotheses, ignore_case, delimiter), "Reference's word number should be greater than 0.")


def corpus_cer(references, hypotheses, ignore_case=False, remove_space=False):
    """sum of the character distances / sum of the references' lengths over the corpus."""
    return _corpus(*char_errors_batch(references, hypotheses, ignore_case, remove_space), "Length of reference should be greater than 0.")
