#!/usr/bin/env python
"""tests/golden/error_rate.json: what the REFERENCE's ``word_errors``, ``char_errors``, ``wer`` and ``cer``
(parakeet/utils/error_rate.py, imported through tools/ref_import.py; the module needs numpy alone) return on seeded cases.

The file holds data only: per case the function's name, the two input strings, the options, and the returned value (a
``[distance, ref_len]`` pair or a rate) or the text of the ``ValueError`` raised.  Cases: English and Mandarin sentences with
planted edits; mixed case with ``ignore_case`` both ways; runs of spaces, leading and trailing ones; ``remove_space`` both
ways; another ``delimiter``; an empty hypothesis; an empty reference; an identical pair; the pair of the module's own
``__main__``.  Token counts include 0, 1, 63, 64, 65 and about 130.
Needs the reference checkout.  Run from the repository root:  python tools/make_golden_error_rate.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_import  # noqa: E402

EN = ("the quick brown fox jumps over a lazy dog while seven wizards quietly judge every boxing match near Old Harbour "
      "and Nobody Asked why The river kept its silver secrets under Broken bridges").split()
ZH = "今天天气很好我们一起去公园散步然后回家吃晚饭明年春季他打算到北京学习中文和历史的课程"
MAIN_REF = ['j', 'iou4', 'zh', 'e4', 'iang5', 'x', 'v2', 'b', 'o1', 'k', 'ai1', 'sh', 'iii3', 'l', 'e5', 'b', 'ei3', 'p', 'iao1',
            'sh', 'eng1', 'ia2']
MAIN_HYP = ['j', 'iou4', 'zh', 'e4', 'iang4', 'x', 'v2', 'b', 'o1', 'k', 'ai1', 'sh', 'iii3', 'l', 'e5', 'b', 'ei3', 'p', 'iao1',
            'sh', 'eng1', 'ia2']


def edited(rng, tokens, pool, n_edits):
    out = list(tokens)
    for e in range(n_edits):
        kind = e % 3
        if kind == 0 and out:
            out[int(rng.integers(len(out)))] = pool[int(rng.integers(len(pool)))]
        elif kind == 1 and out:
            del out[int(rng.integers(len(out)))]
        else:
            out.insert(int(rng.integers(len(out) + 1)), pool[int(rng.integers(len(pool)))])
    return out


def cases():
    rng = np.random.default_rng(2021)
    pick = lambda pool, n: [pool[int(i)] for i in rng.integers(len(pool), size=n)]   # noqa: E731
    out = []

    def add(fn, ref, hyp, **kw):
        out.append(dict(fn=fn, reference=ref, hypothesis=hyp, kwargs=kw))
    for n in (0, 1, 2, 17, 63, 64, 65, 130):                       # English words, Mandarin characters, planted edits
        words = pick(EN, n)
        hyp = edited(rng, words, EN, max(1, n // 6))
        for fn in ("word_errors", "wer"):
            add(fn, " ".join(words), " ".join(hyp))
        chars = pick(ZH, n)
        hypc = edited(rng, chars, ZH, max(1, n // 5))
        for fn in ("char_errors", "cer"):
            add(fn, "".join(chars), "".join(hypc))
        add("word_errors", " ".join(chars), " ".join(hypc))         # characters as words: the form the G2P recipe scores
        add("char_errors", " ".join(chars), " ".join(hypc), remove_space=True)
        add("char_errors", " ".join(chars), " ".join(hypc), remove_space=False)
    mixed_ref, mixed_hyp = "The Quick brown FOX Jumps over a lazy Dog", "the quick Brown fox jumped over lazy dog"
    for ic in (False, True):
        for fn in ("word_errors", "wer", "char_errors", "cer"):
            add(fn, mixed_ref, mixed_hyp, ignore_case=ic)
    spaced_ref, spaced_hyp = "  the  quick   brown fox ", "the quick  brown  fix  "
    for fn in ("word_errors", "wer"):
        add(fn, spaced_ref, spaced_hyp)
    for rs in (False, True):
        for fn in ("char_errors", "cer"):
            add(fn, spaced_ref, spaced_hyp, remove_space=rs)
            add(fn, " 今天 天气  很好 ", "今天天气 不 好", remove_space=rs)
    for fn in ("word_errors", "wer"):
        add(fn, "a|b||c|d e|f", "a|b|c||x|f|", delimiter="|")
        add(fn, "a|b||c|d e|f", "a|b|c||x|f|")                      # the same strings, split on spaces
    for fn in ("word_errors", "wer", "char_errors", "cer"):
        add(fn, "nothing came back", "")                            # empty hypothesis
        add(fn, "", "something from nothing")                       # empty reference: the rates raise
        add(fn, "", "")
        add(fn, "   ", "x")
        add(fn, "exactly the same words", "exactly the same words")
        add(fn, " ".join(MAIN_REF), " ".join(MAIN_HYP))
    add("word_errors", " ".join(pick(EN, 131)), " ".join(pick(EN, 127)))    # unrelated long pairs
    add("char_errors", "".join(pick(ZH, 129)), "".join(pick(ZH, 133)))
    return out


def main():
    mod = ref_import.load("parakeet.utils.error_rate")
    recs = []
    for c in cases():
        rec = dict(c)
        try:
            v = getattr(mod, c["fn"])(c["reference"], c["hypothesis"], **c["kwargs"])
            rec["result"] = [float(v[0]), int(v[1])] if isinstance(v, tuple) else float(v)
        except ValueError as e:
            rec["error"] = str(e)
        recs.append(rec)
    path = os.path.join(ref_import.golden_dir(), "error_rate.json")
    with open(path, "wt", encoding="utf-8") as f:
        json.dump(dict(source="parakeet/utils/error_rate.py", cases=recs), f, ensure_ascii=False, indent=0)
        f.write("\n")
    print(path, len(recs), "cases", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
