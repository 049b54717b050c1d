"""g20_caption_eval.npz: Div-n and style precision / recall of a small diverse-caption corpus, computed by the reference's own
eval/eval.py functions (n_gram_diversity, generate_ngrams, get_n_words, eval_style).  eval.py is Python 2 and reads pickles at
import time, so the text of those four pure functions is taken from the file and executed alone, with word_tokenize = str.split
and an exact ngrams: the corpus has no punctuation and no clitics, so the stand-ins change nothing.  The top-5 Div-n is
n_gram_diversity over the 5 captions per image of highest CIDEr-D by tests/captionevalref.py (pycocoevalcap is not available
to compute CIDEr-D from the reference side).  The fixture holds only inputs (id arrays + word list) and outputs.

    python tests/golden/make_eval_golden.py /path/to/reference/eval/eval.py"""
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))


def reference_functions(path):
    text = open(path).read()
    ns = {"word_tokenize": str.split,
          "ngrams": lambda toks, n: [tuple(toks[i:i + n]) for i in range(len(toks) - n + 1)]}
    for name in ("generate_ngrams", "get_n_words", "n_gram_diversity", "eval_style"):
        m = re.search(r"^def %s\(.*?(?=^\S)" % name, text, flags=re.S | re.M)
        exec(compile(m.group(0), path + ":" + name, "exec"), ns)
    return ns


def corpus(seed=20):
    rng = np.random.default_rng(seed)
    words = [f"w{i}" for i in range(18)] + ["happy", "sad", "lovely", "ugly", "nice"]
    style_words = ["happy", "sad", "lovely", "ugly", "nice", "gloomy"]   # "gloomy": in the TSV, never in a caption
    V = len(words)
    I, N = 7, 6
    refs, cands = [], []
    for i in range(I):
        nr = int(rng.integers(1, 5))
        refs.append([list(rng.integers(0, V, int(rng.integers(1, 12)))) for _ in range(nr)])
        base = list(rng.integers(0, V, int(rng.integers(2, 10))))
        caps = []
        for n in range(N):
            if n % 3 == 1:
                caps.append(list(base))   # duplicate captions
            else:
                caps.append(list(rng.integers(0, 9 if i % 2 else V, int(rng.integers(1, 11)))))
        cands.append(caps)
    return words, style_words, refs, cands


def main():
    import captionevalref as R
    ref_path = sys.argv[1] if len(sys.argv) > 1 else "eval/eval.py"
    F = reference_functions(ref_path)
    words, style_words, refs, cands = corpus()
    I, N = len(cands), len(cands[0])
    s = lambda ids: " ".join(words[t] for t in ids)
    preds = [{"image_id": i, "caption": s(c)} for i in range(I) for c in cands[i]]
    div1 = F["n_gram_diversity"](preds, 1)
    div2 = F["n_gram_diversity"](preds, 2)
    tr = [[[words[t] for t in r] for r in rs] for rs in refs]
    tc = [[[words[t] for t in c] for c in cs] for cs in cands]
    per, _ = R.evaluate(tc, tr)
    top = [{"image_id": i, "caption": s(cands[i][n])} for i in range(I) for n in per["top5"][i]]
    t5d1 = F["n_gram_diversity"](top, 1)
    t5d2 = F["n_gram_diversity"](top, 2)
    gts = {i: [s(r) for r in refs[i]] for i in range(I)}
    res = [{i: [s(cands[i][n])] for i in range(I)} for n in range(N)]
    prec, rec, anp = F["eval_style"](gts, res, {"senti": style_words})
    L = max(len(c) for cs in cands for c in cs)
    cand_ids = np.full((I, N, L), -1, dtype=np.int32)
    for i in range(I):
        for n in range(N):
            cand_ids[i, n, :len(cands[i][n])] = cands[i][n]
    ref_tok = np.array([t for rs in refs for r in rs for t in r], dtype=np.int32)
    ref_len = np.array([len(r) for rs in refs for r in rs], dtype=np.int32)
    ref_count = np.array([len(rs) for rs in refs], dtype=np.int32)
    np.savez_compressed(os.path.join(HERE, "g20_caption_eval.npz"), words=np.array(words), style_words=np.array(style_words),
                        cand_ids=cand_ids, ref_tokens=ref_tok, ref_lengths=ref_len, ref_counts=ref_count,
                        div=np.array([div1, div2, t5d1, t5d2]), style=np.array([prec, rec, anp]),
                        top5=np.asarray(per["top5"], dtype=np.int32))
    print("div", div1, div2, "top5", t5d1, t5d2, "style", prec, rec, anp)


if __name__ == "__main__":
    main()
