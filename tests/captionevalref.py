"""Float64 restatement of the caption metrics of ssc_runtime.evaluation, on token lists, with no device code.

BLEU-1..4 (coco-caption BleuScorer, option "closest"), ROUGE-L (coco-caption Rouge, beta 1.2), CIDEr-D (coco-caption CiderScorer,
sigma 6, document frequencies over the evaluated images' references), the oracle / mean reductions of the reference's
eval/eval.py:276-472, its Div-n (:145-172) and its style precision / recall (:95-131).  A token is any hashable value; a candidate
token that must match nothing (the vocabulary's @@UNKNOWN@@) is given as a value no reference holds."""
import math
from collections import Counter

import numpy as np

TINY, SMALL = 1e-15, 1e-9
BETA2 = 1.2 * 1.2
SIGMA = 6.0


def ngram_counts(toks, n=4):
    c = Counter()
    for k in range(1, n + 1):
        for i in range(len(toks) - k + 1):
            c[tuple(toks[i:i + k])] += 1
    return c


def bleu_stats(cand, refs):
    """(testlen, reflen, guess[4], correct[4]) of one candidate (BleuScorer.cook_test with option 'closest')."""
    testlen = len(cand)
    reflen = min((abs(len(r) - testlen), len(r)) for r in refs)[1]
    maxref = {}
    for r in refs:
        for g, c in ngram_counts(r).items():
            maxref[g] = max(maxref.get(g, 0), c)
    guess = [max(0, testlen - k + 1) for k in range(1, 5)]
    correct = [0] * 4
    for g, c in ngram_counts(cand).items():
        correct[len(g) - 1] += min(maxref.get(g, 0), c)
    return testlen, reflen, guess, correct


def bleu_from_stats(testlen, reflen, guess, correct):
    out, b = [], 1.0
    for k in range(4):
        b *= (float(correct[k]) + TINY) / (float(guess[k]) + SMALL)
        out.append(b ** (1.0 / (k + 1)))
    ratio = (testlen + TINY) / (reflen + SMALL)
    if ratio < 1:
        out = [x * math.exp(1 - 1 / ratio) for x in out]
    return out


def lcs(a, b):
    prev = [0] * (len(b) + 1)
    for x in a:
        cur = [0]
        for j, y in enumerate(b):
            cur.append(prev[j] + 1 if x == y else max(prev[j + 1], cur[j]))
        prev = cur
    return prev[-1]


def rouge_l(cand, refs):
    if not cand:
        return 0.0
    P = max(lcs(cand, r) / float(len(cand)) for r in refs)
    Q = max(lcs(cand, r) / float(len(r)) for r in refs)
    if P != 0 and Q != 0:
        return ((1 + BETA2) * P * Q) / float(Q + BETA2 * P)
    return 0.0


class Cider:
    """CIDEr-D with the document frequencies of `refs` (one list of reference token lists per evaluated image)."""

    def __init__(self, refs):
        self.df = Counter()
        for rs in refs:
            for g in set(g for r in rs for g in ngram_counts(r)):
                self.df[g] += 1
        self.ref_len = math.log(float(len(refs)))
        self._cache = {}

    def vec(self, toks):
        v, norm = [{} for _ in range(4)], [0.0] * 4
        for g, tf in ngram_counts(toks).items():
            k = len(g) - 1
            w = float(tf) * (self.ref_len - math.log(max(1.0, self.df.get(g, 0))))
            v[k][g] = w
            norm[k] += w * w
        return v, [math.sqrt(x) for x in norm], max(0, len(toks) - 1)

    def score(self, cand, refs):
        vc, nc, lc = self.vec(cand)
        total = [0.0] * 4
        for r in refs:
            key = tuple(r)
            if key not in self._cache:
                self._cache[key] = self.vec(r)
            vr, nr, lr = self._cache[key]
            delta = float(lc - lr)
            for k in range(4):
                val = 0.0
                for g, w in vc[k].items():
                    wr = vr[k].get(g, 0.0)
                    val += min(w, wr) * wr
                if nc[k] != 0 and nr[k] != 0:
                    val /= nc[k] * nr[k]
                val *= math.exp(-(delta ** 2) / (2 * SIGMA ** 2))
                total[k] += val
        return float(np.mean(total)) / len(refs) * 10.0


def div_counts(captions, n):
    """(distinct n-grams over the captions, total words) of one image."""
    grams = set()
    words = 0
    for c in captions:
        words += len(c)
        grams.update(tuple(c[i:i + n]) for i in range(len(c) - n + 1))
    return len(grams), words


def div_n(images, n):
    """eval.py n_gram_diversity over lists of captions per image; an image whose captions are all empty scores 0."""
    tot = 0.0
    for caps in images:
        d, w = div_counts(caps, n)
        tot += d / w if w else 0.0
    return tot / len(images)


def top5(cider_row):
    """The 5 sample indices of highest CIDEr, stable descending (ties: lower index first)."""
    return [int(i) for i in np.argsort(-np.asarray(cider_row, dtype=np.float64), kind="stable")[:5]]


def style_counts(ref_caps, cand_caps, style_words):
    """(candidate style tokens, matched, reference style tokens) of one image (eval.py eval_style)."""
    rs = set(t for c in ref_caps for t in c if t in style_words)
    cs = set(t for c in cand_caps for t in c if t in style_words)
    return len(cs), len(cs & rs), len(rs)


def evaluate(cands, refs, style_words=None, div_only=()):
    """cands: per evaluated image, N candidate token lists; refs: per evaluated image, its reference token lists.
    div_only: candidates (N token lists each) of prediction images without references - they count toward Div-1 / Div-2 only.
    Returns (per-candidate dict of (I, N) arrays, summary dict with eval.py's printed names)."""
    I, N = len(cands), len(cands[0])
    assert all(len(c) == N for c in cands)
    cid = Cider(refs)
    B = np.zeros((I, N, 4))
    R = np.zeros((I, N))
    C = np.zeros((I, N))
    stats = np.zeros((I, N, 10), dtype=np.int64)
    for i in range(I):
        for n in range(N):
            t, rl, g, c = bleu_stats(cands[i][n], refs[i])
            stats[i, n] = [t, rl] + g + c
            B[i, n] = bleu_from_stats(t, rl, g, c)
            R[i, n] = rouge_l(cands[i][n], refs[i])
            C[i, n] = cid.score(cands[i][n], refs[i])
    s = {}
    all_imgs = [list(c) for c in cands] + [list(c) for c in div_only]
    s["Div-1"] = div_n(all_imgs, 1)
    s["Div-2"] = div_n(all_imgs, 2)
    rows = np.arange(I)
    oracle = {}
    for k in range(4):
        best = np.argmax(B[:, :, k], axis=1)
        oracle[f"B{k + 1}"] = best
        sel = stats[rows, best]
        s[f"B{k + 1}"] = bleu_from_stats(sel[:, 0].sum(), sel[:, 1].sum(), sel[:, 2:6].sum(0), sel[:, 6:10].sum(0))[k]
    for k in range(4):
        s[f"mean B{k + 1}"] = float(np.mean([bleu_from_stats(stats[:, n, 0].sum(), stats[:, n, 1].sum(), stats[:, n, 2:6].sum(0),
                                                             stats[:, n, 6:10].sum(0))[k] for n in range(N)]))
    oracle["rouge"] = np.argmax(R, axis=1)
    oracle["cider"] = np.argmax(C, axis=1)
    s["rouge"] = float(np.mean(R.max(1)))
    s["mean rouge"] = float(np.mean(R.mean(0)))
    s["cider"] = float(np.mean(C.max(1)))
    s["mean cider"] = float(np.mean(C.mean(0)))
    t5 = np.array([top5(C[i]) for i in range(I)], dtype=np.int64) if N >= 5 else None
    if t5 is not None:
        sel = [[cands[i][n] for n in t5[i]] for i in range(I)]
        s["top5 Div-1"] = div_n(sel, 1)
        s["top5 Div-2"] = div_n(sel, 2)
    if style_words is not None:
        st = np.array([style_counts(refs[i], cands[i], style_words) for i in range(I)])
        s["senti_prec"] = st[:, 1].sum() / st[:, 0].sum() if st[:, 0].sum() else float("nan")
        s["senti_rec"] = st[:, 1].sum() / st[:, 2].sum() if st[:, 2].sum() else float("nan")
        s["has_anp"] = float(np.mean(st[:, 0] > 0))
    per = {"bleu": B, "rouge": R, "cider": C, "stats": stats, "oracle": oracle, "top5": t5}
    return per, s
