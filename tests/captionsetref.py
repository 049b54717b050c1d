"""Float64 restatement of the caption-SET diversity metrics of ssc_runtime.evaluation (ssc_eval_set), on token lists, with no
device code and no code of the runtime: mBLEU-1..4, Self-CIDEr and Unique as DESIGN.md 7e defines them.

A token is any hashable value.  `df` maps an n-gram (a tuple of tokens) to the number of evaluated images whose references hold
it; a candidate token that no reference holds simply never occurs in it."""
import math
from collections import Counter

import numpy as np

TINY, SMALL = 1e-15, 1e-9
EIG_CUT = 1e-6


def ngrams(toks):
    c = Counter()
    for k in range(1, 5):
        for i in range(len(toks) - k + 1):
            c[tuple(toks[i:i + k])] += 1
    return c


def reference_df(refs):
    """refs: per evaluated image, its reference token lists -> (df Counter, number of images)."""
    df = Counter()
    for rs in refs:
        seen = set()
        for r in rs:
            seen.update(ngrams(r))
        for g in seen:
            df[g] += 1
    return df, len(refs)


def set_stats(caps):
    """(N, 10): testlen, reflen ("closest"), guess[4], correct[4] of every caption against the other captions of its image."""
    grams = [ngrams(c) for c in caps]
    out = np.zeros((len(caps), 10), dtype=np.int64)
    for i, c in enumerate(caps):
        others = [j for j in range(len(caps)) if j != i]
        testlen = len(c)
        reflen = min((abs(len(caps[j]) - testlen), len(caps[j])) for j in others)[1]
        correct = [0] * 4
        for g, tf in grams[i].items():
            correct[len(g) - 1] += min(tf, max(grams[j].get(g, 0) for j in others))
        out[i] = [testlen, reflen] + [max(0, testlen - k) for k in range(4)] + correct
    return out


def corpus_bleu(testlen, reflen, guess, correct):
    out, b = [], 1.0
    for k in range(4):
        b *= (float(correct[k]) + TINY) / (float(guess[k]) + SMALL)
        out.append(b ** (1.0 / (k + 1)))
    ratio = (testlen + TINY) / (reflen + SMALL)
    if ratio < 1:
        out = [x * math.exp(1 - 1 / ratio) for x in out]
    return out


def mbleu(stats):
    """stats (P, N, 10) -> mBLEU-1..4: corpus BLEU of the statistics summed over the images at sample index n, averaged over n."""
    stats = np.asarray(stats)
    per = [corpus_bleu(stats[:, n, 0].sum(), stats[:, n, 1].sum(), stats[:, n, 2:6].sum(0), stats[:, n, 6:10].sum(0))
           for n in range(stats.shape[1])]
    return [float(np.mean([b[k] for b in per])) for k in range(4)]


def kernel_matrix(caps, df, n_images):
    """K_ij = 1/4 sum_n cos(g_i^n, g_j^n), g = tf (log I - log max(1, df)); a cosine with a zero vector is 0."""
    log_i = math.log(float(n_images))
    vecs = []
    for c in caps:
        v = [{} for _ in range(4)]
        for g, tf in ngrams(c).items():
            v[len(g) - 1][g] = float(tf) * (log_i - math.log(max(1.0, float(df.get(g, 0)))))
        vecs.append((v, [math.sqrt(sum(w * w for w in v[k].values())) for k in range(4)]))
    N = len(caps)
    K = np.zeros((N, N))
    for i in range(N):
        for j in range(N):
            tot = 0.0
            for k in range(4):
                ni, nj = vecs[i][1][k], vecs[j][1][k]
                if ni != 0 and nj != 0:
                    dot = sum(w * vecs[j][0][k].get(g, 0.0) for g, w in vecs[i][0][k].items())
                    tot += dot / (ni * nj)
            K[i, j] = tot / 4.0
    return K


def eigenvalues(K):
    return np.linalg.eigvalsh(np.asarray(K, dtype=np.float64))[::-1].copy()


def self_cider(lam):
    """(value, degenerate) from the eigenvalues of one image's kernel matrix, descending."""
    lam = np.sort(np.asarray(lam, dtype=np.float64))[::-1]
    top = lam[0]
    if not top > 0:
        return 0.0, True
    kept = np.where(lam < EIG_CUT * top, 0.0, lam)
    r = math.sqrt(top) / float(np.sum(np.sqrt(kept)))
    return -math.log(r) / math.log(len(lam)), False


def near_cut(lam):
    """True when an eigenvalue lies within a factor 10 of the cut-off: two solvers may then keep different eigenvalues."""
    lam = np.asarray(lam, dtype=np.float64)
    top = lam.max()
    return bool(top > 0 and np.any((lam > 1e-7 * top) & (lam < 1e-5 * top)))


def distinct(caps):
    return len(set(tuple(c) for c in caps))


def evaluate(images, refs=None, scored=None):
    """images: per prediction image, N caption token lists.  refs: per EVALUATED image its reference token lists; scored: the
    indices into `images` of the evaluated images, in the order of refs.  Returns (per-image dict, summary dict)."""
    N = len(images[0])
    stats = np.stack([set_stats(c) for c in images])
    dist = np.array([distinct(c) for c in images], dtype=np.int64)
    s = {f"mBLEU-{k + 1}": v for k, v in enumerate(mbleu(stats))}
    per = {"set_stats": stats, "distinct": dist, "kernel": {}, "eigenvalues": {}, "self_cider": {}, "degenerate": 0}
    if refs:
        df, n_images = reference_df(refs)
        for p in scored:
            K = kernel_matrix(images[p], df, n_images)
            lam = eigenvalues(K)
            v, deg = self_cider(lam)
            per["kernel"][p], per["eigenvalues"][p], per["self_cider"][p] = K, lam, v
            per["degenerate"] += deg
        s["self-cider"] = float(np.mean([per["self_cider"][p] for p in scored]))
    s["unique"] = float(np.mean(dist / float(N)))
    return per, s
