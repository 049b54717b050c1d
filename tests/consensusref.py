"""Float64 restatement of consensus re-ranking (ssc_runtime.evaluation.ConsensusBank), with no device code, written from the
definition: cosine similarities of pooled feature rows, the k nearest bank rows (similarity descending, ties to the lower bank row,
an optional excluded row per query), CIDEr-D of every candidate against the pooled captions of those rows with the BANK's document
frequencies, and the pick / stable order by that score.  The CIDEr pieces are those of captionevalref."""
import numpy as np

import captionevalref as R


def cosine(queries, bank):
    """(Q, M) float64: <q / |q|, b / |b|>; a zero row has similarity 0 to everything."""
    def unit(x):
        x = np.asarray(x, dtype=np.float64)
        n = np.sqrt((x * x).sum(1, keepdims=True))
        return np.where(n > 0, x / np.where(n > 0, n, 1.0), 0.0)
    return unit(queries) @ unit(bank).T


def neighbours(sims, k, exclude=None):
    """(Q, k) bank rows by similarity, descending, ties to the lower row; exclude[p] (a bank row or -1) is skipped; -1 fills the
    slots a small bank leaves."""
    sims = np.asarray(sims, dtype=np.float64)
    Q, M = sims.shape
    out = np.full((Q, k), -1, dtype=np.int64)
    for p in range(Q):
        rows = [j for j in np.argsort(-sims[p], kind="stable") if exclude is None or j != exclude[p]][:k]
        out[p, :len(rows)] = rows
    return out


def pooled_scores(cider, cands, pool):
    """C(p, c) of one query: CIDEr-D x 10 of every candidate with `pool` (token lists) as its reference list."""
    return np.array([cider.score(c, pool) for c in cands], dtype=np.float64)


def rerank(bank_refs, cands, nb):
    """bank_refs: per bank image its reference token lists; cands: per query N candidate token lists; nb (P, k) bank rows or -1.
    -> scores (P, N), pool_refs (P,), pick (P,), order (P, N)."""
    cider = R.Cider(bank_refs)
    P, N = len(cands), len(cands[0])
    scores = np.zeros((P, N))
    pool_refs = np.zeros(P, dtype=np.int64)
    for p in range(P):
        pool = [r for j in nb[p] if j >= 0 for r in bank_refs[j]]
        pool_refs[p] = len(pool)
        scores[p] = pooled_scores(cider, cands[p], pool)
    order = np.argsort(-scores, axis=1, kind="stable")
    return scores, pool_refs, order[:, 0].copy(), order
