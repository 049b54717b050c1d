"""NumPy restatement of latent-guided decoding (include/ssc.h: ssc_latent_guide, ssc_latent_guide_rows, ssc_caption_match): the z
block of one decode step under a guide, in float32 with the library's operation order and in float64, and the caption comparison
(lengths, equal positions, exact match, word-level Levenshtein distance) by the textbook dynamic programme."""
import numpy as np


def guided_entries(steps, length, t, B):
    """(B,) bool: which entries are guided at step t."""
    if t >= steps:
        return np.zeros(B, dtype=bool)
    if length is None:
        return np.ones(B, dtype=bool)
    return t < np.asarray(length)


def guide_rows(mean, var, length, t, eps, sent, pm_scale, prior_var, rows_per_entry, ldz=None, dtype=np.float32):
    """mean / var (steps, B, ld >= Z) - var or None -, length (B) or None, eps (rows, Z), sent (rows) or None -> z (rows, ldz) with the
    pad columns Z .. round4(Z) (below ldz) zero and everything behind them NaN (never written).  dtype float32: every operation
    rounded as the kernel rounds it (product, then sum; a correctly rounded square root); float64: the exact-arithmetic yardstick.
    Entries that the kernel must not read are not read here either, so NaNs planted there stay out of the result."""
    rows, Z = eps.shape
    B = rows // rows_per_entry
    assert rows == B * rows_per_entry
    ldz = Z if ldz is None else ldz
    z = np.full((rows, ldz), np.nan, dtype=dtype)
    z[:, Z:min((Z + 3) // 4 * 4, ldz)] = 0
    steps = mean.shape[0]
    guided = guided_entries(steps, length, t, B)
    sd = np.sqrt(dtype(prior_var))
    for r in range(rows):
        b = r // rows_per_entry
        if guided[b]:
            m = mean[t, b, :Z].astype(dtype)
            if var is None:
                z[r, :Z] = m
            else:
                z[r, :Z] = eps[r].astype(dtype) * np.sqrt(var[t, b, :Z].astype(dtype)) + m
        else:
            pm = dtype(pm_scale) * dtype(sent[r]) if sent is not None else dtype(0)
            z[r, :Z] = eps[r].astype(dtype) * sd + pm
    return z


def guide_bound(mean, var, length, t, eps, sent, pm_scale, prior_var, rows_per_entry):
    """(rows, Z) float64: |eps| sqrt(var) + |mean| of every element, with the prior's terms on unguided rows - what the kernel's
    error is measured in."""
    rows, Z = eps.shape
    B = rows // rows_per_entry
    guided = guided_entries(mean.shape[0], length, t, B)
    out = np.zeros((rows, Z))
    for r in range(rows):
        b = r // rows_per_entry
        if guided[b]:
            out[r] = np.abs(mean[t, b, :Z].astype(np.float64))
            if var is not None:
                out[r] += np.abs(eps[r].astype(np.float64)) * np.sqrt(var[t, b, :Z].astype(np.float64))
        else:
            out[r] = np.abs(eps[r].astype(np.float64)) * np.sqrt(float(prior_var)) + (abs(float(pm_scale) * float(sent[r])) if sent is not None else 0.0)
    return out


def caption_len(c, end_index):
    """tokens before the first end_index or negative id"""
    n = 0
    while n < len(c) and c[n] >= 0 and c[n] != end_index:
        n += 1
    return n


def levenshtein(a, b):
    """word-level edit distance (insertions, deletions, substitutions of cost 1) by the full table"""
    D = [[0] * (len(b) + 1) for _ in range(len(a) + 1)]
    for i in range(len(a) + 1):
        D[i][0] = i
    for j in range(len(b) + 1):
        D[0][j] = j
    for i in range(1, len(a) + 1):
        for j in range(1, len(b) + 1):
            D[i][j] = min(D[i - 1][j] + 1, D[i][j - 1] + 1, D[i - 1][j - 1] + (0 if a[i - 1] == b[j - 1] else 1))
    return D[len(a)][len(b)]


def caption_match(pred, ref, end_index):
    """pred (n, Lp), ref (n, Lr) -> (n, 5) int32: n_pred, n_ref, equal positions below the shorter length, exact, distance"""
    out = np.zeros((len(pred), 5), dtype=np.int32)
    for q, (p, r) in enumerate(zip(pred, ref)):
        p, r = [int(x) for x in p], [int(x) for x in r]
        n_p, n_r = caption_len(p, end_index), caption_len(r, end_index)
        eq = sum(1 for j in range(min(n_p, n_r)) if p[j] == r[j])
        out[q] = (n_p, n_r, eq, int(n_p == n_r and eq == n_p), levenshtein(p[:n_p], r[:n_r]))
    return out
