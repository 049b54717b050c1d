"""float64 restatement of the word samplers' truncation (ssc_truncation, include/ssc.h): typical, min-p, eta and epsilon cuts of a
row of raw logits, with the entropy and - a condition on a test's INPUTS - the tokens whose membership float32 arithmetic cannot be
expected to decide.

Undecidable tokens (the bands are fixed here, never fitted to the device):
  typical  any token other than the cut whose d lies within D_BAND = 2e-5 nats of the cut's d and whose logit is not an exact
           duplicate of the cut's logit (duplicates are decided by the index rule, exactly); any token whose mass ahead lies within
           MASS_BAND = 1e-6 of tau.
  2 to 4   any token with |log q_v - threshold| < D_BAND (the lowest-index maximum of kinds 3 and 4, always kept, is never one;
           nor is an entry equal to the maximum under min-p, kept in any arithmetic).
D_BAND is four to five times the largest float32-against-float64 error of d and H a NumPy restatement shows (4.3e-6 over
V = 37 .. 40 000, T = 0.7 .. 1.3); MASS_BAND is samplerref.check_against_reference's own.  Every device comparison first asserts
that the restatement finds no undecidable token."""
import numpy as np

KIND = {"none": 0, "typical": 1, "min-p": 2, "eta": 3, "epsilon": 4}
D_BAND = 2e-5
MASS_BAND = 1e-6


class Cut:
    """kept (V,) bool; H the entropy in nats; undecidable: sorted token ids; q (V,) the tempered distribution (0 at -inf entries);
    d (V,) |s - H| (typical; inf at -inf entries) or log q (kinds 2 to 4); cut: the typical cut's token or -1"""

    def __init__(self, kept, H, undecidable, q, d, cut=-1):
        self.kept, self.H, self.undecidable, self.q, self.d, self.cut = kept, H, undecidable, q, d, cut


def row_stats(x, T):
    """x (V,) logits -> (finite mask, q, log q, H) in float64; None where no entry is finite"""
    x = np.asarray(x, dtype=np.float64)
    fin = np.isfinite(x)
    if not fin.any():
        return None
    a = np.where(fin, (x - x[fin].max()) / T, -np.inf)
    e = np.where(fin, np.exp(a), 0.0)
    Z = e.sum()
    q = e / Z
    logq = np.where(fin, a - np.log(Z), -np.inf)
    H = float(-(q[fin] * logq[fin]).sum())   # (finite entries only: 0 * -inf is never formed)
    return fin, q, logq, H


def truncate_row(x, kind, value, T=1.0):
    """-> Cut of one row of raw logits x (V,) (float32 values).  A row without a finite entry: nothing kept, H = 0."""
    x32 = np.asarray(x, dtype=np.float32)
    V = x32.shape[0]
    st = row_stats(x32, T)
    if st is None:
        return Cut(np.zeros(V, dtype=bool), 0.0, [], np.zeros(V), np.full(V, np.inf))
    fin, q, logq, H = st
    if kind == 0:
        return Cut(fin.copy(), H, [], q, logq)
    if kind == 1:
        d = np.where(fin, np.abs(-logq - H), np.inf)
        order = np.lexsort((np.arange(V), d))          # ascending d, equal d by the lower index
        order = order[fin[order]]
        ahead = np.cumsum(q[order]) - q[order]
        if value >= 1.0:    # tau = 1 keeps every finite entry
            return Cut(fin.copy(), H, [], q, d, int(order[-1]))
        keep_n = int(np.searchsorted(ahead, value, side="left"))   # entries with mass ahead < tau
        keep_n = max(keep_n, 1)
        kept = np.zeros(V, dtype=bool)
        kept[order[:keep_n]] = True
        cut = int(order[keep_n - 1])
        near = (np.abs(d[order] - d[cut]) < D_BAND) & (x32[order] != x32[cut]) & (order != cut)
        near |= (np.abs(ahead - value) < MASS_BAND) & (np.arange(order.size) > 0)
        return Cut(kept, H, sorted(int(v) for v in order[near]), q, d, cut)
    first = int(np.argmax(np.where(fin, x32, -np.inf)))   # the lowest-index maximum
    if kind == 2:
        thr = np.log(value) + logq[first]
    elif kind == 3:
        thr = min(np.log(value), 0.5 * np.log(value) - H)
    elif kind == 4:
        thr = np.log(value)
    else:
        raise ValueError(kind)
    kept = fin & (logq >= thr)
    und = [int(v) for v in np.nonzero(fin & (np.abs(logq - thr) < D_BAND))[0]]
    if kind == 2:       # an entry equal to the maximum has (x - max) / T = 0 >= log m in any arithmetic
        und = [v for v in und if x32[v] != x32[first]]
    else:
        kept[first] = True
        und = [v for v in und if v != first]
    return Cut(kept, H, und, q, logq)


def edit_rows(x, V, kind, value, T, last_pred=None, end=None):
    """x (rows, ld) float32 -> (edited copy, entropy (rows,) float64, kept (rows,) int, undecidable: [(row, token)]).  Rows whose
    last_pred is `end` and columns V .. ld - 1 are returned as they came; dropped entries are -inf, kept ones keep their bits."""
    out = np.array(x, dtype=np.float32, copy=True)
    rows = out.shape[0]
    ent = np.zeros(rows)
    kept = np.zeros(rows, dtype=np.int64)
    und = []
    for r in range(rows):
        if last_pred is not None and int(last_pred[r]) == end:
            continue
        c = truncate_row(out[r, :V], kind, value, T)
        if kind != 0:
            out[r, :V][~c.kept & np.isfinite(out[r, :V])] = -np.inf
        ent[r] = c.H
        kept[r] = int(c.kept.sum())
        und += [(r, v) for v in c.undecidable]
    return out, ent, kept, und


def renormalised(x, kept, T):
    """The float64 distribution the draw is made from: softmax(x / T) over the kept set"""
    x = np.asarray(x, dtype=np.float64)
    a = np.where(kept, x / T, -np.inf)
    e = np.exp(a - a[kept].max())
    return e / e.sum()
