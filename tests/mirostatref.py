"""float64 restatement of Mirostat 2.0 for the word samplers (ssc_mirostat, include/ssc.h): the cut of a row of raw logits at the
row's running threshold mu, the update of mu behind the draw, and the whole control loop, with - a condition on a test's INPUTS -
the tokens whose membership float32 arithmetic cannot be expected to decide.

All quantities in nats.  With T the temperature, over the finite entries of x: q = softmax(x / T), the surprise of v is -log q_v.
  cut     v is kept iff -log q_v <= mu, or v is the lowest-index maximum.
  update  s = -log q_w of the drawn word under the tempered distribution BEFORE the cut; mu' = mu - eta (s - tau).
Undecidable tokens: |log q_v + mu| < band.  `first` is kept in any arithmetic and is never one.  A maximal entry other than `first`
is cut when mu lies below the top surprise, so it is reported like any other entry (stricter than leaving it out: the condition
on the inputs only grows).
  stand-alone cut, the device handed the same fp32 mu:  band = truncationref.D_BAND (2e-5), the same kind of quantity, fixed.
  step t of a decode, mu_t having accumulated t surprise errors scaled by eta:  band(t) = D_BAND * (1 + eta * t).
Every device comparison first asserts that the restatement finds no undecidable token."""
import numpy as np

from truncationref import D_BAND, row_stats

LN2 = float(np.log(2.0))


def band(t=0, eta=0.0):
    return D_BAND * (1.0 + eta * t)


class Cut:
    """kept (V,) bool; mx, logz: the row's maximum and log-normaliser (float64); logq (V,) (-inf at -inf entries); first: the
    lowest-index maximum (-1: no finite entry); undecidable: sorted token ids; live: the row has a finite entry"""

    def __init__(self, kept, mx, logz, logq, first, undecidable, live):
        self.kept, self.mx, self.logz, self.logq, self.first, self.undecidable, self.live = kept, mx, logz, logq, first, undecidable, live


def cut_row(x, mu, T=1.0, band_=D_BAND):
    """-> Cut of one row of raw logits x (V,) (float32 values) at threshold mu.  A row without a finite entry: nothing kept."""
    x32 = np.asarray(x, dtype=np.float32)
    V = x32.shape[0]
    st = row_stats(x32, T)
    if st is None:
        return Cut(np.zeros(V, dtype=bool), 0.0, 0.0, np.full(V, -np.inf), -1, [], False)
    fin, q, logq, _ = st
    x64 = x32.astype(np.float64)
    mx = float(x64[fin].max())
    logz = float(np.log(np.exp((x64[fin] - mx) / T).sum()))
    first = int(np.argmax(np.where(fin, x32, -np.inf)))   # the lowest-index maximum
    mu = float(mu)
    kept = fin & (-logq <= mu)
    kept[first] = True
    with np.errstate(invalid="ignore"):   # (-inf + inf at a dropped entry under an infinite mu: masked by `fin`)
        und = [int(v) for v in np.nonzero(fin & (np.abs(logq + mu) < band_))[0] if v != first]
    return Cut(kept, mx, logz, logq, first, und, True)


def cut_rows(x, V, mu, T, last_pred=None, end=None, band_=D_BAND):
    """x (rows, ld) float32, mu (rows,) -> (edited copy, kept (rows,) int, norm (2, rows) float64 with NaN where the device leaves
    norm alone, undecidable: [(row, token)]).  Rows whose last_pred is `end`, rows without a finite entry and columns V .. ld - 1
    are returned as they came; dropped entries are -inf, kept ones keep their bits."""
    out = np.array(x, dtype=np.float32, copy=True)
    rows = out.shape[0]
    kept = np.zeros(rows, dtype=np.int64)
    norm = np.full((2, rows), np.nan)
    und = []
    for r in range(rows):
        if last_pred is not None and int(last_pred[r]) == end:
            continue
        c = cut_row(out[r, :V], mu[r], T, band_)
        if not c.live:
            continue
        out[r, :V][~c.kept & np.isfinite(out[r, :V])] = -np.inf
        kept[r] = int(c.kept.sum())
        norm[0, r], norm[1, r] = c.mx, c.logz
        und += [(r, v) for v in c.undecidable]
    return out, kept, norm, und


def update_rows(x, V, T, tau, eta, pred, mu, last_pred=None, end=None):
    """The update behind the draw of pred (rows,) from the rows x (rows, ld) - edited or not: a drawn word is a kept word and the
    surprise is that under the distribution BEFORE the cut, which the finite entries of the row as it ARRIVED at the cut define;
    pass that row.  -> (mu' (rows,), surprise (rows,)) float64.  Pass-through rows (ended, a token outside [0, V), x_w = -inf):
    mu' = mu, surprise = 0."""
    x = np.asarray(x, dtype=np.float32)
    rows = x.shape[0]
    mu2 = np.array(mu, dtype=np.float64, copy=True)
    sur = np.zeros(rows)
    for r in range(rows):
        if last_pred is not None and int(last_pred[r]) == end:
            continue
        w = int(pred[r])
        if not 0 <= w < V or not np.isfinite(x[r, w]):
            continue
        st = row_stats(x[r, :V], T)
        s = float(-st[2][w])
        sur[r] = s
        mu2[r] = mu2[r] - eta * (s - tau)
    return mu2, sur


def control_loop(rows_fn, steps, tau, eta, mu0, T, draw):
    """The whole control of ONE caption: rows_fn(t) -> the raw logits (V,) of step t, draw(t, q) -> a token from the renormalised
    kept distribution q (V,).  -> (tokens, mu (steps + 1,), surprise (steps,), kept (steps,))."""
    mu = np.zeros(steps + 1)
    mu[0] = mu0
    sur = np.zeros(steps)
    kept = np.zeros(steps, dtype=np.int64)
    toks = []
    for t in range(steps):
        x = np.asarray(rows_fn(t), dtype=np.float32)
        c = cut_row(x, mu[t], T)
        qk = np.where(c.kept, np.exp(c.logq), 0.0)
        qk /= qk.sum()
        w = int(draw(t, qk))
        assert c.kept[w]
        toks.append(w)
        kept[t] = int(c.kept.sum())
        sur[t] = -c.logq[w]
        mu[t + 1] = mu[t] - eta * (sur[t] - tau)
    return toks, mu, sur, kept
