"""Beam search under the decode rules as include/ssc.h defines it (ssc_rules_desc), restated in plain numpy float32 the obvious
way: a full V-long masked array per row, stable sorts.  Not the device's ban list and block argmax.

Every beam carries its true summed log-prob phi, its token history, its length and its score.  At step t:
  banned tokens of a live row: the suppress list; END if t < min_length; with n >= 1 every token v such that the n-gram
    (w_{t-n+1}, .., w_{t-1}, v) already occurs in the history w_0 .. w_{t-1} (END is never banned by this rule)
  live row: the per_node unbanned tokens of largest lp, descending, ties to the lower token; sum s = phi + lp (fp32 add), length
    L = t + 1, key = s / table[L - 1] (fp32 division)
  ended row: one candidate, END, s = phi, L = len, key = phi / table[len - 1]
  merge: the k candidates of largest key, descending, ties to the lower candidate index j * per_node + slot; the slot gets the
    token, back-pointer j, the TRUE sum s, len = L, score = key, and the parent's history with the token appended
  step 0: one row per entry with an empty history
  a slot with no finite candidate: END at -inf, identity back-pointer, its own history plus END, len = t + 1, score -inf
"""
import numpy as np

END = 1
F = np.float32
MAX_LEN = 64


def top_by(x, n):
    """indices of the n largest of x (1-d), descending, ties to the lower index."""
    return np.argsort(-x, kind="stable")[:n]


def penalty_table(alpha):
    """L ** alpha for L = 1..64, formed in float64 and rounded to float32 once."""
    return (np.arange(1, MAX_LEN + 1, dtype=np.float64) ** float(alpha)).astype(F)


class Rules:
    def __init__(self, ngram=0, min_length=0, suppress=(), table=None):
        self.n, self.m, self.suppress = int(ngram), int(min_length), tuple(int(v) for v in suppress)
        self.table = np.ones(MAX_LEN, dtype=F) if table is None else np.asarray(table, dtype=F)
        assert self.table.shape == (MAX_LEN,)

    @property
    def off(self):
        return self.n == 0 and self.m == 0 and not self.suppress and (self.table == F(1)).all()


def banned(V, hist, t, rules, end=END):
    """-> (V,) bool: the tokens a live row with history hist (its first t entries) may not emit at step t."""
    ban = np.zeros(V, dtype=bool)
    for v in rules.suppress:
        ban[v] = True
    if t < rules.m:
        ban[end] = True
    n = rules.n
    if n >= 1 and t >= n:
        h = [int(v) for v in hist[:t]]
        suffix = h[t - (n - 1):t] if n > 1 else []
        for i in range(t - n + 1):
            if h[i:i + n - 1] == suffix and h[i + n - 1] != end:
                ban[h[i + n - 1]] = True
    return ban


def _gaps(vals):
    """smallest gap between neighbours of a descending list (inf for fewer than two)."""
    v = np.asarray(vals, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return float(np.min(v[:-1] - v[1:])) if v.size > 1 else np.inf


def _merge(b, t, k, per, ckey, csum, ctok, clen, forced, nxt, own_hist, parent_hist, out, end):
    """the k best of one entry's candidates into slot arrays `out`; -> the entry's selection margin."""
    tok, sums, bp, lens, scores, hist = out
    sel = top_by(ckey, min(k + 1, ckey.size))
    kept = [x for x in sel[:k] if ckey[x] > -np.inf and not np.isnan(ckey[x])]
    gaps = [_gaps(ckey[sel])] if len(kept) == k else [np.inf]
    for i in range(k):
        if i < len(kept):
            x = kept[i]
            j = x // per
            tok[b, i], sums[b, i], bp[b, i], lens[b, i], scores[b, i] = ctok[x], csum[x], j, clen[x], ckey[x]
            hist[b, i, :t] = parent_hist(j)
            if x % per == per - 1 and not forced[x]:
                gaps.append(float(ckey[x]) - nxt[j])
        else:
            tok[b, i], sums[b, i], bp[b, i], lens[b, i], scores[b, i] = end, -np.inf, i, t + 1, -np.inf
            hist[b, i, :t] = own_hist(i)
        hist[b, i, t] = tok[b, i]
    return min(gaps)


def _outputs(B, k, t, end):
    return (np.full((B, k), end, dtype=np.int64), np.full((B, k), -np.inf, dtype=F), np.tile(np.arange(k, dtype=np.int64), (B, 1)),
            np.zeros((B, k), dtype=np.int32), np.full((B, k), -np.inf, dtype=F), np.zeros((B, k, t + 1), dtype=np.int32))


def first_step(lp, k, rules, end=END):
    """Step 0 from (B, V) float32 log-probs -> tokens (B, k) int64, sums (B, k) float32, lengths (B, k) int32, scores (B, k) float32,
    histories (B, k, 1) int32, margin (B,) float64."""
    lp = np.asarray(lp, dtype=F)
    B, V = lp.shape
    out = _outputs(B, k, 0, end)
    margin = np.full(B, np.inf)
    for b in range(B):
        x = np.where(banned(V, [], 0, rules, end), F(-np.inf), lp[b]).astype(F)
        o = top_by(x, min(k + 1, V))
        ckey = np.full(k, -np.inf, dtype=F)
        csum = np.full(k, -np.inf, dtype=F)
        ctok = np.full(k, end, dtype=np.int64)
        for s, v in enumerate(o[:k]):
            if x[v] > -np.inf:
                csum[s], ctok[s] = x[v], v
                ckey[s] = csum[s] / rules.table[0]
        nxt = [float(x[o[k]] / rules.table[0]) if len(o) > k else -np.inf]
        margin[b] = _merge(b, 0, k, k, ckey, csum, ctok, np.ones(k, dtype=np.int32), np.zeros(k, dtype=bool), nxt,
                           lambda i: [], lambda j: [], out, end)
    tok, sums, _, lens, scores, hist = out
    return tok, sums, lens, scores, hist, margin


def next_step(lp, last_pred, phi, hist, lens, t, B, k, per, rules, end=END):
    """Step t >= 1 from (B * k, V) float32 log-probs, the last tokens, running sums and lengths (B, k) and the histories (B, k, >= t)
    -> tokens, sums, back-pointers, lengths, scores (B, k), histories (B, k, t + 1) and the selection margin (B,): the smallest gap
    between neighbouring keys in the kept order, between the last kept and the first rejected candidate, and - for a row whose last
    candidate was kept - between that candidate's key and the key its next unbanned token would have had."""
    lp = np.asarray(lp, dtype=F)
    V = lp.shape[1]
    last_pred = np.asarray(last_pred).reshape(B, k)
    phi = np.asarray(phi, dtype=F).reshape(B, k)
    lens = np.asarray(lens).reshape(B, k)
    hist = np.asarray(hist)
    out = _outputs(B, k, t, end)
    margin = np.full(B, np.inf)
    for b in range(B):
        ckey = np.full(k * per, -np.inf, dtype=F)
        csum = np.full(k * per, -np.inf, dtype=F)
        ctok = np.full(k * per, end, dtype=np.int64)
        clen = np.full(k * per, t + 1, dtype=np.int32)
        forced = np.zeros(k * per, dtype=bool)
        nxt = np.full(k, -np.inf)
        for j in range(k):
            p = phi[b, j]
            if last_pred[b, j] == end:
                csum[j * per] = p
                with np.errstate(invalid="ignore"):
                    ckey[j * per] = p / rules.table[lens[b, j] - 1]
                clen[j * per] = lens[b, j]
                forced[j * per] = True
                continue
            row = b * k + j
            x = np.where(banned(V, hist[b, j], t, rules, end), F(-np.inf), lp[row]).astype(F)
            o = top_by(x, min(per + 1, V))
            for s, v in enumerate(o[:per]):
                if x[v] > -np.inf:
                    csum[j * per + s] = p + x[v]
                    ckey[j * per + s] = csum[j * per + s] / rules.table[t]
                    ctok[j * per + s] = v
            if len(o) > per and x[o[per]] > -np.inf:
                nxt[j] = float(F(p + x[o[per]]) / rules.table[t])
        margin[b] = _merge(b, t, k, per, ckey, csum, ctok, clen, forced, nxt, lambda i: hist[b, i, :t], lambda j: hist[b, j, :t],
                           out, end)
    tok, sums, bp, lens_out, scores, hist_out = out
    return tok, sums, bp, lens_out, scores, hist_out, margin


def search(step, states, B, k, per, rules, max_steps, end=END, early_stop=True):
    """The whole search.  step(tokens (rows,) int64, states) -> (log-probs (rows, V) float32, new states): step 0 with the B start
    rows (tokens = END), later steps with the B * k beam rows.  states: a dict of arrays with the rows leading; enlarged to k rows
    per entry after step 0 and re-ordered by back-pointer after every later step.
    -> predictions (B, k, steps), sums (B, k) float32, record {"tok", "lp", "bp", "len", "score", "hist", "margin"}: lists per
    step."""
    lp0, states = step(np.full(B, end, dtype=np.int64), states)
    tok, sums, lens, scores, hist, mg = first_step(lp0, k, rules, end)
    rec = {"tok": [tok], "lp": [sums], "bp": [None], "len": [lens], "score": [scores], "hist": [hist], "margin": [mg]}
    states = {key: np.repeat(np.asarray(v), k, axis=0) for key, v in states.items()}
    for t in range(1, max_steps):
        if early_stop and (rec["tok"][-1] == end).all():
            break
        lp, states = step(rec["tok"][-1].reshape(-1), states)
        tok, sums, bp, lens, scores, hist, mg = next_step(lp, rec["tok"][-1], rec["lp"][-1], rec["hist"][-1], rec["len"][-1], t, B, k,
                                                          per, rules, end)
        idx = (np.arange(B)[:, None] * k + bp).reshape(-1)
        states = {key: np.asarray(v)[idx] for key, v in states.items()}
        for key, v in (("tok", tok), ("lp", sums), ("bp", bp), ("len", lens), ("score", scores), ("hist", hist), ("margin", mg)):
            rec[key].append(v)
    steps = len(rec["tok"])
    pred = np.empty((B, k, steps), dtype=np.int64)
    idx = np.tile(np.arange(k), (B, 1))
    for t in range(steps - 1, -1, -1):
        pred[:, :, t] = np.take_along_axis(rec["tok"][t], idx, 1)
        if t > 0:
            idx = np.take_along_axis(rec["bp"][t], idx, 1)
    return pred, rec["lp"][-1], rec


def repeated_ngram(tokens, n, end=END):
    """True when the caption (cut before its first END) holds some n-gram twice."""
    toks = [int(v) for v in tokens]
    if end in toks:
        toks = toks[:toks.index(end)]
    grams = [tuple(toks[i:i + n]) for i in range(len(toks) - n + 1)]
    return len(set(grams)) < len(grams)
