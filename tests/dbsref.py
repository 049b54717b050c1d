"""Diverse beam search (Vijayakumar et al., AAAI 2018) as include/ssc.h defines it (ssc_diverse_desc), restated in plain numpy
float32 the obvious way: per group a full V-long penalised array per row, stable sorts.  Not the device's top-m shortcut.

Beam k = Gr groups of k' = k / Gr consecutive beams; the groups of an entry in order; c[v] = how many beams of the EARLIER groups
of the entry selected token v at this step (the forced END of an ended beam and an empty slot are not counted).
  live row, running true log-prob phi:  r = lp - (lambda * c)  (one fp32 multiply, one fp32 subtract); candidates: the n tokens of
    largest r, descending, ties to the lower token; augmented sum a = phi + r, true sum s = phi + lp (fp32 adds)
  ended row: one candidate, END, a = s = phi
  group merge: the k' candidates of largest a, descending, ties to the lower candidate index j * n + slot; the slot gets the token,
    back-pointer g * k' + j and the TRUE sum s
  step 0: one row per entry, every group takes the k' tokens of largest r (phi = 0)
  a slot with no finite candidate: END at -inf, identity back-pointer
"""
import numpy as np

END = 1
F = np.float32


def top_by(x, n):
    """indices of the n largest of x (1-d), descending, ties to the lower index."""
    return np.argsort(-x, kind="stable")[:n]


def log_softmax64(x):
    """float64 log-softmax of (rows, V), for callers that want log-probs from logits on the CPU."""
    x = np.asarray(x, dtype=np.float64)
    m = x.max(1, keepdims=True)
    return x - m - np.log(np.exp(x - m).sum(1, keepdims=True))


def _gaps(vals):
    """smallest gap between neighbours of a descending list (inf for fewer than two)."""
    v = np.asarray(vals, dtype=np.float64)
    return float(np.min(v[:-1] - v[1:])) if v.size > 1 else np.inf


def first_step(lp, k, Gr, lam, end=END):
    """Step 0 from (B, V) float32 log-probs -> tokens (B, k) int64, log-probs (B, k) float32, margin (B, Gr) float64."""
    lp = np.asarray(lp, dtype=F)
    B, V = lp.shape
    kp = k // Gr
    tok = np.full((B, k), end, dtype=np.int64)
    out = np.full((B, k), -np.inf, dtype=F)
    margin = np.full((B, Gr), np.inf)
    for b in range(B):
        c = np.zeros(V, dtype=F)
        for g in range(Gr):
            r = lp[b] - (F(lam) * c)
            o = top_by(r, kp + 1 if V > kp else kp)
            margin[b, g] = _gaps(r[o])
            for i, v in enumerate(o[:kp]):
                if np.isfinite(r[v]):
                    tok[b, g * kp + i] = v
                    out[b, g * kp + i] = lp[b, v]
                    c[v] += 1
    return tok, out, margin


def next_step(lp, last_pred, phi, B, k, Gr, n, lam, end=END):
    """Step >= 1 from (B * k, V) float32 log-probs, last tokens and running log-probs (B * k,) -> tokens, log-probs (float32),
    back-pointers (B, k) and the selection margin (B, Gr): the smallest gap between neighbours in a group's kept order, between
    its last kept and first rejected candidate, and - for a row whose last candidate was kept - between that candidate and the
    row's next token."""
    lp = np.asarray(lp, dtype=F)
    V = lp.shape[1]
    last_pred = np.asarray(last_pred).reshape(B, k)
    phi = np.asarray(phi, dtype=F).reshape(B, k)
    kp = k // Gr
    tok = np.full((B, k), end, dtype=np.int64)
    out = np.full((B, k), -np.inf, dtype=F)
    bp = np.tile(np.arange(k, dtype=np.int64), (B, 1))
    margin = np.full((B, Gr), np.inf)
    for b in range(B):
        c = np.zeros(V, dtype=F)
        for g in range(Gr):
            ca = np.full(kp * n, -np.inf, dtype=F)
            cs = np.full(kp * n, -np.inf, dtype=F)
            ct = np.full(kp * n, end, dtype=np.int64)
            forced = np.zeros(kp * n, dtype=bool)
            nxt = np.full(kp, -np.inf)   # a row's first token outside its candidates, augmented
            for j in range(kp):
                row = b * k + g * kp + j
                p = phi[b, g * kp + j]
                if last_pred[b, g * kp + j] == end:
                    ca[j * n] = cs[j * n] = p
                    forced[j * n] = True
                    continue
                r = lp[row] - (F(lam) * c)
                o = top_by(r, n + 1 if V > n else n)
                for s, v in enumerate(o[:n]):
                    ca[j * n + s] = p + r[v]
                    cs[j * n + s] = p + lp[row, v]
                    ct[j * n + s] = v
                if len(o) > n:
                    nxt[j] = float(p + r[o[n]])
            sel = top_by(ca, min(kp + 1, kp * n))
            kept = [x for x in sel[:kp] if ca[x] > -np.inf and not np.isnan(ca[x])]
            gaps = [_gaps(ca[sel])] if len(kept) == kp else [np.inf]
            for i, x in enumerate(kept):
                o_ = g * kp + i
                tok[b, o_] = ct[x]
                out[b, o_] = cs[x]
                bp[b, o_] = g * kp + x // n
                if x % n == n - 1 and not forced[x]:
                    gaps.append(float(ca[x]) - nxt[x // n])
            for x in kept:
                if not forced[x]:
                    c[ct[x]] += 1
            margin[b, g] = min(gaps)
    return tok, out, bp, margin


def search(step, states, B, k, Gr, n, lam, max_steps, end=END, early_stop=True):
    """The whole search.  step(tokens (rows,) int64, states) -> (log-probs (rows, V) float32, new states): step 0 with the B start
    rows (tokens = END), later steps with the B * k beam rows.  states: a dict of arrays with the rows leading; enlarged to k rows
    per entry after step 0 and re-ordered by back-pointer after every later step (cbs.py:152-155, :236-250).
    -> predictions (B, k, steps), log-probs (B, k) float32, record {"tok", "lp", "bp", "margin"}: lists per step."""
    lp0, states = step(np.full(B, end, dtype=np.int64), states)
    tok, lps, mg = first_step(lp0, k, Gr, lam, end)
    rec = {"tok": [tok], "lp": [lps], "bp": [None], "margin": [mg]}
    states = {key: np.repeat(np.asarray(v), k, axis=0) for key, v in states.items()}
    for t in range(1, max_steps):
        if early_stop and (rec["tok"][-1] == end).all():
            break
        lp, states = step(rec["tok"][-1].reshape(-1), states)
        tok, lps, bp, mg = next_step(lp, rec["tok"][-1], rec["lp"][-1], B, k, Gr, n, lam, end)
        idx = (np.arange(B)[:, None] * k + bp).reshape(-1)
        states = {key: np.asarray(v)[idx] for key, v in states.items()}
        for key, v in (("tok", tok), ("lp", lps), ("bp", bp), ("margin", mg)):
            rec[key].append(v)
    steps = len(rec["tok"])
    pred = np.empty((B, k, steps), dtype=np.int64)
    idx = np.tile(np.arange(k), (B, 1))
    for t in range(steps - 1, -1, -1):
        pred[:, :, t] = np.take_along_axis(rec["tok"][t], idx, 1)
        if t > 0:
            idx = np.take_along_axis(rec["bp"][t], idx, 1)
    return pred, rec["lp"][-1], rec


def top_n_from_list(lp_row, counts, lam, n, m):
    """The device's shortcut for one row: its n best tokens under r computed from its m best under lp only."""
    lp_row = np.asarray(lp_row, dtype=F)
    lst = top_by(lp_row, m)
    r = lp_row[lst] - (F(lam) * np.asarray(counts, dtype=F)[lst])
    # (value descending, token ascending) inside the list
    order = sorted(range(len(lst)), key=lambda e: (-float(r[e]), int(lst[e])))
    return [int(lst[e]) for e in order[:n]]
