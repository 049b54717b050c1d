"""The definition of an attention trace, named once for the attention-trace tests: a NumPy restatement of the `anc` a one-call
decode writes (include/ssc.h: ssc_attn_record) and of what ssc_attn_gather reads from a trace."""
import numpy as np


def ancestry(words, backs, ctl0, end_index, log_probs=None):
    """words (T, B, SB) ints: the words chosen at every step, in that step's order (a scoring call: the targets, -1 from the caption's
    end on).  backs (T - 1, B, SB) or None (the identity): backs[t - 1][b, j] = the place, after step t - 1, of the beam that became
    beam j at step t.  ctl0: the number of steps that ran (None: all T).  log_probs (B, SB) or None: the final beams' log-probs.
    -> anc (B * SB, T) int32: the row of step t that produced the attention behind word t of final caption (b, j), or -1.
    Rows of step t >= 1 are (b, place after step t - 1), SB per batch entry; step 0 has one row per batch entry."""
    words = np.asarray(words)
    T, B, SB = words.shape
    steps = T if ctl0 is None else min(max(int(ctl0), 1), T)
    anc = np.full((B, SB, T), -1, dtype=np.int32)
    for b in range(B):
        for j in range(SB):
            if log_probs is not None and np.asarray(log_probs)[b, j] <= -1e19:
                continue   # a beam nothing finite led to
            place = np.zeros(steps, dtype=np.int64)   # place[t]: where the caption's beam stood after step t
            place[steps - 1] = j
            for t in range(steps - 1, 0, -1):
                place[t - 1] = place[t] if backs is None else backs[t - 1][b, place[t]]
            for t in range(steps):
                if words[t, b, place[t]] < 0:
                    continue   # no word here
                if t == 0:
                    anc[b, j, t] = b
                elif words[t - 1, b, place[t - 1]] != end_index:   # (after an END the row is not stepped: a forced END read nothing)
                    anc[b, j, t] = b * SB + place[t - 1]
    return anc.reshape(B * SB, T)


def gather(hist, anc, sel=None):
    """hist (steps, rows, R) float32, anc (n_caps, steps) ints, sel: caption numbers (None: all).
    -> maps (n, steps, R) float32 (bit copies; zeros where anc is outside [0, rows) or the caption number outside [0, n_caps)),
    top_region (n, steps) int32 (first arg-max; -1 on a zero row), top_weight (n, steps) float32, entropy (n, steps) float64."""
    hist = np.asarray(hist, dtype=np.float32)
    anc = np.asarray(anc)
    steps, rows, R = hist.shape
    n_caps = anc.shape[0]
    sel = np.arange(n_caps) if sel is None else np.asarray(sel).reshape(-1)
    n = len(sel)
    maps = np.zeros((n, steps, R), dtype=np.float32)
    top = np.full((n, steps), -1, dtype=np.int32)
    wgt = np.zeros((n, steps), dtype=np.float32)
    ent = np.zeros((n, steps), dtype=np.float64)
    for i, q in enumerate(sel):
        if not 0 <= q < n_caps:
            continue
        for t in range(steps):
            a = int(anc[q, t])
            if not 0 <= a < rows:
                continue
            row = hist[t, a]
            maps[i, t] = row
            top[i, t] = int(np.argmax(row))
            wgt[i, t] = row[top[i, t]]
            p = row[row > 0].astype(np.float64)
            ent[i, t] = -(p * np.log(p)).sum()
    return maps, top, wgt, ent
