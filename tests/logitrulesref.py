"""NumPy float32 restatement of the logit rules of the word samplers (include/ssc.h: ssc_logit_rules), one operation per line.

A live row at step t has the history w_0 .. w_{t-1}.  Its raw logits are edited in this order: bias, penalties, bans.  Every
arithmetic step is one float32 operation, so the result is comparable with the device's bit for bit."""
import numpy as np

F = np.float32
NEG_INF = F(-np.inf)


class Rules:
    """The fields of ssc_logit_rules (the bias as a host array (n_bias, V) or None, bias_row as a list or None)."""

    def __init__(self, no_repeat_ngram=0, min_length=0, suppress=(), repetition_penalty=1.0, presence_penalty=0.0,
                 frequency_penalty=0.0, bias=None, bias_row=None):
        self.no_repeat_ngram = int(no_repeat_ngram)
        self.min_length = int(min_length)
        self.suppress = tuple(int(v) for v in suppress)
        self.repetition_penalty = F(repetition_penalty)
        self.presence_penalty = F(presence_penalty)
        self.frequency_penalty = F(frequency_penalty)
        self.bias = None if bias is None else np.asarray(bias, dtype=np.float32)
        self.bias_row = None if bias_row is None else [int(v) for v in bias_row]


def ended(history, end_index):
    """A row whose last token is END has ended: it is neither read nor written."""
    return len(history) >= 1 and int(history[-1]) == end_index


def ngram_bans(history, n, V, end_index):
    """The tokens v such that (w_{t-n+1}, .., w_{t-1}, v) already occurs in the history; END and ids outside [0, V) never."""
    t = len(history)
    out = set()
    if n < 1:
        return out
    for j in range(0, t - n + 1):   # the n-gram that starts at position j ends inside the history
        hit = True
        for q in range(n - 1):
            if int(history[j + q]) != int(history[t - (n - 1) + q]):
                hit = False
        tok = int(history[j + n - 1])
        if hit and tok != end_index and 0 <= tok < V:
            out.add(tok)
    return out


def edit_row(x, V, history, r, end_index, row=0):
    """The edited copy of one row x (ld,) float32 of row index `row` under the rules r with the history `history` (its length is the
    step t).  Columns V .. ld - 1 are never touched; an ended row comes back as it is."""
    x = np.array(x, dtype=np.float32, copy=True)
    if ended(history, end_index):
        return x
    t = len(history)
    with np.errstate(all="ignore"):
        # 1. bias
        if r.bias is not None:
            br = 0 if r.bias_row is None else r.bias_row[row]
            if 0 <= br < r.bias.shape[0]:
                x[:V] = x[:V] + r.bias[br, :V]   # (elementwise: one float32 addition per entry)
        # 2. penalties: every distinct token of the history, once
        seen = []
        for c in history:
            c = int(c)
            if c < 0 or c >= V or c in seen:
                continue
            seen.append(c)
            n_c = sum(1 for w in history if int(w) == c)
            if x[c] > 0:
                x[c] = F(x[c] / r.repetition_penalty)
            else:
                x[c] = F(x[c] * r.repetition_penalty)
            f = F(r.frequency_penalty * F(n_c))
            s = F(r.presence_penalty + f)
            x[c] = F(x[c] - s)
    # 3. bans
    for v in r.suppress:
        x[v] = NEG_INF
    if t < r.min_length:
        x[end_index] = NEG_INF
    for v in ngram_bans(history, r.no_repeat_ngram, V, end_index):
        x[v] = NEG_INF
    return x


def edit_rows(logits, V, hist, t, r, end_index):
    """logits (rows, ld) float32, hist (>= t, rows) integer (token j of row i is hist[j, i]) or None at t = 0 -> the edited copy."""
    out = np.array(logits, dtype=np.float32, copy=True)
    for i in range(out.shape[0]):
        history = [int(hist[j, i]) for j in range(t)]
        out[i] = edit_row(out[i], V, history, r, end_index, row=i)
    return out


def banned(V, history, r, end_index, row=0):
    """The set of tokens with an edited logit of -inf whatever the logits: the three bans and the bias's -inf entries."""
    t = len(history)
    out = set(r.suppress) | ngram_bans(history, r.no_repeat_ngram, V, end_index)
    if t < r.min_length:
        out.add(end_index)
    if r.bias is not None:
        br = 0 if r.bias_row is None else r.bias_row[row]
        if 0 <= br < r.bias.shape[0]:
            out |= set(int(v) for v in np.nonzero(np.isneginf(r.bias[br, :V]))[0])
    return out
