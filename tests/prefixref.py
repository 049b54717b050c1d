"""The definition of prompted decoding, named once for the prefix tests: priming as a teacher-forced loop over oracle.decode_step
from zero states (the style of tests/scoreref.py), the join of prefix and continuation restated in NumPy, the step closure of a
search that starts from the primed oracle state, and the margins of the selections oracle.cbs_search makes."""
import contextlib

import numpy as np
import torch

import oracle
import scoreref as SR
from oracle.seqcvae_oracle import zero_states

STATE_KEYS = ("h1", "c1", "h_decoder", "c_decoder")   # ssc_start_state's h1, c1, hd, cd
MARGIN = 2e-4   # twice the project's 1e-4 log-prob tolerance: a selection with a larger gap cannot be flipped by it


def prefix_lengths(prefix, V, end_index):
    """prefix (B, Lp) ints -> (B,) the leading ids that lie in [0, V) and are not end_index."""
    p = np.asarray(prefix, dtype=np.int64)
    ok = (p >= 0) & (p < V) & (p != end_index)
    return np.logical_and.accumulate(ok, axis=1).sum(1)


def expand_rows(t, nimg, rep):
    return t.unsqueeze(1).expand(nimg, rep, *t.shape[1:]).reshape(nimg * rep, *t.shape[1:])


def prime(params, cfg, feats, sentiment, prefix, n_samples, eps, obj_atts=None):
    """The teacher-forced oracle of ssc_decode_prime: feats (nimg, R, F), sentiment (nimg,) or None, prefix (B, Lp) with
    B = nimg * n_samples rows (image, sample), eps (Lp, B, Z).  Step 0 feeds END from zero states, step t feeds prefix[:, t - 1];
    a row is captured after the step that was scored against its last prefix word.
    -> dict(states {h1, c1, h_decoder, c_decoder} (B, H) float32 tensors, tokens (B,), lengths (B,), log_probs (B,) float64,
    token_lp (B, Lp) float64)."""
    prefix = np.asarray(prefix, dtype=np.int64)
    B, Lp = prefix.shape
    nimg = feats.size(0)
    assert B == nimg * n_samples
    end, V = cfg.boundary_index, cfg.vocab_size
    lens = prefix_lengths(prefix, V, end)
    fr = expand_rows(feats, nimg, n_samples)
    se = sentiment.reshape(nimg, 1).expand(nimg, n_samples).reshape(B, 1) if sentiment is not None else None
    ob = expand_rows(obj_atts, nimg, n_samples) if obj_atts is not None else None
    pm, pv = oracle.prior_from_sentiment(cfg, se, B, fr)
    states = zero_states(B, cfg.hidden_size, fr)
    out = {k: torch.zeros(B, cfg.hidden_size) for k in STATE_KEYS}
    tokens = np.full(B, end, dtype=np.int64)
    total = np.zeros(B, dtype=np.float64)
    token_lp = np.zeros((B, Lp), dtype=np.float64)
    with torch.no_grad():
        for t in range(Lp):
            live = lens > t
            fed = np.where(live & (t > 0), prefix[:, t - 1] if t > 0 else end, end)
            tgt = np.where(live, prefix[:, t], -1)
            lp, states, _, _, _ = oracle.decode_step(params, cfg, fr, torch.from_numpy(fed), states, False, se, pm, pv, eps[t], obj_atts=ob)
            token_lp[:, t], _, total = SR.score_rows(lp.double().numpy(), tgt, None, end, total)
            cap = lens == t + 1
            for k in STATE_KEYS:
                out[k][cap] = states[k][cap]
            tokens[cap] = prefix[cap, t]
    return {"states": out, "tokens": tokens, "lengths": lens, "log_probs": total, "token_lp": token_lp}


def join(prefix, lengths, predictions, ctl0, log_probs, prefix_lp, end_index):
    """ssc_prefix_join restated: prefix (B, Lp), lengths (B,), predictions (B, Q, steps), ctl0 the number of valid columns or None,
    log_probs (B, Q) float32, prefix_lp (B,) float32 -> (captions (B, Q, Lp + steps) int64, total (B, Q) float32)."""
    prefix = np.asarray(prefix, dtype=np.int64)
    pred = np.asarray(predictions, dtype=np.int64)
    lps = np.asarray(log_probs, dtype=np.float32)
    B, Lp = prefix.shape
    _, Q, steps = pred.shape
    n = steps if ctl0 is None else min(max(int(ctl0), 0), steps)
    caps = np.full((B, Q, Lp + steps), end_index, dtype=np.int64)
    for b in range(B):
        k = int(lengths[b])
        caps[b, :, :k] = prefix[b, :k]
        caps[b, :, k:k + n] = pred[b, :, :n]
    total = np.where(lps <= np.float32(-1e19), lps, np.asarray(prefix_lp, dtype=np.float32)[:, None] + lps).astype(np.float32)
    return caps, total


def start_state(primed):
    """The start_state argument of oracle.cbs_search from prime()'s result (the encoder states of the eval cell are unused zeros)."""
    st = {k: v.clone() for k, v in primed["states"].items()}
    z = torch.zeros_like(st["h1"])
    st["h_encoder"], st["c_encoder"] = z, z.clone()
    return st


def step_fn(params, cfg, feats, sentiment, nimg, n_samples, eps0, eps, obj_atts=None, first_tokens=None, numpy_io=False):
    """step(tokens, state) of a search over the B = nimg * n_samples entries: oracle.decode_step in eval mode, call k fed eps0
    (k = 0) and then eps[k - 1].  first_tokens: tokens the FIRST call is fed instead of the ones it is given - for the reference
    searches that hard-wire END as their start (tests/dbsref.search, rulesref.search).  numpy_io: tokens / log-probs / states as
    NumPy arrays (float32 log-probs), for those searches."""
    B = nimg * n_samples
    calls = {"k": 0}

    def step(tokens, state):
        k = calls["k"]
        calls["k"] = k + 1
        if numpy_io:
            tokens = torch.from_numpy(np.asarray(tokens, dtype=np.int64))
            state = None if state is None else {n: torch.from_numpy(np.ascontiguousarray(v)) for n, v in state.items()}
        if k == 0 and first_tokens is not None:
            tokens = torch.as_tensor(first_tokens, dtype=torch.int64)
        rows = tokens.numel()
        fr = expand_rows(feats, nimg, rows // nimg)
        se = expand_rows(sentiment.reshape(nimg, 1), nimg, rows // nimg) if sentiment is not None else None
        ob = expand_rows(obj_atts, nimg, rows // nimg) if obj_atts is not None else None
        pm, pv = oracle.prior_from_sentiment(cfg, se, rows, fr)
        with torch.no_grad():
            lp, st, _, _, _ = oracle.decode_step(params, cfg, fr, tokens, state, False, se, pm, pv, eps0 if k == 0 else eps[k - 1],
                                                 obj_atts=ob)
        if numpy_io:
            return lp.numpy().astype(np.float32), {n: v.numpy() for n, v in st.items()}
        return lp, st

    step.calls = calls
    return step


@contextlib.contextmanager
def topk_margins():
    """Records, for every Tensor.topk(k) made inside the block (oracle.cbs_search selects with nothing else), the gap between the
    last kept and the first rejected candidate of every row, as list entries of a dict {"gaps": [...]}: float64 arrays.  A row
    whose last kept candidate is dead (<= -1e19: a masked token, a beam that does not exist) has no gap to speak of: +inf."""
    rec = {"gaps": []}
    orig = torch.Tensor.topk

    def topk(self, k, *a, **kw):
        if not a and not kw and self.size(-1) > k and self.is_floating_point():
            v = orig(self, k + 1)[0].double()
            gap = (v[..., k - 1] - v[..., k]).numpy()
            dead = (v[..., k - 1] <= -1e19).numpy()
            rec["gaps"].append(np.where(dead, np.inf, np.nan_to_num(gap, nan=np.inf, posinf=np.inf)))
        return orig(self, k, *a, **kw)

    torch.Tensor.topk = topk
    try:
        yield rec
    finally:
        torch.Tensor.topk = orig


def min_margin(rec):
    return min((float(g.min()) for g in rec["gaps"] if g.size), default=float("inf"))


def search(params, cfg, feats, sentiment, primed, n_samples, eps0, eps, beam, per_node, max_steps, fsm=None, obj_atts=None,
           early_stop=True):
    """The prefixed search: oracle.cbs_search(start = the captured tokens, start_state = the captured states, ...) over the step
    closure above.  primed None: the unprefixed search (END from zero states).  fsm (B, S, S, V) uint8 or None: the trivial machine.
    -> (predictions (B, S, beam, steps), log_probs (B, S, beam), the smallest selection margin)."""
    nimg = feats.size(0)
    B = nimg * n_samples
    end = cfg.boundary_index
    if fsm is None:
        fsm = torch.ones(B, 1, 1, cfg.vocab_size, dtype=torch.uint8)
    start = torch.full((B,), end, dtype=torch.long) if primed is None else torch.from_numpy(primed["tokens"])
    state = None if primed is None else start_state(primed)
    step = step_fn(params, cfg, feats, sentiment, nimg, n_samples, eps0, eps, obj_atts)
    with topk_margins() as rec:
        pred, lps = oracle.cbs_search(start, state, step, fsm, end, max_steps, beam, per_node, early_stop)
    return pred, lps, min_margin(rec)
