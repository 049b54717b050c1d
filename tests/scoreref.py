"""The definition of caption scoring, named once for the scoring tests: a float64 NumPy restatement of ssc_score_rows
(include/ssc.h) and the teacher-forced loop over oracle.decode_step that ssc_decode_score runs on the device."""
import numpy as np
import torch

import oracle
from oracle.seqcvae_oracle import zero_states


def score_rows(logits, target, last_target, end_index, row_lp=None):
    """logits (rows, V) of any float type, taken as they are and widened to float64; target / last_target (rows,) ints
    (last_target None: no row has ended).  -> (lp (rows,) float64, rank (rows,) int64, row_lp (rows,) float64 or None).
    lp = logits[target] - logsumexp(logits); rank = #{x > x_target} + #{x == x_target at a lower index}.  An ended row
    (last_target == end_index, or target < 0): lp 0, rank -1, row_lp unchanged, logits not looked at.  target >= V: lp -inf,
    rank -1, row_lp -inf."""
    x = np.asarray(logits)
    rows, V = x.shape
    target = np.asarray(target, dtype=np.int64)
    lp = np.zeros(rows, dtype=np.float64)
    rank = np.full(rows, -1, dtype=np.int64)
    out = None if row_lp is None else np.array(row_lp, dtype=np.float64)
    for r in range(rows):
        t = int(target[r])
        if t < 0 or (last_target is not None and int(last_target[r]) == end_index):
            continue
        if t >= V:
            lp[r] = -np.inf
        else:
            row = x[r].astype(np.float64)
            m = row.max()
            lp[r] = (row[t] - m) - np.log(np.exp(row - m).sum())
            rank[r] = int((row > row[t]).sum() + (row[:t] == row[t]).sum())
        if out is not None:
            out[r] += lp[r]
    return lp, rank, out


def prepare_targets(targets, n_samples, V, end_index):
    """targets (nimg, C, L) -> (tgt (L, G), fed (L, G), n_tokens (nimg, C)) with rows g = (image, caption, sample): what the
    device's preparation kernel forms.  fed[0] = END, fed[t] = target t - 1 with every id that cannot index the embedding
    replaced by END; an absent slot (first entry negative) is -1 throughout, and so is what follows a caption's end; n_tokens
    counts up to and including the first END (or out-of-range id), a negative id ends the caption before it, no END inside L: L."""
    t = np.asarray(targets, dtype=np.int64)
    nimg, C, L = t.shape
    t = np.where(t[..., :1] < 0, -1, t)
    n_tokens = np.zeros((nimg, C), dtype=np.int64)
    for i in range(nimg):
        for c in range(C):
            for k in range(L):
                x = t[i, c, k]
                if x >= 0:
                    n_tokens[i, c] += 1
                if x < 0 or x >= V or x == end_index:
                    t[i, c, k + 1:] = -1   # nothing after a caption's end is scored or fed
                    break
    tgt = np.repeat(t.reshape(nimg * C, L), n_samples, axis=0).T.copy()          # (L, G)
    fed = np.full_like(tgt, end_index)
    fed[1:] = np.where((tgt[:-1] < 0) | (tgt[:-1] >= V), end_index, tgt[:-1])
    return tgt, fed, n_tokens


def score_captions(params, cfg, feats, sentiment, targets, n_samples, eps0, eps, obj_atts=None):
    """The teacher-forced oracle: feats (nimg, R, F), sentiment (nimg,) or None, targets (nimg, C, L), eps0 (G, Z), eps (L - 1, G, Z),
    obj_atts (nimg, R, Z) for SENTIMENT_VAE = 2.  Step 0 feeds END from zero states, step t feeds target t - 1; every step's
    log-probs go through score_rows.
    -> dict(log_probs (G,), token_lp (G, L), token_rank (G, L), n_tokens (nimg, C), step_lp: list of the oracle's (G, V) log-probs)."""
    nimg, C, L = targets.shape
    rpi = C * n_samples
    G = nimg * rpi
    end = cfg.boundary_index
    tgt, fed, n_tokens = prepare_targets(targets, n_samples, cfg.vocab_size, end)
    fr = feats.unsqueeze(1).expand(nimg, rpi, *feats.shape[1:]).reshape(G, *feats.shape[1:])
    se = sentiment.reshape(nimg, 1).expand(nimg, rpi).reshape(G, 1) if sentiment is not None else None
    ob = obj_atts.unsqueeze(1).expand(nimg, rpi, *obj_atts.shape[1:]).reshape(G, *obj_atts.shape[1:]) if obj_atts is not None else None
    pm, pv = oracle.prior_from_sentiment(cfg, se, G, fr)
    states = zero_states(G, cfg.hidden_size, fr)
    total = np.zeros(G, dtype=np.float64)
    token_lp = np.zeros((G, L), dtype=np.float64)
    token_rank = np.full((G, L), -1, dtype=np.int64)
    step_lp = []
    with torch.no_grad():
        for t in range(L):
            e = eps0 if t == 0 else eps[t - 1]
            lp, states, _, _, _ = oracle.decode_step(params, cfg, fr, torch.from_numpy(fed[t]), states, False, se, pm, pv, e, obj_atts=ob)
            step_lp.append(lp.double().numpy())
            token_lp[:, t], token_rank[:, t], total = score_rows(step_lp[-1], tgt[t], None if t == 0 else fed[t], end, total)
    return {"log_probs": total, "token_lp": token_lp, "token_rank": token_rank, "n_tokens": n_tokens, "step_lp": step_lp}
