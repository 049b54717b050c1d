"""Restatements for the scheduled-sampling tests (include/ssc.h: ssc_sched_sampling).

1. The decision: u[t, b] from Philox4x32-10 (tests/samplerref.py) with key = seed and counter (0, t, b, 1), word 0, mapped to (0, 1) as
   the samplers map it; an ELIGIBLE row (w[t, b] = w[t-1, b] = 1, t >= 1) fires iff u < prob, compared in float32.  The word of a
   fired row is samplerref's draw (filter in float64, Gumbel-max in float32) from the logits row (t-1, b) at step t, row id b.
2. A train forward that takes the fed ids as GIVEN: a loop over oracle.decode_step with in[t] as inputs and tok[t+1] as targets, loss
   and KL formed as oracle.train_forward forms them, differentiable.  With in = tok[:-1] it is oracle.train_forward."""
import numpy as np
import torch

import oracle
import samplerref as S

KIND_NAME = {0: "multinomial", 1: "top-k", 2: "top-p"}


def uniforms(seed, T, B):
    """u (T, B) float32, exact: the odd multiples of 2^-24."""
    ctr = np.zeros((T, B, 4), dtype=np.uint32)
    ctr[..., 1] = np.arange(T, dtype=np.uint32)[:, None]
    ctr[..., 2] = np.arange(B, dtype=np.uint32)[None, :]
    ctr[..., 3] = 1
    x = S.philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32))[..., 0]
    return (((x >> np.uint32(9)) << np.uint32(1)) | np.uint32(1)).astype(np.float32) * np.float32(2.0 ** -24)


def uniforms_step(seed, step, rows):
    """u (rows,) of one step (the kernel's view: row r is batch entry r)."""
    return uniforms(seed, step + 1, rows)[step]


def eligible(w):
    """w (T, B) 0/1 -> (T, B) bool: t >= 1, the step has a target and so had the previous one."""
    w = np.asarray(w) != 0
    e = np.zeros_like(w)
    e[1:] = w[1:] & w[:-1]
    return e


def fires(u, elig, prob):
    return np.asarray(elig) & (np.asarray(u, dtype=np.float32) < np.float32(prob))


def draw_row(logits_row, kind, k, p, T, seed, step, b):
    """-> (token, unambiguous): the word a fired row is fed.  unambiguous = False where float32 / float64 rounding may decide - the
    top two perturbed scores within 1e-5 (the bound tests/test_sampling_gpu.py uses), or a top-p cut within 1e-6 of a token's mass
    ahead."""
    x = np.asarray(logits_row, dtype=np.float32)
    lp = x.astype(np.float64)
    lp = lp - (lp.max() + np.log(np.exp(lp - lp.max()).sum()))
    name = KIND_NAME[kind]
    ahead = None
    kept = np.ones(x.shape[0], dtype=bool)   # (the kept SET, whatever mass a tempered tail keeps in float64)
    if name == "top-k" and k < x.shape[0]:
        kept[:] = False
        kept[np.argsort(-lp, kind="stable")[:k]] = True
    elif name == "top-p" and p < 1.0:
        _, ahead = S.filter_dist(lp, name, k, p, T)
        kept = ahead < p
        kept[np.argsort(-lp, kind="stable")[0]] = True
    tok, sc = S.draw(x, kept, T, seed, step, b)
    top2 = np.sort(sc[np.isfinite(sc)])[-2:]
    sure = not (len(top2) == 2 and top2[1] - top2[0] <= 1e-5)
    if ahead is not None and (np.abs(ahead - p) < 1e-6).any():
        sure = False
    return tok, sure


def mix_rows(logits, truth, w_prev, w_cur, step, prob, kind, k, p, T, seed):
    """One step of the kernel on (rows, V) logits -> (tok (rows,) int64, fed (rows,) bool, sure (rows,) bool)."""
    rows = len(truth)
    u = uniforms_step(seed, step, rows)
    elig = (np.asarray(w_prev) != 0) & (np.asarray(w_cur) != 0)
    fed = fires(u, elig, prob)
    tok = np.array(truth, dtype=np.int64)
    sure = np.ones(rows, dtype=bool)
    for r in np.nonzero(fed)[0]:
        tok[r], sure[r] = draw_row(np.asarray(logits[r]), kind, k, p, T, seed, step, int(r))
    return tok, fed, sure


def tokens_and_weights(cfg, caption_tokens):
    """tok (L+2, B) int64 time-major and w (T, B) float, as the train step forms them."""
    tokens, _ = oracle.add_sentence_boundary_token_ids(caption_tokens, caption_tokens != cfg.pad_index, cfg.boundary_index,
                                                       cfg.boundary_index)
    tok = tokens.t().contiguous()
    return tok, (tok[1:] != cfg.pad_index).float()


def train_forward_fed(params, cfg, feats, caption_tokens, sentiment, eps, fed_tokens, return_steps=False, obj_atts=None):
    """oracle.train_forward with the inputs of the attention LSTM given: fed_tokens (T, B) int64 (constants).  Targets, weights,
    loss and KL are those of oracle.train_forward."""
    B = feats.size(0)
    prior_mean, prior_var = oracle.prior_from_sentiment(cfg, sentiment, B, feats)
    tokens, _ = oracle.add_sentence_boundary_token_ids(caption_tokens, caption_tokens != cfg.pad_index, cfg.boundary_index,
                                                       cfg.boundary_index)
    tokens_mask = tokens != cfg.pad_index
    T = tokens.size(1) - 1
    assert tuple(fed_tokens.shape) == (T, B)
    states, cache = None, {}
    step_logits, step_klds, steps = [], [], []
    for t in range(T):
        logits, states, mean, log_var, alpha, prior_mean = oracle.decode_step(
            params, cfg, feats, fed_tokens[t], states, True, sentiment, prior_mean, prior_var, eps[t], cache, obj_atts, True)
        step_klds.append(oracle.kld_step(cfg, mean, log_var, prior_mean, prior_var).unsqueeze(1))
        step_logits.append(logits.unsqueeze(1))
        if return_steps:
            steps.append({"mean": mean, "log_var": log_var, "logits": logits, "prior_mean": prior_mean})
    logits = torch.cat(step_logits, 1)
    klds = torch.cat(step_klds, 1) * tokens_mask[:, 1:].float()
    tmask = tokens_mask[:, 1:].contiguous()
    lengths = tmask.sum(-1).float()
    loss = lengths * oracle.sequence_cross_entropy_with_logits(logits, tokens[:, 1:].contiguous(), tmask)
    out = {"loss": loss, "kld": klds.sum(1)}
    if return_steps:
        out["steps"] = steps
        out["tokens"] = tokens
        out["logits"] = logits
    return out
