"""Ensemble decoding (include/ssc.h: ssc_ensemble_rows_desc, ssc_ensemble_desc) restated in float64 numpy, and the oracle's eval
decode step run under several parameter sets with the results combined - the step function of an ensemble search on the CPU
(tests/dbsref.search with one group and strength 0 for the trivial machine, oracle.cbs_search for a machine)."""
import numpy as np
import torch

import oracle
from oracle.seqcvae_oracle import zero_states

MODES = {"prob": 0, "logprob": 1}


def normalise(weights, M):
    """The members' weights as the driver takes them: positive, any scale (None: uniform) -> float64, summing to 1."""
    w = np.full(M, 1.0 / M) if weights is None else np.asarray(weights, dtype=np.float64)
    assert w.shape == (M,) and (w > 0).all() and np.isfinite(w).all()
    return w / w.sum()


def log_softmax64(x):
    x = np.asarray(x, dtype=np.float64)
    m = x.max(-1, keepdims=True)
    return x - m - np.log(np.exp(x - m).sum(-1, keepdims=True))


def combine_log_probs(lp, weights, mode):
    """lp (M, rows, V) float64 log-probs of the members, weights (M) summing to 1 -> (rows, V) float64.
    mode 0: log sum_m w_m exp(lp_m); mode 1: sum_m w_m lp_m, renormalised."""
    lp = np.asarray(lp, dtype=np.float64)
    w = np.asarray(weights, dtype=np.float64).reshape(-1, 1, 1)
    if mode == 0:
        y = lp + np.log(w)
        mx = y.max(0)
        with np.errstate(invalid="ignore"):
            out = mx + np.log(np.exp(y - mx).sum(0))
        return np.where(np.isneginf(mx), -np.inf, out)
    s = (w * lp).sum(0)
    mx = s.max(-1, keepdims=True)
    return s - mx - np.log(np.exp(s - mx).sum(-1, keepdims=True))


def combine(logits, weights, mode):
    """logits (M, rows, V) raw logits -> the ensemble's log-probs (rows, V), float64."""
    return combine_log_probs(log_softmax64(logits), weights, mode)


def oracle_step_fn(cfg, params_list, weights, mode, feats, senti, eps0, eps, nimg, ns, numpy_io=True):
    """step(tokens, states) for a search over the ensemble: oracle.decode_step under every parameter set - each member on its own
    states, all on the same noise, sentiment and features -, combined in float64.  The states of the members travel in one dict
    under the keys "<member>/<state>", rows leading, so that a search re-orders every member's states alike.
    numpy_io: tokens / log-probs / states as numpy arrays (float32 log-probs: tests/dbsref.search); otherwise torch tensors
    (oracle.cbs_search)."""
    M = len(params_list)
    w = normalise(weights, M)
    B = nimg * ns
    R_ = feats.size(1)
    sent_b = senti.view(nimg, 1).expand(nimg, ns).reshape(B, 1)
    t_of = {"t": 0}

    def step(tokens, states):
        tokens = torch.as_tensor(tokens)
        rows = tokens.shape[0]
        fr = feats.unsqueeze(1).expand(nimg, rows // nimg, R_, feats.size(2)).reshape(rows, R_, -1)
        se = sent_b.repeat_interleave(rows // B, 0)
        pm, pv = oracle.prior_from_sentiment(cfg, se, rows, fr)
        t = t_of["t"]
        e = eps0 if t == 0 else eps[t - 1]
        t_of["t"] = t + 1
        lps, new = [], {}
        for m, params in enumerate(params_list):
            if states is None:
                st = zero_states(rows, cfg.hidden_size, fr)
            else:
                st = {k.split("/", 1)[1]: torch.as_tensor(np.ascontiguousarray(v) if numpy_io else v)
                      for k, v in states.items() if k.startswith(f"{m}/")}
            with torch.no_grad():
                lp, st, _, _, _ = oracle.decode_step(params, cfg, fr, tokens, st, False, se, pm, pv, e)
            lps.append(lp.double().numpy())
            for k, v in st.items():
                new[f"{m}/{k}"] = v.numpy() if numpy_io else v
        out = combine_log_probs(np.stack(lps), w, mode).astype(np.float32)
        return (out, new) if numpy_io else (torch.from_numpy(out), new)

    return step
