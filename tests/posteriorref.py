"""The definition of posterior scoring, named once for the posterior tests: a float64 restatement of ssc_posterior_rows
(include/ssc.h), the bounds formed from the log importance weights, and the whole path on the float64 oracle
(oracle.train_forward(..., return_steps=True)).

Rows are (image, caption, sample); step t = 0..T-1; w_tb the train forward's step weight.  The generative prior is the one the
eval decode samples, p(z_t) = N(pm_tb, pv), the posterior q(z_t | x) = N(mu_tb, exp(lv_tb)), z = eps * exp(lv / 2) + mu:
    log_ratio_b = sum_t w_tb sum_j 1/2 (eps^2 + lv - log pv - (z - pm)^2 / pv) = sum_t w_tb [log p(z_t) - log q(z_t | x)]
    log_w_b     = -nll_b + log_ratio_b
    kl_b        = the training KL in the formula of kld_mode (0: against N(0, 1); 1, 2: against N(pm, pv), with pv + 1e-5 as its
                  denominator), split by latent dimension (kl_dim) and by step (step_kl)."""
import math

import torch

import oracle


def posterior_rows(mu, lv, z, eps, w, pm, kld_mode, prior_var):
    """mu / lv / z / eps (T, B, Z), w (T, B), pm (T, B, Z), (B,) - a value per row - or None (0); any float type, widened to float64.
    A step with w == 0 contributes nothing, whatever its entries hold (NaN included).
    -> dict of float64 tensors: log_ratio (B), kl (B), kl_dim (B, Z), step_kl (T, B), step_ratio (T, B) and, for error bounds, the
    sums of the ABSOLUTE parts of the terms behind each of them under the same names with an `abs_` prefix:
    w 1/2 (eps^2 + |lv| + |log pv| + d^2 / pv) for the ratio, w 1/2 (1 + |lv| + mu^2 + exp(lv)) (mode 0) or
    w 1/2 (1 + |lv| + |log pv| + ((mu - pm)^2 + exp(lv)) / (pv + 1e-5)) for the KL."""
    mu, lv, z, eps, w = (torch.as_tensor(x).double() for x in (mu, lv, z, eps, w))
    T, B, Z = mu.shape
    if pm is None:
        pm = torch.zeros(T, B, Z, dtype=torch.float64)
    pm = torch.as_tensor(pm).double()
    if pm.dim() == 1:
        pm = pm.view(1, B, 1).expand(T, B, Z)
    pv = float(prior_var)
    lpv = math.log(pv)
    live = (w != 0).unsqueeze(-1)
    wt = w.unsqueeze(-1)
    d = z - pm
    ratio = 0.5 * (eps ** 2 + lv - lpv - d ** 2 / pv)
    ratio_abs = 0.5 * (eps ** 2 + lv.abs() + abs(lpv) + d ** 2 / pv)
    if kld_mode == 0:
        kl = -0.5 * (1 + lv - mu ** 2 - lv.exp())
        kl_abs = 0.5 * (1 + lv.abs() + mu ** 2 + lv.exp())
    else:
        kl = -0.5 * (1 + lv - lpv - ((mu - pm) ** 2 + lv.exp()) / (pv + 0.00001))
        kl_abs = 0.5 * (1 + lv.abs() + abs(lpv) + ((mu - pm) ** 2 + lv.exp()) / (pv + 0.00001))
    zero = torch.zeros((), dtype=torch.float64)
    ratio, ratio_abs, kl, kl_abs = (torch.where(live, wt * x, zero) for x in (ratio, ratio_abs, kl, kl_abs))
    out = {}
    for name, x in (("", (ratio, kl)), ("abs_", (ratio_abs, kl_abs))):
        r, k = x
        out[name + "log_ratio"] = r.sum((0, 2))
        out[name + "kl"] = k.sum((0, 2))
        out[name + "kl_dim"] = k.sum(0)
        out[name + "step_kl"] = k.sum(2)
        out[name + "step_ratio"] = r.sum(2)
    return out


def bounds(log_w):
    """log_w (..., K) -> (elbo = mean_k, iwae = logsumexp_k - log K, ess = exp(2 lse(log_w) - lse(2 log_w))), float64."""
    log_w = torch.as_tensor(log_w).double()
    lse = torch.logsumexp(log_w, -1)
    return log_w.mean(-1), lse - math.log(log_w.size(-1)), torch.exp(2 * lse - torch.logsumexp(2 * log_w, -1))


def kl_closed_form(mu, lv, pm, prior_var):
    """KL(N(mu, exp(lv)) || N(pm, pv)) summed over the last axis, float64 (no 1e-5 in the denominator: the exact one)."""
    mu, lv, pm = (torch.as_tensor(x).double() for x in (mu, lv, pm))
    pv = float(prior_var)
    return 0.5 * (math.log(pv) - lv + (lv.exp() + (mu - pm) ** 2) / pv - 1).sum(-1)


def kld_mode_of(cfg):
    return 0 if cfg.sentiment_vae == 0 else (2 if cfg.sentiment_vae == 2 and not cfg.simple_vae else 1)


def posterior_forward(params, cfg, feats, caps, sentiment, eps, obj_atts=None):
    """The whole path in float64 on the oracle: feats (B, R, F), caps (B, L) 0-padded, sentiment (B, 1) or None, eps (L + 1, B, Z).
    -> posterior_rows' dict plus nll (B), kld (B) - the forward's own - , log_w (B), w (T, B), and mu / lv / z / pm (T, B, Z)."""
    dd = lambda x: None if x is None else x.double()
    p64 = {k: v.double() for k, v in params.items()}
    B = feats.size(0)
    sent = dd(sentiment.reshape(B, 1)) if sentiment is not None else torch.zeros(B, 1, dtype=torch.float64)
    fwd = oracle.train_forward(p64, cfg, dd(feats), caps, sent, dd(eps), return_steps=True, obj_atts=dd(obj_atts))
    steps = fwd["steps"]
    mu = torch.stack([s["mean"] for s in steps])
    lv = torch.stack([s["log_var"] for s in steps])
    pm = torch.stack([s["prior_mean"] for s in steps])
    z = eps.double() * (lv / 2).exp() + mu
    w = (fwd["tokens"][:, 1:] != cfg.pad_index).double().t()
    out = posterior_rows(mu, lv, z, eps, w, pm, kld_mode_of(cfg), cfg.prior_std ** 2)
    out.update(nll=fwd["loss"], kld=fwd["kld"], log_w=out["log_ratio"] - fwd["loss"], w=w, mu=mu, lv=lv, z=z, pm=pm)
    return out
