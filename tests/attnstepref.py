"""One attention step and its backward in plain torch on the CPU, the float64 reference of the attention op tests.

Forward (include/ssc.h "Bottom-up top-down attention step"; img(g) = g // rpi):
    logit[g,r] = wa . tanh(q[g] + pv[img(g),r])        x = logit * m        p = softmax(x) * m
    alpha = p / (sum_r p + 1e-13)        att = sum_r alpha_r feats_r        pool = sum_r alpha_r obj_r
Backward: torch autograd through exactly that forward - no gradient formula is written down here.  The upstream gradient of att is
datt; that of pool is dpool_a, zero-extended from its Da columns to D, plus dpool_b.  wa enters the forward once per row g, so
that its gradient is available per row (the kernels keep it per row, the caller sums over g)."""
import torch


def logits_of(q, pv, wa_rows, rpi=1):
    """q (G,A), pv (nimg,R,A), wa_rows (G,A): one copy of wa per row -> (G,R)"""
    img = torch.arange(q.size(0)) // rpi
    return (torch.tanh(q[:, None, :] + pv[img]) * wa_rows[:, None, :]).sum(-1)


def alpha_of(logits, mask, rpi=1):
    """allennlp masked_softmax: masked logits are zeroed, not -inf'd; the result is masked again and renormalised"""
    m = mask[torch.arange(logits.size(0)) // rpi]
    p = torch.softmax(logits * m, dim=1) * m
    return p / (p.sum(1, keepdim=True) + 1e-13)


def pooled(alpha, x, rpi=1):
    """sum_r alpha[g,r] x[img(g),r,:]"""
    return (alpha[:, :, None] * x[torch.arange(alpha.size(0)) // rpi]).sum(1)


def forward(q, pv, wa, mask, feats, obj=None, rpi=1, dtype=torch.float64):
    """-> dict(logits, alpha, att, pool (None without obj)), computed in `dtype`"""
    c = lambda t: None if t is None else t.to(dtype)
    q, pv, wa, mask, feats, obj = c(q), c(pv), c(wa), c(mask), c(feats), c(obj)
    logits = logits_of(q, pv, wa.expand(q.size(0), -1), rpi)
    alpha = alpha_of(logits, mask, rpi)
    return {"logits": logits, "alpha": alpha, "att": pooled(alpha, feats, rpi),
            "pool": None if obj is None else pooled(alpha, obj, rpi)}


def pool_grad(D, dpool_a=None, dpool_b=None, dtype=torch.float64):
    """the upstream gradient of pool (G,D): dpool_a (G,Da), Da <= D, zero-extended, plus dpool_b (G,D)"""
    ref = dpool_a if dpool_a is not None else dpool_b
    d = torch.zeros(ref.size(0), D, dtype=dtype)
    if dpool_a is not None:
        d[:, :dpool_a.size(1)] += dpool_a.to(dtype)
    if dpool_b is not None:
        d += dpool_b.to(dtype)
    return d


def objective(att, pool, datt, dpool):
    return (att * datt).sum() + (0.0 if pool is None else (pool * dpool).sum())


def backward(q, pv, wa, mask, feats, datt, obj=None, dpool_a=None, dpool_b=None, rpi=1, dtype=torch.float64):
    """Autograd in `dtype` through forward().  -> dict with the forward's entries and dq (G,A), dpv (nimg,R,A), dwa (A),
    dwa_rows (G,A), dalpha (G,R), dlogit (G,R)."""
    c = lambda t: None if t is None else t.detach().to(dtype)
    q, pv, mask, feats, obj, datt = c(q), c(pv), c(mask), c(feats), c(obj), c(datt)
    q.requires_grad_(True)
    pv.requires_grad_(True)
    wa_rows = c(wa).expand(q.size(0), -1).clone().requires_grad_(True)
    logits = logits_of(q, pv, wa_rows, rpi)
    alpha = alpha_of(logits, mask, rpi)
    att = pooled(alpha, feats, rpi)
    pool = None if obj is None else pooled(alpha, obj, rpi)
    dpool = None if obj is None else pool_grad(obj.size(2), dpool_a, dpool_b, dtype)
    dq, dpv, dwa_rows, dalpha, dlogit = torch.autograd.grad(objective(att, pool, datt, dpool), [q, pv, wa_rows, alpha, logits])
    return {"logits": logits.detach(), "alpha": alpha.detach(), "att": att.detach(), "pool": None if pool is None else pool.detach(),
            "dq": dq, "dpv": dpv, "dwa": dwa_rows.sum(0), "dwa_rows": dwa_rows, "dalpha": dalpha, "dlogit": dlogit}
