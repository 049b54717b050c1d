"""Float64 restatement of the label-smoothed vocabulary cross-entropy (include/ssc.h, ssc_ce_fwd_smooth / ssc_ce_bwd_smooth):
time-major logits (T, B, V), targets (T, B) int64, loss weights w (T, B), smoothing eps in [0, 1).

    row(eps) = lse(x) - (1 - eps) x[y] - (eps / V) sum_v x[v]              (torch's label_smoothing: uniform over all V classes)
    loss_b   = n_b sum_t w row(eps) / (n_b + 1e-13),  n_b = sum_t w
    dx[v]    = (softmax(x)[v] - (1 - eps) [v == y] - eps / V) gl_b w n_b / (n_b + 1e-13)

Everything here is differentiable torch in float64, so it also serves as the loss of an autograd reference."""
import torch


def rows(logits, targets, eps):
    """(..., V), (...) -> (...) float64: row(eps) of every row."""
    x = logits.double()
    V = x.size(-1)
    lse = torch.logsumexp(x, dim=-1)
    xy = x.gather(-1, targets.long().unsqueeze(-1)).squeeze(-1)
    return lse - (1.0 - eps) * xy - (eps / V) * x.sum(-1)


def loss(logits, targets, w, eps):
    """(T, B, V), (T, B), (T, B) -> (B,) float64.  Rows with w = 0 contribute nothing whatever their logits hold."""
    w = w.double()
    r = rows(torch.where((w != 0).unsqueeze(-1), logits.double(), torch.zeros((), dtype=torch.float64)), targets, eps)
    n = w.sum(0)
    return n * ((w * r).sum(0) / (n + 1e-13))


def dlogits(logits, targets, w, gl, eps):
    """The closed form of d(sum_b gl_b loss_b) / dlogits, (T, B, V) float64; zero rows where w = 0."""
    w = w.double()
    live = (w != 0).unsqueeze(-1)
    x = torch.where(live, logits.double(), torch.zeros((), dtype=torch.float64))
    V = x.size(-1)
    n = w.sum(0)
    coef = gl.double().unsqueeze(0) * w * (n / (n + 1e-13)).unsqueeze(0)
    onehot = torch.zeros_like(x).scatter_(-1, targets.long().unsqueeze(-1), 1.0)
    d = (torch.softmax(x, dim=-1) - (1.0 - eps) * onehot - eps / V) * coef.unsqueeze(-1)
    return torch.where(live, d, torch.zeros((), dtype=torch.float64))
