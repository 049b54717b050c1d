"""Float64 restatement of the distilled vocabulary cross-entropy (include/ssc.h, ssc_distill; ssc_ce_fwd_distill /
ssc_ce_bwd_distill): time-major student logits x (T, B, V), teacher scores s (T, B, V) - raw logits or log-probs, entries may be
-inf -, targets (T, B) int64, loss weights w (T, B), smoothing eps in [0, 1), mixing weight alpha in [0, 1], temperature tau > 0.

    q      = softmax(s / tau),  p_tau = softmax(x / tau)
    kd_row = tau^2 sum_{v: q[v] > 0} q[v] (log q[v] - log p_tau[v])
    row    = (1 - alpha) row(eps) + alpha kd_row                       row(eps): smoothref.rows
    loss_b = n_b sum_t w row / (n_b + 1e-13),  kd_b = n_b sum_t w kd_row / (n_b + 1e-13),  n_b = sum_t w
    dx[v]  = ((1 - alpha) (softmax(x)[v] - (1 - eps) [v == y] - eps / V) + alpha tau (p_tau[v] - q[v])) gl_b w n_b / (n_b + 1e-13)

The teacher is a constant (it is detached here).  Everything is differentiable torch in float64, so it also serves as the loss of
an autograd reference."""
import torch

import smoothref

ZERO = torch.zeros((), dtype=torch.float64)


def kd_rows(logits, scores, tau):
    """(..., V), (..., V) -> (...) float64: tau^2 KL(softmax(s / tau) || softmax(x / tau)) of every row; q = 0 entries contribute
    nothing whatever the student holds there."""
    x = logits.double()
    s = scores.detach().double()
    logq = torch.log_softmax(s / tau, dim=-1)
    logp = torch.log_softmax(x / tau, dim=-1)
    q = logq.exp()
    pos = q != 0          # (a NaN in the teacher's row makes every q of it NaN: the row is NaN, not skipped)
    term = q * (torch.where(pos, logq, ZERO) - torch.where(pos, logp, ZERO))
    return (tau * tau) * torch.where(pos, term, ZERO).sum(-1)


def _live(t, w):
    return torch.where((w != 0).unsqueeze(-1), t.double(), ZERO)


def rows(logits, scores, targets, eps, alpha, tau):
    """-> (row, kd_row), each (...) float64."""
    kd = kd_rows(logits, scores, tau)
    hard = smoothref.rows(logits, targets, eps)
    return ((1.0 - alpha) * hard + alpha * kd) if alpha < 1.0 else kd, kd


def loss(logits, scores, targets, w, eps, alpha, tau):
    """(T, B, V), (T, B, V), (T, B), (T, B) -> (loss (B,), kd (B,)) float64.  Rows with w = 0 contribute nothing whatever either
    matrix holds."""
    w = w.double()
    r, kd = rows(_live(logits, w), _live(scores, w), targets, eps, alpha, tau)
    n = w.sum(0)
    return n * ((w * r).sum(0) / (n + 1e-13)), n * ((w * kd).sum(0) / (n + 1e-13))


def dlogits(logits, scores, targets, w, gl, eps, alpha, tau):
    """The closed form of d(sum_b gl_b loss_b) / dlogits, (T, B, V) float64; zero rows where w = 0."""
    w = w.double()
    live = (w != 0).unsqueeze(-1)
    x, s = _live(logits, w), _live(scores, w)
    V = x.size(-1)
    n = w.sum(0)
    coef = gl.double().unsqueeze(0) * w * (n / (n + 1e-13)).unsqueeze(0)
    onehot = torch.zeros_like(x).scatter_(-1, targets.long().unsqueeze(-1), 1.0)
    hard = torch.softmax(x, dim=-1) - (1.0 - eps) * onehot - eps / V
    soft = tau * (torch.softmax(x / tau, dim=-1) - torch.softmax(s / tau, dim=-1))
    d = ((1.0 - alpha) * hard + alpha * soft) * coef.unsqueeze(-1)
    return torch.where(live, d, ZERO)
