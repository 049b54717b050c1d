"""Float64 restatement of token-level unlikelihood training in the vocabulary cross-entropy (include/ssc.h, ssc_unlikelihood;
ssc_ce_fwd_unlike / ssc_ce_bwd_unlike): time-major logits x (T, B, V), targets y (T, B) int64, loss weights w (T, B), smoothing eps
in [0, 1), weight alpha >= 0, clamp delta in (0, 1).

    C(t,b) = {y[s,b] : s < t, w[s,b] != 0} - {y[t,b]}                                     (plain Python sets here)
    ul_row = - sum_{c in C} log max(1 - p[c], delta),  p = softmax(x)
    g_c    = p[c] / (1 - p[c]) where 1 - p[c] > delta, else 0;  G = sum_c g_c
    row    = row(eps) + alpha ul_row                                                      row(eps): smoothref.rows
    loss_b = n_b sum_t w row / (n_b + 1e-13),  ul_b = n_b sum_t w ul_row / (n_b + 1e-13),  n_b = sum_t w
    dx[v]  = (p[v] - (1 - eps) [v == y] - eps / V - alpha G p[v] + alpha g_v [v in C]) gl_b w n_b / (n_b + 1e-13)

1 - p[c] is formed as -expm1(x[c] - lse), which keeps its digits when p[c] is small.  Everything is differentiable torch in float64
(the clamp is torch.clamp: no gradient below it), so it also serves as the loss of an autograd reference."""
import torch

import smoothref

ZERO = torch.zeros((), dtype=torch.float64)


def candidates(targets, w):
    """-> c[t][b]: the candidate set of every row as a sorted list of ints (empty where w[t,b] = 0: such a row has no term)."""
    T, B = targets.shape
    y, live = targets.tolist(), (w != 0).tolist()
    out = []
    for t in range(T):
        out.append([])
        for b in range(B):
            c = {y[s][b] for s in range(t) if live[s][b]} - {y[t][b]} if live[t][b] else set()
            out[t].append(sorted(c))
    return out


def cand_mask(targets, w, V):
    """(T, B, V) bool: v in C(t,b)."""
    T, B = targets.shape
    m = torch.zeros(T, B, V, dtype=torch.bool)
    for t, row in enumerate(candidates(targets, w)):
        for b, c in enumerate(row):
            if c:
                m[t, b, c] = True
    return m


def _live(t, w):
    return torch.where((w != 0).unsqueeze(-1), t.double(), ZERO)


def one_minus_p(x):
    """(..., V) float64 -> 1 - softmax(x), elementwise, as -expm1(x - lse)."""
    return -torch.expm1(x - torch.logsumexp(x, dim=-1, keepdim=True))


def margins(logits, targets, w):
    """1 - p of every candidate of every row with w != 0, as one flat float64 tensor (empty when there is none)."""
    w = w.double()
    x = _live(logits, w)
    return one_minus_p(x)[cand_mask(targets, w, x.size(-1))]


def check_margins(logits, targets, w, delta, lo=0.05):
    """The condition under which float32 decides the clamp as float64 does: every candidate's 1 - p is >= lo or <= delta / 100.
    -> (the smallest unclamped margin, the number of clamped candidates); an AssertionError otherwise."""
    m = margins(logits, targets, w)
    clamped = m <= delta / 100.0
    free = m[~clamped]
    assert bool((free >= lo).all()), f"a candidate's 1 - p lies in ({delta / 100.0}, {lo}): {free.min().item()}"
    return (free.min().item() if free.numel() else float("inf")), int(clamped.sum())


def ul_rows(logits, targets, w, delta):
    """(T, B, V), (T, B), (T, B) -> (ul_row (T, B), G (T, B)) float64; rows with w = 0 hold 0."""
    w = w.double()
    x = _live(logits, w)
    mask = cand_mask(targets, w, x.size(-1))
    om = one_minus_p(x)
    term = -torch.log(torch.clamp(om, min=delta))
    g = torch.where(om > delta, (1.0 - om) / om, ZERO)
    return torch.where(mask, term, ZERO).sum(-1), torch.where(mask, g.detach(), ZERO).sum(-1)


def rows(x, y, w, eps, alpha, delta):
    """-> (row, ul_row, G), each (T, B) float64; logits of rows with w = 0 are never looked at."""
    w = w.double()
    ul, G = ul_rows(x, y, w, delta)
    return smoothref.rows(_live(x, w), y, eps) + alpha * ul, ul, G


def loss(x, y, w, eps, alpha, delta):
    """-> (loss (B,), ul (B,)) float64."""
    w = w.double()
    r, ul, _ = rows(x, y, w, eps, alpha, delta)
    n = w.sum(0)
    return n * ((w * r).sum(0) / (n + 1e-13)), n * ((w * ul).sum(0) / (n + 1e-13))


def dlogits(x, y, w, gl, eps, alpha, delta):
    """The closed form of d(sum_b gl_b loss_b) / dlogits, (T, B, V) float64; zero rows where w = 0."""
    w = w.double()
    live = (w != 0).unsqueeze(-1)
    xl = _live(x, w)
    V = xl.size(-1)
    n = w.sum(0)
    coef = gl.double().unsqueeze(0) * w * (n / (n + 1e-13)).unsqueeze(0)
    onehot = torch.zeros_like(xl).scatter_(-1, y.long().unsqueeze(-1), 1.0)
    p = torch.softmax(xl, dim=-1)
    om = one_minus_p(xl)
    g = torch.where(cand_mask(y, w, V) & (om > delta), p / om, ZERO)
    G = g.sum(-1, keepdim=True)
    d = (p - (1.0 - eps) * onehot - eps / V - alpha * G * p + alpha * g) * coef.unsqueeze(-1)
    return torch.where(live, d, ZERO)


def dlogits_autograd(x, y, w, gl, eps, alpha, delta):
    """The same through autograd of loss()."""
    xv = x.double().clone().requires_grad_(True)
    l, _ = loss(xv, y, w, eps, alpha, delta)
    (l * gl.double()).sum().backward()
    return xv.grad


def train_reference(cfg, params, feats, caps, senti, eps_noise, label_smoothing, alpha, delta, free_bits_kld=None):
    """The train-step objective on the CPU oracle's logits, as tests/test_label_smoothing_gpu.py::medium builds its own: the
    oracle's forward with its per-step logits in the autograd graph, loss() of them, the gradients of mean(loss) + mean(kld) /
    kld_weight.  free_bits_kld: None, or a function out -> the (B,) KL that enters the objective instead of out["kld"]."""
    import oracle
    p = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    out = oracle.train_forward(p, cfg, feats, caps, senti, eps_noise, return_steps=True)
    logits = torch.stack([s["logits"] for s in out["steps"]], 0)
    targets = out["tokens"][:, 1:].t().contiguous()
    w = (targets != cfg.pad_index).double()
    l, ul = loss(logits, targets, w, label_smoothing, alpha, delta)
    kld = out["kld"].double() if free_bits_kld is None else free_bits_kld(out)
    (l.mean() + kld.mean() / cfg.kld_weight).backward()
    grads = {k: v.grad.clone() for k, v in p.items()}
    margin = check_margins(logits.detach(), targets, w, delta)
    return dict(loss=l.detach(), ul=ul.detach(), kld=kld.detach(), nll=out["loss"].detach(), grads=grads, targets=targets, w=w,
                logits=logits.detach(), margin=margin)
