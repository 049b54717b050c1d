"""Float64 reference of the free-bits floor on the KL of the latent head (include/ssc.h: ssc_free_bits), differentiable.

With k[t, b, j] the per-element closed-form KL (-0.5 times the bracket of oracle.kld_step), w[t, b] the step weights and lam the floor:
  mode 1 "element": kld_b = sum_t w sum_j max(lam, k)        gate[t, b, j] = k > lam
  mode 2 "step":    kld_b = sum_t w max(lam, sum_j k)        gate[t, b]    = sum_j k > lam
  mode 3 "dim":     kld_b = sum_j (gate_j ? S_bj : lam)      gate[j]       = K_j > lam,  S = sum_t w k,  K = mean_b S
max is torch.where(x > lam, x, lam): the comparison is strict, a term AT the floor is closed.  The gates are constants of the
graph, so autograd through `floored` gives the gated gradients; `dlatent` is the same in closed form."""
import torch

MODES = {"element": 1, "step": 2, "dim": 3}


def k_elem(mean, log_var, prior_mean, prior_var, kld_mode):
    """(..., Z) per-element KL; kld_mode 0: against N(0, 1) (prior_mean / prior_var unused), else against N(prior_mean, prior_var)
    with the reference's + 1e-5 in the denominator.  prior_var: a float."""
    mean, log_var = mean.double(), log_var.double()
    if kld_mode == 0:
        return -0.5 * (1 + log_var - mean.pow(2) - log_var.exp())
    pv = torch.as_tensor(prior_var, dtype=torch.float64)
    return -0.5 * (1 + log_var - pv.log() - ((mean - prior_mean.double()).pow(2) + log_var.exp()) / (pv + 0.00001))


def raw(k, w):
    """(B,) sum_t w sum_j k."""
    return (w.double() * k.sum(-1)).sum(0)


def compared(k, w, mode):
    """The values the mode holds against the floor: k (T, B, Z), the step sums (T, B) or K (Z)."""
    mode = MODES.get(mode, mode)
    if mode == 1:
        return k
    if mode == 2:
        return k.sum(-1)
    return (w.double().unsqueeze(-1) * k).sum(0).mean(0)


def floored(k, w, lam, mode):
    """-> (kld (B,), gate (bool; shape by mode), K (Z,) or None)."""
    mode = MODES.get(mode, mode)
    w = w.double()
    lam_t = torch.as_tensor(float(lam), dtype=torch.float64)
    if mode == 1:
        gate = k.detach() > lam_t
        return (w * torch.where(gate, k, lam_t).sum(-1)).sum(0), gate, None
    if mode == 2:
        s = k.sum(-1)
        gate = s.detach() > lam_t
        return (w * torch.where(gate, s, lam_t)).sum(0), gate, None
    if mode == 3:
        S = (w.unsqueeze(-1) * k).sum(0)
        K = S.mean(0)
        gate = K.detach() > lam_t
        return torch.where(gate.unsqueeze(0), S, lam_t).sum(1), gate, K.detach()
    raise ValueError(mode)


def gate_full(gate, shape):
    """The gate of any mode broadcast to (T, B, Z)."""
    T, B, Z = shape
    if gate.dim() == 3:
        return gate
    if gate.dim() == 2:
        return gate.unsqueeze(-1).expand(T, B, Z)
    return gate.view(1, 1, Z).expand(T, B, Z)


def dlatent(mean, log_var, prior_mean, prior_var, kld_mode, w, gk, gate):
    """Closed-form gradient of sum_b gk_b kld_b with respect to mean, log_var and prior_mean, all (T, B, Z); gate: as `floored`
    returns it (all True: the raw KL).  The prior-mean gradient is zero for kld_mode 0."""
    mean, log_var = mean.double(), log_var.double()
    g = gate_full(gate, mean.shape).double() * (gk.double().view(1, -1) * w.double()).unsqueeze(-1)
    if kld_mode == 0:
        return g * mean, g * -0.5 * (1 - log_var.exp()), torch.zeros_like(mean)
    den = float(prior_var) + 0.00001
    dm = mean - prior_mean.double()
    return g * dm / den, g * -0.5 * (1 - log_var.exp() / den), -g * dm / den


def pick_lambda(values, lo=0.3, hi=0.7):
    """The floor no gate is a coin toss at: the midpoint of the widest gap among the sorted `values` between their `lo` and `hi`
    quantile -> (lam, half the gap).  At least one value lies on either side."""
    v = torch.sort(values.detach().double().flatten()).values
    n = v.numel()
    a, b = int(lo * (n - 1)), max(int(hi * (n - 1)), int(lo * (n - 1)) + 1)
    if b >= n:
        raise ValueError("pick_lambda needs at least two values")
    gaps = v[a + 1:b + 1] - v[a:b]
    i = int(torch.argmax(gaps))
    return float((v[a + i] + v[a + i + 1]) / 2), float(gaps[i] / 2)
