"""A float64 NumPy restatement of the clip + Adam / AdamW step that include/ssc.h states for ssc_adam_step, with the first-order
forward-error bound of its fp32 evaluation.  Shares no code with the runtime.

    coef = min(1, max_norm / (sqrt(sqnorm) * gscale + 1e-6)) * gscale
    d = g * coef;   Adam: d += wd * p;   AdamW: p *= 1 - lr * wd
    m = beta1 m + (1 - beta1) d;   v = beta2 v + (1 - beta2) d d
    p -= (lr / bc1) * (m / (sqrt(v) / sqrt(bc2) + eps)),   bc1 = 1 - beta1^step, bc2 = 1 - beta2^step

By default the scalars are taken as the device call receives them: rounded to fp32 (lr, betas, eps, weight_decay, gscale,
max_norm and the 1e-6 of the clip), then used in float64; fp32_scalars=False keeps them as given (the comparison with torch.optim).
"""
import numpy as np

U = 2.0 ** -24        # unit round-off of one fp32 operation (round to nearest)
TINY = 2.0 ** -149    # spacing of the fp32 subnormals: the absolute error of an operation whose result underflows (m: 3, v: 4 products / sums)
# Additions on the longest path of the two-pass squared-norm reduction that feeds the clip (one square, a thread's serial sum,
# two block reductions of 256 threads, 1024 partial sums four per thread): an upper bound, plus n / 2^18 for the serial part.
SQ_NORM_DEPTH = 32


def f32(x):
    return float(np.float32(x))


def sq_norm_rel_err(n):
    """Relative error bound of a squared norm of n elements summed in fp32 by the two-pass reduction (all terms >= 0)."""
    return (SQ_NORM_DEPTH + -(-int(n) // (1 << 18))) * U


def coef_of(sqnorm, gscale, max_norm, fp32_scalars=True):
    rnd = f32 if fp32_scalars else float
    gscale, max_norm = rnd(gscale), rnd(max_norm)
    return min(1.0, max_norm / (np.sqrt(float(sqnorm)) * gscale + rnd(1e-6))) * gscale


def step(p, g, m, v, sqnorm, gscale, max_norm, lr, beta1, beta2, eps, wd, decoupled, step, err_in=None, sq_rel_err=0.0,
         fp32_scalars=True):
    """One update of float64 arrays p, g, m, v (any shape).  -> dict p, m, v (new values) and Ep, Em, Ev: per element, the
    first-order bound on |fp32 evaluation - these values|.
    err_in = (Ep, Em, Ev) of the inputs (a previous step's), propagated to first order; sq_rel_err: relative error of `sqnorm`
    itself (the device's fp32 reduction against an exact one), half of which reaches coef while the clip is active.

    Rounding errors counted, u each (relative to the result of the operation):
      coef   sqrt, * gscale, + 1e-6, max_norm / ., * gscale                                              5u (+ sq_rel_err / 2)
      d      g * coef: 1;  Adam: wd * p: 1, the sum: 1                            6u|g coef| (+ u|wd p| + u|d|)
      m      beta1 * m: 1;  (1 - beta1) rounded: 1, * d: 1;  the sum: 1           u|b1 m| + 2u|(1-b1) d| + (1-b1) Ed + u|m'|
      v      beta2 * v: 1;  (1 - beta2) rounded: 1, * d: 1, * d: 1;  the sum: 1   u|b2 v| + 3u|(1-b2) d^2| + 2(1-b2)|d| Ed + u|v'|
      s      sqrt(v'): 1;  1 / sqrt(bc2) rounded: 1, the product: 1               Ev / (2 sqrt v') / sqrt(bc2) + 3u s
      den    s + eps: 1                                                           Es + u den
      q      m' / den: 1                                                          Em / den + |m'| Eden / den^2 + u|q|
      upd    lr / bc1 rounded: 1, * q: 1                                          (lr / bc1) Eq + 2u|upd|
      p'     AdamW: (1 - lr wd) rounded: 1, p * .: 1                              2u|p decay|
      p_new  p' - upd: 1                                                          Ep' + Eupd + u|p_new|
    """
    p, g, m, v = (np.asarray(x, dtype=np.float64) for x in (p, g, m, v))
    rnd = f32 if fp32_scalars else float
    lr, beta1, beta2, eps, wd = rnd(lr), rnd(beta1), rnd(beta2), rnd(eps), rnd(wd)
    Ep0, Em0, Ev0 = err_in if err_in is not None else (0.0, 0.0, 0.0)
    coef = coef_of(sqnorm, gscale, max_norm, fp32_scalars)
    e_coef = (5 * U + 0.5 * sq_rel_err) * abs(coef)
    d = g * coef
    Ed = np.abs(g) * e_coef + U * np.abs(d)
    if decoupled:
        decay = 1.0 - lr * wd
        p1 = p * decay
        Ep1 = 2 * U * np.abs(p1) + decay * Ep0
    else:
        d = d + wd * p
        Ed = Ed + U * np.abs(wd * p) + U * np.abs(d) + wd * Ep0
        p1, Ep1 = p, Ep0 + np.zeros_like(p)
    omb1, omb2 = 1.0 - beta1, 1.0 - beta2
    m1 = beta1 * m + omb1 * d
    Em = U * np.abs(beta1 * m) + 2 * U * np.abs(omb1 * d) + omb1 * Ed + U * np.abs(m1) + beta1 * Em0 + 3 * TINY
    v1 = beta2 * v + omb2 * d * d
    Ev = U * np.abs(beta2 * v) + 3 * U * omb2 * d * d + 2 * omb2 * np.abs(d) * Ed + U * v1 + beta2 * Ev0 + 4 * TINY
    bc1, bc2 = 1.0 - beta1 ** int(step), 1.0 - beta2 ** int(step)
    r = 1.0 / np.sqrt(bc2)
    root = np.sqrt(v1)
    s = root * r
    with np.errstate(divide="ignore", invalid="ignore"):
        # first order where Ev << v'; where it is not (v' at the subnormals, or 0): |sqrt(a) - sqrt(b)| <= min(|a-b| / sqrt(b), sqrt|a-b|)
        Es = np.where(Ev < 1e-3 * v1, Ev / (2 * root) * (1 + 1e-3), np.minimum(Ev / root, np.sqrt(Ev))) * r + 3 * U * s
    den = s + eps
    Eden = Es + U * den
    q = m1 / den
    Eq = Em / den + np.abs(m1) * Eden / den ** 2 + U * np.abs(q)
    step_size = lr / bc1
    upd = step_size * q
    Eupd = step_size * Eq + 2 * U * np.abs(upd)
    p2 = p1 - upd
    Ep = Ep1 + Eupd + U * np.abs(p2)
    return {"p": p2, "m": m1, "v": v1, "Ep": Ep, "Em": Em, "Ev": Ev}
