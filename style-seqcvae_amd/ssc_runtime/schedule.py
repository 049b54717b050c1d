"""KL annealing: the weight beta of the KL term as a pure function of the iteration number (OPTIM.KL_ANNEAL*).  A resumed run
needs no state beyond the iteration it resumes at."""
KINDS = ("none", "linear", "cyclical")


def kl_beta(iteration: int, kind: str = "none", iters: int = 1, ratio: float = 0.5, start: float = 0.0) -> float:
    """beta of iteration `iteration` (>= 0).
    none:     1.
    linear:   start + (1 - start) * min(1, iteration / iters) - from `start` to 1 over `iters` iterations, then 1.
    cyclical (Fu et al. 2019, "Cyclical Annealing Schedule"): with tau = (iteration mod iters) / iters the position in the cycle,
              start + (1 - start) * min(1, tau / ratio) - the ramp takes the first `ratio` of every cycle of `iters` iterations."""
    if kind not in KINDS:
        raise ValueError(f"kl_beta: kind must be one of {' | '.join(KINDS)}; found {kind!r}")
    if kind == "none":
        return 1.0
    iteration, iters = int(iteration), int(iters)
    if iteration < 0 or iters < 1:
        raise ValueError(f"kl_beta: iteration must be >= 0 and iters >= 1; found {iteration}, {iters}")
    if not 0.0 <= start <= 1.0 or not 0.0 < ratio <= 1.0:
        raise ValueError(f"kl_beta: start must be in [0, 1] and ratio in (0, 1]; found {start!r}, {ratio!r}")
    if kind == "linear":
        ramp = min(1.0, iteration / iters)
    else:
        ramp = min(1.0, (iteration % iters) / iters / ratio)
    return float(start + (1.0 - start) * ramp)


def kl_beta_from_config(optim, iteration: int) -> float:
    """beta of `iteration` under the OPTIM.KL_ANNEAL* keys of a Config."""
    return kl_beta(iteration, optim.KL_ANNEAL, optim.KL_ANNEAL_ITERS, optim.KL_ANNEAL_RATIO, optim.KL_ANNEAL_START)
