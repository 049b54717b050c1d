"""Schedules of the cross-entropy steps as pure functions of the iteration number: KL annealing (the weight beta of the KL term,
OPTIM.KL_ANNEAL*) and scheduled sampling (the probability that a fed word is the model's own, OPTIM.SCHEDULED_SAMPLING_*, and the
seed of an iteration's draws).  A resumed run needs no state beyond the iteration it resumes at."""
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


def ss_prob(iteration: int, start: int = -1, every: int = 5000, increase: float = 0.05, maximum: float = 0.25) -> float:
    """Scheduled-sampling probability of iteration `iteration` (float64): 0 for start < 0 (off) or before `start`, else
    min(maximum, increase * ((iteration - start) // every)) - 0 on the first `every` iterations from `start`, then one `increase`
    more every `every` iterations up to `maximum` (the UpDown cross-entropy schedule: +0.05 every few epochs, capped at 0.25)."""
    iteration, start, every = int(iteration), int(start), int(every)
    if every < 1:
        raise ValueError(f"ss_prob: every must be >= 1; found {every}")
    if not 0.0 <= increase <= 1.0 or not 0.0 <= maximum <= 1.0:
        raise ValueError(f"ss_prob: increase and maximum must be in [0, 1]; found {increase!r}, {maximum!r}")
    if start < 0 or iteration < start:
        return 0.0
    return float(min(float(maximum), float(increase) * ((iteration - start) // every)))


def ss_prob_from_config(optim, iteration: int) -> float:
    """ss_prob of `iteration` under the OPTIM.SCHEDULED_SAMPLING_* keys of a Config."""
    return ss_prob(iteration, optim.SCHEDULED_SAMPLING_START, optim.SCHEDULED_SAMPLING_INCREASE_EVERY,
                   optim.SCHEDULED_SAMPLING_INCREASE_PROB, optim.SCHEDULED_SAMPLING_MAX_PROB)


def ss_sampler_from_config(optim):
    """The word sampler of the scheduled-sampling draws under OPTIM.SCHEDULED_SAMPLING_SAMPLER / _TEMPERATURE, as the (kind, top_k,
    top_p, temperature) TrainEngine.forward's ss_sampler takes: "multinomial" draws from softmax(logits / temperature), "argmax"
    is top-k with k = 1."""
    if optim.SCHEDULED_SAMPLING_SAMPLER == "argmax":
        return (1, 1, 1.0, 1.0)
    return (0, 0, 1.0, float(optim.SCHEDULED_SAMPLING_TEMPERATURE))


def ss_seed(random_seed: int, iteration: int, rank: int = 0) -> int:
    """The 64-bit seed of one iteration's scheduled-sampling decisions and draws on one rank: a pure function of (RANDOM_SEED,
    iteration, rank) - a resumed run draws what the uninterrupted run would have drawn - mixed by splitmix64 from another constant
    than scst_seed, so that the two features never share a stream for the same arguments."""
    mask = (1 << 64) - 1
    x = (int(random_seed) * 0xD1342543DE82EF95 + int(iteration) * 0x9E3779B97F4A7C15 + int(rank) * 0xC2B2AE3D27D4EB4F
         + 0x5851F42D4C957F2D) & mask
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & mask
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & mask
    x ^= x >> 31
    return x
