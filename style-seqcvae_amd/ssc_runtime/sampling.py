"""Word-level samplers for the diverse decode: multinomial, top-k and top-p (nucleus) draws of one word per row on the device
(ssc_sample_rows / ssc_decode_sample, include/ssc.h).

Reference: MultinomialSampler, TopKSampler, TopPSampler (var_updown/var_updown/modules/beam_search.py:103-293) - same constructor
signatures and argument checks.  The reference draws with torch.multinomial; here the draw is Gumbel-max over the kept set with
counter-based Philox4x32-10 noise keyed by a 64-bit seed: the same distribution, reproducible bit for bit.  The word decode
(DecodeEngine.sample / ssc_decode_sample) makes one draw per row (beam 1, per_node_beam_size 1), where `with_replacement` has no
effect; the sampled-node beam search (DecodeEngine.sampled_beam / ssc_decode_sampled_beam, MODEL.SAMPLED_BEAM_SEARCH) draws
per_node candidates per beam at any beam, with or without replacement as `with_replacement` says.  Top-p keeps every token at
p = 1 (the reference's fp32 cumsum can fall short of 1 and drop tail tokens there).

GumbelSampler (beam_search.py:294-432) is the stochastic beam search: `beam` captions per batch entry without replacement, at any
beam (DecodeEngine.stochastic_beam / ssc_decode_stochastic_beam).

DiverseBeam is no sampler: the deterministic diverse beam search (Vijayakumar et al., AAAI 2018; DecodeEngine.diverse_beam /
ssc_decode_diverse_beam, MODEL.DIVERSE_BEAM_SEARCH), the "Div-BS" baseline the sampled decoders are compared with.

DecodeRules is no sampler either: the controls a best-1 caption is decoded under - blocking of repeated n-grams, a minimum length,
suppressed tokens and a length penalty in the ranking (DecodeEngine.rules_beam / ssc_decode_rules_beam, MODEL.NO_REPEAT_NGRAM /
MIN_CAPTION_LENGTH / LENGTH_PENALTY_ALPHA / SUPPRESS_UNKNOWN), for the deterministic beam search.

LogitRules are the word samplers' own controls, a second and separate mechanism: the raw logits of every sampled step are edited in
front of the draw - a word bias, repetition / presence / frequency penalties, blocked n-grams, a minimum length, suppressed tokens
(DecodeEngine.sample(logit_rules=) / ssc_sample_opts.rules, MODEL.SAMPLER_NO_REPEAT_NGRAM and its kin) - so that the sampler
draws from the edited distribution, where DecodeRules ban after the log-softmax and renormalise nothing.

Truncation is the word samplers' entropy-adaptive cut - locally typical, min-p, eta and epsilon sampling - made the same way: one
more edit of the raw logits between the logit rules and the draw (DecodeEngine.sample(truncation=) / ssc_sample_opts.trunc,
MODEL.SAMPLER_TRUNCATION / SAMPLER_TRUNCATION_VALUE).  The samplers themselves are unchanged.

Mirostat is the one control with state: a surprise target held by feedback, a cut behind the truncation and an update behind the draw
(DecodeEngine.sample(mirostat=) / ssc_decode_sample_mirostat, MODEL.SAMPLER_MIROSTAT_TAU / SAMPLER_MIROSTAT_ETA).

Arithmetic replaces the draw itself: every caption decodes along a code point, the codes of an image form a randomly shifted lattice
(DecodeEngine.sample(arithmetic=) / ssc_decode_sample_arith, MODEL.SAMPLER_ARITHMETIC / SAMPLER_ARITHMETIC_SHARE_LATENT).
"""
import math

import numpy as np

from . import lib as _lib

KINDS = {"multinomial": 0, "top-k": 1, "top-p": 2}


class Sampler:
    kind = -1
    name = ""
    beam_search = False   # True: a sequence-level sampler that runs at any beam (GumbelSampler); False: a word sampler, beam 1 only

    def desc(self, seed: int) -> "_lib.SamplerDesc":
        """The C struct ssc_sampler_desc for a call with this 64-bit seed."""
        d = _lib.SamplerDesc()
        d.kind = self.kind
        d.top_k = int(getattr(self, "k", 0))
        d.top_p = float(getattr(self, "p", 1.0))
        d.temperature = float(self.temperature)
        d.seed = int(seed) & (2 ** 64 - 1)
        return d

    def check_vocab(self, V: int) -> None:
        pass

    def __repr__(self):
        args = ", ".join(f"{k}={v!r}" for k, v in vars(self).items())
        return f"{type(self).__name__}({args})"


def _check_temperature(t) -> None:
    if t < 0:
        raise ValueError(f"temperature must not be negative, got {t}")


class MultinomialSampler(Sampler):
    """Draws from softmax(log_probs / temperature) (beam_search.py:103-141)."""
    kind = 0
    name = "multinomial"

    def __init__(self, temperature: float = 1.0, with_replacement: bool = False) -> None:
        _check_temperature(temperature)
        if temperature <= 0:   # (the reference would divide by zero and draw from NaN)
            raise ValueError(f"multinomial sampling needs temperature > 0, got {temperature}")
        self.temperature = float(temperature)
        self.with_replacement = with_replacement


class TopKSampler(Sampler):
    """Keeps the k largest log-probs (ties: lower index first), draws from softmax(kept / temperature) (beam_search.py:144-205).
    A temperature of 0 means 1, as in the reference."""
    kind = 1
    name = "top-k"

    def __init__(self, k: int = 1, temperature: float = 1.0, with_replacement: bool = False):
        _check_temperature(temperature)
        if int(k) != k or k < 1:
            raise ValueError("k must be a postive integer no less than per_node_beam_size and no greater than vocabulary size")
        self.k = int(k)
        self.temperature = float(temperature or 1.0)
        self.with_replacement = with_replacement

    def check_vocab(self, V: int) -> None:
        if not 1 <= self.k <= V:   # (beam_search.py:180-183)
            raise ValueError("k must be a postive integer no less than per_node_beam_size and no greater than vocabulary size")


class TopPSampler(Sampler):
    """Keeps the smallest prefix of the tempered distribution, sorted descending (ties: lower index first), whose mass reaches p,
    draws from it renormalised (beam_search.py:208-293).  A temperature of 0 means 1, as in the reference."""
    kind = 2
    name = "top-p"

    def __init__(self, p: float = 0.9, temperature: float = 1.0, with_replacement: bool = False):
        if p < 0.0 or p > 1.0:
            raise ValueError("p must be a positive float no greater than 1.0")
        _check_temperature(temperature)
        self.p = float(p)
        self.temperature = float(temperature or 1.0)
        self.with_replacement = with_replacement


class GumbelSampler(Sampler):
    """Stochastic beam search (beam_search.py:294-432, Kool et al. 2019): the beam keeps `beam` distinct captions per batch entry,
    sampled without replacement with sequence-level probabilities through the Gumbel-top-k trick (ssc_decode_stochastic_beam,
    include/ssc.h).  temperature tempers the perturbed scores of the steps after the first, as in the reference."""
    kind = -2
    name = "gumbel"
    beam_search = True

    def __init__(self, temperature: float = 1.0):
        if not temperature > 0:   # (the reference would divide by zero)
            raise ValueError(f"the Gumbel sampler needs temperature > 0, got {temperature}")
        self.temperature = float(temperature)

    def desc(self, seed: int) -> "_lib.GumbelDesc":
        """The C struct ssc_gumbel_desc for a call with this 64-bit seed."""
        d = _lib.GumbelDesc()
        d.temperature = float(self.temperature)
        d.seed = int(seed) & (2 ** 64 - 1)
        return d


class DiverseBeam:
    """Diverse beam search: the beam is `groups` groups of beam // groups beams searched in order; a word that beams of the
    earlier groups selected at a step is ranked `strength` lower per selection for the later ones (Hamming diversity,
    ssc_diverse_desc in include/ssc.h).  groups = 1 is beam search; strength = 0 runs the groups as independent searches."""

    def __init__(self, groups: int = 1, strength: float = 0.5) -> None:
        if int(groups) != groups or groups < 1:
            raise ValueError(f"groups must be a positive integer, got {groups}")
        if not (strength >= 0 and strength < float("inf")):
            raise ValueError(f"strength must be finite and not negative, got {strength}")
        self.groups = int(groups)
        self.strength = float(strength)

    def check_beam(self, beam: int) -> None:
        if beam % self.groups != 0:
            raise ValueError(f"the beam size ({beam}) must be a multiple of the number of groups ({self.groups})")

    def per_node(self, beam: int) -> int:
        """The reference's per-node rule (beam // 2, or beam) applied to the group width."""
        kp = beam // self.groups
        return kp // 2 or kp

    def desc(self) -> "_lib.DiverseDesc":
        """The C struct ssc_diverse_desc."""
        d = _lib.DiverseDesc()
        d.groups = self.groups
        d.strength = self.strength
        return d

    def __repr__(self):
        return f"DiverseBeam(groups={self.groups}, strength={self.strength})"


def diverse_beam_from_config(model_cfg):
    """MODEL.DIVERSE_BEAM_SEARCH / DIVERSE_BEAM_GROUPS / DIVERSE_BEAM_STRENGTH -> DiverseBeam, or None when off.  Needs
    DECODE_SAMPLER "beam", STOCHASTIC_BEAM_SEARCH and SAMPLED_BEAM_SEARCH False, USE_CBS False and
    BEAM_SIZE % DIVERSE_BEAM_GROUPS == 0."""
    if not bool(getattr(model_cfg, "DIVERSE_BEAM_SEARCH", False)):
        return None
    kind = str(model_cfg.DECODE_SAMPLER).strip().lower()
    if kind != "beam":
        raise ValueError(f"MODEL.DIVERSE_BEAM_SEARCH needs MODEL.DECODE_SAMPLER 'beam', got {model_cfg.DECODE_SAMPLER!r} (the diverse "
                         "beam search is deterministic)")
    if bool(getattr(model_cfg, "STOCHASTIC_BEAM_SEARCH", False)):
        raise ValueError("MODEL.DIVERSE_BEAM_SEARCH and MODEL.STOCHASTIC_BEAM_SEARCH exclude each other")
    if bool(getattr(model_cfg, "SAMPLED_BEAM_SEARCH", False)):
        raise ValueError("MODEL.DIVERSE_BEAM_SEARCH and MODEL.SAMPLED_BEAM_SEARCH exclude each other")
    if bool(getattr(model_cfg, "USE_CBS", False)):
        raise ValueError("MODEL.DIVERSE_BEAM_SEARCH does not take constraints: MODEL.USE_CBS must be False")
    groups = int(getattr(model_cfg, "DIVERSE_BEAM_GROUPS", 1))
    strength = float(getattr(model_cfg, "DIVERSE_BEAM_STRENGTH", 0.5))
    if groups < 1:
        raise ValueError(f"MODEL.DIVERSE_BEAM_GROUPS must be at least 1, got {groups}")
    if not (strength >= 0 and strength < float("inf")):
        raise ValueError(f"MODEL.DIVERSE_BEAM_STRENGTH must be finite and not negative, got {strength}")
    beam = int(model_cfg.BEAM_SIZE)
    if beam % groups != 0:
        raise ValueError(f"MODEL.BEAM_SIZE ({beam}) must be a multiple of MODEL.DIVERSE_BEAM_GROUPS ({groups})")
    return DiverseBeam(groups, strength)


class DecodeRules:
    """The decode rules of the beam search (ssc_rules_desc in include/ssc.h): no_repeat_ngram n - a token that would complete an
    n-gram the caption already holds is not a candidate (0: off; 3 is the usual choice) -, min_length - END is not a candidate before
    that many words -, length_alpha - beams are ranked by their summed log-prob over length ** alpha, the END counted (0: the raw
    sum) - and suppress: up to 8 token ids that are never emitted.  The log-probs themselves are never changed."""

    def __init__(self, no_repeat_ngram: int = 0, min_length: int = 0, length_alpha: float = 0.0, suppress=()) -> None:
        if isinstance(no_repeat_ngram, bool) or int(no_repeat_ngram) != no_repeat_ngram or not 0 <= no_repeat_ngram <= _lib.SSC_RULES_MAX_LEN:
            raise ValueError(f"no_repeat_ngram must be an integer in 0..{_lib.SSC_RULES_MAX_LEN}, got {no_repeat_ngram!r}")
        if isinstance(min_length, bool) or int(min_length) != min_length or min_length < 0:
            raise ValueError(f"min_length must be an integer and not negative, got {min_length!r}")
        if isinstance(length_alpha, bool) or not math.isfinite(length_alpha):
            raise ValueError(f"length_alpha must be a finite number, got {length_alpha!r}")
        suppress = tuple(suppress)
        if len(suppress) > _lib.SSC_RULES_MAX_SUPPRESS:
            raise ValueError(f"at most {_lib.SSC_RULES_MAX_SUPPRESS} tokens can be suppressed, got {len(suppress)}")
        if any(isinstance(v, bool) or int(v) != v or v < 0 for v in suppress) or len(set(suppress)) != len(suppress):
            raise ValueError(f"suppress must hold distinct token ids, none negative, got {suppress!r}")
        self.no_repeat_ngram = int(no_repeat_ngram)
        self.min_length = int(min_length)
        self.length_alpha = float(length_alpha)
        self.suppress = tuple(int(v) for v in suppress)

    @property
    def active(self) -> bool:
        """False when every rule is off: the search is then the plain beam search."""
        return bool(self.no_repeat_ngram or self.min_length or self.length_alpha != 0.0 or self.suppress)

    def table(self) -> np.ndarray:
        """(64,) float32: entry L - 1 = L ** length_alpha, formed in float64 and rounded once."""
        with np.errstate(over="ignore"):   # (an alpha beyond float32's range gives inf: check() refuses it)
            return (np.arange(1, _lib.SSC_RULES_MAX_LEN + 1, dtype=np.float64) ** self.length_alpha).astype(np.float32)

    def check(self, V: int, end_index: int, max_steps: int) -> None:
        if max_steps > _lib.SSC_RULES_MAX_LEN:
            raise ValueError(f"the beam search under decode rules runs at most {_lib.SSC_RULES_MAX_LEN} steps, got {max_steps}")
        for v in self.suppress:
            if v >= V or v == end_index:
                raise ValueError(f"a suppressed token must lie in [0, {V}) and must not be the boundary token {end_index}, got {v}")
        t = self.table()
        if not (np.isfinite(t).all() and (t > 0).all()):
            raise ValueError(f"length_alpha {self.length_alpha} gives a penalty that is not finite and positive in float32")

    def desc(self) -> "_lib.RulesDesc":
        """The C struct ssc_rules_desc."""
        d = _lib.RulesDesc()
        d.no_repeat_ngram, d.min_length, d.n_suppress = self.no_repeat_ngram, self.min_length, len(self.suppress)
        for i, v in enumerate(self.suppress):
            d.suppress[i] = v
        for i, v in enumerate(self.table()):
            d.length_penalty[i] = float(v)
        return d

    def __repr__(self):
        return (f"DecodeRules(no_repeat_ngram={self.no_repeat_ngram}, min_length={self.min_length}, length_alpha={self.length_alpha}, "
                f"suppress={self.suppress})")


def decode_rules_from_config(model_cfg, vocabulary=None):
    """MODEL.NO_REPEAT_NGRAM / MIN_CAPTION_LENGTH / LENGTH_PENALTY_ALPHA / SUPPRESS_UNKNOWN -> DecodeRules, or None when every key
    has its default (no new code path runs then).  The rules belong to the deterministic beam search: DECODE_SAMPLER "beam",
    STOCHASTIC_BEAM_SEARCH, SAMPLED_BEAM_SEARCH and DIVERSE_BEAM_SEARCH False, USE_CBS False.  vocabulary: where @@UNKNOWN@@ is
    looked up for SUPPRESS_UNKNOWN (None: only the keys are checked, and the id is left out)."""
    n = getattr(model_cfg, "NO_REPEAT_NGRAM", 0)
    m = getattr(model_cfg, "MIN_CAPTION_LENGTH", 0)
    alpha = getattr(model_cfg, "LENGTH_PENALTY_ALPHA", 0.0)
    unk = bool(getattr(model_cfg, "SUPPRESS_UNKNOWN", False))
    set_keys = [k for k, on in (("NO_REPEAT_NGRAM", n != 0), ("MIN_CAPTION_LENGTH", m != 0), ("LENGTH_PENALTY_ALPHA", alpha != 0.0),
                                ("SUPPRESS_UNKNOWN", unk)) if on]
    if not set_keys:
        return None
    key = "MODEL." + set_keys[0]
    kind = str(model_cfg.DECODE_SAMPLER).strip().lower()
    if kind != "beam":
        raise ValueError(f"{key} needs MODEL.DECODE_SAMPLER 'beam', got {model_cfg.DECODE_SAMPLER!r} (the decode rules belong to the "
                         "deterministic beam search)")
    for other in ("STOCHASTIC_BEAM_SEARCH", "SAMPLED_BEAM_SEARCH", "DIVERSE_BEAM_SEARCH"):
        if bool(getattr(model_cfg, other, False)):
            raise ValueError(f"{key} and MODEL.{other} exclude each other (the decode rules belong to the deterministic beam search)")
    if bool(getattr(model_cfg, "USE_CBS", False)):
        raise ValueError(f"{key} does not take constraints: MODEL.USE_CBS must be False")
    suppress = ()
    if unk and vocabulary is not None:
        from .vocab import UNKNOWN
        suppress = (int(vocabulary.get_token_index(UNKNOWN)),)
    try:
        return DecodeRules(n, m, alpha, suppress)
    except ValueError as e:
        raise ValueError(f"MODEL.NO_REPEAT_NGRAM / MIN_CAPTION_LENGTH / LENGTH_PENALTY_ALPHA: {e}") from None


class LogitRules:
    """The logit rules of the word samplers (ssc_logit_rules in include/ssc.h): the raw logits of every step are edited in front of
    the draw - first `bias` is added, then the words the caption already holds are penalised (repetition_penalty theta: a positive
    logit is divided by theta, any other multiplied; presence_penalty + frequency_penalty * count is then taken off), then tokens
    are banned (no_repeat_ngram n, min_length, suppress: as DecodeRules words them).  The sampler draws from the edited
    distribution and reports the log-prob under it.  bias: a float32 device tensor (V,), (1, V) - one row for all - or (nimg, V) -
    one row per image; -inf bans a word, +inf and NaN are refused."""

    def __init__(self, no_repeat_ngram: int = 0, min_length: int = 0, suppress=(), repetition_penalty: float = 1.0,
                 presence_penalty: float = 0.0, frequency_penalty: float = 0.0, bias=None) -> None:
        if isinstance(no_repeat_ngram, bool) or int(no_repeat_ngram) != no_repeat_ngram or not 0 <= no_repeat_ngram <= _lib.SSC_RULES_MAX_LEN:
            raise ValueError(f"no_repeat_ngram must be an integer in 0..{_lib.SSC_RULES_MAX_LEN}, got {no_repeat_ngram!r}")
        if isinstance(min_length, bool) or int(min_length) != min_length or min_length < 0:
            raise ValueError(f"min_length must be an integer and not negative, got {min_length!r}")
        suppress = tuple(suppress)
        if len(suppress) > _lib.SSC_RULES_MAX_SUPPRESS:
            raise ValueError(f"at most {_lib.SSC_RULES_MAX_SUPPRESS} tokens can be suppressed, got {len(suppress)}")
        if any(isinstance(v, bool) or int(v) != v or v < 0 for v in suppress) or len(set(suppress)) != len(suppress):
            raise ValueError(f"suppress must hold distinct token ids, none negative, got {suppress!r}")
        for name, v in (("repetition_penalty", repetition_penalty), ("presence_penalty", presence_penalty),
                        ("frequency_penalty", frequency_penalty)):
            if isinstance(v, bool) or not math.isfinite(v) or abs(v) > float(np.finfo(np.float32).max):
                raise ValueError(f"{name} must be a finite number, got {v!r}")
        if not float(np.float32(repetition_penalty)) > 0:
            raise ValueError(f"repetition_penalty must be positive, got {repetition_penalty!r}")
        if bias is not None:
            import torch
            if not (isinstance(bias, torch.Tensor) and bias.dtype == torch.float32 and bias.dim() in (1, 2) and bias.numel() > 0):
                raise ValueError("bias must be a float32 tensor of shape (V,), (1, V) or (nimg, V)")
            bias = bias.reshape(1, -1) if bias.dim() == 1 else bias
        self.no_repeat_ngram = int(no_repeat_ngram)
        self.min_length = int(min_length)
        self.suppress = tuple(int(v) for v in suppress)
        self.repetition_penalty = float(repetition_penalty)
        self.presence_penalty = float(presence_penalty)
        self.frequency_penalty = float(frequency_penalty)
        self.bias = bias

    @property
    def active(self) -> bool:
        """False when every control is off and there is no bias: the decode is then the plain sampled decode."""
        return bool(self.no_repeat_ngram or self.min_length or self.suppress or np.float32(self.repetition_penalty) != 1
                    or np.float32(self.presence_penalty) != 0 or np.float32(self.frequency_penalty) != 0 or self.bias is not None)

    def check(self, V: int, end_index: int, max_steps: int, nimg: int) -> None:
        """The limits of ssc_decode_sample_opts' rules for a call over nimg images, and the bias's contents (one read-back)."""
        if not self.active:
            return
        if max_steps > _lib.SSC_RULES_MAX_LEN:
            raise ValueError(f"the sampled decode under logit rules runs at most {_lib.SSC_RULES_MAX_LEN} steps, got {max_steps}")
        for v in self.suppress:
            if v >= V or v == end_index:
                raise ValueError(f"a suppressed token must lie in [0, {V}) and must not be the boundary token {end_index}, got {v}")
        if V <= max_steps + len(self.suppress):
            raise ValueError(f"the logit rules need a vocabulary above max_steps + suppressed tokens = {max_steps + len(self.suppress)}"
                             f", got {V} (the rules alone must not empty a row)")
        if self.bias is not None:
            b = self.bias
            if not b.is_cuda:
                raise ValueError("bias must be a device tensor")
            if b.size(1) != V or b.size(0) not in (1, nimg):
                raise ValueError(f"bias must have shape ({V},), (1, {V}) or ({nimg}, {V}), got {tuple(b.shape)}")
            import torch
            if bool((torch.isnan(b) | (b == float("inf"))).any()):
                raise ValueError("bias holds NaN or +inf (-inf bans a word; +inf and NaN are refused)")

    def desc(self, n_samples: int):
        """-> (the C struct ssc_logit_rules for a call of n_samples entries per image, the tensors behind it: keep them until the
        call is queued).  bias_row is the image index of every entry b = (image, sample); NULL with one shared row."""
        d = _lib.LogitRules()
        d.no_repeat_ngram, d.min_length, d.n_suppress = self.no_repeat_ngram, self.min_length, len(self.suppress)
        for i, v in enumerate(self.suppress):
            d.suppress[i] = v
        d.repetition_penalty, d.presence_penalty, d.frequency_penalty = (self.repetition_penalty, self.presence_penalty,
                                                                         self.frequency_penalty)
        keep = []
        if self.bias is not None:
            import torch
            b = self.bias.contiguous()
            keep.append(b)
            d.bias, d.ld_bias, d.n_bias = b.data_ptr(), b.size(1), b.size(0)
            if b.size(0) > 1:
                rows = torch.arange(b.size(0), dtype=torch.int32, device=b.device).repeat_interleave(int(n_samples)).contiguous()
                keep.append(rows)
                d.bias_row = rows.data_ptr()
        return d, keep

    def __repr__(self):
        return (f"LogitRules(no_repeat_ngram={self.no_repeat_ngram}, min_length={self.min_length}, suppress={self.suppress}, "
                f"repetition_penalty={self.repetition_penalty}, presence_penalty={self.presence_penalty}, "
                f"frequency_penalty={self.frequency_penalty}, bias={None if self.bias is None else tuple(self.bias.shape)})")


_LOGIT_RULE_KEYS = (("SAMPLER_NO_REPEAT_NGRAM", 0), ("SAMPLER_MIN_LENGTH", 0), ("SAMPLER_SUPPRESS_UNKNOWN", False),
                    ("SAMPLER_REPETITION_PENALTY", 1.0), ("SAMPLER_PRESENCE_PENALTY", 0.0), ("SAMPLER_FREQUENCY_PENALTY", 0.0))


def logit_rules_from_config(model_cfg, vocabulary=None):
    """MODEL.SAMPLER_NO_REPEAT_NGRAM / SAMPLER_MIN_LENGTH / SAMPLER_SUPPRESS_UNKNOWN / SAMPLER_REPETITION_PENALTY /
    SAMPLER_PRESENCE_PENALTY / SAMPLER_FREQUENCY_PENALTY -> LogitRules, or None when every key has its default (no new code path
    runs then).  The rules belong to the word samplers: DECODE_SAMPLER multinomial / top-k / top-p, SAMPLED_BEAM_SEARCH and
    STOCHASTIC_BEAM_SEARCH False.  vocabulary: where @@UNKNOWN@@ is looked up for SAMPLER_SUPPRESS_UNKNOWN (None: only the keys
    are checked, and the id is left out)."""
    vals = {k: getattr(model_cfg, k, dflt) for k, dflt in _LOGIT_RULE_KEYS}
    set_keys = [k for k, dflt in _LOGIT_RULE_KEYS if vals[k] != dflt]
    if not set_keys:
        return None
    key = "MODEL." + set_keys[0]
    kind = str(model_cfg.DECODE_SAMPLER).strip().lower()
    if kind not in KINDS:
        raise ValueError(f"{key} needs MODEL.DECODE_SAMPLER 'multinomial', 'top-k' or 'top-p', got {model_cfg.DECODE_SAMPLER!r} (the "
                         "logit rules belong to the word samplers; the beam search has MODEL.NO_REPEAT_NGRAM and its kin)")
    for other in ("SAMPLED_BEAM_SEARCH", "STOCHASTIC_BEAM_SEARCH"):
        if bool(getattr(model_cfg, other, False)):
            raise ValueError(f"{key} and MODEL.{other} exclude each other (the logit rules belong to the word-sampled decode)")
    suppress = ()
    if vals["SAMPLER_SUPPRESS_UNKNOWN"] and vocabulary is not None:
        from .vocab import UNKNOWN
        suppress = (int(vocabulary.get_token_index(UNKNOWN)),)
    try:
        return LogitRules(vals["SAMPLER_NO_REPEAT_NGRAM"], vals["SAMPLER_MIN_LENGTH"], suppress, vals["SAMPLER_REPETITION_PENALTY"],
                          vals["SAMPLER_PRESENCE_PENALTY"], vals["SAMPLER_FREQUENCY_PENALTY"])
    except ValueError as e:
        raise ValueError(f"MODEL.SAMPLER_NO_REPEAT_NGRAM / SAMPLER_MIN_LENGTH / SAMPLER_*_PENALTY: {e}") from None


TRUNCATION_KINDS = {"none": 0, "typical": 1, "min-p": 2, "eta": 3, "epsilon": 4}


class Truncation:
    """A truncation of the word samplers' distribution (ssc_truncation in include/ssc.h): a cut that adapts to each step's entropy,
    made on the raw logits of every step between the logit rules and the draw (DecodeEngine.sample(truncation=) /
    ssc_sample_opts.trunc), so that the sampler - multinomial, top-k or top-p - draws from the cut distribution, tempered by the
    sampler's temperature, and reports the log-prob under it.  kind: 0 off, 1 typical, 2 min-p, 3 eta, 4 epsilon; value: the mass
    tau / the ratio m in (0, 1], or epsilon in (0, 1)."""
    name = "none"

    def __init__(self, kind: int = 0, value: float = 0.0) -> None:
        if isinstance(kind, bool) or int(kind) != kind or not 0 <= kind <= 4:
            raise ValueError(f"the truncation kind must be an integer in 0..4, got {kind!r}")
        kind = int(kind)
        try:
            value = float(value)
        except (TypeError, ValueError):
            raise ValueError(f"the truncation value must be a number, got {value!r}") from None
        name = [n for n, k in TRUNCATION_KINDS.items() if k == kind][0]
        if kind in (1, 2) and not (0.0 < value <= 1.0):   # (false for NaN)
            raise ValueError(f"{name} truncation needs a value in (0, 1], got {value}")
        if kind in (3, 4) and not (0.0 < value < 1.0):
            raise ValueError(f"{name} truncation needs an epsilon in (0, 1), got {value}")
        self.kind = kind
        self.value = value
        self.name = name

    @property
    def active(self) -> bool:
        return self.kind != 0

    def desc(self, entropy=None, kept=None) -> "_lib.Truncation":
        """The C struct ssc_truncation; entropy / kept: the statistics tensors of the call, or None."""
        d = _lib.Truncation()
        d.kind, d.value = self.kind, self.value
        d.entropy = entropy.data_ptr() if entropy is not None else None
        d.kept = kept.data_ptr() if kept is not None else None
        return d

    def __repr__(self):
        return f"{type(self).__name__}({self.name}, {self.value})"


class TypicalTruncation(Truncation):
    """Locally typical sampling (Meister et al. 2022): the words whose surprise is closest to the step's entropy, up to `mass`."""

    def __init__(self, mass: float = 0.9) -> None:
        super().__init__(1, mass)


class MinPTruncation(Truncation):
    """Min-p (Nguyen et al. 2024): the words at least `min_p` times as probable as the most probable one."""

    def __init__(self, min_p: float = 0.05) -> None:
        super().__init__(2, min_p)


class EtaTruncation(Truncation):
    """Eta sampling (Hewitt et al. 2022): the words with probability at least min(epsilon, sqrt(epsilon) * exp(-entropy))."""

    def __init__(self, epsilon: float = 3e-4) -> None:
        super().__init__(3, epsilon)


class EpsilonTruncation(Truncation):
    """Epsilon sampling (Hewitt et al. 2022): the words with probability at least `epsilon`."""

    def __init__(self, epsilon: float = 3e-4) -> None:
        super().__init__(4, epsilon)


_TRUNCATION_CLASSES = {"typical": TypicalTruncation, "min-p": MinPTruncation, "eta": EtaTruncation, "epsilon": EpsilonTruncation}


def truncation_from_name(name: str, value=None):
    """"typical" / "min-p" / "eta" / "epsilon" (+ a value, None: the kind's default) -> its Truncation; "none" -> None."""
    key = str(name).strip().lower()
    if key == "none":
        return None
    if key not in _TRUNCATION_CLASSES:
        raise ValueError(f"the truncation must be one of none | typical | min-p | eta | epsilon, got {name!r}")
    return _TRUNCATION_CLASSES[key]() if value is None else _TRUNCATION_CLASSES[key](value)


def truncation_from_config(model_cfg):
    """MODEL.SAMPLER_TRUNCATION (none | typical | min-p | eta | epsilon) / SAMPLER_TRUNCATION_VALUE (0 = the kind's default) ->
    Truncation, or None when off (no new code path runs then).  The truncation belongs to the word samplers: DECODE_SAMPLER
    multinomial / top-k / top-p, SAMPLED_BEAM_SEARCH and STOCHASTIC_BEAM_SEARCH False."""
    name = str(getattr(model_cfg, "SAMPLER_TRUNCATION", "none")).strip().lower()
    value = float(getattr(model_cfg, "SAMPLER_TRUNCATION_VALUE", 0.0))
    if name == "none":
        return None
    kind = str(model_cfg.DECODE_SAMPLER).strip().lower()
    if kind not in KINDS:
        raise ValueError(f"MODEL.SAMPLER_TRUNCATION needs MODEL.DECODE_SAMPLER 'multinomial', 'top-k' or 'top-p', got "
                         f"{model_cfg.DECODE_SAMPLER!r} (the truncation belongs to the word samplers)")
    for other in ("SAMPLED_BEAM_SEARCH", "STOCHASTIC_BEAM_SEARCH"):
        if bool(getattr(model_cfg, other, False)):
            raise ValueError(f"MODEL.SAMPLER_TRUNCATION and MODEL.{other} exclude each other (the truncation belongs to the "
                             "word-sampled decode)")
    try:
        return truncation_from_name(name, None if value == 0 else value)
    except ValueError as e:
        raise ValueError(f"MODEL.SAMPLER_TRUNCATION / SAMPLER_TRUNCATION_VALUE: {e}") from None


LN2 = math.log(2.0)
MIROSTAT_UNITS = {"bits": LN2, "nats": 1.0}


class Mirostat:
    """Mirostat 2.0 for the word samplers (ssc_mirostat in include/ssc.h; Basu et al., ICLR 2021): the surprise of the drawn words is
    held at the target `tau` by feedback - every word whose surprise exceeds a running threshold mu is cut in front of the draw, and
    after the draw mu moves by eta times the error between the drawn word's surprise and tau (DecodeEngine.sample(mirostat=) /
    ssc_decode_sample_mirostat).  mu0: every caption's mu at its first word, None: 2 tau (the paper's start).  unit: "bits" (the
    paper's, the default) or "nats" - what tau, mu0 and the returned statistics are in; the device works in nats, the conversion is
    made once here (ln 2 in double, rounded to fp32).  tau = 0: off; eta = 0: a fixed surprise cut at mu0."""

    def __init__(self, tau: float = 3.0, eta: float = 0.1, mu0=None, unit: str = "bits") -> None:
        if unit not in MIROSTAT_UNITS:
            raise ValueError(f"the Mirostat unit must be 'bits' or 'nats', got {unit!r}")
        try:
            tau, eta = float(tau), float(eta)
            mu0 = 2.0 * tau if mu0 is None else float(mu0)
        except (TypeError, ValueError):
            raise ValueError(f"the Mirostat tau, eta and mu0 must be numbers, got {tau!r}, {eta!r}, {mu0!r}") from None
        if not (tau >= 0.0 and math.isfinite(tau)):   # (false for NaN)
            raise ValueError(f"the Mirostat target tau must be finite and >= 0 (0: off), got {tau}")
        if not (eta >= 0.0 and math.isfinite(eta)):
            raise ValueError(f"the Mirostat learning rate eta must be finite and >= 0, got {eta}")
        if not math.isfinite(mu0):
            raise ValueError(f"the Mirostat start mu0 must be finite, got {mu0}")
        self.tau, self.eta, self.mu0, self.unit = tau, eta, mu0, unit

    @property
    def scale(self) -> float:
        """nats per unit"""
        return MIROSTAT_UNITS[self.unit]

    @property
    def tau_nats(self) -> float:
        return _f32(self.tau * self.scale)

    @property
    def mu0_nats(self) -> float:
        return _f32(self.mu0 * self.scale)

    @property
    def active(self) -> bool:
        return self.tau_nats != 0.0

    def from_nats(self, t):
        """A tensor of device statistics (nats) in this object's unit."""
        return t if self.unit == "nats" else t / self.scale

    def desc(self, mu=None, surprise=None, kept=None) -> "_lib.Mirostat":
        """The C struct ssc_mirostat (nats); mu / surprise / kept: the blocks of the call, or None."""
        d = _lib.Mirostat()
        d.tau, d.eta, d.mu0 = self.tau_nats, self.eta, self.mu0_nats
        d.mu = mu.data_ptr() if mu is not None else None
        d.surprise = surprise.data_ptr() if surprise is not None else None
        d.kept = kept.data_ptr() if kept is not None else None
        return d

    def __repr__(self):
        return f"{type(self).__name__}(tau={self.tau}, eta={self.eta}, mu0={self.mu0}, unit={self.unit!r})"


def _f32(v: float) -> float:
    """v rounded to fp32 (what the C struct will hold)"""
    import ctypes
    return ctypes.c_float(v).value


def mirostat_from_config(model_cfg):
    """MODEL.SAMPLER_MIROSTAT_TAU (bits, 0 = off) / SAMPLER_MIROSTAT_ETA -> Mirostat, or None when off (no new code path runs then).
    Mirostat belongs to the word samplers: DECODE_SAMPLER multinomial / top-k / top-p, SAMPLED_BEAM_SEARCH and
    STOCHASTIC_BEAM_SEARCH False."""
    tau = float(getattr(model_cfg, "SAMPLER_MIROSTAT_TAU", 0.0))
    eta = float(getattr(model_cfg, "SAMPLER_MIROSTAT_ETA", 0.1))
    if tau == 0.0:
        return None
    try:
        m = Mirostat(tau, eta)
    except ValueError as e:
        raise ValueError(f"MODEL.SAMPLER_MIROSTAT_TAU / SAMPLER_MIROSTAT_ETA: {e}") from None
    kind = str(model_cfg.DECODE_SAMPLER).strip().lower()
    if kind not in KINDS:
        raise ValueError(f"MODEL.SAMPLER_MIROSTAT_TAU needs MODEL.DECODE_SAMPLER 'multinomial', 'top-k' or 'top-p', got "
                         f"{model_cfg.DECODE_SAMPLER!r} (Mirostat belongs to the word samplers)")
    for other in ("SAMPLED_BEAM_SEARCH", "STOCHASTIC_BEAM_SEARCH"):
        if bool(getattr(model_cfg, other, False)):
            raise ValueError(f"MODEL.SAMPLER_MIROSTAT_TAU and MODEL.{other} exclude each other (Mirostat belongs to the word-sampled "
                             "decode)")
    return m


class Arithmetic:
    """Arithmetic sampling for the word samplers (ssc_arith in include/ssc.h; Vilnis et al., ICML 2023): every caption decodes along
    a code point in [0, 1) by inverse CDF in vocabulary order, the code renormalised into the chosen word's interval after every
    step (DecodeEngine.sample(arithmetic=) / ssc_decode_sample_arith).  It replaces only the draw: each caption is on its own an
    exact draw from the sampler's distribution, every edit in front of the draw works as before.
    codes: "lattice" (the default) - the N codes of an image are a lattice of spacing 1 / N shifted by a random offset per image
    that the sampler's seed decides (ssc_arith_codes), so the set of an image is stratified -, or a tensor of B = images x samples
    codes, torch.uint64 (or int64 holding the same bits), code c meaning c / 2^64.
    share_latent: diverse_decode gives all samples of an image the latent noise of its sample 0, so that the N captions of an image
    differ by their codes alone (DecodeEngine.sample, which is handed its noise, does not read it)."""

    def __init__(self, codes="lattice", share_latent: bool = False) -> None:
        import torch
        if isinstance(codes, str):
            if codes != "lattice":
                raise ValueError(f'the arithmetic codes must be "lattice" or a uint64 tensor (B,), got {codes!r}')
        elif not isinstance(codes, torch.Tensor):
            raise ValueError(f'the arithmetic codes must be "lattice" or a uint64 tensor (B,), got {type(codes).__name__}')
        elif codes.dtype not in (torch.uint64, torch.int64) or codes.dim() != 1:
            raise ValueError(f"the arithmetic codes must be a uint64 (or int64) tensor of shape (B,), got {codes.dtype} "
                             f"{tuple(codes.shape)}")
        if not isinstance(share_latent, bool):
            raise ValueError(f"share_latent must be a bool, got {share_latent!r}")
        self.codes, self.share_latent = codes, share_latent

    @property
    def lattice(self) -> bool:
        return isinstance(self.codes, str)

    def desc(self, code) -> "_lib.Arith":
        """The C struct ssc_arith over the call's (max_steps + 1, B) int64 block `code`; given codes are copied into its slab 0."""
        import torch
        d = _lib.Arith()
        d.mode = 1 if self.lattice else 2
        if not self.lattice:
            if self.codes.numel() != code.size(1):
                raise ValueError(f"the arithmetic codes hold {self.codes.numel()} entries for {code.size(1)} rows")
            code[0].copy_(self.codes.view(torch.int64))
        d.code = code.data_ptr()
        return d

    def __repr__(self):
        return f"{type(self).__name__}(codes={'lattice' if self.lattice else 'tensor'!r}, share_latent={self.share_latent})"


def arithmetic_from_config(model_cfg):
    """MODEL.SAMPLER_ARITHMETIC / SAMPLER_ARITHMETIC_SHARE_LATENT -> Arithmetic, or None when off (no new code path runs then).
    Arithmetic sampling belongs to the word samplers: DECODE_SAMPLER multinomial / top-k / top-p, SAMPLED_BEAM_SEARCH and
    STOCHASTIC_BEAM_SEARCH False."""
    on = bool(getattr(model_cfg, "SAMPLER_ARITHMETIC", False))
    share = bool(getattr(model_cfg, "SAMPLER_ARITHMETIC_SHARE_LATENT", False))
    if not on:
        if share:
            raise ValueError("MODEL.SAMPLER_ARITHMETIC_SHARE_LATENT needs MODEL.SAMPLER_ARITHMETIC True")
        return None
    kind = str(model_cfg.DECODE_SAMPLER).strip().lower()
    if kind not in KINDS:
        raise ValueError(f"MODEL.SAMPLER_ARITHMETIC needs MODEL.DECODE_SAMPLER 'multinomial', 'top-k' or 'top-p', got "
                         f"{model_cfg.DECODE_SAMPLER!r} (arithmetic sampling belongs to the word samplers)")
    for other in ("SAMPLED_BEAM_SEARCH", "STOCHASTIC_BEAM_SEARCH"):
        if bool(getattr(model_cfg, other, False)):
            raise ValueError(f"MODEL.SAMPLER_ARITHMETIC and MODEL.{other} exclude each other (arithmetic sampling belongs to the "
                             "word-sampled decode)")
    return Arithmetic("lattice", share_latent=share)


def from_config(model_cfg):
    """The sampler the MODEL keys DECODE_SAMPLER / SAMPLER_TOP_K / SAMPLER_TOP_P / SAMPLER_TEMPERATURE / SAMPLER_WITH_REPLACEMENT /
    STOCHASTIC_BEAM_SEARCH describe, or None for "beam" (beam search, the default).  STOCHASTIC_BEAM_SEARCH with DECODE_SAMPLER
    "beam" gives GumbelSampler(SAMPLER_TEMPERATURE).  Checks MODEL.SAMPLED_BEAM_SEARCH (sampled_beam_from_config) and
    MODEL.DIVERSE_BEAM_SEARCH (diverse_beam_from_config) and the decode-rule keys (decode_rules_from_config)."""
    kind = str(model_cfg.DECODE_SAMPLER).strip().lower()
    T = float(model_cfg.SAMPLER_TEMPERATURE)
    sbs = bool(getattr(model_cfg, "STOCHASTIC_BEAM_SEARCH", False))
    rep = bool(getattr(model_cfg, "SAMPLER_WITH_REPLACEMENT", False))
    sampled_beam_from_config(model_cfg)
    diverse_beam_from_config(model_cfg)
    decode_rules_from_config(model_cfg)
    logit_rules_from_config(model_cfg)
    truncation_from_config(model_cfg)
    mirostat_from_config(model_cfg)
    arithmetic_from_config(model_cfg)
    from .contrast import contrast_from_config
    contrast_from_config(model_cfg)
    if sbs and kind != "beam":
        raise ValueError(f"MODEL.STOCHASTIC_BEAM_SEARCH needs MODEL.DECODE_SAMPLER 'beam', got {model_cfg.DECODE_SAMPLER!r} (the word "
                         "samplers draw one word per row; the stochastic beam search is a kind of beam search)")
    if kind == "beam":
        return GumbelSampler(temperature=T) if sbs else None
    if kind == "multinomial":
        return MultinomialSampler(temperature=T, with_replacement=rep)
    if kind == "top-k":
        return TopKSampler(k=int(model_cfg.SAMPLER_TOP_K), temperature=T, with_replacement=rep)
    if kind == "top-p":
        return TopPSampler(p=float(model_cfg.SAMPLER_TOP_P), temperature=T, with_replacement=rep)
    raise ValueError(f"MODEL.DECODE_SAMPLER must be one of 'beam', 'multinomial', 'top-k', 'top-p', got {model_cfg.DECODE_SAMPLER!r} "
                     "(for the Gumbel / stochastic beam sampler set MODEL.STOCHASTIC_BEAM_SEARCH True with DECODE_SAMPLER 'beam')")


def sampled_beam_from_config(model_cfg) -> bool:
    """MODEL.SAMPLED_BEAM_SEARCH: run the word sampler as the reference's BeamSearch does - per_node candidates per beam at
    BEAM_SIZE (DecodeEngine.sampled_beam).  Needs DECODE_SAMPLER multinomial / top-k / top-p and STOCHASTIC_BEAM_SEARCH False."""
    on = bool(getattr(model_cfg, "SAMPLED_BEAM_SEARCH", False))
    if on:
        kind = str(model_cfg.DECODE_SAMPLER).strip().lower()
        if kind not in KINDS:
            raise ValueError(f"MODEL.SAMPLED_BEAM_SEARCH needs MODEL.DECODE_SAMPLER 'multinomial', 'top-k' or 'top-p', got "
                             f"{model_cfg.DECODE_SAMPLER!r}")
        if bool(getattr(model_cfg, "STOCHASTIC_BEAM_SEARCH", False)):
            raise ValueError("MODEL.SAMPLED_BEAM_SEARCH and MODEL.STOCHASTIC_BEAM_SEARCH exclude each other (a word sampler's beam "
                             "search or the Gumbel sampler's)")
    return on
