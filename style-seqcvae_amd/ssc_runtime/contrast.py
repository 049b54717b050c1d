"""Contrastive decoding for the word samplers (ssc_contrast in include/ssc.h; Li et al. 2023, Leng et al. 2023).

A second, *amateur* stream is decoded in lock-step with the normal *expert* stream, fed the same words, and every step's raw logits
become  lp_e + alpha * (lp_e - lp_a)  on the expert's plausible words (lp_e >= log(beta) + max lp_e), -inf elsewhere, in front of the
logit rules, the truncation and the unchanged draw (DecodeEngine.sample(contrast=) / ssc_sample_opts.contrast).  What the amateur
lacks is what the decode gets more of:

    Contrast(1.0, features="mean")            the image: every region replaced by the image's mean region - the language prior
    Contrast(1.0, features="noise:0.5")       the image under diffusion-style noise (visual contrastive decoding)
    Contrast(1.0, latent="mean")              the latent: z at the prior mean - a guidance scale for z
    Contrast(1.0, sentiment=0.0)              the style: a neutral sentiment
    Contrast(1.0, guide="prior")              the exemplar: the amateur ignores the call's latent guide
    Contrast(1.0, engine=early_checkpoint)    the training: a weak checkpoint of the same configuration

The KL between the two streams' word distributions comes out of the same pass (contrast_stats=True): per word, how much it depended on
what the amateur lacks.  Greedy contrastive decoding is the top-k sampler with k = 1.
"""
import ctypes as C
import math
from typing import Optional, Union

import torch

from . import lib as _lib

AMATEURS = ("mean-features", "noise-features", "prior-mean", "neutral-sentiment")
GUIDE_MODES = {"shared": 0, "prior": 1}


def amateur_features(feats: torch.Tensor, kind: str, generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """The amateur's view of feats (nimg, R, F), made on the host of the tensors' device with plain tensor operations, once per
    call.  "mean": every non-padded region becomes the mean of its image's non-padded regions.  "noise:g", 0 < g <= 1:
    sqrt(1 - g) f + sqrt(g) std_image n with n ~ N(0, 1) from `generator` and std_image the standard deviation of the image's
    non-padded entries.  A padded region - all zeros - stays zero in both, so the region mask does not change."""
    if feats.dim() != 3:
        raise ValueError(f"amateur_features: feats must be (nimg, R, F), got {tuple(feats.shape)}")
    f = feats.to(torch.float32)
    live = (f != 0).any(-1, keepdim=True)                                  # (nimg, R, 1): the regions the mask keeps
    n = live.sum(1, keepdim=True).clamp(min=1).to(torch.float32)           # (nimg, 1, 1)
    mean = (f * live).sum(1, keepdim=True) / n                             # (nimg, 1, F)
    if kind == "mean":
        return torch.where(live, mean.expand_as(f), torch.zeros_like(f)).contiguous()
    g = _noise_level(kind)
    cnt = n * f.size(2)
    mu = (f * live).sum((1, 2), keepdim=True) / cnt
    std = ((((f - mu) * live) ** 2).sum((1, 2), keepdim=True) / cnt).sqrt()
    noise = torch.randn(f.shape, device=f.device, dtype=torch.float32, generator=generator)
    out = math.sqrt(1.0 - g) * f + math.sqrt(g) * std * noise
    return torch.where(live, out, torch.zeros_like(f)).contiguous()


def _noise_level(kind: str) -> float:
    name, _, value = str(kind).partition(":")
    try:
        g = float(value)
    except ValueError:
        g = float("nan")
    if name != "noise" or not (0.0 < g <= 1.0):
        raise ValueError(f'Contrast: features must be a tensor, "mean" or "noise:g" with 0 < g <= 1, got {kind!r}')
    return g


class Contrast:
    """The contrast of a word-sampled decode and the description of its amateur.
    alpha >= 0: the weight of lp_e - lp_a (0: the plausibility cut alone - no amateur is decoded); beta in [0, 1): a word is kept
    iff its expert probability is at least beta times the top word's (0: every word).  Both 0: inactive - the plain call.
    The amateur is the expert except for what is set here:
      engine     another DecodeEngine of the same dims (a checkpoint): its parameters; its image context is prepared from the
                 amateur's features (the expert's, unless `features` says otherwise)
      features   a (nimg, R, F) tensor, "mean" or "noise:g" (amateur_features); generator: the noise's generator
      latent     "mean": zero noise - z at the prior mean (at a guide's mean, where the amateur follows a guide)
      sentiment  a number or a tensor (nimg,) / (B,): the amateur's sentiment
      guide      "shared": the amateur follows the call's latent guide; "prior": it ignores it
    prepare() forms the amateur's image context for a call (DecodeEngine.sample and diverse_decode call it); start carries the
    amateur's primed StartState where the call has a start= (diverse_decode(prefix=) sets it)."""

    def __init__(self, alpha: float, beta: float = 0.1, engine=None, features: Union[None, str, torch.Tensor] = None,
                 latent: Optional[str] = None, sentiment=None, guide: str = "shared", generator: Optional[torch.Generator] = None):
        alpha, beta = float(alpha), float(beta)
        if not (alpha >= 0.0 and math.isfinite(alpha)):
            raise ValueError(f"Contrast: alpha must be finite and >= 0, got {alpha!r}")
        if not (0.0 <= beta < 1.0):
            raise ValueError(f"Contrast: beta must lie in [0, 1), got {beta!r}")
        if isinstance(features, str) and features != "mean":
            _noise_level(features)
        elif features is not None and not isinstance(features, (str, torch.Tensor)):
            raise ValueError(f'Contrast: features must be a tensor, "mean" or "noise:g", got {features!r}')
        if latent not in (None, "mean"):
            raise ValueError(f'Contrast: latent must be None or "mean", got {latent!r}')
        if guide not in GUIDE_MODES:
            raise ValueError(f'Contrast: guide must be "shared" or "prior", got {guide!r}')
        self.alpha, self.beta = alpha, beta
        self.engine, self.features, self.latent, self.sentiment, self.guide = engine, features, latent, sentiment, guide
        self.generator = generator
        self.ctx = None     # the amateur's ImageContext of the current call (prepare) ...
        self._for = None    # ... and the expert's features it was formed for
        self.start = None   # the amateur's StartState of the current call

    active = property(lambda self: self.alpha != 0.0 or self.beta != 0.0)
    steps_amateur = property(lambda self: self.alpha != 0.0)
    own_context = property(lambda self: self.engine is not None or self.features is not None)

    def check_engine(self, dec):
        """The amateur's engine must have the expert's dims: one ssc_model_cfg describes both parameter sets."""
        if self.engine is not None and self.engine.dims != dec.dims:
            raise ValueError("Contrast: the amateur's engine must have the dims of the expert's (checkpoints of one configuration)")

    def prepare(self, dec, feats: torch.Tensor, obj_means: Optional[torch.Tensor] = None,
                generator: Optional[torch.Generator] = None) -> "Contrast":
        """Form the amateur's image context for a call over feats (nimg, R, F) on the expert engine `dec`: the amateur's features
        under the amateur's parameters.  generator: the call's, for "noise:g" features (default: the Contrast's own, else the
        global one).  Nothing to do for an amateur that shares the expert's context, or is never stepped."""
        self.ctx = self._for = None
        if not (self.steps_amateur and self.own_context):
            return self
        self.check_engine(dec)
        if isinstance(self.features, torch.Tensor):
            af = self.features.to(feats.device, torch.float32)
            if tuple(af.shape) != tuple(feats.shape):
                raise ValueError(f"Contrast: the amateur's features are {tuple(af.shape)}, the call's {tuple(feats.shape)}")
        elif self.features is not None:
            af = amateur_features(feats, self.features, generator if generator is not None else self.generator)
        else:
            af = feats
        if bool((af == 0).all()):
            raise ValueError("Contrast: the amateur's features are all zero: every region would be masked")
        self.ctx = (self.engine or dec).prepare(af, obj_means)
        self._for = feats
        return self

    def desc(self, dec, ctx, n_samples: int, max_steps: int, has_start: bool, kept: Optional[torch.Tensor] = None,
             divergence: Optional[torch.Tensor] = None):
        """-> (ssc_contrast for a call of `dec` over the expert context `ctx`, everything it points to: keep it until the call is
        queued).  kept / divergence: (max_steps, B) int32 / float32 blocks or None."""
        dev, Z = dec.device, dec.dims.Z
        B = ctx.nimg * n_samples
        cd = _lib.Contrast()
        keep = [kept, divergence]
        cd.alpha, cd.beta = self.alpha, self.beta
        cd.kept, cd.divergence = _lib.ptr(kept), _lib.ptr(divergence)
        cd.guide_mode = GUIDE_MODES[self.guide]
        if not self.steps_amateur:
            return cd, keep
        self.check_engine(dec)
        if self.own_context:
            if self.ctx is None or self._for is not ctx.feats:   # (not prepared for this call's images)
                self.prepare(dec, ctx.feats, ctx.obj)
            if (self.ctx.nimg, self.ctx.R) != (ctx.nimg, ctx.R):
                raise ValueError(f"Contrast: the amateur's context holds {self.ctx.nimg} images of {self.ctx.R} regions, the call's "
                                 f"{ctx.nimg} of {ctx.R}")
            cd.feats, cd.imgbuf, cd.obj_atts = self.ctx.feats.data_ptr(), self.ctx.buf.data_ptr(), _lib.ptr(self.ctx.obj)
            keep.append(self.ctx)
        if self.engine is not None:
            p = self.engine._params()
            cd.params = C.addressof(p)
            keep.append(p)
        if self.sentiment is not None:
            s = torch.as_tensor(self.sentiment, dtype=torch.float32).to(dev)
            if s.numel() == 1:
                s = s.reshape(1).expand(B)
            elif s.numel() == ctx.nimg:
                s = s.reshape(ctx.nimg, 1).expand(ctx.nimg, n_samples)
            elif s.numel() != B:
                raise ValueError(f"Contrast: sentiment holds {s.numel()} values for {ctx.nimg} images x {n_samples} samples")
            s = s.reshape(B).contiguous()
            cd.sentiment = s.data_ptr()
            keep.append(s)
        if self.latent == "mean":
            e0 = torch.zeros(B, Z, dtype=torch.float32, device=dev)
            e = torch.zeros(max(max_steps - 1, 1), B, Z, dtype=torch.float32, device=dev)
            cd.eps0, cd.eps = e0.data_ptr(), e.data_ptr()
            keep += [e0, e]
        if has_start:
            if self.start is None:
                raise ValueError("Contrast: the call has a start state (start=) - the amateur needs its own (Contrast.start, "
                                 "DecodeEngine.prime over the amateur's context)")
            sdesc, sk = self.start.desc(dev, B, dec.dims.H)
            cd.start = C.pointer(sdesc)
            keep += [sdesc, sk]
        return cd, keep


def contrast_from_config(model_cfg) -> Optional[Contrast]:
    """MODEL.CONTRAST_ALPHA / CONTRAST_BETA / CONTRAST_AMATEUR / CONTRAST_NOISE -> the run's Contrast, or None with
    CONTRAST_ALPHA 0."""
    if float(getattr(model_cfg, "CONTRAST_ALPHA", 0.0)) == 0.0:
        return None
    kind = str(model_cfg.DECODE_SAMPLER).strip().lower()
    if kind not in ("multinomial", "top-k", "top-p"):
        raise ValueError(f"MODEL.CONTRAST_ALPHA needs MODEL.DECODE_SAMPLER 'multinomial', 'top-k' or 'top-p', got "
                         f"{model_cfg.DECODE_SAMPLER!r} (the contrast belongs to the word samplers)")
    for other in ("SAMPLED_BEAM_SEARCH", "STOCHASTIC_BEAM_SEARCH"):
        if bool(getattr(model_cfg, other, False)):
            raise ValueError(f"MODEL.CONTRAST_ALPHA and MODEL.{other} exclude each other (the contrast belongs to the word-sampled "
                             "decode)")
    return contrast_from_name(float(model_cfg.CONTRAST_ALPHA), float(model_cfg.CONTRAST_BETA), str(model_cfg.CONTRAST_AMATEUR),
                              float(model_cfg.CONTRAST_NOISE))


def contrast_from_name(alpha: float, beta: float, amateur: str, noise: float = 0.5, engine=None) -> Contrast:
    """The Contrast of an amateur kind of the configuration: mean-features | noise-features | prior-mean | neutral-sentiment."""
    if amateur not in AMATEURS:
        raise ValueError(f"the amateur must be one of {' | '.join(AMATEURS)}; found {amateur!r}")
    kw = {"mean-features": {"features": "mean"}, "noise-features": {"features": f"noise:{noise!r}"},
          "prior-mean": {"latent": "mean"}, "neutral-sentiment": {"sentiment": 0.0}}[amateur]
    return Contrast(alpha, beta, engine=engine, **kw)
