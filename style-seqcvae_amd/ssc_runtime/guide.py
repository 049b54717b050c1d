"""Latent-guided decoding (include/ssc.h: ssc_latent_guide): decode under a caption's posterior instead of the configured prior.

A LatentGuide gives every batch entry of a one-call decode, per step, the distribution its latent z_t is drawn from.  The builders
here - encode_captions, LatentGuide.from_encoding, LatentGuide.lerp - are torch ops that run once per call, off the step path; the
step path is DecodeEngine.search / sample / score(guide=...), one library call each.  reconstruct_captions is the standard check of
how much z carries: decode each caption under its own z path and compare (ssc_caption_match)."""
import math
from dataclasses import dataclass
from typing import Dict, NamedTuple, Optional

import torch

from . import lib as _lib

FEATURE = "latent guides (guide=)"


def guide_unsupported(what: str):
    """The error of every decoder that takes no guide."""
    raise NotImplementedError(f"{FEATURE} are not implemented for {what}: they steer the beam search (plain or constrained), the "
                              "sampled decode and caption scoring of a single engine")


class Encoding(NamedTuple):
    """What encode_captions returns: the posterior branch's latent path of every caption.  z, mu, lv (T, B, Z) - the stored z of ONE
    forward, and the mean and log-variance q(z_t | x, z_<t) it was drawn from - and length (B) int32: the steps of every caption,
    its END included (the steps with a non-zero weight)."""
    z: torch.Tensor
    mu: torch.Tensor
    lv: torch.Tensor
    length: torch.Tensor


def encode_captions(train_engine, feats: torch.Tensor, caps: torch.Tensor, sentiment: Optional[torch.Tensor],
                    eps: Optional[torch.Tensor] = None, obj_atts: Optional[torch.Tensor] = None) -> Encoding:
    """The latent path of given captions: feats (B, R, F), caps (B, L) int64 in the training layout (the words, then pad),
    sentiment (B,) or None, through TrainEngine.posterior_forward.  eps (L + 1, B, Z): the posterior's noise; None: zero noise -
    the mean path, z_t = mu_t.  Each mu_t depends on the earlier z, so a guide is the stored z of one forward, never a mu paired
    with fresh noise (LatentGuide.from_encoding)."""
    d = train_engine.dims
    dev = train_engine.device
    B, L = caps.shape
    feats = feats.to(dev, torch.float32).contiguous()
    caps = caps.to(dev, torch.int64).contiguous()
    if eps is None:
        eps = torch.zeros(L + 1, B, d.Z, dtype=torch.float32, device=dev)
    else:
        if tuple(eps.shape) != (L + 1, B, d.Z):
            raise ValueError(f"eps must be (L + 1, B, Z) = {(L + 1, B, d.Z)}, got {tuple(eps.shape)}")
        eps = eps.to(dev, torch.float32).contiguous()
    sent = sentiment.to(dev, torch.float32) if sentiment is not None else None
    train_engine.posterior_forward(feats, caps, sent, eps, obj_atts)
    z = train_engine.posterior_view("z").clone()
    mu = train_engine.posterior_view(7).clone()
    lv = train_engine.posterior_view(8).clone()
    length = (train_engine.posterior_view("w") != 0).sum(0).to(torch.int32)
    return Encoding(z, mu, lv, length)


class LatentGuide:
    """mean (T, B, Z): the latent of step t of batch entry b is drawn around mean[t, b]; var (T, B, Z) or None: its variance - None:
    z = mean, no noise is read; length (B) or None: entry b is guided for the steps t < length[b] (None: all T) and decodes under
    the prior from then on, as every entry does from step T on.  B: nimg * n_samples entries (image, sample) for search / sample,
    nimg * C * n_samples rows (image, caption, sample) for score.  A negative variance gives NaN latents."""

    def __init__(self, mean: torch.Tensor, var: Optional[torch.Tensor] = None, length: Optional[torch.Tensor] = None):
        if mean.dim() != 3 or mean.size(0) < 1 or mean.size(1) < 1:
            raise ValueError(f"LatentGuide: mean must be (T, B, Z) with T, B >= 1, got {tuple(mean.shape)}")
        if var is not None and tuple(var.shape) != tuple(mean.shape):
            raise ValueError(f"LatentGuide: var {tuple(var.shape)} does not match mean {tuple(mean.shape)}")
        if length is not None and tuple(length.shape) != (mean.size(1),):
            raise ValueError(f"LatentGuide: length must be (B,) = ({mean.size(1)},), got {tuple(length.shape)}")
        self.mean = mean.to(torch.float32)
        self.var = var.to(torch.float32) if var is not None else None
        self.length = length.to(torch.int32) if length is not None else None

    steps = property(lambda self: self.mean.size(0))
    B = property(lambda self: self.mean.size(1))
    Z = property(lambda self: self.mean.size(2))

    @staticmethod
    def from_encoding(enc: Encoding, jitter: float = 0.0, repeat: int = 1) -> "LatentGuide":
        """The guide of an encoding: mean = the stored z, var = jitter^2 exp(lv) (None at jitter 0: the path itself), length = the
        captions' steps; every entry repeated `repeat` times in place (entry (b, n) = b * repeat + n: one per latent sample)."""
        jitter = float(jitter)
        if not math.isfinite(jitter) or jitter < 0:
            raise ValueError(f"LatentGuide.from_encoding: jitter must be finite and >= 0, got {jitter}")
        if repeat < 1:
            raise ValueError(f"LatentGuide.from_encoding: repeat must be at least 1, got {repeat}")
        rep = lambda t, dim: t.repeat_interleave(repeat, dim) if repeat > 1 else t
        var = rep((jitter * jitter) * torch.exp(enc.lv), 1) if jitter > 0 else None
        return LatentGuide(rep(enc.z, 1), var, rep(enc.length, 0))

    @staticmethod
    def lerp(a: "LatentGuide", b: "LatentGuide", lam: float) -> "LatentGuide":
        """The guide between two: means and standard deviations mixed linearly, (1 - lam) a + lam b, over the steps both have; the
        length is the shorter of the two."""
        lam = float(lam)
        if not math.isfinite(lam):
            raise ValueError(f"LatentGuide.lerp: lam must be finite, got {lam}")
        if a.B != b.B or a.Z != b.Z:
            raise ValueError(f"LatentGuide.lerp: guides of different extent: (B, Z) = {(a.B, a.Z)} and {(b.B, b.Z)}")
        T = min(a.steps, b.steps)
        mean = (1.0 - lam) * a.mean[:T] + lam * b.mean[:T].to(a.mean.device)
        var = None
        if a.var is not None or b.var is not None:
            sd = lambda g: torch.sqrt(g.var[:T]).to(mean.device) if g.var is not None else torch.zeros_like(mean)
            var = ((1.0 - lam) * sd(a) + lam * sd(b)) ** 2
        length = None
        if a.length is not None or b.length is not None:
            ln = lambda g: g.length.to(mean.device) if g.length is not None else torch.full((a.B,), g.steps, dtype=torch.int32, device=mean.device)
            length = torch.minimum(ln(a), ln(b)).clamp(max=T)
        return LatentGuide(mean, var, length)

    def desc(self, device, B: int, Z: int):
        """-> (ssc_latent_guide over contiguous device tensors, those tensors: keep them until the call is queued)."""
        if self.B != B or self.Z != Z:
            raise ValueError(f"the guide is for (B, Z) = {(self.B, self.Z)}; this call has {B} entries of Z = {Z}")
        mean = self.mean.to(device).contiguous()
        var = self.var.to(device).contiguous() if self.var is not None else None
        length = self.length.to(device).contiguous() if self.length is not None else None
        return _lib.LatentGuideDesc(self.steps, _lib.ptr(mean), _lib.ptr(var), Z, _lib.ptr(length)), (mean, var, length)


MATCH_MAX_LEN = 128


def caption_match(pred: torch.Tensor, ref: torch.Tensor, end_index: int) -> torch.Tensor:
    """pred (n, Lp), ref (n, Lr) int64 on the device -> (n, 5) int32: n_pred, n_ref, equal positions below the shorter length, exact
    (0 / 1), word-level Levenshtein distance; a caption's length is the tokens before its first end_index or negative id
    (ssc_caption_match)."""
    if pred.dim() != 2 or ref.dim() != 2 or pred.size(0) != ref.size(0):
        raise ValueError(f"caption_match: pred (n, Lp) and ref (n, Lr), got {tuple(pred.shape)} and {tuple(ref.shape)}")
    if not (1 <= pred.size(1) <= MATCH_MAX_LEN and 1 <= ref.size(1) <= MATCH_MAX_LEN):
        raise ValueError(f"caption_match: caption widths must be in [1, {MATCH_MAX_LEN}], got {pred.size(1)} and {ref.size(1)}")
    lib = _lib.load()
    pred = pred.to(torch.int64).contiguous()
    ref = ref.to(pred.device, torch.int64).contiguous()
    out = torch.empty(pred.size(0), 5, dtype=torch.int32, device=pred.device)
    lib.ssc_caption_match(_lib.ptr(pred), pred.size(1), _lib.ptr(ref), ref.size(1), pred.size(0), end_index, _lib.ptr(out),
                          _lib.stream_ptr())
    return out


def match_summary(match: torch.Tensor) -> Dict[str, float]:
    """Means over the pairs of a caption_match result: token_accuracy = sum equal / sum max(n_pred, n_ref), exact_rate, wer =
    sum distance / sum n_ref (pairs with an empty reference count in the numerator only)."""
    m = match.to("cpu", torch.float64)
    longest = torch.maximum(m[:, 0], m[:, 1]).sum().item()
    return {"n_pairs": int(m.size(0)), "token_accuracy": m[:, 2].sum().item() / max(longest, 1.0),
            "exact_rate": m[:, 3].mean().item() if m.size(0) else 0.0, "wer": m[:, 4].sum().item() / max(m[:, 1].sum().item(), 1.0)}


@dataclass
class Reconstruction:
    """What reconstruct_captions returns.  predictions (B, steps): the captions decoded under their own z path; match (B, 5) int32:
    ssc_caption_match's columns against the given captions; token_accuracy, exact_rate, wer: their means (match_summary);
    guided_log_prob (B,): the teacher-forced log-prob of the GIVEN caption under its z path; prior_log_prob (B,): its Monte-Carlo
    marginal under prior samples; z_gain (B,) = guided - prior: what z buys, in nats per caption (both None with prior_samples 0)."""
    predictions: torch.Tensor
    match: torch.Tensor
    token_accuracy: float
    exact_rate: float
    wer: float
    guided_log_prob: torch.Tensor
    prior_log_prob: Optional[torch.Tensor]
    z_gain: Optional[torch.Tensor]


def reconstruct_captions(train_engine, dec, feats: torch.Tensor, sentiment: Optional[torch.Tensor], captions: torch.Tensor, beam: int,
                         boundary_index: int, max_steps: Optional[int] = None, eps: Optional[torch.Tensor] = None,
                         prior_samples: int = 4, pad_index: int = 0, prior_seed: Optional[int] = None) -> Reconstruction:
    """Reconstruction through z: feats (B, R, F), sentiment (B,) or None, captions (B, L) int64 in the training layout - one
    caption per image.  Each caption is encoded on its image (encode_captions; eps None: the mean path), decoded back by the beam
    search under its own z path (DecodeEngine.search(guide=...), no noise), compared with the given words (ssc_caption_match) and
    scored teacher-forced under the guide and under prior_samples draws from the prior (DecodeEngine.score; 0: not scored under the
    prior).  The prior draws come from a generator of the call's own seeded by prior_seed (None: ONE draw of the global CPU
    generator); with prior_samples 0 the call is deterministic and draws nothing."""
    if captions.dim() != 2 or captions.size(0) != feats.size(0):
        raise ValueError(f"captions must be (B, L) with B = {feats.size(0)}, got {tuple(captions.shape)}")
    dev = dec.device
    d = dec.dims
    B, L = captions.shape
    caps = captions.to(dev, torch.int64)
    is_pad = caps == pad_index
    n_words = torch.where(is_pad.any(-1), is_pad.float().argmax(-1), torch.full((B,), L, device=dev))
    caps = torch.where(torch.arange(L, device=dev).view(1, -1) >= n_words.view(-1, 1), torch.full_like(caps, pad_index), caps)
    enc = encode_captions(train_engine, feats, caps, sentiment, eps)
    guide = LatentGuide.from_encoding(enc)
    steps = int(max_steps) if max_steps is not None else L + 1
    per_node = (beam // 2) or beam
    feats = feats.to(dev, torch.float32)
    ctx = dec.prepare(feats)
    sent = sentiment.reshape(B).to(dev, torch.float32) if sentiment is not None else None
    zeros = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)
    pred, _ = dec.search(ctx, sent, 1, beam, per_node, steps, boundary_index, zeros(B, d.Z), zeros(max(steps - 1, 1), B * beam, d.Z),
                         guide=guide)
    pred = pred[:, 0, 0, :].contiguous()
    # the given captions as the decoders write them: the words, then END
    ref = torch.where(torch.arange(L + 1, device=dev).view(1, -1) >= n_words.view(-1, 1),
                      torch.full((B, L + 1), boundary_index, dtype=torch.int64, device=dev),
                      torch.nn.functional.pad(caps, (0, 1), value=boundary_index))
    match = caption_match(pred, ref, boundary_index)
    s = match_summary(match)
    T = L + 1
    tg = ref.view(B, 1, T)
    g_lp, _, _, _ = dec.score(ctx, sent, tg, 1, boundary_index, zeros(B, d.Z), zeros(max(T - 1, 1), B, d.Z)[: T - 1] if T > 1 else None,
                              guide=guide)
    N = int(prior_samples)
    if N < 1:
        return Reconstruction(pred, match, s["token_accuracy"], s["exact_rate"], s["wer"], g_lp, None, None)
    gen = torch.Generator(device=dev)
    gen.manual_seed(int(prior_seed) if prior_seed is not None else int(torch.randint(0, 2 ** 62, (1,)).item()))
    sent_n = sent.repeat_interleave(N) if sent is not None else None
    p_lp, _, _, _ = dec.score(ctx, sent_n, tg, N, boundary_index, torch.randn(B * N, d.Z, device=dev, generator=gen),
                              torch.randn(T - 1, B * N, d.Z, device=dev, generator=gen) if T > 1 else None)
    prior = torch.logsumexp(p_lp.view(B, N), -1) - math.log(N)
    return Reconstruction(pred, match, s["token_accuracy"], s["exact_rate"], s["wer"], g_lp, prior, g_lp - prior)
