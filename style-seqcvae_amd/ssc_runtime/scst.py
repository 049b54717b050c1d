"""Self-critical sequence training (SCST: Rennie et al. 2017; Luo 2020, "A better variant of self-critical sequence training"):
a train step whose captions are the model's own samples and whose per-caption weights are their rewards minus a baseline.

One step on P images with N latent samples each (G = P * N rows, row g = p * N + i):
  1. sample   DecodeEngine.sample draws G captions (word sampler: multinomial by default; prior noise from a device generator
              seeded by the caller's seed);
  2. reward   r_g = sum_k w_k score_k over the six columns of ssc_eval_score (B1..B4, ROUGE-L, CIDEr-D) against the image's
              references, prepared once over ALL reference images (CIDEr-D's document frequencies are the corpus's, not the batch's);
  3. baseline "loo": the mean reward of the image's other N - 1 samples; "greedy": the reward of one more caption per image,
              decoded with top-k = 1 and zero latent noise; "none";
  4. update   the samples are the `caps` of an ordinary train step with the upstream gradients gl_g = (r_g - b_g) / G and
              gk_g = 1 / (G * KLD_WEIGHT): the minimised quantity is sum_g gl_g loss_g + sum_g gk_g kld_g with loss_g, kld_g exactly what
              ssc_train_fwd returns for caption g - the training branch of the reference's forward() on sampled captions, its
              per-caption losses weighted by the advantage.  With z drawn from the posterior this is the advantage-weighted ELBO
              term, NOT an unbiased policy gradient of the prior-sampled decoder.
Steps 2 -> 4 are joined on the device by ssc_scst_prepare (csrc/scst.hip): no torch indexing, no read-back of rewards.

    scst = SelfCritical(train_engine, decode_engine, CaptionReferences(refs), vocabulary, n_samples=5)
    loss, kld, stats = scst.step(feats, image_ids, sentiment, lr=..., kld_weight=..., seed=scst_seed(RANDOM_SEED, iteration, rank))

Rewards and baselines are per rank; only gradients are exchanged (TrainEngine.backward_update).
"""
import ctypes as C
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np
import torch

from . import lib as _lib
from . import sampling
from .evaluation import MAX_SAMPLES, MAX_TOKENS, MAX_WORDS, UNKNOWN, CaptionReferences, _eval_score, _norm_id

BASELINES = {"none": 0, "loo": 1, "greedy": 2}
CIDER_ONLY = (0.0, 0.0, 0.0, 0.0, 0.0, 1.0)


def scst_seed(random_seed: int, iteration: int, rank: int = 0) -> int:
    """The seed of iteration `iteration` on rank `rank`: a function of the three numbers alone, so that a resumed run draws what
    the uninterrupted run would."""
    return ((int(random_seed) * 1000003 + int(iteration)) * 4099 + int(rank)) % (2 ** 62)


def parse_reward_weights(text: str):
    """"B1,B2,B3,B4,R,C" -> six floats."""
    w = tuple(float(x) for x in text.split(","))
    if len(w) != 6:
        raise ValueError(f"reward weights: six numbers B1,B2,B3,B4,R,C are needed, got {text!r}")
    return w


@dataclass
class Rollout:
    """What one rollout left on the device.  predictions (G, steps) as sampled; caps (G, L), lengths (G) int32: the train step's
    captions; reward, advantage, gl, gk (G) fp32; stats (4) fp64: mean reward, mean baseline, mean |advantage|, share of rows with
    no end; scores (P, N, 6) fp64; base_predictions / base_scores: the greedy baseline's captions (P, steps') and scores (P, 6), else
    None.  The noise used: eps0 (G, Z), eps (max_steps - 1, G, Z) of the decode, word_seed of the sampler, train_eps (L + 1, G, Z) of
    the train step's posterior.  feats (G, R, F), sentiment (G) or None, obj_atts (G, R, Z) or None: the train step's rows."""
    predictions: torch.Tensor
    caps: torch.Tensor
    lengths: torch.Tensor
    reward: torch.Tensor
    advantage: torch.Tensor
    gl: torch.Tensor
    gk: torch.Tensor
    stats: torch.Tensor
    scores: torch.Tensor
    ref_image: torch.Tensor
    base_predictions: Optional[torch.Tensor]
    base_scores: Optional[torch.Tensor]
    eps0: torch.Tensor
    eps: Optional[torch.Tensor]
    word_seed: int
    train_eps: torch.Tensor
    feats: torch.Tensor
    sentiment: Optional[torch.Tensor]
    obj_atts: Optional[torch.Tensor]


def scst_prepare(predictions, scores, base_scores, end_index, L, baseline, reward_weights, loss_scale, kld_scale):
    """ssc_scst_prepare on device tensors: predictions (G, steps) int64, scores (P, N, 6) fp64, base_scores (P, 6) fp64 or None.
    -> (caps (G, L), lengths, reward, advantage, gl, gk, stats), all on the device, nothing read back."""
    P, N = scores.shape[:2]
    G, steps = predictions.shape
    if G != P * N:
        raise ValueError(f"{G} prediction rows for {P} x {N} scores")
    assert predictions.dtype == torch.int64 and predictions.is_contiguous() and scores.dtype == torch.float64 and scores.is_contiguous()
    assert base_scores is None or (base_scores.dtype == torch.float64 and base_scores.is_contiguous() and base_scores.numel() == P * 6)
    dev = predictions.device
    caps = torch.empty(G, max(int(L), 0), dtype=torch.int64, device=dev)
    lengths = torch.empty(G, dtype=torch.int32, device=dev)
    reward, advantage, gl, gk = (torch.empty(G, dtype=torch.float32, device=dev) for _ in range(4))
    stats = torch.empty(4, dtype=torch.float64, device=dev)
    d = _lib.ScstDesc()
    d.P, d.N, d.steps, d.L, d.end_index = P, N, steps, int(L), int(end_index)
    d.predictions, d.scores, d.base_scores = predictions.data_ptr(), scores.data_ptr(), base_scores.data_ptr() if base_scores is not None else None
    for k in range(6):
        d.reward_weights[k] = float(reward_weights[k])
    d.baseline, d.loss_scale, d.kld_scale = int(baseline), float(loss_scale), float(kld_scale)
    d.caps, d.lengths, d.reward, d.advantage = caps.data_ptr(), lengths.data_ptr(), reward.data_ptr(), advantage.data_ptr()
    d.gl, d.gk, d.stats = gl.data_ptr(), gk.data_ptr(), stats.data_ptr()
    with torch.cuda.device(dev):
        _lib.load().ssc_scst_prepare(C.byref(d), _lib.stream_ptr())
    return caps, lengths, reward, advantage, gl, gk, stats


class SelfCritical:
    """The self-critical step over a TrainEngine and a DecodeEngine that read the same parameters.
    references: a CaptionReferences (an image without references gets reward 0 and, leave-one-out, advantage 0).
    vocabulary: a Vocabulary or the list of words by id (its @@UNKNOWN@@ matches no reference word); the captions end at the
    engines' boundary index.  sampler: a word sampler of ssc_runtime.sampling (default: multinomial, temperature 1).
    baseline: "loo" | "greedy" | "none".  reward_weights: (B1, B2, B3, B4, ROUGE-L, CIDEr-D), default CIDEr-D alone."""

    def __init__(self, train_engine, decode_engine, references: CaptionReferences, vocabulary, n_samples: int = 5, sampler=None,
                 baseline: str = "loo", reward_weights: Sequence[float] = CIDER_ONLY, max_steps: int = 20):
        if baseline not in BASELINES:
            raise ValueError(f"baseline must be one of {sorted(BASELINES)}, got {baseline!r}")
        if not 1 <= n_samples <= MAX_SAMPLES:
            raise ValueError(f"n_samples = {n_samples}: 1..{MAX_SAMPLES} are supported")
        if baseline == "loo" and n_samples < 2:
            raise ValueError("the leave-one-out baseline needs at least 2 samples per image")
        if not 1 <= max_steps <= MAX_TOKENS:
            raise ValueError(f"max_steps = {max_steps}: 1..{MAX_TOKENS} are supported (the scorer's caption length)")
        reward_weights = tuple(float(w) for w in reward_weights)
        if len(reward_weights) != 6:
            raise ValueError("reward_weights: six numbers (B1, B2, B3, B4, ROUGE-L, CIDEr-D)")
        if sampler is not None and getattr(sampler, "beam_search", False):
            raise ValueError(f"sampler {sampler!r} is a beam search: the self-critical step draws one caption per row")
        self.eng, self.dec, self.refs = train_engine, decode_engine, references
        self.n_samples, self.baseline, self.reward_weights, self.max_steps = n_samples, baseline, reward_weights, max_steps
        self.sampler = sampler if sampler is not None else sampling.MultinomialSampler()
        self.end_index = train_engine.dims.boundary
        if hasattr(vocabulary, "get_vocab_size"):
            words = [vocabulary.get_token_from_index(i) for i in range(vocabulary.get_vocab_size())]
        else:
            words = list(vocabulary)
        if len(words) != train_engine.dims.V:
            raise ValueError(f"the vocabulary holds {len(words)} words, the model {train_engine.dims.V}")
        if len(words) > MAX_WORDS:
            raise ValueError(f"{len(words)} prediction ids: at most {MAX_WORDS} are supported")
        dev = train_engine.device
        id_map = np.array([references.word_id.get(w, 0) for w in words], dtype=np.int32)
        if UNKNOWN in words:
            id_map[words.index(UNKNOWN)] = 0
        self._id_map = torch.from_numpy(id_map).to(dev)
        self._V = len(words)
        self._prep = references.prepared(references.image_ids)   # once: every score call of every step reads it

    # ---- rollout ---------------------------------------------------------------------------------------
    def _ref_image(self, image_ids, P):
        if len(image_ids) != P:
            raise ValueError(f"{len(image_ids)} image ids for {P} images")
        if torch.is_tensor(image_ids):
            image_ids = image_ids.tolist()
        rows = [self._prep.index.get(_norm_id(i), -1) for i in image_ids]
        return torch.tensor(rows, dtype=torch.int32, device=self.eng.device)

    def rollout(self, feats, image_ids, sentiment, seed: int, obj_atts=None, kld_weight: float = 750.0) -> Rollout:
        """feats (P, R, F) fp32 on the device, image_ids (P) keys of the references, sentiment (P) or None, obj_atts (P, R, Z) for
        SENTIMENT_VAE = 2.  Samples, scores and prepares the train step's inputs; changes no parameter.
        The train step reads its features per row: they are expanded to (G, R, F) with repeat_interleave - G * R * F * 4 bytes
        (C2 widths, P = 32, N = 5, R = 36: 47 MB)."""
        if self.dec.weights_frozen:
            raise ValueError("DecodeEngine.weights_frozen is set: the self-critical step changes the weights between rollouts")
        eng, dec, N = self.eng, self.dec, self.n_samples
        dev, Z = eng.device, eng.dims.Z
        P, R, _ = feats.shape
        G = P * N
        feats = feats.to(dev, torch.float32).contiguous()
        if eng.lib.ssc_train_workspace_bytes(C.byref(eng._cfg), G, R, self.max_steps) == 0:
            raise ValueError(f"{P} images x {N} samples = {G} rows of {R} regions: not a batch the train step accepts")
        ref_image = self._ref_image(image_ids, P)
        sent = sentiment.reshape(P).to(dev, torch.float32) if sentiment is not None else None
        sent_rows = sent.repeat_interleave(N) if sent is not None else None
        ctx = dec.prepare(feats, obj_atts)
        gen = torch.Generator(device=dev)
        gen.manual_seed(int(seed))
        steps = self.max_steps
        eps0 = torch.randn(G, Z, device=dev, generator=gen)
        eps = torch.randn(steps - 1, G, Z, device=dev, generator=gen) if steps > 1 else None
        with torch.no_grad():
            pred, _ = dec.sample(ctx, sent_rows, N, steps, self.end_index, eps0, eps, self.sampler, int(seed))
            base_pred = base_scores = None
            if self.baseline == "greedy":
                z0 = torch.zeros(P, Z, device=dev)
                zs = torch.zeros(steps - 1, P, Z, device=dev) if steps > 1 else None
                base_pred, _ = dec.sample(ctx, sent, 1, steps, self.end_index, z0, zs, sampling.TopKSampler(k=1), int(seed))
                base_scores = _eval_score(self._prep, base_pred.view(P, 1, -1), self.end_index, self._V, self._id_map, None,
                                          ref_image)[0].view(P, 6)
            L = pred.size(1)
            scores = _eval_score(self._prep, pred.view(P, N, L), self.end_index, self._V, self._id_map, None, ref_image)[0]
            caps, lengths, reward, advantage, gl, gk, stats = scst_prepare(
                pred, scores, base_scores, self.end_index, L, BASELINES[self.baseline], self.reward_weights, 1.0 / G,
                1.0 / (G * float(kld_weight)))
            train_eps = torch.randn(L + 1, G, Z, device=dev, generator=gen)
            obj_rows = obj_atts.to(dev, torch.float32).repeat_interleave(N, dim=0) if (obj_atts is not None and eng.dims.kld_mode == 2) else None
            return Rollout(pred, caps, lengths, reward, advantage, gl, gk, stats, scores, ref_image, base_pred, base_scores, eps0, eps,
                           int(seed), train_eps, feats.repeat_interleave(N, dim=0), sent_rows, obj_rows)

    # ---- step ---------------------------------------------------------------------------------------------
    def step(self, feats, image_ids, sentiment, lr, kld_weight=750.0, momentum=0.9, weight_decay=0.001, max_norm=12.5,
             decoder_frozen=False, group=None, seed: int = 0, obj_atts=None, optim=None):
        """A rollout, then the train step on its captions with its upstream gradients: forward, and the backward / all-reduce /
        clip / SGD path TrainEngine.train_step takes (optim: an engine.OptimSpec - Adam or AdamW behind the clip instead).
        -> (loss (G,), kld (G,), stats (4,) fp64 on the device)."""
        ro = self.rollout(feats, image_ids, sentiment, seed, obj_atts, kld_weight)
        loss, kld = self.eng.forward(ro.feats, ro.caps, ro.sentiment, ro.train_eps, ro.obj_atts)
        self.eng.backward_update(ro.gl, ro.gk, lr, momentum, weight_decay, max_norm, decoder_frozen, group, optim)
        return loss, kld, ro.stats
