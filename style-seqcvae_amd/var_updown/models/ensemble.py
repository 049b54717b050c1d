"""CaptionerEnsemble: several UpDownCaptioners of one configuration (checkpoints of one run: seeds, cross-entropy or
self-critical training, SGD or Adam) decoded as ONE beam search, their word distributions averaged at every step
(ssc_runtime.decode.EnsembleDecodeEngine, ssc_decode_search_ensemble).  Eval only."""
from typing import Optional

import torch
from torch import nn

from ssc_runtime.decode import ENSEMBLE_MODES, EnsembleDecodeEngine, ensemble_weights
from ssc_runtime.decoding import select_best_beam_simple_batched

from .updown_captioner import UpDownCaptioner

# what two members must agree on besides their architecture (ModelDims) and vocabulary: how the eval forward decodes
_DECODE_ATTRS = ("_max_caption_length", "_use_cbs", "_min_constraints_to_satisfy", "cbs_simple", "latent_embedding",
                 "latent_embedding_multip", "simple_vae", "sentiment_vae")


class CaptionerEnsemble(nn.Module):
    """captioners: 1 .. 8 UpDownCaptioners built from the same configuration over the same vocabulary; weights: positive, any
    scale (None: uniform); mode "prob" (mean of the probabilities) or "logprob" (normalised mean of the log-probs).  The eval
    forward takes UpDownCaptioner.forward's arguments and returns what its eval forward returns, {"predictions": (B, steps)}: beam
    0 of the beam search at member 0's BEAM_SIZE (with a constraint machine, CBS_SIMPLE's pick over the states).  The latent
    noise is drawn as member 0 draws it and is the same for every member.  Samplers, the diverse beam search, the decode rules and
    attention traces belong to a single captioner."""

    def __init__(self, captioners, weights=None, mode: str = "prob"):
        super().__init__()
        captioners = list(captioners)
        if not captioners or not all(isinstance(c, UpDownCaptioner) for c in captioners):
            raise ValueError("CaptionerEnsemble: needs at least one UpDownCaptioner")
        if len(captioners) > 8:
            raise ValueError(f"CaptionerEnsemble: at most 8 members, got {len(captioners)}")
        if mode not in ENSEMBLE_MODES:
            raise ValueError(f"CaptionerEnsemble: unknown mode {mode!r} (one of {sorted(ENSEMBLE_MODES)})")
        lead = captioners[0]
        words = lead._vocabulary.get_index_to_token_vocabulary()
        for i, c in enumerate(captioners[1:], 1):
            if c._vocabulary.get_index_to_token_vocabulary() != words:
                raise ValueError(f"CaptionerEnsemble: member {i} has another vocabulary than member 0")
            if c._dims() != lead._dims():
                raise ValueError(f"CaptionerEnsemble: member {i} has another configuration than member 0: {c._dims()} != {lead._dims()}")
            diff = [a for a in _DECODE_ATTRS if getattr(c, a) != getattr(lead, a)]
            if diff or c._beam_search.beam_size != lead._beam_search.beam_size:
                raise ValueError(f"CaptionerEnsemble: member {i} has another configuration than member 0 ({', '.join(diff) or 'beam size'})")
        for c in captioners:
            if c.sampler is not None or c.diverse_beam is not None or c.decode_rules is not None or c._decode_attention is not None:
                raise ValueError("CaptionerEnsemble: ensemble decoding runs the beam search only - build the members without a "
                                 "sampler, diverse_beam, decode rules and decode_attention")
        self.weights = ensemble_weights(weights, len(captioners))
        self.mode = mode
        self.members = nn.ModuleList(captioners)
        self._ens: Optional[EnsembleDecodeEngine] = None
        super().train(False)   # (an eval-time module from the start, its members with it)

    def train(self, mode: bool = True):
        if mode:
            raise RuntimeError("CaptionerEnsemble is an eval-time decoder: train its members one by one")
        return super().train(False)

    def engine(self) -> EnsembleDecodeEngine:
        """The members' decode engines as one EnsembleDecodeEngine (their parameters adopted as they are now)."""
        for c in self.members:
            c._engine()
        decs = [c._dec for c in self.members]
        if self._ens is None or any(a is not b for a, b in zip(self._ens.members, decs)):
            self._ens = EnsembleDecodeEngine(decs, self.weights, self.mode)
        return self._ens

    def forward(self, image_features: torch.Tensor, obj_atts=None, image_attributes=None, caption_tokens=None, sentiment=None,
                fsm: torch.Tensor = None, num_constraints: torch.Tensor = None, constraints=None, constraint2states=None):
        if self.training:
            raise RuntimeError("CaptionerEnsemble is an eval-time decoder: train its members one by one")
        lead = self.members[0]
        ens = self.engine()
        dev = ens.device
        B, num_boxes, _ = image_features.size()
        L = lead._max_caption_length
        k = lead._beam_search.beam_size
        per = lead._beam_search.per_node_beam_size or k
        with torch.no_grad():
            obj_means = lead._obj_means(obj_atts, B, num_boxes)
            fsm_d = None
            if lead._use_cbs and fsm is not None:
                if not lead.cbs_simple:
                    raise ValueError("CaptionerEnsemble with a constraint machine needs CBS_SIMPLE")
                fsm_d = fsm.to(dev).to(torch.uint8).contiguous()
            S = 1 if fsm_d is None else fsm_d.size(1)
            eps0 = lead._draw_eps(1, B, dev)[0]
            eps = lead._draw_eps(L - 1, B * S * k, dev) if L > 1 else None
            sent = sentiment.reshape(B).to(dev) if sentiment is not None else None
            ctx = ens.prepare(image_features.to(dev, torch.float32), obj_means)
            beams, lps = ens.search(ctx, sent, 1, k, per, L, lead._boundary_index, eps0, eps, fsm=fsm_d)
            if fsm_d is not None and S > 1:
                best, _ = select_best_beam_simple_batched(beams, lps, num_constraints, lead._min_constraints_to_satisfy)
            else:
                best = beams[:, 0, 0, :]
        return {"predictions": best}
