"""UpDownCaptioner (Style-SeqCVAE): MI355X-native drop-in for
var_updown/var_updown/models/updown_captioner.py:20-466 of the reference - same constructor / from_config /
forward / _decode_step signatures, attribute names (``_updown_cell._language_lstm_cell_decoder`` is part of the
API: var_updown/scripts/train.py:157,160) and state_dict keys.

Underneath, parameters live in one flat HBM buffer (views with 16-B aligned rows), the teacher-forced training
forward and its BPTT are one fused C-ABI call each (ssc_train_fwd / ssc_train_bwd, exposed to autograd through a
single torch.autograd.Function), and eval decoding runs ssc_decode_step + on-device constrained beam search.
There is no CPU fallback: calling the model on a CPU tensor raises.
"""
import functools
from typing import Dict, Optional

import numpy as np
import torch
from torch import nn

from ssc_runtime import lib as _lib
from ssc_runtime import sampling
from ssc_runtime.cellops import cell_train_step
from ssc_runtime.decode import DecodeEngine
from ssc_runtime.decoding import select_best_beam_with_constraints
from ssc_runtime.engine import FIELD_OF, ModelDims, TrainEngine, check_free_bits, check_label_smoothing, check_sched_sampling
from ssc_runtime.engine import check_distill, check_distill_sampling, check_unlikelihood, check_unlikelihood_distill

from ..modules import ConstrainedBeamSearch, UpDownCell


class _SeqCVAETrainFn(torch.autograd.Function):
    """loss_b, kld_b = f(params; feats, caps, sentiment, eps) with the hand-derived BPTT as backward."""

    @staticmethod
    def forward(ctx, eng, names, feats, caps, sentiment, eps, obj_means, label_smoothing, free_bits, free_bits_mode, ss, distill, unlikelihood,
                *params):
        loss, kld = eng.forward(feats, caps, sentiment, eps, obj_means, label_smoothing, free_bits, free_bits_mode, *ss, distill=distill,
                                unlikelihood=unlikelihood[0], unlikelihood_clamp=unlikelihood[1])
        ctx.eng, ctx.names = eng, names
        ctx.version = eng.fwd_version
        return loss, kld

    @staticmethod
    def backward(ctx, gl, gk):
        eng = ctx.eng
        if eng.fwd_version != ctx.version:
            raise RuntimeError("UpDownCaptioner: backward() after a newer forward(); the activation workspace holds "
                               "only the latest forward")
        need = ctx.needs_input_grad[13:]
        skip = [n for n, k in zip(ctx.names, need) if not k]
        eng.backward(gl, gk, skip=skip)
        if eng.dp_autograd:   # data parallel on the autograd path: ONE sum all-reduce of the flat gradient buffer, then the mean
            world = eng.allreduce_grads()
            if world > 1:
                eng.grads.flat.mul_(1.0 / world)
        frozen = set(eng.frozen_names)
        grads = tuple(eng.grads.views[n].clone() if (k and n not in frozen) else None for n, k in zip(ctx.names, need))
        return (None,) * 13 + grads


class UpDownCaptioner(nn.Module):
    def __init__(self, vocabulary, image_feature_size, embedding_size, hidden_size, attention_projection_size,
                 max_caption_length=20, beam_size=1, use_cbs=False, min_constraints_to_satisfy=2, z_space=150,
                 prior_std=None, simple_vae=False, latent_embedding=None, latent_embedding_multip=1,
                 sentiment_vae=False, senti_prior_multip=1, cbs_simple=False, device=None, mean_choice=None, sampler=None,
                 sampled_beam=False, diverse_beam=None, label_smoothing=0.0, decode_rules=None, free_bits=0.0,
                 free_bits_mode="dim", unlikelihood=0.0, unlikelihood_clamp=1e-5):
        """Same parameters as the reference (updown_captioner.py:21-41) plus `mean_choice` (SENTIMENT_VAE = 2 only): the attribute
        word -> z_space-vector table the reference builds from files at hard-coded paths (`/path/to/sentiglove10.pkl`,
        `/path/to/wordform_swd_scores.json`, updown_captioner.py:79-93) - and cannot finish building as shipped (`self.senti_glove_5`
        is never defined, :89).  Here the caller supplies it: a dict of vectors, or use mean_choice_from_sentiglove /
        mean_choice_from_senti_wordnet, which restate :80-86.
        `sampler` (optional): a word sampler of ssc_runtime.sampling (MODEL.DECODE_SAMPLER) - the eval forward then draws every word
        on the device (ssc_decode_sample) instead of running beam search; needs beam_size 1 and no CBS decode.  Or
        sampling.GumbelSampler (MODEL.STOCHASTIC_BEAM_SEARCH): the eval forward runs the stochastic beam search at beam_size with
        per_node_beam_size beam_size // 2 (beam_size when that is 0) in one library call and returns beam 0; no CBS decode.
        `sampled_beam` (MODEL.SAMPLED_BEAM_SEARCH) with a word sampler: the eval forward runs the sampled-node beam search
        (ssc_decode_sampled_beam: the reference's BeamSearch with that sampler) at beam_size, per_node_beam_size as above, and
        returns beam 0.
        `diverse_beam` (MODEL.DIVERSE_BEAM_SEARCH): a sampling.DiverseBeam(groups, strength) - the eval forward runs the diverse beam
        search (ssc_decode_diverse_beam) at beam_size in one library call and returns the caption with the highest log-prob; no
        sampler, no CBS decode, beam_size a multiple of the groups.
        `decode_rules` (MODEL.NO_REPEAT_NGRAM / MIN_CAPTION_LENGTH / LENGTH_PENALTY_ALPHA / SUPPRESS_UNKNOWN): a
        sampling.DecodeRules - the eval forward runs the beam search under them (ssc_decode_rules_beam) at beam_size in one library
        call and returns beam 0, the best caption under the length penalty; no sampler, no diverse_beam, no CBS decode.  None, or
        rules with every control off: the eval forward is what it is without them.
        `label_smoothing` (OPTIM.LABEL_SMOOTHING), in [0, 1): the cross-entropy of the training forward spreads this much of every
        target's mass over all V classes (torch.nn.functional.cross_entropy's label_smoothing, ssc_ce_fwd_smooth); 0 = the
        reference's plain masked NLL.  scst_step and score_captions never smooth.
        `free_bits` (OPTIM.FREE_BITS, nats) / `free_bits_mode` (OPTIM.FREE_BITS_MODE: "element" | "step" | "dim"): a floor under the KL
        of the training forward (ssc_latent_fwd_fb) - out["kld"] is then the floored KL and a term at or below its floor has no
        gradient; the KL without the floor is `_engine().kld_raw()`.  "dim" floors the mean over the rows of the call of every latent
        dimension.  0 = off.  Any annealing weight is the caller's multiplier on out["kld"], as KLD_WEIGHT is.  scst_step,
        score_captions and posterior_score_captions never floor.
        `unlikelihood` (OPTIM.UNLIKELIHOOD_ALPHA, a finite number >= 0) / `unlikelihood_clamp` (in (0, 1)): token-level unlikelihood
        training of the training forward (Welleck et al. 2020; ssc_ce_fwd_unlike) - every word adds `unlikelihood` times
        - sum log max(1 - p[c], unlikelihood_clamp) over the words c its caption has already used (its own target left out) to its
        loss; out["ul"] is that term alone, unweighted.  0 = off.  Not together with distill().  scst_step, score_captions and
        posterior_score_captions never apply it."""
        super().__init__()
        self.unlikelihood, self.unlikelihood_clamp = check_unlikelihood(unlikelihood, unlikelihood_clamp)
        self.label_smoothing = check_label_smoothing(label_smoothing)
        self.free_bits = check_free_bits(free_bits, free_bits_mode)[0]
        self.free_bits_mode = free_bits_mode
        self._sched_sampling = (0.0, None, 0)   # scheduled_sampling(): off
        self._distill = None                    # distill(): off
        if diverse_beam is not None:
            if sampler is not None:
                raise ValueError("MODEL.DIVERSE_BEAM_SEARCH needs MODEL.DECODE_SAMPLER 'beam' without MODEL.STOCHASTIC_BEAM_SEARCH")
            if beam_size % diverse_beam.groups != 0:
                raise ValueError(f"MODEL.BEAM_SIZE ({beam_size}) must be a multiple of MODEL.DIVERSE_BEAM_GROUPS ({diverse_beam.groups})")
        self.diverse_beam = diverse_beam
        if decode_rules is not None and not decode_rules.active:
            decode_rules = None
        if decode_rules is not None:
            if sampler is not None or sampled_beam:
                raise ValueError("MODEL.NO_REPEAT_NGRAM / MIN_CAPTION_LENGTH / LENGTH_PENALTY_ALPHA / SUPPRESS_UNKNOWN need "
                                 "MODEL.DECODE_SAMPLER 'beam' without MODEL.STOCHASTIC_BEAM_SEARCH")
            if diverse_beam is not None:
                raise ValueError("MODEL.NO_REPEAT_NGRAM / MIN_CAPTION_LENGTH / LENGTH_PENALTY_ALPHA / SUPPRESS_UNKNOWN and "
                                 "MODEL.DIVERSE_BEAM_SEARCH exclude each other")
            decode_rules.check(vocabulary.get_vocab_size(), vocabulary.get_token_index("@@BOUNDARY@@"), max_caption_length)
        self.decode_rules = decode_rules
        if sampled_beam and (sampler is None or sampler.beam_search):
            raise ValueError("MODEL.SAMPLED_BEAM_SEARCH needs MODEL.DECODE_SAMPLER 'multinomial', 'top-k' or 'top-p'")
        if sampler is not None and not sampler.beam_search and not sampled_beam and beam_size != 1:
            raise ValueError(f"MODEL.BEAM_SIZE must be 1 with MODEL.DECODE_SAMPLER {sampler.name!r} (word sampling draws one word per "
                             f"row), got {beam_size}")
        self.sampler = sampler
        self.sampled_beam = bool(sampled_beam)
        self._vocabulary = vocabulary
        self.image_feature_size = image_feature_size
        self.embedding_size = embedding_size
        self.hidden_size = hidden_size
        self.attention_projection_size = attention_projection_size
        self._max_caption_length = max_caption_length
        self._use_cbs = use_cbs
        self._min_constraints_to_satisfy = min_constraints_to_satisfy
        self.z_space = z_space
        _vocab_size = vocabulary.get_vocab_size()
        self._pad_index = vocabulary.get_token_index("@@UNKNOWN@@")
        self._boundary_index = vocabulary.get_token_index("@@BOUNDARY@@")
        self.prior_std = 1.0 if prior_std is None else prior_std
        self.sentiment_vae = int(sentiment_vae)
        self.senti_prior_multip = senti_prior_multip
        self.simple_vae = simple_vae
        self.latent_embedding = latent_embedding
        self.latent_embedding_multip = latent_embedding_multip
        self.mean_choice = None
        if self.sentiment_vae == 2:
            # attention-grounded style prior (updown_captioner.py:76-93, updown_cell.py:160-163,185-188,219-222)
            if latent_embedding not in ("glove", "senti_word_net"):
                raise NotImplementedError()          # (updown_captioner.py:92-93)
            if mean_choice is None:
                mean_choice = self._load_mean_choice()
            self.mean_choice = {k: np.asarray(v, dtype=np.float64).reshape(-1) for k, v in mean_choice.items()}
            bad = [k for k, v in self.mean_choice.items() if v.shape[0] != z_space]
            if bad:
                raise ValueError(f"mean_choice vectors must have z_space = {z_space} entries (e.g. {bad[0]!r} has {self.mean_choice[bad[0]].shape[0]})")
            if not simple_vae and latent_embedding == "glove" and z_space != 150:
                raise ValueError("SENTIMENT_VAE = 2 with LATENT_EMBEDDING 'glove' conditions the language LSTMs on 150 columns "
                                 "(updown_cell.py:63-70): Z_SPACE must be 150")
        self._tied = self.embedding_size in (300, 600)
        if self._tied:  # frozen GloVe(+deps) table, output layer tied to it (updown_captioner.py:75-100,112-119)
            glove_vectors = self._initialize_glove()
            self._embedding_layer = nn.Embedding.from_pretrained(glove_vectors, freeze=True, padding_idx=self._pad_index)
        else:
            self._embedding_layer = nn.Embedding(_vocab_size, embedding_size, padding_idx=self._pad_index)
            assert not use_cbs, "CBS is not supported without Frozen GloVe embeddings (300d)"
        self._updown_cell = UpDownCell(image_feature_size, embedding_size, hidden_size, attention_projection_size, z_space,
                                       self.sentiment_vae, simple_vae, device, latent_embedding)
        self._updown_cell._host = _HostRef(self)
        if self._tied:
            self._output_projection = nn.Sequential(nn.Linear(hidden_size, self.embedding_size), nn.Tanh())
            self._output_layer = nn.Linear(self.embedding_size, _vocab_size, bias=False)
            self._output_layer.weight = self._embedding_layer.weight
        else:
            self._output_projection = nn.Identity()
            self._output_layer = nn.Linear(hidden_size, _vocab_size)
        self._log_softmax = nn.LogSoftmax(dim=1)
        # The reference's non-CBS branch (allennlp BeamSearch) cannot unpack the 5-tuple step;
        # here non-CBS decoding is CBS over the trivial one-state FSM.
        self._beam_search = ConstrainedBeamSearch(self._boundary_index, max_steps=max_caption_length,
                                                  beam_size=beam_size, per_node_beam_size=beam_size // 2)
        self.device = device
        self.cbs_simple = cbs_simple
        # noise source: "cpu" reproduces the reference's stream (one CPU torch.randn((rows, Z)) per step,
        # updown_cell.py:206) without its per-step host sync; "device" draws on the GPU (not bit-comparable).
        self.eps_source = "cpu"
        self._eps_override = None      # test hook: explicit (T,B,Z) / list of (G,Z)
        self._eng: Optional[TrainEngine] = None
        self._dec: Optional[DecodeEngine] = None
        self._scst = None   # (key, SelfCritical, its references) of the last scst_step
        self._ctx_cache = None
        self.n_z_samples = 1           # latent samples per caption of score_captions (from_config: MODEL.N_Z_SAMPLES)
        self._decode_attention = None  # decode_attention(): "summary" / "full" attention traces in the eval forward's output
        self._decode_guide = None      # decode_guide(): a LatentGuide the NEXT eval forwards draw their latents around
        self._logit_rules = None       # logit_rules(): sampling.LogitRules the NEXT eval forwards of a word sampler draw under
        self._truncation = None        # truncation(): sampling.Truncation the NEXT eval forwards of a word sampler cut their steps with
        self._mirostat = None          # mirostat(): sampling.Mirostat the NEXT eval forwards of a word sampler hold their surprise with
        self._arithmetic = None        # arithmetic(): sampling.Arithmetic the NEXT eval forwards of a word sampler draw their words along
        self._contrast = None          # contrast():contrast.Contrast the NEXT eval forwards of a word sampler decode against an amateur with
        self._decode_prefix = None     # decode_prefix(): a DecodePrefix every caption of the NEXT eval forwards starts with

    # ------------------------------------------------------------------------------------------------------
    @classmethod
    def from_config(cls, config, **kwargs):
        """Instantiate from a Config (updown_captioner.py:141-166); extra kwargs such as cbs_simple are ignored as in
        the reference.  mean_choice=... (SENTIMENT_VAE = 2) is handed to the constructor.  MODEL.SAMPLED_BEAM_SEARCH is read only
        with a sampler=... (the decode's); a model built without one (scripts/train.py) ignores it, as it ignores the other
        decode keys; diverse_beam=... (sampling.diverse_beam_from_config) likewise comes from the caller.  The decode rules
        (sampling.decode_rules_from_config) are read here; with their keys at the defaults there are none.  The logit rules of the
        word samplers (MODEL.SAMPLER_NO_REPEAT_NGRAM and its kin, sampling.logit_rules_from_config) are read only with a word
        sampler=... that is not run as a sampled-node beam search: a model built without one never reads them."""
        _C = config
        vocabulary = kwargs.pop("vocabulary")
        model = cls(vocabulary=vocabulary, image_feature_size=_C.MODEL.IMAGE_FEATURE_SIZE,
                    embedding_size=_C.MODEL.EMBEDDING_SIZE, hidden_size=_C.MODEL.HIDDEN_SIZE,
                    attention_projection_size=_C.MODEL.ATTENTION_PROJECTION_SIZE, beam_size=_C.MODEL.BEAM_SIZE,
                    max_caption_length=_C.DATA.MAX_CAPTION_LENGTH, use_cbs=_C.MODEL.USE_CBS,
                    min_constraints_to_satisfy=_C.MODEL.MIN_CONSTRAINTS_TO_SATISFY, z_space=_C.MODEL.Z_SPACE,
                    prior_std=_C.MODEL.PRIOR_STD, simple_vae=_C.MODEL.SIMPLE_VAE, latent_embedding=_C.MODEL.LATENT_EMBEDDING,
                    sentiment_vae=_C.MODEL.SENTIMENT_VAE, senti_prior_multip=_C.MODEL.SENTI_PRIOR_MULTIP,
                    latent_embedding_multip=_C.MODEL.LATENT_EMBEDDING_MULTIP, cbs_simple=_C.MODEL.CBS_SIMPLE,
                    device=kwargs["device"], mean_choice=kwargs.get("mean_choice"), sampler=kwargs.get("sampler"),
                    sampled_beam=kwargs.get("sampler") is not None and sampling.sampled_beam_from_config(_C.MODEL),
                    diverse_beam=kwargs.get("diverse_beam"), label_smoothing=_C.OPTIM.LABEL_SMOOTHING,
                    decode_rules=sampling.decode_rules_from_config(_C.MODEL, vocabulary), free_bits=_C.OPTIM.FREE_BITS,
                    free_bits_mode=_C.OPTIM.FREE_BITS_MODE, unlikelihood=_C.OPTIM.UNLIKELIHOOD_ALPHA)
        model.n_z_samples = max(1, int(_C.MODEL.N_Z_SAMPLES))   # default latent sample count of score_captions
        model.decode_attention(_C.MODEL.DECODE_ATTENTION)
        if model.sampler is not None and not model.sampler.beam_search and not model.sampled_beam:
            model.logit_rules(sampling.logit_rules_from_config(_C.MODEL, vocabulary))
            model.truncation(sampling.truncation_from_config(_C.MODEL))
            model.mirostat(sampling.mirostat_from_config(_C.MODEL))
            model.arithmetic(sampling.arithmetic_from_config(_C.MODEL))
            from ssc_runtime.contrast import contrast_from_config
            model.contrast(contrast_from_config(_C.MODEL))
        if str(_C.MODEL.DECODE_PREFIX).strip():
            from ssc_runtime.prefix import DecodePrefix
            model.decode_prefix(DecodePrefix.from_words(vocabulary, str(_C.MODEL.DECODE_PREFIX)))
        return model

    def _initialize_glove(self):
        """GloVe 42B (+ dependency embeddings for 600-d) rows for the vocabulary (updown_captioner.py:168-226).
        Needs torchtext and its vector cache, like the reference; override in a subclass to supply a table."""
        try:
            from torchtext.vocab import GloVe, Vectors
        except ImportError as e:  # no silent substitute for pretrained vectors
            raise ImportError("EMBEDDING_SIZE in {300,600} initialises frozen GloVe embeddings through torchtext "
                              "(not installed); subclass and override _initialize_glove() to provide the table") from e
        V = self._vocabulary.get_vocab_size()
        glove = GloVe(name="42B", dim=300, cache="/path/to/.vector_cache")
        deps = Vectors(name="deps.words", cache="/path/to/.vector_cache") if self.embedding_size == 600 else None
        table = torch.zeros(V, self.embedding_size)
        for word, i in self._vocabulary.get_token_to_index_vocabulary().items():
            parts = []
            for src in ([glove] if deps is None else [glove, deps]):
                parts.append(src.vectors[src.stoi[word]] if word in src.stoi else 2 * torch.randn(300) - 1)
            table[i] = torch.cat(parts, 0)
        return table

    # ---- SENTIMENT_VAE = 2: attribute table and per-object means --------------------------------------------------
    def _load_mean_choice(self):
        """Hook for subclasses: the attribute table when none was passed to the constructor (the reference reads pickles at
        hard-coded paths here, updown_captioner.py:79-86)."""
        raise ValueError("SENTIMENT_VAE = 2 needs the attribute table: pass mean_choice={word: vector of z_space floats} "
                         "(see mean_choice_from_sentiglove / mean_choice_from_senti_wordnet) or override _load_mean_choice()")

    @staticmethod
    def mean_choice_from_sentiglove(senti_glove_10, z_space):
        """updown_captioner.py:79-81: each 10-d sentiment-GloVe vector repeated z_space / 10 times per entry (np.repeat)."""
        return {k: np.repeat(np.asarray(v), int(z_space / 10)) for k, v in senti_glove_10.items()}

    @staticmethod
    def mean_choice_from_senti_wordnet(scores, z_space):
        """updown_captioner.py:83-86: (positive - negative) SentiWordNet score of a word form, z_space times
        (data/wordform_swd_scores.json: word -> [pos, obj, neg])."""
        return {k: np.repeat(v[0] - v[2], z_space) for k, v in scores.items()}

    def translate_obj_atts2obj_means(self, obj_atts):
        """Per image a list of objects `(name, [attribute strings])` -> (B, max objects, z_space) float32: the mean of the table
        vectors of an object's attributes (first word of each attribute string; unknown words are skipped; no known attribute ->
        zeros), zero-padded over objects, times LATENT_EMBEDDING_MULTIP (updown_captioner.py:509-532)."""
        Z = self.z_space
        per_image = []
        for im in obj_atts:
            means = np.zeros((len(im), Z))
            for i_o, obj in enumerate(im):
                vecs = []
                for att in obj[1]:
                    try:                                   # (the reference skips whatever it cannot look up, :517-520)
                        vecs.append(self.mean_choice[att.split(" ")[0]])
                    except Exception:                      # noqa: BLE001
                        pass
                if vecs:
                    means[i_o] = np.mean(vecs, axis=0)
            per_image.append(means)
        out = np.zeros((len(per_image), max(len(x) for x in per_image), Z))
        for i_i, m in enumerate(per_image):
            out[i_i, : len(m)] = m
        dev = self._embedding_layer.weight.device
        return torch.Tensor(out * self.latent_embedding_multip).to(dev)

    def _obj_means(self, obj_atts, batch_size, num_boxes):
        """The per-region attribute means the cell pools (updown_cell.py:160-163) from what forward() was given: the reference's
        nested lists (translated as above), or - an extension - a (B, R, z_space) tensor of means as is."""
        if self.sentiment_vae != 2 or self.simple_vae:
            return None
        if obj_atts is None:
            raise ValueError("SENTIMENT_VAE = 2: forward() needs obj_atts (the reference multiplies the attention weights with it, "
                             "updown_cell.py:160-163)")
        means = obj_atts if torch.is_tensor(obj_atts) else self.translate_obj_atts2obj_means(obj_atts)
        if tuple(means.shape) != (batch_size, num_boxes, self.z_space):
            raise ValueError(f"obj_atts means {tuple(means.shape)} do not line up with the image features: expected "
                             f"({batch_size}, {num_boxes}, {self.z_space}) - one entry per region, as the attention weights have")
        return means.to(self._embedding_layer.weight.device, torch.float32).contiguous()

    # ---- engine plumbing -------------------------------------------------------------------------------------
    def _dims(self) -> ModelDims:
        sv1 = self.sentiment_vae == 1 and not self.simple_vae
        sv2 = self.sentiment_vae == 2 and not self.simple_vae
        return ModelDims(V=self._vocabulary.get_vocab_size(), E=self.embedding_size, H=self.hidden_size,
                         A=self.attention_projection_size, F=self.image_feature_size, Z=self.z_space,
                         S=self._updown_cell.senti_cols, tied=self._tied, kld_mode=0 if self.sentiment_vae == 0 else (2 if sv2 else 1),
                         pm_scale=float(self.senti_prior_multip) if sv1 else 0.0, prior_var=float(self.prior_std) ** 2,
                         pad=self._pad_index, boundary=self._boundary_index)

    def _named(self) -> Dict[str, nn.Parameter]:
        out = {}
        for n, p in self.named_parameters():  # named_parameters() de-duplicates the tied output weight
            if n in FIELD_OF:
                out[n] = p
        return out

    def _engine(self) -> TrainEngine:
        dev = self._embedding_layer.weight.device
        if dev.type != "cuda":
            raise RuntimeError("UpDownCaptioner (MI355X build) runs on a ROCm GPU only: move the model with "
                               ".to('cuda'); there is no CPU fallback")
        if self._eng is None or self._eng.device != dev:
            self._eng = TrainEngine(self._dims(), dev)
            self._dec = DecodeEngine(self._eng.dims, self._eng.params.c_struct, dev)
        self._eng.adopt(self._named())
        return self._eng

    def _draw_eps(self, steps: int, rows: int, device) -> torch.Tensor:
        if self._eps_override is not None:
            e = self._eps_override
            assert tuple(e.shape) == (steps, rows, self.z_space), (e.shape, (steps, rows, self.z_space))
            return e.to(device, torch.float32).contiguous()
        if self.eps_source == "device":
            return torch.randn(steps, rows, self.z_space, device=device)
        host = torch.empty(steps, rows, self.z_space, pin_memory=True)
        for t in range(steps):  # one (rows, Z) draw per step: the reference's CPU stream (updown_cell.py:206)
            host[t] = torch.randn(rows, self.z_space)
        return host.to(device, non_blocking=True)

    # ---- forward ---------------------------------------------------------------------------------------------
    def forward(self, image_features: torch.Tensor, obj_atts=None, image_attributes=None, caption_tokens=None,
                sentiment=None, fsm: torch.Tensor = None, num_constraints: torch.Tensor = None, constraints=None,
                constraint2states=None):
        batch_size, num_boxes, _ = image_features.size()
        eng = self._engine()
        dev = eng.device
        if self.training and caption_tokens is not None:
            # training branch (updown_captioner.py:263-323): boundary tokens, T-step loop, KLD, masked NLL - all fused
            L = caption_tokens.size(1)
            eps = self._draw_eps(L + 1, batch_size, dev)
            names = list(self._named().keys())
            params = [self._named()[n] for n in names]
            sent = sentiment if sentiment is not None else None
            obj_means = self._obj_means(obj_atts, batch_size, num_boxes)
            feats, caps = image_features.contiguous().float(), caption_tokens.contiguous().long()
            kd = None
            if self._distill is not None:   # the teachers' forwards on this minibatch and this noise, ahead of the student's
                teacher, alpha, temperature = self._distill
                check_distill_sampling(alpha, self._sched_sampling[0])
                check_unlikelihood_distill(self.unlikelihood, alpha)
                kd = teacher.distill(feats, caps, sent, eps, alpha, temperature, obj_means)
            loss, kld = _SeqCVAETrainFn.apply(eng, names, feats, caps, sent, eps, obj_means, self.label_smoothing,
                                              self.free_bits, self.free_bits_mode, self._sched_sampling, kd,
                                              (self.unlikelihood, self.unlikelihood_clamp), *params)
            if kd is not None:
                return {"loss": loss, "kld": kld, "kd": eng.kd().clone()}
            if self.unlikelihood > 0:
                return {"loss": loss, "kld": kld, "ul": eng.ul().clone()}
            return {"loss": loss, "kld": kld}
        # eval branch (updown_captioner.py:324-366)
        start_predictions = torch.full((batch_size,), self._boundary_index, dtype=torch.long, device=dev)
        obj_means = self._obj_means(obj_atts, batch_size, num_boxes)   # (updown_captioner.py:246-247)
        step = functools.partial(self._decode_step, image_features, obj_means, sentiment=sentiment)
        if self._decode_prefix is not None:
            with torch.no_grad():
                return self._prefixed_decode(image_features, obj_means, sentiment, fsm if self._use_cbs else None, num_constraints)
        if self._decode_guide is not None:
            from ssc_runtime.guide import guide_unsupported
            if self.sampler is not None and (self.sampler.beam_search or self.sampled_beam):
                guide_unsupported("the stochastic and the sampled-node beam search (MODEL.DECODE_SAMPLER with a beam)")
            if self.diverse_beam is not None:
                guide_unsupported("the diverse beam search (MODEL.DIVERSE_BEAM_SEARCH)")
            if self.decode_rules is not None:
                guide_unsupported("the beam search under decode rules")
        if self.sampler is not None:
            if self._use_cbs and fsm is not None:
                raise ValueError(f"MODEL.USE_CBS with a constraint machine cannot be combined with MODEL.DECODE_SAMPLER "
                                 f"{self.sampler.name!r}: constrained sampling is not supported")
            with torch.no_grad():
                return self._sample_decode(image_features, obj_means, sentiment)
        if self.diverse_beam is not None:
            if self._use_cbs and fsm is not None:
                raise ValueError("MODEL.USE_CBS with a constraint machine cannot be combined with MODEL.DIVERSE_BEAM_SEARCH")
            with torch.no_grad():
                return self._diverse_beam_decode(image_features, obj_means, sentiment)
        if self.decode_rules is not None:
            if self._use_cbs and fsm is not None:
                raise ValueError("MODEL.USE_CBS with a constraint machine cannot be combined with the decode rules "
                                 "(MODEL.NO_REPEAT_NGRAM / MIN_CAPTION_LENGTH / LENGTH_PENALTY_ALPHA / SUPPRESS_UNKNOWN)")
            with torch.no_grad():
                return self._rules_beam_decode(image_features, obj_means, sentiment)
        if self._decode_attention is not None or self._decode_guide is not None:
            with torch.no_grad():
                return self._traced_beam_decode(image_features, obj_means, sentiment, fsm if self._use_cbs else None,
                                                num_constraints)
        with torch.no_grad():
            if self._use_cbs and fsm is not None:
                fsm_d = fsm.to(dev).to(torch.uint8)
                beams, lps = self._beam_search.search(start_predictions, None, step, fsm_d)
                best, _valid = select_best_beam_with_constraints(beams, lps, num_constraints, constraints, constraint2states,
                                                                 self._min_constraints_to_satisfy, self.cbs_simple)
            else:
                V = self._vocabulary.get_vocab_size()
                fsm_d = torch.ones(batch_size, 1, 1, V, dtype=torch.uint8, device=dev)
                beams, lps = self._beam_search.search(start_predictions, None, step, fsm_d)
                best = beams[:, 0, 0, :]
        return {"predictions": best}

    def scheduled_sampling(self, prob, seed=0, sampler=None):
        """Scheduled sampling of the NEXT training forwards (the autograd path; include/ssc.h: ssc_sched_sampling): with probability
        `prob` an eligible position is fed the word the model draws from its own logits of the previous step, the draws and the
        decisions seeded by `seed` (ssc_runtime.schedule.ss_seed for a resumable run: call this once per iteration).  sampler: None
        (multinomial, temperature 1), a word sampler of ssc_runtime.sampling, or (kind, top_k, top_p, temperature).  prob 0 (the
        default state) = off.  The eval forward, scst_step, score_captions and posterior_score_captions never sample."""
        check_sched_sampling(prob, sampler, seed)
        self._sched_sampling = (float(prob), sampler, int(seed))

    def distill(self, teacher, alpha, temperature=1.0):
        """Knowledge distillation of the NEXT training forwards (the autograd path; include/ssc.h: ssc_distill): `teacher` (an
        ssc_runtime.distill.DistillTeacher of this captioner's architecture and vocabulary) runs its members' forwards on every
        minibatch and the same noise, and loss becomes (1 - alpha) * the (smoothed) hard loss + alpha * temperature^2 KL(teacher ||
        student) per word; the output dict gains "kd", the KL term alone.  teacher None or alpha 0 (the default state) = off.  Not
        together with scheduled_sampling (ValueError at the forward).  The eval forward, scst_step, score_captions and
        posterior_score_captions never distil."""
        if teacher is None:
            self._distill = None
            return
        alpha, temperature = check_distill(alpha, temperature)
        teacher.check_student(self._dims())
        self._distill = (teacher, alpha, temperature) if alpha > 0.0 else None

    def decode_attention(self, mode):
        """Attention traces of the NEXT eval forwards (include/ssc.h: ssc_attn_record): "summary" - the output dict gains, per
        image and word of the returned caption, attention_top_region (B, steps) int32 (the region the word attended most; -1 for
        the words after the caption's END, which read nothing), attention_top_weight (the weight there) and attention_entropy
        (nats) -, "full" - additionally attention (B, steps, R), the whole map -, or None / "none" (the default state): off, the
        dict is what it is without.  Every decoder of the eval forward; the predictions are those of the same forward without it
        given the same noise.  With it set the plain and the constrained beam search run as one library call
        (DecodeEngine.search) with the noise of all steps drawn up front, as the sampled decodes draw theirs; constraints need
        CBS_SIMPLE."""
        if mode in (None, "none"):
            self._decode_attention = None
        elif mode in ("summary", "full"):
            self._decode_attention = mode
        else:
            raise ValueError(f'decode_attention: mode must be None, "none", "summary" or "full", got {mode!r}')

    def decode_guide(self, guide):
        """A latent guide for the NEXT eval forwards (ssc_runtime.guide.LatentGuide over the B images of the forward, one entry per
        image; include/ssc.h: ssc_latent_guide): the latent of step t of image b is drawn around guide.mean[t, b] instead of the
        prior - reconstruction, style transfer from an exemplar caption, interpolation.  None (the default state): off.  The plain
        and the constrained beam search then run as one library call (DecodeEngine.search) with the noise of all steps drawn up
        front, as under decode_attention (constraints need CBS_SIMPLE); word sampling takes the guide as well; every other decoder
        raises NotImplementedError naming the feature.  The guide must match the batch of every forward it is set for."""
        if guide is not None:
            from ssc_runtime.guide import LatentGuide
            if not isinstance(guide, LatentGuide):
                raise ValueError(f"decode_guide: a ssc_runtime.guide.LatentGuide or None, got {type(guide).__name__}")
            if guide.Z != self.z_space:
                raise ValueError(f"decode_guide: the guide has Z = {guide.Z}, the model {self.z_space}")
        self._decode_guide = guide

    def decode_prefix(self, prefix):
        """A prompt for the NEXT eval forwards (ssc_runtime.prefix.DecodePrefix with one row - the same prompt for every image - or
        one row per image of the forward; include/ssc.h: ssc_start_state, ssc_decode_prime): every returned caption starts with its
        prompt's words, the configured decoder - beam search, plain or constrained (CBS_SIMPLE), a word sampler, the stochastic,
        sampled-node and diverse beam searches, the beam search under decode rules - continues from there, and "predictions" is
        (B, Lp + steps).  None (the default state): off, the forward is what it is without.  The machine of a constrained search
        starts in its start state after the prompt, rules and logit rules see the continuation only, MAX_CAPTION_LENGTH bounds the
        continuation.  The decode runs as ssc_runtime.inference.diverse_decode(prefix=...) with one latent sample per image and the
        noise of a generator seeded by one draw of the global one.  NotImplementedError at the forward together with
        decode_attention or decode_guide."""
        if prefix is not None:
            from ssc_runtime.prefix import DecodePrefix
            if not isinstance(prefix, DecodePrefix):
                raise ValueError(f"decode_prefix: a ssc_runtime.prefix.DecodePrefix or None, got {type(prefix).__name__}")
            V = self._vocabulary.get_vocab_size()
            ids = prefix.ids
            if bool(((ids >= V) | (ids == self._boundary_index)).any()):
                raise ValueError(f"decode_prefix: the prefix holds @@BOUNDARY@@ or an id outside the vocabulary of {V}")
        self._decode_prefix = prefix

    def _prefixed_decode(self, image_features, obj_means, sentiment, fsm, num_constraints):
        """Eval forward with decode_prefix set: whichever decoder is configured, through inference.diverse_decode(prefix=...)."""
        from ssc_runtime.inference import diverse_decode
        from ssc_runtime.prefix import DecodePrefix, prefix_unsupported
        if self._decode_attention is not None:
            prefix_unsupported("attention traces (decode_attention): the trace would not cover the prefix words")
        if self._decode_guide is not None:
            prefix_unsupported("latent guides (decode_guide)")
        B = image_features.size(0)
        dev = self._eng.device
        ids = self._decode_prefix.ids
        if ids.size(0) == 1 and B > 1:
            ids = ids.expand(B, ids.size(1))
        if ids.size(0) != B:
            raise ValueError(f"decode_prefix: the prefix has {ids.size(0)} rows, the forward {B} images")
        fsm_d = None
        if fsm is not None:
            if not self.cbs_simple:
                raise ValueError("decode_prefix with a constraint machine needs CBS_SIMPLE")
            fsm_d = fsm.to(dev).to(torch.uint8).contiguous()
        words = self.sampler is not None and not self.sampler.beam_search and not self.sampled_beam
        k = 1 if words else self._beam_search.beam_size
        per = None if (words or self.diverse_beam is not None or self.sampler is not None or self.decode_rules is not None) \
            else (self._beam_search.per_node_beam_size or None)
        out = diverse_decode(self._dec, image_features.to(dev).float().contiguous(),
                             sentiment.reshape(B).to(dev) if sentiment is not None else None, 1, k, self._max_caption_length,
                             self._boundary_index, fsm=fsm_d, num_constraints=num_constraints,
                             min_constraints_to_satisfy=self._min_constraints_to_satisfy, per_node=per, obj_means=obj_means,
                             sampler=self.sampler, sampled_beam=bool(self.sampled_beam and self.sampler is not None),
                             diverse_beam=self.diverse_beam, rules=self.decode_rules,
                             logit_rules=self._logit_rules if words else None, prefix=DecodePrefix(ids),
                             **({"truncation": self._truncation} if words and self._truncation is not None else {}),
                             **({"mirostat": self._mirostat} if words and self._mirostat is not None else {}),
                             **({"arithmetic": self._arithmetic} if words and self._arithmetic is not None else {}),
                             **({"contrast": self._contrast} if words and self._contrast is not None else {}))
        return {"predictions": out[0][:, 0, :]}

    def logit_rules(self, rules):
        """Logit rules for the NEXT eval forwards of a word sampler (ssc_runtime.sampling.LogitRules; include/ssc.h:
        ssc_logit_rules): every step's raw logits are edited in front of the draw - a word bias (one row, or one per image of the
        forward), repetition / presence / frequency penalties, blocked n-grams, a minimum length, suppressed tokens.  None (the
        default state), or rules with every control off: off, the forward is what it is without.  ValueError without a word
        sampler (the beam search has decode_rules).  Training forwards, scst_step, score_captions and every beam search never read
        them."""
        if rules is not None:
            if not isinstance(rules, sampling.LogitRules):
                raise ValueError(f"logit_rules: a ssc_runtime.sampling.LogitRules or None, got {type(rules).__name__}")
            if self.sampler is None or self.sampler.beam_search or self.sampled_beam:
                raise ValueError("logit_rules needs a word sampler (MODEL.DECODE_SAMPLER 'multinomial', 'top-k' or 'top-p' without "
                                 "MODEL.SAMPLED_BEAM_SEARCH): the logit rules belong to the word-sampled decode")
            rules.check(self._vocabulary.get_vocab_size(), self._boundary_index, self._max_caption_length,
                        rules.bias.size(0) if rules.bias is not None else 1)
            if not rules.active:
                rules = None
        self._logit_rules = rules

    def truncation(self, truncation):
        """A truncation for the NEXT eval forwards of a word sampler (ssc_runtime.sampling.Truncation; include/ssc.h:
        ssc_truncation): every step's distribution is cut - typical, min-p, eta or epsilon - between the logit rules and the draw.
        None (the default state) or an inactive one: off, the forward is what it is without.  ValueError without a word sampler.
        Training forwards, scst_step, score_captions and every beam search never read it."""
        if truncation is not None:
            if not isinstance(truncation, sampling.Truncation):
                raise ValueError(f"truncation takes a ssc_runtime.sampling.Truncation or None, got {type(truncation).__name__}")
            if self.sampler is None or self.sampler.beam_search or self.sampled_beam:
                raise ValueError("truncation needs a word sampler (MODEL.DECODE_SAMPLER 'multinomial', 'top-k' or 'top-p' without "
                                 "MODEL.SAMPLED_BEAM_SEARCH): the truncation belongs to the word-sampled decode")
            if not truncation.active:
                truncation = None
        self._truncation = truncation

    def mirostat(self, mirostat):
        """A Mirostat for the NEXT eval forwards of a word sampler (ssc_runtime.sampling.Mirostat; include/ssc.h: ssc_mirostat):
        the surprise of every caption's words is held at the target - a cut behind the truncation, an update behind the draw.
        None (the default state) or an inactive one: off, the forward is what it is without.  ValueError without a word sampler.
        Training forwards, scst_step, score_captions and every beam search never read it."""
        if mirostat is not None:
            if not isinstance(mirostat, sampling.Mirostat):
                raise ValueError(f"mirostat takes a ssc_runtime.sampling.Mirostat or None, got {type(mirostat).__name__}")
            if self.sampler is None or self.sampler.beam_search or self.sampled_beam:
                raise ValueError("mirostat needs a word sampler (MODEL.DECODE_SAMPLER 'multinomial', 'top-k' or 'top-p' without "
                                 "MODEL.SAMPLED_BEAM_SEARCH): Mirostat belongs to the word-sampled decode")
            if not mirostat.active:
                mirostat = None
        self._mirostat = mirostat

    def arithmetic(self, arithmetic):
        """Arithmetic sampling for the NEXT eval forwards of a word sampler (ssc_runtime.sampling.Arithmetic; include/ssc.h:
        ssc_arith): every step's draw is made by inverse CDF along a code point per caption, the codes of an image a randomly
        shifted lattice.  None (the default state): off, the forward is what it is without.  ValueError without a word sampler.
        Training forwards, scst_step, score_captions and every beam search never read it."""
        if arithmetic is not None:
            if not isinstance(arithmetic, sampling.Arithmetic):
                raise ValueError(f"arithmetic takes a ssc_runtime.sampling.Arithmetic or None, got {type(arithmetic).__name__}")
            if self.sampler is None or self.sampler.beam_search or self.sampled_beam:
                raise ValueError("arithmetic needs a word sampler (MODEL.DECODE_SAMPLER 'multinomial', 'top-k' or 'top-p' without "
                                 "MODEL.SAMPLED_BEAM_SEARCH): arithmetic sampling belongs to the word-sampled decode")
        self._arithmetic = arithmetic

    def contrast(self, contrast):
        """A contrast for the NEXT eval forwards of a word sampler (ssc_runtime.contrast.Contrast; include/ssc.h: ssc_contrast):
        an amateur stream - degraded features, z at the prior mean, a neutral sentiment, a weak checkpoint - is decoded in lock-step
        and every step's logits are contrasted with it in front of the logit rules.  None (the default state) or an inactive one:
        off, the forward is what it is without.  ValueError without a word sampler.  Training forwards, scst_step, score_captions and
        every beam search never read it."""
        if contrast is not None:
            from ssc_runtime.contrast import Contrast
            if not isinstance(contrast, Contrast):
                raise ValueError(f"contrast takes a ssc_runtime.contrast.Contrast or None, got {type(contrast).__name__}")
            if self.sampler is None or self.sampler.beam_search or self.sampled_beam:
                raise ValueError("contrast needs a word sampler (MODEL.DECODE_SAMPLER 'multinomial', 'top-k' or 'top-p' without "
                                 "MODEL.SAMPLED_BEAM_SEARCH): the contrast belongs to the word-sampled decode")
            if not contrast.active:
                contrast = None
        self._contrast = contrast

    def reconstruct_captions(self, image_features: torch.Tensor, caption_tokens: torch.Tensor, sentiment=None, beam: Optional[int] = None,
                             eps=None, prior_samples: int = 4, prior_seed: Optional[int] = None):
        """Reconstruction through z with the model as it stands: every caption (B, L) int64 in the training layout is encoded on its
        own image by the posterior branch (eps (L + 1, B, Z): its noise; None: the mean path), decoded back by the beam search under
        its own z path, compared with the given words (token accuracy, exact rate, word error rate) and scored teacher-forced
        under the path and under prior_samples prior samples (0: not under the prior - the call then draws nothing).  No autograd; a backward() of an earlier training forward is not disturbed.
        -> ssc_runtime.guide.Reconstruction.  Not for SENTIMENT_VAE = 2."""
        from ssc_runtime.guide import reconstruct_captions
        eng = self._engine()
        B = image_features.size(0)
        sent = sentiment.reshape(B) if sentiment is not None else None
        with torch.no_grad():
            return reconstruct_captions(eng, self._dec, image_features.to(eng.device, torch.float32), sent, caption_tokens,
                                        int(beam or self._beam_search.beam_size), self._boundary_index, eps=eps,
                                        prior_samples=prior_samples, pad_index=self._pad_index, prior_seed=prior_seed)

    def _traced(self, pred, rec, sel):
        """The eval forward's output dict: predictions and, with decode_attention set, the trace of captions `sel` (B,) of `rec`."""
        out = {"predictions": pred}
        if rec:
            n = pred.size(-1)
            tr = self._dec.attention(rec[0], sel, maps=self._decode_attention == "full", summary=True)
            out.update(attention_top_region=tr.top_region[:, :n], attention_top_weight=tr.top_weight[:, :n],
                       attention_entropy=tr.entropy[:, :n])
            if tr.maps is not None:
                out["attention"] = tr.maps[:, :n]
        return out

    def _traced_beam_decode(self, image_features, obj_means, sentiment, fsm, num_constraints):
        """Eval forward of the plain / constrained beam search with decode_attention or decode_guide set: the search in one library
        call (DecodeEngine.search), the noise drawn as the step-by-step path draws it (one (rows, Z) draw per step)."""
        from ssc_runtime.decoding import select_best_state_simple_batched
        B = image_features.size(0)
        L = self._max_caption_length
        dev = self._eng.device
        ctx = self._image_context(image_features, obj_means)
        k, per = self._beam_search.beam_size, self._beam_search.per_node_beam_size
        fsm_d = None
        if fsm is not None:
            if not self.cbs_simple:
                raise ValueError("decode_attention / decode_guide with a constraint machine needs CBS_SIMPLE")
            fsm_d = fsm.to(dev).to(torch.uint8).contiguous()
        S = 1 if fsm_d is None else fsm_d.size(1)
        eps0 = self._draw_eps(1, B, dev)[0]
        eps = self._draw_eps(L - 1, B * S * k, dev) if L > 1 else None
        sent = sentiment.reshape(B) if sentiment is not None else None
        beams, lps, *rec = self._dec.search(ctx, sent, 1, k, per or k, L, self._boundary_index, eps0, eps, fsm=fsm_d,
                                            attention=self._decode_attention is not None, guide=self._decode_guide)
        state = torch.zeros(B, dtype=torch.long, device=dev)
        if fsm_d is not None and S > 1:
            state = select_best_state_simple_batched(lps, num_constraints, self._min_constraints_to_satisfy)
        rows = torch.arange(B, device=dev)
        return self._traced(beams[rows, state, 0, :], rec, (rows * S + state) * k)

    def score_captions(self, image_features: torch.Tensor, caption_tokens: torch.Tensor, sentiment=None, obj_atts=None,
                       n_samples: Optional[int] = None, layout: str = "padded", want_tokens: bool = False, want_ranks: bool = False,
                       eps_steps=None, attention: Optional[str] = None):
        """How likely are the given captions under the model as it stands: image_features (B, R, F), caption_tokens (B, L) or
        (B, C, L) int64 - by default in the training layout (0-padded, no boundary tokens; layout="decoded": a decoder's output) -,
        each scored under n_samples (default: MODEL.N_Z_SAMPLES) latent samples drawn from the prior, the pooled prior of
        SENTIMENT_VAE = 2 included (obj_atts as in forward()).  eps_steps: the caller's own noise, one (B * C * n_samples, Z) tensor per
        step (default: a generator of the call's own, seeded by one draw of the global CPU generator).  One library call, no autograd; the mode (train / eval) is left as
        it is and plays no part.  -> ssc_runtime.inference.CaptionScores.
        The image context is formed from the parameters as they are NOW, so the call is correct between optimizer steps - unless
        the caller has set DecodeEngine.weights_frozen, which promises that they do not change.
        attention: None, "summary" or "full" - CaptionScores.attention then holds every (caption, sample)'s trace."""
        from ssc_runtime.inference import score_captions
        self._engine()
        B, R, _ = image_features.shape
        caps = caption_tokens if caption_tokens.dim() == 3 else caption_tokens.unsqueeze(1)
        obj_means = self._obj_means(obj_atts, B, R)
        sent = sentiment.reshape(B) if sentiment is not None else None
        with torch.no_grad():
            return score_captions(self._dec, image_features.to(self._eng.device, torch.float32), sent, caps,
                                  n_samples or self.n_z_samples, self._boundary_index, layout, eps_steps=eps_steps, obj_means=obj_means,
                                  want_tokens=want_tokens, want_ranks=want_ranks, attention=attention)

    def posterior_score_captions(self, image_features: torch.Tensor, caption_tokens: torch.Tensor, sentiment=None, obj_atts=None,
                                 n_samples: int = 1, eps=None, want_steps: bool = False):
        """The given captions under the POSTERIOR branch of the model as it stands (encoder LSTM, fc_mean, fc_log_var): the log
        importance weights log p(x | z, image) + log p(z) - log q(z | x) of n_samples draws z ~ q(z | x) per caption, the ELBO, the
        importance-weighted bound, and the training KL per caption, per step and per latent dimension.  image_features (B, R, F),
        caption_tokens (B, L) or (B, C, L) int64 in the training layout (0-padded, no boundary tokens); obj_atts as in forward()
        (SENTIMENT_VAE = 2).  eps: the caller's own noise (L + 1, B * C * n_samples, Z), rows (image, caption, sample); default: a
        generator of the call's own, seeded by one draw of the global CPU generator.  No autograd; the parameters are read as they
        are at the call; the mode (train / eval) is left as it is and plays no part; a backward() of an earlier training forward is
        not disturbed.  -> ssc_runtime.inference.PosteriorScores."""
        from ssc_runtime.inference import posterior_score_captions
        eng = self._engine()
        B, R, _ = image_features.shape
        caps = caption_tokens if caption_tokens.dim() == 3 else caption_tokens.unsqueeze(1)
        obj_means = self._obj_means(obj_atts, B, R)
        sent = sentiment.reshape(B).to(eng.device, torch.float32) if sentiment is not None else None
        with torch.no_grad():
            return posterior_score_captions(eng, image_features.to(eng.device, torch.float32), sent, caps, n_samples, eps=eps,
                                            obj_means=obj_means, pad_index=self._pad_index, want_steps=want_steps)

    def scst_step(self, image_features: torch.Tensor, image_ids, sentiment=None, obj_atts=None, *, references, lr, seed,
                  kld_weight: float = 750.0, momentum: float = 0.9, weight_decay: float = 0.001, max_norm: float = 12.5,
                  decoder_frozen: bool = False, group=None, n_samples: int = 5, sampler=None, baseline: str = "loo",
                  reward_weights=None, max_steps: Optional[int] = None, optim=None):
        """One self-critical training step (ssc_runtime.scst.SelfCritical.step) on the engines this module owns: n_samples captions
        per image are sampled from the model as it stands, rewarded by CIDEr-D (reward_weights: B1, B2, B3, B4, ROUGE-L, CIDEr-D)
        against `references` (a CaptionReferences keyed by image_ids), and the parameters are updated in place - clip + SGD on the
        flat buffers, as scripts/train.py --fused-optimizer (optim: a ssc_runtime.engine.OptimSpec, clip + Adam / AdamW instead).  obj_atts as in forward().  max_steps defaults to the maximum caption
        length.  -> (loss (B * n_samples,), kld (B * n_samples,), stats (4,) fp64: mean reward, mean baseline, mean |advantage|, share
        of samples without an end)."""
        from ssc_runtime.scst import CIDER_ONLY, SelfCritical
        eng = self._engine()
        B, R, _ = image_features.shape
        weights = tuple(reward_weights) if reward_weights is not None else CIDER_ONLY
        steps = int(max_steps or self._max_caption_length)
        key = (id(references), n_samples, repr(sampler), baseline, weights, steps)
        if self._scst is None or self._scst[0] != key or self._scst[1].eng is not eng:
            self._scst = (key, SelfCritical(eng, self._dec, references, self._vocabulary, n_samples, sampler, baseline, weights, steps),
                          references)
        sent = sentiment.reshape(B) if sentiment is not None else None
        return self._scst[1].step(image_features, image_ids, sent, lr, kld_weight, momentum, weight_decay, max_norm, decoder_frozen,
                                  group, seed, self._obj_means(obj_atts, B, R), optim)

    def _sample_decode(self, image_features, obj_means, sentiment):
        """Eval forward with a word sampler: the whole decode in one library call (DecodeEngine.sample).  The latent noise is drawn
        for every step up front from the same source as the beam path's (one (B, Z) draw per step); the word seed is one draw from
        the global generator.  With the Gumbel sampler: the stochastic beam search (DecodeEngine.stochastic_beam), noise drawn as
        the beam path draws it ((B, Z) for the first step, (B * beam, Z) for every later one), beam 0 returned; the sampled-node
        beam search (sampled_beam, DecodeEngine.sampled_beam) likewise."""
        B = image_features.size(0)
        L = self._max_caption_length
        dev = self._eng.device
        ctx = self._image_context(image_features, obj_means)
        if self.sampler.beam_search or self.sampled_beam:
            k = self._beam_search.beam_size
            eps0 = self._draw_eps(1, B, dev)[0]
            eps = self._draw_eps(L - 1, B * k, dev) if L > 1 else None
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())
            sent = sentiment.reshape(B) if sentiment is not None else None
            run = self._dec.sampled_beam if self.sampled_beam else self._dec.stochastic_beam
            beams, _, *rec = run(ctx, sent, 1, k, k // 2 or k, L, self._boundary_index, eps0, eps, self.sampler, seed,
                                 attention=self._decode_attention is not None)
            return self._traced(beams[:, 0, :], rec, torch.arange(B, device=dev) * k)
        eps = self._draw_eps(L, B, dev)
        seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        sent = sentiment.reshape(B) if sentiment is not None else None
        pred, _, *rec = self._dec.sample(ctx, sent, 1, L, self._boundary_index, eps[0], eps[1:] if L > 1 else None, self.sampler, seed,
                                         attention=self._decode_attention is not None, guide=self._decode_guide,
                                         **({"logit_rules": self._logit_rules} if self._logit_rules is not None else {}),
                                         **({"truncation": self._truncation} if self._truncation is not None else {}),
                                         **({"mirostat": self._mirostat} if self._mirostat is not None else {}),
                                         **({"arithmetic": self._arithmetic} if self._arithmetic is not None else {}),
                                         **({"contrast": self._contrast} if self._contrast is not None else {}))
        return self._traced(pred, rec, torch.arange(B, device=dev))

    def _diverse_beam_decode(self, image_features, obj_means, sentiment):
        """Eval forward with MODEL.DIVERSE_BEAM_SEARCH: the diverse beam search in one library call (DecodeEngine.diverse_beam), the
        noise drawn as the beam path draws it; the caption with the highest log-prob of every image (ties: the lower beam)."""
        B = image_features.size(0)
        L = self._max_caption_length
        dev = self._eng.device
        ctx = self._image_context(image_features, obj_means)
        k = self._beam_search.beam_size
        eps0 = self._draw_eps(1, B, dev)[0]
        eps = self._draw_eps(L - 1, B * k, dev) if L > 1 else None
        sent = sentiment.reshape(B) if sentiment is not None else None
        beams, lps, *rec = self._dec.diverse_beam(ctx, sent, 1, k, self.diverse_beam.per_node(k), L, self._boundary_index, eps0, eps,
                                                  self.diverse_beam, attention=self._decode_attention is not None)
        bi = lps.argmax(-1)
        return self._traced(beams.gather(1, bi.view(B, 1, 1).expand(B, 1, beams.size(-1))).squeeze(1), rec,
                            torch.arange(B, device=dev) * k + bi)

    def _rules_beam_decode(self, image_features, obj_means, sentiment):
        """Eval forward with decode rules: the beam search under them in one library call (DecodeEngine.rules_beam), the noise
        drawn as the beam path draws it; beam 0 of every image - the best caption under the length penalty."""
        B = image_features.size(0)
        L = self._max_caption_length
        dev = self._eng.device
        ctx = self._image_context(image_features, obj_means)
        k = self._beam_search.beam_size
        eps0 = self._draw_eps(1, B, dev)[0]
        eps = self._draw_eps(L - 1, B * k, dev) if L > 1 else None
        sent = sentiment.reshape(B) if sentiment is not None else None
        beams, _, _, _, *rec = self._dec.rules_beam(ctx, sent, 1, k, k // 2 or k, L, self._boundary_index, eps0, eps, self.decode_rules,
                                                    attention=self._decode_attention is not None)
        return self._traced(beams[:, 0, :], rec, torch.arange(B, device=dev) * k)

    def _image_context(self, image_features, obj_means=None):
        """Per-image terms (mask, averaged features, projected features, hoisted gate term) for the eval decode step, computed
        once per image set and parameter version.  The cache entry keeps a REFERENCE to the caller's tensor and is hit only
        for that very tensor object at the same in-place version: a freed tensor's address can be handed to the next batch
        by the caching allocator (same pointer, same shape, version 0), so a key made of data_ptr/shape would alias."""
        c = self._ctx_cache
        if (c is None or c[0] is not image_features or c[1] != image_features._version or
                c[3] != self._eng.param_version() or c[4] is not obj_means):
            ctx = self._dec.prepare(image_features.float(), obj_means)
            self._ctx_cache = (image_features, image_features._version, ctx, self._eng.param_version(), obj_means)
        return self._ctx_cache[2]

    def _rows(self, t, B, G):
        """(B, k) per-image tensor -> (G, k) per-row, batch-major."""
        if t is None:
            return None
        t = t.reshape(B, -1)
        return t.unsqueeze(1).expand(B, G // B, t.size(1)).reshape(G, t.size(1))

    def _decode_step(self, image_features, obj_atts, previous_predictions, states=None, sentiment=None, attrib_cond=None,
                     prior_mean=None, prior_var=None):
        """One decoding step (updown_captioner.py:371-455).  Eval mode: rows = B * net_beam_size, returns the 5-tuple
        (log_probs, states, prior_mean, prior_log_var, attention_weights).  prior_mean / prior_var are derived from
        `sentiment` (SENTI_PRIOR_MULTIP, PRIOR_STD) exactly as forward() does (:249-261)."""
        if self.training:
            # stand-alone training-mode step (no autograd): the 7-tuple of updown_captioner.py:452-453.  The
            # differentiable path is forward(), which fuses all T steps.
            eng = self._engine()
            G = previous_predictions.size(0)
            emb = self._embedding_layer.weight.detach()[previous_predictions.to(eng.device)]
            eps = self._eps_override.pop(0) if self._eps_override is not None else (
                torch.randn(G, self.z_space, device=eng.device) if self.eps_source == "device" else torch.randn(G, self.z_space))
            h_dec, states, mean, log_var, alpha, _ = cell_train_step(eng.dims, eng.params.views, image_features.to(eng.device),
                                                                     emb, states, sentiment, eps)
            d = eng.dims
            logits = torch.empty(G, d.V, device=eng.device)
            lib = _lib.load()
            if self._tied:
                raise NotImplementedError("stand-alone training step with the tied head: use forward()")
            ow = eng.params.views["_output_layer.weight"]
            from ssc_runtime.cellops import _gemm
            _gemm(lib, [(h_dec.data_ptr(), d.H, ow.data_ptr(), ow.stride(0), d.H)], G, d.V, logits,
                  bias=eng.params.views["_output_layer.bias"])
            pm = (sentiment.reshape(G, 1).to(eng.device) * d.pm_scale).expand(G, self.z_space) if (
                sentiment is not None and d.pm_scale != 0.0) else torch.zeros(G, self.z_space, device=eng.device)
            plv = torch.full((G, self.z_space), float(torch.log(torch.tensor(d.prior_var))), device=eng.device)
            return logits, states, mean, log_var, pm, plv, alpha
        eng = self._engine()
        dev = eng.device
        B = image_features.size(0)
        G = previous_predictions.size(0)
        d = eng.dims
        obj_means = obj_atts if (d.kld_mode == 2 and torch.is_tensor(obj_atts)) else self._obj_means(obj_atts, B, image_features.size(1))
        ctx = self._image_context(image_features, obj_means)
        sent_rows = self._rows(sentiment, B, G) if sentiment is not None else None
        if self._eps_override is not None:
            eps = self._eps_override.pop(0)
        elif self.eps_source == "device":
            eps = torch.randn(G, self.z_space, device=dev)
        else:
            eps = torch.randn(G, self.z_space)
        # prior_mean / prior_var: what forward() derives from `sentiment` (updown_captioner.py:249-261) unless the caller hands its own
        # (:371-381); per image (B, Z) -> one row per beam, batch-major like the image features, or already (G, Z)
        def per_row(t):
            if t is None:
                return None
            t = t.to(dev, torch.float32)
            return t if t.size(0) == G else self._rows(t, B, G)
        pm_in, pv_in = per_row(prior_mean), per_row(prior_var)
        if self.simple_vae and pm_in is not None:
            pm_in = torch.zeros_like(pm_in)            # updown_cell.py:165-166
        pm_out = torch.empty(G, self.z_space, device=dev) if d.kld_mode == 2 else None
        lp, states, alpha = self._dec.step(ctx, previous_predictions, states, sent_rows, eps, prior_mean_out=pm_out,
                                           prior_mean=None if d.kld_mode == 2 else pm_in, prior_var=pv_in)
        if pm_out is not None:
            pm = pm_out                                  # the attention-pooled attribute means (updown_cell.py:160-163)
        elif pm_in is not None:
            pm = pm_in
        elif sent_rows is not None and d.pm_scale != 0.0:
            pm = (sent_rows * d.pm_scale).expand(G, self.z_space)
        else:
            pm = torch.zeros(G, self.z_space, device=dev)
        plv = pv_in.log() if pv_in is not None else torch.full((G, self.z_space), float(torch.log(torch.tensor(d.prior_var))), device=dev)
        return lp, states, pm, plv, alpha

    def _cell_forward(self, image_features, token_embedding, states, training, sentiment, prior_mean, prior_var, eps):
        """UpDownCell.forward backend (eval branch; updown_cell.py:86-231 with training=False)."""
        if training:  # stand-alone training-mode cell step (encoder LSTM + posterior sample), no autograd
            eng = self._engine()
            G = token_embedding.size(0)
            if eps is None:
                eps = torch.randn(G, self.z_space)
            h_dec, new_states, mean, log_var, alpha, _ = cell_train_step(eng.dims, eng.params.views,
                                                                         image_features.to(eng.device),
                                                                         token_embedding.to(eng.device), states, sentiment, eps)
            d = eng.dims
            pm = prior_mean if prior_mean is not None else torch.zeros(G, self.z_space, device=eng.device)
            if self.simple_vae:
                pm = torch.zeros_like(pm)
            pv = prior_var if prior_var is not None else torch.full((G, self.z_space), d.prior_var, device=eng.device)
            return h_dec, new_states, mean, log_var, pm, pv.log(), alpha
        eng = self._engine()
        G = token_embedding.size(0)
        B = image_features.size(0)
        ctx = self._image_context(image_features)
        if eps is None:
            eps = torch.randn(G, self.z_space)
        sent_rows = self._rows(sentiment, B, G) if sentiment is not None and sentiment.size(0) == B else sentiment
        d = eng.dims
        # the cell samples z from the prior it is HANDED (updown_cell.py:200-208)
        pm = prior_mean.to(eng.device, torch.float32) if prior_mean is not None else torch.zeros(G, self.z_space, device=eng.device)
        if self.simple_vae:
            pm = torch.zeros_like(pm)                  # updown_cell.py:165-166
        pv = prior_var.to(eng.device, torch.float32) if prior_var is not None else torch.full((G, self.z_space), d.prior_var, device=eng.device)
        _, new_states, alpha = self._dec.step_from_embedding(ctx, token_embedding, states, sent_rows, eps,
                                                             prior_mean=pm if prior_mean is not None else None,
                                                             prior_var=pv if prior_var is not None else None)
        return new_states["h_decoder"], new_states, pm, pv.log(), pm, pv.log(), alpha

    def _get_loss(self, logits: torch.Tensor, targets: torch.Tensor, target_mask: torch.Tensor,
                  label_smoothing: float = 0.0) -> torch.Tensor:
        """(batch,) summed masked negative log-likelihood of the targets (updown_captioner.py:457-466: target length times allennlp's
        per-sequence average) on the HIP path (ssc_ce_fwd: row-wise log-sum-exp + NLL, the kernel inside ssc_train_fwd).  logits
        (B, T, V), targets (B, T) int64, target_mask (B, T).  The training forward computes this inside its fused call; this is the
        stand-alone entry the reference exposes.  label_smoothing in [0, 1): the smoothed loss instead (ssc_ce_fwd_smooth).
        No autograd."""
        label_smoothing = check_label_smoothing(label_smoothing)
        lib = _lib.load()
        dev = logits.device
        if dev.type != "cuda":
            raise RuntimeError("UpDownCaptioner._get_loss runs on a ROCm GPU only (no CPU fallback)")
        B, T, V = logits.shape
        lg = logits.detach().to(torch.float32).transpose(0, 1).contiguous().view(T * B, V)     # time-major rows (t, b)
        tg = targets.to(dev, torch.int64).t().contiguous()
        w = target_mask.to(dev, torch.float32).t().contiguous()
        nvalid = w.sum(0).contiguous()
        lse = torch.empty(3 * T * B, dtype=torch.float32, device=dev)
        loss = torch.empty(B, dtype=torch.float32, device=dev)
        lib.ssc_ce_fwd_smooth(_lib.ptr(lg), V, _lib.ptr(tg), _lib.ptr(w), _lib.ptr(nvalid), T, B, V, label_smoothing, _lib.ptr(lse),
                              _lib.ptr(loss), None, _lib.stream_ptr())
        return loss


class _HostRef:
    """Weak-ish back reference from the cell to its captioner that nn.Module will not register as a submodule."""

    def __init__(self, host):
        object.__setattr__(self, "_h", host)

    def __getattr__(self, name):
        return getattr(object.__getattribute__(self, "_h"), name)
