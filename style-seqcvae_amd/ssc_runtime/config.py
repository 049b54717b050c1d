"""Config with the reference's keys, defaults, yaml merge, dotted CLI overrides, validation and freezing
(updown-baseline/updown/config.py:4-154), on PyYAML (yacs is not a dependency here)."""
import ast
import copy
from typing import Any, List, Optional

import yaml


class _Node(dict):
    """Attribute-access dict (the part of yacs.CfgNode the code base uses)."""

    def __init__(self, d=None):
        super().__init__()
        object.__setattr__(self, "_frozen", False)
        for k, v in (d or {}).items():
            self[k] = _Node(v) if isinstance(v, dict) else v

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k)

    def __setattr__(self, k, v):
        if object.__getattribute__(self, "_frozen"):
            raise AttributeError(f"config is frozen; cannot set {k}")
        self[k] = v

    def freeze(self):
        object.__setattr__(self, "_frozen", True)
        for v in self.values():
            if isinstance(v, _Node):
                v.freeze()

    def to_dict(self):
        return {k: (v.to_dict() if isinstance(v, _Node) else v) for k, v in self.items()}


def _defaults() -> dict:
    # key set and default values: updown-baseline/updown/config.py:6-104
    return {
        "LOG_TO_FILE": True, "CHECKPOINT_EVERY_N_EPOCHS": 10, "PRINT_EVERY_N_BATCHES": 100, "RANDOM_SEED": 0,
        "DATA": {
            "VOCABULARY": "data/vocabulary",
            "TRAIN_FEATURES": "data/coco_train2017_vg_detector_features_adaptive.h5",
            "INFER_FEATURES": "data/nocaps_val_vg_detector_features_adaptive.h5",
            "TRAIN_CAPTIONS": "data/coco/captions_train2017.json",
            "INFER_CAPTIONS": "data/nocaps/nocaps_val_image_info.json",
            "SENTICAP_CAPTIONS": "", "DO_LOAD_COCO": True, "DO_LOAD_SENTICAP": False, "SENTICAP_SENTIMENT": "",
            "EXPERT_CAPTIONS": "", "COCO_ATTRIBS_OBJS": "", "REMOVE_SAMPLES_WITHOUT_ATTRIBS": False,
            "USE_OBJ_ATT_PREDS": False, "ATT_PRED_THRESH": 0.3, "MAX_CAPTION_LENGTH": 20,
            "CBS": {"INFER_BOXES": "data/nocaps_val_oi_detector_boxes.json", "CLASS_HIERARCHY": "data/cbs/class_hierarchy.json",
                    "WORDFORMS": "", "WORDFORMS_ATTRIBS": "", "NMS_THRESHOLD": 0.85, "MAX_GIVEN_OBJECTS": 2,
                    "MAX_GIVEN_CONSTRAINTS": 3, "MAX_WORDS_PER_CONSTRAINT": 3},
        },
        "MODEL": {
            "IMAGE_FEATURE_SIZE": 2048, "EMBEDDING_SIZE": 1000, "HIDDEN_SIZE": 1200, "ATTENTION_PROJECTION_SIZE": 768,
            "BEAM_SIZE": 5, "USE_CBS": False, "CBS_SIMPLE": True, "MIN_CONSTRAINTS_TO_SATISFY": 2,
            "PRIOR_MODE": "AG", "DO_USE_CLUSTER_VECTOR": True, "FC_LAYER_PER_ATTRIB": True, "NUM_LSTM_LAYERS": 1,
            "LSTM_DROPOUT": 0.1, "Z_SPACE": 150, "SENTIMENT_VAE": 0, "SENTI_PRIOR_MULTIP": 1.0,
            "LATENT_EMBEDDING_MULTIP": 1.0, "KLD_WEIGHT": 750, "N_Z_SAMPLES": 0, "STATE_MACHINE_PER_Z_SAMPLE": False,
            "LATENT_EMBEDDING": "glove", "PRIOR_STD": 1.0, "SIMPLE_VAE": True, "DO_USE_KLD_ANNEALING": False,
            "KLD_DECREASING": False, "KLD_INITIAL_WEIGHT": 2.0, "KLD_ANNEALING_PER_EPOCH": 0.25,
            "KLD_N_EPOCHS_BEFORE_RESET": 4,
            # word-level sampling in place of beam search (ssc_runtime/sampling.py): "beam" (default), "multinomial", "top-k",
            # "top-p" - the reference's MultinomialSampler / TopKSampler / TopPSampler (modules/beam_search.py:103-293); needs
            # BEAM_SIZE 1 and no CBS
            "DECODE_SAMPLER": "beam", "SAMPLER_TOP_K": 0, "SAMPLER_TOP_P": 1.0, "SAMPLER_TEMPERATURE": 1.0,
            # stochastic beam search (the reference's GumbelSampler, modules/beam_search.py:294-432): BEAM_SIZE captions sampled without
            # replacement per latent sample; needs DECODE_SAMPLER "beam" and no CBS; SAMPLER_TEMPERATURE applies
            "STOCHASTIC_BEAM_SEARCH": False,
            # sampled-node beam search (the reference's BeamSearch with a word sampler, modules/beam_search.py:592-768): every beam
            # draws BEAM_SIZE // 2 (or BEAM_SIZE) candidate words from DECODE_SAMPLER, the BEAM_SIZE best by log-prob are kept; needs
            # DECODE_SAMPLER multinomial / top-k / top-p, STOCHASTIC_BEAM_SEARCH False and no CBS.  SAMPLER_WITH_REPLACEMENT: the
            # samplers' with_replacement (the draws of one beam may repeat a word)
            "SAMPLED_BEAM_SEARCH": False, "SAMPLER_WITH_REPLACEMENT": False,
            # diverse beam search (Vijayakumar et al., AAAI 2018: the "Div-BS" baseline; ssc_runtime/sampling.py DiverseBeam): the
            # BEAM_SIZE beams are DIVERSE_BEAM_GROUPS groups searched in order, a word the earlier groups chose at a step costs the
            # later ones DIVERSE_BEAM_STRENGTH per choice; deterministic.  Needs DECODE_SAMPLER "beam", STOCHASTIC_BEAM_SEARCH and
            # SAMPLED_BEAM_SEARCH False, no CBS and BEAM_SIZE % DIVERSE_BEAM_GROUPS == 0; scripts/inference.py then writes the best
            # caption of every group (N_Z_SAMPLES * DIVERSE_BEAM_GROUPS per image)
            "DIVERSE_BEAM_SEARCH": False, "DIVERSE_BEAM_GROUPS": 1, "DIVERSE_BEAM_STRENGTH": 0.5,
            # decode rules of the deterministic beam search (ssc_runtime/sampling.py DecodeRules; ssc_rules_desc): any non-default
            # value selects the beam search under rules (one library call, beam 0 = the best caption under the length penalty).
            # Needs DECODE_SAMPLER "beam", STOCHASTIC_ / SAMPLED_ / DIVERSE_BEAM_SEARCH False and no CBS.
            # NO_REPEAT_NGRAM n: a word that would complete an n-gram the caption already holds is not a candidate (0 = off, 3 is
            # the usual choice; at most 64)
            "NO_REPEAT_NGRAM": 0,
            # MIN_CAPTION_LENGTH m: the caption cannot end before it has m words
            "MIN_CAPTION_LENGTH": 0,
            # LENGTH_PENALTY_ALPHA a: beams are ranked by (summed log-prob) / length ** a, the boundary token counted (0 = the raw
            # sum, which favours short captions; 1 = the mean log-prob per token)
            "LENGTH_PENALTY_ALPHA": 0.0,
            # SUPPRESS_UNKNOWN: @@UNKNOWN@@ is never emitted (its log-prob is not given to the other words)
            "SUPPRESS_UNKNOWN": False,
            # logit rules of the word samplers (ssc_runtime/sampling.py LogitRules; ssc_logit_rules): the raw logits of every step
            # are edited in front of the draw, so the sampler draws from the edited distribution.  A second mechanism, apart from
            # the decode rules above.  Any non-default value needs DECODE_SAMPLER multinomial / top-k / top-p with SAMPLED_ and
            # STOCHASTIC_BEAM_SEARCH False.  SAMPLER_NO_REPEAT_NGRAM n (0 = off, at most 64) and SAMPLER_MIN_LENGTH m as above;
            # SAMPLER_SUPPRESS_UNKNOWN: @@UNKNOWN@@ is never drawn; SAMPLER_REPETITION_PENALTY theta > 0 (1 = off): the logit of a
            # word the caption holds is divided by theta where positive, multiplied where not; SAMPLER_PRESENCE_PENALTY /
            # SAMPLER_FREQUENCY_PENALTY (0 = off): presence + frequency * count is taken off such a logit
            "SAMPLER_NO_REPEAT_NGRAM": 0, "SAMPLER_MIN_LENGTH": 0, "SAMPLER_SUPPRESS_UNKNOWN": False,
            "SAMPLER_REPETITION_PENALTY": 1.0, "SAMPLER_PRESENCE_PENALTY": 0.0, "SAMPLER_FREQUENCY_PENALTY": 0.0,
            # truncation of the word samplers (ssc_runtime/sampling.py Truncation; ssc_truncation): a cut that adapts to each step's
            # entropy, made on the raw logits between the logit rules and the draw.  "none" (default), "typical" (locally typical
            # sampling: the words whose surprise is closest to the entropy, up to a mass of VALUE, default 0.9), "min-p" (at least
            # VALUE times the top word's probability, default 0.05), "eta" / "epsilon" (probability at least
            # min(VALUE, sqrt(VALUE) exp(-entropy)) / VALUE, default 3e-4).  SAMPLER_TRUNCATION_VALUE 0 = the kind's default.  Needs
            # DECODE_SAMPLER multinomial / top-k / top-p with SAMPLED_ and STOCHASTIC_BEAM_SEARCH False
            "SAMPLER_TRUNCATION": "none", "SAMPLER_TRUNCATION_VALUE": 0.0,
            # Mirostat 2.0 for the word samplers (ssc_runtime/sampling.py Mirostat; ssc_mirostat): the surprise of the drawn words
            # is held at SAMPLER_MIROSTAT_TAU bits (0, the default: off) - words more surprising than a running threshold mu are
            # cut behind the truncation, and after each draw mu moves by SAMPLER_MIROSTAT_ETA times the error; mu starts at
            # 2 TAU.  Needs DECODE_SAMPLER multinomial / top-k / top-p with SAMPLED_ and STOCHASTIC_BEAM_SEARCH False
            "SAMPLER_MIROSTAT_TAU": 0.0, "SAMPLER_MIROSTAT_ETA": 0.1,
            # arithmetic sampling for the word samplers (ssc_runtime/sampling.py Arithmetic; ssc_arith): the draw of every step is
            # made by inverse CDF along a code point per caption, the codes of an image a randomly shifted lattice - the captions of
            # an image are stratified instead of independent.  SAMPLER_ARITHMETIC_SHARE_LATENT: the samples of an image also share
            # the latent noise of its first sample, so they differ by their codes alone.  Needs DECODE_SAMPLER multinomial / top-k /
            # top-p with SAMPLED_ and STOCHASTIC_BEAM_SEARCH False
            "SAMPLER_ARITHMETIC": False, "SAMPLER_ARITHMETIC_SHARE_LATENT": False,
            # contrastive decoding of the word samplers (ssc_runtime/contrast.py Contrast; ssc_contrast): an amateur stream is decoded
            # in lock-step with the normal one and every step's logits become lp + CONTRAST_ALPHA (lp - lp_amateur) on the words
            # whose probability is at least CONTRAST_BETA times the top word's.  CONTRAST_ALPHA 0 (default): off.  CONTRAST_AMATEUR:
            # "mean-features" (every region replaced by the image's mean region), "noise-features" (the features under noise of
            # level CONTRAST_NOISE in (0, 1]), "prior-mean" (z at the prior mean), "neutral-sentiment" (sentiment 0).  Needs
            # DECODE_SAMPLER multinomial / top-k / top-p with SAMPLED_ and STOCHASTIC_BEAM_SEARCH False
            "CONTRAST_ALPHA": 0.0, "CONTRAST_BETA": 0.1, "CONTRAST_AMATEUR": "mean-features", "CONTRAST_NOISE": 0.5,
            # attention traces of the eval decode (ssc_attn_record; DecodeEngine.attention): "none" (default), "summary" - per word
            # of every returned caption the region it attended most, the weight there and the entropy of its attention - or "full"
            # - the whole map over the regions as well.  Any decoder; the captions themselves do not change
            "DECODE_ATTENTION": "none",
            # prompted decoding (ssc_start_state, ssc_decode_prime; UpDownCaptioner.decode_prefix): words every caption of the eval
            # decode starts with, e.g. "a happy"; "" (default): off.  Any decoder continues from the prompt; constraints, rules and
            # MAX_CAPTION_LENGTH apply to the continuation.  Not together with DECODE_ATTENTION
            "DECODE_PREFIX": "",
        },
        "OPTIM": {
            "BATCH_SIZE": 150, "NUM_ITERATIONS": 70000, "LR": 0.015, "MOMENTUM": 0.9, "LR_DECAY_EVERY_N": 7,
            "LR_DECAY": 0.5, "LR_DECAY_START_EPOCH": 10, "WEIGHT_DECAY": 0.001, "CLIP_GRADIENTS": 12.5,
            "EPOCH_START_DECODER_TRAINING": 40000, "BEFORE_UPDATE_DECODER_EVERY": 30,
            # the optimiser behind the gradient clip on every path of scripts/train.py: "sgd" (the reference's: MOMENTUM), "adam"
            # (WEIGHT_DECAY as L2 in the gradient) or "adamw" (decoupled WEIGHT_DECAY) - what self-critical fine-tuning is run with,
            # at an LR of 5e-5 or so.  LR, WEIGHT_DECAY, CLIP_GRADIENTS and the linear decay are shared by the kinds
            "OPTIMIZER": "sgd", "ADAM_BETAS": [0.9, 0.999], "ADAM_EPS": 1e-8,
            # label smoothing of the cross-entropy steps (torch.nn.functional.cross_entropy's label_smoothing: the mass is spread
            # over all V classes), in [0, 1); 0 = the reference's plain masked NLL.  Self-critical steps and validation never smooth
            "LABEL_SMOOTHING": 0.0,
            # KL annealing of the cross-entropy steps (ssc_runtime/schedule.py: kl_beta): the KL term of the objective is multiplied
            # by beta(iteration), a pure function of the iteration number.  "none": 1; "linear": from KL_ANNEAL_START to 1 over
            # KL_ANNEAL_ITERS iterations; "cyclical" (Fu et al. 2019): the ramp restarts every KL_ANNEAL_ITERS iterations, rises over
            # the first KL_ANNEAL_RATIO of a cycle and stays at 1 for the rest.  The reference's MODEL.KLD_* annealing keys above are
            # read by nothing there or here
            "KL_ANNEAL": "none", "KL_ANNEAL_ITERS": 10000, "KL_ANNEAL_RATIO": 0.5, "KL_ANNEAL_START": 0.0,
            # free bits: a floor of FREE_BITS nats under the KL (0 = off).  FREE_BITS_MODE "element": every (step, dimension) term,
            # "step": the KL of every step, "dim" (Kingma et al. 2016): the minibatch mean of every latent dimension, summed over the
            # steps - the minibatch of one process.  A term at or below its floor has no gradient.  Self-critical steps and validation
            # are never annealed or floored
            "FREE_BITS": 0.0, "FREE_BITS_MODE": "dim",
            # scheduled sampling of the cross-entropy steps (Bengio et al. 2015; ssc_runtime/schedule.py: ss_prob): from iteration
            # SCHEDULED_SAMPLING_START on (-1 = off) a word the decoder is fed is, with a probability that rises by
            # SCHEDULED_SAMPLING_INCREASE_PROB every SCHEDULED_SAMPLING_INCREASE_EVERY iterations up to SCHEDULED_SAMPLING_MAX_PROB,
            # one the model draws from its own distribution of the previous step ("multinomial", at SCHEDULED_SAMPLING_TEMPERATURE)
            # or its most likely word ("argmax").  Self-critical steps and validation never sample
            "SCHEDULED_SAMPLING_START": -1, "SCHEDULED_SAMPLING_INCREASE_EVERY": 5000, "SCHEDULED_SAMPLING_INCREASE_PROB": 0.05,
            "SCHEDULED_SAMPLING_MAX_PROB": 0.25, "SCHEDULED_SAMPLING_SAMPLER": "multinomial", "SCHEDULED_SAMPLING_TEMPERATURE": 1.0,
            # knowledge distillation of the cross-entropy steps (Hinton et al. 2015; word-level: Kim & Rush 2016): with teacher
            # checkpoints given to scripts/train.py (--distill-checkpoints) the loss of a word is (1 - DISTILL_ALPHA) * the
            # (smoothed) hard loss + DISTILL_ALPHA * DISTILL_TEMPERATURE^2 * KL(teacher || student) at that temperature; 0 = off.
            # DISTILL_MODE: how several teachers are combined, "prob" (the mean of their probabilities) or "logprob" (the normalised
            # mean of their log-probs), as in ensemble decoding.  Not together with scheduled sampling; self-critical steps and
            # validation never distil
            "DISTILL_ALPHA": 0.0, "DISTILL_TEMPERATURE": 1.0, "DISTILL_MODE": "prob",
            # token-level unlikelihood training of the cross-entropy steps (Welleck et al. 2020): a word's loss gains
            # UNLIKELIHOOD_ALPHA * (- sum log(1 - p[c])) over the words c its caption has already used, the word's own target left
            # out - the training-side remedy for repetition; a finite number >= 0, 0 = off.  Not together with DISTILL_ALPHA > 0;
            # self-critical steps and validation never apply it
            "UNLIKELIHOOD_ALPHA": 0.0,
        },
    }


def _merge(dst: dict, src: dict, path=""):
    for k, v in src.items():
        if k not in dst:
            raise KeyError(f"Non-existent config key: {path}{k}")
        if isinstance(dst[k], dict):
            if not isinstance(v, dict):
                raise ValueError(f"{path}{k} must be a mapping")
            _merge(dst[k], v, path + k + ".")
        else:
            dst[k] = _coerce(v, dst[k], path + k)


def _coerce(value: Any, old: Any, key: str):
    if isinstance(value, str) and not isinstance(old, str):
        try:
            value = ast.literal_eval(value)
        except (ValueError, SyntaxError):
            pass
    if isinstance(old, bool) or old is None:
        return value
    if isinstance(old, float) and isinstance(value, int):
        return float(value)
    if isinstance(old, int) and isinstance(value, float) and not isinstance(old, bool):
        return value  # yacs allows int -> float replacement for numeric keys (KLD_WEIGHT: 750 vs 750.0)
    if type(value) is not type(old):
        raise ValueError(f"Type mismatch for config key {key}: {type(old).__name__} vs {type(value).__name__}")
    return value


class Config(object):
    def __init__(self, config_file: Optional[str] = None, config_override: List[Any] = []):
        tree = _defaults()
        if config_file is not None:
            with open(config_file) as f:
                _merge(tree, yaml.safe_load(f) or {})
        if len(config_override) % 2 != 0:
            raise ValueError("config_override must be a list of key value pairs")
        for k, v in zip(config_override[0::2], config_override[1::2]):
            node = tree
            parts = k.split(".")
            for p in parts[:-1]:
                node = node[p]
            if parts[-1] not in node:
                raise KeyError(f"Non-existent config key: {k}")
            node[parts[-1]] = _coerce(v, node[parts[-1]], k)
        self._C = _Node(tree)
        self._validate()
        self._C.freeze()

    def dump(self, file_path: str):
        with open(file_path, "w") as f:
            yaml.safe_dump(self._C.to_dict(), f, default_flow_style=False)

    def _validate(self):
        # updown-baseline/updown/config.py:129-140
        if self._C.MODEL.USE_CBS:
            assert self._C.MODEL.EMBEDDING_SIZE in (300, 600), (
                "Word embeddings must be initialized with fixed GloVe Embeddings (300/600 dim) for CBS decoding; "
                f"found MODEL.EMBEDDING_SIZE {self._C.MODEL.EMBEDDING_SIZE}")
        assert self._C.MODEL.MIN_CONSTRAINTS_TO_SATISFY <= self._C.DATA.CBS.MAX_GIVEN_CONSTRAINTS, \
            "Satisfying more constraints than maximum specified is not possible."
        m = self._C.MODEL
        ngram, min_len, alpha = m.NO_REPEAT_NGRAM, m.MIN_CAPTION_LENGTH, m.LENGTH_PENALTY_ALPHA
        if isinstance(ngram, bool) or not isinstance(ngram, int) or not 0 <= ngram <= 64:
            raise ValueError(f"MODEL.NO_REPEAT_NGRAM must be an integer in 0..64; found {ngram!r}")
        if isinstance(min_len, bool) or not isinstance(min_len, int) or min_len < 0:
            raise ValueError(f"MODEL.MIN_CAPTION_LENGTH must be an integer and not negative; found {min_len!r}")
        if isinstance(alpha, bool) or not isinstance(alpha, (int, float)) or alpha != alpha or abs(alpha) == float("inf"):
            raise ValueError(f"MODEL.LENGTH_PENALTY_ALPHA must be a finite number; found {alpha!r}")
        if not isinstance(m.SUPPRESS_UNKNOWN, bool):
            raise ValueError(f"MODEL.SUPPRESS_UNKNOWN must be True or False; found {m.SUPPRESS_UNKNOWN!r}")
        if ngram or min_len or alpha != 0 or m.SUPPRESS_UNKNOWN:   # the beam search under decode rules is selected
            max_len = self._C.DATA.MAX_CAPTION_LENGTH
            if min_len >= max_len:
                raise ValueError(f"MODEL.MIN_CAPTION_LENGTH ({min_len}) must be below DATA.MAX_CAPTION_LENGTH ({max_len})")
            if max_len > 64:
                raise ValueError("the decode rules (MODEL.NO_REPEAT_NGRAM / MIN_CAPTION_LENGTH / LENGTH_PENALTY_ALPHA / "
                                 f"SUPPRESS_UNKNOWN) need DATA.MAX_CAPTION_LENGTH <= 64; found {max_len}")
        s_ngram, s_min = m.SAMPLER_NO_REPEAT_NGRAM, m.SAMPLER_MIN_LENGTH
        if isinstance(s_ngram, bool) or not isinstance(s_ngram, int) or not 0 <= s_ngram <= 64:
            raise ValueError(f"MODEL.SAMPLER_NO_REPEAT_NGRAM must be an integer in 0..64; found {s_ngram!r}")
        if isinstance(s_min, bool) or not isinstance(s_min, int) or s_min < 0:
            raise ValueError(f"MODEL.SAMPLER_MIN_LENGTH must be an integer and not negative; found {s_min!r}")
        if not isinstance(m.SAMPLER_SUPPRESS_UNKNOWN, bool):
            raise ValueError(f"MODEL.SAMPLER_SUPPRESS_UNKNOWN must be True or False; found {m.SAMPLER_SUPPRESS_UNKNOWN!r}")
        for key in ("SAMPLER_REPETITION_PENALTY", "SAMPLER_PRESENCE_PENALTY", "SAMPLER_FREQUENCY_PENALTY"):
            v = getattr(m, key)
            if isinstance(v, bool) or not isinstance(v, (int, float)) or v != v or abs(v) == float("inf"):
                raise ValueError(f"MODEL.{key} must be a finite number; found {v!r}")
        if not m.SAMPLER_REPETITION_PENALTY > 0:
            raise ValueError(f"MODEL.SAMPLER_REPETITION_PENALTY must be positive; found {m.SAMPLER_REPETITION_PENALTY!r}")
        if (s_ngram or s_min or m.SAMPLER_SUPPRESS_UNKNOWN or m.SAMPLER_REPETITION_PENALTY != 1 or m.SAMPLER_PRESENCE_PENALTY != 0
                or m.SAMPLER_FREQUENCY_PENALTY != 0):   # the sampled decode under logit rules is selected
            max_len = self._C.DATA.MAX_CAPTION_LENGTH
            if s_min >= max_len:
                raise ValueError(f"MODEL.SAMPLER_MIN_LENGTH ({s_min}) must be below DATA.MAX_CAPTION_LENGTH ({max_len})")
            if max_len > 64:
                raise ValueError(f"the logit rules (MODEL.SAMPLER_NO_REPEAT_NGRAM ...) need DATA.MAX_CAPTION_LENGTH <= 64; found {max_len}")
        if m.SAMPLER_TRUNCATION not in ("none", "typical", "min-p", "eta", "epsilon"):
            raise ValueError(f"MODEL.SAMPLER_TRUNCATION must be one of none | typical | min-p | eta | epsilon; found {m.SAMPLER_TRUNCATION!r}")
        tv = m.SAMPLER_TRUNCATION_VALUE
        if isinstance(tv, bool) or not isinstance(tv, (int, float)) or tv != tv:
            raise ValueError(f"MODEL.SAMPLER_TRUNCATION_VALUE must be a number; found {tv!r}")
        hi_ok = tv <= 1 if m.SAMPLER_TRUNCATION in ("typical", "min-p") else tv < 1
        if m.SAMPLER_TRUNCATION != "none" and not (0 <= tv and hi_ok):   # (0: the kind's default)
            raise ValueError(f"MODEL.SAMPLER_TRUNCATION_VALUE must lie in (0, 1] for typical / min-p and in (0, 1) for eta / epsilon, "
                             f"or be 0 for the kind's default; found {tv!r}")
        for key, what in (("SAMPLER_MIROSTAT_TAU", "a finite number of bits >= 0 (0 = off)"), ("SAMPLER_MIROSTAT_ETA", "a finite number >= 0")):
            mv = getattr(m, key)
            if isinstance(mv, bool) or not isinstance(mv, (int, float)) or not 0 <= mv < float("inf"):   # (false for NaN)
                raise ValueError(f"MODEL.{key} must be {what}; found {mv!r}")
        for key in ("SAMPLER_ARITHMETIC", "SAMPLER_ARITHMETIC_SHARE_LATENT"):
            if not isinstance(getattr(m, key), bool):
                raise ValueError(f"MODEL.{key} must be True or False; found {getattr(m, key)!r}")
        if m.SAMPLER_ARITHMETIC_SHARE_LATENT and not m.SAMPLER_ARITHMETIC:
            raise ValueError("MODEL.SAMPLER_ARITHMETIC_SHARE_LATENT needs MODEL.SAMPLER_ARITHMETIC True")
        for key, ok, what in (("CONTRAST_ALPHA", lambda v: 0 <= v < float("inf"), "a finite number >= 0 (0 = off)"),
                              ("CONTRAST_BETA", lambda v: 0 <= v < 1, "in [0, 1)"), ("CONTRAST_NOISE", lambda v: 0 < v <= 1, "in (0, 1]")):
            cv = getattr(m, key)
            if isinstance(cv, bool) or not isinstance(cv, (int, float)) or cv != cv or not ok(cv):
                raise ValueError(f"MODEL.{key} must be {what}; found {cv!r}")
        if m.CONTRAST_AMATEUR not in ("mean-features", "noise-features", "prior-mean", "neutral-sentiment"):
            raise ValueError("MODEL.CONTRAST_AMATEUR must be one of mean-features | noise-features | prior-mean | neutral-sentiment; "
                             f"found {m.CONTRAST_AMATEUR!r}")
        if m.DECODE_ATTENTION not in ("none", "summary", "full"):
            raise ValueError(f"MODEL.DECODE_ATTENTION must be one of none | summary | full; found {m.DECODE_ATTENTION!r}")
        if not isinstance(m.DECODE_PREFIX, str):
            raise ValueError(f"MODEL.DECODE_PREFIX must be a string of words; found {m.DECODE_PREFIX!r}")
        if m.DECODE_PREFIX.strip() and m.DECODE_ATTENTION != "none":
            raise ValueError("MODEL.DECODE_PREFIX cannot be combined with MODEL.DECODE_ATTENTION: the trace would not cover the prefix words")
        o = self._C.OPTIM
        if o.OPTIMIZER not in ("sgd", "adam", "adamw"):
            raise ValueError(f'OPTIM.OPTIMIZER must be "sgd", "adam" or "adamw"; found {o.OPTIMIZER!r}')
        betas = o.ADAM_BETAS
        if len(betas) != 2 or not all(isinstance(b, (int, float)) and 0.0 <= b < 1.0 for b in betas):
            raise ValueError(f"OPTIM.ADAM_BETAS must be two numbers in [0, 1); found {betas!r}")
        if not o.ADAM_EPS > 0:
            raise ValueError(f"OPTIM.ADAM_EPS must be positive; found {o.ADAM_EPS!r}")
        ls = o.LABEL_SMOOTHING
        if isinstance(ls, bool) or not isinstance(ls, (int, float)) or not 0.0 <= ls < 1.0:
            raise ValueError(f"OPTIM.LABEL_SMOOTHING must be a number in [0, 1); found {ls!r}")
        num = lambda x: isinstance(x, (int, float)) and not isinstance(x, bool)
        if o.KL_ANNEAL not in ("none", "linear", "cyclical"):
            raise ValueError(f"OPTIM.KL_ANNEAL must be one of none | linear | cyclical; found {o.KL_ANNEAL!r}")
        if isinstance(o.KL_ANNEAL_ITERS, bool) or not isinstance(o.KL_ANNEAL_ITERS, int) or o.KL_ANNEAL_ITERS < 1:
            raise ValueError(f"OPTIM.KL_ANNEAL_ITERS must be an integer >= 1; found {o.KL_ANNEAL_ITERS!r}")
        if not num(o.KL_ANNEAL_RATIO) or not 0.0 < o.KL_ANNEAL_RATIO <= 1.0:
            raise ValueError(f"OPTIM.KL_ANNEAL_RATIO must be a number in (0, 1]; found {o.KL_ANNEAL_RATIO!r}")
        if not num(o.KL_ANNEAL_START) or not 0.0 <= o.KL_ANNEAL_START <= 1.0:
            raise ValueError(f"OPTIM.KL_ANNEAL_START must be a number in [0, 1]; found {o.KL_ANNEAL_START!r}")
        if not num(o.FREE_BITS) or not 0.0 <= o.FREE_BITS < float("inf"):
            raise ValueError(f"OPTIM.FREE_BITS must be a finite number >= 0; found {o.FREE_BITS!r}")
        if o.FREE_BITS_MODE not in ("element", "step", "dim"):
            raise ValueError(f"OPTIM.FREE_BITS_MODE must be one of element | step | dim; found {o.FREE_BITS_MODE!r}")
        integer = lambda x: isinstance(x, int) and not isinstance(x, bool)
        if not integer(o.SCHEDULED_SAMPLING_START) or o.SCHEDULED_SAMPLING_START < -1:
            raise ValueError(f"OPTIM.SCHEDULED_SAMPLING_START must be an iteration (an integer >= 0) or -1 for off; found {o.SCHEDULED_SAMPLING_START!r}")
        if not integer(o.SCHEDULED_SAMPLING_INCREASE_EVERY) or o.SCHEDULED_SAMPLING_INCREASE_EVERY < 1:
            raise ValueError(f"OPTIM.SCHEDULED_SAMPLING_INCREASE_EVERY must be an integer >= 1; found {o.SCHEDULED_SAMPLING_INCREASE_EVERY!r}")
        for key in ("SCHEDULED_SAMPLING_INCREASE_PROB", "SCHEDULED_SAMPLING_MAX_PROB"):
            if not num(o[key]) or not 0.0 <= o[key] <= 1.0:
                raise ValueError(f"OPTIM.{key} must be a number in [0, 1]; found {o[key]!r}")
        if o.SCHEDULED_SAMPLING_SAMPLER not in ("multinomial", "argmax"):
            raise ValueError(f"OPTIM.SCHEDULED_SAMPLING_SAMPLER must be one of multinomial | argmax; found {o.SCHEDULED_SAMPLING_SAMPLER!r}")
        if not num(o.SCHEDULED_SAMPLING_TEMPERATURE) or not 0.0 < o.SCHEDULED_SAMPLING_TEMPERATURE < float("inf"):
            raise ValueError(f"OPTIM.SCHEDULED_SAMPLING_TEMPERATURE must be a finite number > 0; found {o.SCHEDULED_SAMPLING_TEMPERATURE!r}")
        if not num(o.DISTILL_ALPHA) or not 0.0 <= o.DISTILL_ALPHA <= 1.0:
            raise ValueError(f"OPTIM.DISTILL_ALPHA must be a number in [0, 1]; found {o.DISTILL_ALPHA!r}")
        if not num(o.DISTILL_TEMPERATURE) or not 0.0 < o.DISTILL_TEMPERATURE < float("inf"):
            raise ValueError(f"OPTIM.DISTILL_TEMPERATURE must be a finite number > 0; found {o.DISTILL_TEMPERATURE!r}")
        if o.DISTILL_MODE not in ("prob", "logprob"):
            raise ValueError(f"OPTIM.DISTILL_MODE must be one of prob | logprob; found {o.DISTILL_MODE!r}")
        if not num(o.UNLIKELIHOOD_ALPHA) or not 0.0 <= o.UNLIKELIHOOD_ALPHA < float("inf"):
            raise ValueError(f"OPTIM.UNLIKELIHOOD_ALPHA must be a finite number >= 0; found {o.UNLIKELIHOOD_ALPHA!r}")
        if o.UNLIKELIHOOD_ALPHA > 0 and o.DISTILL_ALPHA > 0:
            raise ValueError(f"OPTIM.UNLIKELIHOOD_ALPHA {o.UNLIKELIHOOD_ALPHA} and OPTIM.DISTILL_ALPHA {o.DISTILL_ALPHA} cannot both be "
                             "positive: unlikelihood training and distillation do not compose")

    def __getattr__(self, attr: str):
        return getattr(self.__dict__["_C"], attr)

    def __str__(self):
        d = self._C.to_dict()
        return "\n".join(yaml.safe_dump({k: d[k]}, default_flow_style=False) for k in ("RANDOM_SEED", "DATA", "MODEL", "OPTIM"))

    def __repr__(self):
        return repr(self._C.to_dict())
