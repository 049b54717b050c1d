#!/usr/bin/env python3
"""Diverse captioning inference on MI355X - counterpart of the reference's var_updown/scripts/inference.py:19-191: same
flags and JSON output ([{"image_id", "caption"}...], N_Z_SAMPLES captions per image), but images x latent samples are
decoded as ONE batched beam search per chunk instead of a per-image Python loop of N_Z_SAMPLES model calls."""
import argparse
import json
import math
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "style-seqcvae_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ssc_runtime.config import Config  # noqa: E402
from ssc_runtime.data import SyntheticCaptionData, TensorFileData  # noqa: E402
from ssc_runtime.inference import diverse_decode, score_captions  # noqa: E402
from ssc_runtime import sampling  # noqa: E402
from ssc_runtime.contrast import AMATEURS  # noqa: E402
from ssc_runtime.vocab import Vocabulary  # noqa: E402
from var_updown.models import CaptionerEnsemble, UpDownCaptioner  # noqa: E402

parser = argparse.ArgumentParser("Run diverse-decoding inference with a trained Style-SeqCVAE captioner (MI355X).")
parser.add_argument("--config", required=True)
parser.add_argument("--config-override", default=[], nargs="*")
parser.add_argument("--gpu-ids", required=True, nargs="+", type=int)
parser.add_argument("--cpu-workers", type=int, default=0)
parser.add_argument("--in-memory", action="store_true")
parser.add_argument("--checkpoint-path", default="", help="checkpoint with a 'model' state_dict; empty: random init")
parser.add_argument("--ensemble-checkpoints", default=[], nargs="+", metavar="P",
                    help="ensemble decoding: further checkpoints of the SAME configuration and vocabulary (--checkpoint-path is member "
                         "0); one beam search over all members, their word distributions averaged at every step")
parser.add_argument("--ensemble-weights", default=None, nargs="+", type=float,
                    help="with --ensemble-checkpoints: one positive weight per member, member 0 first (any scale; default uniform)")
parser.add_argument("--ensemble-mode", default=None, choices=["prob", "logprob"],
                    help="with --ensemble-checkpoints: average the members' probabilities (prob, the default) or their log-probs")
parser.add_argument("--output-path", default="predictions.json")
parser.add_argument("--evalai-submit", action="store_true", help="accepted for flag parity; EvalAI is a network service")
parser.add_argument("--infer-tensors", default="")
parser.add_argument("--synthetic", type=int, default=0)
parser.add_argument("--vocab-size", type=int, default=10000)
parser.add_argument("--num-boxes", type=int, default=36)
parser.add_argument("--images-per-call", type=int, default=100)
parser.add_argument("--sentiment", type=float, default=None, help="override the per-image sentiment (-1, 0, 1)")
parser.add_argument("--constraints-json", default="",
                    help='constrained beam search: {"<image_id>": ["dog", "fire hydrant", ...]} - up to DATA.CBS.MAX_GIVEN_CONSTRAINTS '
                         "constraint classes per image (what the reference's EvaluationDatasetWithConstraints derives from detector "
                         "boxes, updown-baseline/updown/data/datasets.py:470-620); needs --wordforms-tsv")
parser.add_argument("--wordforms-tsv", default="", help="class name <TAB> comma separated word forms (data/constraint_wordforms*.tsv)")
parser.add_argument("--boxes-json", default="",
                    help='instead of --constraints-json: raw detections {"<image_id>": {"boxes": [[x1, y1, x2, y2], ...], "class_names": [...], '
                         '"scores": [...]}}, filtered to constraints by ssc_runtime.constraints.ConstraintFilter '
                         "(updown-baseline/updown/utils/constraints.py:56-209); needs --hierarchy-json and --wordforms-tsv")
parser.add_argument("--hierarchy-json", default="", help="Open Images class hierarchy (bbox_labels_600_hierarchy_readable.json)")
parser.add_argument("--references", default="",
                    help="score the decoded captions on the device right after decoding (ssc_runtime.evaluation, as scripts/evaluate.py "
                         'prints): COCO annotations {"annotations": [{"image_id", "caption"}]} or {image_id: [captions]}')
parser.add_argument("--style-wordforms", default="", help="with --references: wordforms TSV of the style words (senti_prec / senti_rec)")
parser.add_argument("--set-diversity", action="store_true",
                    help="with --references: also compare each image's captions with each other (mBLEU-1..4, Self-CIDEr, unique)")
parser.add_argument("--consensus-bank", default="",
                    help="consensus re-ranking: a bank of training images (scripts/build_consensus_bank.py); every image's captions are "
                         "ranked by their mean CIDEr-D against the captions of its nearest bank images, no test reference involved")
parser.add_argument("--consensus-k", type=int, default=60, help="with --consensus-bank: nearest bank images per decoded image")
parser.add_argument("--consensus-output", default="",
                    help='with --consensus-bank: write the picked caption of every image here ([{"image_id", "caption"}, ...])')
parser.add_argument("--select-k", type=int, default=0,
                    help="keep K captions per image that are good and different from each other (ssc_runtime.evaluation.select_captions "
                         "on the caption kernel of the image's decoded captions); needs --select-output")
parser.add_argument("--select-method", default="dpp", choices=["dpp", "mmr", "mbr"],
                    help="greedy DPP MAP (quality x diversity), maximal marginal relevance, or minimum Bayes risk under the caption kernel")
parser.add_argument("--select-quality", default="consensus", choices=["consensus", "logprob"],
                    help="the per-caption quality: the consensus scores (needs --consensus-bank) or the captions' log-probs under the "
                         "model (the groups' own with MODEL.DIVERSE_BEAM_SEARCH, else the marginal of ssc_runtime.inference.score_captions "
                         "over max(1, --likelihood-samples) latent samples, which draws from the run's random stream); the kernel's document frequencies are the bank's, or "
                         "without a bank those of --references")
parser.add_argument("--select-lambda", type=float, default=0.5, help="mmr: weight of the quality against the similarity to a pick")
parser.add_argument("--select-theta", type=float, default=1.0, help="dpp: weight of the quality")
parser.add_argument("--select-output", default="",
                    help='with --select-k: write the K captions per image here, in pick order ([{"image_id", "caption"}, ...])')
parser.add_argument("--likelihood-samples", type=int, default=0,
                    help="likelihood re-ranking: score every image's decoded captions under M FRESH latent samples "
                         "(ssc_runtime.inference.score_captions: log p(caption | image) ~ log mean_m p(caption | z^m, image)) and pick "
                         "the likeliest - the model's own best-1, no reference involved; needs --likelihood-output")
parser.add_argument("--likelihood-output", default="",
                    help='with --likelihood-samples: per image {"image_id", "caption" (highest marginal), "caption_per_token" (highest '
                         'marginal / n_tokens), "pick", "pick_per_token", "marginal": [...], "n_tokens": [...]}')
parser.add_argument("--attention-output", default="",
                    help="write the attention trace of every written caption to this .pt file (torch.save): a list, in the order of "
                         'the predictions, of {"image_id", "sample", "tokens", "top_region", "top_weight", "entropy"} - one entry per '
                         "word up to and including the caption's end: the region the word attended most, the weight there and the "
                         "entropy of its attention in nats.  The predictions file is what it is without the flag")
parser.add_argument("--attention-full", action="store_true",
                    help='with --attention-output: every entry also holds "maps" (words, regions), the whole attention of every word')
parser.add_argument("--exemplar-tensors", default="",
                    help="latent-guided decoding: a .pt file (torch.save) {\"image_id\": [...], \"captions\": (N, L) int64, 0-padded} with "
                         "ONE exemplar caption per image.  Each is encoded on that image's own features by the posterior branch and the "
                         "image's captions are decoded under the exemplar's latent path instead of the prior (beam search, constrained "
                         "or not, and word sampling).  The predictions file has its usual layout")
parser.add_argument("--exemplar-jitter", type=float, default=None,
                    help="with --exemplar-tensors: sample AROUND the exemplar's path - standard deviation J times the posterior's "
                         "(default 0: every latent sample of an image decodes the path itself)")
parser.add_argument("--word-bias", default="",
                    help='logit bias for word sampling: a JSON file {word: bias} - the bias is added to that word\'s raw logit at every '
                         'step of every image, in front of the draw ("-inf" bans the word; a word outside the vocabulary is an error). '
                         "Needs MODEL.DECODE_SAMPLER multinomial / top-k / top-p without SAMPLED_BEAM_SEARCH; composes with the "
                         "MODEL.SAMPLER_* logit rules")
parser.add_argument("--truncation", default="",
                    help="truncation for word sampling: KIND[:VALUE] with KIND typical | min-p | eta | epsilon, e.g. --truncation "
                         "typical:0.9 (default: MODEL.SAMPLER_TRUNCATION / SAMPLER_TRUNCATION_VALUE) - every step's distribution is cut "
                         "between the logit rules and the draw.  Needs MODEL.DECODE_SAMPLER multinomial / top-k / top-p without "
                         "SAMPLED_BEAM_SEARCH")
parser.add_argument("--mirostat", default="",
                    help="Mirostat 2.0 for word sampling: TAU[:ETA], the surprise target in bits and the learning rate, e.g. --mirostat "
                         "3:0.1 (default: MODEL.SAMPLER_MIROSTAT_TAU / SAMPLER_MIROSTAT_ETA; TAU 0 = off) - words more surprising than a "
                         "running threshold are cut behind the truncation, and the threshold follows the drawn words' surprise.  Needs "
                         "MODEL.DECODE_SAMPLER multinomial / top-k / top-p without SAMPLED_BEAM_SEARCH")
parser.add_argument("--mirostat-output", default="",
                    help="with an active Mirostat: write per returned caption the threshold mu and the drawn word's surprise at every "
                         "word, in bits (JSON: image_id, caption, mu, surprise)")
parser.add_argument("--arithmetic", action="store_true",
                    help="arithmetic sampling for word sampling (default: MODEL.SAMPLER_ARITHMETIC): every word is drawn by inverse CDF "
                         "along a code point per caption, the codes of an image a randomly shifted lattice - the captions of an image "
                         "are stratified instead of independent.  Needs MODEL.DECODE_SAMPLER multinomial / top-k / top-p without "
                         "SAMPLED_BEAM_SEARCH")
parser.add_argument("--arithmetic-share-latent", action="store_true",
                    help="with arithmetic sampling: the latent samples of an image share the noise of its first one, so its captions "
                         "differ by their codes alone (default: MODEL.SAMPLER_ARITHMETIC_SHARE_LATENT)")
parser.add_argument("--contrast", default="",
                    help="contrastive decoding for word sampling: ALPHA[:BETA], e.g. --contrast 1:0.1 (default: MODEL.CONTRAST_ALPHA / "
                         "CONTRAST_BETA; ALPHA 0 = off) - an amateur stream is decoded in lock-step and every step's logits become "
                         "lp + ALPHA (lp - lp_amateur) on the words at least BETA times as probable as the top word.  Needs "
                         "MODEL.DECODE_SAMPLER multinomial / top-k / top-p without SAMPLED_BEAM_SEARCH")
parser.add_argument("--contrast-amateur", default="",
                    help="the amateur of --contrast: mean-features | noise-features | prior-mean | neutral-sentiment (default: "
                         "MODEL.CONTRAST_AMATEUR)")
parser.add_argument("--contrast-checkpoint", default="",
                    help="the amateur's weights: a checkpoint of the SAME configuration and vocabulary (e.g. an early one); with it the "
                         "amateur kind applies only where --contrast-amateur is given")
parser.add_argument("--contrast-output", default="",
                    help="with an active contrast: write per returned caption the KL of the expert's word distribution from the "
                         "amateur's at every word, in nats (JSON: image_id, caption, divergence)")
parser.add_argument("--prefix", default="",
                    help='prompted decoding: words every caption starts with, e.g. --prefix "a happy" - one prompt for every image '
                         "(default: MODEL.DECODE_PREFIX).  The prompt is teacher-forced, the configured decoder continues from it; "
                         "constraints, rules and DATA.MAX_CAPTION_LENGTH apply to the continuation.  A word outside the vocabulary "
                         "is an error")
parser.add_argument("--prefix-json", default="",
                    help='prompted decoding with a prompt per image: a JSON file {image_id: "words"}.  Images without an entry get no '
                         "prompt; prompts of different lengths share one call")


class _LocalGlove(UpDownCaptioner):
    """Frozen embedding table comes from the checkpoint; no GloVe download at construction time."""

    def _initialize_glove(self):
        return torch.zeros(self._vocabulary.get_vocab_size(), self.embedding_size)


def check_ensemble_args(_A):
    """The ensemble flags, checked before anything is loaded -> (weights or None, mode) for CaptionerEnsemble."""
    if not _A.ensemble_checkpoints:
        if _A.ensemble_weights is not None or _A.ensemble_mode is not None:
            raise SystemExit("--ensemble-weights / --ensemble-mode need --ensemble-checkpoints")
        return None, "prob"
    if not _A.checkpoint_path:
        raise SystemExit("--ensemble-checkpoints needs --checkpoint-path (member 0)")
    n = 1 + len(_A.ensemble_checkpoints)
    if n > 8:
        raise SystemExit(f"--ensemble-checkpoints: at most 8 members in all, got {n}")
    for p in [_A.checkpoint_path] + _A.ensemble_checkpoints:
        if not os.path.isfile(p):
            raise SystemExit(f"--ensemble-checkpoints: no such checkpoint {p!r}")
    w = _A.ensemble_weights
    if w is not None and (len(w) != n or any(not math.isfinite(x) or x <= 0 for x in w)):
        raise SystemExit(f"--ensemble-weights: {n} positive finite weights wanted (member 0 first), got {w}")
    for flag, what in (("attention_output", "--attention-output"), ("likelihood_samples", "--likelihood-samples")):
        if getattr(_A, flag):
            raise SystemExit(f"{what} is not available with --ensemble-checkpoints: an ensemble runs the beam search only")
    return w, _A.ensemble_mode or "prob"


def check_exemplar_args(_A):
    """The exemplar flags, checked before anything is loaded -> the jitter (0.0 without --exemplar-jitter)."""
    if not _A.exemplar_tensors:
        if _A.exemplar_jitter is not None:
            raise SystemExit("--exemplar-jitter needs --exemplar-tensors")
        return 0.0
    if not os.path.isfile(_A.exemplar_tensors):
        raise SystemExit(f"--exemplar-tensors: no such file {_A.exemplar_tensors!r}")
    j = 0.0 if _A.exemplar_jitter is None else _A.exemplar_jitter
    if not math.isfinite(j) or j < 0:
        raise SystemExit(f"--exemplar-jitter: a finite standard-deviation factor >= 0 wanted, got {j}")
    if _A.ensemble_checkpoints:
        raise SystemExit("--exemplar-tensors is not available with --ensemble-checkpoints: latent guides steer a single model")
    return j


def check_word_bias_args(_A, model_cfg=None):
    """--word-bias, checked before anything is loaded; with model_cfg (the MODEL node) also that the run samples words."""
    if not _A.word_bias:
        return
    if not os.path.isfile(_A.word_bias):
        raise SystemExit(f"--word-bias: no such file {_A.word_bias!r}")
    if _A.ensemble_checkpoints:
        raise SystemExit("--word-bias is not available with --ensemble-checkpoints: an ensemble runs the beam search only")
    if model_cfg is not None:
        kind = str(model_cfg.DECODE_SAMPLER).strip().lower()
        if kind not in sampling.KINDS or model_cfg.SAMPLED_BEAM_SEARCH or model_cfg.STOCHASTIC_BEAM_SEARCH:
            raise SystemExit("--word-bias needs a word sampler: MODEL.DECODE_SAMPLER 'multinomial', 'top-k' or 'top-p' without "
                             f"MODEL.SAMPLED_BEAM_SEARCH / STOCHASTIC_BEAM_SEARCH, got {model_cfg.DECODE_SAMPLER!r}")


def check_truncation_args(_A, model_cfg=None):
    """--truncation KIND[:VALUE], checked before anything is loaded -> its sampling.Truncation, or None without the flag; with
    model_cfg (the MODEL node) also that the run samples words."""
    if not _A.truncation:
        return None
    name, _, value = _A.truncation.partition(":")
    try:
        tr = sampling.truncation_from_name(name, float(value) if value.strip() else None)
    except ValueError as e:
        raise SystemExit(f"--truncation: {e}")
    if tr is None:
        return None
    if _A.ensemble_checkpoints:
        raise SystemExit("--truncation is not available with --ensemble-checkpoints: an ensemble runs the beam search only")
    if model_cfg is not None:
        kind = str(model_cfg.DECODE_SAMPLER).strip().lower()
        if kind not in sampling.KINDS or model_cfg.SAMPLED_BEAM_SEARCH or model_cfg.STOCHASTIC_BEAM_SEARCH:
            raise SystemExit("--truncation needs a word sampler: MODEL.DECODE_SAMPLER 'multinomial', 'top-k' or 'top-p' without "
                             f"MODEL.SAMPLED_BEAM_SEARCH / STOCHASTIC_BEAM_SEARCH, got {model_cfg.DECODE_SAMPLER!r}")
    return tr


def check_mirostat_args(_A, model_cfg=None):
    """--mirostat TAU[:ETA] / --mirostat-output, checked before anything is loaded -> its sampling.Mirostat, or None without the flag
    (or with TAU 0); with model_cfg (the MODEL node) the keys stand in for a missing flag and it is checked that the run samples
    words."""
    m = None
    if _A.mirostat:
        t, _, e = _A.mirostat.partition(":")
        try:
            tau, eta = float(t), (float(e) if e.strip() else None)
        except ValueError:
            raise SystemExit(f"--mirostat: TAU[:ETA] wanted, two numbers, got {_A.mirostat!r}")
        if eta is None:
            eta = float(model_cfg.SAMPLER_MIROSTAT_ETA) if model_cfg is not None else 0.1
        try:
            m = sampling.Mirostat(tau, eta)
        except ValueError as err:
            raise SystemExit(f"--mirostat: {err}")
    elif model_cfg is not None and float(model_cfg.SAMPLER_MIROSTAT_TAU) != 0:
        m = sampling.Mirostat(float(model_cfg.SAMPLER_MIROSTAT_TAU), float(model_cfg.SAMPLER_MIROSTAT_ETA))
    if m is not None and not m.active:
        m = None
    if m is None:
        if _A.mirostat_output and (model_cfg is not None or _A.mirostat):
            raise SystemExit("--mirostat-output needs an active Mirostat: --mirostat TAU[:ETA] or MODEL.SAMPLER_MIROSTAT_TAU")
        return None
    if _A.ensemble_checkpoints:
        raise SystemExit("--mirostat is not available with --ensemble-checkpoints: an ensemble runs the beam search only")
    if model_cfg is not None:
        kind = str(model_cfg.DECODE_SAMPLER).strip().lower()
        if kind not in sampling.KINDS or model_cfg.SAMPLED_BEAM_SEARCH or model_cfg.STOCHASTIC_BEAM_SEARCH:
            raise SystemExit("--mirostat needs a word sampler: MODEL.DECODE_SAMPLER 'multinomial', 'top-k' or 'top-p' without "
                             f"MODEL.SAMPLED_BEAM_SEARCH / STOCHASTIC_BEAM_SEARCH, got {model_cfg.DECODE_SAMPLER!r}")
    return m


def check_arithmetic_args(_A, model_cfg=None):
    """--arithmetic / --arithmetic-share-latent, checked before anything is loaded -> its sampling.Arithmetic, or None without the
    flag; with model_cfg (the MODEL node) the keys stand in for a missing flag and it is checked that the run samples words."""
    on = _A.arithmetic or (model_cfg is not None and bool(model_cfg.SAMPLER_ARITHMETIC))
    share = _A.arithmetic_share_latent or (model_cfg is not None and bool(model_cfg.SAMPLER_ARITHMETIC_SHARE_LATENT))
    if not on:
        if _A.arithmetic_share_latent and model_cfg is not None:   # (before the config is read the key may still turn it on)
            raise SystemExit("--arithmetic-share-latent needs arithmetic sampling: --arithmetic or MODEL.SAMPLER_ARITHMETIC")
        return None
    if _A.ensemble_checkpoints:
        raise SystemExit("--arithmetic is not available with --ensemble-checkpoints: an ensemble runs the beam search only")
    if model_cfg is not None:
        kind = str(model_cfg.DECODE_SAMPLER).strip().lower()
        if kind not in sampling.KINDS or model_cfg.SAMPLED_BEAM_SEARCH or model_cfg.STOCHASTIC_BEAM_SEARCH:
            raise SystemExit("--arithmetic needs a word sampler: MODEL.DECODE_SAMPLER 'multinomial', 'top-k' or 'top-p' without "
                             f"MODEL.SAMPLED_BEAM_SEARCH / STOCHASTIC_BEAM_SEARCH, got {model_cfg.DECODE_SAMPLER!r}")
    return sampling.Arithmetic("lattice", share_latent=bool(share))


def check_contrast_args(_A, model_cfg=None):
    """--contrast ALPHA[:BETA] / --contrast-amateur / --contrast-checkpoint / --contrast-output, checked before anything is loaded
    -> (alpha, beta, amateur kind or None) of the flags, None for what a flag does not give; with model_cfg (the MODEL node) the
    keys fill the gaps and the result is (alpha, beta, kind), or None when the contrast is off - and it is checked that the run
    samples words."""
    alpha = beta = None
    if _A.contrast:
        a, _, b = _A.contrast.partition(":")
        try:
            alpha, beta = float(a), (float(b) if b.strip() else None)
        except ValueError:
            raise SystemExit(f"--contrast: ALPHA[:BETA] wanted, two numbers, got {_A.contrast!r}")
        if not (0 <= alpha < float("inf")):
            raise SystemExit(f"--contrast: ALPHA must be finite and >= 0, got {alpha!r}")
        if beta is not None and not (0 <= beta < 1):
            raise SystemExit(f"--contrast: BETA must lie in [0, 1), got {beta!r}")
    kind = _A.contrast_amateur or None
    if kind is not None and kind not in AMATEURS:
        raise SystemExit(f"--contrast-amateur: one of {' | '.join(AMATEURS)} wanted, got {kind!r}")
    if _A.contrast_checkpoint and not os.path.exists(_A.contrast_checkpoint):
        raise SystemExit(f"--contrast-checkpoint: no such checkpoint {_A.contrast_checkpoint!r}")
    if model_cfg is None:
        return alpha, beta, kind
    alpha = float(model_cfg.CONTRAST_ALPHA) if alpha is None else alpha
    cut_alone = alpha == 0 and beta is not None and beta != 0   # (--contrast 0:BETA; ALPHA 0 is off whatever the keys' BETA)
    beta = float(model_cfg.CONTRAST_BETA) if beta is None else beta
    if alpha == 0 and not cut_alone:
        for flag, name in ((_A.contrast_amateur, "--contrast-amateur"), (_A.contrast_checkpoint, "--contrast-checkpoint"),
                           (_A.contrast_output, "--contrast-output")):
            if flag and not _A.contrast:
                raise SystemExit(f"{name} needs an active contrast: --contrast ALPHA[:BETA] or MODEL.CONTRAST_ALPHA")
        return None
    if _A.ensemble_checkpoints:
        raise SystemExit("--contrast is not available with --ensemble-checkpoints: an ensemble runs the beam search only")
    sk = str(model_cfg.DECODE_SAMPLER).strip().lower()
    if sk not in sampling.KINDS or model_cfg.SAMPLED_BEAM_SEARCH or model_cfg.STOCHASTIC_BEAM_SEARCH:
        raise SystemExit("--contrast needs a word sampler: MODEL.DECODE_SAMPLER 'multinomial', 'top-k' or 'top-p' without "
                         f"MODEL.SAMPLED_BEAM_SEARCH / STOCHASTIC_BEAM_SEARCH, got {model_cfg.DECODE_SAMPLER!r}")
    if kind is None and not _A.contrast_checkpoint:
        kind = str(model_cfg.CONTRAST_AMATEUR)
    return alpha, beta, kind


def check_prefix_args(_A):
    """--prefix / --prefix-json, checked before anything is loaded -> {image_id: "words"} of --prefix-json, or None."""
    if not _A.prefix and not _A.prefix_json:
        return None
    if _A.prefix and _A.prefix_json:
        raise SystemExit("--prefix and --prefix-json exclude each other")
    if _A.prefix and not _A.prefix.split():
        raise SystemExit("--prefix: at least one word wanted")
    for flag, what, why in (("ensemble_checkpoints", "--ensemble-checkpoints", "every member would need its own primed states"),
                            ("exemplar_tensors", "--exemplar-tensors", "a latent guide's steps are those of a caption decoded from "
                                                                        "@@BOUNDARY@@"),
                            ("attention_output", "--attention-output", "the trace would not cover the prefix words")):
        if getattr(_A, flag):
            raise SystemExit(f"--prefix / --prefix-json is not available with {what}: {why}")
    if not _A.prefix_json:
        return None
    if not os.path.isfile(_A.prefix_json):
        raise SystemExit(f"--prefix-json: no such file {_A.prefix_json!r}")
    try:
        blob = json.load(open(_A.prefix_json, encoding="utf-8"))
    except ValueError as e:
        raise SystemExit(f"--prefix-json: {_A.prefix_json!r} is not JSON ({e})")
    if not isinstance(blob, dict) or not blob or not all(isinstance(v, str) for v in blob.values()):
        raise SystemExit('--prefix-json: a non-empty JSON object {image_id: "words"} wanted')
    try:
        return {int(k): v for k, v in blob.items()}
    except ValueError:
        raise SystemExit("--prefix-json: the keys must be image ids (integers)")


def load_word_bias(path, vocabulary):
    """-> (V,) float32 bias row of a --word-bias file {word: bias}; "-inf" bans a word"""
    try:
        blob = json.load(open(path, encoding="utf-8"))
    except ValueError as e:
        raise SystemExit(f"--word-bias: {path!r} is not JSON ({e})")
    if not isinstance(blob, dict) or not blob:
        raise SystemExit('--word-bias: a non-empty JSON object {word: bias} wanted')
    row = torch.zeros(vocabulary.get_vocab_size(), dtype=torch.float32)
    boundary = vocabulary.get_token_index("@@BOUNDARY@@")
    for word, value in blob.items():
        idx = vocabulary.get_token_index(word)
        if vocabulary.get_token_from_index(idx) != word:   # (an unknown word maps to @@UNKNOWN@@)
            raise SystemExit(f"--word-bias: the word {word!r} is not in the vocabulary")
        try:
            v = float(value)
        except (TypeError, ValueError):
            raise SystemExit(f"--word-bias: the bias of {word!r} must be a number or \"-inf\", got {value!r}")
        if isinstance(value, bool) or v != v or v == float("inf"):
            raise SystemExit(f"--word-bias: the bias of {word!r} must be finite or \"-inf\", got {value!r}")
        if idx == boundary and v == float("-inf"):
            raise SystemExit("--word-bias: @@BOUNDARY@@ cannot be banned (no caption could end)")
        row[idx] = v
    return row


def load_exemplars(path, max_len):
    """-> {image_id: caption row (L,) int64} of an --exemplar-tensors file"""
    blob = torch.load(path, map_location="cpu", weights_only=True)
    if not isinstance(blob, dict) or "image_id" not in blob or "captions" not in blob:
        raise SystemExit('--exemplar-tensors: a dict {"image_id": [...], "captions": (N, L) int64} wanted')
    caps = torch.as_tensor(blob["captions"]).to(torch.int64)
    ids = [int(x) for x in blob["image_id"]]
    if caps.dim() != 2 or caps.size(0) != len(ids) or caps.size(1) < 1 or caps.size(1) > max_len:
        raise SystemExit(f"--exemplar-tensors: captions must be (N, L) with N = {len(ids)} image ids and 1 <= L <= DATA.MAX_CAPTION_LENGTH "
                         f"= {max_len}, got {tuple(caps.shape)}")
    return {i: caps[k] for k, i in enumerate(ids)}


def main():
    _A = parser.parse_args()
    prompts = check_prefix_args(_A)
    ens_weights, ens_mode = check_ensemble_args(_A)
    jitter = check_exemplar_args(_A)
    check_word_bias_args(_A)
    check_truncation_args(_A)
    check_contrast_args(_A)
    check_mirostat_args(_A)
    check_arithmetic_args(_A)
    _C = Config(_A.config, _A.config_override)
    check_word_bias_args(_A, _C.MODEL)
    truncation = check_truncation_args(_A, _C.MODEL)
    contrast_args = check_contrast_args(_A, _C.MODEL)
    mirostat = check_mirostat_args(_A, _C.MODEL)   # --mirostat, else MODEL.SAMPLER_MIROSTAT_TAU / SAMPLER_MIROSTAT_ETA
    arithmetic = check_arithmetic_args(_A, _C.MODEL)   # --arithmetic, else MODEL.SAMPLER_ARITHMETIC / SAMPLER_ARITHMETIC_SHARE_LATENT
    prompt = _A.prefix or ("" if prompts is not None else str(_C.MODEL.DECODE_PREFIX).strip())
    if (prompt or prompts is not None) and not _A.prefix and not _A.prefix_json:   # (MODEL.DECODE_PREFIX: the flags' refusals apply)
        _A.prefix = prompt
        check_prefix_args(_A)
    if (prompt or prompts is not None) and _C.MODEL.DECODE_ATTENTION != "none":
        raise SystemExit("--prefix / --prefix-json cannot be combined with MODEL.DECODE_ATTENTION: the trace would not cover the "
                         "prefix words")
    random.seed(_C.RANDOM_SEED)
    np.random.seed(_C.RANDOM_SEED)
    torch.manual_seed(_C.RANDOM_SEED)
    device = torch.device("cuda", _A.gpu_ids[0])
    torch.cuda.set_device(device)
    if _A.synthetic:
        vocabulary = Vocabulary.synthetic(_A.vocab_size)
        data = SyntheticCaptionData(_A.synthetic, _A.num_boxes, _C.MODEL.IMAGE_FEATURE_SIZE, _C.DATA.MAX_CAPTION_LENGTH,
                                    _A.vocab_size, seed=4321,
                                    obj_dim=_C.MODEL.Z_SPACE if (_C.MODEL.SENTIMENT_VAE == 2 and not _C.MODEL.SIMPLE_VAE) else 0)
    else:
        vocabulary = Vocabulary.from_files(_C.DATA.VOCABULARY)
        if not _A.infer_tensors:
            raise SystemExit("pass --infer-tensors file.pt or --synthetic N (h5 readers are out of scope)")
        data = TensorFileData(_A.infer_tensors)
    cls = _LocalGlove if (_C.MODEL.EMBEDDING_SIZE in (300, 600) and _A.checkpoint_path) else UpDownCaptioner
    extra = {"mean_choice": {}} if _C.MODEL.SENTIMENT_VAE == 2 else {}   # (per-region attribute MEANS come with the data: data.obj)
    sampler = sampling.from_config(_C.MODEL)   # MODEL.DECODE_SAMPLER / STOCHASTIC_BEAM_SEARCH: None = beam search
    sampled_beam = sampling.sampled_beam_from_config(_C.MODEL)   # MODEL.SAMPLED_BEAM_SEARCH: the word sampler at BEAM_SIZE
    diverse = sampling.diverse_beam_from_config(_C.MODEL)   # MODEL.DIVERSE_BEAM_SEARCH: groups of beams with a Hamming penalty
    # MODEL.NO_REPEAT_NGRAM / MIN_CAPTION_LENGTH / LENGTH_PENALTY_ALPHA / SUPPRESS_UNKNOWN: the beam search under decode rules
    rules = sampling.decode_rules_from_config(_C.MODEL, vocabulary)
    # MODEL.SAMPLER_NO_REPEAT_NGRAM / SAMPLER_MIN_LENGTH / ... and --word-bias: the logit rules of the word-sampled decode
    logit_rules = sampling.logit_rules_from_config(_C.MODEL, vocabulary)
    if _A.word_bias:
        kw = {} if logit_rules is None else dict(no_repeat_ngram=logit_rules.no_repeat_ngram, min_length=logit_rules.min_length,
                                                 suppress=logit_rules.suppress, repetition_penalty=logit_rules.repetition_penalty,
                                                 presence_penalty=logit_rules.presence_penalty,
                                                 frequency_penalty=logit_rules.frequency_penalty)
        logit_rules = sampling.LogitRules(bias=load_word_bias(_A.word_bias, vocabulary).to(device), **kw)
    # --truncation, else MODEL.SAMPLER_TRUNCATION / SAMPLER_TRUNCATION_VALUE: the cut of the word-sampled decode's distribution
    if not _A.truncation:
        truncation = sampling.truncation_from_config(_C.MODEL)
    # --prefix / --prefix-json / MODEL.DECODE_PREFIX: every image's prompt as word ids, padded to the longest (-1)
    prefix_ids = None
    if prompt or prompts is not None:
        from ssc_runtime.prefix import DecodePrefix
        try:
            per_image = [prompt if prompts is None else prompts.get(int(i), "") for i in data.image_id]
            prefix_ids = DecodePrefix.from_words(vocabulary, per_image).ids
        except ValueError as e:
            raise SystemExit(f"--prefix / --prefix-json: {e}")
    model = cls.from_config(_C, vocabulary=vocabulary, device=device, sampler=sampler, diverse_beam=diverse, **extra).to(device)
    if _A.checkpoint_path:
        model.load_state_dict(torch.load(_A.checkpoint_path, map_location=device, weights_only=True)["model"])
    model.eval()
    model._engine()
    dec = model._dec
    if _A.ensemble_checkpoints:
        if sampler is not None or diverse is not None or rules is not None or _C.MODEL.DECODE_ATTENTION != "none":
            raise SystemExit("--ensemble-checkpoints runs the beam search only: no MODEL.DECODE_SAMPLER / STOCHASTIC_BEAM_SEARCH / "
                             "DIVERSE_BEAM_SEARCH, no decode rules and no MODEL.DECODE_ATTENTION")
        members = [model]
        with torch.random.fork_rng(devices=[]):   # (the members' initialisation draws nothing from the run's random stream)
            for path in _A.ensemble_checkpoints:
                m = cls.from_config(_C, vocabulary=vocabulary, device=device, **extra).to(device)
                m.load_state_dict(torch.load(path, map_location=device, weights_only=True)["model"])
                members.append(m)
        dec = CaptionerEnsemble(members, ens_weights, ens_mode).engine()
    dec.weights_frozen = True   # the checkpoint's weights stay as they are for the whole run: weight-only tables are formed once
    # --contrast / MODEL.CONTRAST_*: the amateur of the word-sampled decode - a kind, the weights of --contrast-checkpoint, or both
    contrast = None
    model.contrast(None)   # (the run's own decode below is handed the contrast itself)
    if contrast_args is not None:
        from ssc_runtime.contrast import Contrast, contrast_from_name
        c_alpha, c_beta, c_kind = contrast_args
        amateur_engine = None
        if _A.contrast_checkpoint:
            with torch.random.fork_rng(devices=[]):   # (the amateur's initialisation draws nothing from the run's random stream)
                am = cls.from_config(_C, vocabulary=vocabulary, device=device, **extra).to(device)
                am.load_state_dict(torch.load(_A.contrast_checkpoint, map_location=device, weights_only=True)["model"])
            am.eval()
            am._engine()
            amateur_engine = am._dec
            amateur_engine.weights_frozen = True
        contrast = (contrast_from_name(c_alpha, c_beta, c_kind, float(_C.MODEL.CONTRAST_NOISE), engine=amateur_engine)
                    if c_kind is not None else Contrast(c_alpha, c_beta, engine=amateur_engine))
    divergences = []   # --contrast-output: one record per returned caption
    miro_traces = []   # --mirostat-output: one record per returned caption
    model.mirostat(None)   # (the run's own decode below is handed the Mirostat itself)
    model.arithmetic(None)
    n_z = max(1, _C.MODEL.N_Z_SAMPLES)
    beam = _C.MODEL.BEAM_SIZE
    if sampler is not None and (_A.constraints_json or _A.boxes_json):
        what = ("MODEL.STOCHASTIC_BEAM_SEARCH" if sampler.beam_search else "MODEL.SAMPLED_BEAM_SEARCH" if sampled_beam
                else f"MODEL.DECODE_SAMPLER {_C.MODEL.DECODE_SAMPLER!r}")
        raise SystemExit(f"{what} does not take constraints: constrained sampling is not supported")
    if diverse is not None and (_A.constraints_json or _A.boxes_json):
        raise SystemExit("MODEL.DIVERSE_BEAM_SEARCH does not take constraints")
    if rules is not None and (_A.constraints_json or _A.boxes_json):
        raise SystemExit("MODEL.NO_REPEAT_NGRAM / MIN_CAPTION_LENGTH / LENGTH_PENALTY_ALPHA / SUPPRESS_UNKNOWN do not take constraints")
    exemplars = None
    if _A.exemplar_tensors:
        if (sampler is not None and (sampler.beam_search or sampled_beam)) or diverse is not None or rules is not None:
            raise SystemExit("--exemplar-tensors steers the beam search (constrained or not) and word sampling: no "
                             "MODEL.STOCHASTIC_BEAM_SEARCH / SAMPLED_BEAM_SEARCH / DIVERSE_BEAM_SEARCH and no decode rules")
        if _C.MODEL.SENTIMENT_VAE == 2 and not _C.MODEL.SIMPLE_VAE:
            raise SystemExit("--exemplar-tensors is not available with MODEL.SENTIMENT_VAE 2")
        exemplars = load_exemplars(_A.exemplar_tensors, _C.DATA.MAX_CAPTION_LENGTH)
        V = vocabulary.get_vocab_size()
        for i, c in exemplars.items():
            if bool(((c < 0) | (c >= V)).any()) or int(c[0]) == 0:
                raise SystemExit(f"--exemplar-tensors: the caption of image {i} is empty or holds ids outside the vocabulary [0, {V})")
    boundary = vocabulary.get_token_index("@@BOUNDARY@@")
    predictions = []
    id2word = np.array([vocabulary.get_token_from_index(i) for i in range(vocabulary.get_vocab_size())], dtype=object)
    constraints, builder = {}, None
    per_call = _A.images_per_call
    if _A.constraints_json or _A.boxes_json:
        from ssc_runtime.constraints import ConstraintFilter, FiniteStateMachineBuilder
        if not _A.wordforms_tsv:
            raise SystemExit("--constraints-json / --boxes-json need --wordforms-tsv")
        kmax = max(1, _C.DATA.CBS.MAX_GIVEN_CONSTRAINTS)
        if _A.boxes_json:
            if not _A.hierarchy_json:
                raise SystemExit("--boxes-json needs --hierarchy-json")
            cfilter = ConstraintFilter(_A.hierarchy_json, _C.DATA.CBS.NMS_THRESHOLD, kmax)
            constraints = {int(k): sorted(cfilter(np.asarray(v["boxes"], dtype=np.float32).reshape(-1, 4), v["class_names"],
                                                  np.asarray(v["scores"], dtype=np.float32)))
                           for k, v in json.load(open(_A.boxes_json)).items()}
        else:
            constraints = {int(k): v for k, v in json.load(open(_A.constraints_json)).items()}
        builder = FiniteStateMachineBuilder(vocabulary, _A.wordforms_tsv, None, max_given_constraints=kmax,
                                            max_words_per_constraint=_C.DATA.CBS.MAX_WORDS_PER_CONSTRAINT)
        # (one machine per IMAGE, shared by its N_Z samples and compiled on the device - ssc_fsm_compile -: a call is sized by its rows)
    chunks = []   # (image ids, predictions on the device) of every chunk, for --references
    bank, consensus, best = None, [], []
    if _A.consensus_bank:
        from ssc_runtime.evaluation import ConsensusBank, ConsensusResult, pool_features
        bank = ConsensusBank.load(_A.consensus_bank, device=device)
    elif _A.consensus_output:
        raise SystemExit("--consensus-output needs --consensus-bank")
    if bool(_A.select_k > 0) != bool(_A.select_output) or _A.select_k < 0:
        raise SystemExit("--select-k K (K >= 1) and --select-output FILE go together")
    select_refs, selections, selected = None, [], []
    if _A.select_k:
        if _A.select_quality == "consensus" and bank is None:
            raise SystemExit("--select-quality consensus needs --consensus-bank")
        if bank is None:
            if not _A.references:
                raise SystemExit("--select-k needs --consensus-bank or --references (the document frequencies of the caption kernel)")
            from ssc_runtime.evaluation import CaptionReferences, load_references
            select_refs = CaptionReferences(load_references(_A.references), device=device)
    if bool(_A.likelihood_samples > 0) != bool(_A.likelihood_output) or _A.likelihood_samples < 0:
        raise SystemExit("--likelihood-samples M (M >= 1) and --likelihood-output FILE go together")
    likelihood, lik_pick, lik_pick_len = [], [], []
    if _A.attention_full and not _A.attention_output:
        raise SystemExit("--attention-full needs --attention-output")
    attn_mode = ("full" if _A.attention_full else "summary") if _A.attention_output else (
        None if _C.MODEL.DECODE_ATTENTION == "none" else _C.MODEL.DECODE_ATTENTION)
    if attn_mode and not _A.attention_output:
        raise SystemExit("MODEL.DECODE_ATTENTION needs --attention-output FILE to write the traces to")
    traces = []
    ROW_BUDGET = 40000   # rows (image, sample, state, beam) per decode step of a constrained call
    with torch.no_grad():
        lo = 0
        while lo < len(data):
            built = None
            n_here = min(per_call, len(data) - lo)
            if builder is not None:
                # one machine per image, padded to the chunk's largest state count: the states an image does not use have no
                # incoming transition and never hold a finite beam (their rows are skipped: diverse_decode(skip_dead=True));
                # the chunk ends where its rows per step would exceed the budget
                built, S = [], 0
                for i in range(n_here):
                    m = builder.build([c for c in constraints.get(int(data.image_id[lo + i]), [])][:kmax])
                    if built and (len(built) + 1) * n_z * max(S, m[1]) * beam > ROW_BUDGET:
                        break
                    built.append(m)
                    S = max(S, m[1])
                n_here = len(built)
            feats = data.feats[lo: lo + n_here].to(device)
            senti = data.senti[lo: lo + n_here, 0].to(device)
            if _A.sentiment is not None:
                senti = torch.full_like(senti, _A.sentiment)
            fsm = ncons = None
            if built is not None:
                V = vocabulary.get_vocab_size()
                fsm = torch.zeros(n_here, S, S, V, dtype=torch.uint8)
                for i, (m, ns, _) in enumerate(built):
                    fsm[i, :ns, :ns] = m[:ns, :ns]
                fsm = fsm.to(device)
                ncons = torch.tensor([len(constraints.get(int(data.image_id[lo + i]), [])[:kmax]) for i in range(n_here)]
                                     ).repeat_interleave(n_z)
            obj = data.obj[lo: lo + n_here, : feats.size(1)].to(device) if getattr(data, "obj", None) is not None else None
            guide = None
            if exemplars is not None:   # every image's exemplar, encoded on the image's own features: the path its samples decode
                from ssc_runtime.guide import LatentGuide, encode_captions
                here = [int(x) for x in data.image_id[lo: lo + n_here]]
                missing = [i for i in here if i not in exemplars]
                if missing:
                    raise SystemExit(f"--exemplar-tensors holds no caption for image {missing[0]} ({len(missing)} images of this call)")
                caps = torch.stack([exemplars[i] for i in here]).to(device)
                guide = LatentGuide.from_encoding(encode_captions(model._eng, feats, caps, senti), jitter=jitter, repeat=n_z)
            pkw = {}   # (a call without a prefix is made exactly as before)
            if prefix_ids is not None:
                from ssc_runtime.prefix import DecodePrefix
                pkw = {"prefix": DecodePrefix(prefix_ids[lo: lo + n_here])}
            if diverse is not None:   # every group's best caption: N_Z_SAMPLES * DIVERSE_BEAM_GROUPS captions per image
                out = diverse_decode(dec, feats, senti, n_z, beam, _C.DATA.MAX_CAPTION_LENGTH, boundary, obj_means=obj,
                                     diverse_beam=diverse, return_groups=True, attention=attn_mode, **pkw)
                pred = out[0]
                pred = pred.reshape(pred.size(0), n_z * diverse.groups, pred.size(-1))
            else:
                out = diverse_decode(dec, feats, senti, n_z, beam, _C.DATA.MAX_CAPTION_LENGTH, boundary, fsm=fsm,
                                     num_constraints=ncons, min_constraints_to_satisfy=_C.MODEL.MIN_CONSTRAINTS_TO_SATISFY,
                                     obj_means=obj, sampler=sampler, sampled_beam=sampled_beam, rules=rules, attention=attn_mode,
                                     guide=guide, **({"logit_rules": logit_rules} if logit_rules is not None else {}),
                                     **({"truncation": truncation} if truncation is not None else {}),
                                     **({"contrast": contrast, "contrast_stats": True} if contrast is not None else {}),
                                     **({"mirostat": mirostat, "mirostat_stats": bool(_A.mirostat_output)} if mirostat is not None else {}),
                                     **({"arithmetic": arithmetic} if arithmetic is not None else {}),
                                     **pkw)
                pred = out[0]
                if mirostat is not None and _A.mirostat_output:
                    out, (m_mu, m_sur) = out[:-1], (out[-1][0].cpu().numpy(), out[-1][1].cpu().numpy())   # (images, n_z, steps)
                if contrast is not None:
                    out, c_div = out[:-1], out[-1][1].cpu().numpy()   # (images, n_z, steps of the continuation)
            trace = out[-1] if attn_mode else None
            # ids -> words, cut at the first @@BOUNDARY@@ (inference.py:180-182): one table lookup for the whole chunk - the
            # per-token Python calls this replaces took as long as the chunk's 20 decode steps on the GPU
            if _A.references:
                chunks.append(([int(x) for x in data.image_id[lo: lo + n_here]], pred))
            ids = pred.cpu().numpy()                                   # (images, n_z, steps)
            words = id2word[ids]
            is_end = ids == boundary
            n_keep = np.where(is_end.any(-1), is_end.argmax(-1), ids.shape[-1])
            for i in range(ids.shape[0]):
                image_id = int(data.image_id[lo + i])
                for k in range(ids.shape[1]):
                    predictions.append({"image_id": image_id, "caption": " ".join(words[i, k, : n_keep[i, k]])})
                    if mirostat is not None and _A.mirostat_output and diverse is None:   # the caption's words and its END, less a prefix's
                        n_m = max(1, min(int(n_keep[i, k]) + 1 - (ids.shape[-1] - m_mu.shape[-1]), m_mu.shape[-1]))
                        miro_traces.append({"image_id": image_id, "caption": predictions[-1]["caption"],
                                            "mu": [float(v) for v in m_mu[i, k, :n_m]],
                                            "surprise": [float(v) for v in m_sur[i, k, :n_m]]})
                    if contrast is not None and _A.contrast_output:   # the caption's words and its END, less a prefix's words
                        n_div = max(1, min(int(n_keep[i, k]) + 1 - (ids.shape[-1] - c_div.shape[-1]), c_div.shape[-1]))
                        divergences.append({"image_id": image_id, "caption": predictions[-1]["caption"],
                                            "divergence": [float(v) for v in c_div[i, k, :n_div]]})
            if trace is not None:
                # (images, captions per image, steps[, R]) like the predictions; every caption cut behind its end
                tr = {n: getattr(trace, n).reshape(ids.shape[0], ids.shape[1], *getattr(trace, n).shape[-(2 if n == "maps" else 1):]).cpu()
                      for n in ("top_region", "top_weight", "entropy", "maps") if getattr(trace, n) is not None}
                for i in range(ids.shape[0]):
                    for k in range(ids.shape[1]):
                        n = min(int(n_keep[i, k]) + 1, ids.shape[-1])
                        entry = {"image_id": int(data.image_id[lo + i]), "sample": k, "tokens": torch.from_numpy(ids[i, k, :n].copy())}
                        entry.update({name: v[i, k, :n].clone() for name, v in tr.items()})
                        traces.append(entry)
            if bank is not None:
                # an image that is itself in the bank is not its own neighbour
                here = [int(x) for x in data.image_id[lo: lo + n_here]]
                cons = bank.rerank(pred, boundary, vocabulary, pool_features(feats), k=_A.consensus_k, exclude_ids=here)
                consensus.append(cons)
                for i, image_id in enumerate(here):
                    k = int(cons.pick[i])
                    best.append({"image_id": image_id, "caption": " ".join(words[i, k, : n_keep[i, k]])})
            sc = None
            if _A.likelihood_samples:
                # each caption under M fresh latent samples, not under the one sample that produced it
                sc = score_captions(model._dec, feats, senti, pred, _A.likelihood_samples, boundary, "decoded", obj_means=obj)
                marg = sc.marginal.double().cpu().numpy()
                ntok = sc.n_tokens.cpu().numpy()
                for i in range(ids.shape[0]):
                    k, kl = int(marg[i].argmax()), int((marg[i] / np.maximum(ntok[i], 1)).argmax())
                    lik_pick.append(k)
                    lik_pick_len.append(kl)
                    likelihood.append({"image_id": int(data.image_id[lo + i]), "caption": " ".join(words[i, k, : n_keep[i, k]]),
                                       "caption_per_token": " ".join(words[i, kl, : n_keep[i, kl]]), "pick": k, "pick_per_token": kl,
                                       "marginal": [float(x) for x in marg[i]], "n_tokens": [int(x) for x in ntok[i]]})
            if _A.select_k:
                here = [int(x) for x in data.image_id[lo: lo + n_here]]
                logprob = None
                if _A.select_quality == "logprob":
                    if diverse is not None:
                        logprob = out[2].reshape(pred.size(0), pred.size(1))
                    else:
                        if sc is None:
                            sc = score_captions(model._dec, feats, senti, pred, 1, boundary, "decoded", obj_means=obj)
                        logprob = sc.marginal
                kw = dict(quality=_A.select_quality, consensus=consensus[-1] if bank is not None else None, logprob=logprob,
                          k=min(_A.select_k, pred.size(1)), method=_A.select_method, lam=_A.select_lambda, theta=_A.select_theta)
                if bank is not None:
                    sel = bank.select(pred, boundary, vocabulary, **kw)
                else:
                    sel = select_refs.select(pred, boundary, vocabulary, image_ids=here, **kw)
                selections.append(sel)
                for i, image_id in enumerate(here):
                    selected += [{"image_id": image_id, "caption": " ".join(words[i, n, : n_keep[i, n]])} for n in sel.picks[i] if n >= 0]
            lo += n_here
    json.dump(predictions, open(_A.output_path, "w", encoding="utf-8"))
    if contrast is not None and _A.contrast_output:
        json.dump(divergences, open(_A.contrast_output, "w", encoding="utf-8"))
    if mirostat is not None and _A.mirostat_output:
        json.dump(miro_traces, open(_A.mirostat_output, "w", encoding="utf-8"))
    print(f"wrote {len(predictions)} captions to {_A.output_path}")
    if _A.attention_output:
        torch.save(traces, _A.attention_output)
        print(f"wrote {len(traces)} attention traces to {_A.attention_output}")
    if _A.consensus_output:
        json.dump(best, open(_A.consensus_output, "w", encoding="utf-8"))
        print(f"wrote {len(best)} consensus captions to {_A.consensus_output}")
    if _A.select_output:
        json.dump(selected, open(_A.select_output, "w", encoding="utf-8"))
        print(f"wrote {len(selected)} selected captions ({_A.select_method}, k = {_A.select_k}) to {_A.select_output}")
    if _A.likelihood_output:
        json.dump(likelihood, open(_A.likelihood_output, "w", encoding="utf-8"))
        print(f"wrote {len(likelihood)} likelihood picks to {_A.likelihood_output}")
    if _A.references:
        from ssc_runtime.evaluation import CaptionReferences, format_summary, load_references, style_words_from_tsv
        style = style_words_from_tsv(_A.style_wordforms) if _A.style_wordforms else None
        refs = CaptionReferences(load_references(_A.references), style_words=style, device=device)
        steps = max(p.size(-1) for _, p in chunks)
        pred = torch.cat([torch.nn.functional.pad(p, (0, steps - p.size(-1)), value=boundary) for _, p in chunks])
        result = refs.score(pred, boundary, vocabulary, image_ids=[i for ids, _ in chunks for i in ids],
                            set_diversity=_A.set_diversity, consensus=ConsensusResult.concat(consensus) if consensus else None)
        summ = result.summary()
        if selections:
            from ssc_runtime.evaluation import CaptionSelection
            summ.update(result.subset_summary(CaptionSelection.concat(selections), "select"))
        for line in format_summary(summ):
            print(line)
        if likelihood:   # best-1 by likelihood, next to the consensus lines: the pick by marginal and the pick by marginal per token
            for name, pick in (("likelihood", lik_pick), ("likelihood/len", lik_pick_len)):
                ps = result.pick_summary(pick, name)
                print(f"{name} B4: {np.round(ps[name + ' B4'] * 100.0, 2)}")
                print(f"{name} CIDEr: {np.round(ps[name + ' cider'] * 100.0, 2)}")
        if result.degenerate_sets:
            print(f"{result.degenerate_sets} image(s) whose captions hold no weighted n-gram: Self-CIDEr 0")


if __name__ == "__main__":
    main()
