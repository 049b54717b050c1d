"""Diverse-caption evaluation on the device: the reference's eval/eval.py (oracle and mean BLEU-1..4, ROUGE-L, CIDEr-D over N
latent samples per image, Div-1 / Div-2 over all and over the top 5 captions by CIDEr, style precision / recall) with the
coco-caption scorers it calls, minus METEOR.  Per-candidate scores and per-image counts come from ONE library call
(ssc_eval_score, csrc/caption_eval.hip) on the decode's int64 prediction tensor as it lies on the device; the O(images x samples)
reductions (argmax, corpus BLEU sums, means) run here in float64.

    refs = CaptionReferences({image_id: [caption, ...]}, style_words=style_words_from_tsv(tsv))
    result = refs.score(predictions, boundary_index, vocabulary)        # (images, N, steps) int64 from diverse_decode
    result = refs.score_captions(json.load(open("predictions.json")))   # the JSON scripts/inference.py writes
    print("\\n".join(format_summary(result.summary())))

Caption-SET diversity (the N captions of an image against each other: mBLEU-1..4, Self-CIDEr, the share of distinct captions) is
one more library call (ssc_eval_set) on the same tensor, asked for with set_diversity=True; set_diversity(predictions, ...)
gives mBLEU and Unique with no references at all.

Consensus re-ranking (the papers' "best-1 after consensus re-ranking": the pick uses no test reference) needs a bank of training
images - pooled features and captions:

    bank = ConsensusBank.load("bank.pt")                                 # scripts/build_consensus_bank.py writes it
    cons = bank.rerank(predictions, boundary_index, vocabulary, pooled_queries, k=60, exclude_ids=image_ids)
    best = cons.pick                                                     # one sample index per image
    result = refs.score(predictions, boundary_index, vocabulary, consensus=cons)   # adds the "consensus ..." numbers

Diverse subset selection (the k captions of an image to show: good AND different from each other, chosen with no test reference)
is one more library call (ssc_eval_select: MBR, MMR or the greedy MAP of a DPP) on the caption kernel and a quality per candidate:

    sel = bank.select(predictions, boundary_index, vocabulary, quality="consensus", consensus=cons, k=5, method="dpp")
    kept = sel.gather(predictions, boundary_index)                       # (images, k, steps), in pick order
    summary = {**result.summary(), **result.subset_summary(sel, "select")}
"""
import ctypes
import json
from collections import OrderedDict
from typing import Any, Callable, Dict, Iterable, List, Optional, Sequence

import numpy as np
import torch

from . import lib as L
from .constraints import read_wordforms
from .vocab_builder import caption_words, simple_tokenize

MAX_TOKENS = 64     # per reference and per candidate (caption_eval.hip EV_L)
MAX_SAMPLES = 128   # per image (EV_MAX_N)
MAX_WORDS = 65535   # compact reference words, and candidate ids
UNKNOWN = "@@UNKNOWN@@"
TINY, SMALL = 1e-15, 1e-9


def _norm_id(k):
    """JSON object keys are strings: "123" and 123 name the same image."""
    if isinstance(k, str) and k.lstrip("-").isdigit():
        return int(k)
    return k


def style_words_from_tsv(path: str) -> set:
    """Every word form of a wordforms TSV (eval.py: senti_words = every item of every class's comma-separated list)."""
    return set(w for forms in read_wordforms(path).values() for w in forms)


def load_references(path_or_obj, tokenize: Callable[[str], List[str]] = simple_tokenize) -> "OrderedDict[Any, List[str]]":
    """COCO annotations {"annotations": [{"image_id", "caption"}, ...]} or {image_id: [caption, ...]} -> {image_id: [captions]}."""
    obj = json.load(open(path_or_obj)) if isinstance(path_or_obj, str) else path_or_obj
    out: "OrderedDict[Any, List[str]]" = OrderedDict()
    if isinstance(obj, dict) and "annotations" in obj:
        for a in obj["annotations"]:
            out.setdefault(_norm_id(a["image_id"]), []).append(a["caption"])
    elif isinstance(obj, dict):
        for k, v in obj.items():
            if not isinstance(v, list) or not all(isinstance(c, str) for c in v):
                raise ValueError(f"references: image {k!r} must map to a list of caption strings")
            out[_norm_id(k)] = list(v)
    else:
        raise ValueError('references: expected {"annotations": [...]} or {image_id: [captions]}')
    return out


def load_predictions(path_or_obj) -> "OrderedDict[Any, List[str]]":
    """[{"image_id", "caption"}, ...] (what scripts/inference.py writes) -> {image_id: [captions in file order]}."""
    obj = json.load(open(path_or_obj)) if isinstance(path_or_obj, str) else path_or_obj
    if not isinstance(obj, list):
        raise ValueError('predictions: expected a list of {"image_id", "caption"}')
    out: "OrderedDict[Any, List[str]]" = OrderedDict()
    for e in obj:
        out.setdefault(_norm_id(e["image_id"]), []).append(e["caption"])
    return out


def _samples_per_image(groups) -> int:
    ns = sorted(set(len(v) for v in groups))
    if len(ns) != 1:
        raise ValueError(f"every image needs the same number of captions N; found N in {ns}")
    return ns[0]


def corpus_bleu(testlen, reflen, guess, correct) -> List[float]:
    """BleuScorer.compute_score on summed statistics: BLEU-1..4."""
    out, b = [], 1.0
    for k in range(4):
        b *= float(correct[k] + TINY) / (guess[k] + SMALL)
        out.append(b ** (1.0 / (k + 1)))
    ratio = (testlen + TINY) / (reflen + SMALL)
    if ratio < 1:
        out = [x * np.exp(1 - 1 / ratio) for x in out]
    return [float(x) for x in out]


EIG_CUT = 1e-6   # eigenvalues of the Self-CIDEr kernel below EIG_CUT x the largest are taken as 0


def mbleu(set_stats) -> List[float]:
    """mBLEU-1..4 of set statistics (P, N, 10): corpus BLEU of the statistics summed over the images at sample index n, averaged
    over n (the reduction of `mean B{k}`).  Lower = more diverse."""
    st = np.asarray(set_stats, dtype=np.float64)
    per = [corpus_bleu(st[:, n, 0].sum(), st[:, n, 1].sum(), st[:, n, 2:6].sum(0), st[:, n, 6:10].sum(0)) for n in range(st.shape[1])]
    return [float(np.mean([b[k] for b in per])) for k in range(4)]


def self_cider(eigenvalues):
    """Self-CIDEr of one image from the eigenvalues of its caption kernel matrix: -log(sqrt(l_1) / sum sqrt(l_i)) / log N with the
    eigenvalues below EIG_CUT l_1 set to 0.  Returns (value, degenerate): l_1 <= 0 (no caption has a weighted n-gram) gives 0."""
    lam = np.sort(np.asarray(eigenvalues, dtype=np.float64))[::-1]
    top = lam[0]
    if not top > 0.0:
        return 0.0, True
    root = np.sqrt(np.where(lam < EIG_CUT * top, 0.0, lam))
    return float(-np.log(root[0] / root.sum()) / np.log(len(lam))), False


class SetDiversity:
    """What ssc_eval_set wrote: set_stats (P, N, 10) int - BleuScorer's statistics of every caption against the other N - 1 of
    its image -, distinct (P,) distinct captions per image, and for the images with references set_kernel (P, N, N) and
    set_eigenvalues (P, N) descending (both 0 elsewhere)."""

    def __init__(self, set_stats, distinct, kernel=None, eigenvalues=None, scored_rows=()):
        self.set_stats, self.distinct, self.set_kernel, self.set_eigenvalues = set_stats, distinct, kernel, eigenvalues
        self.scored_rows = list(scored_rows)
        vals = [self_cider(eigenvalues[p]) for p in self.scored_rows]
        self.self_cider_values = np.array([v for v, _ in vals], dtype=np.float64)
        self.degenerate_sets = int(sum(d for _, d in vals))

    def summary(self) -> Dict[str, float]:
        s = {f"mBLEU-{k + 1}": v for k, v in enumerate(mbleu(self.set_stats))}
        if self.scored_rows:
            s["self-cider"] = float(np.mean(self.self_cider_values))
        s["unique"] = float(np.mean(self.distinct / float(self.set_stats.shape[1])))
        return s


def _eval_set_call(pred: torch.Tensor, boundary_index: int, vocab_size: int, prep, id_map, ref_image, keep_kernel=True):
    """One ssc_eval_set call on (P, N, steps) int64 predictions on the device; prep None: no references (mBLEU / Unique only).
    -> (set_counts, distinct, kernel or None, eigenvalues, ref_image) on the device."""
    P, N, steps = pred.shape
    if not 2 <= N <= MAX_SAMPLES:
        raise ValueError(f"set diversity needs 2..{MAX_SAMPLES} captions per image, got N = {N}")
    if not 1 <= vocab_size <= MAX_WORDS:
        raise ValueError(f"{vocab_size} prediction ids: 1..{MAX_WORDS} are supported")
    dev = pred.device
    scored = prep is not None
    counts = torch.empty(P, N, 10, dtype=torch.int32, device=dev)
    kern = torch.empty(P, N, N, dtype=torch.float64, device=dev) if scored and keep_kernel else None
    eig = torch.empty(P, N, dtype=torch.float64, device=dev)
    dist = torch.empty(P, dtype=torch.int32, device=dev)
    if ref_image is None:
        ref_image = torch.full((P,), -1, dtype=torch.int32, device=dev)
    d = L.EvalSetDesc(L.ptr(pred), P, N, steps, int(boundary_index), int(vocab_size), L.ptr(id_map), L.ptr(ref_image), L.ptr(counts),
                      L.ptr(kern), L.ptr(eig), L.ptr(dist))
    lib = L.load()
    rp = ctypes.byref(prep.desc) if scored else None
    nbytes = lib.ssc_eval_set_workspace_bytes(rp, ctypes.byref(d))
    if nbytes == 0:
        raise ValueError(f"set diversity: arguments out of range ({P} images x {N} samples x {steps} steps)")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        lib.ssc_eval_set(rp, ctypes.byref(d), L.ptr(ws), ws.numel(), L.stream_ptr())
    return counts, dist, kern, eig, ref_image


def _eval_set(pred: torch.Tensor, boundary_index: int, vocab_size: int, prep, id_map, ref_image, keep_kernel=True) -> SetDiversity:
    """_eval_set_call with its outputs copied to the host."""
    scored = prep is not None
    counts, dist, kern, eig, ref_image = _eval_set_call(pred, boundary_index, vocab_size, prep, id_map, ref_image, keep_kernel)
    rows = [p for p, i in enumerate(ref_image.cpu().tolist()) if i >= 0] if scored else []
    return SetDiversity(counts.cpu().numpy().astype(np.int64), dist.cpu().numpy().astype(np.int64),
                        kern.cpu().numpy() if kern is not None else None, eig.cpu().numpy() if scored else None, rows)


def set_diversity(predictions: torch.Tensor, boundary_index: int, vocab_size: int) -> SetDiversity:
    """mBLEU-1..4 and Unique of (images, N, steps) int64 predictions on the device, ids 0..vocab_size-1, with no references:
    set_diversity(pred, boundary, V).summary().  Self-CIDEr needs document frequencies: CaptionReferences.score(...,
    set_diversity=True)."""
    if predictions.dim() != 3 or predictions.dtype != torch.int64:
        raise ValueError(f"predictions must be (images, N, steps) int64, got {tuple(predictions.shape)} {predictions.dtype}")
    if not predictions.is_cuda:
        raise ValueError("predictions must lie on the device")
    return _eval_set(predictions.contiguous(), boundary_index, vocab_size, None, None, None)


# ---- diverse subset selection ---------------------------------------------------------------------------------------------------

SELECT_METHODS = {"mbr": 1, "mmr": 2, "dpp": 3}


class CaptionSelection:
    """What ssc_eval_select chose for P images: picks (P, k) int64 candidate indices in pick order (-1: fewer than k candidates
    were eligible), gains (P, k) float64 the rule's value of every pick when it was made (0 for fallback picks and -1 slots),
    n_primary (P,) the picks the rule itself made before the fallback by quality filled up; method, k."""

    def __init__(self, picks, gains, n_primary, method: str):
        self.picks, self.gains, self.n_primary, self.method = picks, gains, n_primary, method
        self.k = int(picks.shape[1])

    def gather(self, predictions: torch.Tensor, boundary_index: int = 0) -> torch.Tensor:
        """(P, N, steps) predictions -> (P, k, steps) the picked rows in pick order, on the predictions' device; a -1 slot becomes an
        empty caption (a row of boundary_index)."""
        if predictions.dim() != 3 or predictions.size(0) != self.picks.shape[0]:
            raise ValueError(f"predictions must be ({self.picks.shape[0]}, N, steps), got {tuple(predictions.shape)}")
        idx = torch.from_numpy(np.ascontiguousarray(self.picks)).to(predictions.device)
        if int(idx.max()) >= predictions.size(1):
            raise ValueError(f"a pick names candidate {int(idx.max())} of {predictions.size(1)}")
        rows = predictions.gather(1, idx.clamp(min=0).unsqueeze(-1).expand(-1, -1, predictions.size(2)))
        return torch.where((idx < 0).unsqueeze(-1), torch.full_like(rows, int(boundary_index)), rows)

    def captions(self, groups) -> "OrderedDict[Any, List[str]]":
        """{image_id: [N captions]} in the selection's image order -> {image_id: [the picked captions in pick order]}."""
        if len(groups) != self.picks.shape[0]:
            raise ValueError(f"{len(groups)} images for a selection over {self.picks.shape[0]}")
        return OrderedDict((iid, [caps[int(n)] for n in row if n >= 0]) for (iid, caps), row in zip(groups.items(), self.picks))

    @staticmethod
    def concat(parts: Sequence["CaptionSelection"]) -> "CaptionSelection":
        """The selections of several calls (the same method and k) as one, in call order."""
        cat = lambda name: np.concatenate([getattr(r, name) for r in parts])   # noqa: E731
        return CaptionSelection(cat("picks"), cat("gains"), cat("n_primary"), parts[0].method)


def select_captions(kernel, quality=None, k: int = 5, method: str = "dpp", lam: float = 0.5, theta: float = 1.0,
                    min_gain: float = 1e-10, normalize: bool = True, eligible=None) -> CaptionSelection:
    """From the N candidates of every image the k that are good and different from each other (one ssc_eval_select call).
    kernel (P, N, N) float64 on the device: the caption similarity ssc_eval_set leaves (SetDiversity.set_kernel, or what
    CaptionReferences.select / ConsensusBank.select build themselves).  quality (P, N): consensus scores, caption log-probs, ...;
    None for "mbr", and for "dpp" with theta = 0.  method: "mbr" - the candidates closest to all others; "mmr" - lam x quality
    against (1 - lam) x the largest similarity to a pick; "dpp" - the greedy MAP of the DPP exp(theta q^_i) K_ij exp(theta q^_j),
    which stops at gains below min_gain (duplicates of a pick) and fills the rest by quality.  normalize: the rules see every
    image's quality scaled to [0, 1].  eligible (P, N): 0 / False = never pick (an empty or filtered caption)."""
    if method not in SELECT_METHODS:
        raise ValueError(f"method {method!r}: one of {sorted(SELECT_METHODS)}")
    kern = torch.as_tensor(kernel)
    if kern.dim() != 3 or kern.size(1) != kern.size(2) or kern.dtype != torch.float64:
        raise ValueError(f"kernel must be (images, N, N) float64, got {tuple(kern.shape)} {kern.dtype}")
    P, N, _ = kern.shape
    if not 1 <= N <= MAX_SAMPLES or not 1 <= int(k) <= N:
        raise ValueError(f"k = {k} of N = {N} candidates: 1 <= k <= N <= {MAX_SAMPLES} is supported")
    if quality is None and (method == "mmr" or (method == "dpp" and theta != 0)):
        raise ValueError(f"method {method!r} needs a quality per candidate" + (" (or theta = 0)" if method == "dpp" else ""))
    for name, t in (("quality", quality), ("eligible", eligible)):
        if t is not None and tuple(torch.as_tensor(t).shape) != (P, N):
            raise ValueError(f"{name} must be ({P}, {N}), got {tuple(torch.as_tensor(t).shape)}")
    kern = (kern if kern.is_cuda else kern.cuda()).contiguous()
    dev = kern.device
    qual = elig = None
    if quality is not None:
        qual = torch.as_tensor(quality).to(device=dev, dtype=torch.float64).contiguous()
    if eligible is not None:
        elig = (torch.as_tensor(eligible).to(dev) != 0).to(torch.uint8).contiguous()
    k = int(k)
    picks = torch.empty(P, k, dtype=torch.int32, device=dev)
    gains = torch.empty(P, k, dtype=torch.float64, device=dev)
    nprim = torch.empty(P, dtype=torch.int32, device=dev)
    d = L.EvalSelectDesc(P, N, k, SELECT_METHODS[method], L.ptr(kern), L.ptr(qual), int(bool(normalize)), float(lam), float(theta),
                         float(min_gain), L.ptr(elig), L.ptr(picks), L.ptr(gains), L.ptr(nprim))
    lib = L.load()
    nbytes = lib.ssc_eval_select_workspace_bytes(ctypes.byref(d))
    if nbytes == 0:
        raise ValueError(f"selection: arguments out of range (lam = {lam}, theta = {theta}, min_gain = {min_gain}, {P} images)")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        lib.ssc_eval_select(ctypes.byref(d), L.ptr(ws), ws.numel(), L.stream_ptr())
    return CaptionSelection(picks.cpu().numpy().astype(np.int64), gains.cpu().numpy(), nprim.cpu().numpy().astype(np.int64), method)


def _select_quality(quality, consensus, logprob, P, N):
    """The (P, N) quality a select() call names: "consensus" - the ConsensusResult's scores; "logprob" - the given log-probs; a
    tensor - itself; None."""
    if isinstance(quality, str):
        if quality == "consensus":
            if not isinstance(consensus, ConsensusResult):
                raise ValueError('quality="consensus" needs consensus=ConsensusResult (ConsensusBank.rerank on the same predictions)')
            quality = consensus.scores
        elif quality == "logprob":
            if logprob is None:
                raise ValueError('quality="logprob" needs logprob=(images, N) caption log-probs')
            quality = logprob
        else:
            raise ValueError(f'quality {quality!r}: "consensus", "logprob", a tensor or None')
    if quality is not None and tuple(quality.shape) != (P, N):
        raise ValueError(f"quality holds {tuple(quality.shape)} values for ({P}, {N}) predictions")
    return quality


def _select_on_kernel(pred, boundary_index, vocab_size, prep, id_map, ref_image, quality, eligible, kw) -> CaptionSelection:
    """The caption kernel of (P, N, steps) predictions on the device (ssc_eval_set) and the selection on it; empty captions are not
    eligible.  N = 1: the kernel is not needed (the one candidate, if it is not empty).  prep None (no image has references): the
    zero kernel every image without references gets."""
    P, N, _ = pred.shape
    if N >= 2 and prep is not None:
        kern = _eval_set_call(pred, boundary_index, vocab_size, prep, id_map, ref_image)[2]
    elif N >= 2:
        kern = torch.zeros(P, N, N, dtype=torch.float64, device=pred.device)
    else:
        kern = torch.ones(P, 1, 1, dtype=torch.float64, device=pred.device)
    elig = pred[:, :, 0] != int(boundary_index)
    if eligible is not None:
        elig = elig & (torch.as_tensor(eligible).to(pred.device) != 0)
    return select_captions(kern, quality, eligible=elig, **kw)


class EvalResult:
    """Per-candidate scores of the evaluated images (those with predictions and references, in prediction order) and the
    per-image counts, with eval.py's reductions.
      image_ids (I,); bleu (I, N, 4); rouge, cider (I, N); stats (I, N, 10) int: testlen, reflen, guess[4], correct[4]
      oracle: {"B1".."B4", "rouge", "cider"} -> (I,) best sample per image (argmax: lowest index on a tie)
      top5 (I, 5): samples by CIDEr, stable descending
      empty_images: prediction images whose N captions are all empty (their Div-n is 0; eval.py divides by zero there).
    With set_diversity=True also (None otherwise): set_stats (P, N, 10) and distinct (P,) over ALL prediction images, set_kernel
    (P, N, N) and set_eigenvalues (P, N) (0 for images without references), self_cider_values (I,) per evaluated image,
    degenerate_sets: evaluated images whose kernel matrix is 0 (Self-CIDEr 0)."""

    def __init__(self, image_ids, scores, stats, image_counts, eval_rows, top5, has_style, set_out: Optional[SetDiversity] = None,
                 consensus: Optional["ConsensusResult"] = None):
        self._set = set_out
        self._ctx = None   # (references, predictions on the device, boundary, words, image ids, unk): what subset_summary scores again
        # consensus_pick (I,): the consensus re-ranking's sample of every evaluated image (None without consensus=)
        self.consensus_pick = np.asarray(consensus.pick, dtype=np.int64)[eval_rows] if consensus is not None else None
        self.set_stats = set_out.set_stats if set_out else None
        self.set_kernel = set_out.set_kernel if set_out else None
        self.set_eigenvalues = set_out.set_eigenvalues if set_out else None
        self.distinct = set_out.distinct if set_out else None
        self.self_cider_values = set_out.self_cider_values if set_out else None
        self.degenerate_sets = set_out.degenerate_sets if set_out else None
        self.image_ids = [image_ids[p] for p in eval_rows]
        self.eval_rows = np.asarray(eval_rows, dtype=np.int64)   # rows of the predictions that were evaluated (have references)
        self.bleu = scores[eval_rows, :, :4]
        self.rouge = scores[eval_rows, :, 4]
        self.cider = scores[eval_rows, :, 5]
        self.stats = stats[eval_rows]
        self.top5 = top5[eval_rows]
        self.div_counts = image_counts[:, :3]                     # (P, 3): all prediction images
        self._top5_counts = image_counts[eval_rows, 3:6]
        self.style_counts = image_counts[eval_rows, 6:9] if has_style else None
        self.oracle = {f"B{k + 1}": np.argmax(self.bleu[:, :, k], axis=1) for k in range(4)}
        self.oracle["rouge"] = np.argmax(self.rouge, axis=1)
        self.oracle["cider"] = np.argmax(self.cider, axis=1)
        self.empty_images = int((self.div_counts[:, 2] == 0).sum())

    @staticmethod
    def _div(distinct, words):
        return float(np.mean(np.where(words > 0, distinct / np.maximum(words, 1), 0.0)))

    def summary(self) -> Dict[str, float]:
        s = {}
        dc = self.div_counts
        s["Div-1"] = self._div(dc[:, 0], dc[:, 2])
        s["Div-2"] = self._div(dc[:, 1], dc[:, 2])
        st = self.stats.astype(np.float64)
        I, N = self.cider.shape
        rows = np.arange(I)
        for k in range(4):
            sel = st[rows, self.oracle[f"B{k + 1}"]]
            s[f"B{k + 1}"] = corpus_bleu(sel[:, 0].sum(), sel[:, 1].sum(), sel[:, 2:6].sum(0), sel[:, 6:10].sum(0))[k]
        for k in range(4):
            s[f"mean B{k + 1}"] = float(np.mean([corpus_bleu(st[:, n, 0].sum(), st[:, n, 1].sum(), st[:, n, 2:6].sum(0),
                                                             st[:, n, 6:10].sum(0))[k] for n in range(N)]))
        s["rouge"] = float(np.mean(self.rouge.max(1)))
        s["mean rouge"] = float(np.mean(self.rouge.mean(0)))
        s["cider"] = float(np.mean(self.cider.max(1)))
        s["mean cider"] = float(np.mean(self.cider.mean(0)))
        # top 5: the per-image counts of the evaluated images
        t5 = self._top5_counts
        s["top5 Div-1"] = self._div(t5[:, 0], t5[:, 2])
        s["top5 Div-2"] = self._div(t5[:, 1], t5[:, 2])
        if self.style_counts is not None:
            c, m, r = (self.style_counts[:, j].sum() for j in range(3))
            s["senti_prec"] = float(m / c) if c else float("nan")
            s["senti_rec"] = float(m / r) if r else float("nan")
            s["has_anp"] = float(np.mean(self.style_counts[:, 0] > 0))
        if self._set is not None:
            s.update(self._set.summary())
        if self.consensus_pick is not None:
            pick = self.consensus_pick
            sel = st[rows, pick]
            for k, b in enumerate(corpus_bleu(sel[:, 0].sum(), sel[:, 1].sum(), sel[:, 2:6].sum(0), sel[:, 6:10].sum(0))):
                s[f"consensus B{k + 1}"] = b
            s["consensus rouge"] = float(np.mean(self.rouge[rows, pick]))
            s["consensus cider"] = float(np.mean(self.cider[rows, pick]))
            s["consensus agreement"] = float(np.mean(pick == self.oracle["cider"]))
        return s


    def pick_summary(self, pick, name: str) -> Dict[str, float]:
        """A best-1 choice made elsewhere (e.g. by likelihood, ssc_runtime.inference.score_captions), scored like the consensus
        pick: pick (P,) - one sample per PREDICTION image, in the order of the predictions - -> {"<name> B1".."<name> B4",
        "<name> rouge", "<name> cider", "<name> agreement"} over the evaluated images."""
        pick = np.asarray(pick, dtype=np.int64)[self.eval_rows]
        rows = np.arange(pick.shape[0])
        sel = self.stats.astype(np.float64)[rows, pick]
        s = {f"{name} B{k + 1}": b for k, b in enumerate(corpus_bleu(sel[:, 0].sum(), sel[:, 1].sum(), sel[:, 2:6].sum(0),
                                                                      sel[:, 6:10].sum(0)))}
        s[f"{name} rouge"] = float(np.mean(self.rouge[rows, pick]))
        s[f"{name} cider"] = float(np.mean(self.cider[rows, pick]))
        s[f"{name} agreement"] = float(np.mean(pick == self.oracle["cider"]))
        return s


    def subset_summary(self, selection: "CaptionSelection", name: str) -> Dict[str, float]:
        """The k captions per image a selection kept (select_captions, CaptionReferences.select, ConsensusBank.select on the SAME
        predictions), evaluated as a caption set of their own: the gathered (P, k, steps) predictions go through the score call and,
        for k >= 2, the set call again.  -> {"<name> subset Div-1", "... Div-2", "... distinct" (mean distinct captions per image),
        "... unique", "... mBLEU-1".."... mBLEU-4", "... self-cider", "... oracle cider", "... mean cider", "... oracle B4",
        "... mean B4"}; a -1 slot counts as an empty caption."""
        if self._ctx is None:
            raise ValueError("subset_summary needs a result of CaptionReferences.score / score_captions")
        refs, pred, boundary, words, image_ids, unk = self._ctx
        if selection.picks.shape[0] != pred.size(0):
            raise ValueError(f"the selection holds {selection.picks.shape[0]} images, the predictions {pred.size(0)}")
        sub = refs._score_ids(selection.gather(pred, boundary), boundary, words, image_ids, unk, set_diversity=selection.k >= 2,
                              _min_n=1)
        s = sub.summary()
        out = {f"{name} subset Div-1": s["Div-1"], f"{name} subset Div-2": s["Div-2"]}
        if sub.distinct is not None:
            out[f"{name} subset distinct"] = float(np.mean(sub.distinct))
            for key in ("unique", "mBLEU-1", "mBLEU-2", "mBLEU-3", "mBLEU-4", "self-cider"):
                if key in s:
                    out[f"{name} subset {key}"] = s[key]
        out[f"{name} subset oracle cider"], out[f"{name} subset mean cider"] = s["cider"], s["mean cider"]
        out[f"{name} subset oracle B4"], out[f"{name} subset mean B4"] = s["B4"], s["mean B4"]
        return out


def format_summary(s: Dict[str, float]) -> List[str]:
    """The lines eval.py prints: BLEU / ROUGE-L / CIDEr x 100 rounded to 2 decimals; METEOR is not computed."""
    out = [f"Div-1: {s['Div-1']}", f"Div-2: {s['Div-2']}"]
    for k in ("B1", "B2", "B3", "B4", "mean B1", "mean B2", "mean B3", "mean B4", "rouge", "mean rouge", "cider", "mean cider"):
        out.append(f"{k}: {np.round(s[k] * 100.0, 2)}")
    # best-1 after consensus re-ranking (consensus=): the picked caption of every image, scored like the oracle lines
    for k in ("consensus B1", "consensus B2", "consensus B3", "consensus B4", "consensus rouge", "consensus cider"):
        if k in s:
            out.append(f"{k}: {np.round(s[k] * 100.0, 2)}")
    if "consensus agreement" in s:
        out.append(f"consensus agreement: {np.round(s['consensus agreement'], 4)}")
    out.append("meteor: not computed (METEOR needs Java and WordNet)")
    out += [f"top5 Div-1: {s['top5 Div-1']}", f"top5 Div-2: {s['top5 Div-2']}"]
    if "senti_prec" in s:
        out.append(f"senti_prec: {s['senti_prec']} senti_rec: {s['senti_rec']} has_anp: {s['has_anp']}")
    # caption-set diversity (set_diversity=True): mBLEU x 100 as the BLEU lines; Self-CIDEr and Unique are shares in [0, 1]
    for k in ("mBLEU-1", "mBLEU-2", "mBLEU-3", "mBLEU-4"):
        if k in s:
            out.append(f"{k}: {np.round(s[k] * 100.0, 2)}")
    for k in ("self-cider", "unique"):
        if k in s:
            out.append(f"{k}: {np.round(s[k], 4)}")
    # a selected subset (EvalResult.subset_summary): BLEU / CIDEr / mBLEU x 100 as above, the shares and counts as they are
    for k in s:
        if " subset " in k:
            scaled = k.rsplit(" subset ", 1)[1] in ("mBLEU-1", "mBLEU-2", "mBLEU-3", "mBLEU-4", "oracle cider", "mean cider",
                                                    "oracle B4", "mean B4")
            out.append(f"{k}: {np.round(s[k] * 100.0, 2) if scaled else np.round(s[k], 4)}")
    return out


def _caption_ids(predictions):
    """Caption strings ([{"image_id", "caption"}, ...] or {image_id: [captions]}) -> ({image_id: [captions]}, (images, N, steps) int64
    ids with 0 after each caption, the words by id): captions split on whitespace, every word itself."""
    groups = load_predictions(predictions) if isinstance(predictions, (str, list)) else \
        OrderedDict((_norm_id(k), list(v)) for k, v in predictions.items())
    N = _samples_per_image(groups.values())
    toks = [[c.split() for c in caps] for caps in groups.values()]
    longest = max((len(t) for caps in toks for t in caps), default=0)
    if longest > MAX_TOKENS:
        raise ValueError(f"a caption has {longest} words: at most {MAX_TOKENS} are supported")
    words = [""] + sorted(set(w for caps in toks for t in caps for w in t))   # id 0: the end of a caption
    wid = {w: i for i, w in enumerate(words)}
    arr = np.zeros((len(toks), N, max(1, longest)), dtype=np.int64)
    for i, caps in enumerate(toks):
        for n, t in enumerate(caps):
            arr[i, n, :len(t)] = [wid[w] for w in t]
    return groups, arr, words


def _eval_score(prep: "_Prepared", pred: torch.Tensor, boundary_index: int, vocab_size: int, id_map, style, ref_image):
    """One ssc_eval_score call on device tensors: pred (P, N, steps) int64 contiguous, id_map (vocab_size) int32, style optional
    (vocab_size) uint8, ref_image (P) int32.  -> (scores (P, N, 6) fp64, counts (P, N, 10), image_counts (P, 9), top5 (P, 5)) on the
    device; nothing but the call's own error flag is read back."""
    P, N, steps = pred.shape
    dev = pred.device
    scores = torch.empty(P, N, 6, dtype=torch.float64, device=dev)
    counts = torch.empty(P, N, 10, dtype=torch.int32, device=dev)
    img = torch.empty(P, 9, dtype=torch.int32, device=dev)
    top5 = torch.empty(P, 5, dtype=torch.int32, device=dev)
    d = L.EvalScoreDesc(L.ptr(pred), P, N, steps, int(boundary_index), int(vocab_size), L.ptr(id_map), L.ptr(style), L.ptr(ref_image),
                        L.ptr(scores), L.ptr(counts), L.ptr(img), L.ptr(top5))
    lib = L.load()
    ws = torch.empty(lib.ssc_eval_score_workspace_bytes(ctypes.byref(prep.desc), ctypes.byref(d)), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        lib.ssc_eval_score(ctypes.byref(prep.desc), ctypes.byref(d), L.ptr(ws), ws.numel(), L.stream_ptr())
    return scores, counts, img, top5


class _Prepared:
    """The device state of one evaluated image set: its references as CSR arrays and what ssc_eval_prepare_refs wrote."""

    def __init__(self, refs: "CaptionReferences", ids: Sequence, device):
        ref_off, tok_off, toks = [0], [0], []
        for iid in ids:
            for r in refs.tokens[iid]:
                toks += [refs.word_id[w] for w in r]
                tok_off.append(len(toks))
            ref_off.append(len(tok_off) - 1)
        self.index = {iid: i for i, iid in enumerate(ids)}
        style = None
        if refs.style_words is not None:
            style = np.zeros(refs.W + 1, dtype=np.uint8)
            for w, c in refs.word_id.items():
                style[c] = w in refs.style_words
        self._prepare(ref_off, tok_off, toks, refs.W, style, device)

    @classmethod
    def from_csr(cls, ref_off, tok_off, toks, W: int, device) -> "_Prepared":
        """References given as compact ids 1..W in CSR form (image i holds references ref_off[i] .. ref_off[i + 1] - 1, reference r
        the tokens toks[tok_off[r] : tok_off[r + 1]]): no strings, no tokeniser."""
        self = cls.__new__(cls)
        self.index = {i: i for i in range(len(ref_off) - 1)}
        self._prepare(ref_off, tok_off, toks, W, None, device)
        return self

    def _prepare(self, ref_off, tok_off, toks, W, style, device):
        lib = L.load()
        self.I, self.nref, self.ntok = len(ref_off) - 1, len(tok_off) - 1, len(toks)
        self.ref_off = torch.as_tensor(np.asarray(ref_off, dtype=np.int32)).to(device)
        self.tok_off = torch.as_tensor(np.asarray(tok_off, dtype=np.int32)).to(device)
        self.toks = torch.as_tensor(np.asarray(toks, dtype=np.int32)).to(device)
        self.style = torch.from_numpy(style).to(device) if style is not None else None
        nbytes = lib.ssc_eval_refs_bytes(self.I, self.nref, self.ntok)
        if nbytes == 0:
            raise ValueError(f"reference set out of range: {self.I} images, {self.nref} captions, {self.ntok} tokens")
        self.state = torch.empty(nbytes, dtype=torch.uint8, device=device)
        self.desc = L.EvalRefs(self.I, self.nref, self.ntok, W, L.ptr(self.ref_off), L.ptr(self.tok_off), L.ptr(self.toks),
                               L.ptr(self.style), L.ptr(self.state), nbytes)
        with torch.cuda.device(device):
            lib.ssc_eval_prepare_refs(ctypes.byref(self.desc), L.stream_ptr())


class CaptionReferences:
    """Reference captions {image_id: [caption, ...]}, tokenised as the vocabulary builder does (lower case, `tokenize`,
    punctuation tokens dropped), prepared on the device once per evaluated image set and reused by every score call.
    style_words: the style word set (style_words_from_tsv) for senti_prec / senti_rec / has_anp; None leaves them out."""

    def __init__(self, references: Dict[Any, List[str]], tokenize: Callable[[str], List[str]] = simple_tokenize,
                 style_words: Optional[Iterable[str]] = None, device="cuda"):
        self.device = torch.device(device)
        self.image_ids = [_norm_id(k) for k in references]
        self.tokens: Dict[Any, List[List[str]]] = {}
        for k, caps in references.items():
            k = _norm_id(k)
            if not caps:
                raise ValueError(f"image {k!r} has no reference captions")
            toks = [caption_words(c, tokenize) for c in caps]
            for c, t in zip(caps, toks):
                if not 1 <= len(t) <= MAX_TOKENS:
                    raise ValueError(f"image {k!r}: reference {c!r} has {len(t)} tokens (1..{MAX_TOKENS} are supported)")
            self.tokens[k] = toks
        words = sorted(set(w for toks in self.tokens.values() for t in toks for w in t))
        if len(words) > MAX_WORDS:
            raise ValueError(f"{len(words)} distinct reference words: at most {MAX_WORDS} are supported")
        self.word_id = {w: i + 1 for i, w in enumerate(words)}
        self.W = max(1, len(words))
        self.style_words = set(style_words) if style_words is not None else None
        self._prepared: Dict[tuple, _Prepared] = {}

    def prepared(self, ids: Sequence) -> _Prepared:
        key = tuple(ids)
        if key not in self._prepared:
            self._prepared[key] = _Prepared(self, ids, self.device)
        return self._prepared[key]

    def _score_ids(self, pred: torch.Tensor, boundary_index: int, words: Sequence[str], image_ids: Sequence, unk: Optional[int],
                   set_diversity: bool = False, consensus: Optional["ConsensusResult"] = None, _min_n: int = 5):
        if pred.dim() != 3 or pred.dtype != torch.int64:
            raise ValueError(f"predictions must be (images, N, steps) int64, got {tuple(pred.shape)} {pred.dtype}")
        P, N, steps = pred.shape
        if len(image_ids) != P:
            raise ValueError(f"{len(image_ids)} image ids for {P} prediction images")
        if len(set(image_ids)) != P:
            raise ValueError("an image id occurs twice among the predictions")
        if N < _min_n:
            raise ValueError(f"top-5 Div-n needs at least 5 captions per image, got N = {N}")
        if N > MAX_SAMPLES:
            raise ValueError(f"N = {N} captions per image: at most {MAX_SAMPLES} are supported")
        if len(words) > MAX_WORDS:
            raise ValueError(f"{len(words)} prediction ids: at most {MAX_WORDS} are supported")
        if consensus is not None:
            if not isinstance(consensus, ConsensusResult):
                raise TypeError(f"consensus must be a ConsensusResult, got {type(consensus).__name__}")
            if tuple(consensus.scores.shape) != (P, N):
                raise ValueError(f"consensus holds {tuple(consensus.scores.shape)} scores for ({P}, {N}) predictions")
        ids = [i for i in image_ids if i in self.tokens]
        if not ids:
            raise ValueError("no prediction image has reference captions")
        prep = self.prepared(ids)
        dev = self.device
        id_map = np.array([self.word_id.get(w, 0) for w in words], dtype=np.int32)
        if unk is not None and 0 <= unk < len(words):
            id_map[unk] = 0   # the vocabulary's @@UNKNOWN@@ matches nothing
        style = None
        if self.style_words is not None:
            style = torch.from_numpy(np.array([w in self.style_words for w in words], dtype=np.uint8)).to(dev)
        id_map = torch.from_numpy(id_map).to(dev)
        ref_image = torch.tensor([prep.index.get(i, -1) for i in image_ids], dtype=torch.int32, device=dev)
        pred = pred.to(dev).contiguous()
        scores, counts, img, top5 = _eval_score(prep, pred, boundary_index, len(words), id_map, style, ref_image)
        rows = [p for p, i in enumerate(image_ids) if i in self.tokens]
        imgc = img.cpu().numpy().astype(np.int64)
        set_out = _eval_set(pred, boundary_index, len(words), prep, id_map, ref_image) if set_diversity else None
        res = EvalResult(list(image_ids), scores.cpu().numpy(), counts.cpu().numpy().astype(np.int64), imgc, rows,
                         top5.cpu().numpy().astype(np.int64), self.style_words is not None, set_out, consensus)
        res._ctx = (self, pred, boundary_index, list(words), list(image_ids), unk)
        return res

    def _select_ids(self, pred: torch.Tensor, boundary_index: int, words: Sequence[str], image_ids: Sequence, unk: Optional[int],
                    quality, consensus, logprob, eligible, kw) -> "CaptionSelection":
        if pred.dim() != 3 or pred.dtype != torch.int64:
            raise ValueError(f"predictions must be (images, N, steps) int64, got {tuple(pred.shape)} {pred.dtype}")
        P, N, _ = pred.shape
        if len(image_ids) != P:
            raise ValueError(f"{len(image_ids)} image ids for {P} prediction images")
        ids = [i for i in image_ids if i in self.tokens]
        prep = id_map = ref_image = None
        if ids:   # (a call whose images all lack references still selects: by the quality alone)
            prep = self.prepared(ids)
            id_map = np.array([self.word_id.get(w, 0) for w in words], dtype=np.int32)
            if unk is not None and 0 <= unk < len(words):
                id_map[unk] = 0   # the vocabulary's @@UNKNOWN@@ matches nothing
            id_map = torch.from_numpy(id_map).to(self.device)
            ref_image = torch.tensor([prep.index.get(i, -1) for i in image_ids], dtype=torch.int32, device=self.device)
        quality = _select_quality(quality, consensus, logprob, P, N)
        return _select_on_kernel(pred.to(self.device).contiguous(), boundary_index, len(words), prep, id_map, ref_image, quality,
                                 eligible, kw)

    def select(self, predictions: torch.Tensor, boundary_index: int, vocabulary, image_ids: Optional[Sequence] = None,
               quality="consensus", consensus: Optional["ConsensusResult"] = None, logprob=None, eligible=None,
               **kw) -> "CaptionSelection":
        """The k captions per image to keep: the caption kernel of the predictions (ssc_eval_set with these references' document
        frequencies - only the frequencies: no caption is compared with a reference) and select_captions on it, all on the device.
        predictions, boundary_index, vocabulary, image_ids: as for score(); an image without references has a zero kernel (a DPP
        then falls back to the quality order).  quality: "consensus" (the scores of consensus=, a ConsensusResult on the same
        predictions), "logprob" (logprob=, (images, N) caption log-probs), a (images, N) tensor, or None.  Empty captions are never
        picked; eligible (images, N) excludes more.  **kw: k, method, lam, theta, min_gain, normalize of select_captions."""
        if hasattr(vocabulary, "get_vocab_size"):
            words = [vocabulary.get_token_from_index(i) for i in range(vocabulary.get_vocab_size())]
        else:
            words = list(vocabulary)
        unk = words.index(UNKNOWN) if UNKNOWN in words else None
        ids = self.image_ids if image_ids is None else [_norm_id(i) for i in image_ids]
        return self._select_ids(predictions, boundary_index, words, ids, unk, quality, consensus, logprob, eligible, kw)


    def score(self, predictions: torch.Tensor, boundary_index: int, vocabulary, image_ids: Optional[Sequence] = None,
              set_diversity: bool = False, consensus: Optional["ConsensusResult"] = None) -> EvalResult:
        """predictions (images, N, steps) int64 on the device (diverse_decode's output); a row is cut at its first boundary_index.
        vocabulary: a Vocabulary (its @@UNKNOWN@@ matches nothing) or the list of words by id.  image_ids: one per prediction
        image (default: this object's images, in order); images without references count toward Div-1 / Div-2 only.
        set_diversity: also compare each image's N captions with each other (one ssc_eval_set call): mBLEU-1..4, Self-CIDEr and
        Unique in summary(); images without references count toward mBLEU and Unique only.
        consensus: the ConsensusResult of ConsensusBank.rerank on the same predictions: summary() then also holds the picked
        captions' corpus BLEU-1..4 (consensus B1..B4), mean ROUGE-L and CIDEr-D (consensus rouge / cider) and the share of images
        whose pick is the CIDEr oracle's (consensus agreement)."""
        if not isinstance(set_diversity, bool):
            raise TypeError(f"set_diversity must be a bool, got {type(set_diversity).__name__}")
        if hasattr(vocabulary, "get_vocab_size"):
            words = [vocabulary.get_token_from_index(i) for i in range(vocabulary.get_vocab_size())]
        else:
            words = list(vocabulary)
        unk = words.index(UNKNOWN) if UNKNOWN in words else None
        ids = self.image_ids if image_ids is None else [_norm_id(i) for i in image_ids]
        return self._score_ids(predictions, boundary_index, words, ids, unk, set_diversity, consensus)

    def score_captions(self, predictions, set_diversity: bool = False, consensus: Optional["ConsensusResult"] = None) -> EvalResult:
        """Caption strings: [{"image_id", "caption"}, ...] (N per image in file order, as eval.py reads them) or
        {image_id: [captions]}.  Captions are split on whitespace; every word is itself, including words no vocabulary holds.
        set_diversity, consensus: as for score() (consensus: of ConsensusBank.rerank_captions on the same captions)."""
        if not isinstance(set_diversity, bool):
            raise TypeError(f"set_diversity must be a bool, got {type(set_diversity).__name__}")
        groups, arr, words = _caption_ids(predictions)
        return self._score_ids(torch.from_numpy(arr).to(self.device), 0, words, list(groups), None, set_diversity, consensus)


# ---- consensus re-ranking -------------------------------------------------------------------------------------------------------

MAX_NEIGHBOURS = 128            # consensus.hip KNN_MAX_K
SIM_BUFFER_BYTES = 64 << 20     # the (queries x bank chunk) similarity buffer stays below this
MAX_CHUNK_ROWS = 1 << 22        # consensus.hip KNN_MAX_CHUNK


def pool_features(feats: torch.Tensor) -> torch.Tensor:
    """(B, R, F) region features on the device -> (B, F) masked means over the regions (ssc_feat_prep's avg: all-zero regions
    are padding), the rows a ConsensusBank holds and is queried with."""
    if feats.dim() != 3 or not feats.is_cuda:
        raise ValueError(f"features must be (images, regions, F) on the device, got {tuple(feats.shape)} on {feats.device}")
    feats = feats.contiguous().float()
    B, R, F = feats.shape
    mask = torch.empty(B, R, dtype=torch.float32, device=feats.device)
    avg = torch.empty(B, F, dtype=torch.float32, device=feats.device)
    with torch.cuda.device(feats.device):
        L.load().ssc_feat_prep(L.ptr(feats), B, R, F, L.ptr(mask), L.ptr(avg), L.stream_ptr())
    return avg


def pool_rows(data, rows: Sequence[int], device, batch: int = 256) -> torch.Tensor:
    """Pooled features (len(rows), F) float32 on the host of rows `rows` of a TensorFileData-like source (dense `feats` (N, R, F),
    or ragged: every batch zero-padded to its largest region count), pooled on the device batch by batch."""
    out = []
    for lo in range(0, len(rows), batch):
        sel = [int(r) for r in rows[lo: lo + batch]]
        if getattr(data, "ragged", None) is None:
            f = data.feats[sel]
        else:
            flat, nb, off = data.ragged
            f = torch.zeros(len(sel), max(1, int(nb[sel].max())), flat.size(1))
            for i, r in enumerate(sel):
                f[i, : int(nb[r])] = flat[int(off[r]): int(off[r + 1])]
        out.append(pool_features(f.to(device)).cpu())
    return torch.cat(out)


def _unit_rows(x: torch.Tensor, device) -> torch.Tensor:
    """(rows, F) -> (rows, F rounded up to 4) float32 unit rows on the device (zero rows stay zero, the added columns are zero: the
    product's operands are 16-byte aligned whatever F)."""
    x = torch.as_tensor(x)
    if x.dim() != 2 or x.size(0) < 1 or x.size(1) < 1:
        raise ValueError(f"pooled features must be (rows, F), got {tuple(x.shape)}")
    x = x.to(device=device, dtype=torch.float32).contiguous()
    rows, F = x.shape
    Fp = (F + 3) // 4 * 4
    out = torch.zeros(rows, Fp, dtype=torch.float32, device=device)
    with torch.cuda.device(device):
        L.load().ssc_l2_normalize_rows(L.ptr(x), rows, F, F, L.ptr(out), Fp, L.stream_ptr())
    return out


class ConsensusResult:
    """What ConsensusBank.rerank found for P query images of N candidates: scores (P, N) float64 - a candidate's mean CIDEr-D x 10
    against the pooled references of its image's neighbours -, pick (P,) the best sample (lowest index on a tie), order (P, N) the
    samples by score (stable descending), neighbours (P, k) bank rows (-1 = unused) with neighbour_sims (P, k) (None when the lists
    were given), pool_refs (P,) the pooled references per image."""

    def __init__(self, scores, pick, order, neighbours, pool_refs, neighbour_sims=None):
        self.scores, self.pick, self.order = scores, pick, order
        self.neighbours, self.pool_refs, self.neighbour_sims = neighbours, pool_refs, neighbour_sims

    @staticmethod
    def concat(parts: Sequence["ConsensusResult"]) -> "ConsensusResult":
        """The results of several calls (the same N and k) as one, in call order."""
        cat = lambda name: np.concatenate([getattr(r, name) for r in parts])   # noqa: E731
        sims = cat("neighbour_sims") if all(r.neighbour_sims is not None for r in parts) else None
        return ConsensusResult(cat("scores"), cat("pick"), cat("order"), cat("neighbours"), cat("pool_refs"), sims)


class ConsensusBank:
    """A bank of M training images for consensus re-ranking: pooled (M, F) features (masked means over regions: pool_features),
    one image id per row and every image's reference captions (a list of M caption lists, or {image_id: [captions]}).  Holds the
    unit-norm bank rows on the device and the captions as a CaptionReferences prepared over all M images, so CIDEr's document
    frequencies and log I are the bank's."""

    def __init__(self, pooled, image_ids: Sequence, references, device="cuda",
                 tokenize: Callable[[str], List[str]] = simple_tokenize):
        self.device = torch.device(device)
        self.pooled = torch.as_tensor(pooled).detach().to("cpu", torch.float32)
        ids = image_ids.tolist() if hasattr(image_ids, "tolist") else list(image_ids)
        self.image_ids = [_norm_id(i) for i in ids]
        M = len(self.image_ids)
        if self.pooled.dim() != 2 or self.pooled.size(0) != M or M < 1:
            raise ValueError(f"pooled must be (M, F) with one row per image id, got {tuple(self.pooled.shape)} for {M} ids")
        if len(set(self.image_ids)) != M:
            raise ValueError("an image id occurs twice in the bank")
        if isinstance(references, dict):
            references = {_norm_id(k): v for k, v in references.items()}
            missing = [i for i in self.image_ids if i not in references]
            if missing:
                raise ValueError(f"bank image {missing[0]!r} has no reference captions")
            caps = [list(references[i]) for i in self.image_ids]
        else:
            caps = [list(c) for c in references]
        if len(caps) != M:
            raise ValueError(f"{len(caps)} caption lists for {M} bank images")
        self.captions = caps
        self.index = {iid: j for j, iid in enumerate(self.image_ids)}
        self.F = self.pooled.size(1)
        self.bank = _unit_rows(self.pooled, self.device)
        self.references = CaptionReferences(OrderedDict(zip(self.image_ids, caps)), tokenize=tokenize, device=self.device)
        self.prep = self.references.prepared(self.image_ids)

    def __len__(self):
        return len(self.image_ids)

    # -- file: plain tensors, lists and strings only (torch.load(weights_only=True) reads it) --
    @staticmethod
    def write_file(path: str, pooled, image_ids: Sequence, captions: Sequence[Sequence[str]]) -> None:
        """The bank file: {"pooled": (M, F) float32, "image_id": (M,) int64 (a list of strings when an id is not an integer),
        "captions": M lists of strings}."""
        ids = image_ids.tolist() if hasattr(image_ids, "tolist") else list(image_ids)
        pooled = torch.as_tensor(pooled).detach().to("cpu", torch.float32).contiguous()
        caps = [[str(c) for c in cs] for cs in captions]
        if pooled.dim() != 2 or pooled.size(0) != len(ids) or len(caps) != len(ids):
            raise ValueError(f"bank file: {tuple(pooled.shape)} features, {len(ids)} ids, {len(caps)} caption lists")
        image_id = torch.tensor(ids, dtype=torch.int64) if all(isinstance(i, int) for i in ids) else [str(i) for i in ids]
        torch.save({"pooled": pooled, "image_id": image_id, "captions": caps}, path)

    @staticmethod
    def read_file(path: str):
        """-> (pooled (M, F) float32, image ids, captions) of a bank file, read with weights_only=True."""
        d = torch.load(path, map_location="cpu", weights_only=True)
        for k in ("pooled", "image_id", "captions"):
            if not isinstance(d, dict) or k not in d:
                raise ValueError(f"{path}: not a consensus bank (no {k!r})")
        ids = d["image_id"].tolist() if hasattr(d["image_id"], "tolist") else list(d["image_id"])
        return d["pooled"].float(), ids, d["captions"]

    def save(self, path: str) -> None:
        self.write_file(path, self.pooled, self.image_ids, self.captions)

    @classmethod
    def load(cls, path: str, device="cuda", tokenize: Callable[[str], List[str]] = simple_tokenize) -> "ConsensusBank":
        pooled, ids, caps = cls.read_file(path)
        return cls(pooled, ids, caps, device=device, tokenize=tokenize)

    # -- neighbours --
    def _exclude_rows(self, exclude_ids, Q):
        if exclude_ids is None:
            return None
        ex = exclude_ids.tolist() if hasattr(exclude_ids, "tolist") else list(exclude_ids)
        if len(ex) != Q:
            raise ValueError(f"{len(ex)} exclude ids for {Q} queries")
        return torch.tensor([self.index.get(_norm_id(i), -1) for i in ex], dtype=torch.int32, device=self.device)

    def neighbours(self, pooled_queries, k: int = 60, exclude_ids: Optional[Sequence] = None, chunk_rows: Optional[int] = None):
        """The k nearest bank rows of every query row by cosine similarity -> (idx (Q, k) int32, sim (Q, k) float32) on the device,
        similarity descending, ties to the lower bank row; slots past the bank's size hold (-1, -inf).  exclude_ids: one image id
        per query; a query whose id is in the bank skips that row.  The similarities are ssc_gemm NT products of the unit rows,
        one bank chunk at a time (chunk_rows: default the most that keeps the buffer below 64 MB), each merged by ssc_knn_merge."""
        if not 1 <= int(k) <= MAX_NEIGHBOURS:
            raise ValueError(f"k = {k}: 1..{MAX_NEIGHBOURS} neighbours are supported")
        k = int(k)
        q = torch.as_tensor(pooled_queries)
        if q.dim() != 2 or q.size(1) != self.F:
            raise ValueError(f"queries must be (Q, {self.F}), got {tuple(q.shape)}")
        q = _unit_rows(q, self.device)
        Q, Fp = q.shape
        M = len(self)
        excl = self._exclude_rows(exclude_ids, Q)
        cap = min(MAX_CHUNK_ROWS, max(4, SIM_BUFFER_BYTES // (4 * Q) // 4 * 4))
        rows = cap if chunk_rows is None else int(chunk_rows)
        if not 1 <= rows <= cap:
            raise ValueError(f"chunk_rows = {rows}: 1..{cap} rows fit the similarity buffer of {Q} queries")
        rows = min(rows, M)
        ld = (rows + 3) // 4 * 4
        sims = torch.empty(Q, ld, dtype=torch.float32, device=self.device)
        best_sim = torch.full((Q, k), float("-inf"), dtype=torch.float32, device=self.device)
        best_idx = torch.full((Q, k), -1, dtype=torch.int32, device=self.device)
        lib = L.load()
        d = L.GemmDesc()
        d.nseg, d.M, d.a_kc, d.b_kc, d.splits = 1, Q, 1, 1, 1   # one pass over K: an entry's value does not depend on the split count
        d.seg[0].A, d.seg[0].lda, d.seg[0].ldb, d.seg[0].K = q.data_ptr(), Fp, Fp, Fp
        d.C, d.ldc = sims.data_ptr(), ld
        with torch.cuda.device(self.device):
            st = L.stream_ptr()
            for off in range(0, M, rows):
                mc = min(rows, M - off)
                d.N = mc
                d.seg[0].B = self.bank.data_ptr() + 4 * off * Fp
                lib.ssc_gemm(ctypes.byref(d), st)
                lib.ssc_knn_merge(L.ptr(sims), ld, Q, mc, off, k, L.ptr(excl), L.ptr(best_sim), L.ptr(best_idx), st)
        return best_idx, best_sim

    # -- scores --
    def _words(self, vocabulary):
        if hasattr(vocabulary, "get_vocab_size"):
            return [vocabulary.get_token_from_index(i) for i in range(vocabulary.get_vocab_size())]
        return list(vocabulary)

    def _rerank_ids(self, pred, boundary_index, words, unk, pooled_queries, k, exclude_ids, neighbours) -> ConsensusResult:
        if pred.dim() != 3 or pred.dtype != torch.int64:
            raise ValueError(f"predictions must be (images, N, steps) int64, got {tuple(pred.shape)} {pred.dtype}")
        P, N, steps = pred.shape
        if not 1 <= N <= MAX_SAMPLES:
            raise ValueError(f"N = {N} captions per image: 1..{MAX_SAMPLES} are supported")
        if not 1 <= len(words) <= MAX_WORDS:
            raise ValueError(f"{len(words)} prediction ids: 1..{MAX_WORDS} are supported")
        dev = self.device
        sims = None
        if neighbours is None:
            if pooled_queries is None:
                raise ValueError("rerank needs pooled_queries or neighbours")
            nb, sims = self.neighbours(pooled_queries, k, exclude_ids)
        else:
            nb = torch.as_tensor(neighbours).to(device=dev, dtype=torch.int32).contiguous()
        if nb.dim() != 2 or nb.size(0) != P or not 1 <= nb.size(1) <= MAX_NEIGHBOURS:
            raise ValueError(f"neighbours must be ({P}, 1..{MAX_NEIGHBOURS}), got {tuple(nb.shape)}")
        refs = self.references
        id_map = np.array([refs.word_id.get(w, 0) for w in words], dtype=np.int32)
        if unk is not None and 0 <= unk < len(words):
            id_map[unk] = 0   # the vocabulary's @@UNKNOWN@@ matches nothing
        id_map = torch.from_numpy(id_map).to(dev)
        pred = pred.to(dev).contiguous()
        scores = torch.empty(P, N, dtype=torch.float64, device=dev)
        pool = torch.empty(P, dtype=torch.int32, device=dev)
        pick = torch.empty(P, dtype=torch.int32, device=dev)
        order = torch.empty(P, N, dtype=torch.int32, device=dev)
        d = L.EvalConsensusDesc(L.ptr(pred), P, N, steps, int(boundary_index), len(words), L.ptr(id_map), L.ptr(nb), nb.size(1),
                                L.ptr(scores), L.ptr(pool), L.ptr(pick), L.ptr(order))
        lib = L.load()
        nbytes = lib.ssc_eval_consensus_workspace_bytes(ctypes.byref(self.prep.desc), ctypes.byref(d))
        if nbytes == 0:
            raise ValueError(f"consensus: arguments out of range ({P} images x {N} samples x {steps} steps, k = {nb.size(1)})")
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            lib.ssc_eval_consensus(ctypes.byref(self.prep.desc), ctypes.byref(d), L.ptr(ws), ws.numel(), L.stream_ptr())
        i64 = lambda t: t.cpu().numpy().astype(np.int64)   # noqa: E731
        return ConsensusResult(scores.cpu().numpy(), i64(pick), i64(order), i64(nb), i64(pool),
                               sims.cpu().numpy() if sims is not None else None)

    def rerank(self, predictions: torch.Tensor, boundary_index: int, vocabulary, pooled_queries=None, k: int = 60,
               exclude_ids: Optional[Sequence] = None, neighbours=None) -> ConsensusResult:
        """Consensus re-ranking of (images, N, steps) int64 predictions (a row is cut at its first boundary_index): the k nearest
        bank images of every image by its pooled features (P, F), then every candidate's mean CIDEr-D against those images'
        captions.  vocabulary: as CaptionReferences.score.  exclude_ids: one image id per prediction image - an image that is
        itself in the bank is not its own neighbour.  neighbours (P, k') int, bank rows or -1: use these lists instead of a search."""
        words = self._words(vocabulary)
        unk = words.index(UNKNOWN) if UNKNOWN in words else None
        return self._rerank_ids(predictions, boundary_index, words, unk, pooled_queries, k, exclude_ids, neighbours)

    def _select_ids(self, pred, boundary_index, words, unk, quality, consensus, logprob, eligible, kw) -> "CaptionSelection":
        if pred.dim() != 3 or pred.dtype != torch.int64:
            raise ValueError(f"predictions must be (images, N, steps) int64, got {tuple(pred.shape)} {pred.dtype}")
        P, N, _ = pred.shape
        refs = self.references
        id_map = np.array([refs.word_id.get(w, 0) for w in words], dtype=np.int32)
        if unk is not None and 0 <= unk < len(words):
            id_map[unk] = 0   # the vocabulary's @@UNKNOWN@@ matches nothing
        id_map = torch.from_numpy(id_map).to(self.device)
        # (any prepared image: the kernel reads the set's document frequencies and log I, not the image's references)
        ref_image = torch.zeros(P, dtype=torch.int32, device=self.device)
        quality = _select_quality(quality, consensus, logprob, P, N)
        return _select_on_kernel(pred.to(self.device).contiguous(), boundary_index, len(words), self.prep, id_map, ref_image,
                                 quality, eligible, kw)

    def select(self, predictions: torch.Tensor, boundary_index: int, vocabulary, quality="consensus",
               consensus: Optional[ConsensusResult] = None, logprob=None, eligible=None, **kw) -> "CaptionSelection":
        """CaptionReferences.select with the BANK's document frequencies: the k captions per image to keep, chosen with no test
        reference at all.  quality="consensus": the scores of consensus= (this bank's rerank on the same predictions)."""
        words = self._words(vocabulary)
        unk = words.index(UNKNOWN) if UNKNOWN in words else None
        return self._select_ids(predictions, boundary_index, words, unk, quality, consensus, logprob, eligible, kw)

    def select_captions(self, predictions, quality="consensus", consensus: Optional[ConsensusResult] = None, logprob=None,
                        eligible=None, **kw) -> "CaptionSelection":
        """select() for caption strings, read as rerank_captions reads them."""
        _, arr, words = _caption_ids(predictions)
        return self._select_ids(torch.from_numpy(arr).to(self.device), 0, words, None, quality, consensus, logprob, eligible, kw)

    def rerank_captions(self, predictions, pooled_queries=None, k: int = 60, exclude_ids: Optional[Sequence] = None,
                        neighbours=None) -> ConsensusResult:
        """The same for caption strings ([{"image_id", "caption"}, ...] or {image_id: [captions]}, as CaptionReferences.score_captions
        reads them); pooled_queries: one row per image, in the captions' image order."""
        _, arr, words = _caption_ids(predictions)
        return self._rerank_ids(torch.from_numpy(arr).to(self.device), 0, words, None, pooled_queries, k, exclude_ids, neighbours)
