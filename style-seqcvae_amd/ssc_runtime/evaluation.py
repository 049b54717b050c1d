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


def _eval_set(pred: torch.Tensor, boundary_index: int, vocab_size: int, prep, id_map, ref_image, keep_kernel=True) -> SetDiversity:
    """One ssc_eval_set call on (P, N, steps) int64 predictions on the device; prep None: no references (mBLEU / Unique only)."""
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

    def __init__(self, image_ids, scores, stats, image_counts, eval_rows, top5, has_style, set_out: Optional[SetDiversity] = None):
        self._set = set_out
        self.set_stats = set_out.set_stats if set_out else None
        self.set_kernel = set_out.set_kernel if set_out else None
        self.set_eigenvalues = set_out.set_eigenvalues if set_out else None
        self.distinct = set_out.distinct if set_out else None
        self.self_cider_values = set_out.self_cider_values if set_out else None
        self.degenerate_sets = set_out.degenerate_sets if set_out else None
        self.image_ids = [image_ids[p] for p in eval_rows]
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
        return s


def format_summary(s: Dict[str, float]) -> List[str]:
    """The lines eval.py prints: BLEU / ROUGE-L / CIDEr x 100 rounded to 2 decimals; METEOR is not computed."""
    out = [f"Div-1: {s['Div-1']}", f"Div-2: {s['Div-2']}"]
    for k in ("B1", "B2", "B3", "B4", "mean B1", "mean B2", "mean B3", "mean B4", "rouge", "mean rouge", "cider", "mean cider"):
        out.append(f"{k}: {np.round(s[k] * 100.0, 2)}")
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
    return out


class _Prepared:
    """The device state of one evaluated image set: its references as CSR arrays and what ssc_eval_prepare_refs wrote."""

    def __init__(self, refs: "CaptionReferences", ids: Sequence, device):
        lib = L.load()
        ref_off, tok_off, toks = [0], [0], []
        for iid in ids:
            for r in refs.tokens[iid]:
                toks += [refs.word_id[w] for w in r]
                tok_off.append(len(toks))
            ref_off.append(len(tok_off) - 1)
        self.I, self.nref, self.ntok = len(ids), len(tok_off) - 1, len(toks)
        self.index = {iid: i for i, iid in enumerate(ids)}
        i32 = dict(dtype=torch.int32, device=device)
        self.ref_off = torch.tensor(ref_off, **i32)
        self.tok_off = torch.tensor(tok_off, **i32)
        self.toks = torch.tensor(toks, **i32)
        self.style = None
        if refs.style_words is not None:
            flags = np.zeros(refs.W + 1, dtype=np.uint8)
            for w, c in refs.word_id.items():
                flags[c] = w in refs.style_words
            self.style = torch.from_numpy(flags).to(device)
        nbytes = lib.ssc_eval_refs_bytes(self.I, self.nref, self.ntok)
        if nbytes == 0:
            raise ValueError(f"reference set out of range: {self.I} images, {self.nref} captions, {self.ntok} tokens")
        self.state = torch.empty(nbytes, dtype=torch.uint8, device=device)
        self.desc = L.EvalRefs(self.I, self.nref, self.ntok, refs.W, L.ptr(self.ref_off), L.ptr(self.tok_off), L.ptr(self.toks),
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
                   set_diversity: bool = False):
        if pred.dim() != 3 or pred.dtype != torch.int64:
            raise ValueError(f"predictions must be (images, N, steps) int64, got {tuple(pred.shape)} {pred.dtype}")
        P, N, steps = pred.shape
        if len(image_ids) != P:
            raise ValueError(f"{len(image_ids)} image ids for {P} prediction images")
        if len(set(image_ids)) != P:
            raise ValueError("an image id occurs twice among the predictions")
        if N < 5:
            raise ValueError(f"top-5 Div-n needs at least 5 captions per image, got N = {N}")
        if N > MAX_SAMPLES:
            raise ValueError(f"N = {N} captions per image: at most {MAX_SAMPLES} are supported")
        if len(words) > MAX_WORDS:
            raise ValueError(f"{len(words)} prediction ids: at most {MAX_WORDS} are supported")
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
        scores = torch.empty(P, N, 6, dtype=torch.float64, device=dev)
        counts = torch.empty(P, N, 10, dtype=torch.int32, device=dev)
        img = torch.empty(P, 9, dtype=torch.int32, device=dev)
        top5 = torch.empty(P, 5, dtype=torch.int32, device=dev)
        d = L.EvalScoreDesc(L.ptr(pred), P, N, steps, int(boundary_index), len(words), L.ptr(id_map), L.ptr(style), L.ptr(ref_image),
                            L.ptr(scores), L.ptr(counts), L.ptr(img), L.ptr(top5))
        lib = L.load()
        ws = torch.empty(lib.ssc_eval_score_workspace_bytes(ctypes.byref(prep.desc), ctypes.byref(d)), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            lib.ssc_eval_score(ctypes.byref(prep.desc), ctypes.byref(d), L.ptr(ws), ws.numel(), L.stream_ptr())
        rows = [p for p, i in enumerate(image_ids) if i in self.tokens]
        imgc = img.cpu().numpy().astype(np.int64)
        set_out = _eval_set(pred, boundary_index, len(words), prep, id_map, ref_image) if set_diversity else None
        return EvalResult(list(image_ids), scores.cpu().numpy(), counts.cpu().numpy().astype(np.int64), imgc, rows,
                          top5.cpu().numpy().astype(np.int64), self.style_words is not None, set_out)

    def score(self, predictions: torch.Tensor, boundary_index: int, vocabulary, image_ids: Optional[Sequence] = None,
              set_diversity: bool = False) -> EvalResult:
        """predictions (images, N, steps) int64 on the device (diverse_decode's output); a row is cut at its first boundary_index.
        vocabulary: a Vocabulary (its @@UNKNOWN@@ matches nothing) or the list of words by id.  image_ids: one per prediction
        image (default: this object's images, in order); images without references count toward Div-1 / Div-2 only.
        set_diversity: also compare each image's N captions with each other (one ssc_eval_set call): mBLEU-1..4, Self-CIDEr and
        Unique in summary(); images without references count toward mBLEU and Unique only."""
        if not isinstance(set_diversity, bool):
            raise TypeError(f"set_diversity must be a bool, got {type(set_diversity).__name__}")
        if hasattr(vocabulary, "get_vocab_size"):
            words = [vocabulary.get_token_from_index(i) for i in range(vocabulary.get_vocab_size())]
        else:
            words = list(vocabulary)
        unk = words.index(UNKNOWN) if UNKNOWN in words else None
        ids = self.image_ids if image_ids is None else [_norm_id(i) for i in image_ids]
        return self._score_ids(predictions, boundary_index, words, ids, unk, set_diversity)

    def score_captions(self, predictions, set_diversity: bool = False) -> EvalResult:
        """Caption strings: [{"image_id", "caption"}, ...] (N per image in file order, as eval.py reads them) or
        {image_id: [captions]}.  Captions are split on whitespace; every word is itself, including words no vocabulary holds.
        set_diversity: as for score()."""
        if not isinstance(set_diversity, bool):
            raise TypeError(f"set_diversity must be a bool, got {type(set_diversity).__name__}")
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
        return self._score_ids(torch.from_numpy(arr).to(self.device), 0, words, list(groups), None, set_diversity)
