"""Prompted decoding (include/ssc.h: ssc_start_state, ssc_decode_prime, ssc_prefix_join): start the one-call decodes from a forced
prefix - "a happy ...", "two dogs ...", a per-image attribute word.

A DecodePrefix holds the prompt words of every image (or of every batch entry).  DecodeEngine.prime teacher-forces them on the
B = images x samples rows of a call and returns a StartState; every search and the sampled decode take it as start=... and return
the CONTINUATION; join_prefix puts prompt and continuation together.  inference.diverse_decode(prefix=...) does all three."""
from typing import NamedTuple, Optional, Sequence, Union

import torch

from . import lib as _lib
from .vocab import BOUNDARY

FEATURE = "a decode prefix (prefix= / start=)"
PAD = -1


def prefix_unsupported(what: str):
    """The error of everything a prefix is not combined with."""
    raise NotImplementedError(f"{FEATURE} is not implemented together with {what}")


class StartState(NamedTuple):
    """What DecodeEngine.prime returns and the decoders take as start=: h1, c1, hd, cd (B, H) - the states the first step of the
    continuation reads -, tokens (B) int64 - the word it is fed; an id outside [0, V) is fed as end_index -, lengths (B) int32 - the
    prefix words of every entry -, log_probs (B) - the prefix's summed log-prob -, token_lp (B, Lp) or None."""
    h1: torch.Tensor
    c1: torch.Tensor
    hd: torch.Tensor
    cd: torch.Tensor
    tokens: torch.Tensor
    lengths: torch.Tensor
    log_probs: torch.Tensor
    token_lp: Optional[torch.Tensor] = None

    def desc(self, device, B: int, H: int):
        """-> (ssc_start_state over contiguous device tensors, those tensors: keep them until the call is queued)."""
        st = [t.to(device, torch.float32).contiguous() for t in (self.h1, self.c1, self.hd, self.cd)]
        for t in st:
            if tuple(t.shape) != (B, H):
                raise ValueError(f"the start state is for {tuple(t.shape)} (entries, H); this call has {B} entries of H = {H}")
        tok = self.tokens.to(device, torch.int64).contiguous()
        if tuple(tok.shape) != (B,):
            raise ValueError(f"the start state holds {tuple(tok.shape)} tokens; this call has {B} entries")
        return _lib.StartState(*[_lib.ptr(t) for t in st], _lib.ptr(tok)), (st, tok)


class DecodePrefix:
    """ids (n, Lp) int64, one row per image (or per batch entry), the prompt's word ids padded with -1.  A row of -1 is an image
    without a prompt: it decodes as in an unprefixed call."""

    def __init__(self, ids: torch.Tensor):
        ids = torch.as_tensor(ids)
        if ids.dim() != 2 or ids.size(0) < 1 or ids.size(1) < 1 or ids.dtype.is_floating_point:
            raise ValueError(f"DecodePrefix: ids must be an integer (n, Lp) tensor with n, Lp >= 1, got {tuple(ids.shape)} {ids.dtype}")
        self.ids = ids.to(torch.int64)

    n = property(lambda self: self.ids.size(0))
    Lp = property(lambda self: self.ids.size(1))

    @staticmethod
    def from_words(vocabulary, words: Union[str, Sequence[Union[str, Sequence[str], None]]], n: Optional[int] = None,
                   vocab_size: Optional[int] = None) -> "DecodePrefix":
        """The prefix of a prompt.  words: a string - ONE prompt, its words separated by blanks, for all n images (n None: one
        row) -, or a list with one prompt PER IMAGE, each a string, a list of words, or None / "" for no prompt; prompts of
        different lengths share one prefix.  ValueError for a word the vocabulary does not hold, for @@BOUNDARY@@ and for an id >=
        vocab_size (the model's V; None: the vocabulary's size)."""
        V = int(vocab_size) if vocab_size is not None else vocabulary.get_vocab_size()
        known = vocabulary.get_token_to_index_vocabulary()

        def one(prompt):
            toks = prompt.split() if isinstance(prompt, str) else list(prompt or [])
            out = []
            for w in toks:
                if not isinstance(w, str):
                    raise ValueError(f"DecodePrefix: a prompt is a string or a list of words, got {w!r}")
                if w == BOUNDARY:
                    raise ValueError(f"DecodePrefix: {BOUNDARY} cannot be part of a prefix (it ends a caption)")
                if w not in known:
                    raise ValueError(f"DecodePrefix: the word {w!r} is not in the vocabulary")
                if known[w] >= V:
                    raise ValueError(f"DecodePrefix: the word {w!r} has id {known[w]}, outside the model's vocabulary of {V}")
                out.append(known[w])
            return out

        if isinstance(words, str):
            rows = [one(words)] * (n if n is not None else 1)
        else:
            rows = [one(w) for w in words]
            if n is not None and len(rows) != n:
                raise ValueError(f"DecodePrefix: {len(rows)} prompts for {n} images")
        Lp = max(1, max(len(r) for r in rows))
        ids = torch.full((len(rows), Lp), PAD, dtype=torch.int64)
        for i, r in enumerate(rows):
            if r:
                ids[i, :len(r)] = torch.tensor(r, dtype=torch.int64)
        return DecodePrefix(ids)

    @property
    def empty(self) -> bool:
        """No row holds a word."""
        return bool((self.ids[:, 0] < 0).all())

    def expand(self, n_samples: int) -> "DecodePrefix":
        """One row per batch entry (image, sample): every row repeated n_samples times in place."""
        if n_samples < 1:
            raise ValueError(f"DecodePrefix.expand: n_samples must be at least 1, got {n_samples}")
        return DecodePrefix(self.ids.repeat_interleave(n_samples, 0)) if n_samples > 1 else self


def join_prefix(prefix_ids: torch.Tensor, start: StartState, predictions: torch.Tensor, log_probs: torch.Tensor, end_index: int,
                ctl: Optional[torch.Tensor] = None):
    """Prompt + continuation (ssc_prefix_join).  prefix_ids (B, Lp) int64 as DecodeEngine.prime took them, start its result,
    predictions (B, ..., steps) / log_probs (B, ...) a decode's under that start state.
    -> (captions (B, ..., Lp + steps): the prompt's words, the continuation, then end_index; total (B, ...): prefix log-prob +
    continuation log-prob, a beam that does not exist (<= -1e19) kept as it is)."""
    lib = _lib.load()
    dev = predictions.device
    B, Lp = prefix_ids.shape
    steps = predictions.size(-1)
    if predictions.size(0) != B or tuple(predictions.shape[:-1]) != tuple(log_probs.shape):
        raise ValueError(f"join_prefix: predictions {tuple(predictions.shape)} / log_probs {tuple(log_probs.shape)} do not belong to "
                         f"a prefix of {B} entries")
    Q = log_probs.numel() // B
    pre = prefix_ids.to(dev, torch.int64).contiguous()
    pred = predictions.to(torch.int64).contiguous()
    lps = log_probs.to(torch.float32).contiguous()
    lens = start.lengths.to(dev, torch.int32).contiguous()
    plp = start.log_probs.to(dev, torch.float32).contiguous()
    caps = torch.empty(*log_probs.shape, Lp + steps, dtype=torch.int64, device=dev)
    total = torch.empty_like(lps)
    lib.ssc_prefix_join(_lib.ptr(pre), _lib.ptr(lens), Lp, _lib.ptr(pred), _lib.ptr(ctl), steps, _lib.ptr(lps), _lib.ptr(plp), B, Q,
                        end_index, _lib.ptr(caps), _lib.ptr(total), _lib.stream_ptr())
    return caps, total
